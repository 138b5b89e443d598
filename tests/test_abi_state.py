"""Call-sequence parity of the engine's host state machine (rifraf_hip.hip's
arenas, plan caches, validation skip and per-band metadata).

A seeded generator (`Gen`) builds a random sequence of C-ABI calls over 12
sequence ids, 4 template ids and 16 slots.  Its shadow model is plain Python:
per sequence / template id the current content and an upload count, per band
either nothing or the alignment it was filled for (sequence and template
content and upload counts, bandwidth, skew / trim, the row stride by the
engine's rule: the call's padding, or the partner band's stride when that
band holds the same alignment).  Every read-back op carries the shadow's
verdict: legal, with the band records the oracle's value follows from, or
refused (no band; A and B of different alignments or strides; the template or
the sequence uploaded again since the fill), in which case the call must
raise RifrafError and the engine must go on as if it had not been made.

A forward band filled with RF_SKEW / RF_TRIM beside a plain backward band is
neither: the header does not refuse it and the reference never scores such a
pair, so the generator backtraces and downloads such slots but never scores
them.

Shapes: each template id has a base length in 27..113; its templates are
within +-7 and its reads within +-8 of it (|n - m| <= 15), bandwidth 2..12,
or 32..40 for the calls whose widest band has H >= 64 (RF_OPT_BAND_PAD's
padded strides).

The GPU test replays the ops on the session engine against the oracle; the
CPU test runs the generator alone and checks that the state transitions the
engine can get wrong all occur, each followed by a read-back of an affected
slot.  A failure names the seed, the op index and the last ten ops.
"""
import numpy as np
import pytest

import oracle
from _util import SEQ_SCORES, all_proposals_arrays, dense_slot, inband_mask, random_seq
from rifraf_amd import RifrafSequence
from rifraf_amd.align import moves_to_proposals_np
from rifraf_amd.bandedarrays import band_stride
from rifraf_amd.engine import RF_BAND_A, RF_BAND_B, RF_BWD, RF_FWD, RF_SKEW, RF_TRIM, Engine, RifrafError
from rifraf_amd.errormodel import phred_to_log_p
from rifraf_amd.model import _add_base_distributions

SEEDS = (7101, 7102, 7103)
NOPS = 250
SEQ_IDS, TPL_IDS, SLOTS = 12, 4, 16
PER_TPL = SEQ_IDS // TPL_IDS
# options documented to select between bit-identical paths (rifraf_hip.h)
FLIPS = {"score_mode": (0, 1, 2), "score_kernel": (0, 1, 2, 3), "band_pad": (64, 1, 0), "dp_lat": (0, 2048),
         "bt_nw": (4, 1)}
DEFAULTS = {"score_mode": 0, "score_kernel": 0, "band_pad": 64, "dp_lat": 0, "bt_nw": 4}
LP_TABLE = phred_to_log_p(np.arange(256, dtype=np.uint8).view(np.int8))
with np.errstate(divide="ignore", invalid="ignore"):
    MATCH_TABLE = np.log10(1.0 - np.power(10.0, LP_TABLE))

TRANSITIONS = ("tpl_same_len", "tpl_other_len", "seq_same_len", "seq_shorter", "seq_longer", "pad_differs",
               "realign_repeat", "dense_repeat", "release_refill", "option_flip", "refused_then_legal")


class SeqC:
    """One sequence content: bases and Phred scores."""

    def __init__(self, uid, bases, phred):
        self.uid, self.bases, self.phred = uid, np.ascontiguousarray(bases, np.uint8), np.ascontiguousarray(phred, np.int8)
        self.n = len(self.bases)
        self._rs = {}

    def rs(self, bw=9):
        if bw not in self._rs:
            self._rs[bw] = RifrafSequence(self.bases, self.phred, bw, SEQ_SCORES)
        return self._rs[bw]


class Fill:
    """What one band was filled for."""
    __slots__ = ("seq", "seqc", "seqver", "tpl", "tplc", "tplver", "bw", "skew", "trim", "P", "pad", "at")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)

    @property
    def n(self):
        return self.seqc.n

    @property
    def m(self):
        return len(self.tplc)

    def key(self, fwd):
        return (self.seqc.uid, self.tplc.tobytes(), self.bw, fwd and self.skew, fwd and self.trim)


class Op:
    """One engine call (or an identical call made `repeat` times in a row)."""

    def __init__(self, kind, **kw):
        self.kind = kind
        self.reads, self.mutates, self.events = set(), set(), []
        self.legal = None      # read-backs: True / False
        self.__dict__.update(kw)

    def __repr__(self):
        skip = ("kind", "reads", "mutates", "events", "fills", "contents", "groups_fills")
        arg = ", ".join(f"{k}={v!r}" for k, v in self.__dict__.items() if k not in skip)
        return f"{self.kind}({arg})" + ("" if self.legal is None else " legal" if self.legal else " refused")


READBACKS = ("download", "backtrace", "aln_props", "dense", "score", "aln_sums")
SCORING = ("dense", "score")


class Gen:
    """Seeded op generator with its shadow model."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        rng = self.rng
        self.uid = 0
        self.base = [int(x) for x in rng.permutation([27, 46, 84, 113])]
        self.anc = [random_seq(b + 8, rng) for b in self.base]
        self.seqs, self.seqver = [None] * SEQ_IDS, [0] * SEQ_IDS
        self.tpls, self.tplver = [None] * TPL_IDS, [0] * TPL_IDS
        self.tplcount = 0
        self.bands = [[None, None] for _ in range(SLOTS)]
        self.opt = dict(DEFAULTS)
        self.queue = []
        self.released = False
        self.nops = 0
        self.inf_reads = 0
        self.flipped = {}
        self.emitted = dict.fromkeys(("same", "shorter", "longer", "tsame", "tother", "release", "drep", "pad", "option", "reserve"), 0)

    def least(self, forms):
        """The form emitted least often so far (ties: the first)."""
        return min(forms, key=lambda f: self.emitted[f])

    def users(self, what, i):
        """Slots holding a current band filled from sequence / template id i."""
        return {s for s in range(SLOTS) for f in self.bands[s]
                if f is not None and (f.seq if what == "seq" else f.tpl) == i and self.current(f)}

    # -- contents -------------------------------------------------------
    def new_seq(self, t, n=None, inf=False):
        rng, b = self.rng, self.base[t]
        n = int(rng.integers(b - 8, b + 9)) if n is None else n
        bases = self.anc[t][:n].copy()
        hit = rng.random(n) < 0.06
        bases[hit] = rng.integers(0, 4, int(hit.sum()))
        phred = rng.integers(5, 41, n).astype(np.int8)
        if inf:
            phred[int(rng.integers(0, n))] = 0      # log p = 0: match = -Inf (not lean eligible)
            self.inf_reads += 1
        self.uid += 1
        return SeqC(self.uid, bases, phred)

    def new_tpl(self, t, m=None, like=None):
        rng, b = self.rng, self.base[t]
        m = int(rng.integers(b - 7, b + 8)) if m is None else m
        while True:
            tpl = self.anc[t][:m].copy()
            hit = rng.random(m) < 0.04
            hit[int(rng.integers(0, m))] = True
            tpl[hit] = (tpl[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
            if like is None or not np.array_equal(tpl, like):
                return tpl

    # -- the shadow's verdicts -----------------------------------------
    def current(self, f):
        return f is not None and self.tplver[f.tpl] == f.tplver and self.seqver[f.seq] == f.seqver

    def state(self, slot, kind, which=0):
        """'legal', 'refused' or 'open' (not refused by the header, no
        reference value: never read back this way)."""
        a, b = self.bands[slot]
        if kind == "download":
            return "legal" if self.bands[slot][which] is not None else "refused"
        if kind in ("backtrace", "aln_props", "aln_sums"):
            return "legal" if self.current(a) else "refused"
        if a is None or b is None:
            return "refused"
        if (a.seq, a.tpl, a.bw, a.tplver, a.seqver, a.n, a.m) != (b.seq, b.tpl, b.bw, b.tplver, b.seqver, b.n, b.m):
            return "refused"
        if a.P != b.P or not self.current(a):
            return "refused"
        return "open" if (a.skew or a.trim) else "legal"

    def live_slots(self):
        return [s for s in range(SLOTS) if any(f is not None for f in self.bands[s])]

    # -- mutating ops ---------------------------------------------------
    def op_set_sequences(self, first=None, count=None):
        rng = self.rng
        if first is None:
            count = int(rng.integers(1, 4))
            first = int(rng.integers(0, SEQ_IDS - count + 1))
            used = [i for i in range(SEQ_IDS) if self.users("seq", i)]
            if used and rng.random() < 0.85:     # a range that holds an id with live bands
                first = min(max(int(rng.choice(used)) - int(rng.integers(0, count)), 0), SEQ_IDS - count)
        contents, events = [], []
        for i in range(first, first + count):
            t, old = i // PER_TPL, self.seqs[i]
            users = self.users("seq", i)
            lo, hi = self.base[t] - 8, self.base[t] + 8
            if old is None:
                c = self.new_seq(t, inf=(i % 5 == 2))
            else:
                form = "identical" if rng.random() < 0.1 else self.least(["same", "shorter", "longer"]) if users \
                    else str(rng.choice(["same", "shorter", "longer"]))
                if form == "shorter" and old.n == lo:
                    form = "longer"
                if form == "longer" and old.n == hi:
                    form = "shorter"
                if form == "identical":
                    c = old
                else:
                    n = old.n if form == "same" else int(rng.integers(lo, old.n)) if form == "shorter" \
                        else int(rng.integers(old.n + 1, hi + 1))
                    c = self.new_seq(t, n, inf=rng.random() < 0.08)
                if users:
                    if c is not old:
                        self.emitted["same" if c.n == old.n else "shorter" if c.n < old.n else "longer"] += 1
                    events.append(("seq_identical" if c is old else "seq_same_len" if c.n == old.n else
                                   "seq_shorter" if c.n < old.n else "seq_longer", users))
            contents.append(c)
            self.seqs[i] = c
            self.seqver[i] += 1
        op = Op("set_sequences", first=first, path=str(rng.choice(["tables", "codes"])), contents=contents,
                lens=[c.n for c in contents])
        op.events = events
        return op

    def op_set_templates(self, ids=None):
        rng = self.rng
        sparse = ids is None and rng.random() < 0.5
        if ids is None:
            k = int(rng.integers(1, 3))
            if sparse:
                ids = [int(x) for x in rng.permutation(TPL_IDS)[:k]]
            else:
                first = int(rng.integers(0, TPL_IDS - k + 1))
                ids = list(range(first, first + k))
            used = [t for t in range(TPL_IDS) if self.users("tpl", t)]
            if used and not set(used) & set(ids):
                ids[0] = int(rng.choice(used))
                if not sparse:
                    ids = ids[:1]
        contents, events = [], []
        for t in ids:
            old = self.tpls[t]
            users = self.users("tpl", t)
            if old is None:
                c = self.new_tpl(t)
            else:
                form = "identical" if rng.random() < 0.15 else \
                    {"tsame": "same", "tother": "other"}[self.least(["tsame", "tother"])] if users \
                    else str(rng.choice(["same", "other"]))
                if users and form != "identical":
                    self.emitted["t" + form] += 1
                if form == "identical":
                    c = old.copy()
                elif form == "same":
                    c = self.new_tpl(t, len(old), like=old)
                else:
                    m = len(old)
                    while m == len(old):
                        m = int(rng.integers(self.base[t] - 7, self.base[t] + 8))
                    c = self.new_tpl(t, m)
                if users:
                    events.append(("tpl_identical" if form == "identical" else "tpl_same_len" if form == "same"
                                   else "tpl_other_len", users))
            contents.append(c)
            self.tpls[t] = c
            self.tplcount += 1
            self.tplver[t] = self.tplcount
        op = Op("set_templates", ids=ids, sparse=sparse, contents=contents, lens=[len(c) for c in contents])
        op.events = events
        return op

    def pick_alignment(self, slot, wide=False, keep=0.6):
        rng = self.rng
        old = self.bands[slot][0] or self.bands[slot][1]
        if old is not None and not wide and rng.random() < keep:
            return old.seq, old.tpl, old.bw
        t = int(rng.integers(0, TPL_IDS))
        seq = t * PER_TPL + int(rng.integers(0, PER_TPL))
        bw = int(rng.integers(32, 41)) if wide else int(rng.integers(2, 13))
        return seq, t, bw

    def op_realign(self, jobs=None, flags=None, repeat=None):
        """jobs: [(slot, seq, tpl, bw)]; flags: one int or one per job."""
        rng = self.rng
        if jobs is None:
            k = int(rng.integers(1, 9))
            slots = [int(s) for s in rng.permutation(SLOTS)[:k]]
            wide = rng.random() < 0.25
            jobs = [(s,) + self.pick_alignment(s, wide and j == 0) for j, s in enumerate(slots)]
        if flags is None:
            r = rng.random()
            if r < 0.5:
                flags = RF_FWD | RF_BWD
            elif r < 0.75:
                flags = int(rng.choice([RF_FWD, RF_BWD, RF_FWD | RF_SKEW, RF_FWD | RF_BWD | RF_TRIM]))
            else:
                flags = [int(x) for x in rng.choice([RF_FWD | RF_SKEW, RF_FWD | RF_TRIM, RF_FWD | RF_SKEW | RF_TRIM,
                                                     RF_BWD, RF_BWD, RF_FWD | RF_BWD, RF_FWD], len(jobs))]
        if repeat is None:
            repeat = int(rng.choice([1, 1, 1, 1, 1, 1, 2, 3]))
        jf = flags if isinstance(flags, list) else [flags] * len(jobs)
        H = [2 * bw + abs(self.seqs[q].n - len(self.tpls[t])) + 1 for _, q, t, bw in jobs]
        pad = self.opt["band_pad"] > 0 and max(H) >= self.opt["band_pad"]
        events, fills = [], [None] * len(jobs)
        differs = set()
        for d in (0, 1):
            for j, (s, q, t, bw) in enumerate(jobs):
                if not jf[j] & (RF_BWD if d else RF_FWD):
                    continue
                S, T, o = self.seqs[q], self.tpls[t], self.bands[s][1 - d]
                partner = (o is not None and (o.seq, o.tpl, o.bw, o.n, o.m, o.tplver, o.seqver) ==
                           (q, t, bw, S.n, len(T), self.tplver[t], self.seqver[q]))
                P = o.P if partner else band_stride(H[j], 1 if pad else 0)
                if partner and o.pad != pad:
                    differs.add(s)
                f = Fill(seq=q, seqc=S, seqver=self.seqver[q], tpl=t, tplc=T, tplver=self.tplver[t], bw=bw,
                         skew=bool(d == 0 and jf[j] & RF_SKEW), trim=bool(d == 0 and jf[j] & RF_TRIM), P=P, pad=pad,
                         at=self.nops)
                self.bands[s][d] = f
                if d == 0 or not jf[j] & RF_FWD:
                    fills[j] = f          # out_score: the forward score wins
        slots = {j[0] for j in jobs}
        if differs:
            events.append(("pad_differs", differs))
            self.emitted["pad"] += 1
        if repeat > 1:
            events.append(("realign_repeat", set(slots)))
        if self.released:
            events.append(("release_refill", set(slots)))
            self.released = False
        op = Op("realign", jobs=jobs, flags=flags, repeat=repeat, fills=fills, pad=pad)
        op.mutates, op.events = slots, events
        return op

    def op_release(self):
        self.bands = [[None, None] for _ in range(SLOTS)]
        self.released = True
        op = Op("release_bands")
        op.mutates = set(range(SLOTS))
        self.emitted["release"] += 1
        if self.rng.random() < 0.8:
            self.queue.append(lambda: self.op_readback(
                kind=str(self.rng.choice(["download", "download", "dense", "backtrace"]))))
        if self.rng.random() < 0.85:
            self.queue.append(lambda: self.op_realign(flags=RF_FWD | RF_BWD if self.rng.random() < 0.7 else None))
        return op

    def op_reserve(self):
        self.emitted["reserve"] += 1
        return Op("reserve", nbytes=int(self.rng.choice([1024, 1 << 21, 6 << 20, 16 << 20, 40 << 20])))

    def op_option(self):
        name = min(self.rng.permutation(list(FLIPS)), key=lambda k: self.flipped.get(k, 0))   # the rarest so far
        name = str(name)
        self.flipped[name] = self.flipped.get(name, 0) + 1
        value = int(self.rng.choice([v for v in FLIPS[name] if v != self.opt[name]]))
        self.opt[name] = value
        self.emitted["option"] += 1
        op = Op("set_option", name=name, value=value)
        live = set(self.live_slots())
        if live:
            op.events = [("option_flip", live)]
        return op

    # -- read-backs -----------------------------------------------------
    def group_of(self, slot, kind, size):
        """Legal slots of `slot`'s template (it first), up to `size`."""
        t = self.bands[slot][0].tpl
        others = [s for s in range(SLOTS) if s != slot and self.state(s, kind) == "legal" and
                  self.bands[s][0].tpl == t]
        self.rng.shuffle(others)
        return [slot] + [int(s) for s in others[:size - 1]]

    def op_readback(self, prefer=None, kind=None, repeat=None):
        rng = self.rng
        if kind is None:
            kind = str(rng.choice(READBACKS, p=[0.2, 0.17, 0.12, 0.22, 0.17, 0.12]))
        which = int(rng.integers(0, 2))
        cand = list(range(SLOTS)) if not prefer else sorted(prefer)
        cand = [s for s in cand if self.state(s, kind, which) != "open"]
        if not cand:
            kind, cand = "backtrace", (sorted(prefer) if prefer else list(range(SLOTS)))
        legal = [s for s in cand if self.state(s, kind, which) == "legal"]
        if prefer:
            slot = int(rng.choice(cand))
        elif legal and rng.random() < 0.9:
            slot = int(rng.choice(legal))
        else:
            slot = int(rng.choice(cand))
        ok = self.state(slot, kind, which) == "legal"
        op = Op(kind, legal=ok)
        if kind == "download":
            op.slot, op.which, op.fills = slot, which, [self.bands[slot][which]]
            op.reads = {slot}
            return op
        if kind == "backtrace":
            extra = [s for s in range(SLOTS) if s != slot and self.state(s, kind) == "legal"] if ok else []
            rng.shuffle(extra)
            op.slots = [slot] + [int(s) for s in extra[:int(rng.integers(0, 5))]]
            rng.shuffle(op.slots)
            op.fills = [self.bands[s][0] for s in op.slots]
            op.reads = set(op.slots)
            return op
        groups = [self.group_of(slot, kind, int(rng.integers(1, 6)))] if ok else [[slot]]
        if ok:
            for _ in range(int(rng.integers(0, 3 if kind in ("dense", "aln_props") else 2))):
                used = {s for g in groups for s in g}
                tp = {self.bands[g[0]][0].tpl for g in groups}
                more = [s for s in range(SLOTS) if s not in used and self.state(s, kind) == "legal" and
                        self.bands[s][0].tpl not in tp]
                if more:
                    groups.append(self.group_of(int(rng.choice(more)), kind, int(rng.integers(1, 5))))
        op.groups = groups
        op.groups_fills = [[self.bands[s][0] for s in g] for g in groups]
        op.reads = {s for g in groups for s in g}
        if kind == "aln_props":
            op.do_indels = bool(rng.integers(0, 2))
        if kind == "dense":
            op.repeat = (repeat or int(rng.choice([1, 1, 1, 1, 2, 3]))) if ok else 1
            if op.repeat > 1:
                self.emitted["drep"] += 1
                op.events = [("dense_repeat", set(op.reads))]
        if kind == "score":
            op.pick = int(rng.integers(0, 1 << 30))     # seeds the proposal subset
        return op

    # -- the schedule ---------------------------------------------------
    def follow_up(self, op):
        """After a transition: read an affected slot back next (usually),
        then sometimes refill it and read it back again."""
        rng = self.rng
        affected = set().union(*[sl for _, sl in op.events]) if op.events else set()
        if op.kind in READBACKS or not affected or (op.kind in ("realign", "set_option") and rng.random() > 0.8):
            return
        kind = None
        if any(name == "pad_differs" for name, _ in op.events):
            affected = set().union(*[sl for name, sl in op.events if name == "pad_differs"])
            kind = str(rng.choice(SCORING))
        if op.kind in ("set_sequences", "set_templates"):
            for _, sl in op.events[:-1]:         # every id's bands, not just one of the upload's
                self.queue.append(lambda sl=sl: self.op_readback(prefer=sl))
            affected = op.events[-1][1]
        self.queue.append(lambda sl=affected: self.op_readback(prefer=sl, kind=kind))
        affected = set().union(*[sl for _, sl in op.events])
        stale = [s for s in affected if self.state(s, "backtrace") == "refused"]
        if stale and rng.random() < 0.85:
            def refill():
                jobs = []
                for s in stale[:6]:
                    old = self.bands[s][0] or self.bands[s][1]
                    jobs.append((s, old.seq, old.tpl, old.bw) if old is not None else (s,) + self.pick_alignment(s))
                return self.op_realign(jobs=jobs, flags=RF_FWD | RF_BWD)
            self.queue.append(refill)
            for _ in range(2 + (rng.random() < 0.5)):
                self.queue.append(lambda: self.op_readback(prefer=set(stale[:6])))

    def lacking(self):
        """An op for a transition emitted fewer than 6 times so far, or None."""
        rng, e = self.rng, self.emitted
        want = []
        if min(e["same"], e["shorter"], e["longer"]) < 6 and any(self.users("seq", i) for i in range(SEQ_IDS)):
            want.append(self.op_set_sequences)
        if min(e["tsame"], e["tother"]) < 6 and any(self.users("tpl", t) for t in range(TPL_IDS)):
            want.append(self.op_set_templates)
        if e["release"] < 6 and len(self.live_slots()) >= 4:
            want.append(self.op_release)
        if e["pad"] < 6:
            want.append(self.split_directions)
        if e["drep"] < 6 and any(self.state(s, "dense") == "legal" for s in range(SLOTS)):
            want.append(lambda: self.op_readback(kind="dense", repeat=int(rng.integers(2, 4))))
        if e["option"] < 6 and self.live_slots():
            want.append(self.op_option)
        if e["reserve"] < 3:
            want.append(self.op_reserve)
        return want[int(rng.integers(0, len(want)))]() if want else None

    def split_directions(self):
        """Forward fills in a call that pads (one wide job beside them), the
        backward fills of the same alignments in one that does not, or the
        other way round: the partner-stride rule."""
        rng = self.rng
        if self.opt["band_pad"] != 64:           # all or no calls pad: back to the default first
            self.queue.append(self.split_directions)
            self.opt["band_pad"] = 64
            op = Op("set_option", name="band_pad", value=64)
            op.events = [("option_flip", set(self.live_slots()))] if self.live_slots() else []
            return op
        slots = [int(s) for s in rng.permutation(SLOTS)[:int(rng.integers(3, 7))]]
        jobs = [(s,) + self.pick_alignment(s, keep=0.0) for s in slots[1:]]
        widejob = (slots[0],) + self.pick_alignment(slots[0], wide=True)
        first, second = (RF_FWD, RF_BWD) if rng.random() < 0.5 else (RF_BWD, RF_FWD)
        wide_first = bool(rng.random() < 0.6)
        a = self.op_realign(jobs=jobs + [widejob] if wide_first else jobs, flags=first, repeat=1)
        self.queue.append(lambda: self.op_realign(jobs=jobs if wide_first else jobs + [widejob], flags=second, repeat=1))
        return a

    def next(self):
        rng = self.rng
        if self.nops == 0:
            op = self.op_set_sequences(0, SEQ_IDS)
        elif self.nops == 1:
            op = self.op_set_templates(list(range(TPL_IDS)))
        elif self.queue:
            op = self.queue.pop(0)()
        else:
            op = self.lacking() if rng.random() < 0.8 else None
            r = rng.random() if op is None else 2.0
            if op is not None:
                pass
            elif r < 0.20:
                op = self.op_realign()
            elif r < 0.27:
                op = self.split_directions()
            elif r < 0.72:
                op = self.op_readback()
            elif r < 0.78:
                op = self.op_set_sequences()
            elif r < 0.83:
                op = self.op_set_templates()
            elif r < 0.86:
                op = self.op_release()
            elif r < 0.90:
                op = self.op_reserve()
            else:
                op = self.op_option()
        op.index = self.nops
        self.nops += 1
        self.follow_up(op)
        return op


def generate(seed, nops=NOPS):
    g = Gen(seed)
    ops = [g.next() for _ in range(nops)]
    return ops, g


def coverage(ops):
    """Transitions that were followed by a read-back of an affected slot
    before that slot's next mutation; and the legal share of the read-backs."""
    counts = dict.fromkeys(TRANSITIONS, 0)
    pending = []                   # [name, slots still unmutated, fill-seen (option_flip)]
    refused = set()                # slots whose last read-back was refused
    nread = nlegal = 0
    for op in ops:
        if op.kind in READBACKS:
            nread += 1
            nlegal += bool(op.legal)
            for p in pending:
                if p[1] & op.reads:
                    counts[p[0]] += 1
                    p[1] = set()
            for s in op.reads:
                if not op.legal:
                    refused.add(s)
                elif s in refused:
                    refused.discard(s)
                    counts["refused_then_legal"] += 1
        for p in pending:
            p[1] = p[1] - op.mutates
        pending = [p for p in pending if p[1]]
        for name, slots in op.events:
            if name in counts:
                if name == "dense_repeat":      # the repeated call is the read-back
                    counts[name] += 1
                else:
                    pending.append([name, set(slots)])
    return counts, nread, nlegal


@pytest.mark.parametrize("seed", SEEDS)
def test_generator_reaches_every_transition(seed):
    """The op sequence of each seed holds every state transition at least 5
    times, each followed by a read-back of an affected slot before that slot
    is filled or released again, and at least 70 % of its read-backs are
    legal; it uploads through both paths and holds reads with a -Inf match
    score, padded and unpadded calls, per-job flags and every option."""
    ops, g = generate(seed)
    counts, nread, nlegal = coverage(ops)
    print(seed, counts, f"{nlegal}/{nread} read-backs legal")
    for name in TRANSITIONS:
        assert counts[name] >= 5, (seed, name, counts)
    assert nlegal >= 0.7 * nread, (seed, nlegal, nread)
    assert nread >= 80
    kinds = {op.kind for op in ops}
    assert kinds >= set(READBACKS) | {"realign", "set_sequences", "set_templates", "release_bands", "reserve",
                                      "set_option"}
    assert {op.path for op in ops if op.kind == "set_sequences"} == {"tables", "codes"}
    assert {op.sparse for op in ops if op.kind == "set_templates"} == {True, False}
    assert {op.pad for op in ops if op.kind == "realign"} == {True, False}
    assert any(isinstance(op.flags, list) for op in ops if op.kind == "realign")
    assert {op.name for op in ops if op.kind == "set_option"} == set(FLIPS)
    assert g.inf_reads >= 1
    for kind in READBACKS:
        assert any(op.kind == kind and op.legal for op in ops), kind
        assert any(op.kind == kind and not op.legal for op in ops), kind


# ---------------------------------------------------------------------
# the oracle's side of a read-back
# ---------------------------------------------------------------------
_FWD, _BWD, _WALK = {}, {}, {}


def fwd(f):
    k = f.key(True)
    if k not in _FWD:
        _FWD[k] = oracle.forward(f.tplc, f.seqc.rs(f.bw), moves=True, skew=f.skew, trim=f.trim)
    return _FWD[k]


def bwd(f):
    k = f.key(False)
    if k not in _BWD:
        _BWD[k] = oracle.backward(f.tplc, f.seqc.rs(f.bw))
    return _BWD[k]


def walk(f):
    k = f.key(True)
    if k not in _WALK:
        mv = oracle.backtrace(fwd(f)[1], f.n + 1, f.m + 1, f.bw)
        _WALK[k] = (mv, oracle.count_errors(mv, f.tplc, f.seqc.bases))
    return _WALK[k]


def same(got, exp):
    got, exp = np.asarray(got), np.asarray(exp)
    return (got == exp) | (np.isnan(got) & np.isnan(exp))


def dense_mask(t):
    mask = np.ones((len(t) + 1, 9), bool)
    mask[0, :5] = False
    mask[np.arange(1, len(t) + 1), np.asarray(t, np.int64)] = False
    return mask


_DENSE = {}


def expected_dense(fills):
    k = tuple(f.key(False) for f in fills)
    if k not in _DENSE:
        _DENSE[k] = oracle.cpu_pass(fills[0].tplc, [f.seqc.rs(f.bw) for f in fills], nthreads=1)[0]
    return _DENSE[k]


def expected_sums(fills):
    probs = np.zeros((fills[0].m, 4))
    _add_base_distributions(probs, [walk(f)[0] for f in fills], [f.seqc.rs(f.bw) for f in fills])
    return probs


def run_op(e, op):
    """Make the call; returns what a refused read-back must leave untouched."""
    k = op.kind
    if k == "set_sequences":
        if op.path == "tables":
            e.set_sequences(op.first, [c.rs() for c in op.contents])
        else:
            off = np.zeros(len(op.contents) + 1, np.int64)
            np.cumsum([c.n for c in op.contents], out=off[1:])
            assert e.set_sequences_codes(op.first, np.concatenate([c.bases for c in op.contents]), off,
                                         np.concatenate([c.phred for c in op.contents]).view(np.uint8), LP_TABLE,
                                         MATCH_TABLE, SEQ_SCORES)
    elif k == "set_templates":
        if op.sparse:
            e.set_templates_ids(op.ids, op.contents)
        else:
            e.set_templates(op.ids[0], op.contents)
    elif k == "realign":
        sl, sq, tp, bw = (np.array(x, np.int32) for x in zip(*op.jobs))
        for _ in range(op.repeat):
            got = e.realign(sl, sq, tp, bw, op.flags if not isinstance(op.flags, list) else np.array(op.flags, np.int32))
            jf = op.flags if isinstance(op.flags, list) else [op.flags] * len(op.jobs)
            for j, f in enumerate(op.fills):
                h = max(f.m - f.n, 0) + f.bw
                exp = fwd(f)[0][f.n - f.m + h, f.m] if jf[j] & RF_FWD else bwd(f)[h, 0]
                assert got[j] == exp, f"job {j}: score {got[j]!r} != {exp!r}"
    elif k == "release_bands":
        e.release_bands()
    elif k == "reserve":
        e.reserve(op.nbytes)
    elif k == "set_option":
        e.set_option(op.name, op.value)
    elif not op.legal:
        with pytest.raises(RifrafError):
            read_back(e, op)
    else:
        read_back(e, op)


def read_back(e, op):
    k = op.kind
    if k == "download":
        f = op.fills[0]
        got = e.download_band(op.slot, RF_BAND_B if op.which else RF_BAND_A)
        exp = bwd(f) if op.which else fwd(f)[0]
        mask = inband_mask(f.n + 1, f.m + 1, f.bw)
        assert got.data.shape == exp.shape
        assert same(got.data[mask], exp[mask]).all(), "band cells"
    elif k == "backtrace":
        moves, nerr = e.backtrace(op.slots)
        for j, f in enumerate(op.fills):
            np.testing.assert_array_equal(moves[j], walk(f)[0], err_msg=f"moves of slot {op.slots[j]}")
            assert nerr[j] == walk(f)[1], f"n_errors of slot {op.slots[j]}"
    elif k == "aln_props":
        got = e.alignment_proposals(op.groups, op.do_indels)
        for g, fills in enumerate(op.groups_fills):
            exp = np.zeros((fills[0].m + 1, 9), np.uint8)
            for f in fills:
                kd, p, b = moves_to_proposals_np(walk(f)[0], f.tplc, f.seqc.bases)
                if not op.do_indels:
                    keep = kd == 0
                    kd, p, b = kd[keep], p[keep], b[keep]
                exp[p, dense_slot(kd, b)] = 1
            np.testing.assert_array_equal(got[g], exp, err_msg=f"mask of group {g}")
    elif k == "dense":
        groups = [np.array(g, np.int32) for g in op.groups]
        first = None
        for _ in range(op.repeat):
            got = [d.copy() for d in e.score_dense(groups)]
            for g, fills in enumerate(op.groups_fills):
                mask = dense_mask(fills[0].tplc)
                assert same(got[g][mask], expected_dense(fills)[mask]).all(), f"dense totals of group {g}"
                if first is not None:
                    assert same(got[g], first[g]).all(), "a repeated rf_score_dense changed its totals"
            first = got
    elif k == "score":
        rng = np.random.default_rng(op.pick)
        calls = []
        for g, fills in zip(op.groups, op.groups_fills):
            kd, p, b = all_proposals_arrays(fills[0].tplc if fills[0] is not None else np.zeros(5, np.uint8))
            take = np.sort(rng.permutation(len(kd))[:int(rng.integers(1, 40))])
            calls.append((g, -1, (kd[take], p[take], b[take])))
        tot, per = e.score(calls, per_seq=True)
        for g, fills in enumerate(op.groups_fills):
            kd, p, b = calls[g][2]
            at = (p, dense_slot(kd, b))
            assert same(tot[g], expected_dense(fills)[at]).all(), f"totals of group {g}"
            for r, f in enumerate(fills):            # 0.0 + s_r of the read alone
                assert same(per[g][:, r], expected_dense([f])[at]).all(), f"per-read scores of group {g}, read {r}"
    elif k == "aln_sums":
        seqs = [[f.seqc.rs() if f is not None else SeqC(0, [0], [20]).rs() for f in fills] for fills in op.groups_fills]
        tlens = [fills[0].m if fills[0] is not None else 1 for fills in op.groups_fills]
        got = e.aln_error_sums(op.groups, tlens, seqs)
        for g, fills in enumerate(op.groups_fills):
            assert same(got[g], expected_sums(fills)).all(), f"alignment sums of group {g}"


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_call_sequence_matches_shadow_model(engine, opts, seed):
    """Replay one seed's ops on the session engine: every read-back the
    shadow model calls legal equals the oracle bit for bit, every other one
    raises RifrafError, and the engine goes on."""
    for name, value in DEFAULTS.items():
        opts(name, value)                    # restored by the fixture afterwards
    ops, _ = generate(seed)
    for i, op in enumerate(ops):
        try:
            run_op(engine, op)
        except BaseException as err:         # noqa: BLE001 -- re-raised with the trace
            trace = "\n".join(f"  {o.index:3d} {o!r}" for o in ops[max(0, i - 9):i + 1])
            raise AssertionError(f"seed {seed}, op {i} ({op.kind}): {type(err).__name__}: {err}\n"
                                 f"last ops:\n{trace}") from err


# ---------------------------------------------------------------------
# arena growth under live bands
# ---------------------------------------------------------------------
def _read_cluster(e, sl, pg, props):
    """The read-backs of one cluster, always with the same argument lists."""
    dense = e.score_dense(pg)[0].copy()
    moves, nerr = e.backtrace(sl)
    band = e.download_band(int(sl[2]), RF_BAND_B).data.copy()
    tot = e.score([(sl, -1, props)])[0]
    return dense, moves, nerr, band, tot


@pytest.mark.gpu
@pytest.mark.parametrize("x_first", [True, False])
def test_arena_growth_under_live_bands(x_first):
    """Cluster X (8 reads, m = 100, A and B bands) is filled and read back;
    then, without a call that touches X's slots, the band arena grows twice
    (cluster Y, 40 reads at m = 600) and the table and byte arenas grow
    (more sequences at new ids): after each compaction X's dense totals, proposal
    scores, backtraces and a downloaded band are the bits they were, through
    the same argument lists (the cached plans), and the oracle's.  With
    x_first False, part of Y is filled first, so that X's bands sit at
    offsets behind Y's first bands (filled from the start of a released
    arena) and move from there."""
    from bench import band_bytes
    from rifraf_amd.engine import pack_groups
    rng = np.random.default_rng(5150 + x_first)
    tx, ty = random_seq(100, rng), random_seq(600, rng)
    from _util import make_read
    xs = [make_read(tx, rng, 0.03, 9) for _ in range(8)]
    ys = [make_read(ty, rng, 0.02, 9) for _ in range(40)]
    y_bytes = sum(2 * band_bytes(len(r), 600, 9) for r in ys)
    assert y_bytes > 3 * (2 << 20), "Y outgrows the first band arena more than once"
    slx, sly = np.arange(8, dtype=np.int32), np.arange(8, 48, dtype=np.int32)
    pg = pack_groups([slx])
    props = all_proposals_arrays(tx)
    exp_dense, _ = oracle.cpu_pass(tx, xs, nthreads=2)
    mask = dense_mask(tx)
    e = Engine(0)
    try:
        e.set_option("dp_lat", 0)
        e.set_sequences(0, xs + ys)
        e.set_templates(0, [tx, ty])
        if not x_first:
            # X's slots filled and dropped, then part of Y from the arena's start, then X behind it
            e.realign(slx, slx, 0, [9] * 8, RF_FWD | RF_BWD)
            e.release_bands()
            e.realign(sly[:12], sly[:12], 1, [9] * 12, RF_FWD | RF_BWD)
            e.realign(slx[::-1], slx[::-1], 0, [9] * 8, RF_FWD | RF_BWD)
            parts = (sly[12:26], sly[26:])
        else:
            e.realign(slx, slx, 0, [9] * 8, RF_FWD | RF_BWD)
            parts = (sly[:12], sly[12:])
        first = _read_cluster(e, slx, pg, props)
        first = _read_cluster(e, slx, pg, props)          # the plans are cached now

        def check(what):
            got = _read_cluster(e, slx, pg, props)
            assert same(got[0], first[0]).all(), f"{what}: dense totals moved"
            assert same(got[0][mask], exp_dense[mask]).all(), f"{what}: dense totals differ from the oracle"
            for k in range(8):
                np.testing.assert_array_equal(got[1][k], first[1][k], err_msg=f"{what}: moves of read {k}")
                A, mv = oracle.forward(tx, xs[k], moves=True)
                np.testing.assert_array_equal(got[1][k], oracle.backtrace(mv, len(xs[k]) + 1, 101, 9))
            np.testing.assert_array_equal(got[2], first[2], err_msg=f"{what}: error counts")
            assert same(got[3], first[3]).all(), f"{what}: downloaded band moved"
            bm = inband_mask(len(xs[2]) + 1, 101, 9)
            assert same(got[3][bm], oracle.backward(tx, xs[2])[bm]).all(), f"{what}: band differs from the oracle"
            assert same(got[4], first[4]).all(), f"{what}: proposal scores moved"
            kd, p, b = props
            assert same(got[4], exp_dense[p, dense_slot(kd, b)]).all(), f"{what}: proposal scores differ"

        check("before growth")
        # band arena: Y in two calls, device_bytes rises at each
        sizes = [e.device_bytes()]
        for part in parts:
            sc = e.realign(part, part, 1, [9] * len(part), RF_FWD | RF_BWD)
            assert np.isfinite(sc).all()
            sizes.append(e.device_bytes())
            check(f"band arena growth to {sizes[-1]} bytes")
        assert sizes[0] < sizes[2] and (not x_first or sizes[0] < sizes[1] < sizes[2]), sizes
        # table arena: reads of Y's length at new ids (about 1.4 MB of tables an
        # upload, the arena holds about 3 MB) until the total rises
        extra = [make_read(ty, rng, 0.02, 9) for _ in range(60)]
        at, grew = 48, False
        for _ in range(6):
            before = e.device_bytes()
            e.set_sequences(at, extra)
            at += len(extra)
            if e.device_bytes() > before:
                grew = True
                check(f"table arena growth at id {at}")
                break
        assert grew, "the table arena did not grow"
        # byte arena: 256 B a sequence, 2 MB at first -- 9,000 one-base reads outgrow it
        tiny = [RifrafSequence(np.array([b], np.uint8), np.array([-1.0]), 9, SEQ_SCORES) for b in range(4)] * 2250
        before = e.device_bytes()
        e.set_sequences(at, tiny)
        assert e.device_bytes() > before, "the byte arena did not grow"
        check("byte arena growth")
        # Y was moved too: one of its reads against the oracle
        k = int(sly[20])
        got = e.download_band(k, RF_BAND_A).data
        bm = inband_mask(len(ys[20]) + 1, 601, 9)
        assert same(got[bm], oracle.forward(ty, ys[20])[0][bm]).all(), "a moved band of Y differs from the oracle"
    finally:
        e.close()


# ---------------------------------------------------------------------
# one pinned landing zone for every call family
# ---------------------------------------------------------------------
@pytest.mark.gpu
def test_landing_zone_growth_across_call_families():
    """rf_realign's scores, rf_alignment_proposals' masks and rf_backtrace's
    counts and moves land in one pinned zone of 1 MB at first.  On a fresh
    context: a small rf_realign (2 reads, n ~ m ~ 12, bw 3), then the masks
    of 120 one-read groups at m = 1000 (9 (m + 1) 120 = 1,081,080 bytes: the
    zone is freed and allocated again), the small rf_realign again, and
    rf_backtrace of two of the long slots.  Every result is the oracle's, and
    the two small calls return the same bits."""
    from _util import make_read
    rng = np.random.default_rng(6021)
    G, M = 120, 1000
    ts, tl = random_seq(12, rng), random_seq(M, rng)
    small = [make_read(ts, rng, 0.03, 3) for _ in range(2)]
    large = [make_read(tl, rng, 0.02, 9) for _ in range(G)]
    assert 9 * (M + 1) * G + 16 > 1 << 20 >= 9 * (M + 1) * (G - 4) + 16, "the masks just outgrow the first zone"

    def fill(t, r):
        A, mv = oracle.forward(t, r, moves=True)
        n, m, bw = len(r), len(t), r.bandwidth
        wk = oracle.backtrace(mv, n + 1, m + 1, bw)
        return A[n - m + max(m - n, 0) + bw, m], wk, oracle.count_errors(wk, t, r.seq)

    exp_small = np.array([fill(ts, r)[0] for r in small])
    exp_large = [fill(tl, r) for r in large]
    sls, sll = np.arange(2, dtype=np.int32), np.arange(2, 2 + G, dtype=np.int32)
    e = Engine(0)
    try:
        e.set_sequences(0, small + large)
        e.set_templates(0, [ts, tl])
        first = e.realign(sls, sls, 0, [3, 3], RF_FWD).copy()
        assert same(first, exp_small).all()
        got = e.realign(sll, sll, 1, [9] * G, RF_FWD)
        assert same(got, [x[0] for x in exp_large]).all()
        masks = e.alignment_proposals([sll[g:g + 1] for g in range(G)], True)
        for g in range(G):
            exp = np.zeros((M + 1, 9), np.uint8)
            kd, p, b = moves_to_proposals_np(exp_large[g][1], tl, large[g].seq)
            exp[p, dense_slot(kd, b)] = 1
            np.testing.assert_array_equal(masks[g], exp, err_msg=f"mask of group {g}")
        again = e.realign(sls, sls, 0, [3, 3], RF_FWD)
        assert again.tobytes() == first.tobytes()
        pick = [5, G - 1]
        moves, nerr = e.backtrace(sll[pick])
        for j, g in enumerate(pick):
            np.testing.assert_array_equal(moves[j], exp_large[g][1], err_msg=f"moves of slot {sll[g]}")
            assert nerr[j] == exp_large[g][2]
    finally:
        e.close()
