"""Exhaustive small-shape parity sweep: every (m, n, bw) with m, n in 1..12
and bw in {1, 2, 3, 5} -- 576 alignments per input class, one slot and one
template each, uploaded once and realigned in one call -- against the CPU
oracle, bit for bit: bands, A[end, end], skew / trim fills, backtraces, error
counts, proposal marking, read scoring (dense, proposal lists, 48-read ragged
groups), reference (codon) scoring of every STAGE_SCORE proposal (k_codon) and
the dense table with the reference's score added in every slot
(rf_score_dense_ref, k_codon_dense: 576 groups in one call, then with every
third group's reference taken out; the codon classes as the reference under
the fused and the split fold and both row strides, the non-codon classes as
a reference without codon tables).  Nothing
is sampled and nothing is masked beyond the dense table's non-proposal slots
(p = 0 sub / del and the consensus base's own slot).  The oracle raises on no
alignment and no proposal of any class; an OracleError fails the test (in
the non-codon reference sweep it would be a NaN that the engine has to meet;
there is none).

Input classes (fixed seeds): `seq` / `ref` (SEQ_SCORES / REF_SCORES, random
bases, error_log_p = log10(U(0.01, 0.3))), `seq0` / `ref0` (the same with
~20 % of positions at error_log_p = 0.0: match = -Inf) and `tie_seq` /
`tie_ref` (two-letter homopolymer runs, the read a copy of the template with
runs shortened or lengthened, constant error_log_p: exact move ties, counted
from the oracle's A band alone).

k_qv (the quality pass's normalisations) is compared with an 80-bit
evaluation of model.jl:722-771, 835-839 over the bit-exact inputs the kernel
consumes, at consensus lengths on both sides of its 256-thread stride.

Per class: 576 alignments, 24,226 in-band cells per band and 32,256
proposals.  The oracle side of a class is computed once per session (a
module-level cache).
"""
import math

import numpy as np
import pytest

import oracle
from _util import REF_SCORES, SEQ_SCORES, all_proposals_arrays, dense_slot, inband_mask, make_read, random_seq
from _util import tie_pair as _tie_pair
from rifraf_amd import RifrafSequence
from rifraf_amd.align import moves_to_proposals_np
from rifraf_amd.engine import RF_BAND_A, RF_BAND_B, RF_BWD, RF_FWD, RF_SKEW, RF_TRIM
from test_gpu_parity import launched_tasks
from test_sharded import QV_ATOL, QV_RTOL

pytestmark = pytest.mark.gpu

SHAPES = [(m, n, bw) for m in range(1, 13) for n in range(1, 13) for bw in (1, 2, 3, 5)]
NA = len(SHAPES)                      # 576 alignments per class
PER_M = NA // 12                      # the 48 alignments of one m are consecutive
BLOCK_TPL = np.repeat(np.arange(12) * PER_M, PER_M)   # per alignment: the first template of its m
SEEDS = {"seq": 1201, "ref": 1202, "seq0": 1203, "ref0": 1204, "tie_seq": 1205, "tie_ref": 1206}
CODON = ("ref", "ref0", "tie_ref")
NONCODON = ("seq", "seq0", "tie_seq")
TIE_LP = -1.0
GAP = 4


def _random_reads(rng, scores, zeros):
    out = []
    for m, n, bw in SHAPES:
        lp = np.log10(rng.uniform(0.01, 0.3, n))
        if zeros:
            lp[rng.random(n) < 0.2] = 0.0
        out.append(RifrafSequence(random_seq(n, rng), lp, bw, scores))
    return out


class _Class:
    """One input class: 576 (template, sequence) pairs and, computed once per
    session on first use, the oracle's results for them."""

    def __init__(self, name):
        self.name = name
        self.codon = name in CODON
        scores = REF_SCORES if self.codon else SEQ_SCORES
        rng = np.random.default_rng(SEEDS[name])
        self.templates, self.seqs = [], []
        if name.startswith("tie"):
            for m, n, bw in SHAPES:
                t, s = _tie_pair(m, n, rng)
                self.templates.append(t)
                self.seqs.append(RifrafSequence(s, np.full(n, TIE_LP), bw, scores))
        else:
            self.templates = [random_seq(m, rng) for m, _, _ in SHAPES]
            self.seqs = _random_reads(rng, scores, name.endswith("0"))
        self.bws = [bw for _, _, bw in SHAPES]
        self.props = [all_proposals_arrays(t) for t in self.templates]
        self.masks = [inband_mask(n + 1, m + 1, bw) for m, n, bw in SHAPES]
        self._memo = {}

    def memo(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    # -- the oracle side ------------------------------------------------
    def fills(self, skew=False, trim=False):
        """[(A, moves band)] of forward_moves! per alignment."""
        return self.memo(("fwd", skew, trim), lambda: [
            oracle.forward(t, s, moves=True, skew=skew, trim=trim) for t, s in zip(self.templates, self.seqs)])

    def backward(self):
        return self.memo("bwd", lambda: [oracle.backward(t, s) for t, s in zip(self.templates, self.seqs)])

    def walks(self, skew=False, trim=False):
        """[(moves, n_errors)] of backtrace / count_errors per alignment."""
        def run():
            out = []
            for (m, n, bw), t, s, (_, mv) in zip(SHAPES, self.templates, self.seqs, self.fills(skew, trim)):
                w = oracle.backtrace(mv, n + 1, m + 1, bw)
                out.append((w, oracle.count_errors(w, t, s.seq)))
            return out
        return self.memo(("walk", skew, trim), run)

    def marks(self, do_indels):
        """The (m + 1, 9) proposal mask of each alignment's walk."""
        def run():
            out = []
            for t, s, (w, _) in zip(self.templates, self.seqs, self.walks()):
                k, p, b = moves_to_proposals_np(w, t, s.seq)
                if not do_indels:
                    keep = k == 0
                    k, p, b = k[keep], p[keep], b[keep]
                e = np.zeros((len(t) + 1, 9), np.uint8)
                e[p, dense_slot(k, b)] = 1
                out.append(e)
            return out
        return self.memo(("marks", do_indels), run)

    def dense(self):
        """cpu_pass totals of each alignment alone (non-codon classes)."""
        return self.memo("dense", lambda: [oracle.cpu_pass(t, [s], nthreads=1)[0]
                                           for t, s in zip(self.templates, self.seqs)])

    def dense_by_m(self):
        """cpu_pass totals of the 48 reads of one m against one template
        (the first alignment's of that m), folded in slot order."""
        return self.memo("dense_m", lambda: [
            oracle.cpu_pass(self.templates[g * PER_M], self.seqs[g * PER_M:(g + 1) * PER_M], nthreads=1)[0]
            for g in range(12)])

    def block_walks(self):
        """The backtrace of each alignment's read against its m's first
        template (BLOCK_TPL: the consensus the reads of one m share)."""
        def run():
            out = []
            for k, ((m, n, bw), s) in enumerate(zip(SHAPES, self.seqs)):
                t = self.templates[BLOCK_TPL[k]]
                out.append(oracle.backtrace(oracle.forward(t, s, moves=True)[1], n + 1, m + 1, bw))
            return out
        return self.memo("block_walks", run)

    def ref_scores(self):
        """score_proposal of every STAGE_SCORE proposal with the class's
        sequence as the reference: [(totals = 0.0 + s_ref, per-sequence column)]."""
        A, B = self.fills(), self.backward()
        return self.memo("refsc", lambda: [
            oracle.score_list(self.props[k], [], [], [], self.templates[k], A[k][0], B[k], self.seqs[k],
                              per_seq=True, nthreads=1) for k in range(NA)])

    def companions(self):
        """Two non-codon reads per alignment (same n and bw, other bases),
        scored beside the codon slot as a group's batch.  The codon classes
        share them, so their tables enter the engine's row-code dictionary
        once."""
        def run():
            rng = np.random.default_rng(1300)
            a, b = _random_reads(rng, SEQ_SCORES, False), _random_reads(rng, SEQ_SCORES, False)
            return [r for pair in zip(a, b) for r in pair]
        return self.memo("comp", run)

    def mixed_totals(self):
        """score_total of every proposal over the two companions and the
        codon reference, per alignment."""
        def run():
            A, B, comp = self.fills(), self.backward(), self.companions()
            out = []
            for k in range(NA):
                t, rs = self.templates[k], comp[2 * k:2 * k + 2]
                out.append(oracle.score_list(self.props[k], [oracle.forward(t, r)[0] for r in rs],
                                             [oracle.backward(t, r) for r in rs], rs, t, A[k][0], B[k],
                                             self.seqs[k], nthreads=1))
            return out
        return self.memo("mixed", run)

    def plain_ref_totals(self):
        """mixed_totals for a non-codon class: the two companions, then the
        class's sequence as a reference without codon tables (score_nocodon /
        seq_score_deletion).  Where score_list raises, the alignment is
        evaluated proposal by proposal and a proposal the oracle raises on is
        NaN."""
        def run():
            A, B, comp = self.fills(), self.backward(), self.companions()
            out = []
            for k in range(NA):
                t, rs, ref = self.templates[k], comp[2 * k:2 * k + 2], self.seqs[k]
                As, Bs = [oracle.forward(t, r)[0] for r in rs], [oracle.backward(t, r) for r in rs]
                try:
                    tot = oracle.score_list(self.props[k], As, Bs, rs, t, A[k][0], B[k], ref, nthreads=1)
                except oracle.OracleError:
                    tot = np.empty(len(self.props[k][0]))
                    for j, prop in enumerate(zip(*self.props[k])):
                        try:
                            tot[j] = oracle.score_total(prop, As, Bs, rs, t, A[k][0], B[k], ref)
                        except oracle.OracleError:
                            tot[j] = np.nan
                out.append(tot)
            return out
        return self.memo("plainref", run)


_CLASSES = {}


def cls_of(name):
    if name not in _CLASSES:
        _CLASSES[name] = _Class(name)
    return _CLASSES[name]


def move_tie_count(t, rs, A):
    """In-band cells of the oracle's A band whose value is reached by two or
    more moves (align.jl:50-112 restated over the sequence's tables): the
    cells where the strict `>` order match, insert, delete, codon insert,
    codon delete decides the trace."""
    s, n, m, bw = rs.seq, len(rs.seq), len(t), rs.bandwidth
    nrows, ncols, H = n + 1, m + 1, A.shape[0]
    off = max(ncols - nrows, 0) + bw

    def inband(i, j):
        return 1 <= i <= nrows and 1 <= j <= ncols and 0 <= i - j + off < H

    ncins, ncdel = len(rs.codon_ins_scores), len(rs.codon_del_scores)
    ties = 0
    for j in range(1, ncols + 1):
        for i in range(1, nrows + 1):
            if not inband(i, j) or (i == 1 and j == 1):
                continue
            seq_i = max(i - 1, 1)
            sb = s[i - 2] if i > 1 else GAP
            tb = t[j - 2] if j > 1 else GAP
            moves = [(rs.match_scores[seq_i - 1] if sb == tb else rs.mismatch_scores[seq_i - 1], 1, 1),
                     (rs.ins_scores[seq_i - 1], 1, 0), (rs.del_scores[i - 1], 0, 1)]
            if ncins > 0 and i > 3:
                moves.append((rs.codon_ins_scores[i - 4], 3, 0))
            if ncdel > 0 and j > 3:
                moves.append((rs.codon_del_scores[i - 1], 0, 3))
            cand = [A[i - di - (j - dj) + off, j - dj - 1] + sc for sc, di, dj in moves if inband(i - di, j - dj)]
            best = max(cand)
            assert best == A[i - j + off, j - 1]
            ties += cand.count(best) >= 2
    return ties


def same(got, exp):
    """Elementwise bit-equality, NaN equal to NaN only where both are NaN."""
    got, exp = np.asarray(got), np.asarray(exp)
    return (got == exp) | (np.isnan(got) & np.isnan(exp))


def upload(engine, c, flags, tpl=None, per_direction=False):
    """Upload a class and fill its bands: one rf_realign of every job, or
    (per_direction) the forward fills in one call and the backward fills in
    the next, 576 tasks each.  Returns A[end, end] per alignment."""
    engine.set_sequences(0, c.seqs)
    engine.set_templates(0, c.templates)
    ids = np.arange(NA)
    tpl = ids if tpl is None else tpl
    if not per_direction:
        return engine.realign(ids, ids, tpl, c.bws, flags)
    scores = engine.realign(ids, ids, tpl, c.bws, flags & ~RF_BWD)
    engine.realign(ids, ids, tpl, c.bws, RF_BWD)
    return scores


def upload_with_companions(engine, c):
    """Upload a class's sequences (slots 0 .. NA - 1) and its two companions
    per alignment (slots NA + 2 k, NA + 2 k + 1) and fill every band in one
    rf_realign.  Returns the batch slots of each alignment's group."""
    engine.set_sequences(0, c.seqs + c.companions())
    engine.set_templates(0, c.templates)
    ids = np.arange(3 * NA)
    tpl = np.concatenate([np.arange(NA), np.repeat(np.arange(NA), 2)])
    bws = np.concatenate([c.bws, np.repeat(c.bws, 2)])
    engine.realign(ids, ids, tpl, bws, RF_FWD | RF_BWD)
    return [np.array([NA + 2 * k, NA + 2 * k + 1]) for k in range(NA)]


def check_A(engine, c, scores, fills):
    for k, (m, n, bw) in enumerate(SHAPES):
        A = fills[k][0]
        got = engine.download_band(k, RF_BAND_A).data
        assert same(got[c.masks[k]], A[c.masks[k]]).all(), (c.name, "A", m, n, bw)
        if scores is not None:
            assert scores[k] == A[n - m + max(m - n, 0) + bw, m], (c.name, "A[end, end]", m, n, bw)


def check_walks(engine, c, walks, chunk=NA):
    for a in range(0, NA, chunk):
        moves, nerr = engine.backtrace(np.arange(a, min(a + chunk, NA)))
        for k, mv in enumerate(moves, a):
            np.testing.assert_array_equal(mv, walks[k][0], err_msg=f"{c.name} {SHAPES[k]}")
            assert nerr[k - a] == walks[k][1], (c.name, "n_errors", SHAPES[k])


def dense_mask(t):
    mask = np.ones((len(t) + 1, 9), bool)
    mask[0, :5] = False                                   # p = 0 has no sub / del
    mask[np.arange(1, len(t) + 1), np.asarray(t, np.int64)] = False   # the consensus base's own slot
    return mask


# The planner (rf_realign) sorts a call's DP tasks into launch classes; only
# the options that move these classes' tasks are crossed.
#   lean tasks (finite tables, no codon moves, no skew / trim: `seq` and
#   `tie_seq`; every H here is <= 22):
#     "tp"   dp_lat 0: the 16-lane throughput classes (k_dpr, lean)
#     "lat"  dp_lat 2048: the call's 1,152 lean tasks (<= dp_lat) all run in the
#            64-lane latency-mode class (k_dpx, lean), one task per wave
#   non-lean tasks (codon moves: `ref`, `ref0`, `tie_ref`; a read with a -Inf
#   table entry: most of `seq0`, whose all-finite reads are lean and so take
#   the "lat" leg as well; any forward fill with skew / trim).  dp_lat counts
#   lean tasks only and does not reach them; dp_nl64 does:
#     "nl16" dp_nl64 0: the 16-lane non-lean class (k_dpr, general step)
#     "nl64" dp_nl64 1024: a call with at most 1,024 non-lean tasks runs them in
#            the 64-lane k_dpx, one task per wave.  Forward + backward of a
#            class is 1,152 tasks, so this leg fills the two directions in
#            separate calls of 576 tasks (per_direction); the skew / trim
#            fills are forward only, 576 tasks in one call
LEAN = ("seq", "tie_seq")
DP_OPTS = {"tp": ("dp_lat", 0), "lat": ("dp_lat", 2048), "nl16": ("dp_nl64", 0), "nl64": ("dp_nl64", 1024)}


# the kernel families (Engine.last_dp_launches) a leg's tasks run in
LEG_KERNELS = {"tp": {"dpr_lean", "dpr_lean_pm"}, "lat": {"dpx_lean"}, "nl16": {"dpr"}, "nl64": {"dpx_codon"}}
LEAN_KERNELS = {"dpr_lean", "dpr_lean_pm", "dpr_wide64", "dpr_wide32", "dpx_lean"}


def check_leg(engine, dp, ntasks):
    """The last rf_realign ran its lean ("tp", "lat") or its non-lean ("nl16",
    "nl64") tasks in the leg's kernel family and in no other, with NP = 1
    (every H here is <= 22); ntasks: the call held only such tasks, this many
    (None: a call of lean and non-lean tasks, `seq0`)."""
    ran = launched_tasks(engine)
    assert {npi for _, npi in ran} == {0}, ran
    side = {k for k, _ in ran if (k in LEAN_KERNELS) == (dp in ("tp", "lat"))}
    assert side and side <= LEG_KERNELS[dp], (dp, ran)
    if ntasks is not None:
        assert {k for k, _ in ran} == side and sum(ran.values()) == ntasks, (dp, ran)


def dp_modes(names):
    """(class, launch class, band_pad) for the plain forward + backward fill."""
    legs = {name: ("tp", "lat") if name in LEAN else ("nl16", "nl64") for name in names}
    legs["seq0"] = ("nl16", "nl64", "lat")   # lean and non-lean reads in one call
    return [(name, dp, pad) for name in names for dp in legs[name] for pad in (64, 1)]


@pytest.mark.parametrize("name", ["tie_seq", "tie_ref"])
def test_tie_class_has_move_ties(name):
    """The tie classes hold cells whose best value is reached by two or more
    moves, by the oracle alone (A band + tables): 6,149 (tie_seq) and 9,885
    (tie_ref) of the 24,226 in-band cells of the 576 alignments."""
    c = cls_of(name)
    ties = sum(move_tie_count(t, s, A) for t, s, (A, _) in zip(c.templates, c.seqs, c.fills()))
    print(f"{name}: {ties} in-band cells with tied moves")
    assert ties > 0


@pytest.mark.parametrize("name,dp,pad", dp_modes(list(SEEDS)))
def test_sweep_bands(engine, opts, name, dp, pad):
    """A, B and A[end, end] of all 576 alignments of a class in each launch
    class its tasks can take (DP_OPTS above: "tp" / "lat" for the lean
    classes, "nl16" / "nl64" for the non-lean ones, all three for `seq0`), with default and
    all-padded row strides (band_pad).  One rf_realign fills both
    directions, except the "nl64" leg (one call per direction, so that the
    576 non-lean tasks of a call stay within dp_nl64 and run in k_dpx)."""
    c = cls_of(name)
    opts(*DP_OPTS[dp])
    opts("band_pad", pad)
    scores = upload(engine, c, RF_FWD | RF_BWD, per_direction=dp == "nl64")
    check_leg(engine, dp, None if name == "seq0" else NA if dp == "nl64" else 2 * NA)
    check_A(engine, c, scores, c.fills())
    for k, ((m, n, bw), B) in enumerate(zip(SHAPES, c.backward())):
        got = engine.download_band(k, RF_BAND_B).data
        assert same(got[c.masks[k]], B[c.masks[k]]).all(), (name, "B", m, n, bw)


@pytest.mark.parametrize("flags", [RF_SKEW, RF_TRIM, RF_SKEW | RF_TRIM])
@pytest.mark.parametrize("dp", ["nl16", "nl64"])
@pytest.mark.parametrize("name", ["seq", "ref"])
def test_sweep_skew_trim(engine, opts, name, dp, flags):
    """The forward band, A[end, end], backtrace and error count of every
    alignment under skew_matches, trim and both.  Skew / trim fills are
    non-lean tasks whatever the tables: 576 of them in one forward-only call
    run in the 16-lane k_dpr ("nl16") or the 64-lane k_dpx ("nl64")."""
    c = cls_of(name)
    opts(*DP_OPTS[dp])
    skew, trim = bool(flags & RF_SKEW), bool(flags & RF_TRIM)
    scores = upload(engine, c, RF_FWD | flags)
    check_leg(engine, dp, NA)
    check_A(engine, c, scores, c.fills(skew, trim))
    check_walks(engine, c, c.walks(skew, trim))


@pytest.mark.parametrize("nw", [4, 1])
@pytest.mark.parametrize("name", list(SEEDS))
def test_sweep_backtrace_and_marks(engine, opts, name, nw):
    """k_bt_win's moves and error counts, and rf_alignment_proposals' marks
    (one group per alignment, do_indels both ways), for every alignment:
    launches of 64 walks on 4 waves each (bt_nw 4) and one launch of 576
    one-wave walks (bt_nw 1)."""
    c = cls_of(name)
    opts("bt_nw", nw)
    upload(engine, c, RF_FWD | RF_BWD)
    chunk = 64 if nw == 4 else NA
    check_walks(engine, c, c.walks(), chunk)
    for do_indels in (True, False):
        exp = c.marks(do_indels)
        for a in range(0, NA, chunk):
            got = engine.alignment_proposals([[k] for k in range(a, min(a + chunk, NA))], do_indels)
            for k, g in enumerate(got, a):
                np.testing.assert_array_equal(g, exp[k], err_msg=f"{name} {SHAPES[k]} do_indels={do_indels}")


# score_kernel reaches the scorer choice only when every table entry of the
# launch's reads is finite (pick_scorer): `seq` and `tie_seq` run in k_score
# ("general"), k_score_ws ("ws") and k_score_segl ("seg"); "auto" picks k_score_ws for
# these narrow bands (the same kernel as "ws", kept as the setting that ships,
# through the selection code).  A `seq0` launch
# holds -Inf match scores, so every setting runs k_score: one leg, "auto".
SCORER_CASES = [(name, mode, kern) for name in NONCODON for mode in ("fused", "split")
                for kern in (("auto", "general", "ws", "seg") if name in LEAN else ("auto",))]


@pytest.mark.parametrize("name,mode,kern", SCORER_CASES)
def test_sweep_read_scoring(engine, opts, name, mode, kern):
    """rf_score_dense (one group per alignment) and rf_score over
    all_proposals_arrays against oracle.cpu_pass for all 576 alignments
    (32,256 proposals), then twelve groups of 48 reads -- every n and bw of
    one m against one template, maximally ragged members -- for the ordered
    fold; each dense scorer the class can reach (SCORER_CASES), fused and
    split."""
    c = cls_of(name)
    opts("score_mode", mode)
    opts("score_kernel", kern)
    upload(engine, c, RF_FWD | RF_BWD)
    exp = c.dense()
    got = engine.score_dense([np.array([k]) for k in range(NA)])
    lists = engine.score([([k], -1, c.props[k]) for k in range(NA)])
    for k, t in enumerate(c.templates):
        mask = dense_mask(t)
        assert same(got[k][mask], exp[k][mask]).all(), (name, "dense", SHAPES[k])
        kd, p, b = c.props[k]
        assert same(lists[k], exp[k][p, dense_slot(kd, b)]).all(), (name, "list", SHAPES[k])
    # 48 reads per group: the same sequences against their m's first template
    upload(engine, c, RF_FWD | RF_BWD, tpl=np.repeat(np.arange(12) * PER_M, PER_M))
    groups = [np.arange(g * PER_M, (g + 1) * PER_M) for g in range(12)]
    got = engine.score_dense(groups)
    lists = engine.score([(groups[g], -1, c.props[g * PER_M]) for g in range(12)])
    for g, e in enumerate(c.dense_by_m()):
        mask = dense_mask(c.templates[g * PER_M])
        assert same(got[g][mask], e[mask]).all(), (name, "dense, 48 reads", g + 1)
        kd, p, b = c.props[g * PER_M]
        assert same(lists[g], e[p, dense_slot(kd, b)]).all(), (name, "list, 48 reads", g + 1)


@pytest.mark.parametrize("name", CODON)
def test_sweep_reference_scoring(engine, name):
    """k_codon on every STAGE_SCORE proposal (32,256) of all 576 alignments
    with the class's sequence as the reference slot of an otherwise empty
    group: the total 0.0 + s_ref and the per-sequence column against
    oracle.score_proposal (m or n below 4: no codon move fits; bw 1: no
    3-step move stays in band; n far from m; the just_a tail and the
    deletion-at-last-column shortcut at every m)."""
    c = cls_of(name)
    upload(engine, c, RF_FWD | RF_BWD)
    tot, per = engine.score([([], k, c.props[k]) for k in range(NA)], per_seq=True)
    for k, (e_tot, e_per) in enumerate(c.ref_scores()):
        bad = ~same(tot[k], e_tot) | ~same(per[k][:, 0], e_per[:, 0])
        if bad.any():
            j = int(np.argmax(bad))
            kd, p, b = (int(x[j]) for x in c.props[k])
            raise AssertionError(f"{name} {SHAPES[k]} proposal (kind {kd}, pos {p}, base {b}): "
                                 f"{tot[k][j]!r} != {e_tot[j]!r}")


@pytest.mark.parametrize("mode", ["fused", "split"])
@pytest.mark.parametrize("name", CODON)
def test_sweep_reads_plus_reference(engine, opts, name, mode):
    """Groups of two non-codon reads plus the codon slot as the reference,
    one per alignment: the total of every proposal against
    oracle.score_total (reads folded first, the reference last)."""
    c = cls_of(name)
    opts("score_mode", mode)
    batches = upload_with_companions(engine, c)
    tot = engine.score([(batches[k], k, c.props[k]) for k in range(NA)])
    for k, e in enumerate(c.mixed_totals()):
        bad = ~same(tot[k], e)
        if bad.any():
            j = int(np.argmax(bad))
            kd, p, b = (int(x[j]) for x in c.props[k])
            raise AssertionError(f"{name} {SHAPES[k]} proposal (kind {kd}, pos {p}, base {b}): "
                                 f"{tot[k][j]!r} != {e[j]!r}")


def dense_table(c, k, totals):
    """The totals of alignment k's proposal list in the dense layout (NaN in
    the slots that are no proposal)."""
    kd, p, b = c.props[k]
    out = np.full((len(c.templates[k]) + 1, 9), np.nan)
    out[p, dense_slot(kd, b)] = totals
    return out


def check_dense_reference(engine, c, batches, exp):
    """rf_score_dense_ref of all 576 groups in one call (reference slot k for
    group k) against the expected proposal totals under dense_mask; then the
    same call with ref_slot -1 for every k % 3 == 1, so that the kernel's
    descriptor list is a strict subset of the groups with gaps in it: those
    groups have rf_score_dense's bits in every slot, the others the first
    call's."""
    first = engine.score_dense_ref(batches, np.arange(NA))
    masks = [dense_mask(t) for t in c.templates]
    for k in range(NA):
        assert np.isnan(first[k][0, :5]).all(), (c.name, "p = 0 sub / del", SHAPES[k])
        bad = ~same(first[k], dense_table(c, k, exp[k])) & masks[k]
        if bad.any():
            p, slot = (int(x) for x in np.argwhere(bad)[0])
            raise AssertionError(f"{c.name} {SHAPES[k]} pos {p} slot {slot}: "
                                 f"{first[k][p, slot]!r} != {dense_table(c, k, exp[k])[p, slot]!r}")
    refs = np.arange(NA)
    refs[1::3] = -1
    second = engine.score_dense_ref(batches, refs)
    plain = engine.score_dense(batches)
    for k in range(NA):
        if k % 3 == 1:
            assert same(second[k], plain[k]).all(), (c.name, "no reference: rf_score_dense", SHAPES[k])
        else:
            assert np.isnan(second[k][0, :5]).all(), (c.name, "p = 0 sub / del, second call", SHAPES[k])
            assert same(second[k][masks[k]], first[k][masks[k]]).all(), (c.name, "second call", SHAPES[k])


@pytest.mark.parametrize("pad", [64, 1])
@pytest.mark.parametrize("mode", ["fused", "split"])
@pytest.mark.parametrize("name", CODON)
def test_sweep_dense_reference(engine, opts, name, mode, pad):
    """k_codon_dense on every slot of all 576 alignments: groups of two
    non-codon reads with the class's codon sequence as the reference slot, in
    one rf_score_dense_ref call, against oracle.score_total (mixed_totals)
    laid out as the dense table; the reads' fold fused and split (k_reduce
    writes the totals the kernel then adds to), default and all-padded row
    strides.  The tables of `ref` and `ref0` differ at every position, so a
    table read one position off is a different number.  Then the call with
    every third group's reference taken out (check_dense_reference)."""
    c = cls_of(name)
    opts("score_mode", mode)
    opts("band_pad", pad)
    batches = upload_with_companions(engine, c)
    check_dense_reference(engine, c, batches, c.mixed_totals())


@pytest.mark.parametrize("name", NONCODON)
def test_sweep_dense_plain_reference(engine, name):
    """The `ncins == 0 && ncdel == 0` branch of k_codon_dense (score_nocodon
    and seq_score_deletion) on every slot of all 576 alignments: the class's
    sequence, which has no codon tables, as the reference slot beside the two
    companions, against oracle.score_list over the three
    (plain_ref_totals; a proposal the oracle raises on is NaN and must meet
    NaN).  From the oracle alone, asserted before the engine runs: every
    compared slot of `seq` and `tie_seq` is finite, and every alignment of
    every class has a finite compared slot.  No shape of `seq0` is exempt:
    its -Inf match scores leave the mismatch, insertion and deletion moves,
    and the oracle gives all 32,256 slots of each of the three classes a
    finite total and raises on none."""
    c = cls_of(name)
    exp = c.plain_ref_totals()
    finite = [np.isfinite(e) for e in exp]     # a proposal list holds exactly the compared slots
    print(f"{name}: {sum(int(f.sum()) for f in finite)} finite and "
          f"{sum(int(np.isnan(e).sum()) for e in exp)} NaN compared slots of {sum(len(e) for e in exp)}")
    if name in LEAN:
        assert all(f.all() for f in finite), name
    assert all(f.any() for f in finite), name
    batches = upload_with_companions(engine, c)
    check_dense_reference(engine, c, batches, exp)


def test_qv_probs_extended_precision(engine):
    """k_qv against model.jl:722-771 and :835-839 evaluated in 80-bit
    np.longdouble over the kernel's own bit-exact inputs (rf_score_dense
    totals and rf_aln_error_sums, both pinned to the oracle elsewhere):
    consensus lengths 1, 2, 255, 256, 257 and 600 in one call (below, at and
    above the 256-thread stride; the ins rows of later groups start at
    rows + g), 3-5 reads each at bw 9.  The project's QV_RTOL / QV_ATOL; every
    pos row, and every ins row plus the state term, sums to 1 within 1e-12.
    The 80-bit side also keeps the exponent score - max unrounded; the
    largest errors seen are printed."""
    if np.finfo(np.longdouble).nmant < 63:
        pytest.skip("np.longdouble has fewer than 64 significand bits on this host")
    rng = np.random.default_rng(722)
    tlens = [1, 2, 255, 256, 257, 600]
    templates = [random_seq(L, rng) for L in tlens]
    reads = [[make_read(t, rng, 0.03, 9) for _ in range(3 + g % 3)] for g, t in enumerate(templates)]
    flat = [r for rs in reads for r in rs]
    n = len(flat)
    engine.set_sequences(0, flat)
    engine.set_templates(0, templates)
    tpl = np.concatenate([[g] * len(rs) for g, rs in enumerate(reads)])
    sc = engine.realign(np.arange(n), np.arange(n), tpl, [9] * n, RF_FWD | RF_BWD)
    groups, at = [], 0
    for rs in reads:
        groups.append(np.arange(at, at + len(rs)))
        at += len(rs)
    worst, worst_abs = check_qv_probs(engine, groups, templates, reads, sc)
    assert math.isfinite(worst)
    print(f"k_qv: largest relative error against the 80-bit evaluation {worst:.3e} "
          f"(values above {QV_ATOL / QV_RTOL:g}); largest absolute error below that {worst_abs:.3e}")


def check_qv_probs(engine, groups, templates, reads, sc):
    """rf_qv_probs of `groups` (slot lists in batch order; templates[g] and
    reads[g] are group g's consensus and RifrafSequences, sc the A[end, end]
    of every slot) against the 80-bit evaluation of its own inputs.  Returns
    the largest relative and absolute errors seen."""
    tlens = [len(t) for t in templates]
    state = []
    for g in groups:
        tot = 0.0
        for k in g:                                       # batch-order sum
            tot += float(sc[k])
        state.append(tot)
    dense = [d.copy() for d in engine.score_dense(groups)]
    sums = [a.copy() for a in engine.aln_error_sums(groups, tlens, reads)]
    res = engine.qv_probs(groups, tlens, state)
    assert res is not None, "a read has no row codes: the device quality pass did not run"
    pos, ins, aln, err = res
    assert err[0] == 0, f"k_qv reports error {err[0]} in group {err[1]}"
    ld = np.longdouble
    ten = ld(10)
    worst, worst_abs, rows = 0.0, 0.0, 0
    for g, (t, m) in enumerate(zip(templates, tlens)):
        D = dense[g].astype(ld)
        sub = D[1:, 0:4].copy()
        sub[np.arange(m), t.astype(np.int64)] = ld(0.0 + state[g])
        dele, insr = D[1:, 4], D[:, 5:9]
        assert not (np.isnan(sub).any() or np.isnan(dele).any() or np.isnan(insr).any())
        mx = max(sub.max(), dele.max(), insr.max())
        pos_exp = np.power(ten, np.hstack([sub - mx, (dele - mx)[:, None]]))
        e_pos = pos_exp / pos_exp.sum(axis=1, keepdims=True)
        ins_exp = np.power(ten, insr - mx)
        denom = np.power(ten, ld(state[g]) - mx) + ins_exp.sum(axis=1, keepdims=True)
        e_ins = ins_exp / denom
        e_state = np.power(ten, ld(state[g]) - mx) / denom[:, 0]
        a_exp = np.power(ten, sums[g].astype(ld))
        e_aln = 1 - (a_exp / a_exp.sum(axis=1, keepdims=True)).max(axis=1)
        g_pos, g_ins, g_aln = pos[rows:rows + m], ins[rows + g:rows + g + m + 1], aln[rows:rows + m]
        rows += m
        for what, got, exp in (("pos", g_pos, e_pos), ("ins", g_ins, e_ins), ("aln", g_aln, e_aln)):
            diff = np.abs(got.astype(ld) - exp)
            # relative where the rtol term decides (1 - max cancels: aln near 0 is held by atol)
            big = QV_RTOL * np.abs(exp) > QV_ATOL
            worst = max(worst, float((diff[big] / np.abs(exp[big])).max()) if big.any() else 0.0)
            worst_abs = max(worst_abs, float(diff[~big].max()) if (~big).any() else 0.0)
            assert (diff <= QV_ATOL + QV_RTOL * np.abs(exp)).all(), \
                f"group {g} (m = {m}) {what}: largest error {float(diff.max()):.3e}"
        assert np.abs(g_pos.astype(ld).sum(axis=1) - 1).max() <= 1e-12, f"group {g}: pos rows"
        # rf_qv_probs does not return the state term 10^(score - max) / denominator, so it is
        # the 80-bit one: this bounds the sum of the engine's ins row, not an engine-only identity
        assert np.abs(g_ins.astype(ld).sum(axis=1) + e_state - 1).max() <= 1e-12, f"group {g}: ins rows"
    return worst, worst_abs


def ragged_groups():
    """144 groups of 1-6 slots in a drawn (batch) order: for each m, the sizes
    1..6 twice over, drawn without replacement from the 48 alignments of that
    m, every n and bw among them.  The members of a group share the first
    template of their m (BLOCK_TPL)."""
    rng = np.random.default_rng(1400)
    groups = []
    for g in range(12):
        order = g * PER_M + rng.permutation(PER_M)
        at = 0
        for size in (1, 2, 3, 4, 5, 6) * 2:
            groups.append(order[at:at + size].astype(np.int32))
            at += size
    return groups


@pytest.mark.parametrize("marks_min", [128, 0])
@pytest.mark.parametrize("name", LEAN)
def test_sweep_aln_error_sums(engine, opts, name, marks_min):
    """rf_aln_error_sums' device fold over ragged groups of 1-6 reads at
    consensus lengths 1..12 against alignment_error_probs's sums
    (model.jl:817-840) folded on the host over the oracle's walks
    (model._add_base_distributions), bit for bit: k_aln_sums (aln_marks_min
    at its default) and the k_aln_marks + k_aln_fold pair (aln_marks_min 0).
    The host tables are withheld (bptr / mptr None), so a fall-back to the
    library's host fold would return None."""
    from rifraf_amd.model import _add_base_distributions
    c = cls_of(name)
    opts("aln_marks_min", marks_min)
    upload(engine, c, RF_FWD | RF_BWD, tpl=BLOCK_TPL)
    groups = ragged_groups()
    walks = c.block_walks()
    tlens = [SHAPES[g[0]][0] for g in groups]
    got = engine.aln_error_sums_ptr(groups, tlens, None, None, [len(c.seqs[k]) for g in groups for k in g])
    assert got is not None, "a read has no row codes: the device fold did not run"
    assert len(got) == len(groups)
    for g, m, sums in zip(groups, tlens, got):
        exp = np.zeros((m, 4))
        _add_base_distributions(exp, [walks[k] for k in g], [c.seqs[k] for k in g])
        assert sums.shape == (m, 4)
        assert same(sums, exp).all(), (name, "aln sums", [SHAPES[k] for k in g])


@pytest.mark.parametrize("name", LEAN)
def test_sweep_qv_probs(engine, name):
    """k_qv over the same ragged groups (consensus lengths 1..12, 1-6 reads)
    against the 80-bit evaluation of test_qv_probs_extended_precision, at its
    bound (QV_RTOL / QV_ATOL, rows summing to 1 within 1e-12)."""
    if np.finfo(np.longdouble).nmant < 63:
        pytest.skip("np.longdouble has fewer than 64 significand bits on this host")
    c = cls_of(name)
    sc = upload(engine, c, RF_FWD | RF_BWD, tpl=BLOCK_TPL)
    groups = ragged_groups()
    worst, worst_abs = check_qv_probs(engine, groups, [c.templates[BLOCK_TPL[g[0]]] for g in groups],
                                      [[c.seqs[k] for k in g] for g in groups], sc)
    assert math.isfinite(worst)
    print(f"k_qv, {name}: largest relative error against the 80-bit evaluation {worst:.3e}; "
          f"largest absolute error below {QV_ATOL / QV_RTOL:g}: {worst_abs:.3e}")
