"""rf_host_shift_fix (csrc/rifraf_shift_fix.h) and the Python side of
rf_pair_shifts without a GPU.

1. The host restatement of k_pa_fix against the Python one
   (pairalign._single_indels + proposals.apply_proposals) over freely
   generated move lists.
2. The ABI's rules: capacity truncation, NULL arguments, failed pairs.
3. pairalign's wrappers over a stand-in engine whose pair_shifts is the CPU
   oracle's moves fed to host_shift_fix.
4. The generator of the GPU sweep (tests/test_pair_shifts.py), run through
   the oracle, meets its coverage conditions.

The sweep's pairs: correct_shifts' tables make a mismatch far cheaper than a
deletion plus an insertion, and a codon insertion plus a deletion cheaper
than two insertions, so an optimal alignment under them never holds "delete,
then insert at one position".  SPECIAL pairs therefore close the sweep:
their mismatch and codon tables are -Inf, which leaves single indels as the
only way past a substitution, and the cell rule's order (insert before
delete on a tie, align.jl:77-104) makes that "delete, then insert".  For the
same reason two missing bases are not two insertions at one position under
those tables, and a second group of SPECIAL pairs, with -Inf codon tables
alone, holds the sweep's ambiguous sets.
"""
import numpy as np
import pytest

import oracle
from rifraf_amd import (AmbiguousProposalsError, DNASeq, ErrorModel, RifrafSequence, Scores, _lib, apply_proposals,
                        pairalign)
from rifraf_amd.engine import RF_SKEW, RF_TRIM, RifrafError
from rifraf_amd.proposals import DEL, INS
from rifraf_amd.types import dna_str
from test_pair_align_host import SHIFT_KATS, StandInEngine

SHIFT_SCORES = Scores.from_errors(ErrorModel(10.0, 1e-5, 1e-5, 1.0, 1.0))   # correct_shifts' default
NOCODON_SCORES = Scores.from_errors(ErrorModel(10.0, 1e-5, 1e-5, 0.0, 0.0))  # two missing bases: two insertions
EDGE_COUNTS = (63, 64, 65, 128, 129)
DI = {1: 1, 2: 1, 3: 0, 4: 3, 5: 0}
DJ = {1: 1, 2: 0, 3: 1, 4: 0, 5: 3}


# ---------------------------------------------------------------------
# the Python restatement
# ---------------------------------------------------------------------
def python_fix(mv, s, t):
    """(proposals, corrected template or None if ambiguous, tallies) of one move list."""
    props = pairalign._single_indels(np.asarray(mv, np.int8), s)
    try:
        fixed = apply_proposals(np.asarray(t, np.uint8), props)
    except AmbiguousProposalsError:
        fixed = None
    return props, fixed, [int(np.sum(np.asarray(mv) == c)) for c in range(1, 6)]


def check_against_python(r, moves, seqs, tpls, what=None):
    """Every output of a PairShifts (all products, full capacity) against python_fix."""
    assert r.n == len(moves)
    for k, (mv, s, t) in enumerate(zip(moves, seqs, tpls)):
        tag = k if what is None else what[k]
        if mv is None:
            assert (r.fixed_len[k], r.nprops[k]) == (-1, -1) and (r.tally[k] == -1).all(), tag
            assert r.fixed_seq(k) is None and r.proposals(k) is None, tag
            continue
        props, fixed, tally = python_fix(mv, s, t)
        assert r.nprops[k] == len(props) and r.proposals(k) == props, (tag, r.proposals(k), props)
        assert r.tally[k].tolist() == tally, tag
        if fixed is None:
            assert r.fixed_len[k] == -2 and r.fixed_seq(k) is None, tag
        else:
            assert r.fixed_len[k] == len(fixed), tag
            assert r.fixed_seq(k).tolist() == fixed.tolist(), (tag, r.fixed_seq(k), fixed)


# ---------------------------------------------------------------------
# 1. free move lists
# ---------------------------------------------------------------------
def free_lists():
    """About 2,000 move lists of 0..200 moves over all five codes, not from a
    DP, with bases to match: random lists under several code mixes, lists
    of the chunk-edge lengths, and lists with the patterns planted."""
    rng = np.random.default_rng(3101)
    mixes = ([.6, .1, .1, .1, .1], [.2, .2, .2, .2, .2], [.1, .5, .1, .2, .1], [.85, .05, .05, .03, .02],
             [.0, .4, .3, .3, .0])
    lists = []
    for q in range(1900):
        ln = int(rng.integers(0, 201))
        lists.append(rng.choice(np.arange(1, 6), size=ln, p=mixes[q % len(mixes)]).astype(np.int8))
    for ln in (0, 1) + EDGE_COUNTS:
        for mix in mixes[:3]:
            lists.append(rng.choice(np.arange(1, 6), size=ln, p=mix).astype(np.int8))
    plant = ([2, 4, 2], [3, 2], [3, 4, 2], [2, 2], [2, 4, 4, 2], [5, 2], [2, 3, 2])
    for q in range(70):
        pre = rng.choice(np.arange(1, 6), size=int(rng.integers(0, 130)), p=mixes[0]).astype(np.int8)
        post = rng.choice(np.arange(1, 6), size=int(rng.integers(0, 60)), p=mixes[0]).astype(np.int8)
        lists.append(np.concatenate([pre, np.array(plant[q % len(plant)], np.int8), post]))
    for q in range(12):   # inserts before any template base
        lists.append(np.concatenate([np.array([2, 4, 2][:1 + q % 3], np.int8),
                                     rng.choice(np.arange(1, 6), size=20 + q, p=mixes[0]).astype(np.int8)]))
    seqs = [rng.integers(0, 4, size=sum(DI[int(c)] for c in mv)).astype(np.uint8) for mv in lists]
    tpls = [rng.integers(0, 4, size=sum(DJ[int(c)] for c in mv)).astype(np.uint8) for mv in lists]
    return lists, seqs, tpls


def has_run(mv, first, between, last):
    """Does mv hold `first`, any number of `between` codes, then `last`?"""
    mv = [int(c) for c in mv]
    for a, c in enumerate(mv):
        if c != first:
            continue
        b = a + 1
        while b < len(mv) and mv[b] in between:
            b += 1
        if b < len(mv) and mv[b] == last and (not between or b > a + 1):
            return True
    return False


def test_host_shift_fix_equals_python():
    lists, seqs, tpls = free_lists()
    assert 1900 <= len(lists) <= 2100 and max(len(mv) for mv in lists) <= 200
    # what the lists must hold
    assert {c for mv in lists for c in mv.tolist()} == {1, 2, 3, 4, 5}
    assert any(has_run(mv, 2, (4,), 2) for mv in lists)          # insert, codon insert, insert
    assert any(has_run(mv, 3, (), 2) for mv in lists)            # delete then insert at one position
    assert any(len(mv) and mv[0] == 2 for mv in lists)           # an insert before any template base
    assert {0, 1, 63, 64, 65, 128, 129} <= {len(mv) for mv in lists}
    r = _lib.host_shift_fix(lists, seqs, tpls)
    check_against_python(r, lists, seqs, tpls)
    assert 20 < int((r.fixed_len == -2).sum()) < len(lists)      # both outcomes of are_ambiguous are exercised
    ins0 = sum(any(p.kind == INS and p.pos == 0 for p in r.proposals(k)) for k in range(r.n))
    both = sum(bool({p.pos for p in r.proposals(k) if p.kind == INS} & {p.pos for p in r.proposals(k) if p.kind == DEL})
               for k in range(r.n))
    assert ins0 >= 10 and both >= 10


# ---------------------------------------------------------------------
# 2. the ABI's rules
# ---------------------------------------------------------------------
def small_case():
    mv = [np.array([2, 1, 3, 2, 1, 4, 1, 5, 3, 2], np.int8), None, np.array([1, 1, 2, 2, 1], np.int8)]
    s = [np.array([0, 1, 2, 3, 0, 1, 2, 3, 0], np.uint8), np.array([1, 1], np.uint8), np.array([0, 1, 2, 3, 0], np.uint8)]
    t = [np.array([3, 2, 1, 0, 3, 2, 1, 0], np.uint8), np.array([2], np.uint8), np.array([0, 1, 0], np.uint8)]
    return mv, s, t


def test_capacity_truncation():
    mv, s, t = small_case()
    full = _lib.host_shift_fix(mv, s, t)
    assert full.nprops.tolist() == [5, -1, 2] and full.fixed_len.tolist() == [len(full.fixed_seq(0)), -1, -2]
    cut = _lib.host_shift_fix(mv, s, t, prop_cap=[2, 3, 0])
    assert cut.nprops.tolist() == [5, -1, 2]                       # the true counts
    assert cut.proposals(0) == full.proposals(0)[:2] and cut.proposals(2) == []
    assert cut.prop_kind.tolist()[:2] == [INS, DEL] and (cut.prop_kind[2:] == 255).all()   # nothing past the capacity
    assert (cut.prop_pos[2:] == -1).all() and (cut.prop_base[2:] == 255).all()
    assert cut.fixed_seq(0).tolist() == full.fixed_seq(0).tolist()
    assert (cut.fixed[cut.fixed_off[1]:] == 255).all()             # the failed and the ambiguous pair: no bytes


def raw_call(mv, s, t, **nulls):
    """rf_host_shift_fix with chosen arguments NULL -> (rc, PairShifts)."""
    n = len(mv)
    nm = [len(a) + len(b) for a, b in zip(s, t)]
    r = _lib.PairShifts(n, nm, nm)
    cat = lambda xs, ty: np.ascontiguousarray(np.concatenate([np.asarray(x, ty) for x in xs] + [np.zeros(1, ty)]), ty)   # noqa: E731
    off = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)   # noqa: E731
    mvs = [np.zeros(0, np.int8) if x is None else x for x in mv]
    nmoves = np.array([-1 if x is None else len(x) for x in mv], np.int32)
    args = dict(moves=cat(mvs, np.int8), moves_off=off(mvs), nmoves=nmoves, sbases=cat(s, np.uint8), s_off=off(s),
                tbases=cat(t, np.uint8), t_off=off(t), fixed=r.fixed, fixed_off=r.fixed_off, fixed_len=r.fixed_len,
                nprops=r.nprops, prop_off=r.prop_off, prop_kind=r.prop_kind, prop_pos=r.prop_pos,
                prop_base=r.prop_base, tally=r.tally)
    for k, v in nulls.items():
        args[k] = v
    rc = _lib.load().rf_host_shift_fix(n, *(_lib.ptr(a) for a in args.values()))
    return rc, r


def untouched(r):
    return ((r.fixed == 255).all() and (r.fixed_len == -1).all() and (r.nprops == -1).all() and
            (r.prop_kind == 255).all() and (r.prop_pos == -1).all() and (r.tally == -1).all())


def test_null_rules():
    mv, s, t = small_case()
    rc, r = raw_call(mv, s, t)
    assert rc == 0 and r.nprops.tolist() == [5, -1, 2]
    # every output may be NULL, one at a time and all together
    for name in ("fixed", "fixed_len", "nprops", "tally"):
        rc, r = raw_call(mv, s, t, **{name: None})
        assert rc == 0, name
    rc, r = raw_call(mv, s, t, prop_kind=None, prop_pos=None, prop_base=None, prop_off=None, fixed=None, fixed_off=None)
    assert rc == 0 and r.nprops.tolist() == [5, -1, 2] and r.fixed_len.tolist()[1:] == [-1, -2]
    rc, r = raw_call(mv, s, t, fixed=None, fixed_off=None, fixed_len=None, nprops=None, prop_off=None, prop_kind=None,
                     prop_pos=None, prop_base=None, tally=None)
    assert rc == 0
    # refused, and nothing written: fixed without its offsets, records not together or without offsets
    for nulls in (dict(fixed_off=None), dict(prop_off=None), dict(prop_kind=None), dict(prop_pos=None),
                  dict(prop_base=None, prop_kind=None), dict(moves_off=None), dict(nmoves=None), dict(s_off=None)):
        rc, r = raw_call(mv, s, t, **nulls)
        assert rc < 0 and untouched(r), nulls
    # a move code outside 1..5, moves that leave a string, offsets that decrease
    bad = [x if x is None else x.copy() for x in mv]
    bad[2][1] = 6
    rc, r = raw_call(bad, s, t)
    assert rc < 0 and untouched(r)
    rc, r = raw_call(mv, s, [t[0][:-1], t[1], t[2]])
    assert rc < 0 and untouched(r)
    rc, r = raw_call(mv, s, t, prop_off=np.array([0, 4, 2, 9], np.int64))
    assert rc < 0 and untouched(r)


def test_failed_pairs():
    mv, s, t = small_case()
    r = _lib.host_shift_fix([None, mv[2], None], [s[1], s[2], s[1]], [t[1], t[2], t[1]])
    assert r.fixed_len.tolist() == [-1, -2, -1] and r.nprops.tolist() == [-1, 2, -1]
    assert r.tally.tolist() == [[-1] * 5, [3, 2, 0, 0, 0], [-1] * 5]
    assert r.proposals(0) is None and r.fixed_seq(0) is None
    assert (r.fixed == 255).all() and (r.prop_kind[:3] == 255).all() and (r.prop_kind[3:5] == INS).all()
    assert _lib.host_shift_fix([], [], []).n == 0


# ---------------------------------------------------------------------
# 3. pairalign over a stand-in engine
# ---------------------------------------------------------------------
class ShiftStandIn(StandInEngine):
    """StandInEngine with pair_shifts: the oracle's moves fed to host_shift_fix."""

    def __init__(self):
        super().__init__()
        self.uploads, self.shift_calls = [], []

    def set_sequences(self, first, seqs):
        self.uploads.append(len(seqs))
        super().set_sequences(first, seqs)

    def pair_shifts(self, seqs, tpls, bws, flags=0, want_fixed=True, want_proposals=False, prop_cap=None, caps=None):
        sc, moves, _ = self.pair_align(seqs, tpls, bws, flags, caps=caps)
        si, ti = np.broadcast_arrays(np.asarray(seqs), np.asarray(tpls))
        self.shift_calls.append((self.calls.pop(), want_fixed, want_proposals))
        r = _lib.host_shift_fix(moves, [self.seqs[int(i)].seq for i in si.reshape(-1)],
                                [self.tpls[int(j)] for j in ti.reshape(-1)], want_fixed, want_proposals, prop_cap)
        return sc, r


def strs(seqs):
    return [dna_str(g) for g in seqs]


def test_wrappers_kats_and_moves_path():
    cons = [DNASeq(c) for c, _, _ in SHIFT_KATS]
    refs = [DNASeq(r) for _, r, _ in SHIFT_KATS]
    e, old = ShiftStandIn(), StandInEngine()
    got = pairalign.correct_shifts_many(cons, refs, engine=e)
    assert strs(got) == [x for _, _, x in SHIFT_KATS]
    assert strs(pairalign.correct_shifts_many(cons, refs, engine=old)) == strs(got)
    assert len(e.shift_calls) == 1 and e.calls == []
    (si, ti, bws, flags), want_fixed, want_props = e.shift_calls[0]
    assert flags == RF_SKEW and want_fixed and not want_props
    assert bws == old.calls[0][2] and (si, ti) == ([0, 1, 2, 3], [0, 1, 2, 3])
    props = pairalign.single_indel_proposals_many(cons, refs, engine=e)
    assert props == pairalign.single_indel_proposals_many(cons, refs, engine=old)
    assert [len(p) for p in props] == [1, 1, 1, 0] and props[0][0].kind == DEL and props[1][0].kind == INS
    assert e.shift_calls[-1][1:] == (False, True)
    assert [apply_proposals(c, p).tolist() for c, p in zip(cons, props)] == [g.tolist() for g in got]


def test_wrappers_random_pairs_equal_moves_path():
    seqs, tpls, _ = sweep_pairs()
    refs = [s.seq for s in seqs[:40]]
    cons = tpls[:40]
    e, old = ShiftStandIn(), StandInEngine()
    kw = dict(bandwidth=9, scores=NOCODON_SCORES)
    props = pairalign.single_indel_proposals_many(cons, refs, engine=e, **kw)
    assert props == pairalign.single_indel_proposals_many(cons, refs, engine=old, **kw)
    clear = [k for k, p in enumerate(props) if len({q.pos for q in p if q.kind == INS}) == sum(q.kind == INS for q in p)]
    assert 10 < len(clear) < 40
    a = pairalign.correct_shifts_many([cons[k] for k in clear], [refs[k] for k in clear], engine=e, **kw)
    b = pairalign.correct_shifts_many([cons[k] for k in clear], [refs[k] for k in clear], engine=old, **kw)
    assert [x.tolist() for x in a] == [x.tolist() for x in b]
    for eng in (e, old):
        with pytest.raises(AmbiguousProposalsError):
            pairalign.correct_shifts_many(cons, refs, engine=eng, **kw)
    rs = [RifrafSequence(r, np.full(len(r), -1.0), 9, NOCODON_SCORES) for r in refs]
    has = pairalign.has_single_indels_many(cons, rs, engine=e)
    assert has.dtype == bool and has.tolist() == pairalign.has_single_indels_many(cons, rs, engine=old).tolist()
    assert has.any() and not has.all()
    assert e.shift_calls[-1][0][3] == 0 and e.shift_calls[-1][1:] == (False, False)   # unskewed, tallies alone
    assert pairalign.has_single_indels_many(cons, rs, bandwidth=12, engine=e).tolist() == \
        pairalign.has_single_indels_many(cons, rs, bandwidth=12, engine=old).tolist()
    assert e.shift_calls[-1][0][2] == [12] * 40


def test_one_shared_reference_is_uploaded_once():
    e = ShiftStandIn()
    cons = [DNASeq("TTTACCC"), DNASeq("TTTAAACCC"), DNASeq("TTTCCC"), DNASeq("TTTTTTACCCTT")]
    one = pairalign.correct_shifts_many(cons, DNASeq("TTTCGC"), engine=e)
    assert strs(one)[:3] == ["TTTCCC", "TTTAAACCC", "TTTCCC"]
    assert e.uploads == [1] and len(e.seqs) == 1
    (si, ti, bws, _), _, _ = e.shift_calls[0]
    assert si == [0, 0, 0, 0] and ti == [0, 1, 2, 3]
    assert bws == [1, 1, 1, 1]                    # ceil(min(len(c), len(r)) * 0.1), per pair, beside the pair
    long_ref = DNASeq("ACGT" * 6)
    pairalign.correct_shifts_many([DNASeq("ACGT" * 3), DNASeq("ACGT" * 6)], long_ref, engine=e)
    assert e.shift_calls[-1][0][2] == [2, 3] and e.uploads == [1, 1]
    each = pairalign.correct_shifts_many(cons, [DNASeq("TTTCGC")] * 4, bandwidth=2, engine=e)
    assert strs(each) == strs(one) and e.uploads[-1] == 4 and e.shift_calls[-1][0][2] == [2] * 4
    assert strs(pairalign.correct_shifts_many(cons, "TTTCGC", engine=e)) == strs(one)
    assert strs(one) == strs(pairalign.correct_shifts_many(cons, "TTTCGC", engine=StandInEngine()))
    with pytest.raises(ValueError):
        pairalign.correct_shifts_many(cons, [DNASeq("TTT")] * 2, engine=e)
    assert pairalign.correct_shifts_many([], "TTT", engine=e) == []
    has = pairalign.has_single_indels_many(cons, RifrafSequence(DNASeq("TTTCGC"), np.full(6, -1.0), 2, SHIFT_SCORES),
                                           engine=e)
    assert e.uploads[-1] == 1 and e.shift_calls[-1][0][0] == [0] * 4 and len(has) == 4


def invalid_reference(n):
    """A reference no consensus aligns to: every way through its tables is -Inf."""
    bad = RifrafSequence(np.zeros(n, np.uint8), np.full(n, -1.0), 3, SHIFT_SCORES)
    bad.mismatch_scores = bad.ins_scores = np.full(n, -np.inf)
    bad.del_scores = np.full(n + 1, -np.inf)
    bad.codon_ins_scores = np.full(len(bad.codon_ins_scores), -np.inf)
    bad.codon_del_scores = np.full(len(bad.codon_del_scores), -np.inf)
    return bad


def test_first_failing_pair_raises():
    ambiguous, fine = DNASeq("ACGTACTTGCATG"), DNASeq("ACGTACAGTTGCATG")
    ref = DNASeq("ACGTACAGTTGCATG")     # `ambiguous` lacks "AG": two inserts at one position
    for e in (ShiftStandIn(), StandInEngine()):
        with pytest.raises(AmbiguousProposalsError):
            pairalign.correct_shifts_many([fine, ambiguous, fine], ref, bandwidth=3, scores=NOCODON_SCORES, engine=e)
        # single_indel_proposals does not fail on them
        props = pairalign.single_indel_proposals_many([fine, ambiguous], ref, bandwidth=3, scores=NOCODON_SCORES,
                                                      engine=e)
        assert props[0] == [] and [p.kind for p in props[1]] == [INS, INS] and props[1][0].pos == props[1][1].pos
    bad = invalid_reference(9)
    cons = [DNASeq("CCCCCCCCC")] * 3
    e = ShiftStandIn()
    e.set_sequences(0, [bad, RifrafSequence(ref, np.full(len(ref), -1.0), 3, NOCODON_SCORES)])
    e.set_templates(0, [cons[0], ambiguous, fine])
    _, res = e.pair_shifts([1, 0, 1], [1, 0, 2], 3, RF_SKEW)
    assert res.fixed_len.tolist()[:2] == [-2, -1] and res.fixed_len[2] == len(fine)
    with pytest.raises(AmbiguousProposalsError):
        pairalign._raise_failed(res, True)
    with pytest.raises(RifrafError, match="pair 1: new score is invalid"):
        pairalign._raise_failed(res, False)
    _, res = e.pair_shifts([0, 1, 1], [0, 1, 2], 3, RF_SKEW)
    with pytest.raises(RifrafError, match="pair 0: new score is invalid"):
        pairalign._raise_failed(res, True)


def test_package_exports():
    import rifraf_amd
    for name in ("single_indel_proposals_many", "has_single_indels_many", "correct_shifts_many"):
        assert getattr(rifraf_amd, name) is getattr(pairalign, name)
    assert rifraf_amd.host_shift_fix is _lib.host_shift_fix


# ---------------------------------------------------------------------
# 4. the GPU sweep's pairs
# ---------------------------------------------------------------------
SWEEP_BW = 9
N_SPECIAL = 20


def edit_consensus(ref, rng, kinds):
    """ref with one edit of each kind of `kinds`, at sites at least 10 apart,
    applied from the right so the sites stay where they were chosen."""
    n = len(ref)
    sites = np.arange(6, n - 8, 10)
    rng.shuffle(sites)
    cons = list(ref)
    for kind, at in sorted(zip(kinds, sites.tolist()), key=lambda x: -x[1]):
        if kind == "sub":
            cons[at] = (cons[at] + 1 + int(rng.integers(0, 3))) % 4
        elif kind == "ins1":       # the consensus has a base more: a deletion
            cons.insert(at, int(rng.integers(0, 4)))
        elif kind == "del1":       # a base fewer: an insertion
            del cons[at]
        elif kind == "del2":       # two fewer: two insertions at one position, or a codon insertion and a deletion
            del cons[at:at + 2]
        elif kind == "ins3":
            cons[at:at] = rng.integers(0, 4, 3).tolist()
        elif kind == "del3":
            del cons[at:at + 3]
        elif kind == "first":      # the first base is missing: Insertion(0, .)
            pass
    if "first" in kinds:
        del cons[0]
    return np.array(cons, np.uint8)


def sweep_pairs():
    """The GPU sweep's pairs: about 300, fixed seed.  References of 30..200
    bases with correct_shifts' tables (constant log p, SHIFT_SCORES), each
    consensus its reference with random substitutions, single insertions and
    deletions, runs of two missing bases and inserted or removed 3-base
    blocks; then N_SPECIAL pairs whose mismatch and codon tables are -Inf and
    N_SPECIAL whose codon tables are (module docstring).  Bandwidth SWEEP_BW.  -> (sequences, templates,
    what was done to each)."""
    rng = np.random.default_rng(3102)
    seqs, tpls, what = [], [], []
    kinds_all = ("sub", "ins1", "del1", "del2", "ins3", "del3", "first")
    for k in range(262):
        if k < 3 * len(EDGE_COUNTS):     # substitutions alone: the move count is the length
            n = EDGE_COUNTS[k % len(EDGE_COUNTS)]
            kinds = ["sub"] * (k // len(EDGE_COUNTS))
        else:
            n = int(rng.integers(30, 201))
            room = len(np.arange(6, n - 8, 10))
            kinds = [kinds_all[int(x)] for x in rng.integers(0, len(kinds_all), size=int(rng.integers(0, min(room, 5) + 1)))]
            if k % 4 == 0 and room:
                kinds[:1] = ["del2"]
            if k % 5 == 0:
                kinds = [x for x in kinds if x != "first"] + ["first"]
            kinds = [x for q, x in enumerate(kinds) if x != "first" or q == kinds.index("first")]
        ref = rng.integers(0, 4, n).astype(np.uint8)
        seqs.append(RifrafSequence(ref, np.full(n, -1.0), SWEEP_BW, SHIFT_SCORES))
        tpls.append(edit_consensus(ref, rng, kinds))
        what.append(tuple(kinds))
    for k in range(N_SPECIAL):
        n = int(rng.integers(30, 201))
        ref = rng.integers(0, 4, n).astype(np.uint8)
        s = RifrafSequence(ref, np.full(n, -1.0), SWEEP_BW, SHIFT_SCORES)
        s.mismatch_scores = np.full(n, -np.inf)
        s.codon_ins_scores = np.full(len(s.codon_ins_scores), -np.inf)
        s.codon_del_scores = np.full(len(s.codon_del_scores), -np.inf)
        kinds = ["sub"] * (1 + k % 3) + (["del1"] if k % 2 else [])
        seqs.append(s)
        tpls.append(edit_consensus(ref, rng, kinds))
        what.append(("special",) + tuple(kinds))
    for k in range(N_SPECIAL):    # codon tables -Inf alone: two missing bases are two insertions at one position
        n = int(rng.integers(30, 201))
        ref = rng.integers(0, 4, n).astype(np.uint8)
        s = RifrafSequence(ref, np.full(n, -1.0), SWEEP_BW, SHIFT_SCORES)
        s.codon_ins_scores = np.full(len(s.codon_ins_scores), -np.inf)
        s.codon_del_scores = np.full(len(s.codon_del_scores), -np.inf)
        kinds = ["del2"] + ["sub", "ins1"][:k % 3]
        seqs.append(s)
        tpls.append(edit_consensus(ref, rng, kinds))
        what.append(("special",) + tuple(kinds))
    return seqs, tpls, what


def constructed_pairs():
    """Two kinds of constructed pairs, after test_pair_text.codon_pairs: a
    90-base reference against a consensus with one single-base or 3-base
    edit placed so that the proposal or codon move is move number 62..66,
    and one whose two missing bases make inserts of moves 64 and 65.
    -> (sequences, templates, (move number, code))."""
    rng = np.random.default_rng(3103)
    seqs, tpls, what = [], [], []
    for at in (62, 63, 64, 65, 66):
        for code in (2, 3, 4, 5):
            while True:
                ref = rng.integers(0, 4, 90).astype(np.uint8)
                w = 3 if code >= 4 else 1
                blk = ref[at - 1:at - 1 + w] if code in (2, 4) else (ref[at - 1:at - 1 + w] + 2) % 4
                # the edit cannot slide: it differs from what precedes and follows it at its own distance
                if blk[-1] != ref[at - 2] and blk[0] != (ref[at - 1 + w] if code in (2, 4) else ref[at - 1]):
                    break
            if code in (2, 4):     # the consensus lacks the reference's bases: insert / codon insert
                cons = np.concatenate([ref[:at - 1], ref[at - 1 + w:]])
            else:                  # it has more: delete / codon delete
                cons = np.concatenate([ref[:at - 1], blk, ref[at - 1:]])
            seqs.append(RifrafSequence(ref, np.full(len(ref), -1.0), SWEEP_BW, SHIFT_SCORES))
            tpls.append(cons.astype(np.uint8))
            what.append((at, code))
    # a run of two inserts across moves 64 / 65: codon tables off (-Inf), so two missing bases are two inserts
    while True:
        ref = rng.integers(0, 4, 90).astype(np.uint8)
        if ref[64] != ref[62] and ref[63] != ref[65] and ref[63] != ref[62] and ref[64] != ref[65]:
            break
    s = RifrafSequence(ref, np.full(90, -1.0), SWEEP_BW, SHIFT_SCORES)
    s.codon_ins_scores = np.full(len(s.codon_ins_scores), -np.inf)
    s.codon_del_scores = np.full(len(s.codon_del_scores), -np.inf)
    seqs.append(s)
    tpls.append(np.concatenate([ref[:63], ref[65:]]).astype(np.uint8))
    what.append((64, 22))
    return seqs, tpls, what


def oracle_moves_many(seqs, tpls, bw, flags):
    e = StandInEngine()
    e.set_sequences(0, seqs)
    e.set_templates(0, tpls)
    k = np.arange(len(seqs))
    return e.pair_align(k, k, bw, flags)[1]


def sweep_coverage(moves, seqs, tpls):
    """The sweep's coverage conditions over one run's moves (None: a failed pair)."""
    ok = [k for k, mv in enumerate(moves) if mv is not None]
    r = _lib.host_shift_fix(moves, [s.seq for s in seqs], tpls)
    props = [r.proposals(k) for k in ok]
    ambiguous = int((r.fixed_len == -2).sum())
    ins0 = sum(any(p.kind == INS and p.pos == 0 for p in ps) for ps in props)
    both = sum(bool({p.pos for p in ps if p.kind == INS} & {p.pos for p in ps if p.kind == DEL}) for ps in props)
    codes = {int(c) for k in ok for c in moves[k]}
    counts = {len(moves[k]) for k in ok}
    return dict(ambiguous=ambiguous, ins0=ins0, both=both, codes=codes, counts=counts)


def assert_sweep_coverage(cov):
    assert cov["ambiguous"] >= 10, cov["ambiguous"]
    assert cov["ins0"] >= 10, cov["ins0"]
    assert cov["both"] >= 10, cov["both"]
    assert cov["codes"] == {1, 2, 3, 4, 5}, cov["codes"]
    assert set(EDGE_COUNTS) <= cov["counts"], sorted(set(EDGE_COUNTS) - cov["counts"])


def assert_constructed(moves, what):
    for mv, (at, code) in zip(moves, what):
        if code == 22:
            assert mv[at - 1] == 2 and mv[at] == 2, (at, mv[at - 4:at + 4])
        else:
            assert mv[at - 1] == code, (at, code, mv[at - 5:at + 4])
    assert {at for at, _ in what} >= {62, 63, 64, 65, 66}


def test_sweep_generator_conditions():
    seqs, tpls, what = sweep_pairs()
    assert 290 <= len(seqs) <= 310
    assert all(30 <= len(s) <= 200 for s in seqs)
    moves = oracle_moves_many(seqs, tpls, SWEEP_BW, RF_SKEW)
    assert all(mv is not None for mv in moves)
    assert_sweep_coverage(sweep_coverage(moves, seqs, tpls))
    check_against_python(_lib.host_shift_fix(moves, [s.seq for s in seqs], tpls), moves, [s.seq for s in seqs], tpls, what)
    for flags in (0, RF_SKEW | RF_TRIM):
        other = oracle_moves_many(seqs, tpls, SWEEP_BW, flags)
        assert sweep_coverage(other, seqs, tpls)["codes"] == {1, 2, 3, 4, 5}
    cs, ct, cw = constructed_pairs()
    cm = oracle_moves_many(cs, ct, SWEEP_BW, RF_SKEW)
    assert_constructed(cm, cw)
    r = _lib.host_shift_fix(cm, [s.seq for s in cs], ct)
    assert r.fixed_len[-1] == -2 and r.nprops[-1] == 2
