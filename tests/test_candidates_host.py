"""Candidate selection over a dense table on the host (rf_host_candidates,
csrc/rifraf_candidates.h) against a direct restatement with the host paths
that decide today: all_proposals / mask_to_proposals for the proposals and
their order, the `total > score` filter of get_candidates, and
proposals.choose_candidates.  Everything is compared exactly: kinds,
positions, bases, score bits, order and counts.  No GPU."""
import numpy as np
import pytest

from rifraf_amd import _lib
from rifraf_amd.model import Stage, all_proposals, mask_to_proposals
from rifraf_amd.proposals import DEL, INS, SUB, Proposal, ScoredProposal, choose_candidates

SOURCES = (0, 1, 2, 3, 4)
MS = (1, 2, 6, 7, 27, 28, 70)   # 9 (m + 1) slots: 18, 27, 63, 72, 252, 261, 639 -- either side of 64 and 256


def slot_of(p):
    return p.base if p.kind == SUB else 4 if p.kind == DEL else 5 + p.base


def proposals_of(cons, mask, source):
    """The proposal list of one group under `source`, in today's order."""
    cons = np.asarray(cons, np.uint8)

    def legal(p):   # what no source proposes, whatever a mask says
        if p.kind != INS and p.pos == 0:
            return False
        return not (p.kind == SUB and cons[p.pos - 1] == p.base)

    if source == 0:
        return all_proposals(Stage.INIT, cons, False)
    if source == 3:
        return all_proposals(Stage.REFINE, cons, False)
    if source == 4:   # the mask picks from all_proposals, in its order
        return [p for p in all_proposals(Stage.INIT, cons, False) if mask[p.pos, slot_of(p)]]
    props = [p for p in mask_to_proposals(mask) if legal(p)]
    return props if source == 1 else [p for p in props if p.kind == SUB]


def restate(cons, table, mask, score, source, min_dist):
    """(candidates, chosen) of one group; ArithmeticError for a NaN proposal."""
    cands = []
    for p in proposals_of(cons, mask, source):
        tot = float(table[p.pos, slot_of(p)])
        if tot != tot:
            raise ArithmeticError("failed to compute a valid score")
        if tot > score:
            cands.append(ScoredProposal(p, tot))
    return cands, choose_candidates(cands, min_dist)


def same(got, exp):
    """ScoredProposal lists equal, the scores bit for bit."""
    assert [c.proposal for c in got] == [c.proposal for c in exp]
    assert np.array([c.score for c in got]).tobytes() == np.array([c.score for c in exp]).tobytes()


def random_group(rng, m, pool=True):
    """A consensus, a table and a mask; pool: scores from a few values, so
    equal totals across kinds and neighbouring positions are the rule."""
    cons = rng.integers(0, 4, m).astype(np.uint8)
    if pool:
        table = rng.choice([-2.0, -0.5, -0.0, 0.0, 0.25, 0.5, 0.5, 1.0, 3.0, np.inf], (m + 1, 9))
    else:
        table = rng.normal(0.0, 1.0, (m + 1, 9))
    mask = (rng.random((m + 1, 9)) < 0.4).astype(np.uint8)
    return cons, table, mask


def check_groups(run, groups, scores, sources, min_dist):
    """run(...) (rf_host_candidates, or the device call in
    tests/test_candidates.py) equals the restatement for every group."""
    got = run([g[0] for g in groups], [g[1] for g in groups], scores, sources, min_dist,
              masks=[g[2] for g in groups], with_counts=True)
    for (cons, table, mask), sc, src, (cands, chosen, ncand, nchosen) in zip(groups, scores, sources, got):
        ec, eh = restate(cons, table, mask, sc, src, min_dist)
        same(cands, ec)
        same(chosen, eh)
        assert (ncand, nchosen) == (len(ec), len(eh))


def min_dists(m):
    return (0, 1, 3, 15, m + 1)


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("m", MS)
def test_random_tables(m, source):
    rng = np.random.default_rng(1000 * m + source)
    for pool in (True, False):
        grp = random_group(rng, m, pool)
        for md in min_dists(m):
            check_groups(_lib.host_candidates, [grp], [0.0], [source], md)


# ---------------------------------------------------------------- hand-made

def flat_group(m, fill=-1.0):
    """Consensus of A's, every total `fill`, every mask byte set."""
    return np.zeros(m, np.uint8), np.full((m + 1, 9), fill), np.ones((m + 1, 9), np.uint8)


def tie_cases():
    """(name, group, score, source, min_dist, expected chosen proposals)."""
    cases = []
    # one position, three kinds at one score: the within-position order decides
    cons, table, mask = flat_group(6)
    table[3, [1, 4, 5]] = 2.0   # Sub(3, C), Del(3), Ins(3, A)
    sub, dele, ins = Proposal(SUB, 3, 1), Proposal(DEL, 3, 0), Proposal(INS, 3, 0)
    for src, order in ((0, [sub, dele, ins]), (4, [sub, dele, ins]), (1, [sub, ins, dele])):
        cases.append((f"kinds_src{src}_all", (cons, table, mask), 0.0, src, 0, order))
        cases.append((f"kinds_src{src}_one", (cons, table, mask), 0.0, src, 1, order[:1]))
    # a deletion and an insertion tie, the substitution is out: Del first in
    # all_proposals' order, Ins first in the mask's
    cons, table, mask = flat_group(6)
    table[2, [4, 7]] = 1.5      # Del(2), Ins(2, G)
    dele, ins = Proposal(DEL, 2, 0), Proposal(INS, 2, 2)
    cases.append(("del_ins_src0", (cons, table, mask), 0.0, 0, 1, [dele]))
    cases.append(("del_ins_src1", (cons, table, mask), 0.0, 1, 1, [ins]))
    # equal scores at positions closer than min_dist: the earlier position
    # wins and shadows the later; a better score further on wins over both
    cons, table, mask = flat_group(12)
    table[4, 4] = table[5, 4] = table[6, 4] = 1.0
    table[10, 2] = 1.0
    for src in (0, 1):
        cases.append((f"near_src{src}", (cons, table, mask), 0.0, src, 3,
                      [Proposal(DEL, 4, 0), Proposal(SUB, 10, 2)]))
        cases.append((f"near_src{src}_md2", (cons, table, mask), 0.0, src, 2,
                      [Proposal(DEL, 4, 0), Proposal(DEL, 6, 0), Proposal(SUB, 10, 2)]))
    cons, table, mask = flat_group(12)
    table[4, 4] = table[6, 4] = 1.0
    table[5, 5] = 2.0           # Ins(5, A) beats both neighbours and shadows them
    cases.append(("near_better", (cons, table, mask), 0.0, 0, 2, [Proposal(INS, 5, 0)]))
    # Ins(0, b) sorts before position 1; -0.0 and 0.0 are one score
    cons, table, mask = flat_group(3, fill=-5.0)
    table[0, 8] = 0.0
    table[1, 1] = -0.0
    cases.append(("ins0_first", (cons, table, mask), -1.0, 0, 0, [Proposal(INS, 0, 3), Proposal(SUB, 1, 1)]))
    return cases


TIES = tie_cases()


@pytest.mark.parametrize("case", TIES, ids=[c[0] for c in TIES])
def test_ties(case):
    _, grp, score, src, md, exp = case
    check_groups(_lib.host_candidates, [grp], [score], [src], md)
    (_, chosen), = _lib.host_candidates([grp[0]], [grp[1]], [score], [src], md, masks=[grp[2]])
    assert [c.proposal for c in chosen] == exp


def extreme_cases():
    """(name, groups, scores, sources, min_dist, expected (ncand, nchosen) per group)."""
    m = 28
    every = flat_group(m, fill=1.0)
    none = flat_group(m, fill=-1.0)
    equal = flat_group(m, fill=0.0)   # total == score everywhere
    out = [("every_md0", [every], [0.0], [0], 0, [(8 * m + 4, 8 * m + 4)]),
           ("every_md1", [every], [0.0], [0], 1, [(8 * m + 4, m + 1)]),
           ("every_subs", [every], [0.0], [3], 1, [(3 * m, m)]),
           ("every_aln_subs", [every], [0.0], [2], 4, [(3 * m, (m + 3) // 4)]),
           ("none", [none] * 2, [0.0, 0.0], [0, 1], 3, [(0, 0)] * 2),
           ("equal", [equal] * 3, [0.0, -0.0, 0.0], [0, 1, 4], 0, [(0, 0)] * 3),
           ("nan_score", [every], [np.nan], [0], 0, [(0, 0)])]
    return out


EXTREMES = extreme_cases()


@pytest.mark.parametrize("case", EXTREMES, ids=[c[0] for c in EXTREMES])
def test_extremes(case):
    _, groups, scores, sources, md, counts = case
    check_groups(_lib.host_candidates, groups, scores, sources, md)
    got = _lib.host_candidates([g[0] for g in groups], [g[1] for g in groups], scores, sources, md,
                               masks=[g[2] for g in groups], with_counts=True)
    assert [(r[2], r[3]) for r in got] == counts


def nan_cases():
    """(name, group, source, is the NaN in a proposal slot?)"""
    m = 7
    rng = np.random.default_rng(77)
    cons, table, mask = random_group(rng, m, pool=False)
    cons[:] = [0, 1, 2, 3, 0, 1, 2]
    mask[:] = 1
    cases = []

    def with_nan(p, k, mask_bit=1):
        t, k_ = table.copy(), mask.copy()
        t[p, k] = np.nan
        k_[p, k] = mask_bit
        return cons, t, k_

    for src in SOURCES:
        cases.append((f"own_base_src{src}", with_nan(3, 2), src, False))    # Sub(3, G) over G
        cases.append((f"p0_sub_src{src}", with_nan(0, 1), src, False))
        cases.append((f"p0_del_src{src}", with_nan(0, 4), src, False))
    for src in (1, 2, 4):
        cases.append((f"masked_out_src{src}", with_nan(4, 1, mask_bit=0), src, False))
    cases.append(("indel_src2", with_nan(4, 6), 2, False))   # substitutions only
    cases.append(("indel_src3", with_nan(4, 4), 3, False))
    for src in SOURCES:
        cases.append((f"sub_src{src}", with_nan(4, 1), src, True))           # Sub(4, C) over T
    for src in (0, 1, 4):
        cases.append((f"del_src{src}", with_nan(7, 4), src, True))
        cases.append((f"ins0_src{src}", with_nan(0, 5), src, True))
    return cases


NANS = nan_cases()


@pytest.mark.parametrize("case", NANS, ids=[c[0] for c in NANS])
def test_nan_slots(case):
    """NaN where no proposal is: ignored.  NaN in a proposal slot: the call
    fails as rf_score fails for a list with that proposal, above the score or
    not."""
    _, grp, src, fatal = case
    if not fatal:
        check_groups(_lib.host_candidates, [grp], [0.0], [src], 2)
        return
    for score in (0.0, np.inf):
        with pytest.raises(ArithmeticError):
            restate(*grp, score, src, 2)
        with pytest.raises(ArithmeticError, match="failed to compute a valid score"):
            _lib.host_candidates([grp[0]], [grp[1]], [score], [src], 2, masks=[grp[2]])


def capacity_case():
    rng = np.random.default_rng(5)
    groups = [random_group(rng, m) for m in (6, 28)]
    return groups, [0.0, 0.25], [0, 1], 2


@pytest.mark.parametrize("short", ("zero", "exact", "one_short", "counts_only", "chosen_only"))
def test_capacities(short, run=None):
    """The counts stay true whatever the room; the arrays hold the prefix."""
    run = run or _lib.host_candidates
    groups, scores, sources, md = capacity_case()
    exp = [restate(*g, sc, src, md) for g, sc, src in zip(groups, scores, sources)]
    assert all(len(c) > 1 and len(h) > 1 for c, h in exp)
    nc, nh = [len(c) for c, _ in exp], [len(h) for _, h in exp]
    caps = {"zero": ([0, 0], [0, 0]), "exact": (nc, nh), "one_short": ([n - 1 for n in nc], [n - 1 for n in nh]),
            "counts_only": (False, False), "chosen_only": (False, nh)}[short]
    got = run([g[0] for g in groups], [g[1] for g in groups], scores, sources, md, masks=[g[2] for g in groups],
              cand_cap=caps[0], chosen_cap=caps[1], with_counts=True)
    for g, ((ec, eh), (cands, chosen, ncand, nchosen)) in enumerate(zip(exp, got)):
        assert (ncand, nchosen) == (len(ec), len(eh))
        for lst, full, cap in ((cands, ec, caps[0]), (chosen, eh, caps[1])):
            if cap is False:
                assert lst is None
            else:
                same(lst, full[:cap[g]])


def several_groups():
    rng = np.random.default_rng(31)
    groups = [random_group(rng, m) for m in (7, 1, 70, 27, 2)]
    groups[3] = (groups[3][0], groups[3][1], np.zeros((28, 9), np.uint8))   # nothing proposed
    return groups, [0.0, 0.25, 0.5, 0.0, -1.0], [1, 0, 4, 1, 3]


@pytest.mark.parametrize("md", (0, 3))
def test_several_groups(md):
    groups, scores, sources = several_groups()
    check_groups(_lib.host_candidates, groups, scores, sources, md)
    got = _lib.host_candidates([g[0] for g in groups], [g[1] for g in groups], scores, sources, md,
                               masks=[g[2] for g in groups], with_counts=True)
    assert got[3] == ([], [], 0, 0)


def test_bad_arguments():
    cons, table, mask = flat_group(3)
    with pytest.raises(ValueError):
        _lib.host_candidates([cons], [table], [0.0], [5], 1, masks=[mask])     # unknown source
    with pytest.raises(ValueError):
        _lib.host_candidates([cons], [table], [0.0], [1], 1)                   # source 1 without a mask
    assert _lib.host_candidates([], [], [], [], 1) == []
