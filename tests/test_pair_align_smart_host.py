"""Band doubling over pairs without a GPU: the restatement of
smart_forward_moves! (src/model.jl:643-672) that test_pair_align_smart.py
expects the engine to match (oracle_smart), pinned here against
model.smart_forward_moves driven by tests/oracle_engine.py; the Python
pre-check of the band at the largest bandwidth; and the pair / threshold /
fixed plumbing of pairalign.smart_* and assign.cross_scores over a stand-in
engine whose pair_align_smart is oracle_smart.

The helpers of this file (oracle_align, oracle_smart, indel_read, smart_set)
are shared with test_pair_align_smart.py and test_pair_walk_wave.py."""
import copy
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import oracle
from _util import REF_SCORES, SEQ_SCORES, make_read, random_seq
from oracle_engine import OracleEngine
from rifraf_amd import RifrafSequence, assign, model, pairalign
from rifraf_amd.align import moves_to_aligned_seqs
from rifraf_amd.engine import RF_SKEW, RF_TRIM, RifrafError
from rifraf_amd.poisson import cquantile_poisson, cquantile_poisson_many

ALWAYS, NEVER = -1.0, 1e9   # thresholds every count is above / none is


def oracle_align(t, s, bw, skew=False, trim=False):
    """(A[end, end], moves, count_errors) of one pair from the oracle."""
    A, mv = oracle.forward(t, s, moves=True, skew=skew, trim=trim, bandwidth=bw)
    n, m = len(s.seq), len(t)
    w = oracle.backtrace(mv, n + 1, m + 1, bw)
    return A[n - m + max(m - n, 0) + bw, m], w, oracle.count_errors(w, t, s.seq)


def oracle_smart(t, s, bw, thr, fixed, max_doublings=5, memo=None, key=None):
    """smart_forward_moves! (model.jl:643-672) of one pair with forward_moves!
    and count_errors from the oracle.  -> SimpleNamespace(score, moves, nerr,
    bw, rounds, why): the last fill's results, the final bandwidth, the number
    of fills and why the loop stopped -- "fixed", "max" (bw >= max_bandwidth;
    `cap` says which term of min(bw 2^k, m, n) that was), "below" (n_errors <=
    threshold), "stalled" (n_errors >= old_n_errors) or "invalid" (the fill
    raised: score NaN, no moves, -1)."""
    n, m = len(s.seq), len(t)
    grown = bw << max_doublings
    max_bw = bw if fixed else min(grown, m, n)                      # :648-651
    cap = "pow" if grown <= min(m, n) else ("m" if m <= n else "n")
    n_err = old = sys.maxsize
    rounds = 0
    while True:
        rounds += 1
        try:
            if memo is not None and (key, bw) in memo:
                score, mv, ne = memo[key, bw]
            else:
                score, mv, ne = oracle_align(t, s, bw)               # :655
                if memo is not None:
                    memo[key, bw] = (score, mv, ne)
        except oracle.OracleError:
            return SimpleNamespace(score=np.nan, moves=None, nerr=-1, bw=bw, rounds=rounds, why="invalid", cap=cap)
        if fixed or bw >= max_bw:                                    # :656-658
            why = "fixed" if fixed else "max"
            break
        old, n_err = n_err, ne                                       # :659-660
        if n_err > thr and n_err < old:                              # :662
            bw = min(bw * 2, max_bw)
        else:
            why = "below" if n_err <= thr else "stalled"
            break
    return SimpleNamespace(score=score, moves=mv, nerr=ne, bw=bw, rounds=rounds, why=why, cap=cap)


def indel_read(t, rng, bw, scores, width, rate=0.03):
    """A read of template t with a few point errors, one block insertion and
    one block deletion of `width` bases (the alignment leaves the main
    diagonal by `width` and comes back, so a band below `width` misses it)."""
    r = make_read(t, rng, rate, bw, scores)
    s = r.seq
    a = int(rng.integers(len(s) // 8, len(s) // 3))
    b = int(rng.integers(len(s) // 2, len(s) - width - 2))
    s = np.concatenate([s[:a], random_seq(width, rng), s[a:b], s[b + width:]]).astype(np.uint8)
    return RifrafSequence(s, np.log10(rng.uniform(0.01, 0.3, len(s))), bw, scores)


def smart_set(seed=2401, npairs=40):
    """The pairs of the doubling tests: m 60-400, starting bandwidths 2-9,
    lean and codon reads with a block insertion and a block deletion wider
    than the starting band; then short pairs whose largest bandwidth is m or
    n.  -> (seqs, templates, starting bandwidths, fixed)."""
    rng = np.random.default_rng(seed)
    seqs, tpls, bws, fixed = [], [], [], []
    for k in range(npairs):
        m = int(rng.integers(60, 401))
        bw = 2 + k % 8
        scores = REF_SCORES if k % 3 == 2 else SEQ_SCORES
        t = random_seq(m, rng)
        seqs.append(indel_read(t, rng, bw, scores, int(rng.integers(bw + 1, 2 * bw + 2))))
        tpls.append(t)
        bws.append(bw)
        fixed.append(k % 7 == 6)
    for n, m in ((20, 12), (12, 20), (13, 13), (30, 11)):
        t = random_seq(m, rng)
        seqs.append(RifrafSequence(random_seq(n, rng), np.log10(rng.uniform(0.01, 0.3, n)), 9, SEQ_SCORES))
        tpls.append(t)
        bws.append(9)
        fixed.append(False)
    return seqs, tpls, np.array(bws, np.int32), np.array(fixed, bool)


def poisson_thresholds(seqs, pvalue=0.1):
    return np.asarray(cquantile_poisson_many([s.est_n_errors for s in seqs], pvalue), np.float64)


# ---------------------------------------------------------------------
# 1. oracle_smart is model.smart_forward_moves
# ---------------------------------------------------------------------
def slot_smart(engine, t, s, pvalue, fixed):
    """model.smart_forward_moves (rf_realign + rf_backtrace in slot 0) of one
    pair -> (final bandwidth, A[end, end], count_errors of the final fill)."""
    s = copy.copy(s)
    s.bandwidth_fixed = bool(fixed)
    engine.set_sequences(0, [s])
    engine.set_templates(0, [t])
    score = model.smart_forward_moves(SimpleNamespace(e=engine), [(0, 0)], [s], len(t), pvalue)[0]
    assert s.bandwidth_fixed
    _, nerr = engine.backtrace(np.array([0], np.int32), want_moves=False)
    return s.bandwidth, score, int(nerr[0])


def dozen():
    seqs, tpls, bws, fixed = smart_set()
    pick = [0, 1, 2, 5, 6, 8, 13, 17, 23, 40, 41, 43]
    return [(tpls[k], seqs[k], int(bws[k]), bool(fixed[k])) for k in pick]


def test_oracle_smart_is_the_model_loop():
    e = OracleEngine()
    rounds = set()
    for pvalue in (0.1, 0.999999):
        for t, s, bw, fx in dozen():
            assert s.bandwidth == bw
            exp = oracle_smart(t, s, bw, cquantile_poisson(s.est_n_errors, pvalue), fx)
            got = slot_smart(e, t, s, pvalue, fx)
            assert got[0] == exp.bw and got[2] == exp.nerr
            assert np.float64(got[1]).view(np.int64) == np.float64(exp.score).view(np.int64)
            assert s.bandwidth == bw and not s.bandwidth_fixed   # the caller's sequence is a copy's source
            rounds.add(exp.rounds)
    assert {1, 2} <= rounds and max(rounds) >= 3, rounds


# ---------------------------------------------------------------------
# 2. the stand-in engine and the plumbing
# ---------------------------------------------------------------------
class StandInEngine:
    """set_sequences / set_templates / pair_scores / pair_align_smart of
    rifraf_amd.engine.Engine on the oracle; records the calls."""

    def __init__(self):
        self.seqs, self.tpls, self.calls = {}, {}, []

    def set_sequences(self, first, seqs):
        for k, s in enumerate(seqs):
            self.seqs[first + k] = s

    def set_templates(self, first, tpls):
        for k, t in enumerate(tpls):
            self.tpls[first + k] = np.asarray(t, np.uint8)

    def pair_scores(self, seqs, tpls, bws, flags=0):
        seqs, tpls, bws = np.broadcast_arrays(np.asarray(seqs), np.asarray(tpls), np.asarray(bws))
        self.calls.append(("scores", seqs.shape))
        out = [oracle_align(self.tpls[int(j)], self.seqs[int(i)], int(bw))[0]
               for i, j, bw in zip(seqs.reshape(-1), tpls.reshape(-1), bws.reshape(-1))]
        return np.array(out).reshape(seqs.shape)

    def pair_align_smart(self, seqs, tpls, bws, thresholds, fixed=None, max_doublings=5, flags=0, want_moves=True,
                         caps=None):
        if fixed is None:
            fixed = False
        seqs, tpls, bws, thr, fixed = (x.reshape(-1) for x in np.broadcast_arrays(
            np.asarray(seqs), np.asarray(tpls), np.asarray(bws), np.asarray(thresholds, float), np.asarray(fixed)))
        self.calls.append(("smart", seqs.tolist(), tpls.tolist(), bws.tolist(), thr.tolist(), fixed.tolist(),
                           max_doublings, flags, want_moves))
        res = [oracle_smart(self.tpls[int(j)], self.seqs[int(i)], int(bw), float(th), bool(fx), max_doublings)
               for i, j, bw, th, fx in zip(seqs, tpls, bws, thr, fixed)]
        if caps is not None:
            for r, i, j, cap in zip(res, seqs, tpls, np.asarray(caps).reshape(-1)):
                assert cap == len(self.seqs[int(i)]) + len(self.tpls[int(j)])
        return (np.array([r.score for r in res]), ([r.moves for r in res] if want_moves else None),
                np.array([r.nerr for r in res], np.int32), np.array([r.bw for r in res], np.int32),
                np.array([r.rounds for r in res], np.int32))


@pytest.fixture
def data():
    rng = np.random.default_rng(2402)
    tpls = [random_seq(m, rng) for m in (90, 120, 75)]
    seqs = [indel_read(tpls[k], rng, 3 + k, SEQ_SCORES, 5 + k) for k in range(3)]
    seqs[1].bandwidth_fixed = True
    return tpls, seqs


def test_default_pairs_thresholds_and_fixed(data):
    tpls, seqs = data
    e = StandInEngine()
    moves, out_bw = pairalign.smart_align_moves_many(seqs, tpls, engine=e)
    thr = [cquantile_poisson(s.est_n_errors, 0.1) for s in seqs]   # RifrafParams().bandwidth_pvalue
    assert model.RifrafParams().bandwidth_pvalue == pairalign.BANDWIDTH_PVALUE == 0.1
    assert e.calls == [("smart", [0, 1, 2], [0, 1, 2], [3, 4, 5], thr, [False, True, False], 5, 0, True)]
    for k in range(3):
        exp = oracle_smart(tpls[k], seqs[k], 3 + k, thr[k], k == 1)
        np.testing.assert_array_equal(moves[k], exp.moves)
        assert out_bw[k] == exp.bw
    assert out_bw[1] == 4 and out_bw[0] > 3
    # the sequences are inputs only
    assert [s.bandwidth for s in seqs] == [3, 4, 5] and [s.bandwidth_fixed for s in seqs] == [False, True, False]
    with pytest.raises(ValueError):
        pairalign.smart_align_moves_many(seqs, tpls[:2], engine=e)


def test_explicit_pairs_pvalue_doublings_flags(data):
    tpls, seqs = data
    e = StandInEngine()
    pairs = [(2, 0), (0, 0), (1, 2), (0, 1)]
    got, out_bw = pairalign.smart_align_many(seqs, tpls, pairs=pairs, pvalue=0.5, max_doublings=2, bandwidth=2,
                                             skew_matches=True, trim=True, engine=e)
    thr = [cquantile_poisson(seqs[i].est_n_errors, 0.5) for i, _ in pairs]
    assert e.calls == [("smart", [2, 0, 1, 0], [0, 0, 2, 1], [2] * 4, thr, [False, False, True, False], 2,
                        RF_SKEW | RF_TRIM, True)]
    assert len(got) == 4 and out_bw.tolist() == [oracle_smart(tpls[j], seqs[i], 2, th, i == 1, 2).bw
                                                 for (i, j), th in zip(pairs, thr)]
    got, out_bw = pairalign.smart_align_many(seqs, tpls, engine=e)
    for k, (at, as_) in enumerate(got):
        exp = oracle_smart(tpls[k], seqs[k], 3 + k, cquantile_poisson(seqs[k].est_n_errors, 0.1), k == 1)
        assert (at, as_) == moves_to_aligned_seqs(exp.moves, tpls[k], seqs[k].seq)
    empty = pairalign.smart_align_moves_many(seqs, tpls, pairs=np.zeros((0, 2), int), engine=e)
    assert empty[0] == [] and len(empty[1]) == 0
    with pytest.raises(ValueError):
        pairalign.smart_align_moves_many(seqs, tpls, pairs=[(3, 0)], engine=e)


def test_band_at_the_largest_bandwidth_is_checked():
    """n = m = 2,600, bandwidth 100: 201 rows where a pair starts, and
    2 * 2,600 + 1 rows at min(100 * 2^5, m, n); with max_doublings = 4 the
    largest band is 2 * 1,600 + 1 rows and passes the check; a fixed
    sequence stays at its own bandwidth."""
    rng = np.random.default_rng(2403)
    t = random_seq(2600, rng)
    s = RifrafSequence(t.copy(), np.full(2600, -2.0), 100, SEQ_SCORES)
    small = RifrafSequence(t[:30].copy(), np.full(30, -2.0), 3, SEQ_SCORES)
    e = StandInEngine()
    with pytest.raises(RifrafError) as err:
        pairalign.smart_align_moves_many([small, s], [t[:30], t], engine=e)
    assert "pair 1" in str(err.value) and "5201" in str(err.value) and str(pairalign.MAX_BAND_ROWS) in str(err.value)
    assert e.calls == []
    with pytest.raises(RifrafError):
        assign.cross_scores([s], [t], bandwidth_pvalue=0.1, engine=e)
    assert e.calls == []
    bws = np.array([100, 100, 100])
    top = pairalign.max_bandwidths(bws, [False, False, True], np.full(3, 2600), np.array([2600, 2000, 2600]), 5)
    assert top.tolist() == [2600, 2000, 100]
    assert pairalign.max_bandwidths(bws[:1], [False], np.array([2600]), np.array([2600]), 4).tolist() == [1600]
    assert 2 * 1600 + 1 <= pairalign.MAX_BAND_ROWS < 2 * 2600 + 1


def test_cross_scores_routes(data):
    tpls, seqs = data
    e = StandInEngine()
    plain = assign.cross_scores(seqs, tpls, engine=e)
    assert e.calls == [("scores", (3, 3))] and plain.shape == (3, 3)
    sc, bw = assign.cross_scores(seqs, tpls, engine=e, bandwidth_pvalue=0.1, return_bandwidths=True)
    call = e.calls[-1]
    assert call[0] == "smart" and call[1] == [0, 0, 0, 1, 1, 1, 2, 2, 2] and call[2] == [0, 1, 2] * 3
    assert call[3] == [3, 3, 3, 4, 4, 4, 5, 5, 5] and call[5] == [False] * 3 + [True] * 3 + [False] * 3
    assert call[4] == [cquantile_poisson(s.est_n_errors, 0.1) for s in seqs for _ in range(3)]
    assert call[8] is False
    assert sc.shape == bw.shape == (3, 3)
    for r in range(3):
        for j in range(3):
            exp = oracle_smart(tpls[j], seqs[r], 3 + r, cquantile_poisson(seqs[r].est_n_errors, 0.1), r == 1)
            assert sc[r, j] == exp.score and bw[r, j] == exp.bw
    assert bw[1].tolist() == [4, 4, 4] and (bw[0] > 3).any()
    only = assign.cross_scores(seqs, tpls, engine=e, bandwidth_pvalue=0.1)
    assert np.array_equal(only, sc)
    sc9, bw9 = assign.cross_scores(seqs, tpls, bandwidth=9, engine=e, return_bandwidths=True)
    assert (bw9 == 9).all() and e.calls[-1][0] == "scores"


def test_package_exports():
    import rifraf_amd
    for name in ("smart_align_moves_many", "smart_align_many"):
        assert getattr(rifraf_amd, name) is getattr(pairalign, name)
