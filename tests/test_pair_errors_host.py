"""Error counts carried through the fill, without a GPU: align.forward_errors
(the host restatement of what the engine's counting fills keep per cell)
against the oracle's forward_moves! + backtrace + count_errors; the C-ABI
declarations; the routing of assign.cross_scores / choose_references and the
inputs pairalign.count_errors_many / smart_bandwidths_many build, over a
stand-in engine; and the band limit of the two LDS rings.

Equality is exact: bit-equal scores, integer-equal counts."""
import math
import os
import re

import numpy as np
import pytest

import oracle
from _util import REF_SCORES, SEQ_SCORES, random_seq
import rifraf_amd.align as align
from rifraf_amd import RifrafSequence, assign, pairalign
from rifraf_amd.engine import RF_SKEW
from rifraf_amd.poisson import cquantile_poisson
from test_pair_align_smart_host import StandInEngine, oracle_align, oracle_smart, smart_set

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(x):
    return np.float64(x).view(np.int64)


def same(t, s, bw, skew=False, trim=False):
    """forward_errors == (A[end, end], count_errors(backtrace)) of the oracle."""
    got = align.forward_errors(t, s, bandwidth=bw, trim=trim, skew_matches=skew)
    score, _, nerr = oracle_align(t, s, bw, skew=skew, trim=trim)
    assert bits(got[0]) == bits(score) and got[1] == nerr, (len(s.seq), len(t), bw, skew, trim, got, score, nerr)


# ---------------------------------------------------------------------
# 1. the carried count is the walked count
# ---------------------------------------------------------------------
def test_ties_two_letters_constant_phred():
    """Two letters and one Phred: nearly every cell has tied candidates, so
    the order match, insert, delete decides the path."""
    rng = np.random.default_rng(2501)
    for n in range(1, 7):
        for m in range(1, 7):
            for bw in (1, 2, 3):
                for _ in range(4):
                    s = RifrafSequence(rng.integers(0, 2, n).astype(np.uint8), np.full(n, -1.0), bw, SEQ_SCORES)
                    same(rng.integers(0, 2, m).astype(np.uint8), s, bw)


@pytest.mark.parametrize("skew,trim", ((False, False), (True, False), (False, True), (True, True)))
def test_random_phreds_and_flags(skew, trim):
    rng = np.random.default_rng(2502)
    for n in range(1, 7):
        for m in range(1, 7):
            for bw in (1, 2, 3):
                s = RifrafSequence(random_seq(n, rng), np.log10(rng.uniform(0.01, 0.3, n)), bw, SEQ_SCORES)
                same(random_seq(m, rng), s, bw, skew=skew, trim=trim)
                s2 = RifrafSequence(rng.integers(0, 2, n).astype(np.uint8), np.full(n, -1.0), bw, SEQ_SCORES)
                same(rng.integers(0, 2, m).astype(np.uint8), s2, bw, skew=skew, trim=trim)


def test_codon_reads():
    rng = np.random.default_rng(2503)
    codon = 0
    for n in range(3, 9):
        for m in range(3, 9):
            for bw in (1, 2, 3):
                for phred in (np.full(n, -1.0), np.log10(rng.uniform(0.01, 0.3, n))):
                    s = RifrafSequence(rng.integers(0, 2, n).astype(np.uint8), phred, bw, REF_SCORES)
                    t = rng.integers(0, 2, m).astype(np.uint8)
                    assert len(s.codon_ins_scores) and len(s.codon_del_scores)
                    same(t, s, bw)
                    same(t, s, bw, skew=True)
                    codon += int((oracle_align(t, s, bw)[1] >= 4).any())
    assert codon > 0, "no codon move on any path"


def test_smart_set_pairs():
    seqs, tpls, bws, _ = smart_set()
    assert len(seqs) == 44
    for t, s, bw in zip(tpls, seqs, bws):
        same(t, s, int(bw))
    same(tpls[2], seqs[2], 2 * int(bws[2]), skew=True)   # a codon read, skewed, one doubling on


def test_invalid_fill_is_nan_and_minus_one():
    """The pair of test_pair_align_smart.test_invalid_in_round_two: valid at
    bandwidth 2, "new score is invalid" at 4."""
    rng = np.random.default_rng(2411)
    n = 20
    bad = RifrafSequence(random_seq(n, rng), np.log10(rng.uniform(0.01, 0.3, n)), 2, SEQ_SCORES)
    bad.seq[9] = 1
    for name in ("mismatch_scores", "ins_scores", "del_scores"):
        setattr(bad, name, getattr(bad, name).copy())
    bad.mismatch_scores[9] = bad.ins_scores[9] = bad.del_scores[10] = -np.inf
    t = np.full(n, 2, np.uint8)
    t[7:12] = 1
    same(t, bad, 2)
    with pytest.raises(oracle.OracleError):
        oracle_align(t, bad, 4)
    score, nerr = align.forward_errors(t, bad, bandwidth=4)
    assert math.isnan(score) and nerr == -1
    with pytest.raises(ValueError):
        align.forward_errors(t, bad, bandwidth=0)


# ---------------------------------------------------------------------
# 2. the C-ABI and the package
# ---------------------------------------------------------------------
def test_abi_declares_both():
    text = open(os.path.join(REPO, "include", "rifraf_hip.h")).read()
    assert re.search(r"#define RF_ABI_VERSION 1\b", text)
    decl = re.search(r"int rf_pair_errors\(([^;]*)\);", text).group(1)
    names = re.findall(r"\*?(\w+)\s*(?:,|$)", " ".join(decl.split()))
    assert names == ["ctx", "npairs", "seq", "tpl", "bw", "threshold", "fixed", "max_doublings", "flags", "out_score",
                     "nerrors", "out_bw", "out_rounds"]
    assert re.search(r"int rf_last_pair_errors_ms\(const rf_ctx \*ctx, double \*fill_ms\);", text)
    from rifraf_amd import _lib
    assert len(_lib._SIGNATURES["rf_pair_errors"][1]) == 13
    assert len(_lib._SIGNATURES["rf_last_pair_errors_ms"][1]) == 2
    assert _lib.RF_ABI_VERSION == 1
    import rifraf_amd
    for name in ("count_errors_many", "smart_bandwidths_many"):
        assert getattr(rifraf_amd, name) is getattr(pairalign, name)
    assert rifraf_amd.forward_errors is align.forward_errors


def test_two_ring_limit():
    """DP_COUNT_H: the widest band whose score ring (4 x 8 B) and count ring
    (4 x 4 B) of H + 6 entries fit 160 KiB of LDS."""
    text = open(os.path.join(REPO, "rifraf.jl_amd", "csrc", "rifraf_dp_plan.h")).read()
    H = int(re.search(r"constexpr int DP_COUNT_H = (\d+);", text).group(1))
    assert 48 * (H + 6) <= 163840 < 48 * (H + 1 + 6)
    gen64 = int(re.search(r"constexpr int DP_GEN64_H = (\d+);", text).group(1))
    lds = int(re.search(r"constexpr int DP_LDS_H = (\d+);", text).group(1))
    assert gen64 < H < lds   # the whole one-wave tier carries the count; the top of the wide tier takes the trace


# ---------------------------------------------------------------------
# 3. routing and plumbing over a stand-in engine
# ---------------------------------------------------------------------
class CountingStandIn(StandInEngine):
    """StandInEngine with Engine.pair_errors on the oracle."""

    def pair_errors(self, seqs, tpls, bws, thresholds=None, fixed=None, max_doublings=0, flags=0):
        if thresholds is None:
            assert max_doublings == 0
            thresholds = 0.0
        if fixed is None:
            fixed = False
        seqs, tpls, bws, thr, fixed = (x.reshape(-1) for x in np.broadcast_arrays(
            np.asarray(seqs), np.asarray(tpls), np.asarray(bws), np.asarray(thresholds, float), np.asarray(fixed)))
        self.calls.append(("errors", seqs.tolist(), tpls.tolist(), bws.tolist(), thr.tolist(), fixed.tolist(),
                           max_doublings, flags))
        if max_doublings == 0:
            res = []
            for i, j, bw in zip(seqs, tpls, bws):
                sc, _, ne = oracle_align(self.tpls[int(j)], self.seqs[int(i)], int(bw), skew=bool(flags & RF_SKEW))
                res.append((sc, ne, int(bw), 1))
        else:
            assert flags == 0
            res = [(r.score, r.nerr, r.bw, r.rounds) for r in
                   (oracle_smart(self.tpls[int(j)], self.seqs[int(i)], int(bw), float(th), bool(fx), max_doublings)
                    for i, j, bw, th, fx in zip(seqs, tpls, bws, thr, fixed))]
        return (np.array([r[0] for r in res]), np.array([r[1] for r in res], np.int32),
                np.array([r[2] for r in res], np.int32), np.array([r[3] for r in res], np.int32))


@pytest.fixture
def data():
    from test_pair_align_smart_host import indel_read
    rng = np.random.default_rng(2402)
    tpls = [random_seq(m, rng) for m in (90, 120, 75)]
    seqs = [indel_read(tpls[k], rng, 3 + k, SEQ_SCORES, 5 + k) for k in range(3)]
    seqs[1].bandwidth_fixed = True
    return tpls, seqs


def test_carry_counts_routes(data):
    tpls, seqs = data
    e = CountingStandIn()
    sc0, bw0 = assign.cross_scores(seqs, tpls, engine=e, bandwidth_pvalue=0.1, return_bandwidths=True)
    assert e.calls[-1][0] == "smart"
    sc1, bw1 = assign.cross_scores(seqs, tpls, engine=e, bandwidth_pvalue=0.1, return_bandwidths=True,
                                   carry_counts=True)
    assert e.calls[-1][0] == "errors" and e.calls[-1][1:8] == e.calls[-2][1:8]
    assert sc0.tobytes() == sc1.tobytes() and bw0.tobytes() == bw1.tobytes() and sc1.shape == (3, 3)
    # without a p-value there is nothing to count: score-only as before
    assign.cross_scores(seqs, tpls, engine=e, carry_counts=True)
    assert e.calls[-1][0] == "scores"
    clusters = [([s.seq for s in seqs], [np.full(len(s.seq), 20, np.int8) for s in seqs])]
    n = len(e.calls)
    a = assign.choose_references(clusters, tpls, bandwidth=3, engine=e, bandwidth_pvalue=0.1)
    assert e.calls[n][0] == "smart"
    b = assign.choose_references(clusters, tpls, bandwidth=3, engine=e, bandwidth_pvalue=0.1, carry_counts=True)
    assert e.calls[n + 1][0] == "errors" and e.calls[n + 1][1:8] == e.calls[n][1:8]
    assert a[0][0] == b[0][0] and a[0][1].tobytes() == b[0][1].tobytes()


def test_many_build_the_inputs_of_smart_align_moves_many(data):
    tpls, seqs = data
    e = CountingStandIn()
    pairs = [(2, 0), (0, 0), (1, 2), (0, 1)]
    for kw in (dict(), dict(pairs=pairs, pvalue=0.5, max_doublings=2, bandwidth=2)):
        moves, bw_moves = pairalign.smart_align_moves_many(seqs, tpls, engine=e, **kw)
        bw, nerr, sc = pairalign.smart_bandwidths_many(seqs, tpls, engine=e, **kw)
        smart, errors = e.calls[-2], e.calls[-1]
        assert smart[0] == "smart" and errors[0] == "errors"
        assert errors[1:8] == smart[1:8]   # pairs, bandwidths, thresholds, fixed, max_doublings, flags
        assert bw.tolist() == bw_moves.tolist()
        pp = pairs if kw else [(k, k) for k in range(3)]
        for k, (i, j) in enumerate(pp):
            assert nerr[k] == oracle.count_errors(moves[k], tpls[j], seqs[i].seq)
    thr = [cquantile_poisson(s.est_n_errors, 0.1) for s in seqs]
    assert e.calls[1][4] == thr and e.calls[1][5] == [False, True, False]
    # count_errors_many: the reference's count_errors(t, s) skews
    got = pairalign.count_errors_many(seqs, tpls, pairs=pairs, engine=e)
    assert e.calls[-1] == ("errors", [2, 0, 1, 0], [0, 0, 2, 1], [5, 3, 4, 3], [0.0] * 4, [False] * 4, 0, RF_SKEW)
    assert got.tolist() == [oracle_align(tpls[j], seqs[i], seqs[i].bandwidth, skew=True)[2] for i, j in pairs]
    got = pairalign.count_errors_many(seqs, tpls, bandwidth=7, skew_matches=False, engine=e)
    assert e.calls[-1][3] == [7] * 3 and e.calls[-1][7] == 0
    assert len(pairalign.count_errors_many(seqs, tpls, pairs=np.zeros((0, 2), int), engine=e)) == 0
    with pytest.raises(ValueError):
        pairalign.smart_bandwidths_many(seqs, tpls[:2], engine=e)
    assert [s.bandwidth for s in seqs] == [3, 4, 5] and [s.bandwidth_fixed for s in seqs] == [False, True, False]
