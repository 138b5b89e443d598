"""The host side of the pair text products, without a GPU.

Known answers restated from the reference's test/test_align.jl ("alignment"
testset, :183-252): "align 1" and "align 2" for moves_to_aligned_seqs and
"moves_to_indices 1" .. "4" for moves_to_indices, over the oracle's moves of
the same pairs.  The reference's tests hold no case for band_tolerance (the
function is not called anywhere in its test directory), so align.band_tolerance
is pinned instead against a literal transcription of align.jl:262-284 that
walks a BandedArray of the oracle's moves backwards.

Then the fallback of pairalign: an engine without pair_align_text (the stand-in
engines on the oracle) still gives align_many, smart_align_many,
align_indices_many and band_tolerances through the moves and the host loops.
"""
import numpy as np
import pytest

import oracle
from _util import REF_SCORES, SEQ_SCORES, make_read, random_seq
from rifraf_amd import BandedArray, DNASeq, ErrorModel, RifrafSequence, Scores, pairalign
from rifraf_amd.align import OFFSETS, band_tolerance, moves_to_aligned_seqs, moves_to_indices
from rifraf_amd.errormodel import normalize
from test_pair_align_host import StandInEngine, oracle_moves
from test_pair_align_smart_host import StandInEngine as SmartStandIn
from test_pair_align_smart_host import indel_read, oracle_smart, poisson_thresholds

KAT_SCORES = Scores.from_errors(normalize(ErrorModel(1.0, 1.0, 1.0, 0.0, 0.0)))   # test_align.jl:184-185


def kat_moves(template, seq, log_p):
    t, s = DNASeq(template), DNASeq(seq)
    rs = RifrafSequence(s, np.asarray(log_p, np.float64), 10, KAT_SCORES)
    return oracle_moves(t, rs, 10), t, s


def test_kat_align_1():                                            # test_align.jl:187-197
    mv, t, s = kat_moves("ATAA", "AAA", [-2.0, -3.0, -3.0])
    assert moves_to_aligned_seqs(mv, t, s) == ("ATAA", "A-AA")


def test_kat_align_2():                                            # test_align.jl:199-208
    mv, t, s = kat_moves("AACCTT", "AAACCCTT", np.full(8, np.log10(0.1)))
    at, as_ = moves_to_aligned_seqs(mv, t, s)
    assert at[-2:] == "TT"
    assert len(at) == len(as_) and at.replace("-", "") == "AACCTT" and as_.replace("-", "") == "AAACCCTT"


@pytest.mark.parametrize("template,seq,exp", [("AAA", "AAA", [1, 2, 3]), ("AAA", "AAAT", [1, 2, 3]),
                                              ("AAAT", "AAA", [1, 2, 3, 3]), ("TAAA", "AAA", [0, 1, 2, 3])])
def test_kat_moves_to_indices(template, seq, exp):                 # test_align.jl:210-252
    mv, t, s = kat_moves(template, seq, np.full(len(seq), np.log10(0.1)))
    assert moves_to_indices(mv, len(t), len(s)) == exp


def test_indices_codon_deletion_pushes_once():
    """align.jl:322-335: j > last_j is asked once per move."""
    assert moves_to_indices([1, 5, 1], 5, 2) == [1, 1, 2]
    assert moves_to_indices([4, 1], 1, 4) == [4]


def band_tolerance_jl(Amoves):
    """align.jl:262-284, line by line (1-based, over the trace band)."""
    nrows, ncols = Amoves.shape
    dist = nrows
    i, j = nrows, ncols
    while i > 1 or j > 1:
        start, stop = Amoves.row_range(j)
        if start > 1:
            dist = min(dist, abs(i - start))
        if stop < nrows:
            dist = min(dist, abs(i - stop))
        a, b = OFFSETS[int(Amoves[i, j])]
        i, j = i - a, j - b
    start, stop = Amoves.row_range(j)
    if start > 1:
        dist = min(dist, abs(i - start))
    if stop < nrows:
        dist = min(dist, abs(i - stop))
    return dist


def test_band_tolerance_is_the_reference_walk():
    rng = np.random.default_rng(2501)
    seen = set()
    for k in range(60):
        m = int(rng.integers(1, 40))
        bw = int(rng.integers(1, 8))
        scores = REF_SCORES if k % 3 == 0 else SEQ_SCORES
        t = random_seq(m, rng)
        if k % 2 and m > 8:
            s = make_read(t, rng, 0.1, bw, scores)
        else:
            n = int(rng.integers(1, 40))
            s = RifrafSequence(random_seq(n, rng), np.log10(rng.uniform(0.01, 0.3, n)), bw, scores)
        n = len(s.seq)
        _, mv = oracle.forward(t, s, moves=True, bandwidth=bw)
        band = BandedArray((n + 1, m + 1), bw, dtype=np.int8, default=0, data=np.asfortranarray(mv))
        moves = oracle.backtrace(mv, n + 1, m + 1, bw)
        exp = band_tolerance_jl(band)
        assert band_tolerance(moves, n + 1, m + 1, bw) == exp, (n, m, bw)
        seen.add("whole" if exp == n + 1 else ("edge" if exp <= 1 else "inside"))
    assert seen == {"whole", "edge", "inside"}


def test_band_tolerance_known_cases():
    # the band covers the matrix: no start > 1, no stop < nrows
    assert band_tolerance([1, 1, 1], 4, 4, 3) == 4
    # n = m = 6 at bandwidth 1 on the diagonal: start = j - 1, stop = j + 1, one row away on both sides
    assert band_tolerance([1] * 6, 7, 7, 1) == 1
    # the same band, a path along its lower edge: insert, matches, delete
    assert band_tolerance([2, 1, 1, 1, 1, 1, 3], 7, 7, 1) == 0


@pytest.fixture
def data():
    rng = np.random.default_rng(2502)
    tpls = [random_seq(m, rng) for m in (30, 41, 36)]
    seqs = [make_read(tpls[k % 3], rng, 0.06, 4 + k) for k in range(3)]
    return tpls, seqs


def test_fallback_without_pair_align_text(data):
    tpls, seqs = data
    e = StandInEngine()
    assert not hasattr(e, "pair_align_text")
    pairs = [(0, 0), (1, 1), (2, 1), (0, 2)]
    texts = pairalign.align_many(seqs, tpls, pairs=pairs, engine=e)
    idx = pairalign.align_indices_many(seqs, tpls, pairs=pairs, engine=e)
    tol = pairalign.band_tolerances(seqs, tpls, pairs=pairs, engine=e)
    assert len(e.calls) == 3                     # one engine call each
    assert tol.dtype == np.int32
    for k, (i, j) in enumerate(pairs):
        mv = oracle_moves(tpls[j], seqs[i], seqs[i].bandwidth)
        assert texts[k] == moves_to_aligned_seqs(mv, tpls[j], seqs[i].seq)
        assert idx[k].dtype == np.int32 and idx[k].tolist() == moves_to_indices(mv, len(tpls[j]), len(seqs[i]))
        assert tol[k] == band_tolerance(mv, len(seqs[i]) + 1, len(tpls[j]) + 1, seqs[i].bandwidth)
    assert pairalign.align_indices_many(seqs, tpls, pairs=np.zeros((0, 2), int), engine=e) == []
    assert pairalign.band_tolerances(seqs, tpls, pairs=np.zeros((0, 2), int), engine=e).shape == (0,)


def test_fallback_invalid_pair():
    n = 9
    ninf = np.full(n, -np.inf)
    bad = RifrafSequence(np.zeros(n, np.uint8), np.full(n, -2.0), 3, SEQ_SCORES)
    bad.mismatch_scores, bad.ins_scores, bad.del_scores = ninf, ninf, np.full(n + 1, -np.inf)
    rng = np.random.default_rng(2503)
    good = make_read(random_seq(n, rng), rng, 0.05, 3)
    tpls = [np.full(n, 1, np.uint8), random_seq(n, rng)]
    e = StandInEngine()
    assert pairalign.align_many([bad, good], tpls, engine=e)[0] is None
    assert pairalign.align_indices_many([bad, good], tpls, engine=e)[0] is None
    tol = pairalign.band_tolerances([bad, good], tpls, engine=e)
    assert tol[0] == -1 and tol[1] >= 0


def test_fallback_smart():
    rng = np.random.default_rng(2504)
    tpls = [random_seq(m, rng) for m in (90, 120, 75)]
    seqs = [indel_read(tpls[k], rng, 3 + k, SEQ_SCORES, 5 + k) for k in range(3)]
    e = SmartStandIn()
    texts, out_bw = pairalign.smart_align_many(seqs, tpls, engine=e)
    tol = pairalign.band_tolerances(seqs, tpls, max_doublings=5, engine=e)
    idx = pairalign.align_indices_many(seqs, tpls, max_doublings=5, engine=e)
    assert [c[0] for c in e.calls] == ["smart"] * 3
    thr = poisson_thresholds(seqs)
    for k in range(3):
        r = oracle_smart(tpls[k], seqs[k], 3 + k, float(thr[k]), False)
        assert out_bw[k] == r.bw
        assert texts[k] == moves_to_aligned_seqs(r.moves, tpls[k], seqs[k].seq)
        assert tol[k] == band_tolerance(r.moves, len(seqs[k]) + 1, len(tpls[k]) + 1, r.bw)
        assert idx[k].tolist() == moves_to_indices(r.moves, len(tpls[k]), len(seqs[k]))
    assert (out_bw > np.array([3, 4, 5])).any()


def test_package_exports():
    import rifraf_amd
    for name in ("align_indices_many", "band_tolerances"):
        assert getattr(rifraf_amd, name) is getattr(pairalign, name)
    from rifraf_amd import align
    assert rifraf_amd.band_tolerance is align.band_tolerance
