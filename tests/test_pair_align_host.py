"""rifraf_amd.pairalign without a GPU: its four functions over a small
stand-in engine whose pair_align calls the CPU oracle (forward_moves! +
backtrace + count_errors), so the host bookkeeping -- pair lists, bandwidth
defaults, one reference or many, invalid pairs, the too-wide refusal, the
proposals of correct_shifts -- is checked on its own."""
import math

import numpy as np
import pytest

import oracle
from _util import SEQ_SCORES, make_read, random_seq
from rifraf_amd import DNASeq, ErrorModel, RifrafSequence, Scores, pairalign
from rifraf_amd.align import moves_to_aligned_seqs
from rifraf_amd.engine import RF_SKEW, RF_TRIM, RifrafError
from rifraf_amd.types import dna_str


class StandInEngine:
    """set_sequences / set_templates / pair_align of rifraf_amd.engine.Engine
    on the oracle.  Records every pair_align call."""

    def __init__(self):
        self.seqs, self.tpls, self.calls = {}, {}, []

    def set_sequences(self, first, seqs):
        for k, s in enumerate(seqs):
            self.seqs[first + k] = s

    def set_templates(self, first, tpls):
        for k, t in enumerate(tpls):
            self.tpls[first + k] = np.asarray(t, np.uint8)

    def pair_align(self, seqs, tpls, bws, flags=0, want_moves=True, caps=None):
        seqs, tpls, bws = np.broadcast_arrays(np.asarray(seqs), np.asarray(tpls), np.asarray(bws))
        self.calls.append((seqs.reshape(-1).tolist(), tpls.reshape(-1).tolist(), bws.reshape(-1).tolist(), flags))
        scores, moves, nerr = [], [], []
        for si, ti, bw in zip(seqs.reshape(-1), tpls.reshape(-1), bws.reshape(-1)):
            s, t = self.seqs[int(si)], self.tpls[int(ti)]
            n, m = len(s.seq), len(t)
            if caps is not None:
                assert np.asarray(caps).reshape(-1)[len(scores)] == n + m
            try:
                A, mv = oracle.forward(t, s, moves=True, skew=bool(flags & RF_SKEW), trim=bool(flags & RF_TRIM),
                                       bandwidth=int(bw))
            except oracle.OracleError:
                scores.append(np.nan)
                moves.append(None)
                nerr.append(-1)
                continue
            w = oracle.backtrace(mv, n + 1, m + 1, int(bw))
            scores.append(A[n - m + max(m - n, 0) + int(bw), m])
            moves.append(w)
            nerr.append(oracle.count_errors(w, t, s.seq))
        return np.array(scores), (moves if want_moves else None), np.array(nerr, np.int32)


def oracle_moves(t, s, bw, **kw):
    _, mv = oracle.forward(t, s, moves=True, bandwidth=bw, **kw)
    return oracle.backtrace(mv, len(s.seq) + 1, len(t) + 1, bw)


@pytest.fixture
def data():
    rng = np.random.default_rng(2301)
    tpls = [random_seq(m, rng) for m in (30, 41, 36)]
    seqs = [make_read(tpls[k % 3], rng, 0.06, 4 + k) for k in range(3)]
    return tpls, seqs


def test_default_pairs_and_own_bandwidth(data):
    tpls, seqs = data
    e = StandInEngine()
    got = pairalign.align_moves_many(seqs, tpls, engine=e)
    assert len(e.calls) == 1 and e.calls[0] == ([0, 1, 2], [0, 1, 2], [4, 5, 6], 0)
    for k in range(3):
        np.testing.assert_array_equal(got[k], oracle_moves(tpls[k], seqs[k], 4 + k))
    with pytest.raises(ValueError):
        pairalign.align_moves_many(seqs, tpls[:2], engine=e)


def test_explicit_pairs_flags_and_bandwidth(data):
    tpls, seqs = data
    e = StandInEngine()
    pairs = [(2, 0), (0, 0), (1, 2), (0, 1)]
    got = pairalign.align_moves_many(seqs, tpls, pairs=pairs, bandwidth=12, skew_matches=True, trim=True, engine=e)
    assert e.calls == [([2, 0, 1, 0], [0, 0, 2, 1], [12] * 4, RF_SKEW | RF_TRIM)]
    for (i, j), mv in zip(pairs, got):
        np.testing.assert_array_equal(mv, oracle_moves(tpls[j], seqs[i], 12, skew=True, trim=True))
    own = pairalign.align_moves_many(seqs, tpls, pairs=pairs, engine=e)
    assert e.calls[-1][2] == [6, 4, 5, 4]
    assert len(own) == 4
    with pytest.raises(ValueError):
        pairalign.align_moves_many(seqs, tpls, pairs=[(3, 0)], engine=e)
    assert pairalign.align_moves_many(seqs, tpls, pairs=np.zeros((0, 2), int), engine=e) == []


def test_align_many_strings(data):
    tpls, seqs = data
    e = StandInEngine()
    pairs = [(0, 0), (1, 1), (2, 1)]
    got = pairalign.align_many(seqs, tpls, pairs=pairs, engine=e)
    assert len(e.calls) == 1
    for (i, j), (at, as_) in zip(pairs, got):
        assert (at, as_) == moves_to_aligned_seqs(oracle_moves(tpls[j], seqs[i], seqs[i].bandwidth), tpls[j],
                                                  seqs[i].seq)
        assert at.replace("-", "") == dna_str(tpls[j]) and as_.replace("-", "") == dna_str(seqs[i].seq)


def test_invalid_pair_is_none():
    n = 9
    ninf = np.full(n, -np.inf)
    bad = RifrafSequence(np.zeros(n, np.uint8), np.full(n, -2.0), 3, SEQ_SCORES)
    bad.mismatch_scores, bad.ins_scores, bad.del_scores = ninf, ninf, np.full(n + 1, -np.inf)
    rng = np.random.default_rng(2302)
    good = make_read(random_seq(n, rng), rng, 0.05, 3)
    tpls = [np.full(n, 1, np.uint8), random_seq(n, rng)]
    e = StandInEngine()
    got = pairalign.align_moves_many([bad, good], tpls, engine=e)
    assert got[0] is None
    np.testing.assert_array_equal(got[1], oracle_moves(tpls[1], good, 3))
    assert pairalign.align_many([bad, good], tpls, engine=e)[0] is None


def test_too_wide_is_refused(data):
    tpls, seqs = data
    e = StandInEngine()
    long_t = np.zeros(len(seqs[1].seq) + pairalign.MAX_BAND_ROWS, np.uint8)   # H = MAX + 2 bw + 1
    with pytest.raises(RifrafError) as err:
        pairalign.align_moves_many(seqs[:2], [tpls[0], long_t], engine=e)
    assert "pair 1" in str(err.value) and str(pairalign.MAX_BAND_ROWS) in str(err.value)
    assert e.calls == []
    # the widest band that is accepted: H = MAX_BAND_ROWS exactly (not run here: only the check)
    bw = seqs[0].bandwidth
    edge = np.zeros(len(seqs[0].seq) + pairalign.MAX_BAND_ROWS - 2 * bw - 1, np.uint8)
    rows = 2 * bw + abs(len(seqs[0].seq) - len(edge)) + 1
    assert rows == pairalign.MAX_BAND_ROWS


def test_edit_distances():
    rng = np.random.default_rng(2303)
    tpls = [random_seq(m, rng) for m in (20, 33, 27)]
    seqs = [make_read(t, rng, 0.15).seq for t in tpls]
    e = StandInEngine()
    got = pairalign.edit_distances(tpls, seqs, engine=e)
    assert len(e.calls) == 1
    bws = [int(math.ceil(min(len(t), len(s)) * 0.5)) for t, s in zip(tpls, seqs)]
    assert e.calls[0][2] == bws and e.calls[0][3] == RF_SKEW
    sc = Scores.from_errors(ErrorModel(1.0, 1.0, 1.0))
    for k, (t, s) in enumerate(zip(tpls, seqs)):
        rs = RifrafSequence(s, np.full(len(s), -1.0), bws[k], sc)
        w = oracle_moves(t, rs, bws[k], skew=True)
        assert got[k] == oracle.count_errors(w, t, s)
    assert pairalign.edit_distances([tpls[0]], [tpls[0]], engine=e)[0] == 0
    with pytest.raises(ValueError):
        pairalign.edit_distances(tpls, seqs[:2], engine=e)


SHIFT_KATS = [("TTTT", "TTT", "TTT"), ("TT", "TTT", "TTT"), ("TTTACCC", "TTTCGC", "TTTCCC"),
              ("TTTAAACCC", "TTTCGC", "TTTAAACCC")]   # test/test_correct_shifts.jl:8-35


def test_correct_shifts_kats():
    e = StandInEngine()
    got = pairalign.correct_shifts_many([DNASeq(c) for c, _, _ in SHIFT_KATS], [DNASeq(r) for _, r, _ in SHIFT_KATS],
                                        engine=e)
    assert [dna_str(g) for g in got] == [x for _, _, x in SHIFT_KATS]
    assert len(e.calls) == 1 and e.calls[0][3] == RF_SKEW
    assert e.calls[0][2] == [int(math.ceil(min(len(c), len(r)) * 0.1)) for c, r, _ in SHIFT_KATS]


def test_correct_shifts_one_reference_or_one_each():
    e = StandInEngine()
    cons = [DNASeq("TTTACCC"), DNASeq("TTTAAACCC"), DNASeq("TTTCCC")]
    one = pairalign.correct_shifts_many(cons, DNASeq("TTTCGC"), engine=e)
    assert [dna_str(g) for g in one] == ["TTTCCC", "TTTAAACCC", "TTTCCC"]
    as_str = pairalign.correct_shifts_many(cons, "TTTCGC", engine=e)
    each = pairalign.correct_shifts_many(cons, [DNASeq("TTTCGC")] * 3, bandwidth=2, engine=e)
    assert [dna_str(g) for g in as_str] == [dna_str(g) for g in one]
    assert [dna_str(g) for g in each] == [dna_str(g) for g in one]
    assert e.calls[-1][2] == [2, 2, 2]
    with pytest.raises(ValueError):
        pairalign.correct_shifts_many(cons, [DNASeq("TTT")] * 2, engine=e)


def test_package_exports():
    import rifraf_amd
    for name in ("align_moves_many", "align_many", "edit_distances", "correct_shifts_many"):
        assert getattr(rifraf_amd, name) is getattr(pairalign, name)
