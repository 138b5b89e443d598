"""k_pa_walk_w, the wave-per-pair walk of rf_pair_align (RF_OPT_PAIR_WALK =
2), beside k_pa_walk (1): every case runs under both values, against the CPU
oracle's forward_moves! + backtrace + count_errors and against each other.
Equality is exact: integer-equal moves and counts, bit-equal scores."""
from types import SimpleNamespace

import numpy as np
import pytest

import oracle
from _util import REF_SCORES, SEQ_SCORES, make_read, random_seq
from rifraf_amd import ErrorModel, RifrafSequence, Scores
from rifraf_amd._lib import ptr
from rifraf_amd.engine import RF_SKEW
from test_pair_align_smart_host import oracle_align

pytestmark = pytest.mark.gpu

WALKS = (1, 2)   # lane per pair, wave per pair


def both(engine, opts, seqs, tpls, bws, flags=0, exp=None, what=None):
    """One pair_align call per walk over pairs k with k; each against exp
    ([(score, moves, nerrors)]) and the two against each other."""
    engine.set_sequences(0, seqs)
    engine.set_templates(0, tpls)
    ids = np.arange(len(seqs))
    got = {}
    for w in WALKS:
        opts("pair_walk", w)
        assert engine.get_option("pair_walk") == w
        got[w] = engine.pair_align(ids, ids, bws, flags)
        counts = engine.pair_align(ids, ids, bws, flags, want_moves=False)   # moves NULL: the same counts
        np.testing.assert_array_equal(counts[2], got[w][2])
    for w in WALKS:
        scores, moves, nerr = got[w]
        for k, e in enumerate(exp):
            tag = (w, k if what is None else what[k])
            assert np.float64(scores[k]).view(np.int64) == np.float64(e[0]).view(np.int64), tag
            assert moves[k] is not None, tag
            np.testing.assert_array_equal(moves[k], e[1], err_msg=str(tag))
            assert nerr[k] == e[2], (tag, nerr[k], e[2])
    assert got[1][0].tobytes() == got[2][0].tobytes() and got[1][2].tobytes() == got[2][2].tobytes()
    return got[2]


def test_option_default(engine):
    assert engine.get_option("pair_walk") == 0


def test_small_shapes(engine, opts):
    """test_pair_align.test_trace_word_edges' shapes: n, m in {14..18, 30..34,
    47..49}, |n - m| <= 3, bw 1, 2, 3, 9 -- periods on, below and above
    multiples of 16, HP < 64 so most lanes of a window are masked -- lean and
    codon reads."""
    rng = np.random.default_rng(2502)
    L = list(range(14, 19)) + list(range(30, 35)) + list(range(47, 50))
    seqs, tpls, bws, what = [], [], [], []
    for scores in (SEQ_SCORES, REF_SCORES):
        for n in L:
            for m in L:
                if abs(n - m) > 3:
                    continue
                for bw in (1, 2, 3, 9):
                    t = random_seq(m, rng)
                    r = make_read(t, rng, 0.08, bw, scores)
                    s = np.concatenate([r.seq, random_seq(max(n - len(r.seq), 0), rng)])[:n]
                    seqs.append(RifrafSequence(s, np.log10(rng.uniform(0.01, 0.3, n)), bw, scores))
                    tpls.append(t)
                    bws.append(bw)
                    what.append((n, m, bw, scores is REF_SCORES))
    exp = [oracle_align(t, s, bw) for t, s, bw in zip(tpls, seqs, bws)]
    assert any((e[1] >= 4).any() for e in exp), "no codon move in the set"
    both(engine, opts, seqs, tpls, bws, exp=exp, what=what)


def diagonals(moves, n, m, bw):
    """The band diagonals d = ii - jj + c the path visits."""
    di = np.array([0, 1, 1, 0, 3, 0])[moves]
    dj = np.array([0, 1, 0, 1, 0, 3])[moves]
    ii = np.concatenate([[0], np.cumsum(di)])
    jj = np.concatenate([[0], np.cumsum(dj)])
    assert ii[-1] == n and jj[-1] == m
    return ii - jj + max(m - n, 0) + bw


def test_window_edges(engine, opts):
    """H > 64 (bw 40 and 100, m of 300-600) and a read with one block
    insertion and one block deletion of 35-90 bases: the path leaves a
    64-diagonal window in both directions; lean and codon reads."""
    rng = np.random.default_rng(2503)
    seqs, tpls, bws, what = [], [], [], []
    for bw, widths in ((40, (35, 38)), (100, (35, 70, 90))):
        for wi in widths:
            for scores in (SEQ_SCORES, REF_SCORES):
                m = int(rng.integers(300, 601))
                t = random_seq(m, rng)
                s = make_read(t, rng, 0.02, bw, scores).seq
                a, b = len(s) // 4, (2 * len(s)) // 3
                wd = int(rng.integers(35, min(bw, 90) + 1))
                if len(seqs) % 2:   # insertion first, or deletion first
                    s = np.concatenate([s[:a], random_seq(wi, rng), s[a:b], s[b + wd:]])
                else:
                    s = np.concatenate([s[:a], s[a + wd:b], random_seq(wi, rng), s[b:]])
                s = s.astype(np.uint8)
                seqs.append(RifrafSequence(s, np.log10(rng.uniform(0.01, 0.3, len(s))), bw, scores))
                tpls.append(t)
                bws.append(bw)
                what.append((bw, wi, wd, len(s), m))
    exp = [oracle_align(t, s, bw) for t, s, bw in zip(tpls, seqs, bws)]
    spans = [np.ptp(diagonals(e[1], len(s.seq), len(t), bw)) for e, s, t, bw in zip(exp, seqs, tpls, bws)]
    assert max(spans) > 64, spans
    assert all(2 * bw + abs(len(s.seq) - len(t)) + 1 > 64 for s, t, bw in zip(seqs, tpls, bws))
    both(engine, opts, seqs, tpls, bws, exp=exp, what=what)


def test_long_match_runs(engine, opts):
    """Identical read and template of 257 and of 1,100 bases: one run of
    matches over many words and blocks."""
    rng = np.random.default_rng(2504)
    tpls = [random_seq(m, rng) for m in (257, 1100)]
    seqs = [RifrafSequence(t.copy(), np.log10(rng.uniform(0.01, 0.3, len(t))), 9, SEQ_SCORES) for t in tpls]
    exp = [oracle_align(t, s, 9) for t, s in zip(tpls, seqs)]
    assert all((e[1] == 1).all() and e[2] == 0 for e in exp)
    both(engine, opts, seqs, tpls, 9, exp=exp)


def test_widest_band(engine, opts):
    """n = m = 2,556 at bw 2,556, skewed, with edit_distance's scores: H = 5,113."""
    rng = np.random.default_rng(2505)
    m = 2556
    t = random_seq(m, rng)
    s = make_read(t, rng, 0.1).seq
    s = np.concatenate([s, random_seq(max(m - len(s), 0), rng)])[:m].astype(np.uint8)
    rs = RifrafSequence(s, np.full(m, -1.0), m, Scores.from_errors(ErrorModel(1.0, 1.0, 1.0)))
    assert 2 * m + 1 == 5113
    exp = [oracle_align(t, rs, m, skew=True)]
    assert exp[0][2] > 0
    both(engine, opts, [rs], [t], m, RF_SKEW, exp=exp)


def test_mixed_sizes(engine, opts):
    """130 pairs of mixed sizes in one call: more waves than one workgroup
    holds, and a last workgroup that is partly filled."""
    rng = np.random.default_rng(2506)
    seqs, tpls, bws = [], [], []
    for k in range(130):
        m = int(rng.integers(5, 700)) if k % 5 else int(rng.integers(1, 8))
        bw = int(rng.integers(1, 40))
        t = random_seq(m, rng)
        seqs.append(make_read(t, rng, 0.06, bw, REF_SCORES if k % 4 == 3 else SEQ_SCORES))
        tpls.append(t)
        bws.append(bw)
    exp = [oracle_align(t, s, bw) for t, s, bw in zip(tpls, seqs, bws)]
    both(engine, opts, seqs, tpls, bws, exp=exp)


def test_invalid_pair_and_null_outputs(engine, opts):
    """test_pair_align.test_invalid_pair_and_null_outputs' inputs: a read
    whose every fill raises between two good ones.  The NaN pair is not
    walked (-1, -1, no moves), its neighbours are exact, and the counts
    without a moves buffer are the same, under both walks."""
    rng = np.random.default_rng(2210)
    n = 9
    good = [RifrafSequence(random_seq(n, rng), np.log10(rng.uniform(0.01, 0.3, n)), 3, SEQ_SCORES) for _ in range(2)]
    bases = np.concatenate([good[0].seq, np.zeros(n, np.uint8), good[1].seq])
    off = np.array([0, n, 2 * n, 3 * n], np.int64)
    ninf = np.full(n, -np.inf)
    match = np.concatenate([good[0].match_scores, np.full(n, -0.01), good[1].match_scores])
    mism = np.concatenate([good[0].mismatch_scores, ninf, good[1].mismatch_scores])
    ins = np.concatenate([good[0].ins_scores, ninf, good[1].ins_scores])
    dele = np.concatenate([good[0].del_scores, np.full(n + 1, -np.inf), good[1].del_scores])
    engine.set_sequences_concat(0, bases, off, match, mism, ins, dele)
    tpls = [random_seq(n, rng), np.full(n, 1, np.uint8), random_seq(n + 2, rng)]
    engine.set_templates(0, tpls)
    raw = SimpleNamespace(seq=np.zeros(n, np.uint8), match_scores=np.full(n, -0.01), mismatch_scores=ninf,
                          ins_scores=ninf, del_scores=np.full(n + 1, -np.inf), codon_ins_scores=np.zeros(0),
                          codon_del_scores=np.zeros(0), bandwidth=3)
    with pytest.raises(oracle.OracleError):
        oracle.forward(tpls[1], raw)
    ids = np.array([0, 1, 2, 1], np.int32)
    bw = np.full(4, 3, np.int32)
    exp = [oracle_align(tpls[0], good[0], 3), oracle_align(tpls[2], good[1], 3)]
    lib, ctx = engine.lib, engine.ctx
    for w in WALKS:
        opts("pair_walk", w)
        sc, mv, ne = engine.pair_align(ids, ids, bw, caps=np.array([2 * n, 2 * n, 2 * n + 2, 2 * n]))
        assert np.isnan(sc[1]) and np.isnan(sc[3])
        assert mv[1] is None and mv[3] is None and ne[1] == -1 and ne[3] == -1
        for k, e in zip((0, 2), exp):
            assert sc[k] == e[0] and ne[k] == e[2]
            np.testing.assert_array_equal(mv[k], e[1])
        cnt = np.zeros(4, np.int32)
        assert lib.rf_pair_align(ctx, 4, ptr(ids), ptr(ids), ptr(bw), 0, None, None, None, None, ptr(cnt)) == 0
        assert list(cnt) == [exp[0][2], -1, exp[1][2], -1]
        assert lib.rf_pair_align(ctx, 4, ptr(ids), ptr(ids), ptr(bw), 0, None, None, None, ptr(cnt), None) == 0
        assert list(cnt) == [len(exp[0][1]), -1, len(exp[1][1]), -1]
