"""rf_pair_align (k_pa / k_pa_gen / k_pa_walk): alignments of independent
(sequence, template) pairs from a 4-bit move trace, against the CPU oracle's
forward_moves! + backtrace + count_errors and against rf_realign(RF_FWD) +
rf_backtrace of the same pairs into slots.  Equality is exact: integer-equal
moves and counts, bit-equal scores (NaN where both are NaN).
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import oracle
from _util import REF_SCORES, SEQ_SCORES, make_read, random_seq
from rifraf_amd import DNASeq, RifrafSequence
import rifraf_amd.align as align_mod
from rifraf_amd import model, pairalign
from rifraf_amd.align import moves_to_aligned_seqs
from rifraf_amd.engine import RF_BWD, RF_FWD, RF_SKEW, RF_TRIM, RifrafError
from rifraf_amd.fastxio import read_fasta_records, read_fastq
from rifraf_amd.types import dna_str
from test_pair_scores import (DPW_LDS_H, GOLDEN1, LADDER_H, PS_CHUNK, SWEEP, _constant, bits_equal, final_cell,
                              random_read)
from test_small_geometry import NA, SHAPES, cls_of

pytestmark = pytest.mark.gpu

PA_TRACE_MB = _constant("PA_TRACE_MB")


def oracle_align(t, s, bw=None, skew=False, trim=False):
    """(score, moves, nerrors) of one pair from the oracle."""
    bw = s.bandwidth if bw is None else bw
    A, mv = oracle.forward(t, s, moves=True, skew=skew, trim=trim, bandwidth=bw)
    n, m = len(s.seq), len(t)
    w = oracle.backtrace(mv, n + 1, m + 1, bw)
    return final_cell(A, n, m, bw), w, oracle.count_errors(w, t, s.seq)


def check(got, exp, what=None):
    """got: Engine.pair_align's triple; exp: [(score, moves, nerrors)]."""
    scores, moves, nerr = got
    assert len(scores) == len(exp) == len(nerr)
    assert bits_equal(scores, [e[0] for e in exp]), [
        (k if what is None else what[k], scores[k], e[0]) for k, e in enumerate(exp) if not scores[k] == e[0]][:5]
    for k, e in enumerate(exp):
        tag = k if what is None else what[k]
        if moves is not None:
            assert moves[k] is not None, tag
            np.testing.assert_array_equal(moves[k], e[1], err_msg=str(tag))
        assert nerr[k] == e[2], (tag, nerr[k], e[2])


def run_pairs(engine, seqs, tpls, bws, flags=0, **kw):
    engine.set_sequences(0, seqs)
    engine.set_templates(0, tpls)
    ids = np.arange(len(seqs))
    return engine.pair_align(ids, ids, bws, flags, **kw)


# ---------------------------------------------------------------------
# 1. exhaustive small shapes
# ---------------------------------------------------------------------
@pytest.mark.parametrize("name,flags", SWEEP)
def test_sweep_small_shapes(engine, name, flags):
    c = cls_of(name)
    skew, trim = bool(flags & RF_SKEW), bool(flags & RF_TRIM)
    got = run_pairs(engine, c.seqs, c.templates, c.bws, flags)
    fills, walks = c.fills(skew, trim), c.walks(skew, trim)
    exp = [(final_cell(fills[k][0], n, m, bw), walks[k][0], walks[k][1]) for k, (m, n, bw) in enumerate(SHAPES)]
    assert len(exp) == NA
    check(got, exp, SHAPES)


# ---------------------------------------------------------------------
# 2. width ladder
# ---------------------------------------------------------------------
def test_width_ladder(engine):
    """m = 12, bw = 2 and every tier edge of test_pair_scores.LADDER_H, n and
    m swapped, reads with and without codon tables, one call."""
    rng = np.random.default_rng(2201)
    seqs, tpls, what = [], [], []
    for H in LADDER_H:
        short, long_ = 12, 12 + H - 5
        for n, m in ((long_, short), (short, long_)):
            for scores in (SEQ_SCORES, REF_SCORES):
                seqs.append(random_read(n, 2, rng, scores))
                tpls.append(random_seq(m, rng))
                what.append((H, n, m, scores is REF_SCORES))
    got = run_pairs(engine, seqs, tpls, 2)
    check(got, [oracle_align(t, s) for t, s in zip(tpls, seqs)], what)


def test_scores_and_align_share_the_fill(engine):
    """pair_scores and pair_align run one recurrence in every class: n == m
    pairs on each side of every fast-tier threshold (H = 2 bw + 1 = 31 / 33,
    63 / 65, 127 / 129, 255 / 257; the last takes the general tier), reads a
    few edits from templates of 3 H bases (two or more lean-interior blocks),
    and one read with codon tables (general tier).  One call each: the score
    bits are equal, and moves, scores and error counts are the oracle's."""
    rng = np.random.default_rng(2210)
    seqs, tpls, bws, what = [], [], [], []

    def add(m, bw, scores):
        t = random_seq(m, rng)
        s = t.copy()
        for i in rng.integers(0, m, 3):   # substitutions, then one deletion and one insertion: n == m
            s[i] = (s[i] + rng.integers(1, 4)) % 4
        s = np.delete(s, rng.integers(0, m))
        s = np.insert(s, rng.integers(0, m), rng.integers(0, 4)).astype(np.uint8)
        seqs.append(RifrafSequence(s, np.log10(rng.uniform(0.01, 0.3, m)), bw, scores))
        tpls.append(t)
        bws.append(bw)
        what.append((m, bw, scores is REF_SCORES))

    for bw in (15, 16, 31, 32, 63, 64, 127, 128):
        add(3 * (2 * bw + 1), bw, SEQ_SCORES)
    add(99, 16, REF_SCORES)
    engine.set_sequences(0, seqs)
    engine.set_templates(0, tpls)
    ids = np.arange(len(seqs))
    scores = engine.pair_scores(ids, ids, bws)
    got = engine.pair_align(ids, ids, bws)
    assert np.array_equal(np.asarray(scores).view(np.int64), np.asarray(got[0]).view(np.int64)), (scores, got[0])
    check(got, [oracle_align(t, s, bw) for t, s, bw in zip(tpls, seqs, bws)], what)


# ---------------------------------------------------------------------
# 3. trace-word edges
# ---------------------------------------------------------------------
def test_trace_word_edges(engine):
    """n, m in {14..18, 30..34, 47..49}, |n - m| <= 3, bw 1, 2, 3, 9: the
    number of periods lands on, below and above multiples of 16; lean and
    codon reads (codon moves cross word boundaries)."""
    rng = np.random.default_rng(2202)
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
    got = run_pairs(engine, seqs, tpls, bws)
    exp = [oracle_align(t, s) for t, s in zip(tpls, seqs)]
    assert any((e[1] >= 4).any() for e in exp), "no codon move in the set"
    check(got, exp, what)


# ---------------------------------------------------------------------
# 4. long pairs
# ---------------------------------------------------------------------
def test_long_pairs(engine):
    """test_pair_scores.test_long_pairs' shapes, against the oracle and
    against realign(RF_FWD) + backtrace of the same pairs into slots."""
    rng = np.random.default_rng(2203)
    L = (63, 64, 65, 255, 256, 257, 600, 1100)
    shapes = [(n, m) for n in L for m in L if abs(n - m) <= 40]
    seqs, tpls = [], []
    for scores in (SEQ_SCORES, REF_SCORES):
        for n, m in shapes:
            t = random_seq(m, rng)
            r = make_read(t, rng, 0.05, 9, scores)
            s = np.concatenate([r.seq, random_seq(max(n - len(r.seq), 0), rng)])[:n]
            seqs.append(RifrafSequence(s, np.log10(rng.uniform(0.01, 0.3, n)), 9, scores))
            tpls.append(t)
    got = run_pairs(engine, seqs, tpls, 9)
    check(got, [oracle_align(t, s) for t, s in zip(tpls, seqs)], shapes + shapes)
    ids = np.arange(len(seqs))
    filled = engine.realign(ids, ids, ids, 9, RF_FWD)
    assert bits_equal(got[0], filled)
    moves, nerr = engine.backtrace(ids)
    for k in ids:
        np.testing.assert_array_equal(got[1][k], moves[k])
    np.testing.assert_array_equal(got[2], nerr)


# ---------------------------------------------------------------------
# 5. edit distances
# ---------------------------------------------------------------------
def test_edit_distances(engine):
    """6 pairs of 200..400 bases: H = min + 1 + |n - m| (general tier,
    skewed), against align.edit_distance pair by pair."""
    rng = np.random.default_rng(2204)
    tpls = [random_seq(m, rng) for m in (200, 251, 300, 333, 380, 400)]
    seqs = [make_read(t, rng, 0.1).seq for t in tpls]
    seqs[1] = seqs[1][:210]
    got = pairalign.edit_distances(tpls, seqs, engine=engine)
    exp = [align_mod.edit_distance(t, s, scratch=align_mod.Scratch(engine)) for t, s in zip(tpls, seqs)]
    np.testing.assert_array_equal(got, exp)
    assert min(exp) > 0


# ---------------------------------------------------------------------
# 6. grid and order
# ---------------------------------------------------------------------
def test_grid_and_order(engine):
    rng = np.random.default_rng(2205)
    tpls = [random_seq(m, rng) for m in (40, 50, 57, 64, 90)]
    seqs = [make_read(tpls[k % 5], rng, 0.05, 3 + k % 7) for k in range(48)]
    r, j = np.divmod(np.arange(240), 5)
    pairs = np.stack([r, j], 1)
    grid = pairalign.align_moves_many(seqs, tpls, pairs=pairs, engine=engine)
    exp = [oracle_align(tpls[b], seqs[a])[1] for a, b in pairs]
    for k in range(240):
        np.testing.assert_array_equal(grid[k], exp[k], err_msg=str(pairs[k]))
    perm = rng.permutation(240)
    shuffled = pairalign.align_moves_many(seqs, tpls, pairs=pairs[perm], engine=engine)
    for k, p in enumerate(perm):
        np.testing.assert_array_equal(shuffled[k], grid[p])
    # the sequences and templates are on the engine as ids 0..: single-pair calls
    for k, (a, b) in enumerate(pairs):
        sc, mv, ne = engine.pair_align([a], [b], [seqs[a].bandwidth])
        np.testing.assert_array_equal(mv[0], grid[k])


# ---------------------------------------------------------------------
# 7. engine state
# ---------------------------------------------------------------------
def test_state_untouched(engine):
    rng = np.random.default_rng(2206)
    tpls = [random_seq(m, rng) for m in (80, 70, 95)]
    seqs = [make_read(tpls[0], rng, 0.03, 9) for _ in range(4)]
    engine.set_sequences(0, seqs)
    engine.set_templates(0, tpls)
    ids = np.arange(4)
    engine.realign(ids, ids, 0, 9, RF_FWD | RF_BWD)
    before = engine.score_dense([ids])[0].copy()
    geo = [engine.geometry(int(k)) for k in ids]
    got = engine.pair_align(ids[:, None], np.array([1, 2])[None, :], 9)
    check(got, [oracle_align(tpls[j], s) for s in seqs for j in (1, 2)])
    after = engine.score_dense([ids])[0]
    assert before.tobytes() == after.tobytes()
    assert geo == [engine.geometry(int(k)) for k in ids]
    moves, _ = engine.backtrace(ids)
    for k in ids:
        np.testing.assert_array_equal(moves[k], oracle_align(tpls[0], seqs[k])[1])


# ---------------------------------------------------------------------
# 8. memory
# ---------------------------------------------------------------------
def test_device_memory_stays_small(engine):
    """4,096 pairs of 300 x 300 at bw 9: the call allocates less than one
    eighth of the bytes their A bands would take."""
    rng = np.random.default_rng(2207)
    tpls = [random_seq(300, rng) for _ in range(64)]
    seqs = [make_read(tpls[k], rng, 0.03, 9) for k in range(64)]
    seqs = [RifrafSequence(np.concatenate([s.seq, random_seq(300, rng)])[:300],
                           np.log10(rng.uniform(0.01, 0.3, 300)), 9, SEQ_SCORES) for s in seqs]
    engine.set_sequences(0, seqs)
    engine.set_templates(0, tpls)
    before = engine.device_bytes()
    sc, moves, nerr = engine.pair_align(np.arange(64)[:, None], np.arange(64)[None, :], 9,
                                        caps=np.full(4096, 600))
    grown = engine.device_bytes() - before
    bands = 4096 * (2 * 9 + 1) * 301 * 8
    print(f"device bytes grown by {grown}; the bands would take {bands}")
    assert 0 <= grown < bands // 8
    pick = [(0, 0), (63, 0), (17, 42), (63, 63)]
    got = ([sc[r * 64 + j] for r, j in pick], [moves[r * 64 + j] for r, j in pick],
           [nerr[r * 64 + j] for r, j in pick])
    check(got, [oracle_align(tpls[j], seqs[r]) for r, j in pick], pick)


# ---------------------------------------------------------------------
# 9. chunking
# ---------------------------------------------------------------------
def _same(a, b):
    assert bits_equal(a[0], b[0])
    assert len(a[1]) == len(b[1])
    for x, y in zip(a[1], b[1]):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(a[2], b[2])


def _join(a, b):
    return np.concatenate([a[0], b[0]]), a[1] + b[1], np.concatenate([a[2], b[2]])


def test_chunked_by_pairs(engine, opts):
    assert engine.get_option("pair_chunk") == PS_CHUNK
    c = cls_of("seq")
    engine.set_sequences(0, c.seqs[:50])
    engine.set_templates(0, c.templates[:7])
    seq, tpl = np.arange(50), np.arange(50) % 7
    whole = engine.pair_align(seq, tpl, 3)
    opts("pair_chunk", 32)
    chunked = engine.pair_align(seq, tpl, 3)
    halves = _join(engine.pair_align(seq[:25], tpl[:25], 3), engine.pair_align(seq[25:], tpl[25:], 3))
    _same(chunked, halves)
    _same(chunked, whole)
    check(chunked, [oracle_align(c.templates[j], c.seqs[k], 3) for k, j in zip(seq, tpl)])


def test_chunked_by_trace(engine, opts):
    """pair_trace_mb = 1 with traces of more than 1 MB in all, one pair alone
    above 1 MB (4000 x 4000 at bw 250: 266 blocks x 502 words x 8 B)."""
    assert engine.get_option("pair_trace_mb") == PA_TRACE_MB
    rng = np.random.default_rng(2208)
    lens = [1000] * 10 + [4000] + [1000] * 10
    bws = [60] * 10 + [250] + [60] * 10
    tpls = [random_seq(m, rng) for m in lens]
    seqs = [make_read(t, rng, 0.04, bw) for t, bw in zip(tpls, bws)]
    words = [(((2 * bw + abs(len(s) - len(t)) + 1 + 2 * len(t) + 1) // 2 + 15) // 16) *
             ((2 * bw + abs(len(s) - len(t)) + 1 + 1) & ~1) for s, t, bw in zip(seqs, tpls, bws)]
    assert words[10] * 8 > 1 << 20 and sum(words) * 8 - words[10] * 8 > 1 << 20
    whole = run_pairs(engine, seqs, tpls, bws)
    opts("pair_trace_mb", 1)
    ids = np.arange(len(seqs))
    chunked = engine.pair_align(ids, ids, bws)
    halves = _join(engine.pair_align(ids[:10], ids[:10], bws[:10]), engine.pair_align(ids[10:], ids[10:], bws[10:]))
    _same(chunked, whole)
    _same(chunked, halves)
    check(chunked, [oracle_align(t, s) for t, s in zip(tpls, seqs)])


# ---------------------------------------------------------------------
# 10. errors, NaN pairs, NULL outputs
# ---------------------------------------------------------------------
def test_errors(engine):
    rng = np.random.default_rng(2209)
    engine.set_sequences(0, [random_read(12, 2, rng)])
    engine.set_templates(0, [random_seq(12, rng), random_seq(12 + DPW_LDS_H + 1 - 5, rng)])
    assert engine.pair_align([0], [0], [2], RF_FWD)[0].shape == (1,)      # RF_FWD is accepted
    for args, text in ((([0], [0], [2], RF_BWD), "RF_BWD"), (([0], [0], [2], RF_FWD | RF_BWD), "RF_BWD"),
                       (([1 << 20], [0], [2]), "unknown"), (([0], [1 << 20], [2]), "unknown"),
                       (([-1], [0], [2]), "unknown"), (([0], [0], [0]), "bandwidth"),
                       (([0], [1], [2]), str(DPW_LDS_H))):
        with pytest.raises(RifrafError) as err:
            engine.pair_align(*args)
        assert text in str(err.value), (args, str(err.value))
    with pytest.raises(RifrafError) as err:
        pairalign.align_moves_many([random_read(12, 2, rng)], [random_seq(12 + DPW_LDS_H + 1 - 5, rng)],
                                   engine=engine)
    assert "pair 0" in str(err.value)


def test_invalid_pair_and_null_outputs(engine):
    """test_pair_scores.test_invalid_pair_is_nan's read: NaN, -1, -1 and no
    moves beside exact neighbours; then every NULL-output combination."""
    from rifraf_amd._lib import ptr
    rng = np.random.default_rng(2210)
    n = 9
    good = [random_read(n, 3, rng) for _ in range(2)]
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
    exp = [oracle_align(tpls[0], good[0]), oracle_align(tpls[2], good[1])]
    for caps in (None, np.array([2 * n, 2 * n, 2 * n + 2, 2 * n])):
        sc, mv, ne = engine.pair_align(ids, ids, bw, caps=caps)
        assert np.isnan(sc[1]) and np.isnan(sc[3])
        assert mv[1] is None and mv[3] is None and ne[1] == -1 and ne[3] == -1
        check((sc[[0, 2]], [mv[0], mv[2]], ne[[0, 2]]), exp)
    # want_moves=False
    sc, mv, ne = engine.pair_align(ids, ids, bw, want_moves=False)
    assert mv is None and np.isnan(sc[1]) and list(ne) == [exp[0][2], -1, exp[1][2], -1]
    # scores only / nerrors only / nmoves only, straight through the C ABI
    lib, ctx = engine.lib, engine.ctx
    out = np.zeros(4)
    assert lib.rf_pair_align(ctx, 4, ptr(ids), ptr(ids), ptr(bw), 0, ptr(out), None, None, None, None) == 0
    assert bits_equal(out[[0, 2]], [exp[0][0], exp[1][0]]) and np.isnan(out[1])
    assert bits_equal(out, engine.pair_scores(ids, ids, bw))
    cnt = np.zeros(4, np.int32)
    assert lib.rf_pair_align(ctx, 4, ptr(ids), ptr(ids), ptr(bw), 0, None, None, None, None, ptr(cnt)) == 0
    assert list(cnt) == [exp[0][2], -1, exp[1][2], -1]
    assert lib.rf_pair_align(ctx, 4, ptr(ids), ptr(ids), ptr(bw), 0, None, None, None, ptr(cnt), None) == 0
    assert list(cnt) == [len(exp[0][1]), -1, len(exp[1][1]), -1]
    # moves without moves_off is refused
    buf = np.zeros(64, np.int8)
    assert lib.rf_pair_align(ctx, 4, ptr(ids), ptr(ids), ptr(bw), 0, None, ptr(buf), None, None, None) != 0
    fill, walk = engine.last_pair_align_ms()
    assert fill >= 0 and walk >= 0


# ---------------------------------------------------------------------
# 11. correct_shifts and the golden reads
# ---------------------------------------------------------------------
SHIFT_KATS = [("TTTT", "TTT", "TTT"), ("TT", "TTT", "TTT"), ("TTTACCC", "TTTCGC", "TTTCCC"),
              ("TTTAAACCC", "TTTCGC", "TTTAAACCC")]   # test_frame_helpers.py / test_correct_shifts.jl:8-35


def test_correct_shifts_many(engine):
    cons = [DNASeq(c) for c, _, _ in SHIFT_KATS]
    refs = [DNASeq(r) for _, r, _ in SHIFT_KATS]
    got = pairalign.correct_shifts_many(cons, refs, engine=engine)
    assert [dna_str(g) for g in got] == [e for _, _, e in SHIFT_KATS]
    one = [dna_str(model.correct_shifts(c, r, engine=engine)) for c, r in zip(cons, refs)]
    assert one == [e for _, _, e in SHIFT_KATS]
    # one reference for all
    same_ref = pairalign.correct_shifts_many(cons[2:], refs[2], engine=engine)
    assert [dna_str(g) for g in same_ref] == ["TTTCCC", "TTTAAACCC"]


def test_align_many_golden(engine):
    """The golden config-1 reads against their golden consensus."""
    cons = dict(read_fasta_records(os.path.join(GOLDEN1, "consensus-results.fasta")))
    for f in ("input-reads-1.fastq", "input-reads-2.fastq"):
        reads, phreds, _ = read_fastq(os.path.join(GOLDEN1, f))
        t = DNASeq(cons[f])
        seqs = [RifrafSequence(s, np.asarray(p, np.int8), 9, SEQ_SCORES) for s, p in zip(reads, phreds)]
        got = pairalign.align_many(seqs, [t], pairs=[(k, 0) for k in range(len(seqs))], engine=engine)
        exp = [moves_to_aligned_seqs(oracle_align(t, s)[1], t, s.seq) for s in seqs]
        assert got == exp
