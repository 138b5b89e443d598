"""rf_pair_align_smart: smart_forward_moves! (src/model.jl:643-672) over
independent pairs, against the loop restated over the CPU oracle
(test_pair_align_smart_host.oracle_smart, pinned there against
model.smart_forward_moves) and against the slot path (rf_realign +
rf_backtrace per round).  Equality is exact: integer-equal moves, counts,
bandwidths and rounds, bit-equal scores.

Thresholds are inputs, so the stop reasons are forced: -1 (every count is
above), 10^9 (none is) and the Poisson values.  The pairs (smart_set) are the
issue's 40 (m 60-400, starting bandwidths 2-9, lean and codon reads with a
block insertion and a block deletion wider than the starting band) and four
short ones (n, m of 11-30 at bandwidth 9) that reach min(bw 2^k, m, n) through
m and through n."""
import numpy as np
import pytest

import oracle
from _util import REF_SCORES, SEQ_SCORES, random_seq
from rifraf_amd import RifrafSequence, assign, pairalign
from rifraf_amd._lib import ptr
from rifraf_amd.align import moves_to_aligned_seqs
from rifraf_amd.engine import RF_BWD, RF_FWD, Engine, RifrafError
from rifraf_amd.poisson import cquantile_poisson
from test_pair_align_smart_host import (ALWAYS, NEVER, dozen, indel_read, oracle_align, oracle_smart,
                                        poisson_thresholds, slot_smart, smart_set)

pytestmark = pytest.mark.gpu

DPW_LDS_H = pairalign.MAX_BAND_ROWS


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def check(got, exp, what=None):
    """got: Engine.pair_align_smart's five; exp: oracle_smart results."""
    scores, moves, nerr, bw, rounds = got
    assert len(scores) == len(exp)
    for k, e in enumerate(exp):
        tag = (k if what is None else what[k], e.why)
        assert bits(scores[k]) == bits(e.score), (tag, scores[k], e.score)
        assert (nerr[k], bw[k], rounds[k]) == (e.nerr, e.bw, e.rounds), (tag, nerr[k], bw[k], rounds[k], e)
        if moves is not None:
            if e.moves is None:
                assert moves[k] is None, tag
            else:
                assert moves[k] is not None, tag
                np.testing.assert_array_equal(moves[k], e.moves, err_msg=str(tag))


@pytest.fixture(scope="module")
def cases():
    """smart_set under the three threshold kinds: one flat list of pairs
    (indices into the set), their thresholds, and a memo of the oracle's
    fills shared by every test of this module."""
    seqs, tpls, bws, fixed = smart_set()
    n = len(seqs)
    idx = np.tile(np.arange(n), 3)
    thr = np.concatenate([np.full(n, ALWAYS), np.full(n, NEVER), poisson_thresholds(seqs)])
    return dict(seqs=seqs, tpls=tpls, bws=bws, fixed=fixed, idx=idx, thr=thr, memo={})


def expected(c, md):
    return [oracle_smart(c["tpls"][k], c["seqs"][k], int(c["bws"][k]), float(th), bool(c["fixed"][k]), md,
                         c["memo"], int(k)) for k, th in zip(c["idx"], c["thr"])]


def run(engine, c, md, **kw):
    engine.set_sequences(0, c["seqs"])
    engine.set_templates(0, c["tpls"])
    idx = c["idx"]
    return engine.pair_align_smart(idx, idx, c["bws"][idx], c["thr"], fixed=c["fixed"][idx], max_doublings=md, **kw)


# ---------------------------------------------------------------------
# 1. the inputs cover every way the loop ends
# ---------------------------------------------------------------------
def test_inputs_cover_the_loop(cases):
    exp = {md: expected(cases, md) for md in (0, 1, 5)}
    rounds = {e.rounds for e in exp[5]}
    assert {1, 2} <= rounds and max(rounds) >= 3, rounds
    why5 = {(e.why, e.cap if e.why == "max" else "") for e in exp[5]}
    assert {("below", ""), ("stalled", ""), ("fixed", ""), ("max", "m"), ("max", "n")} <= why5, why5
    assert ("max", "pow") in {(e.why, e.cap) for e in exp[1] if e.rounds == 2}
    assert all(e.rounds == 1 for e in exp[0])
    assert any(e.moves is not None and (e.moves >= 4).any() for e in exp[5]), "no codon move in the set"
    # the block indels are wider than the starting bands: doubling changes the alignment
    assert sum(e5.nerr < e0.nerr for e5, e0 in zip(exp[5], exp[0])) >= 20


# ---------------------------------------------------------------------
# 2. max_doublings 0, 1, 5 against the oracle
# ---------------------------------------------------------------------
@pytest.mark.parametrize("md", (0, 1, 5))
def test_against_the_oracle(engine, cases, md):
    got = run(engine, cases, md)
    check(got, expected(cases, md), cases["idx"])
    counts = run(engine, cases, md, want_moves=False)
    assert counts[1] is None
    for a, b in zip((got[0], got[2], got[3], got[4]), (counts[0], counts[2], counts[3], counts[4])):
        assert a.tobytes() == b.tobytes()
    if md == 0:
        idx = cases["idx"]
        plain = engine.pair_align(idx, idx, cases["bws"][idx])
        assert bits(plain[0]).tobytes() == bits(got[0]).tobytes()
        np.testing.assert_array_equal(plain[2], got[2])
        for a, b in zip(plain[1], got[1]):
            np.testing.assert_array_equal(a, b)
        assert (got[3] == cases["bws"][idx]).all() and (got[4] == 1).all()


def test_fixed_null_is_none_fixed(engine, cases):
    idx, thr = cases["idx"], cases["thr"]
    got = run(engine, cases, 5)
    free = engine.pair_align_smart(idx, idx, cases["bws"][idx], thr, fixed=None, max_doublings=5)
    exp = [oracle_smart(cases["tpls"][k], cases["seqs"][k], int(cases["bws"][k]), float(th), False, 5, cases["memo"],
                        int(k)) for k, th in zip(idx, thr)]
    check(free, exp, idx)
    assert (free[3] != got[3]).any()


# ---------------------------------------------------------------------
# 3. the slot path
# ---------------------------------------------------------------------
def test_agrees_with_the_slot_path(engine):
    """model.smart_forward_moves over rf_realign(RF_FWD) + rf_backtrace in a
    slot, pair by pair, and one rf_pair_align_smart call over the dozen."""
    pairs = dozen()
    slot = [slot_smart(engine, t, s, 0.1, fx) for t, s, _, fx in pairs]
    engine.set_sequences(0, [s for _, s, _, _ in pairs])
    engine.set_templates(0, [t for t, _, _, _ in pairs])
    ids = np.arange(len(pairs))
    thr = [cquantile_poisson(s.est_n_errors, 0.1) for _, s, _, _ in pairs]
    sc, _, ne, bw, rounds = engine.pair_align_smart(ids, ids, [b for _, _, b, _ in pairs], thr,
                                                    fixed=[fx for _, _, _, fx in pairs], want_moves=False)
    assert bw.tolist() == [x[0] for x in slot]
    assert bits(sc).tolist() == bits([x[1] for x in slot]).tolist()
    assert ne.tolist() == [x[2] for x in slot]
    assert max(rounds) >= 2


# ---------------------------------------------------------------------
# 4. a pair that becomes invalid when its band widens
# ---------------------------------------------------------------------
def test_invalid_in_round_two(engine):
    """n = m = 20 at bandwidth 2.  Read row 10 has -Inf mismatch, insertion
    and deletion scores, so a cell of that row is finite only where the
    template base equals the read's.  The template carries that base in
    columns 8-12 -- every cell of the row inside the band of bandwidth 2 --
    and another base elsewhere: the fill is valid at bandwidth 2 and raises
    at bandwidth 4, which the pair reaches in round 2."""
    rng = np.random.default_rng(2411)
    n = 20
    gt = [random_seq(80, rng) for _ in range(2)]
    good = [indel_read(t, rng, 3, SEQ_SCORES, 5) for t in gt]
    bad = RifrafSequence(random_seq(n, rng), np.log10(rng.uniform(0.01, 0.3, n)), 2, SEQ_SCORES)
    bad.seq[9] = 1
    bad.mismatch_scores = bad.mismatch_scores.copy()
    bad.ins_scores = bad.ins_scores.copy()
    bad.del_scores = bad.del_scores.copy()
    bad.mismatch_scores[9] = bad.ins_scores[9] = bad.del_scores[10] = -np.inf
    t = np.full(n, 2, np.uint8)
    t[7:12] = 1
    oracle_align(t, bad, 2)
    with pytest.raises(oracle.OracleError):
        oracle_align(t, bad, 4)
    seqs, tpls, bws = [good[0], bad, good[1]], [gt[0], t, gt[1]], [3, 2, 3]
    exp = [oracle_smart(tt, s, bw, ALWAYS, False) for tt, s, bw in zip(tpls, seqs, bws)]
    assert (exp[1].why, exp[1].bw, exp[1].rounds) == ("invalid", 4, 2)
    assert all(e.why != "invalid" and e.rounds >= 2 for e in (exp[0], exp[2]))
    engine.set_sequences(0, seqs)
    engine.set_templates(0, tpls)
    ids = np.arange(3)
    got = engine.pair_align_smart(ids, ids, bws, ALWAYS)
    assert np.isnan(got[0][1]) and got[1][1] is None and got[2][1] == -1
    check(got, exp)
    nm = np.zeros(3, np.int32)
    assert engine.lib.rf_pair_align_smart(engine.ctx, 3, ptr(ids.astype(np.int32)), ptr(ids.astype(np.int32)),
                                          ptr(np.array(bws, np.int32)), ptr(np.full(3, ALWAYS)), None, 5, 0, None,
                                          None, None, ptr(nm), None, None, None) == 0
    assert nm.tolist() == [len(exp[0].moves), -1, len(exp[2].moves)]


# ---------------------------------------------------------------------
# 5. argument errors
# ---------------------------------------------------------------------
def test_argument_errors(engine):
    rng = np.random.default_rng(2412)
    L = (DPW_LDS_H + 1 - 1) // 2          # n = m = L: 2 L + 1 = 5,115 rows at bandwidth L
    assert 2 * L + 1 == DPW_LDS_H + 1 == 5115
    small = RifrafSequence(random_seq(30, rng), np.full(30, -2.0), 3, SEQ_SCORES)
    wide = RifrafSequence(random_seq(L, rng), np.full(L, -2.0), 100, SEQ_SCORES)
    engine.set_sequences(0, [small, wide])
    engine.set_templates(0, [random_seq(30, rng), random_seq(L, rng)])
    ids = np.arange(2, dtype=np.int32)
    bws = np.array([3, 100], np.int32)
    thr = np.full(2, ALWAYS)
    lib, ctx = engine.lib, engine.ctx

    def raw(threshold, md, n=2):
        sc, nm, ne = np.full(2, 7.5), np.full(2, 77, np.int32), np.full(2, 77, np.int32)
        ob, rd = np.full(2, 77, np.int32), np.full(2, 77, np.int32)
        rc = lib.rf_pair_align_smart(ctx, n, ptr(ids), ptr(ids), ptr(bws), ptr(threshold), None, md, 0, ptr(sc), None,
                                     None, ptr(nm), ptr(ne), ptr(ob), ptr(rd))
        untouched = (sc == 7.5).all() and all((x == 77).all() for x in (nm, ne, ob, rd))
        return rc, untouched, lib.rf_last_error(ctx).decode()

    rc, untouched, msg = raw(None, 5)
    assert rc != 0 and untouched and "threshold" in msg
    rc, untouched, msg = raw(thr, 6)
    assert rc != 0 and untouched and "max_doublings" in msg
    rc, untouched, msg = raw(thr, -1)
    assert rc != 0 and untouched and "max_doublings" in msg
    # min(100 * 2^5, L, L) = L: 5,115 rows; refused before any launch
    rc, untouched, msg = raw(thr, 5)
    assert rc != 0 and untouched and "pair 1" in msg and "5115" in msg and str(DPW_LDS_H) in msg
    with pytest.raises(RifrafError) as err:
        engine.pair_align_smart(ids, ids, bws, thr)
    assert "pair 1" in str(err.value)
    # with 4 doublings the largest band is 2 * 1,600 + 1 rows, and the first pair alone is fine
    assert raw(thr, 5, n=1)[0] == 0
    rc, untouched, _ = raw(np.full(2, NEVER), 4)
    assert rc == 0 and not untouched
    for args, text in (((ids, ids, bws, thr, None, 5, RF_BWD), "RF_BWD"), (([1 << 20], [0], [3], [0.0]), "unknown"),
                       (([0], [0], [0], [0.0]), "bandwidth")):
        with pytest.raises(RifrafError) as err:
            engine.pair_align_smart(*args)
        assert text in str(err.value)


# ---------------------------------------------------------------------
# 6. engine state and device memory
# ---------------------------------------------------------------------
def test_state_untouched(engine, cases):
    rng = np.random.default_rng(2413)
    t = random_seq(90, rng)
    seqs = [indel_read(t, rng, 3, SEQ_SCORES, 5) for _ in range(4)]
    tpls = [t, random_seq(80, rng), random_seq(95, rng)]
    engine.set_sequences(0, seqs)
    engine.set_templates(0, tpls)
    ids = np.arange(4)
    engine.realign(ids, ids, 0, 3, RF_FWD | RF_BWD)
    before = engine.score_dense([ids])[0].copy()
    geo = [engine.geometry(int(k)) for k in ids]
    bands = [engine.download_band(int(k)).data.tobytes() for k in ids]
    got = engine.pair_align_smart(ids[:, None], np.arange(3)[None, :], 3, ALWAYS)
    check(got, [oracle_smart(tpls[j], s, 3, ALWAYS, False) for s in seqs for j in range(3)])
    assert max(got[4]) >= 3
    assert before.tobytes() == engine.score_dense([ids])[0].tobytes()   # still fresh: no refill asked for
    assert geo == [engine.geometry(int(k)) for k in ids]
    assert bands == [engine.download_band(int(k)).data.tobytes() for k in ids]
    moves, _ = engine.backtrace(ids)
    for k in ids:
        np.testing.assert_array_equal(moves[k], oracle_align(t, seqs[k], 3)[1])


def test_rounds_do_not_grow_device_memory():
    """2,000 pairs (20 pairs of 60 x 60 bases, 100 times each) that all take
    three rounds (bandwidths 3, 6, 12 with max_doublings = 2), in launch sets
    of 256: the device bytes after the call are those after a one-round call
    at the final bandwidth, and the chunked results are the unchunked ones."""
    rng = np.random.default_rng(2414)
    seqs, tpls, exp = [], [], []
    while len(seqs) < 20:
        t = random_seq(60, rng)
        s = t.copy()
        for i in rng.integers(0, 60, 3):
            s[i] = (s[i] + rng.integers(1, 4)) % 4
        a, b = int(rng.integers(8, 20)), int(rng.integers(30, 50))
        s = np.concatenate([s[:a], random_seq(5, rng), s[a:b], s[b + 5:]]).astype(np.uint8)
        rs = RifrafSequence(s, np.log10(rng.uniform(0.01, 0.3, 60)), 3, SEQ_SCORES)
        e = oracle_smart(t, rs, 3, ALWAYS, False, 2)
        if e.rounds == 3:
            seqs.append(rs)
            tpls.append(t)
            exp.append(e)
    assert all(e.bw == 12 for e in exp)
    idx = np.tile(np.arange(20), 100)
    caps = np.full(2000, 120)
    eng = Engine(0)
    try:
        eng.set_sequences(0, seqs)
        eng.set_templates(0, tpls)
        eng.set_option("pair_chunk", 256)
        one = eng.pair_align_smart(idx, idx, 12, ALWAYS, fixed=True, max_doublings=2, caps=caps)
        assert (one[4] == 1).all()
        bytes_one = eng.device_bytes()
        three = eng.pair_align_smart(idx, idx, 3, ALWAYS, max_doublings=2, caps=caps)
        assert eng.device_bytes() == bytes_one
        assert (three[4] == 3).all() and (three[3] == 12).all()
        eng.set_option("pair_chunk", 65536)
        whole = eng.pair_align_smart(idx, idx, 3, ALWAYS, max_doublings=2, caps=caps)
    finally:
        eng.close()
    check(tuple(x[:20] for x in three), exp)
    for a, b in zip(three, whole):
        if isinstance(a, list):
            assert len(a) == len(b)
            for x, y in zip(a, b):
                np.testing.assert_array_equal(x, y)
        else:
            assert a.tobytes() == b.tobytes()
    for k in range(20, 2000):
        np.testing.assert_array_equal(three[1][k], three[1][k % 20])


# ---------------------------------------------------------------------
# 7. the Python layer
# ---------------------------------------------------------------------
def test_smart_align_many(engine, cases):
    seqs, tpls = cases["seqs"], cases["tpls"]
    before = [(s.bandwidth, s.bandwidth_fixed) for s in seqs]
    got, bw = pairalign.smart_align_many(seqs, tpls, engine=engine)
    thr = poisson_thresholds(seqs)
    exp = [oracle_smart(t, s, s.bandwidth, th, s.bandwidth_fixed, 5, cases["memo"], k)
           for k, (t, s, th) in enumerate(zip(tpls, seqs, thr))]
    assert got == [moves_to_aligned_seqs(e.moves, t, s.seq) for e, t, s in zip(exp, tpls, seqs)]
    assert bw.tolist() == [e.bw for e in exp]
    assert (bw != cases["bws"]).any()
    assert before == [(s.bandwidth, s.bandwidth_fixed) for s in seqs]


def test_cross_scores_grid(engine):
    """6 reads x 4 templates: reads 0-2 come from template 0, reads 3-5 from
    template 1 (block indels wider than the starting bandwidth 3); every
    other cell is a read against a template it does not belong to."""
    rng = np.random.default_rng(2415)
    tpls = [random_seq(m, rng) for m in (120, 130, 110, 125)]
    seqs = [indel_read(tpls[k // 3], rng, 3, SEQ_SCORES, 5) for k in range(6)]
    before = [(s.bandwidth, s.bandwidth_fixed) for s in seqs]
    engine.set_sequences(0, seqs)
    engine.set_templates(0, tpls)
    today = engine.pair_scores(np.arange(6)[:, None], np.arange(4)[None, :], 3)
    plain = assign.cross_scores(seqs, tpls, engine=engine, bandwidth_pvalue=None)
    assert bits(plain).tobytes() == bits(today).tobytes()
    sc, bw = assign.cross_scores(seqs, tpls, engine=engine, bandwidth_pvalue=0.1, return_bandwidths=True)
    exp = [[oracle_smart(t, s, 3, cquantile_poisson(s.est_n_errors, 0.1), False) for t in tpls] for s in seqs]
    assert bits(sc).tolist() == bits([[e.score for e in row] for row in exp]).tolist()
    assert bw.tolist() == [[e.bw for e in row] for row in exp]
    off = [exp[r][j] for r in range(6) for j in range(4) if j != r // 3]
    assert any(e.rounds >= 2 for e in off), "no read / template mismatch that doubles"
    assert (sc >= plain).all() and (sc > plain).any()
    assert before == [(s.bandwidth, s.bandwidth_fixed) for s in seqs]
    picks = assign.choose_references([([s.seq for s in seqs[:3]], [np.full(len(s.seq), 20, np.int8) for s in seqs[:3]])],
                                     tpls, bandwidth=3, engine=engine, bandwidth_pvalue=0.1)
    assert picks[0][0] == 0
