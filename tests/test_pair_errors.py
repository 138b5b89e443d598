"""rf_pair_errors: score, count_errors and the band doubling of
smart_forward_moves! (src/model.jl:643-672) of independent pairs with the
error count carried through the fill (k_pe / k_pe_gen) -- no move trace, no
walk -- against the CPU oracle (forward_moves! + backtrace + count_errors,
and test_pair_align_smart_host.oracle_smart for the loop), against
rf_pair_align / rf_pair_align_smart on the same engine, and rf_pair_scores'
bits.  Equality is exact: bit-equal scores, integer-equal counts, bandwidths
and rounds."""
import os
import re

import numpy as np
import pytest

import oracle
from _util import REF_SCORES, SEQ_SCORES, make_read, random_seq
from rifraf_amd import RifrafSequence, assign, pairalign
from rifraf_amd._lib import ptr
from rifraf_amd.engine import RF_BWD, RF_FWD, RF_SKEW, RF_TRIM, Engine
from test_pair_align_smart_host import (ALWAYS, NEVER, indel_read, oracle_align, oracle_smart, poisson_thresholds,
                                        smart_set)

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _constant(name, file="rifraf_hip.hip"):
    src = open(os.path.join(REPO, "rifraf.jl_amd", "csrc", file)).read()
    expr = re.search(r"constexpr int %s = ([0-9 */+()-]+);" % name, src).group(1)
    return int(eval(expr.replace("/", "//"), {"__builtins__": {}}))


PS_FAST_H = _constant("PS_FAST_H")
PS_GEN64_H = _constant("PS_GEN64_H")
DPW_LDS_H = _constant("DPW_LDS_H")
COUNT_H = _constant("DP_COUNT_H", "rifraf_dp_plan.h")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def against_oracle(got, tpls, seqs, bws, skew=False, trim=False, what=None):
    """got: (scores, nerrors, ...) of Engine.pair_errors over pairs k with k."""
    for k, (t, s, bw) in enumerate(zip(tpls, seqs, bws)):
        try:
            score, _, nerr = oracle_align(t, s, int(bw), skew=skew, trim=trim)
        except oracle.OracleError:
            score, nerr = np.nan, -1
        tag = (k if what is None else what[k], len(s.seq), len(t), int(bw), skew, trim)
        assert bits(got[0][k]) == bits(score) or (np.isnan(score) and np.isnan(got[0][k])), (tag, got[0][k], score)
        assert got[1][k] == nerr, (tag, got[1][k], nerr)


# ---------------------------------------------------------------------
# 1. small shapes
# ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    """All n, m in 1..8 at bandwidths 1, 2, 3: two letters and one Phred, so
    nearly every cell has tied candidates."""
    rng = np.random.default_rng(2601)
    seqs, tpls, bws = [], [], []
    for n in range(1, 9):
        for m in range(1, 9):
            for bw in (1, 2, 3):
                seqs.append(RifrafSequence(rng.integers(0, 2, n).astype(np.uint8), np.full(n, -1.0), bw, SEQ_SCORES))
                tpls.append(rng.integers(0, 2, m).astype(np.uint8))
                bws.append(bw)
    return seqs, tpls, np.array(bws, np.int32)


@pytest.mark.parametrize("flags", (0, RF_SKEW, RF_TRIM))
def test_small_shapes(engine, small, flags):
    seqs, tpls, bws = small
    engine.set_sequences(0, seqs)
    engine.set_templates(0, tpls)
    ids = np.arange(len(seqs))
    got = engine.pair_errors(ids, ids, bws, flags=flags)
    against_oracle(got, tpls, seqs, bws, skew=bool(flags & RF_SKEW), trim=bool(flags & RF_TRIM))
    assert (got[2] == bws).all() and (got[3] == 1).all()


# ---------------------------------------------------------------------
# 2. the fast tier: every class, borders and lean interiors
# ---------------------------------------------------------------------
def test_fast_tier_classes(engine):
    """H on both sides of 31/32, 63/64, 127/128 and 255/256 (bw = (H - 1) // 2,
    |n - m| = (H - 1) % 2), five template lengths 40-400 per H, shuffled, so
    that the four tasks of a wave differ in klo / khi, and no class holds a
    multiple of four pairs (5, 10, 10, 10 and the general tier's 5): padding
    tasks run."""
    rng = np.random.default_rng(2602)
    seqs, tpls, bws, what = [], [], [], []
    for H in (31, 32, 63, 64, 127, 128, PS_FAST_H, PS_FAST_H + 1):
        for m in (40, 77, 161, 290, 400):
            t = random_seq(m, rng)
            r = make_read(t, rng, 0.05, 9, SEQ_SCORES)
            n = m + (H - 1) % 2
            s = np.concatenate([r.seq, random_seq(max(n - len(r.seq), 0), rng)])[:n].astype(np.uint8)
            seqs.append(RifrafSequence(s, np.log10(rng.uniform(0.01, 0.3, n)), 9, SEQ_SCORES))
            tpls.append(t)
            bws.append((H - 1) // 2)
            what.append((H, m))
    order = rng.permutation(len(seqs))
    seqs, tpls, what = [seqs[k] for k in order], [tpls[k] for k in order], [what[k] for k in order]
    bws = np.array(bws, np.int32)[order]
    assert all(2 * b + abs(len(s.seq) - len(t)) + 1 == w[0] for b, s, t, w in zip(bws, seqs, tpls, what))
    engine.set_sequences(0, seqs)
    engine.set_templates(0, tpls)
    ids = np.arange(len(seqs))
    got = engine.pair_errors(ids, ids, bws)
    against_oracle(got, tpls, seqs, bws, what=what)
    plain = engine.pair_align(ids, ids, bws, want_moves=False)
    assert got[1].tobytes() == plain[2].tobytes()
    assert bits(got[0]).tobytes() == bits(engine.pair_scores(ids, ids, bws)).tobytes()
    assert got[1].max() > 5


# ---------------------------------------------------------------------
# 3. the general tier
# ---------------------------------------------------------------------
def bad_pair(rng):
    """n = m = 20: a -Inf mismatch, insertion and deletion entry in read row
    10; valid at bandwidth 2, "new score is invalid" at 4
    (test_pair_align_smart.test_invalid_in_round_two)."""
    n = 20
    bad = RifrafSequence(random_seq(n, rng), np.log10(rng.uniform(0.01, 0.3, n)), 2, SEQ_SCORES)
    bad.seq[9] = 1
    for name in ("mismatch_scores", "ins_scores", "del_scores"):
        setattr(bad, name, getattr(bad, name).copy())
    bad.mismatch_scores[9] = bad.ins_scores[9] = bad.del_scores[10] = -np.inf
    t = np.full(n, 2, np.uint8)
    t[7:12] = 1
    return t, bad


@pytest.mark.parametrize("flags", (0, RF_SKEW, RF_TRIM, RF_SKEW | RF_TRIM))
def test_general_tier(engine, flags):
    """Codon reads with a codon-sized block insertion and deletion (m 30-300,
    bandwidths 3-40), lean reads that the flags send to the general tier, and the pair with a -Inf table entry at both
    bandwidths between them."""
    rng = np.random.default_rng(2603)
    seqs, tpls, bws = [], [], []
    for k, m in enumerate((30, 64, 65, 131, 300, 47, 200)):
        t = random_seq(m, rng)
        bw = (3, 9, 40)[k % 3]
        seqs.append(indel_read(t, rng, bw, REF_SCORES if k % 2 == 0 else SEQ_SCORES, 3, rate=0.05))
        tpls.append(t)
        bws.append(bw)
    t, bad = bad_pair(rng)
    for at, bw in ((2, 2), (5, 4)):
        seqs.insert(at, bad)
        tpls.insert(at, t)
        bws.insert(at, bw)
    bws = np.array(bws, np.int32)
    engine.set_sequences(0, seqs)
    engine.set_templates(0, tpls)
    ids = np.arange(len(seqs))
    got = engine.pair_errors(ids, ids, bws, flags=flags)
    against_oracle(got, tpls, seqs, bws, skew=bool(flags & RF_SKEW), trim=bool(flags & RF_TRIM))
    assert np.isnan(got[0][5]) and got[1][5] == -1 and not np.isnan(got[0][2])
    assert np.isnan(got[0]).sum() == 1 and (np.delete(got[1], 5) >= 0).all()
    plain = engine.pair_align(ids, ids, bws, flags, want_moves=False)
    assert got[1].tobytes() == plain[2].tobytes() and bits(got[0]).tobytes() == bits(plain[0]).tobytes()
    if flags == 0:
        codon = [oracle_align(t, s, int(b))[1] for t, s, b in zip(tpls, seqs, bws) if len(s.codon_ins_scores)]
        assert len(codon) == 4 and all((mv >= 4).any() for mv in codon), "a codon read without a codon move"


def test_general_tier_limits(engine):
    """The one-wave boundary (H = PS_GEN64_H, + 1) and the two-ring limit
    (H = DP_COUNT_H, + 1: the pair above it takes the trace fill and the
    walk inside the same call).  The smallest sequences that reach each H:
    12 bases against 12 + H - 5 at bandwidth 2, both ways round, with and
    without codon tables (test_pair_scores' ladder)."""
    rng = np.random.default_rng(2604)
    assert 48 * (COUNT_H + 6) <= 160 * 1024 < 48 * (COUNT_H + 7) and PS_GEN64_H < COUNT_H < DPW_LDS_H
    seqs, tpls, what = [], [], []
    for H in (PS_GEN64_H, PS_GEN64_H + 1, COUNT_H, COUNT_H + 1):
        for n, m in ((12 + H - 5, 12), (12, 12 + H - 5)):
            for scores in (SEQ_SCORES, REF_SCORES):
                seqs.append(RifrafSequence(random_seq(n, rng), np.log10(rng.uniform(0.01, 0.3, n)), 2, scores))
                tpls.append(random_seq(m, rng))
                what.append(H)
    assert all(2 * 2 + abs(len(s.seq) - len(t)) + 1 == H for s, t, H in zip(seqs, tpls, what))
    engine.set_sequences(0, seqs)
    engine.set_templates(0, tpls)
    ids = np.arange(len(seqs))
    bws = np.full(len(seqs), 2, np.int32)
    fw = engine.last_pair_align_ms()
    got = engine.pair_errors(ids, ids, bws)
    against_oracle(got, tpls, seqs, bws, what=what)
    assert engine.last_pair_align_ms() == fw and engine.last_pair_errors_ms() > 0
    plain = engine.pair_align(ids, ids, bws, want_moves=False)
    assert got[1].tobytes() == plain[2].tobytes() and bits(got[0]).tobytes() == bits(plain[0]).tobytes()


# ---------------------------------------------------------------------
# 4. the smart loop
# ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    """test_pair_align_smart's: smart_set under the three threshold kinds."""
    seqs, tpls, bws, fixed = smart_set()
    n = len(seqs)
    idx = np.tile(np.arange(n), 3)
    thr = np.concatenate([np.full(n, ALWAYS), np.full(n, NEVER), poisson_thresholds(seqs)])
    return dict(seqs=seqs, tpls=tpls, bws=bws, fixed=fixed, idx=idx, thr=thr, memo={})


def expected(c, md):
    return [oracle_smart(c["tpls"][k], c["seqs"][k], int(c["bws"][k]), float(th), bool(c["fixed"][k]), md,
                         c["memo"], int(k)) for k, th in zip(c["idx"], c["thr"])]


def check_smart(got, exp, what):
    scores, nerr, bw, rounds = got
    assert len(scores) == len(exp)
    for k, e in enumerate(exp):
        tag = (what[k], e.why)
        assert bits(scores[k]) == bits(e.score), (tag, scores[k], e.score)
        assert (nerr[k], bw[k], rounds[k]) == (e.nerr, e.bw, e.rounds), (tag, nerr[k], bw[k], rounds[k], e)


def test_inputs_cover_every_stop(cases):
    exp = {md: expected(cases, md) for md in (0, 1, 5)}
    why5 = {(e.why, e.cap if e.why == "max" else "") for e in exp[5]}
    assert {("below", ""), ("stalled", ""), ("fixed", ""), ("max", "m"), ("max", "n")} <= why5, why5
    assert ("max", "pow") in {(e.why, e.cap) for e in exp[1] if e.rounds == 2}
    assert all(e.rounds == 1 for e in exp[0]) and max(e.rounds for e in exp[5]) >= 3


@pytest.mark.parametrize("md", (0, 1, 5))
def test_smart_loop(engine, cases, md):
    c = cases
    engine.set_sequences(0, c["seqs"])
    engine.set_templates(0, c["tpls"])
    idx = c["idx"]
    got = engine.pair_errors(idx, idx, c["bws"][idx], c["thr"], fixed=c["fixed"][idx], max_doublings=md)
    check_smart(got, expected(c, md), idx)
    walked = engine.pair_align_smart(idx, idx, c["bws"][idx], c["thr"], fixed=c["fixed"][idx], max_doublings=md,
                                     want_moves=False)
    for a, b in zip(got, (walked[0], walked[2], walked[3], walked[4])):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    if md == 0:
        free = engine.pair_errors(idx, idx, c["bws"][idx])   # threshold may be NULL
        for a, b in zip(got, free):
            assert a.tobytes() == b.tobytes()


def test_invalid_in_round_two(engine):
    rng = np.random.default_rng(2411)
    gt = [random_seq(80, rng) for _ in range(2)]
    good = [indel_read(t, rng, 3, SEQ_SCORES, 5) for t in gt]
    t, bad = bad_pair(rng)
    seqs, tpls, bws = [good[0], bad, good[1]], [gt[0], t, gt[1]], [3, 2, 3]
    exp = [oracle_smart(tt, s, bw, ALWAYS, False) for tt, s, bw in zip(tpls, seqs, bws)]
    assert (exp[1].why, exp[1].bw, exp[1].rounds) == ("invalid", 4, 2)
    engine.set_sequences(0, seqs)
    engine.set_templates(0, tpls)
    ids = np.arange(3)
    got = engine.pair_errors(ids, ids, bws, ALWAYS, max_doublings=5)
    assert np.isnan(got[0][1]) and got[1][1] == -1 and got[2][1] == 4
    check_smart(got, exp, ids)


# ---------------------------------------------------------------------
# 5. launch sets, device memory and engine state
# ---------------------------------------------------------------------
def test_small_chunks_give_the_same(engine, opts, cases):
    c = cases
    engine.set_sequences(0, c["seqs"])
    engine.set_templates(0, c["tpls"])
    idx = c["idx"]
    args = (idx, idx, c["bws"][idx], c["thr"])
    whole = engine.pair_errors(*args, fixed=c["fixed"][idx], max_doublings=5)
    opts("pair_chunk", 7)
    sets = engine.pair_errors(*args, fixed=c["fixed"][idx], max_doublings=5)
    for a, b in zip(whole, sets):
        assert a.tobytes() == b.tobytes()


def trace_bytes(seqs, tpls, bws):
    """The trace of one launch set (rifraf_dp_plan.h: pa_blocks x pa_hp words)."""
    total = 0
    for s, t, bw in zip(seqs, tpls, bws):
        n, m = len(s.seq), len(t)
        H = 2 * int(bw) + abs(n - m) + 1
        total += ((((H + 2 * m + 1) >> 1) + 15) >> 4) * ((H + 1) & ~1) * 8
    return total


def test_device_memory(cases):
    """A second identical call grows nothing; the first call of a fresh
    engine grows less than the same rf_pair_align_smart call by at least the
    trace (the set's widest round: max_doublings = 0 here, one round)."""
    seqs, tpls, bws = cases["seqs"], cases["tpls"], cases["bws"]
    ids = np.arange(len(seqs))
    growth = {}
    for name in ("errors", "smart"):
        eng = Engine(0)
        try:
            eng.set_sequences(0, seqs)
            eng.set_templates(0, tpls)
            base = eng.device_bytes()
            if name == "errors":
                first = eng.pair_errors(ids, ids, bws, NEVER)
                growth[name] = eng.device_bytes() - base
                again = eng.pair_errors(ids, ids, bws, NEVER)
                assert eng.device_bytes() - base == growth[name]
                for a, b in zip(first, again):
                    assert a.tobytes() == b.tobytes()
                # rounds do not grow it either: 12 B per pair and the descriptors
                eng.pair_errors(ids, ids, bws, ALWAYS, max_doublings=5)
                assert eng.device_bytes() - base == growth[name]
            else:
                eng.pair_align_smart(ids, ids, bws, NEVER, max_doublings=0, want_moves=False)
                growth[name] = eng.device_bytes() - base
        finally:
            eng.close()
    assert growth["smart"] - growth["errors"] >= trace_bytes(seqs, tpls, bws) > 0, growth


def test_state_untouched(engine):
    rng = np.random.default_rng(2605)
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
    engine.pair_align(ids, 0, 3, want_moves=False)
    fw = engine.last_pair_align_ms()
    got = engine.pair_errors(ids[:, None], np.arange(3)[None, :], 3, ALWAYS, max_doublings=5)
    check_smart(got, [oracle_smart(tpls[j], s, 3, ALWAYS, False) for s in seqs for j in range(3)], np.arange(12))
    assert max(got[3]) >= 3
    assert engine.last_pair_align_ms() == fw and engine.last_pair_errors_ms() > 0
    assert before.tobytes() == engine.score_dense([ids])[0].tobytes()
    assert geo == [engine.geometry(int(k)) for k in ids]
    assert bands == [engine.download_band(int(k)).data.tobytes() for k in ids]
    moves, _ = engine.backtrace(ids)
    for k in ids:
        np.testing.assert_array_equal(moves[k], oracle_align(t, seqs[k], 3)[1])


# ---------------------------------------------------------------------
# 6. argument errors: rf_pair_align_smart's, under this call's name
# ---------------------------------------------------------------------
def test_argument_errors(engine):
    rng = np.random.default_rng(2606)
    L = DPW_LDS_H // 2          # n = m = L: 2 L + 1 = 5,115 rows at bandwidth L
    assert 2 * L + 1 == DPW_LDS_H + 1 == 5115
    small = RifrafSequence(random_seq(30, rng), np.full(30, -2.0), 3, SEQ_SCORES)
    wide = RifrafSequence(random_seq(L, rng), np.full(L, -2.0), 100, SEQ_SCORES)
    engine.set_sequences(0, [small, wide])
    engine.set_templates(0, [random_seq(30, rng), random_seq(L, rng)])
    lib, ctx = engine.lib, engine.ctx
    i32 = lambda *v: np.array(v, np.int32)   # noqa: E731
    ids, bws, thr = i32(0, 1), i32(3, 100), np.full(2, ALWAYS)

    def both(n, seq, tpl, bw, threshold, md, flags):
        """(rc, message, outputs untouched) of rf_pair_errors and the message of rf_pair_align_smart."""
        sc, ne, ob, rd = np.full(2, 7.5), np.full(2, 77, np.int32), np.full(2, 77, np.int32), np.full(2, 77, np.int32)
        rc = lib.rf_pair_errors(ctx, n, ptr(seq), ptr(tpl), ptr(bw), ptr(threshold), None, md, flags, ptr(sc), ptr(ne),
                                ptr(ob), ptr(rd))
        msg = lib.rf_last_error(ctx).decode()
        untouched = (sc == 7.5).all() and all((x == 77).all() for x in (ne, ob, rd))
        rc2 = lib.rf_pair_align_smart(ctx, n, ptr(seq), ptr(tpl), ptr(bw), ptr(threshold), None, md, flags, None,
                                      None, None, None, None, None, None)
        return rc, msg, untouched, rc2, lib.rf_last_error(ctx).decode()

    for args, text in (((2, ids, ids, bws, thr, 5, RF_BWD), "RF_BWD"),
                       ((1, i32(0), i32(0), i32(0), thr, 5, 0), "bandwidth"),
                       ((1, i32(1 << 20), i32(0), i32(3), thr, 5, 0), "unknown"),
                       ((2, ids, ids, bws, thr, 6, 0), "max_doublings"),
                       ((2, ids, ids, bws, None, 1, 0), "threshold"),
                       ((2, ids, ids, bws, thr, 5, 0), "5115")):     # min(100 * 2^5, L, L) = L
        rc, msg, untouched, rc2, msg2 = both(*args)
        assert rc != 0 and rc == rc2 and untouched, (text, rc, rc2)
        assert text in msg and msg == msg2.replace("rf_pair_align_smart", "rf_pair_errors"), (msg, msg2)
    assert "pair 1" in msg and str(DPW_LDS_H) in msg
    # every output pointer may be NULL; with max_doublings 0 the threshold too
    assert lib.rf_pair_errors(ctx, 1, ptr(ids), ptr(ids), ptr(bws), ptr(thr), None, 5, 0, None, None, None, None) == 0
    assert lib.rf_pair_errors(ctx, 2, ptr(ids), ptr(ids), ptr(bws), None, None, 0, 0, None, None, None, None) == 0
    assert lib.rf_pair_errors(ctx, 0, None, None, None, None, None, 0, 0, None, None, None, None) == 0


# ---------------------------------------------------------------------
# 7. the Python layer
# ---------------------------------------------------------------------
def test_python_surface(engine, cases):
    seqs, tpls = cases["seqs"], cases["tpls"]
    got = pairalign.count_errors_many(seqs, tpls, engine=engine)
    assert got.tolist() == [oracle_align(t, s, s.bandwidth, skew=True)[2] for t, s in zip(tpls, seqs)]
    bw, nerr, sc = pairalign.smart_bandwidths_many(seqs, tpls, engine=engine)
    thr = poisson_thresholds(seqs)
    exp = [oracle_smart(t, s, s.bandwidth, th, s.bandwidth_fixed, 5, cases["memo"], k)
           for k, (t, s, th) in enumerate(zip(tpls, seqs, thr))]
    assert bw.tolist() == [e.bw for e in exp] and nerr.tolist() == [e.nerr for e in exp]
    assert bits(sc).tolist() == bits([e.score for e in exp]).tolist()

    rng = np.random.default_rng(2415)
    gt = [random_seq(m, rng) for m in (120, 130, 110, 125)]
    reads = [indel_read(gt[k // 3], rng, 3, SEQ_SCORES, 5) for k in range(6)]
    a = assign.cross_scores(reads, gt, engine=engine, bandwidth_pvalue=0.1, return_bandwidths=True)
    b = assign.cross_scores(reads, gt, engine=engine, bandwidth_pvalue=0.1, return_bandwidths=True, carry_counts=True)
    assert bits(a[0]).tobytes() == bits(b[0]).tobytes() and a[1].tobytes() == b[1].tobytes()
    assert (a[1] > 3).any()
    clusters = [([s.seq for s in reads[3 * c:3 * c + 3]], [np.full(len(s.seq), 20, np.int8) for s in reads[3 * c:3 * c + 3]])
                for c in range(2)]
    p0 = assign.choose_references(clusters, gt, bandwidth=3, engine=engine, bandwidth_pvalue=0.1)
    p1 = assign.choose_references(clusters, gt, bandwidth=3, engine=engine, bandwidth_pvalue=0.1, carry_counts=True)
    assert [p[0] for p in p0] == [p[0] for p in p1] == [0, 1]
    assert all(x[1].tobytes() == y[1].tobytes() for x, y in zip(p0, p1))
