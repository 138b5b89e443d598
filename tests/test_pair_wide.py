"""The wide tier of the pair calls (RF_OPT_PAIR_WIDE; k_ps_wide, k_pa_wide,
k_pe_wide): bands past DPW_LDS_H with the ring in device memory.  Expected
values are the CPU oracle's (forward_moves! + backtrace + count_errors) and
the same call with the option off where that call is accepted.  Equality is
exact: integer-equal moves and counts, bit-equal scores.

pair_wide = 2 sends every pair through the tier, so the exhaustive small
sweep reaches its body; pair_wide = 1 is the product setting.  The cheap wide
shape is the refusal tests': a 12-base read against 12 + H - 5 template bases
at bandwidth 2, H rows and H + 2 m almost empty anti-diagonals."""
import numpy as np
import pytest

import oracle
from _util import REF_SCORES, SEQ_SCORES, random_seq
from rifraf_amd import RifrafSequence, _lib, pairalign
import rifraf_amd.align as align_mod
from rifraf_amd._lib import ptr
from rifraf_amd.engine import RF_SKEW, RF_TRIM, Engine, RifrafError
from test_pair_align import check, oracle_align, run_pairs
from test_pair_align_smart_host import ALWAYS, oracle_smart
from test_pair_scores import DPW_LDS_H, SWEEP, bits_equal, final_cell, random_read
from test_pair_text import all_text, check_products, host_products
from test_small_geometry import NA, SHAPES, cls_of

pytestmark = pytest.mark.gpu

_ORACLE = {}


def expected(key, t, s, bw, skew=False, trim=False):
    """oracle_align, once per session for each named pair."""
    if key not in _ORACLE:
        _ORACLE[key] = oracle_align(t, s, bw, skew, trim)
    return _ORACLE[key]


def shape_pair(H, rng, scores=SEQ_SCORES):
    """12 bases against 12 + H - 5 at bandwidth 2: H rows."""
    s, t = random_read(12, 2, rng, scores), random_seq(12 + H - 5, rng)
    assert 2 * 2 + abs(12 - len(t)) + 1 == H
    return s, t


# ---------------------------------------------------------------------
# 1. the small sweep through the wide body
# ---------------------------------------------------------------------
@pytest.mark.parametrize("name,flags", SWEEP)
def test_sweep_small_shapes(engine, opts, name, flags):
    """test_small_geometry's 576 shapes of one input class (lean and codon
    reads, -Inf table entries, exact ties), all in the wide tier: scores,
    alignments and carried counts against the oracle and the option off."""
    c = cls_of(name)
    skew, trim = bool(flags & RF_SKEW), bool(flags & RF_TRIM)
    fills, walks = c.fills(skew, trim), c.walks(skew, trim)
    exp = [(final_cell(fills[k][0], n, m, bw), walks[k][0], walks[k][1]) for k, (m, n, bw) in enumerate(SHAPES)]
    ids = np.arange(NA)
    off = run_pairs(engine, c.seqs, c.templates, c.bws, flags)
    off_sc = engine.pair_scores(ids, ids, c.bws, flags)
    off_err = engine.pair_errors(ids, ids, c.bws, flags=flags)
    opts("pair_wide", 2)
    got = run_pairs(engine, c.seqs, c.templates, c.bws, flags)
    check(got, exp, SHAPES)
    assert bits_equal(got[0], off[0]) and got[2].tolist() == off[2].tolist()
    assert all(np.array_equal(a, b) for a, b in zip(got[1], off[1]))
    sc = engine.pair_scores(ids, ids, c.bws, flags)
    assert bits_equal(sc, [e[0] for e in exp]) and bits_equal(sc, off_sc)
    esc, nerr, bw, rounds = engine.pair_errors(ids, ids, c.bws, flags=flags)
    assert bits_equal(esc, [e[0] for e in exp]) and bits_equal(esc, off_err[0])
    assert nerr.tolist() == [e[2] for e in exp] == off_err[1].tolist()
    assert bw.tolist() == list(c.bws) and (rounds == 1).all()


# ---------------------------------------------------------------------
# 2. the threshold
# ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def threshold_pairs():
    """H = 5,114 (LDS tier), 5,115 and 5,116 (odd and even HP), lean reads;
    and 5,115 / 5,116 with codon tables."""
    rng = np.random.default_rng(3611)
    pairs = [shape_pair(H, rng) for H in (DPW_LDS_H, DPW_LDS_H + 1, DPW_LDS_H + 2)]
    pairs += [shape_pair(H, rng, REF_SCORES) for H in (DPW_LDS_H + 1, DPW_LDS_H + 2)]
    return [s for s, _ in pairs], [t for _, t in pairs]


@pytest.mark.parametrize("walk", (1, 2))
def test_threshold(engine, opts, threshold_pairs, walk):
    assert DPW_LDS_H == 5114
    seqs, tpls = threshold_pairs
    opts("pair_walk", walk)
    lds = run_pairs(engine, seqs[:1], tpls[:1], 2)   # the option off: H = 5,114 alone
    opts("pair_wide", 1)
    got = run_pairs(engine, seqs, tpls, 2)
    exp = [expected(("thr", k, 0), t, s, 2) for k, (t, s) in enumerate(zip(tpls, seqs))]
    check(got, exp)
    assert bits_equal(got[0][:1], lds[0]) and np.array_equal(got[1][0], lds[1][0])
    ids = np.arange(len(seqs))
    assert bits_equal(engine.pair_scores(ids, ids, 2), [e[0] for e in exp])
    esc, nerr, _, _ = engine.pair_errors(ids, ids, 2)
    assert bits_equal(esc, [e[0] for e in exp]) and nerr.tolist() == [e[2] for e in exp]
    # codon tables with RF_TRIM
    got = run_pairs(engine, seqs[3:], tpls[3:], 2, RF_TRIM)
    check(got, [expected(("thr", 3 + k, RF_TRIM), t, s, 2, trim=True) for k, (t, s) in enumerate(zip(tpls[3:], seqs[3:]))])


# ---------------------------------------------------------------------
# 3. edit_distance's own shape
# ---------------------------------------------------------------------
L = (DPW_LDS_H + 1) // 2   # n = m = L at bandwidth L: 2 L + 1 = 5,115 rows


@pytest.fixture(scope="module")
def edit_pair():
    """n = m = 2,557, about 12 % edits, as edit_distance builds its sequence."""
    rng = np.random.default_rng(3612)
    t = random_seq(L, rng)
    s = t.copy()
    for i in rng.integers(0, L, 300):
        s[i] = (s[i] + rng.integers(1, 4)) % 4
    for _ in range(20):
        s = np.delete(s, rng.integers(0, len(s)))
        s = np.insert(s, rng.integers(0, len(s)), rng.integers(0, 4)).astype(np.uint8)
    assert len(s) == L and 2 * L + 1 == DPW_LDS_H + 1
    rs = RifrafSequence(s, np.full(L, -1.0), L, pairalign.Scores.from_errors(pairalign.ErrorModel(1.0, 1.0, 1.0)))
    return t, rs, oracle_align(t, rs, L, skew=True)


def test_edit_distance_shape(engine, opts, edit_pair):
    t, rs, (score, _, nerr) = edit_pair
    slots = align_mod.edit_distance(t, rs.seq, scratch=align_mod.Scratch(engine))
    assert slots == nerr
    opts("pair_wide", 1)
    sc, _, ne = run_pairs(engine, [rs], [t], L, RF_SKEW, want_moves=False)
    assert bits_equal(sc, [score]) and ne.tolist() == [nerr]
    esc, ene, _, _ = engine.pair_errors([0], [0], L, flags=RF_SKEW)
    assert bits_equal(esc, [score]) and ene.tolist() == [nerr]
    opts("pair_wide", 0)
    assert pairalign.edit_distances([t], [rs.seq], engine=engine, wide=True).tolist() == [nerr]
    assert engine.get_option("pair_wide") == 0
    # (edit_distance's own bandwidth for this pair is ceil(L / 2): the same count from a narrower band)
    got = pairalign.calibrate_phreds_many([rs.seq], [np.full(L, 20, np.int8)], t, engine=engine)
    assert np.isclose(got[0].sum(), nerr)


def test_edit_distance_shape_moves(engine, opts, edit_pair):
    t, rs, exp = edit_pair
    opts("pair_wide", 1)
    check(run_pairs(engine, [rs], [t], L, RF_SKEW), [exp])


# ---------------------------------------------------------------------
# 4. stale state between the pairs of one workgroup
# ---------------------------------------------------------------------
STALE_H = (5200, 40, 5115, 7, 300)


@pytest.fixture(scope="module")
def stale_pairs():
    rng = np.random.default_rng(3613)
    pairs = [shape_pair(H, rng, REF_SCORES if k % 2 else SEQ_SCORES) for k, H in enumerate(STALE_H)]
    seqs, tpls = [s for s, _ in pairs], [t for _, t in pairs]
    exp = [oracle_align(t, s, 2) for s, t in pairs]
    # the pair the reference raises on: every table entry -Inf
    bad = RifrafSequence(random_seq(12, rng), np.full(12, -2.0), 2, SEQ_SCORES)
    for name in ("match_scores", "mismatch_scores", "ins_scores", "del_scores"):
        setattr(bad, name, np.full(len(getattr(bad, name)), -np.inf))
    with pytest.raises(oracle.OracleError):
        oracle.forward(tpls[1], bad, moves=True, bandwidth=2)
    return seqs, tpls, exp, bad


def test_one_workgroup_takes_every_pair(engine, opts, stale_pairs):
    seqs, tpls, exp, bad = stale_pairs
    assert _lib.host_pair_wide_plan(STALE_H, "trace", 0).nwg == _lib.host_pair_wide_plan(STALE_H, "count", 0).nwg == 1
    opts("pair_ring_mb", 0)
    opts("pair_wide", 2)
    ids = np.arange(5)
    check(run_pairs(engine, seqs, tpls, 2), exp, STALE_H)
    esc, nerr, _, _ = engine.pair_errors(ids, ids, 2)
    assert bits_equal(esc, [e[0] for e in exp]) and nerr.tolist() == [e[2] for e in exp]
    assert bits_equal(engine.pair_scores(ids, ids, 2), [e[0] for e in exp])
    # the second pair raises: NaN / -1 / no moves, its neighbours unchanged
    with_bad = seqs[:1] + [bad] + seqs[2:]
    sc, moves, ne = run_pairs(engine, with_bad, tpls, 2)
    assert np.isnan(sc[1]) and moves[1] is None and ne[1] == -1
    keep = [0, 2, 3, 4]
    check((sc[keep], [moves[k] for k in keep], ne[keep]), [exp[k] for k in keep])
    esc, nerr, _, _ = engine.pair_errors(ids, ids, 2)
    assert np.isnan(esc[1]) and nerr[1] == -1
    assert bits_equal(esc[keep], [exp[k][0] for k in keep]) and nerr[keep].tolist() == [exp[k][2] for k in keep]
    psc = engine.pair_scores(ids, ids, 2)
    assert np.isnan(psc[1]) and bits_equal(psc[keep], [exp[k][0] for k in keep])


# ---------------------------------------------------------------------
# 5. band doubling across the limit
# ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def doubling_pair():
    """n = m = 2,557, starting bandwidth 100, max_doublings 5: max_bw =
    min(3,200, m, n) = 2,557, 5,115 rows.  Unrelated sequences stall at the
    first doubling (their best path stays near the diagonal), so the pair is
    built to gain from every one: the template is 1,250 A then G, the read
    1,300 G then A, and a mismatch costs far more than an insertion and a
    deletion.  The read's A at i matches a template A at j only with
    i - j >= 50, and at bandwidth b the path holds min(b - 50, 1,250) such
    matches, about 50, 150, 350, 750, 1,250 at b = 100 ... 1,600: every count below
    the one before, and the loop ends at max_bw (checked here with the oracle's
    loop)."""
    t = np.concatenate([np.zeros(1250, np.uint8), np.full(L - 1250, 2, np.uint8)])
    seq = np.concatenate([np.full(1300, 2, np.uint8), np.zeros(L - 1300, np.uint8)])
    s = RifrafSequence(seq, np.full(L, -1.0), 100, SEQ_SCORES)
    s.mismatch_scores = np.full(L, -1000.0)
    e = oracle_smart(t, s, 100, ALWAYS, False, 5)
    assert e.bw == L and e.rounds == 6 and e.why == "max", (e.bw, e.rounds, e.why)
    return t, s, e


def test_doubling_reaches_the_wide_tier(engine, opts, doubling_pair):
    t, s, e = doubling_pair
    engine.set_sequences(0, [s])
    engine.set_templates(0, [t])
    with pytest.raises(RifrafError):
        engine.pair_align_smart([0], [0], 100, ALWAYS)
    opts("pair_wide", 1)
    sc, moves, ne, bw, rounds = engine.pair_align_smart([0], [0], 100, ALWAYS, caps=np.array([2 * L]))
    assert bits_equal(sc, [e.score]) and ne.tolist() == [e.nerr]
    assert bw.tolist() == [e.bw] == [L] and rounds.tolist() == [e.rounds]
    np.testing.assert_array_equal(moves[0], e.moves)
    esc, ene, ebw, erounds = engine.pair_errors([0], [0], 100, ALWAYS, max_doublings=5)
    assert bits_equal(esc, [e.score]) and ene.tolist() == [e.nerr]
    assert ebw.tolist() == [L] and erounds.tolist() == [e.rounds]


# ---------------------------------------------------------------------
# 6. the kernels downstream of the trace
# ---------------------------------------------------------------------
def test_text_and_shifts_of_a_wide_pair(engine, opts, threshold_pairs):
    seqs, tpls = threshold_pairs
    s, t = seqs[1], tpls[1]   # 5,115 rows
    mv = expected(("thr", 1, 0), t, s, 2)[1]
    engine.set_sequences(0, [s])
    engine.set_templates(0, [t])
    opts("pair_wide", 1)
    _, r = all_text(engine, [0], [0], 2)
    check_products(r, [host_products(mv, t, s, 2)])
    caps = np.array([len(s) + len(t)], np.int64)
    _, sh = engine.pair_shifts([0], [0], 2, 0, want_fixed=True, want_proposals=True, caps=caps)
    exp = _lib.host_shift_fix([mv], [s.seq], [t])
    assert sh.fixed_len.tolist() == exp.fixed_len.tolist() and sh.nprops.tolist() == exp.nprops.tolist()
    assert sh.tally.tolist() == exp.tally.tolist() and sh.proposals(0) == exp.proposals(0)
    x, y = sh.fixed_seq(0), exp.fixed_seq(0)
    assert (x is None and y is None) or x.tolist() == y.tolist()


# ---------------------------------------------------------------------
# 7. the default is unchanged
# ---------------------------------------------------------------------
def test_default_refuses_and_changes_nothing(threshold_pairs):
    seqs, tpls = threshold_pairs
    e = Engine(0)
    try:
        assert e.get_option("pair_wide") == 0 and e.get_option("pair_ring_mb") == 256
        e.set_sequences(0, seqs[1:2])
        e.set_templates(0, tpls[1:2])
        ids, bws = np.zeros(1, np.int32), np.full(1, 2, np.int32)
        sc, nm, ne = np.full(1, 7.5), np.full(1, 77, np.int32), np.full(1, 77, np.int32)
        rc = e.lib.rf_pair_align(e.ctx, 1, ptr(ids), ptr(ids), ptr(bws), 0, ptr(sc), None, None, ptr(nm), ptr(ne))
        assert rc != 0 and sc[0] == 7.5 and nm[0] == 77 and ne[0] == 77
        assert str(DPW_LDS_H) in e.lib.rf_last_error(e.ctx).decode()
        rc = e.lib.rf_pair_scores(e.ctx, 1, ptr(ids), ptr(ids), ptr(bws), 0, ptr(sc))
        assert rc != 0 and sc[0] == 7.5
        # with the option on the limits are the wide tier's, checked before anything runs
        e.set_option("pair_wide", 1)
        huge = np.full(1, 1 << 23, np.int32)   # 2^24 + 1 rows and more
        rc = e.lib.rf_pair_scores(e.ctx, 1, ptr(ids), ptr(ids), ptr(huge), 0, ptr(sc))
        assert rc != 0 and sc[0] == 7.5 and str(1 << 24) in e.lib.rf_last_error(e.ctx).decode()
    finally:
        e.close()
