"""rifraf_amd.deep: clusters of any depth scored inside a fixed band budget.

CPU part: plan_read_chunks' properties over seeded inputs, rf_host_band_bytes
against the band geometry restated here, and the new symbols' presence.

GPU part: dense_totals_chunked over three clusters under a budget that forces
at least three rounds equals one realign + score_dense (bit for bit, NaN
positions equal) and the oracle, with and without a reference; its band arena
is no larger than the budget and is the one its single reserve made, and its
device footprint is below the one-shot call's.
"""
import ctypes

import numpy as np
import pytest

import oracle
from _util import SEQ_SCORES, random_seq
from rifraf_amd import ErrorModel, RifrafSequence, Scores, _lib, dense_totals_chunked, plan_read_chunks
from rifraf_amd.deep import read_band_bytes


def same(got, exp):
    got, exp = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(exp, np.float64)
    nan = np.isnan(got) | np.isnan(exp)
    return np.where(nan, np.isnan(got) & np.isnan(exp), got.view(np.int64) == exp.view(np.int64))


# ---------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------
def band_bytes(n, m, bw, pad):
    """The geometry restated: H = 2 bw + |n - m| + 1 band rows, row stride
    P = ((H + 1) >> 1) | 1 doubles -- padded: (H + 1) >> 1 rounded up to whole
    128-B lines --, H + 2 m kappa rows, a region rounded up to 256 B; A and B
    are alike."""
    H = 2 * bw + abs(n - m) + 1
    P = (((H + 1) >> 1) + 15) // 16 * 16 if pad else ((H + 1) >> 1) | 1
    one = max((H + 2 * m) * P * 8, 16)
    return 2 * ((one + 255) // 256 * 256)


def test_host_band_bytes_geometry():
    rng = np.random.default_rng(9100)
    cases = [(1, 1, 0), (1, 0, 0), (1, 1, 1), (10000, 10000, 288), (5, 300, 2), (300, 5, 2), (31, 31, 15), (33, 31, 15)]
    cases += [(int(rng.integers(1, 3000)), int(rng.integers(0, 3000)), int(rng.integers(0, 300))) for _ in range(300)]
    for n, m, bw in cases:
        for pad in (False, True):
            assert _lib.host_band_bytes(n, m, bw, pad) == band_bytes(n, m, bw, pad), (n, m, bw, pad)
    assert any(band_bytes(n, m, bw, True) < band_bytes(n, m, bw, False) for n, m, bw in cases)   # why pad=None is a max
    for bad in ((0, 5, 1), (5, -1, 1), (5, 5, -1)):
        with pytest.raises(ValueError):
            _lib.host_band_bytes(*bad)


def test_plan_read_chunks_properties():
    rng = np.random.default_rng(9200)
    for trial in range(300):
        R = int(rng.integers(1, 40))
        m = int(rng.integers(1, 400))
        ns = np.maximum(1, m + rng.integers(-20, 21, R)).tolist()
        bws = rng.integers(1, 40, R).tolist()
        pad = (False, True, None)[trial % 3]
        size = [read_band_bytes(n, m, bw, pad) for n, bw in zip(ns, bws)]
        budget = int(rng.integers(min(size) // 2, 2 * sum(size) // max(1, int(rng.integers(1, R + 1))) + 1))
        plan = plan_read_chunks(ns, m, bws, budget, pad)
        # consecutive, disjoint, covering
        assert plan[0][0] == 0 and plan[-1][1] == R
        assert all(a < b for a, b in plan) and all(p[1] == q[0] for p, q in zip(plan[:-1], plan[1:]))
        for i, (a, b) in enumerate(plan):
            tot = sum(size[a:b])
            assert tot <= budget or b - a == 1, (trial, a, b)            # within budget unless a single read
            if i + 1 < len(plan):
                assert tot + size[b] > budget, (trial, a, b)               # greedy-maximal: the next read did not fit
    assert plan_read_chunks([], 5, [], 100, False) == []
    with pytest.raises(ValueError):
        plan_read_chunks([5, 6], 5, [3], 100, False)


def arena_of(need):
    """rf_reserve's arena for `need` bytes of bands, restated: two 64-KiB
    guards, a margin of an eighth plus 1 MiB, whole MiB."""
    c = need + 2 * 65536
    return (c + c // 8 + (1 << 20) + (1 << 20) - 1) >> 20 << 20


def test_host_reserve_fit():
    rng = np.random.default_rng(9150)
    budgets = [2 << 20, (2 << 20) + 1, (3 << 20) - 1, 3 << 20, 5 << 20, 8 << 30, 288 << 30]
    budgets += [int(rng.integers(2 << 20, 1 << 36)) for _ in range(200)]
    for b in budgets:
        fit = _lib.host_reserve_fit(b)
        assert fit >= 0 and arena_of(fit) <= b < arena_of(fit + 1), (b, fit)     # the largest that fits
    for b in (0, 1 << 20, (2 << 20) - 1):
        with pytest.raises(ValueError):
            _lib.host_reserve_fit(b)


def test_abi_symbols():
    lib = _lib.load()
    for name in ("rf_score_dense_from", "rf_score_dense_from_dev", "rf_host_band_bytes", "rf_host_reserve_fit",
                 "rf_band_arena_bytes"):
        assert name in _lib._SIGNATURES and getattr(lib, name) is not None
    assert lib.rf_host_band_bytes.restype is ctypes.c_int64
    assert lib.rf_abi_version() == 1


# ---------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------
COUNTS = (5, 12, 1)
MS = (40, 120, 77)
BW = 60            # H >= 121: a few hundred KB of bands per read, so that the arenas differ by whole MiB


def read_of(t, d, rng):
    s = list(t)
    for _ in range(abs(d)):
        if d > 0:
            s.insert(int(rng.integers(0, len(s) + 1)), int(rng.integers(0, 4)))
        else:
            del s[int(rng.integers(0, len(s)))]
    s = np.array(s, np.uint8)
    sub = rng.random(len(s)) < 0.05
    s[sub] = (s[sub] + rng.integers(1, 4, int(sub.sum()))) % 4
    return RifrafSequence(s, rng.integers(8, 40, len(s)) / -10.0, BW, SEQ_SCORES)


@pytest.fixture(scope="module")
def clusters():
    rng = np.random.default_rng(9300)
    tpls = [random_seq(m, rng) for m in MS]
    reads = [[read_of(t, int(rng.integers(-3, 4)), rng) for _ in range(c)] for t, c in zip(tpls, COUNTS)]
    ref = RifrafSequence(random_seq(121, rng), np.log10(rng.uniform(0.01, 0.3, 121)), BW,
                         Scores.from_errors(ErrorModel(1.0, 2.0, 2.0)))
    # the budget: an arena of 5 MiB.  What it holds of bands (host_reserve_fit),
    # shared over three clusters, takes three of the deepest cluster's reads
    # and not four, so its twelve reads take four rounds; beside the reference
    # of the second variant a share still holds a read, so no single read
    # forces the arena to grow
    budget = 5 << 20
    fit = _lib.host_reserve_fit(budget)
    assert 0 < fit < budget
    size = [read_band_bytes(len(r), MS[1], BW, None) for r in reads[1]]
    assert max(sum(size[k:k + 3]) for k in range(10)) <= fit // 3 < min(sum(size[k:k + 4]) for k in range(9))
    assert read_band_bytes(len(ref), MS[1], BW, None) + max(size) <= fit // 3
    plans = [plan_read_chunks([len(r) for r in rs], m, [BW] * len(rs), fit // 3, None) for rs, m in zip(reads, MS)]
    assert max(len(p) for p in plans) >= 3 and len(plans[2]) == 1
    orc = [oracle.cpu_pass(t, rs, nthreads=1)[0] for t, rs in zip(tpls, reads)]
    orc_ref = oracle.cpu_pass(tpls[1], reads[1] + [ref], nthreads=1)[0]
    for a in orc + [orc_ref]:
        a.setflags(write=False)
    return dict(tpls=tpls, reads=reads, ref=ref, budget=budget, fit=fit, oracle=orc, oracle_ref=orc_ref)


def one_shot(e, cl, with_ref):
    from rifraf_amd.engine import RF_BWD, RF_FWD
    seqs = [r for rs in cl["reads"] for r in rs] + ([cl["ref"]] if with_ref else [])
    tpl = [g for g, rs in enumerate(cl["reads"]) for _ in rs] + ([1] if with_ref else [])
    e.release_bands()
    e.set_sequences(0, seqs)
    e.set_templates(0, cl["tpls"])
    k = np.arange(len(seqs))
    sc = e.realign(k, k, tpl, BW, RF_FWD | RF_BWD)
    at, groups = 0, []
    for c in COUNTS:
        groups.append(np.arange(at, at + c, dtype=np.int32))
        at += c
    tabs = e.score_dense_ref(groups, [-1, at, -1]) if with_ref else e.score_dense(groups)
    return tabs, [sc[g] for g in groups]


@pytest.mark.gpu
@pytest.mark.parametrize("with_ref", (False, True))
def test_chunked_equals_one_shot(clusters, with_ref):
    """Fresh engines: the footprint comparison needs arenas that nothing else
    has grown."""
    from rifraf_amd.engine import Engine
    cl = clusters
    a, b, c = Engine(0), Engine(0), Engine(0)
    try:
        exp_tabs, exp_sc = one_shot(a, cl, with_ref)
        stats = {}
        tabs, sc = dense_totals_chunked(cl["reads"], cl["tpls"], band_bytes=cl["budget"],
                                        references=[None, cl["ref"], None] if with_ref else None, engine=b,
                                        stats=stats)
        assert max(len(p) for p in stats["plans"]) >= 3
        assert len(stats["round_band_bytes"]) == max(len(p) for p in stats["plans"])
        for g in range(3):
            ok = same(tabs[g], exp_tabs[g])
            assert ok.all(), (g, int((~ok).sum()))
            assert same(sc[g], exp_sc[g]).all(), g
            exp = cl["oracle_ref"] if with_ref and g == 1 else cl["oracle"][g]
            t = cl["tpls"][g]      # the oracle scores proposals: not Sub / Del of p = 0, not the consensus base
            mask = np.ones((len(t) + 1, 9), bool)
            mask[0, :5] = False
            mask[np.arange(1, len(t) + 1), np.asarray(t, np.int64)] = False
            assert same(tabs[g][mask], exp[mask]).all(), ("oracle", g)
        # the band arena: no larger than the budget, and still the one that
        # the driver's single reserve made (an arena that grew afterwards is
        # at least half as large again); the one-shot call's does not fit
        assert max(stats["round_band_bytes"]) <= cl["fit"]
        c.reserve(cl["fit"])
        assert 0 < b.band_arena_bytes() == c.band_arena_bytes() <= cl["budget"] < a.band_arena_bytes()
        assert b.device_bytes() < a.device_bytes()
    finally:
        a.close()
        b.close()
        c.close()
