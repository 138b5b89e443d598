"""rf_score_dense_from / rf_score_dense_from_dev: dense scoring that continues
a fold.  score_proposal's sum over the batch (model.jl:385-399) is a left fold
in read order, so from(init = dense(reads 1..k), reads k+1..R) must have the
bits of dense(reads 1..R) -- every comparison here is of bits, with NaN
positions equal -- in every scorer (k_score, k_score_segl, k_score_ws), in
fused mode (the kernels' totals start from init) and in split mode (k_reduce
starts from init), and must equal oracle.cpu_pass(..., totals=...) folded over
the same chunks.

Shapes are the smallest at which the code paths differ: templates on both
sides of the 64- and 256-column item widths, 2-6 reads (15-33 for k_reduce's
16-wide body), bandwidths 3 and 9 and one band wide enough for k_score_segl's
natural pick.
"""
import functools

import numpy as np
import pytest

import oracle
from _util import SEQ_SCORES, assert_score_launch, make_read, random_seq
from rifraf_amd import ErrorModel, RifrafSequence, Scores, _lib
from rifraf_amd._lib import ptr
from rifraf_amd.engine import RF_BAND_A, RF_BAND_B, RF_BWD, RF_FWD, RifrafError

pytestmark = pytest.mark.gpu

RF_ERR_ARG, RF_ERR_STATE = -1, -4
CODON = Scores.from_errors(ErrorModel(10.0, 1e-5, 1e-5, 1.0, 1.0))
MS = (1, 2, 7, 63, 64, 65, 255, 256, 257)
KERNELS = ("general", "seg", "ws")
MODES = ("fused", "split")


def same(got, exp):
    """Bit equality (int64 views) on non-NaN values, NaN only where both are."""
    got, exp = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(exp, np.float64)
    nan = np.isnan(got) | np.isnan(exp)
    return np.where(nan, np.isnan(got) & np.isnan(exp), got.view(np.int64) == exp.view(np.int64))


def assert_same(got, exp, key):
    ok = same(got, exp)
    assert ok.all(), (key, int((~ok).sum()), np.argwhere(~ok)[:4].tolist())


def assert_oracle(got, t, exp, key):
    """Against oracle.cpu_pass, which scores what the reference scores: every
    slot but Sub / Del of p = 0 (the engine: NaN) and the consensus base's
    own Sub slot (not a proposal)."""
    mask = np.ones((len(t) + 1, 9), bool)
    mask[0, :5] = False
    mask[np.arange(1, len(t) + 1), np.asarray(t, np.int64)] = False
    assert np.isnan(got[0, :5]).all(), key
    assert_same(got[mask], exp[mask], key)


def read_of(t, d, bw, rng):
    """t with d bases inserted (d > 0) or -d deleted and a few substitutions;
    finite tables (the lean scorers' condition)"""
    s = list(t)
    for _ in range(abs(d)):
        if d > 0:
            s.insert(int(rng.integers(0, len(s) + 1)), int(rng.integers(0, 4)))
        elif len(s) > 1:
            del s[int(rng.integers(0, len(s)))]
    s = np.array(s, np.uint8)
    sub = rng.random(len(s)) < 0.05
    s[sub] = (s[sub] + rng.integers(1, 4, int(sub.sum()))) % 4
    return RifrafSequence(s, rng.integers(8, 40, len(s)) / -10.0, bw, SEQ_SCORES)


def make_group(m, R, bw, rng):
    t = random_seq(m, rng)
    return t, [read_of(t, int(rng.integers(-3, 4)), bw, rng) for _ in range(R)]


def load(engine, groups, extra=()):
    """Upload the groups' reads (sequence id = slot id, template g), then
    `extra` sequences as (sequence, template) pairs, and fill every band.
    Returns the slot arrays of the groups and the slots of the extras."""
    engine.release_bands()
    seqs, tpl, slots = [], [], []
    for g, (t, reads) in enumerate(groups):
        slots.append(np.arange(len(seqs), len(seqs) + len(reads), dtype=np.int32))
        seqs += reads
        tpl += [g] * len(reads)
    xs = []
    for s, g in extra:
        xs.append(len(seqs))
        seqs.append(s)
        tpl.append(g)
    engine.set_sequences(0, seqs)
    engine.set_templates(0, [t for t, _ in groups])
    k = np.arange(len(seqs))
    engine.realign(k, k, tpl, [s.bandwidth for s in seqs], RF_FWD | RF_BWD)
    return slots, xs


def chain(engine, slots, cuts, ref_last=None):
    """score_dense_from over the chunks slots[0:cuts[0]], slots[cuts[0]:cuts[1]],
    ... of one group, each continuing the one before."""
    edges = [0, *cuts, len(slots)]
    tab = None
    for i, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        last = i == len(edges) - 2
        tab = engine.score_dense_from([slots[a:b]], tab, [ref_last] if last and ref_last is not None else None)
    return tab[0]


# ---------------------------------------------------------------------
# the cut sweep: every scorer and fold mode, every cut
# ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sweep_groups(bw):
    rng = np.random.default_rng(7100 + bw)
    return [make_group(m, R, bw, rng) for m in MS for R in (2, 3, 6)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("bw", (3, 9))
def test_cut_sweep(engine, opts, bw, kernel, mode):
    """from(init = dense(first k), reads k+1..R) == dense(all R) at every
    0 < k < R.  All 27 groups are loaded once; a cut k is one call over the
    groups that have it."""
    groups = sweep_groups(bw)
    slots, _ = load(engine, groups)
    opts("score_kernel", kernel)
    opts("score_mode", mode)
    whole = engine.score_dense(slots)
    assert_score_launch(engine, kernel, mode)
    for k in range(1, 6):
        idx = [g for g, s in enumerate(slots) if len(s) > k]
        first = engine.score_dense([slots[g][:k] for g in idx])
        got = engine.score_dense_from([slots[g][k:] for g in idx], first)
        assert_score_launch(engine, kernel, mode)
        for g, tab in zip(idx, got):
            assert_same(tab, whole[g], (bw, kernel, mode, len(groups[g][0]), len(slots[g]), k))
    # the oracle, once per bandwidth: the default modes are checked against it elsewhere too
    if kernel == "ws" and mode == "fused":
        for g in (0, 8, 13, 26):
            t, reads = groups[g]
            assert_oracle(whole[g], t, oracle.cpu_pass(t, reads, nthreads=1)[0], ("oracle", bw, g))


@pytest.mark.parametrize("mode", MODES)
def test_wide_band_natural_pick(engine, opts, mode):
    """Bands of H = 2 * 100 + |n - m| + 1 rows: the planner picks k_score_segl
    by itself (no score_kernel option)."""
    rng = np.random.default_rng(7200)
    groups = [make_group(m, 3, 100, rng) for m in (63, 130)]
    slots, _ = load(engine, groups)
    opts("score_mode", mode)
    whole = engine.score_dense(slots)
    assert_score_launch(engine, "seg", mode)
    for k in (1, 2):
        first = engine.score_dense([s[:k] for s in slots])
        got = engine.score_dense_from([s[k:] for s in slots], first)
        assert_score_launch(engine, "seg", mode)
        for g in range(2):
            assert_same(got[g], whole[g], (mode, g, k))


# ---------------------------------------------------------------------
# k_reduce's 16-wide body and its tail with an init
# ---------------------------------------------------------------------
@pytest.mark.parametrize("R", (15, 16, 17, 33))
def test_reduce_unroll(engine, opts, R):
    rng = np.random.default_rng(7300 + R)
    groups = [make_group(40, R, 3, rng)]
    (slots,), _ = load(engine, groups)
    opts("score_mode", "split")
    whole = engine.score_dense([slots])[0]
    assert_score_launch(engine, None, "split")
    for k in sorted({1, 16, R - 1} & set(range(1, R))):
        first = engine.score_dense([slots[:k]])
        got = engine.score_dense_from([slots[k:]], first)[0]
        assert_score_launch(engine, None, "split")
        assert_same(got, whole, (R, k))
    assert_oracle(whole, groups[0][0], oracle.cpu_pass(*groups[0], nthreads=1)[0], ("oracle", R))


# ---------------------------------------------------------------------
# chains of three and more chunks; reads-per-workgroup chunking with init
# ---------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kernel", ("seg", "ws"))
def test_chains(engine, opts, kernel, mode):
    rng = np.random.default_rng(7400)
    groups = [make_group(130, 7, 9, rng)]
    (slots,), _ = load(engine, groups)
    opts("score_kernel", kernel)
    opts("score_mode", mode)
    # few workgroups wanted: several reads per workgroup in split mode
    opts("score_wgs", 1)
    opts("seg_wgs", 4)
    whole = engine.score_dense([slots])[0]
    assert_score_launch(engine, kernel, mode)
    if mode == "split":
        assert engine.last_score_launch().grid_y < len(slots)      # rchunk > 1
    for cuts in ((1, 2), (2, 5), (1, 2, 3, 4, 5, 6), (3, 4)):
        assert_same(chain(engine, slots, cuts), whole, (kernel, mode, cuts))
    # the oracle over the same chunks, and over all reads at once
    t, reads = groups[0]
    tot = None
    for a, b in ((0, 2), (2, 5), (5, 7)):
        tot = oracle.cpu_pass(t, reads[a:b], nthreads=1, totals=tot)[0]
    assert_oracle(chain(engine, slots, (2, 5)), t, tot, "oracle chunks")
    assert_same(tot, oracle.cpu_pass(t, reads, nthreads=1)[0], "oracle one shot")


# ---------------------------------------------------------------------
# identities
# ---------------------------------------------------------------------
def test_identities(engine):
    rng = np.random.default_rng(7500)
    groups = [make_group(65, 3, 9, rng), make_group(7, 2, 3, rng)]
    ref = RifrafSequence(random_seq(66, rng), np.full(66, -1.0), 9, CODON)
    slots, (rs,) = load(engine, groups, [(ref, 0)])
    plain = engine.score_dense(slots)
    for got in (engine.score_dense_from(slots, None), engine.score_dense_from(slots, None, [-1, -1]),
                engine.score_dense_from(slots, [np.zeros_like(p) for p in plain])):
        for g in range(2):
            assert_same(got[g], plain[g], g)
    with_ref = engine.score_dense_ref(slots, [rs, -1])
    got = engine.score_dense_from(slots, None, [rs, -1])
    for g in range(2):
        assert_same(got[g], with_ref[g], ("ref", g))
    assert not same(with_ref[0], plain[0]).all()


# ---------------------------------------------------------------------
# the reference term: added last, and the order is observed
# ---------------------------------------------------------------------
def test_reference_with_last_chunk(engine):
    """The oracle first, on the CPU: (reads + ref) differs from the fold that
    adds the reference after the first chunk in at least one slot."""
    rng = np.random.default_rng(7600)
    t, reads = make_group(40, 5, 9, rng)
    ref = RifrafSequence(random_seq(41, rng), np.log10(rng.uniform(0.01, 0.3, 41)), 9,
                         Scores.from_errors(ErrorModel(1.0, 2.0, 2.0)))      # no codon tables: cpu_pass scores it
    last = oracle.cpu_pass(t, reads + [ref], nthreads=1)[0]
    early = oracle.cpu_pass(t, reads[2:], nthreads=1, totals=oracle.cpu_pass(t, reads[:2] + [ref], nthreads=1)[0])[0]
    mask = np.ones((41, 9), bool)
    mask[0, :5] = False
    mask[np.arange(1, 41), np.asarray(t, np.int64)] = False
    assert (~same(last, early))[mask].any()
    (slots,), (rs,) = load(engine, [(t, reads)], [(ref, 0)])
    one_shot = engine.score_dense_ref([slots], [rs])[0]
    assert_oracle(one_shot, t, last, "oracle")
    assert_same(chain(engine, slots, (2,), ref_last=rs), one_shot, "reference with the last chunk")
    first = engine.score_dense_from([slots[:2]], None, [rs])
    got = engine.score_dense_from([slots[2:]], first)[0]
    assert_oracle(got, t, early, "reference with the first chunk: the oracle's other fold")
    assert (~same(got, one_shot))[mask].any()
    # a codon-table reference (k_codon_dense's other branch) with the last
    # chunk.  The order check above uses a reference without codon tables
    # because the slot that differs has to be shown on the CPU first, and
    # oracle.cpu_pass, the only oracle fold that continues from totals, scores
    # reads without codon moves; with codon tables only the last-chunk
    # equality is checked
    cref = RifrafSequence(random_seq(41, rng), np.full(41, -1.0), 9, CODON)
    (slots,), (rs,) = load(engine, [(t, reads)], [(cref, 0)])
    assert_same(chain(engine, slots, (1, 4), ref_last=rs), engine.score_dense_ref([slots], [rs])[0], "codon")


# ---------------------------------------------------------------------
# non-finite tables and NaN
# ---------------------------------------------------------------------
def test_nonfinite(engine):
    """A read with -Inf table entries sends the launch to the general k_score.
    NaN positions of every chunked fold equal the one-shot fold's; a NaN
    planted in init stays NaN, and only there."""
    rng = np.random.default_rng(7700)
    # n = m = 20 at bandwidth 2: row 10 of the bad read has -Inf mismatch,
    # insertion and deletion scores, and the template carries the read's base
    # in columns 8-12 (every cell of that row inside the band), so the fills
    # are valid and a proposal that brings another base there is one the
    # reference raises on
    t = np.full(20, 2, np.uint8)
    t[7:12] = 1
    bad = RifrafSequence(t.copy(), np.full(20, -1.5), 2, SEQ_SCORES)
    for f in ("mismatch_scores", "ins_scores", "del_scores"):
        setattr(bad, f, np.array(getattr(bad, f), np.float64))
    bad.mismatch_scores[9] = bad.ins_scores[9] = bad.del_scores[10] = -np.inf
    reads = [read_of(t, 0, 3, rng), read_of(t, 1, 3, rng), bad, read_of(t, -1, 3, rng)]
    (slots,), _ = load(engine, [(t, reads)])
    whole = engine.score_dense([slots])[0]
    assert_score_launch(engine, "general", None)
    assert np.isnan(whole[1:]).any() and np.isfinite(whole[1:]).any()
    for cut in (1, 2, 3):
        first = engine.score_dense([slots[:cut]])
        got = engine.score_dense_from([slots[cut:]], first)[0]
        assert_same(got, whole, cut)
        assert np.array_equal(np.isnan(got), np.isnan(whole))
    ok = engine.score_dense([slots[:2]])          # the finite reads alone: the lean scorer
    assert np.isfinite(ok[0][1:]).all()
    planted = ok[0].copy()
    planted[5, 3] = planted[17, 8] = np.nan
    got = engine.score_dense_from([slots[:2]], [planted])[0]
    clean = engine.score_dense_from([slots[:2]], ok)[0]
    exp_nan = np.isnan(clean)
    exp_nan[5, 3] = exp_nan[17, 8] = True
    assert np.array_equal(np.isnan(got), exp_nan)
    assert same(got[~exp_nan], clean[~exp_nan]).all()


# ---------------------------------------------------------------------
# several groups: init rows land on the right group
# ---------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_several_groups(engine, opts, mode):
    rng = np.random.default_rng(7800)
    groups = [make_group(70, 5, 9, rng), make_group(12, 2, 3, rng), make_group(257, 3, 9, rng)]
    slots, _ = load(engine, groups)
    opts("score_mode", mode)
    whole = engine.score_dense(slots)
    cuts = (3, 1, 2)           # a distinct fold per group
    first = engine.score_dense([s[:k] for s, k in zip(slots, cuts)])
    assert not same(first[0][:13], first[1]).all()
    got = engine.score_dense_from([s[k:] for s, k in zip(slots, cuts)], first)
    for g in range(3):
        assert_same(got[g], whole[g], (mode, g))
        assert_oracle(got[g], groups[g][0], oracle.cpu_pass(*groups[g], nthreads=1)[0], ("oracle", mode, g))


# ---------------------------------------------------------------------
# device init / out
# ---------------------------------------------------------------------
def test_dev(engine):
    import torch
    rng = np.random.default_rng(7900)
    groups = [make_group(65, 4, 9, rng), make_group(7, 3, 3, rng)]
    slots, _ = load(engine, groups)
    whole = np.concatenate(engine.score_dense(slots))
    first = np.concatenate(engine.score_dense([s[:2] for s in slots]))
    rest = [s[2:] for s in slots]
    dev = torch.device("cuda", engine.device)
    buf = torch.from_numpy(first.copy()).to(dev)
    engine.score_dense_from_dev(rest, buf.data_ptr(), buf.data_ptr())          # in place
    torch.cuda.synchronize(dev)
    assert_same(buf.cpu().numpy(), whole, "in place")
    src = torch.from_numpy(first.copy()).to(dev)
    dst = torch.full_like(src, 7.0)
    engine.score_dense_from_dev(rest, src.data_ptr(), dst.data_ptr())
    torch.cuda.synchronize(dev)
    assert_same(dst.cpu().numpy(), whole, "two tensors")
    assert_same(src.cpu().numpy(), first, "init untouched")
    engine.score_dense_from_dev(slots, None, dst.data_ptr())                    # NULL init: rf_score_dense
    torch.cuda.synchronize(dev)
    assert_same(dst.cpu().numpy(), whole, "null init")
    pg_off = np.array([0, 2, 3], np.int32)
    rc = engine.lib.rf_score_dense_from_dev(engine.ctx, 2, ptr(pg_off), ptr(np.concatenate(rest)), None,
                                            src.data_ptr(), None)
    assert rc == RF_ERR_ARG
    assert_same(src.cpu().numpy(), first, "refused")


# ---------------------------------------------------------------------
# refusals: nothing changes, out included
# ---------------------------------------------------------------------
def test_refusals(engine):
    rng = np.random.default_rng(8000)
    groups = [make_group(20, 3, 3, rng), make_group(9, 2, 3, rng)]
    slots, _ = load(engine, groups)
    whole = np.concatenate(engine.score_dense(slots))
    first = np.concatenate(engine.score_dense([s[:1] for s in slots]))
    rest = np.concatenate([s[1:] for s in slots]).astype(np.int32)
    off = np.array([0, 2, 3], np.int32)
    sentinel = np.full_like(whole, -12345.0)
    out = sentinel.copy()
    call = lambda o, sl, refs: engine.lib.rf_score_dense_from(engine.ctx, 2, ptr(o), None if sl is None else ptr(sl),
                                                              None if refs is None else ptr(refs), ptr(first),
                                                              ptr(out))
    good = lambda: assert_same(np.concatenate(engine.score_dense_from([s[1:] for s in slots],
                                                                      [first[:21], first[21:]])), whole, "good call")
    assert call(off, None, None) == RF_ERR_ARG                                   # NULL slots
    assert np.array_equal(out, sentinel)
    good()
    assert call(np.array([0, 3, 3], np.int32), rest, None) == RF_ERR_ARG         # an empty group
    assert np.array_equal(out, sentinel)
    good()
    with pytest.raises(ValueError):                                              # wrong-length ref_slots
        engine.score_dense_from([s[1:] for s in slots], None, [-1])
    assert call(off, rest, np.array([99999, -1], np.int32)) == RF_ERR_ARG        # unknown reference slot
    assert np.array_equal(out, sentinel)
    good()
    engine.set_templates(1, [groups[1][0]])                                      # re-upload: group 1's bands are stale
    assert call(off, rest, None) == RF_ERR_STATE
    assert np.array_equal(out, sentinel)
    with pytest.raises(RifrafError):
        engine.score_dense_from([s[1:] for s in slots], [first[:21], first[21:]])
    k = np.concatenate(slots)
    engine.realign(k, k, [0] * 3 + [1] * 2, 3, RF_FWD | RF_BWD)
    good()
    assert call(off, rest, None) == 0
    assert_same(out, whole, "after the refusals")


# ---------------------------------------------------------------------
# rf_host_band_bytes against the arena
# ---------------------------------------------------------------------
@pytest.mark.parametrize("pad", (0, 1))
def test_band_bytes(engine, opts, pad):
    """Engine.host_band_bytes equals the A + B capacities rf_region_offsets
    reports after a fill into fresh slots, padded (RF_OPT_BAND_PAD 1: every
    call pads) and unpadded (0: none does)."""
    rng = np.random.default_rng(8100)
    opts("band_pad", pad)
    shapes = [(1, 1, 1), (5, 9, 2), (40, 33, 3), (64, 64, 9), (130, 120, 40), (70, 100, 31), (257, 250, 15)]
    t = [random_seq(m, rng) for _, m, _ in shapes]
    seqs = [RifrafSequence(random_seq(n, rng), np.full(n, -1.5), bw, SEQ_SCORES) for n, _, bw in shapes]
    engine.release_bands()
    engine.set_sequences(0, seqs)
    engine.set_templates(0, t)
    k = np.arange(len(shapes))
    engine.realign(k, k, k, [bw for _, _, bw in shapes], RF_FWD | RF_BWD)
    for s, (n, m, bw) in enumerate(shapes):
        caps = engine.band_region(s, RF_BAND_A)[1] + engine.band_region(s, RF_BAND_B)[1]
        assert engine.host_band_bytes(n, m, bw, pad=bool(pad)) == caps, (n, m, bw, pad)
    assert _lib.host_band_bytes(130, 120, 40, True) != _lib.host_band_bytes(130, 120, 40, False)
