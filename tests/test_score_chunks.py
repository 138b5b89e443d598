"""Split-mode k_score_segl and k_score_ws with several reads per workgroup,
and the host wait / stream options, against the CPU oracle (bit-exact).

In split mode a workgroup of either scorer takes `rchunk` consecutive reads
of a group (csrc/rifraf_score_plan.h score_chunks): it resets its chain state
between reads, writes one partial per read, and prefetches the next read's
first window while the current read's chains run.  rchunk follows from
RF_OPT_SEG_WGS / RF_OPT_SCORE_WGS and the launch's size, and at the defaults
every small launch has rchunk = 1; here the options are set from the launch's
item count so that rchunk takes 1, 2, 3, 4, max_reads - 1, max_reads and a
value above max_reads, and Engine.last_score_launch() must show the grid.y of
that rchunk.

One shape per kernel: four groups in one launch, of 4, 5, 1 and 11 reads
against templates of 63, 64, 130 and 200 columns.  Consecutive reads of a
group differ in bandwidth and in n - m, so that the reads of a chunk differ in
H, row stride and first diagonal.  k_score_ws cannot hold a column of the
segment scorer's widest reads in LDS (tests/test_score_plan_host.py), so its
shape has narrower wide reads; all else is the same.

Expected values are the oracle's alone: oracle.cpu_pass of a group for dense
and list totals, oracle.cpu_pass of each single read for per-read output.
What the inputs must exercise (partial last chunks, early-returning tail
workgroups, mixed strides in a chunk, a prefetch of diagonal D - 1 across a
read boundary, whole-read and sub-window units in one chunk) is established
from their geometry on the CPU (check_coverage) before the engine runs.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import oracle
from _util import SEQ_SCORES, all_proposals_arrays, dense_slot, inband_mask, random_seq
from rifraf_amd import RifrafSequence, _lib
from rifraf_amd.engine import RF_BAND_A, RF_BAND_B, RF_BWD, RF_FWD
from test_score_chunks_host import rule

pytestmark = pytest.mark.gpu

TEMPLATES = (63, 64, 130, 200)   # a last lane without a Substitution column; an item of one lane; interior items
COUNTS = (4, 5, 1, 11)           # at rchunk 4: a chunk, a chunk and one, less than a chunk, a partial last chunk
MAX_READS = max(COUNTS)
DELTAS = (30, -30, 0)            # n - m
BWS = {"seg": (60, 9, 100), "ws": (40, 9, 16)}
COLS = {"seg": 64, "ws": 256}    # columns per work item
OPTION = {"seg": "seg_wgs", "ws": "score_wgs"}
PADS = (0, 1, 64)                # RF_OPT_BAND_PAD: odd strides only, every row in whole lines, both
RCHUNKS = (1, 2, 3, 4, MAX_READS - 1, MAX_READS, "above")
LDS_DEFAULT = 160 * 1024 // 8    # doubles of LDS of k_score_ws
LDS_SMALL_KB = 112


# ---------------------------------------------------------------------
# the kernels' geometry, restated
# ---------------------------------------------------------------------
def band_H(n, m, bw):
    return 2 * bw + abs(n - m) + 1


def stride(H, pad):
    """the row stride of a band of a realign call whose widest band has H >= pad (pad > 0)"""
    return (((H + 1) >> 1) + 15) & ~15 if pad > 0 and H >= pad else ((H + 1) >> 1) | 1


def lean_need(L, H, P):
    win = ((2 * L + H + 1) * P + 3) & ~1
    return 2 * win + (L + H + 1) * 6


def seg_first_D(m, a0, n, bw):
    """k_score_segl's setup() and first_of(): the first segment of a read in
    the item of columns a0 .. a0 + 63 -- the lowest first diagonal of an
    active lane, rounded down to a multiple of 32"""
    c = max(m - n, 0) + bw
    dlo = min(max(0, min(a + 1, m) - c) - a + c for a in range(a0, a0 + 64) if a <= m)
    return dlo & ~31


def chunks_of(count, rchunk):
    return [range(r, min(r + rchunk, count)) for r in range(0, count, rchunk)]


# ---------------------------------------------------------------------
# inputs and oracle results, once per module
# ---------------------------------------------------------------------
def read_of(t, d, bw, rng):
    """t with d bases inserted (d > 0) or -d deleted, and about 2 % substitutions"""
    s = list(t)
    for _ in range(abs(d)):
        j = int(rng.integers(0, len(s) + (1 if d > 0 else 0)))
        if d > 0:
            s.insert(j, int(rng.integers(0, 4)))
        else:
            del s[j]
    s = np.array(s, np.uint8)
    sub = rng.random(len(s)) < 0.02
    s[sub] = (s[sub] + rng.integers(1, 4, int(sub.sum()))) % 4
    return RifrafSequence(s, rng.integers(8, 40, len(s)) / -10.0, bw, SEQ_SCORES)   # finite tables


def dense_mask(t):
    mask = np.ones((len(t) + 1, 9), bool)
    mask[0, :5] = False                         # p = 0 has no sub / del
    mask[np.arange(1, len(t) + 1), t] = False   # not a proposal
    return mask


def make_shape(kernel):
    rng = np.random.default_rng(5150 + len(kernel))
    sh = SimpleNamespace(kernel=kernel, tpls=[random_seq(m, rng) for m in TEMPLATES], reads=[], tpl_of=[], groups=[])
    for g, (t, count) in enumerate(zip(sh.tpls, COUNTS)):
        sh.groups.append(np.arange(len(sh.reads), len(sh.reads) + count))
        for k in range(g, g + count):   # the cycles start elsewhere in every group
            sh.reads.append(read_of(t, DELTAS[(k + k // 3) % 3], BWS[kernel][k % 3], rng))
            sh.tpl_of.append(g)
    sh.geo = [(len(r.seq), len(sh.tpls[g]), r.bandwidth) for r, g in zip(sh.reads, sh.tpl_of)]
    sh.H = [band_H(*x) for x in sh.geo]
    sh.nitems = sum(len(t) // COLS[kernel] + 1 for t in sh.tpls)
    check_coverage(sh)
    sh.props = [all_proposals_arrays(t) for t in sh.tpls]
    sh.mask = [dense_mask(t) for t in sh.tpls]
    sh.dense = [oracle.cpu_pass(t, [sh.reads[i] for i in g], nthreads=1)[0] for t, g in zip(sh.tpls, sh.groups)]
    sh.per_read = [oracle.cpu_pass(sh.tpls[g], [r], nthreads=1)[0] for r, g in zip(sh.reads, sh.tpl_of)]
    for a in sh.dense + sh.per_read:
        a.setflags(write=False)
    return sh


def check_coverage(sh):
    """What the sweep relies on, from the inputs alone."""
    kernel = sh.kernel
    assert len({len(r.seq) - len(sh.tpls[g]) for r, g in zip(sh.reads, sh.tpl_of)}) == 3
    for pad in PADS:
        P = [stride(H, pad) for H in sh.H]
        if pad == 64:   # both loaders of k_score_segl
            assert {p % 16 == 0 for p in P} == {True, False}
        else:
            assert {p % 16 == 0 for p in P} == {pad == 1}
        if kernel == "ws":   # a column of every read fits LDS: the launch stays in k_score_ws
            assert max(lean_need(1, H, p) for H, p in zip(sh.H, P)) <= LDS_DEFAULT
        for rchunk in (2, 3, 4):
            grid_y = -(-MAX_READS // rchunk)
            assert any(c > rchunk and c % rchunk for c in COUNTS)        # a partial last chunk
            assert any(c < (grid_y - 1) * rchunk for c in COUNTS)        # tail workgroups that return at once
            mixed = odd_even = False
            for g in sh.groups:
                for ch in chunks_of(len(g), rchunk):
                    ps = {P[g[r]] for r in ch}
                    mixed |= len(ps) > 1
                    odd_even |= len({p % 16 == 0 for p in ps}) > 1
            assert mixed and odd_even == (pad == 64), (pad, rchunk)
    if kernel == "seg":
        # the prefetch of diagonal D - 1 across a read boundary: a read that
        # is not the first of its chunk starts at a segment D > 0
        for rchunk in (2, 3, 4, MAX_READS - 1, MAX_READS):
            hit = [(g, a0, r) for g, grp in enumerate(sh.groups) for ch in chunks_of(len(grp), rchunk)
                   for r in ch[1:] for a0 in range(0, TEMPLATES[g] + 1, 64)
                   if seg_first_D(TEMPLATES[g], a0, *sh.geo[grp[r]][::2]) > 0]
            assert hit, rchunk
            # ... and in the item of a single active lane (m = 64, column 64)
            assert rchunk > 4 or any(g == 1 and a0 == 64 for g, a0, _ in hit), rchunk
    else:
        # whole-read and sub-window units in one chunk, at the default budget and at the small one
        for budget, pad in ((LDS_DEFAULT, 0), (LDS_DEFAULT, 1), (LDS_DEFAULT, 64), (LDS_SMALL_KB * 128, 0)):
            whole = [lean_need(256, H, stride(H, pad)) <= budget for H in sh.H]
            for rchunk in (2, 3, 4):
                assert any(len({whole[g[r]] for r in ch}) == 2 for g in sh.groups for ch in chunks_of(len(g), rchunk))
        # the small budget turns reads that were whole into sub-window reads
        assert sum(lean_need(256, H, stride(H, 0)) <= LDS_SMALL_KB * 128 for H in sh.H) < \
            sum(lean_need(256, H, stride(H, 0)) <= LDS_DEFAULT for H in sh.H)


_SHAPES = {}


@pytest.fixture(scope="module")
def shapes():
    def get(kernel):
        if kernel not in _SHAPES:
            _SHAPES[kernel] = make_shape(kernel)
        return _SHAPES[kernel]
    return get


# ---------------------------------------------------------------------
# the engine side
# ---------------------------------------------------------------------
def load(engine, opts, sh, pad):
    """The shape's bands at RF_OPT_BAND_PAD = pad.  A realign call pads all its
    bands or none, so at 64 the narrow reads go first, in a call of their own:
    odd and whole-line strides then meet in one scoring launch."""
    opts("band_pad", pad)
    engine.release_bands()
    engine.set_sequences(0, sh.reads)
    engine.set_templates(0, sh.tpls)
    ids = np.arange(len(sh.reads))
    calls = [ids] if pad != 64 else [ids[np.array(sh.H) < 64], ids[np.array(sh.H) >= 64]]
    for c in calls:
        assert len(c)
        engine.realign(c, c, np.array(sh.tpl_of)[c], [sh.reads[i].bandwidth for i in c], RF_FWD | RF_BWD)


def option_for(kernel, nitems, max_reads, want):
    """A value of the kernel's option at which the launch has rchunk = want
    ("above": more than max_reads); None if no value gives it"""
    for v in range(1, nitems * max_reads + 2):
        kw = {OPTION[kernel]: v}
        rchunk = rule(kernel, True, nitems, max_reads, **kw)[0]
        if rchunk == want or (want == "above" and rchunk > max_reads):
            return v
    return None


def set_chunks(opts, kernel, nitems, max_reads, want):
    v = option_for(kernel, nitems, max_reads, want)
    assert v is not None, (kernel, nitems, max_reads, want)
    opts(OPTION[kernel], v)
    rchunk, grid_y = _lib.host_score_chunks(kernel, True, nitems, max_reads, **{OPTION[kernel]: v})
    assert (rchunk, grid_y) == rule(kernel, True, nitems, max_reads, **{OPTION[kernel]: v})
    assert rchunk == want or (want == "above" and rchunk > max_reads)
    return rchunk, grid_y


def assert_launch(engine, kernel, nitems, max_reads, rchunk, grid_y):
    """the last scoring call ran `kernel` in split mode with rchunk reads per workgroup"""
    launch = engine.last_score_launch()
    assert (launch.kernel, launch.split, launch.items) == (kernel, True, nitems), launch
    assert launch.grid_y == grid_y, (launch, rchunk)
    if rchunk > 1:
        assert launch.grid_y < max_reads, launch


def score_all(engine, opts, sh, idx, kernel, rchunk, grid_y, entries=("dense", "list", "per_read")):
    """The groups idx of the shape through rf_score_dense, rf_score with every
    proposal and rf_score with per-read output, each against the oracle."""
    groups = [sh.groups[g] for g in idx]
    nitems = sum(len(sh.tpls[g]) // COLS[kernel] + 1 for g in idx)
    max_reads = max(len(g) for g in groups)
    lists = [(sh.groups[g], -1, sh.props[g]) for g in idx]
    opts("score_kernel", kernel)
    if "dense" in entries:
        opts("score_mode", "split")
        got = engine.score_dense(groups)
        assert_launch(engine, kernel, nitems, max_reads, rchunk, grid_y)
        for k, g in enumerate(idx):
            np.testing.assert_array_equal(got[k][sh.mask[g]], sh.dense[g][sh.mask[g]], err_msg=f"dense, group {k}")
    if "list" in entries:
        opts("score_mode", "split")
        tots = engine.score(lists)
        assert_launch(engine, kernel, nitems, max_reads, rchunk, grid_y)
        for k, g in enumerate(idx):
            kd, p, b = sh.props[g]
            np.testing.assert_array_equal(tots[k], sh.dense[g][p, dense_slot(kd, b)], err_msg=f"list, group {k}")
    if "per_read" in entries:
        opts("score_mode", "auto")   # per-read output is split mode by itself
        tots, per = engine.score(lists, per_seq=True)
        assert_launch(engine, kernel, nitems, max_reads, rchunk, grid_y)
        for k, g in enumerate(idx):
            kd, p, b = sh.props[g]
            slot = dense_slot(kd, b)
            assert per[k].shape == (len(kd), len(sh.groups[g]))
            for r, i in enumerate(sh.groups[g]):
                np.testing.assert_array_equal(per[k][:, r], sh.per_read[i][p, slot],
                                              err_msg=f"per read, group {k}, read {r} of {len(sh.groups[g])}")
            np.testing.assert_array_equal(tots[k], sh.dense[g][p, slot], err_msg=f"per-read call's totals, group {k}")


@pytest.mark.parametrize("want", RCHUNKS)
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("kernel", ["seg", "ws"])
def test_chunked_reads(engine, opts, shapes, kernel, pad, want):
    """Every rchunk, both kernels, the three entry points.  k_score_ws has 4
    items here, and floor(4 * 11 / score_wgs) is never 10: the launch of
    max_reads - 1 lists the four groups three times (12 items)."""
    sh = shapes(kernel)
    assert sh.nitems == {"seg": 10, "ws": 4}[kernel]
    idx = [0, 1, 2, 3]
    if option_for(kernel, sh.nitems, MAX_READS, want) is None:
        assert (kernel, want) == ("ws", MAX_READS - 1)
        idx = idx * 3
    load(engine, opts, sh, pad)
    rchunk, grid_y = set_chunks(opts, kernel, sh.nitems * len(idx) // 4, MAX_READS, want)
    score_all(engine, opts, sh, idx, kernel, rchunk, grid_y)


# k_score_segl deals its (item, chunk) cells to the workgroups in eight
# interleaved runs (lin & 7 over ncell = items * grid.y): launches of fewer
# than 8 cells, of exactly 8, and of more that are no multiple of 8
SWIZZLE = [
    # groups, rchunk, cells
    ([3], MAX_READS, 4), ([3], 6, 8), ([3], 4, 12), ([1], 2, 6), ([1], 1, 10),
    ([0, 2], 4, 4), ([0, 2], 3, 8), ([0, 2], 2, 8), ([0, 2], 1, 16),
]


@pytest.mark.parametrize("idx,want,cells", SWIZZLE)
def test_seg_cell_swizzle_edges(engine, opts, shapes, idx, want, cells):
    sh = shapes("seg")
    nitems = sum(TEMPLATES[g] // 64 + 1 for g in idx)
    max_reads = max(COUNTS[g] for g in idx)
    load(engine, opts, sh, 64)
    rchunk, grid_y = set_chunks(opts, "seg", nitems, max_reads, want)
    assert nitems * grid_y == cells
    score_all(engine, opts, sh, idx, "seg", rchunk, grid_y, entries=("dense", "per_read"))


def test_swizzle_cases_cover_the_edges():
    assert {c < 8 for _, _, c in SWIZZLE} == {True, False} and any(c == 8 for _, _, c in SWIZZLE)
    assert any(c > 8 and c % 8 for _, _, c in SWIZZLE)


@pytest.mark.parametrize("want", [2, 3, 4, MAX_READS])
def test_ws_sub_window_units_in_chunks(engine, opts, shapes, want):
    """k_score_ws under a smaller LDS budget: more of the reads run as sub-
    window units, beside whole reads in the same chunk (check_coverage)."""
    sh = shapes("ws")
    load(engine, opts, sh, 0)
    opts("lean_lds_kb", LDS_SMALL_KB)
    rchunk, grid_y = set_chunks(opts, "ws", sh.nitems, MAX_READS, want)
    score_all(engine, opts, sh, [0, 1, 2, 3], "ws", rchunk, grid_y)


# ---------------------------------------------------------------------
# host waits and DP streams
# ---------------------------------------------------------------------
def final_cell(A, n, m, bw):
    return A[n - m + max(m - n, 0) + bw, m]


@pytest.fixture(scope="module")
def sequence():
    """One template, lean reads of four DP classes, and the oracle's bands,
    walks and dense totals."""
    rng = np.random.default_rng(977)
    c = SimpleNamespace(t=random_seq(150, rng), reads=[])
    for bw, d in ((9, 0), (9, 2), (9, -1), (23, 0), (23, 3), (40, 0), (40, -4), (80, 0), (80, 5)):
        c.reads.append(read_of(c.t, d, bw, rng))
    c.bws = [r.bandwidth for r in c.reads]
    c.A, c.B, c.walk, c.nerr = [], [], [], []
    for s in c.reads:
        A, mv = oracle.forward(c.t, s, moves=True)
        w = oracle.backtrace(mv, len(s.seq) + 1, len(c.t) + 1, s.bandwidth)
        c.A.append(A)
        c.B.append(oracle.backward(c.t, s))
        c.walk.append(w)
        c.nerr.append(oracle.count_errors(w, c.t, s.seq))
    c.dense = oracle.cpu_pass(c.t, c.reads, nthreads=1)[0]
    return c


@pytest.mark.parametrize("dp_streams", [0, 1])
@pytest.mark.parametrize("sync_block", [0, 1])
def test_host_wait_and_stream_options(engine, opts, sequence, sync_block, dp_streams):
    """RF_OPT_SYNC_BLOCK (spinning or yielding host waits) and
    RF_OPT_DP_STREAMS (DP classes on side streams or all on the context's)
    through one call sequence: a realign of several DP classes, backtrace,
    dense scoring and pair alignment, every output the oracle's."""
    c = sequence
    opts("sync_block", sync_block)
    opts("dp_streams", dp_streams)
    opts("band_pad", 64)
    engine.release_bands()
    engine.set_sequences(0, c.reads)
    engine.set_templates(0, [c.t])
    n, m = len(c.reads), len(c.t)
    ids = np.arange(n)
    scores = engine.realign(ids, ids, 0, c.bws, RF_FWD | RF_BWD)
    launches = engine.last_dp_launches()
    assert len({L.kernel for L in launches}) >= 3, launches
    if dp_streams == 0:
        assert {L.stream for L in launches} == {-1}, launches
    for k, s in enumerate(c.reads):
        mask = inband_mask(len(s.seq) + 1, m + 1, c.bws[k])
        for which, exp in ((RF_BAND_A, c.A[k]), (RF_BAND_B, c.B[k])):
            got = engine.download_band(k, which).data
            np.testing.assert_array_equal(got[mask], np.asarray(exp)[mask], err_msg=f"band {which} of read {k}")
        assert scores[k] == final_cell(c.A[k], len(s.seq), m, c.bws[k])
    moves, nerr = engine.backtrace(ids)
    for k in range(n):
        np.testing.assert_array_equal(moves[k], c.walk[k], err_msg=f"walk of read {k}")
    assert list(nerr) == c.nerr
    got = engine.score_dense([ids])[0]
    assert engine.last_score_launch().items > 0
    mask = dense_mask(c.t)
    np.testing.assert_array_equal(got[mask], c.dense[mask])
    pscores, pmoves, pnerr = engine.pair_align(ids, 0, c.bws)
    for k, s in enumerate(c.reads):
        assert pscores[k] == final_cell(c.A[k], len(s.seq), m, c.bws[k])
        np.testing.assert_array_equal(pmoves[k], c.walk[k], err_msg=f"pair walk of read {k}")
    assert list(pnerr) == c.nerr
