"""The scoring planner on the host (rf_host_score_plan, no GPU): which scorer
a launch takes, its work items, fused or split mode and the group layout.

The three scorers, both modes and both item widths compute the same bits, so
no result can show a routing slip; these tests pin the routing itself.  Each
expectation is worked out from the rules of DESIGN.md §4 "Scoring planner".

A read is given by its band height H = 2 bw + |n - m| + 1: n = m and bw =
(H - 1) / 2 for odd H, n = m + 1 and bw = (H - 2) / 2 for even H.
"""
import numpy as np
import pytest

from rifraf_amd import _lib

BUDGET = 160 * 1024 // 8   # doubles of LDS k_score_ws may take


def band_P(H):
    """the unpadded row stride"""
    return ((H + 1) >> 1) | 1


def padded(H):
    """the stride of a band in rows of whole 128-B lines"""
    return (((H + 1) >> 1) + 15) & ~15


def lean_need(L, H, P):
    """doubles of LDS of a k_score_ws pass over L lanes: both bands' kappa
    rows (evened, with the alignment shift) and six table values per row"""
    win = ((2 * L + H + 1) * P + 3) & ~1
    return 2 * win + (L + H + 1) * 6


def read(H, m, finite=True, stride=None):
    n = m + (H + 1) % 2
    bw = (H - 1 - (H + 1) % 2) // 2
    assert bw >= 1 and 2 * bw + abs(n - m) + 1 == H
    return dict(n=n, m=m, bw=bw, finite=finite, stride=stride or band_P(H))


def plan(groups, **kw):
    """groups: a list of lists of reads"""
    reads = [r for g in groups for r in g]
    off = np.cumsum([0] + [len(g) for g in groups])
    col = lambda k: np.array([r[k] for r in reads], np.int64)
    return _lib.host_score_plan(col("n"), col("m"), col("bw"), off, stride=col("stride"), finite=col("finite"), **kw)


def items_of(groups, cols):
    return [(g, p0) for g, rs in enumerate(groups) if rs for p0 in range(0, rs[0]["m"] + 1, cols)]


# -- pick ---------------------------------------------------------------

def test_fit_boundary_follows_lean_need():
    fits = [H for H in range(3, 64) if lean_need(256, H, band_P(H)) <= BUDGET]
    Hfit = max(fits)
    assert fits == list(range(3, Hfit + 1))   # one boundary
    assert lean_need(256, Hfit + 1, band_P(Hfit + 1)) > BUDGET
    p = plan([[read(Hfit, 80), read(9, 80)]])
    assert (p.kernel, p.cols, p.lds) == ("ws", 256, BUDGET)
    # a launch of one read whose window does not fit: all of its cells are wide
    assert plan([[read(Hfit + 1, 80)]]).kernel == "seg"


def test_seg_once_wide_reads_hold_more_than_half():
    Hw = next(H for H in range(3, 64) if lean_need(256, H, band_P(H)) > BUDGET)
    wide = read(Hw, 50)
    cells = wide["n"] * Hw               # the weight of a read: n * H
    assert cells % 5 == 0
    for extra, kernel in ((0, "ws"), (1, "ws"), (-1, "seg")):   # the exact half still goes to ws
        narrow = read(5, cells // 5 + extra)                     # n * H = cells + 5 * extra
        p = plan([[wide], [narrow]])
        assert p.kernel == kernel, extra
        assert p.cols == (256 if kernel == "ws" else 64)


def test_nonfinite_read_sends_the_launch_general():
    g = [[read(9, 40), read(9, 40, finite=False)], [read(11, 30)]]
    p = plan(g)
    assert (p.kernel, p.cols) == ("general", 64)
    # k_score's staging buffer: the 90th-percentile window of 2 * 64 + H rows, at most 24 KB
    w = sorted((128 + H) * band_P(H) for H in (9, 9, 11))
    assert p.lds == min(w[(3 * 9) // 10], 24 * 1024 // 8)
    assert plan([[read(9, 40)], [read(11, 30)]]).kernel == "ws"


def test_score_kernel_forces_its_family():
    Hw = next(H for H in range(3, 64) if lean_need(256, H, band_P(H)) > BUDGET)
    narrow, wide = [[read(9, 40)]], [[read(Hw, 40)]]
    assert plan(narrow, score_kernel=1).kernel == "general"
    assert plan(narrow, score_kernel=2).kernel == "seg"
    assert plan(wide).kernel == "seg" and plan(wide, score_kernel=3).kernel == "ws"
    # -Inf tables leave only the general scorer, whatever is asked for
    for k in (0, 1, 2, 3):
        assert plan([[read(9, 40, finite=False)]], score_kernel=k).kernel == "general"


def test_forced_ws_yields_to_seg_when_one_column_exceeds_lds():
    # need1: a pass over a single lane
    H1 = next(H for H in range(3, 400) if lean_need(1, H, band_P(H)) > BUDGET)
    p = plan([[read(H1 - 1, 60)]], score_kernel=3)
    assert (p.kernel, p.lds) == ("ws", BUDGET)
    assert plan([[read(H1, 60)]], score_kernel=3).kernel == "seg"


def test_padded_stride_counts_in_the_fit():
    # H >= 64: a band in 128-B-line rows; the stride, not H alone, decides
    H = next(H for H in range(64, 400) if lean_need(1, H, band_P(H)) <= BUDGET < lean_need(1, H, padded(H)))
    assert plan([[read(H, 70)]], score_kernel=3).kernel == "ws"
    assert plan([[read(H, 70, stride=padded(H))]], score_kernel=3).kernel == "seg"


def test_lean_lds_kb_moves_the_budget():
    H = next(H for H in range(3, 64) if lean_need(256, H, band_P(H)) > 64 * 1024 // 8)
    assert lean_need(256, H, band_P(H)) <= BUDGET
    assert plan([[read(H, 40)]]).kernel == "ws"
    assert plan([[read(H, 40)]], lean_lds_kb=64).kernel == "seg"


# -- items --------------------------------------------------------------

@pytest.mark.parametrize("kernel,cols", [("general", 64), ("seg", 64), ("ws", 256)])
def test_items(kernel, cols):
    groups = [[read(9, 63)], [read(9, 64)], [], [read(9, 255), read(9, 255)], [read(9, 256)], [read(9, 257)]]
    p = plan(groups, score_kernel=_lib.OPTION_VALUES["score_kernel"][kernel])
    assert (p.kernel, p.cols) == (kernel, cols)
    assert p.items == items_of(groups, cols)
    counts = [sum(1 for g, _ in p.items if g == k) for k in range(len(groups))]
    assert counts == ([1, 2, 0, 4, 5, 5] if cols == 64 else [1, 1, 0, 1, 2, 2])


# -- split --------------------------------------------------------------

@pytest.mark.parametrize("nitems", [2047, 2048])
@pytest.mark.parametrize("max_reads", [1, 2])
def test_split_threshold(nitems, max_reads):
    m = (nitems - 1) * 64   # m // 64 + 1 items of 64 columns
    p = plan([[read(3, m)] * max_reads], score_kernel=1)
    assert len(p.items) == nitems
    want = nitems < 2048 and max_reads > 1
    assert (p.split_score, p.split_dense) == (want, want)


def test_split_counts_64_column_items_in_rf_score_only():
    # k_score_ws has a quarter of the items; rf_score decides by the 64-column count all the same
    p = plan([[read(3, 2047 * 64)] * 2])
    assert p.kernel == "ws" and len(p.items) == 512
    assert (p.split_score, p.split_dense) == (False, True)


def test_score_mode_and_per_seq():
    few, many = [[read(9, 40)] * 2], [[read(3, 2047 * 64)] * 2]
    for g in (few, many):
        fused = plan(g, score_mode=1)
        assert (fused.split_score, fused.split_dense) == (False, False)
        split = plan(g, score_mode=2)
        assert (split.split_score, split.split_dense) == (True, True)
        # per-read scores exist only in split mode: per_seq overrides fused, in rf_score alone
        per = plan(g, score_mode=1, per_seq=True)
        assert (per.split_score, per.split_dense) == (True, False)
    assert plan(many, score_kernel=1, per_seq=True).split_score
    one = plan([[read(9, 40)]])
    assert (one.split_score, one.split_dense) == (False, False)


# -- layout -------------------------------------------------------------

def test_layout_of_groups_of_0_1_3_reads():
    groups = [[read(9, 40)] * 3, [], [read(9, 27)]]
    p = plan(groups)
    assert p.dense_off == [0, 41 * 9, 41 * 9, 41 * 9 + 28 * 9]
    assert p.split_off == [0, 0, 3 * 41 * 9]
    assert p.items == [(0, 0), (2, 0)]
    with pytest.raises(ValueError):
        plan(groups, empty_ok=False)
    assert plan([groups[0], groups[2]], empty_ok=False).dense_off == [0, 41 * 9, 41 * 9 + 28 * 9]
