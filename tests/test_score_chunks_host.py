"""The reads-per-workgroup rule of the split-mode scorers on the host
(rf_host_score_chunks, no GPU): how many consecutive reads of a group one
workgroup of k_score_segl / k_score_ws takes (rchunk) and the launch's grid.y.

Every rchunk computes the same bits, so no result can show a slip in this
arithmetic; these tests pin it to the rule of DESIGN.md §4 "Scoring planner",
written out here in Python integers (no overflow) independently of the C++.
"""
import itertools

import pytest

from rifraf_amd import _lib

SCORE_WGS, SEG_WGS = 2048, 262144   # the options' defaults


def rule(kernel, split, nitems, max_reads, score_wgs=SCORE_WGS, seg_wgs=SEG_WGS):
    """(rchunk, grid_y) by the written rule"""
    if not split:
        return 1, 1
    if kernel == "general":
        return 1, max_reads
    cells = nitems * max_reads
    if kernel == "seg":
        rchunk = max(1, -(-cells // max(seg_wgs, 1)))   # ceiling
    else:
        rchunk = max(1, cells // max(score_wgs, 1))     # floor
    return rchunk, -(-max_reads // rchunk)


def chunks(kernel, split, nitems, max_reads, **kw):
    return _lib.host_score_chunks(kernel, split, nitems, max_reads, **kw)


def test_defaults_at_the_benchmark_shapes():
    # c5: 157 items x 5,000 reads in k_score_segl; c3: 11 items x 1,000 reads in k_score_ws
    assert chunks("seg", True, 157, 5000) == (3, 1667)
    assert chunks("ws", True, 11, 1000) == (5, 200)
    assert rule("seg", True, 157, 5000) == (3, 1667) and rule("ws", True, 11, 1000) == (5, 200)
    # the other option does not enter
    assert chunks("seg", True, 157, 5000, score_wgs=1) == (3, 1667)
    assert chunks("ws", True, 11, 1000, seg_wgs=1) == (5, 200)


@pytest.mark.parametrize("kernel", ["general", "seg", "ws"])
def test_fused_and_general_take_no_chunks(kernel):
    for nitems, max_reads, wgs in itertools.product((1, 7, 3000), (1, 2, 11, 5000), (-3, 0, 1, 5, 2048)):
        assert chunks(kernel, False, nitems, max_reads, score_wgs=wgs, seg_wgs=wgs) == (1, 1)
        if kernel == "general":
            assert chunks(kernel, True, nitems, max_reads, score_wgs=wgs, seg_wgs=wgs) == (1, max_reads)


@pytest.mark.parametrize("kernel", ["seg", "ws"])
def test_small_shapes_follow_the_rule(kernel):
    seen = set()
    for nitems, max_reads, wgs in itertools.product((1, 2, 3, 4, 7, 8, 10, 12, 157), (1, 2, 4, 5, 11, 12, 1000),
                                                    (-2147483648, -1, 0, 1, 2, 3, 5, 10, 11, 13, 28, 37, 44, 55, 110,
                                                     2048, 262144, 2147483647)):
        kw = dict(score_wgs=wgs, seg_wgs=wgs)
        got = chunks(kernel, True, nitems, max_reads, **kw)
        assert got == rule(kernel, True, nitems, max_reads, **kw), (kernel, nitems, max_reads, wgs)
        rchunk, grid_y = got
        assert rchunk >= 1 and 1 <= grid_y <= max_reads
        assert (grid_y - 1) * rchunk < max_reads <= grid_y * rchunk   # the chunks cover the reads, the last not empty
        seen.add("above" if rchunk > max_reads else "equal" if rchunk == max_reads else "below")
    assert seen == {"above", "equal", "below"}


@pytest.mark.parametrize("kernel", ["seg", "ws"])
def test_options_below_one_count_as_one(kernel):
    for wgs in (0, -1, -2048, -2147483648):
        kw = dict(score_wgs=wgs, seg_wgs=wgs)
        assert chunks(kernel, True, 10, 11, **kw) == chunks(kernel, True, 10, 11, score_wgs=1, seg_wgs=1) == (110, 1)


@pytest.mark.parametrize("kernel", ["general", "seg", "ws"])
def test_one_item_of_one_read(kernel):
    for wgs in (0, 1, 2, 2048):
        assert chunks(kernel, True, 1, 1, score_wgs=wgs, seg_wgs=wgs) == (1, 1)


def test_rchunk_above_max_reads():
    # a whole group per workgroup, and more: grid.y 1
    assert chunks("seg", True, 10, 11, seg_wgs=6) == (19, 1)
    assert chunks("ws", True, 4, 11, score_wgs=2) == (22, 1)
    # the two roundings on one quotient: 110 / 28 = 3.93
    assert chunks("seg", True, 10, 11, seg_wgs=28) == (4, 3)
    assert chunks("ws", True, 10, 11, score_wgs=28) == (3, 4)
    # an exact quotient rounds neither way
    assert chunks("seg", True, 10, 11, seg_wgs=55) == chunks("ws", True, 10, 11, score_wgs=55) == (2, 6)


@pytest.mark.parametrize("kernel", ["seg", "ws"])
def test_products_beyond_2_31(kernel):
    # nitems * max_reads is taken in 64 bits
    for nitems, max_reads, wgs in ((65536, 65536, 262144), (100000, 100000, 2048), (2147483647, 2, 3),
                                   (3, 2147483647, 7), (46341, 46341, 1 << 20), (2147483647, 2147483647, 2147483647),
                                   (2147483647, 2147483647, 1 << 30)):
        assert nitems * max_reads > 2 ** 31
        kw = dict(score_wgs=wgs, seg_wgs=wgs)
        exp = rule(kernel, True, nitems, max_reads, **kw)
        if exp[0] >= 2 ** 31:   # rchunk is an int32 of the kernels
            continue
        assert chunks(kernel, True, nitems, max_reads, **kw) == exp, (nitems, max_reads, wgs)
    assert chunks("seg", True, 100000, 100000) == (38147, 3)
    assert chunks("ws", True, 100000, 100000) == (4882812, 1)


def test_bad_arguments():
    for args in (("seg", True, 0, 5), ("seg", True, 5, 0), ("ws", True, -1, 5), ("ws", False, 5, -1)):
        with pytest.raises(ValueError):
            chunks(*args)
    rchunk = _lib.c_int32()
    assert _lib.load().rf_host_score_chunks(0, 1, 1, 1, 1, 1, rchunk, rchunk) != 0    # no such family
    assert _lib.load().rf_host_score_chunks(4, 1, 1, 1, 1, 1, rchunk, rchunk) != 0
    assert _lib.load().rf_host_score_chunks(2, 1, 1, 1, 1, 1, None, rchunk) != 0
