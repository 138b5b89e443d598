"""The wide-band DP fills at thin, skewed and short-template shapes.

A band has more than 2,040 rows whenever |n - m| is large (H = 2 bw +
|n - m| + 1), not only when m ~ n and bw ~ m / 2 as in the other tests of
k_dpm (test_gpu_parity.test_dpm_*, test_dp_huge_band_global_ring,
test_dp_band_beyond_lds_ring).  There the DP is a thin stripe through the
band: a row pair is in the DP for min(m, n) + 1 periods only, the compute
phases [Pa, Pb] of k_dpm's slices are short and staggered, and many slices
hold no DP cell at all (Pa > Pb).  test_dp_short_and_skewed_shapes has this
family for the narrow kernels (H < 64); this module has it for k_dpm, for its
dp_mc = 0 stand-ins k_dp<DPW_NT> with the LDS ring (H <= 5,114) and the
global ring, and for k_bt_win walking such a band.

The CPU tests show that each case of the table is what it is listed for:
they restate k_dpm's per-pair ranges (`lo`, `hi`) and per-slice compute
phases on the host (slice_phases) and ask rf_host_dp_plan for the routing.
Nothing in them is measured.  The GPU tests hold bands, scores, moves and
error counts to the oracle bit for bit, name the kernel family that ran, and
look at every downloaded cell -- in the DP or not -- for the all-ones pattern
the host fills a k_dpm band with before the launch.
"""
import functools

import numpy as np
import pytest

import oracle
from _util import SEQ_SCORES, random_seq
from rifraf_amd import RifrafSequence, _lib
from rifraf_amd.engine import RF_BAND_A, RF_BAND_B, RF_BWD, RF_FWD, RF_SKEW, RF_TRIM
from test_gpu_parity import _check_bands, assert_band_equal, launched_tasks

# k_dpm's slice geometry (rifraf_dp_plan.h; _lib exposes none of it): DPM_OWN =
# 64 * DPM_NPL - DPM_B = 32 row pairs per slice, DPM_B / 2 = 16 halo pairs on
# each side (DPM_NPL = 1, DPM_B = 32; rifraf_hip.hip static_asserts DPM_OWN > 0
# and 128 % DPM_B == 0).  DP_GEN64_H = 2040 and DP_LDS_H = 5114 are the band
# limits of the planner there.
OWN, HALO = 32, 16
GEN64_H, LDS_H = 2040, 5114

THIN, SHORT, EDGE = "thin", "short", "edge"
FIRST, LAST, INTERIOR = "first", "last", "interior"

# (m, n, bw): (families, where the origin's pair c // 2 lies in its slice,
# where the final cell's pair (n + c) // 2 does).  "last" is the last pair a
# slice owns: pair 31 of 32, or the band's last pair in the last slice.
CASES = {
    # thin, long read
    (30, 2200, 9): ((THIN,), INTERIOR, INTERIOR),
    (30, 2201, 9): ((THIN,), INTERIOR, INTERIOR),
    (1, 2100, 1): ((THIN,), FIRST, LAST),          # pair 0; the band's last pair
    (5, 2150, 3): ((THIN,), INTERIOR, INTERIOR),
    (15, 2150, 9): ((THIN,), INTERIOR, INTERIOR),
    (16, 2150, 9): ((THIN,), INTERIOR, INTERIOR),
    (17, 2151, 9): ((THIN,), INTERIOR, INTERIOR),
    (33, 2200, 12): ((THIN,), INTERIOR, INTERIOR),
    # thin, long template
    (2200, 30, 9): ((THIN,), INTERIOR, INTERIOR),
    (2201, 30, 9): ((THIN,), INTERIOR, INTERIOR),
    (2100, 1, 1): ((THIN,), LAST, LAST),           # both in the band's last pair
    (2150, 16, 9): ((THIN,), INTERIOR, INTERIOR),
    # template or read shorter than the bandwidth
    (5, 200, 1100): ((SHORT,), INTERIOR, INTERIOR),
    (200, 5, 1100): ((SHORT,), INTERIOR, INTERIOR),
    (40, 41, 1030): ((SHORT,), INTERIOR, INTERIOR),
    # past the LDS ring, thin
    (20, 5300, 9): ((THIN,), INTERIOR, INTERIOR),
    # No bandwidth within two of the cases above puts the final cell in the
    # first pair of a slice, or either cell in pair 31 of 32: these two do.
    (30, 2174, 64): ((THIN, EDGE), FIRST, LAST),   # pair 32 = 1 * 32; pair 1119 = 34 * 32 + 31
    (30, 2114, 62): ((THIN, EDGE), LAST, FIRST),   # pair 31; pair 1088 = 34 * 32
}
CASE_LIST = list(CASES)
FLAG_CASES = [(30, 2200, 9), (2200, 30, 9), (1, 2100, 1), (5, 200, 1100)]
# the mixed call: (n, bw) of five reads on one template of 30 bases
MIXED_M = 30
MIXED = [(2200, 9), (2500, 9), (2300, 40), (2100, 1030), (35, 9)]


def geometry(m, n, bw):
    """(c, H, row pairs, slices, first and last band row with DP cells)."""
    c = bw + max(m - n, 0)
    H = 2 * bw + abs(n - m) + 1
    pairs = (H + 1) // 2
    return c, H, pairs, (pairs + OWN - 1) // OWN, max(c - m, 0), min(n + c, H - 1)


def slice_phases(m, n, bw):
    """k_dpm's compute phase (Pa, Pb) of every slice, None for a slice none of
    whose pairs -- its own and the halo -- holds a DP cell (Pa > Pb in the
    kernel).  Cell (pair pp, parity a) is band row d = 2 pp + a; it is in the
    DP at the periods P in [lo, hi]: jj = P - pp in [0, m] and ii = pp + a +
    P - c in [0, n]."""
    c, H, pairs, G, _, _ = geometry(m, n, bw)
    out = []
    for g in range(G):
        pa, pb = None, None
        for pp in range(OWN * g - HALO, OWN * g + OWN + HALO):
            for a in (0, 1):
                lo, hi = max(pp, c - pp - a), min(pp + m, n + c - pp - a)
                if pp >= 0 and 2 * pp + a < H and lo <= hi:
                    pa = lo if pa is None else min(pa, lo)
                    pb = hi if pb is None else max(pb, hi)
        out.append(None if pa is None else (pa, pb))
    return out


def empty_slices_by_rows(m, n, bw):
    """The slices whose pairs, own and halo, all lie outside the band rows
    with DP cells: how many before those rows, how many behind."""
    _, H, _, G, d0, d1 = geometry(m, n, bw)
    before = behind = 0
    for g in range(G):
        rows = [d for d in range(2 * (OWN * g - HALO), 2 * (OWN * g + OWN + HALO)) if 0 <= d < H]
        before += all(d < d0 for d in rows)
        behind += all(d > d1 for d in rows)
    return before, behind


def where_in_slice(pp, pairs):
    own_lo = pp // OWN * OWN
    own_hi = min(own_lo + OWN, pairs)
    return FIRST if pp == own_lo else LAST if pp == own_hi - 1 else INTERIOR


def expected_family(H, mc):
    return "dpm" if mc else ("dpw_lds" if H <= LDS_H else "dpw_global")


def disjoint_phases(ph):
    """Some slice starts its compute phase after another has ended its own."""
    live = [p for p in ph if p is not None]
    return max(p[0] for p in live) > min(p[1] for p in live)


# ---------------------------------------------------------------------
# CPU: the cases are what they are listed for
# ---------------------------------------------------------------------

@pytest.mark.parametrize("m,n,bw", CASE_LIST + [(MIXED_M, n, bw) for n, bw in MIXED[:4]])
def test_cases_are_wide(m, n, bw):
    assert geometry(m, n, bw)[1] > GEN64_H


@pytest.mark.parametrize("mc", [1, 0])
@pytest.mark.parametrize("m,n,bw,flags", [c + (0,) for c in CASE_LIST] +
                         [c + (f,) for c in FLAG_CASES for f in (RF_SKEW, RF_TRIM, RF_SKEW | RF_TRIM)])
def test_cases_route_to_the_wide_kernels(m, n, bw, flags, mc):
    """rf_host_dp_plan with the case's own n, m, bw and flags: k_dpm under
    dp_mc = 1; under dp_mc = 0 k_dp<DPW_NT> with the LDS ring up to 5,114 rows
    and with the global ring above.  Both directions in one launch."""
    H = geometry(m, n, bw)[1]
    dirs = RF_FWD if flags else RF_FWD | RF_BWD
    _, _, _, _, launches = _lib.host_dp_plan([n], [m], [bw], dirs | flags, dp_mc=mc, dp_lat=0)
    assert [(L.kernel, L.count) for L in launches] == [(expected_family(H, mc), 1 if flags else 2)]
    if mc:
        assert launches[0].grid == 8 * geometry(m, n, bw)[3]   # one workgroup per slice, on one XCD of eight


def test_mixed_call_routes_wide_bands_to_one_launch():
    """The mixed call's four wide bands are one k_dpm launch in both
    directions (eight tasks) beside the narrow read's lean class."""
    ns, bws = [n for n, _ in MIXED], [bw for _, bw in MIXED]
    tj, _, tl, _, launches = _lib.host_dp_plan(ns, [MIXED_M] * 5, bws, RF_FWD | RF_BWD, dp_lat=0)
    dpm = [i for i, L in enumerate(launches) if L.kernel == "dpm"]
    assert len(dpm) == 1 and launches[dpm[0]].count == 8
    assert sorted(tj[tl == dpm[0]].tolist()) == [0, 0, 1, 1, 2, 2, 3, 3]
    assert sum(L.count for L in launches if L.kernel != "dpm") == 2
    # bands of different slice counts; the thin stripes cross every slice of
    # theirs, bw 1030 on 30 bases leaves 15 empty slices on each side
    counts = [(len(ph), sum(p is None for p in ph)) for ph in (slice_phases(MIXED_M, n, bw) for n, bw in MIXED[:4])]
    assert counts == [(35, 0), (39, 0), (37, 0), (65, 30)]
    assert empty_slices_by_rows(MIXED_M, *MIXED[3]) == (15, 15)


@pytest.mark.parametrize("m,n,bw", CASE_LIST)
def test_empty_slices_agree_with_dp_rows(m, n, bw):
    """The per-pair ranges and the band rows with DP cells, d in [max(c - m,
    0), min(n + c, H - 1)], name the same empty slices."""
    ph = slice_phases(m, n, bw)
    before, behind = empty_slices_by_rows(m, n, bw)
    live = [g for g, p in enumerate(ph) if p is not None]
    assert live == list(range(live[0], live[-1] + 1))
    assert (before, behind) == (live[0], len(ph) - 1 - live[-1])
    assert all(p[0] <= p[1] for p in ph if p is not None)


@pytest.mark.parametrize("m,n,bw", [c for c in CASE_LIST if THIN in CASES[c][0]])
def test_thin_cases_have_disjoint_compute_phases(m, n, bw):
    """A thin band has slices whose compute phases do not meet: one starts
    after another has ended.

    This cannot hold between two adjacent slices, at any shape: they hold 32
    pairs in common (the upper half of one slice and its halo are the lower
    halo and half of the next), the band rows with DP cells are contiguous,
    and a phase spans the periods of every pair the slice holds; so the
    phases of two adjacent non-empty slices share at least those pairs'
    periods (asserted below).  What thin bands have, and the bands of
    test_dpm_* (m ~ n, bw ~ m / 2) have not, is that slices a few steps apart
    never compute at the same period: the fill is a chain of short staggered
    phases, each started by hand-offs from a neighbour that is itself about
    to end."""
    ph = slice_phases(m, n, bw)
    assert disjoint_phases(ph)
    for p, q in zip(ph, ph[1:]):
        if p is not None and q is not None:
            assert min(p[1], q[1]) >= max(p[0], q[0])
    # a cell is in the DP for min(m, n) + 1 periods; the phase of a slice of
    # 64 pairs of two cells is at most that and one period per further cell
    assert max(p[1] - p[0] + 1 for p in ph if p is not None) <= 65 + min(m, n)


def test_fat_bands_have_no_disjoint_compute_phases():
    """The shape of the other k_dpm tests: every slice's phase meets every other's."""
    assert not disjoint_phases(slice_phases(2300, 2300, 1100))
    assert not disjoint_phases(slice_phases(3400, 3580, 1700))


def test_thin_cases_straddle_the_hand_off_interval():
    """A pair's min(m, n) + 1 periods in the DP: fewer than the 16 periods
    between two hand-offs, exactly 16, and more."""
    spans = {min(m, n) + 1 for (m, n, bw), v in CASES.items() if THIN in v[0]}
    assert min(spans) == 2 and {16, 17, 18} <= spans and max(spans) > 2 * HALO


@pytest.mark.parametrize("m,n,bw", [c for c in CASE_LIST if SHORT in CASES[c][0]])
def test_short_cases_have_empty_slices_on_both_sides(m, n, bw):
    assert min(m, n) < bw
    before, behind = empty_slices_by_rows(m, n, bw)
    assert before >= 8 and behind >= 8
    ph = slice_phases(m, n, bw)
    assert all(p is None for p in ph[:before]) and all(p is None for p in ph[len(ph) - behind:])


@pytest.mark.parametrize("m,n,bw", CASE_LIST)
def test_origin_and_final_pairs_are_where_listed(m, n, bw):
    c, _, pairs, _, _, _ = geometry(m, n, bw)
    _, org, fin = CASES[(m, n, bw)]
    assert where_in_slice(c // 2, pairs) == org
    assert where_in_slice((n + c) // 2, pairs) == fin


def test_cases_cover_parities_and_pair_positions():
    assert {(geometry(*k)[1] + 2 * k[0]) % 2 for k in CASES} == {0, 1}          # K = H + 2 m
    assert {v[1] for v in CASES.values()} == {FIRST, LAST, INTERIOR}             # the origin's pair
    assert {v[2] for v in CASES.values()} == {FIRST, LAST, INTERIOR}             # the final cell's pair
    # ... and not only through the band's first and last pair
    inner = [(c // 2, (n + c) // 2) for (m, n, bw) in CASES for c in [geometry(m, n, bw)[0]]]
    assert any(o % OWN == 0 and o > 0 for o, _ in inner) and any(o % OWN == OWN - 1 for o, _ in inner)
    assert any(f % OWN == 0 for _, f in inner) and any(f % OWN == OWN - 1 for _, f in inner)
    assert {geometry(*k)[1] > LDS_H for k in CASES} == {False, True}
    assert set(FLAG_CASES) <= set(CASES)


# ---------------------------------------------------------------------
# GPU: parity with the oracle at those shapes
# ---------------------------------------------------------------------

def make_case(m, n, bw):
    """The template and the read of a case: random bases, error_log_p drawn
    as in test_dp_short_and_skewed_shapes."""
    rng = np.random.default_rng(m * 100 + n)
    t = random_seq(m, rng)
    return t, RifrafSequence(random_seq(n, rng), np.log10(rng.uniform(0.01, 0.3, n)), bw, SEQ_SCORES)


@functools.lru_cache(maxsize=1)
def reference(m, n, bw, skew=False, trim=False, backward=True):
    """The oracle's bands and moves of a case, once for both dp_mc values
    (the parametrisation runs them one after the other)."""
    t, s = make_case(m, n, bw)
    A, mv = oracle.forward(t, s, moves=True, skew=skew, trim=trim)
    B = oracle.backward(t, s) if backward else None
    moves = oracle.backtrace(mv, n + 1, m + 1, bw)
    for a in (A, B, moves):
        if a is not None:
            a.setflags(write=False)
    return t, s, A, B, moves, oracle.count_errors(moves, t, s.seq)


def assert_no_fill_pattern(band, m, n, bw):
    """No downloaded cell, in the DP or not, holds the all-ones pattern, and
    the band rows without any DP cell hold -Inf."""
    _, H, _, _, d0, d1 = geometry(m, n, bw)
    assert band.data.shape == (H, m + 1)
    left = band.data.view(np.uint64) == np.uint64(2**64 - 1)
    assert not left.any(), f"{left.sum()} cells still hold the fill pattern, first at (d, jj) = {np.argwhere(left)[0]}"
    for rows in (band.data[:d0], band.data[d1 + 1:]):
        assert (rows == -np.inf).all(), f"{(rows != -np.inf).sum()} cells of rows without DP cells are not -Inf"


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,bw,mc", [c + (mc,) for c in CASE_LIST for mc in (1, 0)])
def test_wide_thin_bands_bitexact(engine, opts, m, n, bw, mc):
    """Forward and backward bands of one call, A[end,end], the kernel family
    that ran, the backtrace of the forward band (k_bt_win along a band whose
    path hugs one edge) and its error count, against the oracle.

    rf_download_band writes no cell itself: it copies every (d, jj), 0 <= d <
    H, 0 <= jj <= m, from the device band, so a cell k_dpm left at the host's
    fill pattern arrives as such.  Both wide kernels store -Inf in every such
    cell outside the DP (k_dp for d <= kappa, which is every downloaded cell);
    the cells outside inband_mask are therefore looked at too."""
    opts("dp_mc", mc)
    t, s, A_exp, B_exp, moves_exp, nerr_exp = reference(m, n, bw)
    engine.set_sequences(0, [s])
    engine.set_templates(0, [t])
    score = engine.realign([0], [0], 0, [bw], RF_FWD | RF_BWD)
    c, H, _, _, _, _ = geometry(m, n, bw)
    assert launched_tasks(engine) == {(expected_family(H, mc), 0): 2}
    A = engine.download_band(0, RF_BAND_A)
    B = engine.download_band(0, RF_BAND_B)
    assert_band_equal(A, A_exp, n + 1, m + 1, bw)
    assert_band_equal(B, B_exp, n + 1, m + 1, bw)
    assert score[0] == A_exp[n - m + c, m]
    assert_no_fill_pattern(A, m, n, bw)
    assert_no_fill_pattern(B, m, n, bw)
    moves, nerr = engine.backtrace([0])
    np.testing.assert_array_equal(moves[0], moves_exp)
    assert nerr[0] == nerr_exp


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,bw,flags,mc", [c + (f, mc) for c in FLAG_CASES for f in (RF_SKEW, RF_TRIM, RF_SKEW | RF_TRIM)
                                             for mc in (1, 0)])
def test_wide_thin_bands_skew_trim(engine, opts, m, n, bw, flags, mc):
    """Forward alone with skew_matches and trim (k_dpm<true>; with m = 1 trim
    zeroes the insertion score in both columns): band, score and moves."""
    opts("dp_mc", mc)
    skew, trim = bool(flags & RF_SKEW), bool(flags & RF_TRIM)
    t, s, A_exp, _, moves_exp, nerr_exp = reference(m, n, bw, skew, trim, False)
    engine.set_sequences(0, [s])
    engine.set_templates(0, [t])
    score = engine.realign([0], [0], 0, [bw], RF_FWD | flags)
    c, H, _, _, _, _ = geometry(m, n, bw)
    assert launched_tasks(engine) == {(expected_family(H, mc), 0): 1}
    A = engine.download_band(0, RF_BAND_A)
    assert_band_equal(A, A_exp, n + 1, m + 1, bw)
    assert score[0] == A_exp[n - m + c, m]
    assert_no_fill_pattern(A, m, n, bw)
    moves, nerr = engine.backtrace([0])
    np.testing.assert_array_equal(moves[0], moves_exp)
    assert nerr[0] == nerr_exp


@pytest.mark.gpu
def test_wide_thin_bands_one_call(engine):
    """Four wide bands on one 30-base template -- thin stripes of 35, 39 and
    37 slices and a band of 4,131 rows with 30 of its 65 slices empty -- in
    one k_dpm launch, a 35-base read beside them."""
    rng = np.random.default_rng(30)
    t = random_seq(MIXED_M, rng)
    seqs = [RifrafSequence(random_seq(n, rng), np.log10(rng.uniform(0.01, 0.3, n)), bw, SEQ_SCORES) for n, bw in MIXED]
    _check_bands(engine, t, seqs, [bw for _, bw in MIXED])
    assert launched_tasks(engine)[("dpm", 0)] == 8
    for k, (n, bw) in enumerate(MIXED[:4]):
        for which in (RF_BAND_A, RF_BAND_B):
            assert_no_fill_pattern(engine.download_band(k, which), MIXED_M, n, bw)
