"""rf_realign's DP launch planner on the host (rf_host_dp_plan, no GPU): which
kernel family each (job, direction) takes, in which order, on which stream.

Every kernel family computes the same bits, so no result can show a routing
slip; these tests pin the routing itself.  Each expectation is worked out
from the rules of DESIGN.md §4 "DP launch planner", for a few jobs.

A job is given by its band height H = 2 bw + |n - m| + 1 (of the (n + 1) x
(m + 1) matrix): n = m and bw = (H - 1) / 2 for odd H, n = m + 1 and bw =
(H - 2) / 2 for even H.  The unpadded row stride is P = ceil(H / 2) | 1.
"""
import numpy as np
import pytest

from rifraf_amd import _lib
from rifraf_amd._lib import RF_BWD, RF_FWD, RF_SKEW, RF_TRIM

CODON, INF = "codon", "inf"   # what makes a read non-lean, beside skew / trim
# (block size, tasks per block) of each kernel family
SHAPE = {"dpr": (64, 4), "dpr_lean": (64, 4), "dpr_lean_pm": (64, 4), "dpr_wide64": (64, 1), "dpr_wide32": (64, 2),
         "dpx_codon": (128, 1), "dpx_lean": (128, 1), "dp64": (64, 1), "dpw_lds": (1024, 1), "dpw_global": (1024, 1)}
THROUGHPUT = dict(dp_lat=0, dp_nl64=0)   # neither latency class: the throughput classes show


def job(H, m=50, kind=None, flags=RF_FWD, stride=None):
    return dict(H=H, m=m, kind=kind, flags=flags, stride=stride)


def plan(jobs, **opts):
    """[(job, dir, launch record)] in device order and the launch records in
    issue order; checks what holds for every plan."""
    H = np.array([j["H"] for j in jobs])
    m = np.array([j["m"] for j in jobs])
    n = m + (H + 1) % 2
    bw = (H - 1 - (H + 1) % 2) // 2
    assert (2 * bw + np.abs(n - m) + 1 == H).all() and (bw >= 1).all()
    nci = np.array([j["m"] + 2 if j["kind"] == CODON else 0 for j in jobs])
    fin = np.array([j["kind"] != INF for j in jobs])
    stride = None
    if any(j["stride"] for j in jobs):
        stride = np.array([j["stride"] or (((j["H"] + 1) >> 1) | 1) for j in jobs])
    tj, td, tl, to, launches = _lib.host_dp_plan(n, m, bw, np.array([j["flags"] for j in jobs]), ncins=nci,
                                             finite=fin, stride_a=stride, stride_b=stride, **opts)
    nfill = sum(bool(j["flags"] & RF_FWD) + bool(j["flags"] & RF_BWD) for j in jobs)
    assert len(tj) == len(td) == len(tl) == len(to) == nfill
    # the score slot: the job's own, but njobs + job for a backward fill beside a forward one
    for k, d, slot in zip(tj.tolist(), td.tolist(), to.tolist()):
        assert slot == (len(jobs) + k if d == 1 and jobs[k]["flags"] & RF_FWD else k), (k, d, slot)
    # every (job, direction) once
    assert sorted(zip(tj.tolist(), td.tolist())) == sorted(
        (k, d) for k, j in enumerate(jobs) for d, f in ((0, RF_FWD), (1, RF_BWD)) if j["flags"] & f)
    # the launches tile the task list without gap or overlap
    spans = sorted((L.first, L.count) for L in launches)
    at = 0
    for first, count in spans:
        assert first == at and count > 0
        at += count
    assert at == nfill
    for i, L in enumerate(launches):
        assert (tl[L.first:L.first + L.count] == i).all()
        assert 0 <= L.lds <= 160 * 1024 and -1 <= L.stream <= 2
        Hs = [jobs[k]["H"] for k in tj[L.first:L.first + L.count]]
        if L.kernel == "dpm":
            gm = max(((h + 1) // 2 + 31) // 32 for h in Hs)    # slices of 32 row pairs
            chunk = min(L.count, 8 * max(1, 64 // gm))         # at most 64 slices per XCD and launch
            assert (L.grid, L.block, L.lds) == (8 * ((chunk + 7) // 8) * gm, 64, 0)
        else:
            block, per = SHAPE[L.kernel]
            assert L.block == block and L.grid * per >= L.count > (L.grid - 1) * per
        if L.kernel in ("dp64", "dpw_lds"):
            assert L.lds == 4 * (max(Hs) + 6) * 8              # the ring: four anti-diagonals
        if L.kernel in ("dpr", "dpx_codon", "dpx_lean", "dpw_global"):
            assert L.lds == 0
    plan.slots = to.tolist()
    return [(int(k), int(d), launches[i]) for k, d, i in zip(tj, td, tl)], launches


def route(H, kind=None, flags=RF_FWD, m=50, stride=None, **opts):
    """(kernel, npi, pmi) of one job alone."""
    tasks, launches = plan([job(H, m, kind, flags, stride)], **opts)
    assert len(launches) == 1 and launches[0].stream == -1
    L = tasks[0][2]
    return L.kernel, L.npi, L.pmi


def kernels(tasks):
    return [(k, L.kernel) for k, _, L in tasks]


# lean, throughput classes, defaults otherwise.  P = ceil(H/2)|1; the stride
# classes hold P <= 11, 13, 15, 17 (NP 1), 19, 23, 27, 33 (NP 2), 41, 49, 57,
# 65 (NP 4), 81, 97, 113, 129 (NP 8).  One task of H <= 31 is "at least half":
# NP = 1 splits by stride; a whole NP >= 2 class refits to its widest stride.
@pytest.mark.parametrize("H,exp", [
    (31, ("dpr_lean_pm", 0, 3)),     # P 17
    (32, ("dpr_lean_pm", 1, 0)),     # P 17 <= 19
    (63, ("dpr_lean_pm", 1, 3)),     # P 33
    (64, ("dpr_wide32", 0, 0)),
    (127, ("dpr_wide32", 0, 0)),
    (128, ("dpr_wide64", 0, 0)),
    (255, ("dpr_wide64", 0, 0)),
    (256, ("dp64", 0, 0)),
    (2040, ("dp64", 0, 0)),
    (2041, ("dpm", 0, 0)),
])
def test_h_edges_lean(H, exp):
    assert route(H, **THROUGHPUT) == exp


@pytest.mark.parametrize("H,exp", [
    (64, ("dpr_lean_pm", 2, 0)),     # P 33 <= 41
    (127, ("dpr_lean_pm", 2, 3)),    # P 65
    (128, ("dpr_lean_pm", 3, 0)),    # P 65 <= 81
    (255, ("dpr_lean_pm", 3, 3)),    # P 129
    (256, ("dp64", 0, 0)),
])
def test_h_edges_lean_16_lane(H, exp):
    """dp_wide 0: the 16-lane classes above H 63."""
    assert route(H, dp_wide=0, **THROUGHPUT) == exp
    if H <= 255:
        assert route(H, dp_wide=0, dp_pfit=0, **THROUGHPUT) == ("dpr_lean", exp[1], 0)


@pytest.mark.parametrize("kind", [CODON, INF, RF_SKEW, RF_TRIM])
@pytest.mark.parametrize("H,exp", [
    (31, ("dpr", 0, 0)), (32, ("dpr", 1, 0)), (63, ("dpr", 1, 0)), (64, ("dpr", 2, 0)), (127, ("dpr", 2, 0)),
    (128, ("dpr", 3, 0)), (255, ("dpr", 3, 0)), (256, ("dp64", 0, 0)), (2040, ("dp64", 0, 0)),
])
def test_h_edges_non_lean(H, exp, kind):
    """Codon tables, a -Inf table entry, skew and trim each make a task
    non-lean: the general k_dpr step up to H 255, k_dp<64> up to 2,040."""
    kw = dict(flags=RF_FWD | kind) if isinstance(kind, int) else dict(kind=kind)
    assert route(H, **kw, **THROUGHPUT) == exp
    # default dp_nl64: one such task of H <= 127 is latency-bound
    assert route(H, **kw, dp_lat=0) == (("dpx_codon", 0, 0) if H <= 127 else exp)


def test_h_2041_non_lean():
    """Above 2,040 rows only codon moves keep a band from k_dpm."""
    assert route(2041, kind=CODON)[0] == "dpw_lds"
    assert route(2041, kind=INF)[0] == "dpm"
    assert route(2041, flags=RF_FWD | RF_SKEW | RF_TRIM)[0] == "dpm"
    assert route(2041, flags=RF_BWD)[0] == "dpm"


def test_skew_trim_are_forward_only():
    tasks, _ = plan([job(21, flags=RF_FWD | RF_BWD | RF_SKEW)], **THROUGHPUT)
    assert [(d, L.kernel) for _, d, L in tasks] == [(0, "dpr"), (1, "dpr_lean_pm")]


def test_latency_mode_h_edge():
    """Default dp_lat: a lean task of H <= 127 alone runs in the lean k_dpx."""
    assert route(127) == ("dpx_lean", 0, 0)
    assert route(128) == ("dpr_wide64", 0, 0)
    tasks, _ = plan([job(127), job(128)])
    assert kernels(tasks) == [(1, "dpr_wide64"), (0, "dpx_lean")]


def test_dp_lat_count():
    """dp_lat counts the call's lean tasks of H <= 127, and only those."""
    three = [job(21), job(40), job(100, flags=RF_BWD)]
    tasks, launches = plan(three, dp_lat=3)
    assert [L.kernel for L in launches] == ["dpx_lean"] and launches[0].count == 3
    tasks, _ = plan(three + [job(21)], dp_lat=3)
    assert "dpx_lean" not in {L.kernel for _, _, L in tasks}
    # a lean task of H 128, a codon task and a skewed one are not counted
    tasks, _ = plan(three + [job(128), job(21, kind=CODON), job(21, flags=RF_FWD | RF_SKEW)], dp_lat=3, dp_nl64=0)
    assert kernels(tasks) == [(4, "dpr"), (5, "dpr"), (3, "dpr_wide64"), (2, "dpx_lean"), (1, "dpx_lean"),
                              (0, "dpx_lean")]
    # both directions of a job count
    tasks, _ = plan([job(21, flags=RF_FWD | RF_BWD), job(21, flags=RF_FWD | RF_BWD)], dp_lat=3)
    assert "dpx_lean" not in {L.kernel for _, _, L in tasks}


def test_dp_nl64_count():
    """dp_nl64 counts the non-lean tasks of H <= 127 (that no earlier class took)."""
    three = [job(21, kind=CODON), job(40, kind=INF), job(100, flags=RF_FWD | RF_TRIM)]
    tasks, launches = plan(three, dp_nl64=3, dp_lat=0)
    assert [L.kernel for L in launches] == ["dpx_codon"] and launches[0].count == 3
    tasks, _ = plan(three + [job(21, kind=CODON)], dp_nl64=3, dp_lat=0)
    assert kernels(tasks) == [(0, "dpr"), (3, "dpr"), (1, "dpr"), (2, "dpr")]
    # non-lean tasks of H >= 128 and lean tasks are not counted
    tasks, _ = plan(three + [job(128, kind=CODON), job(21)], dp_nl64=3, dp_lat=0)
    assert kernels(tasks) == [(4, "dpr_lean"), (3, "dpr"), (2, "dpx_codon"), (1, "dpx_codon"), (0, "dpx_codon")]


def test_psplit_auto_half():
    """dp_psplit -1: the NP = 1 class splits by stride only when tasks of H <=
    31 are at least half of the call's."""
    wide = [job(40), job(41)]
    tasks, _ = plan([job(21), job(25)] + wide, dp_lat=0)           # 2 of 4
    assert kernels(tasks)[:2] == [(0, "dpr_lean_pm"), (1, "dpr_lean_pm")]
    assert [(L.npi, L.pmi) for _, _, L in tasks[:2]] == [(0, 0), (0, 1)]   # P 11, P 13
    tasks, _ = plan([job(21)] + wide, dp_lat=0)                    # 1 of 3
    assert kernels(tasks) == [(0, "dpr_lean"), (2, "dpr_lean_pm"), (1, "dpr_lean_pm")]
    # non-lean tasks count on both sides of the rule
    tasks, _ = plan([job(21), job(25, kind=CODON)] + wide, **THROUGHPUT)
    assert (0, "dpr_lean_pm") in kernels(tasks)
    tasks, _ = plan([job(21), job(40, kind=CODON)] + wide, **THROUGHPUT)
    assert (0, "dpr_lean") in kernels(tasks)


@pytest.mark.parametrize("H,P,exp", [
    (21, 11, ("dpr_lean_pm", 0, 0)), (25, 13, ("dpr_lean_pm", 0, 1)), (29, 15, ("dpr_lean_pm", 0, 2)),
    (31, 17, ("dpr_lean_pm", 0, 3)),
    (17, 9, ("dpr_lean", 0, 0)),     # below the stride classes
    (21, 16, ("dpr_lean", 0, 0)),    # a padded (even) stride
    (21, 12, ("dpr_lean", 0, 0)),
    (31, 19, ("dpr_lean", 0, 0)),    # above them
])
def test_np1_exact_stride(H, P, exp):
    """The NP = 1 stride kernels have their stride compiled in: only P = 11,
    13, 15, 17 take them."""
    assert route(H, stride=P, **THROUGHPUT) == exp
    assert route(H, stride=P, dp_psplit=15, **THROUGHPUT) == exp


def test_pfit_whole_class():
    """dp_pfit: an NP = 2 class launched whole takes the stride class of its
    widest task (H 33: P 17, H 41: P 21 -> the class of P <= 23)."""
    two = [job(33), job(41)]
    tasks, launches = plan(two, dp_lat=0)
    assert [(L.kernel, L.npi, L.pmi, L.count) for L in launches] == [("dpr_lean_pm", 1, 1, 2)]
    tasks, launches = plan(two, dp_lat=0, dp_pfit=0)
    assert [(L.kernel, L.npi, L.pmi, L.count) for L in launches] == [("dpr_lean", 1, 0, 2)]
    # split by stride (dp_psplit bit 1), each task takes its own class
    tasks, launches = plan(two, dp_lat=0, dp_psplit=15, dp_streams=0)
    assert [(L.kernel, L.npi, L.pmi, L.count) for L in launches] == [("dpr_lean_pm", 1, 0, 1), ("dpr_lean_pm", 1, 1, 1)]
    # a padded stride counts as it is: P 32 -> the class of P <= 33
    assert route(33, stride=32, dp_lat=0) == ("dpr_lean_pm", 1, 3)


@pytest.mark.parametrize("wide,exp", [(0, ("dpr_lean_pm", "dpr_lean_pm")), (1, ("dpr_lean_pm", "dpr_wide64")),
                                      (2, ("dpr_wide32", "dpr_lean_pm")), (3, ("dpr_wide32", "dpr_wide64"))])
def test_dp_wide_bits(wide, exp):
    """Bit 0: H 128..255 as 64-lane tasks; bit 1: H 64..127 as 32-lane tasks."""
    assert route(100, dp_wide=wide, dp_lat=0)[0] == exp[0]
    assert route(200, dp_wide=wide, dp_lat=0)[0] == exp[1]
    assert route(63, dp_wide=wide, dp_lat=0)[0] == "dpr_lean_pm"
    assert route(256, dp_wide=wide, dp_lat=0)[0] == "dp64"


def test_dp_np8():
    """H 128..255 in 16 lanes: dp_np8 0 sends it to k_dp<64>; dp_np8_lean 0
    keeps k_dpr<8> to its general step."""
    lean = dict(dp_wide=0, dp_lat=0)
    assert route(200, **lean) == ("dpr_lean_pm", 3, 2)             # P 101: the class of P <= 113
    assert route(200, dp_pfit=0, **lean) == ("dpr_lean", 3, 0)
    assert route(200, dp_psplit=15, **lean) == ("dpr_lean_pm", 3, 2)
    assert route(200, dp_np8_lean=0, **lean) == ("dpr", 3, 0)
    assert route(200, dp_np8_lean=0, dp_psplit=15, **lean) == ("dpr", 3, 0)
    assert route(200, dp_np8=0, **lean) == ("dp64", 0, 0)
    assert route(200, dp_np8=0, dp_psplit=15, **lean) == ("dp64", 0, 0)
    assert route(200, kind=CODON) == ("dpr", 3, 0)
    assert route(200, kind=CODON, dp_np8=0) == ("dp64", 0, 0)
    assert route(127, kind=CODON, dp_np8=0, dp_nl64=0) == ("dpr", 2, 0)


def test_dp_mc_and_slices():
    """k_dpm takes H > 2,040 up to 160 slices of 32 row pairs; k_dp's ring is
    in LDS up to H = 160 KB / 32 B - 6 = 5,114."""
    assert route(2041, dp_mc=0)[0] == "dpw_lds"
    assert route(5114, dp_mc=0)[0] == "dpw_lds"
    assert route(5115, dp_mc=0)[0] == "dpw_global"
    assert route(5115)[0] == "dpm"
    assert route(10240)[0] == "dpm"            # 5,120 pairs: 160 slices
    assert route(10241)[0] == "dpw_global"     # 5,121 pairs: 161
    # one launch's ring place follows its widest band
    _, launches = plan([job(3001, kind=CODON), job(5115, kind=CODON)])
    assert [(L.kernel, L.count) for L in launches] == [("dpw_global", 2)]


def test_band_limit_2g():
    """k_dpm and k_dpx address a band with 32-bit offsets: K P 8 < 2^31, K = H + 2 m."""
    H, P = 2041, 1021
    m_fit = ((1 << 31) // (8 * P) - H) // 2
    assert (H + 2 * m_fit) * P * 8 < 1 << 31 <= (H + 2 * (m_fit + 1)) * P * 8
    assert route(H, m=m_fit)[0] == "dpm"
    assert route(H, m=m_fit + 1)[0] == "dpw_lds"
    H, P = 127, 65
    m_fit = ((1 << 31) // (8 * P) - H) // 2
    assert (H + 2 * m_fit) * P * 8 < 1 << 31 <= (H + 2 * (m_fit + 1)) * P * 8
    assert route(H, m=m_fit)[0] == "dpx_lean"
    assert route(H, m=m_fit + 1)[0] == "dpr_wide32"
    assert route(H, m=m_fit, kind=CODON)[0] == "dpx_codon"
    assert route(H, m=m_fit + 1, kind=CODON) == ("dpr", 2, 0)
    # latency mode still holds for the call's other tasks
    tasks, _ = plan([job(H, m=m_fit + 1), job(H)])
    assert kernels(tasks) == [(0, "dpr_wide32"), (1, "dpx_lean")]


def test_both_directions():
    """Forward fills come first.  Forward scores win out_score when both
    directions run: of three jobs, job 0's forward fill writes score slot 0
    and its backward fill slot 3 + 0; a backward-only and a forward-only job
    write their own slots."""
    jobs = [job(21, m=50, flags=RF_FWD | RF_BWD), job(21, m=50, flags=RF_BWD), job(21, m=50, flags=RF_FWD)]
    tasks, launches = plan(jobs, dp_lat=0)
    assert len(launches) == 1
    assert [(k, d) for k, d, _ in tasks] == [(0, 0), (2, 0), (0, 1), (1, 1)]
    assert plan.slots == [0, 2, 3, 1]
    # the same in separate classes: the skewed forward fill is not lean
    tasks, _ = plan([job(21, flags=RF_FWD | RF_BWD | RF_SKEW), job(300, flags=RF_FWD | RF_BWD)], **THROUGHPUT)
    assert [(k, d) for k, d, _ in tasks] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert plan.slots == [0, 2, 1, 3]


def test_longest_first():
    """Within a class the tasks are sorted by K = H + 2 m, longest first, ties
    in job order; k_dpm's class stays in job order."""
    jobs = [job(21, m=30), job(21, m=50), job(21, m=40), job(21, m=50)]
    tasks, _ = plan(jobs, dp_lat=0)
    assert [k for k, _, _ in tasks] == [1, 3, 2, 0]
    tasks, _ = plan(jobs)                                           # latency mode
    assert [k for k, _, _ in tasks] == [1, 3, 2, 0]
    tasks, _ = plan([job(300, m=300), job(300, m=500), job(2040, m=400)])
    assert kernels(tasks) == [(2, "dp64"), (1, "dp64"), (0, "dp64")]
    tasks, _ = plan([job(2041, m=3000), job(2041, m=5000), job(2041, m=4000)])
    assert kernels(tasks) == [(0, "dpm"), (1, "dpm"), (2, "dpm")]
    tasks, _ = plan([job(2041, m=3000), job(2041, m=5000), job(2041, m=4000)], dp_mc=0)
    assert kernels(tasks) == [(1, "dpw_lds"), (2, "dpw_lds"), (0, "dpw_lds")]


def test_device_order_of_classes():
    """k_dpr by NP (general, lean), the stride classes, 64- then 32-lane wide
    tasks, codon k_dpx, lean k_dpx, k_dp<64>, k_dp, k_dpm."""
    jobs = [job(2041), job(2041, kind=CODON), job(300), job(21, kind=CODON), job(100), job(200), job(21),
            job(40, stride=32), job(200, kind=CODON), job(21, stride=16)]
    tasks, _ = plan(jobs, dp_lat=0, dp_pfit=0, dp_psplit=1)
    assert kernels(tasks) == [(9, "dpr_lean"), (7, "dpr_lean"), (8, "dpr"), (6, "dpr_lean_pm"), (5, "dpr_wide64"),
                              (4, "dpr_wide32"), (3, "dpx_codon"), (2, "dp64"), (1, "dpw_lds"), (0, "dpm")]
    tasks, _ = plan([job(200), job(100), job(21)])
    assert kernels(tasks) == [(0, "dpr_wide64"), (1, "dpx_lean"), (2, "dpx_lean")]


def test_issue_order_and_streams():
    """Latency-bound launches (codon k_dpx, k_dp, k_dpm) are issued first and
    the first of them keeps the context's stream; else the largest launch
    does.  The others take side streams 0, 1, 2, 0, ..."""
    small = [job(21)] * 5 + [job(200)] * 2 + [job(100)] * 3
    _, launches = plan(small + [job(21, kind=CODON), job(300)], dp_lat=0)
    assert [(L.kernel, L.count, L.stream) for L in launches] == [
        ("dpx_codon", 1, -1), ("dp64", 1, 0), ("dpr_lean_pm", 5, 1), ("dpr_wide64", 2, 2), ("dpr_wide32", 3, 0)]
    _, launches = plan(small + [job(21, kind=CODON), job(40, kind=CODON)], **THROUGHPUT)
    assert [(L.kernel, L.npi, L.count, L.stream) for L in launches] == [
        ("dpr", 0, 1, 0), ("dpr", 1, 1, 1), ("dpr_lean_pm", 0, 5, -1), ("dpr_wide64", 0, 2, 2), ("dpr_wide32", 0, 3, 0)]
    # equal sizes: the first launch is "the largest"
    _, launches = plan([job(200), job(100)], dp_lat=0)
    assert [(L.kernel, L.stream) for L in launches] == [("dpr_wide64", -1), ("dpr_wide32", 0)]
    # k_dpm after k_dp<64> after k_dpx, all before the throughput classes
    _, launches = plan([job(21)] * 3 + [job(2041), job(300), job(2041, kind=CODON), job(21, kind=CODON)], dp_lat=0)
    assert [(L.kernel, L.stream) for L in launches] == [
        ("dpx_codon", -1), ("dp64", 0), ("dpw_lds", 1), ("dpm", 2), ("dpr_lean_pm", 0)]
    # the lean k_dpx is not one of them
    _, launches = plan([job(21)] * 3 + [job(200)] * 4)
    assert [(L.kernel, L.stream) for L in launches] == [("dpr_wide64", -1), ("dpx_lean", 0)]
    # dp_streams 0: one stream
    _, launches = plan(small + [job(21, kind=CODON), job(300)], dp_lat=0, dp_streams=0)
    assert [L.kernel for L in launches] == ["dpx_codon", "dp64", "dpr_lean_pm", "dpr_wide64", "dpr_wide32"]
    assert {L.stream for L in launches} == {-1}


def test_launch_geometry():
    """Grid, block and LDS of launches of more than one block."""
    _, (L,) = plan([job(21)] * 9, dp_lat=0)
    assert (L.kernel, L.grid, L.block) == ("dpr_lean_pm", 3, 64)
    _, (L,) = plan([job(100)] * 9, dp_lat=0)
    assert (L.kernel, L.grid, L.block) == ("dpr_wide32", 5, 64)
    _, (L,) = plan([job(200)] * 9, dp_lat=0)
    assert (L.kernel, L.grid, L.block) == ("dpr_wide64", 9, 64)
    _, (L,) = plan([job(21)] * 9)
    assert (L.kernel, L.grid, L.block, L.lds) == ("dpx_lean", 9, 128, 0)
    _, (L,) = plan([job(301), job(2040)])
    assert (L.kernel, L.grid, L.block, L.lds) == ("dp64", 2, 64, 4 * 2046 * 8)
    # k_dpm: 2,041 rows are 1,021 pairs = 32 slices; 16 bands per launch keep
    # an XCD to 64 slices, so 20 bands run as 16 + 4 and the first grid is
    # 16 bands x 32 slices
    _, (L,) = plan([job(2041)] * 20)
    assert (L.kernel, L.count, L.grid, L.block) == ("dpm", 20, 512, 64)
    _, (L,) = plan([job(2041)] * 3)
    assert (L.kernel, L.grid) == ("dpm", 8 * 32)                    # bands in eights, one per XCD


def test_empty_call_and_bad_arguments():
    tasks, launches = plan([])
    assert tasks == [] and launches == []
    with pytest.raises(ValueError):
        _lib.host_dp_plan([10], [10], [0], RF_FWD)                  # bandwidth must be positive
    with pytest.raises(ValueError):
        _lib.host_dp_plan([10], [10], [3], RF_SKEW)                 # no direction
    with pytest.raises(ValueError):
        _lib.host_dp_plan([10], [10], [3], RF_FWD, band_pad=1)      # not a planner option
    for bad in (dict(ncins=[-1]), dict(ncdel=[-1]), dict(stride_a=[0]), dict(stride_b=[-3]),
                dict(stride_a=[3]),       # H = 7: a row holds 4 pairs
                dict(stride_b=[21])):     # more than 16 above them
        with pytest.raises(ValueError):
            _lib.host_dp_plan([10], [10], [3], RF_FWD | RF_BWD, **bad)
    _lib.host_dp_plan([10], [10], [3], RF_FWD | RF_BWD, stride_a=[4], stride_b=[20])
    big = 1 << 29                                                   # K = H + 2 m past 2^30
    for n, m, bw in ((big, big, 3), (10, 10, big), (2 * big, 10, 3)):
        with pytest.raises(ValueError):
            _lib.host_dp_plan([n], [m], [bw], RF_FWD)
