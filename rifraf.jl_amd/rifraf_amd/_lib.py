"""ctypes binding of librifraf_hip.so (the C-ABI in include/rifraf_hip.h).

This is the only way the host reaches the hot path: there is no CPU fallback.
If the shared library is missing, cannot be loaded, or no HIP device is
present, every engine entry point raises instead of computing anything.
"""
from __future__ import annotations

import ctypes
import os
from collections import namedtuple
from ctypes import POINTER, c_char_p, c_double, c_int, c_int8, c_int32, c_int64, c_uint8, c_void_p

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("RIFRAF_HIP_LIB", os.path.join(PKG_DIR, "librifraf_hip.so"))

RF_FWD, RF_BWD, RF_SKEW, RF_TRIM = 1, 2, 4, 8
RF_BAND_A, RF_BAND_B = 0, 1
RF_ERR_NEED_HOST = -5
RF_ABI_VERSION = 1

# every symbol include/rifraf_hip.h declares, with its ctypes signature
_SIGNATURES = {
    "rf_abi_version": (c_int, []),
    "rf_create": (c_int, [c_int, POINTER(c_void_p)]),
    "rf_destroy": (c_int, [c_void_p]),
    "rf_last_error": (c_char_p, [c_void_p]),
    "rf_reserve": (c_int, [c_void_p, c_int64]),
    "rf_release_bands": (c_int, [c_void_p]),
    "rf_device_bytes": (c_int64, [c_void_p]),
    "rf_set_sequences_codes": (c_int, [c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_double, c_double, c_double]),
    "rf_set_sequences_codes_prep": (c_int, [c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_void_p, c_double, c_double, c_double] + [c_void_p] * 5),
    "rf_code_stats": (c_int, [c_void_p, POINTER(c_int64), POINTER(c_int64), POINTER(c_int64), POINTER(c_int64)]),
    "rf_set_sequences": (c_int, [c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rf_set_templates": (c_int, [c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "rf_set_templates_ids": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "rf_rifraf_batch": (c_int, [c_void_p, c_int32, c_void_p] + [c_void_p] * 14),
    "rf_batch_fetch": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64]),
    "rf_rifraf_batch_ref": (c_int, [c_void_p, c_int32] + [c_void_p] * 21),
    "rf_batch_fetch_ref": (c_int, [c_void_p, c_int32] + [c_void_p] * 6),
    "rf_batch_release": (None, [c_void_p]),
    "rf_aln_error_sums": (c_int, [c_void_p, c_int32] + [c_void_p] * 7),
    "rf_qv_probs": (c_int, [c_void_p, c_int32] + [c_void_p] * 8),
    "rf_host_julia_sums": (c_int, [c_int64, c_void_p, c_void_p, c_void_p]),
    "rf_host_seq_sums": (c_int, [c_int64, c_void_p, c_void_p, c_void_p]),
    "rf_host_tables_from_codes": (c_int, [c_int64] + [c_void_p] * 5 + [c_double] * 3 + [c_void_p] * 6),
    "rf_host_code_seq_sums": (c_int, [c_int64] + [c_void_p] * 5),
    "rf_host_code_prep": (c_int, [c_int64] + [c_void_p] * 8),
    "rf_host_lse_finish": (c_int, [c_int64] + [c_void_p] * 4),
    "rf_host_qv_prep": (c_int, [c_int64] + [c_void_p] * 8),
    "rf_host_qv_finish": (c_int, [c_int64] + [c_void_p] * 6),
    "rf_realign": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p]),
    "rf_realign_jobs": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rf_pair_scores": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int32, c_void_p]),
    "rf_last_pair_ms": (c_int, [c_void_p, POINTER(c_double)]),
    "rf_pair_align": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p,
                              c_void_p, c_void_p, c_void_p]),
    "rf_last_pair_align_ms": (c_int, [c_void_p, POINTER(c_double), POINTER(c_double)]),
    "rf_pair_align_smart": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32,
                                    c_int32] + [c_void_p] * 7),
    "rf_pair_align_text": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32,
                                   c_int32] + [c_void_p] * 12),
    "rf_last_pair_text_ms": (c_int, [c_void_p, POINTER(c_double)]),
    "rf_pair_errors": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32,
                               c_int32] + [c_void_p] * 4),
    "rf_last_pair_errors_ms": (c_int, [c_void_p, POINTER(c_double)]),
    "rf_pair_shifts": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int32] + [c_void_p] * 10),
    "rf_last_pair_shifts_ms": (c_int, [c_void_p, POINTER(c_double)]),
    "rf_host_shift_fix": (c_int, [c_int64] + [c_void_p] * 16),
    "rf_backtrace": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rf_score": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                         c_void_p, c_void_p, c_void_p]),
    "rf_alignment_proposals": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p]),
    "rf_score_dense": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "rf_score_dense_dev": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "rf_score_dense_ref": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rf_score_dense_from": (c_int, [c_void_p, c_int32] + [c_void_p] * 5),
    "rf_score_dense_from_dev": (c_int, [c_void_p, c_int32] + [c_void_p] * 5),
    "rf_host_band_bytes": (c_int64, [c_int32, c_int32, c_int32, c_int32]),
    "rf_host_reserve_fit": (c_int64, [c_int64]),
    "rf_band_arena_bytes": (c_int64, [c_void_p]),
    "rf_slot_geometry": (c_int, [c_void_p, c_int32, c_int32, POINTER(c_int32), POINTER(c_int32),
                                 POINTER(c_int32), POINTER(c_int32)]),
    "rf_download_band": (c_int, [c_void_p, c_int32, c_int32, c_void_p]),
    "rf_last_timing": (c_int, [c_void_p, POINTER(c_double), POINTER(c_double), POINTER(c_double)]),
    "rf_last_backtrace_ms": (c_int, [c_void_p, POINTER(c_double)]),
    "rf_last_codon_ms": (c_int, [c_void_p, POINTER(c_double)]),
    "rf_last_codon_dense_ms": (c_int, [c_void_p, POINTER(c_double)]),
    "rf_host_dp_plan": (c_int, [c_int32] + [c_void_p] * 9 + [c_int32] + [c_void_p] * 6 + [POINTER(c_int32), c_int32,
                                c_void_p, POINTER(c_int32)]),
    "rf_last_dp_launches": (c_int, [c_void_p, c_int32, c_void_p, POINTER(c_int32)]),
    "rf_region_offsets": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "rf_host_score_plan": (c_int, [c_int32] + [c_void_p] * 5 + [c_int32, c_void_p, c_int32, c_void_p, c_void_p,
                                   c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p, POINTER(c_int32),
                                   c_void_p, c_void_p]),
    "rf_host_score_chunks": (c_int, [c_int32] * 6 + [POINTER(c_int32), POINTER(c_int32)]),
    "rf_host_pair_wide_plan": (c_int, [c_int64, c_void_p, c_int32, c_int64] + [POINTER(c_int64)] * 3),
    "rf_last_score_launch": (c_int, [c_void_p, c_void_p]),
    "rf_host_row_codes": (c_int, [c_int32] + [c_void_p] * 6 + [c_int32, c_void_p, c_void_p, c_int32] + [c_void_p] * 6),
    "rf_host_upload_chunks": (c_int, [c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int64, c_void_p,
                                      POINTER(c_int32)]),
    "rf_candidates": (c_int, [c_void_p, c_int32] + [c_void_p] * 6 + [c_int32] + [c_void_p] * 12),
    "rf_candidates_table": (c_int, [c_void_p, c_int32] + [c_void_p] * 7 + [c_int32] + [c_void_p] * 12),
    "rf_host_candidates": (c_int, [c_int32] + [c_void_p] * 7 + [c_int32] + [c_void_p] * 12),
    "rf_last_candidates_ms": (c_int, [c_void_p, POINTER(c_double), POINTER(c_double)]),
    "rf_set_option": (c_int, [c_void_p, c_int32, c_int32]),
    "rf_get_option": (c_int, [c_void_p, c_int32, POINTER(c_int32)]),
}

# rf_set_option keys (include/rifraf_hip.h RF_OPT_*)
OPTIONS = {"score_mode": 1, "score_kernel": 2, "lean_lds_kb": 4, "dp_psplit": 10,
           "dp_np8": 11, "dp_np8_lean": 12, "dp_streams": 13, "bt_win_kb": 15, "stage_kb": 16,
           "band_pad": 17, "dp_wide": 18, "aln_sums_host": 19,
           "aln_marks_min": 22, "sync_block": 23, "dp_nl64": 24, "dp_lat": 26,
           "score_wgs": 27, "seg_wgs": 28, "dp_pfit": 29, "dp_mc": 30, "bt_nw": 31, "pair_chunk": 32,
           "pair_trace_mb": 33, "pair_walk": 34, "cand_device": 35, "pair_wide": 36, "pair_ring_mb": 37}
# symbolic values of the enum-like options
OPTION_VALUES = {"score_mode": {"auto": 0, "fused": 1, "split": 2},
                 "score_kernel": {"auto": 0, "general": 1, "seg": 2, "ws": 3},
                 "pair_walk": {"auto": 0, "lane": 1, "wave": 2}}

# kernel families of the DP launches (include/rifraf_hip.h RF_DPK_*, by value)
DP_KERNELS = ("dpr", "dpr_lean", "dpr_lean_pm", "dpr_wide64", "dpr_wide32", "dpx_codon", "dpx_lean", "dp64",
              "dpw_lds", "dpw_global", "dpm")
# one launch record (RF_DPL_FIELDS int32): kernel is a DP_KERNELS name, stream -1 the context's stream
DpLaunch = namedtuple("DpLaunch", "kernel npi pmi first count stream grid block lds")
DP_LAUNCH_CAP = 64   # more than the planner's classes


def dp_launch_records(buf, n):
    return [DpLaunch(DP_KERNELS[int(r[0])], *(int(x) for x in r[1:])) for r in buf[:n]]


# kernel families of the scorers (include/rifraf_hip.h RF_SCK_*, by value: the score_kernel option's names)
SCORE_KERNELS = (None, "general", "seg", "ws")
# the scorer launch of a scoring call (RF_SCL_FIELDS int32)
ScoreLaunch = namedtuple("ScoreLaunch", "kernel split items grid_y")
# rf_host_score_plan's outputs: split_score is rf_score's split mode, split_dense the dense calls';
# items are (group, first column) pairs; dense_off has one more entry than groups, the total
ScorePlan = namedtuple("ScorePlan", "kernel lds cols split_score split_dense items dense_off split_off")


class BatchParams(ctypes.Structure):
    """rf_batch_params (include/rifraf_hip.h)."""
    _fields_ = [("max_iters", c_int32), ("min_dist", c_int32), ("bandwidth", c_int32),
                ("do_alignment_proposals", c_int32), ("batch_fixed", c_int32), ("batch_size", c_int32),
                ("batch_threshold", c_double), ("batch_randomness", c_double), ("batch_mult", c_double),
                ("est_n_errors", c_void_p), ("seed", c_void_p)]


class BatchRefParams(ctypes.Structure):
    """rf_batch_ref_params (include/rifraf_hip.h)."""
    _fields_ = [("do_frame", c_int32), ("do_refine", c_int32), ("seed_indels", c_int32),
                ("indel_correction_only", c_int32), ("max_ref_indel_mults", c_int32), ("pad", c_int32),
                ("ref_error_mult", c_double)]


class BatchRef(ctypes.Structure):
    """rf_batch_ref (include/rifraf_hip.h): one cluster's reference record."""
    _fields_ = [("ref_seq", c_int32), ("edit_seq", c_int32), ("ref_slot", c_int32), ("scratch_slot", c_int32),
                ("ref_off", c_int64), ("ref_len", c_int64)]


# rf_ref_callback: (user, cluster, event, value, thr*) -> 0 / nonzero
RefCallback = ctypes.CFUNCTYPE(c_int, c_void_p, c_int32, c_int32, c_double, POINTER(c_double))


_lib = None
_load_error = None


class EngineUnavailable(RuntimeError):
    """The HIP engine cannot run here (library missing or no GPU)."""


def load(path: str | None = None):
    """Load librifraf_hip.so and bind every C-ABI symbol (raises if absent)."""
    global _lib, _load_error
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise EngineUnavailable(
            f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
    try:
        lib = ctypes.CDLL(p)
    except OSError as e:  # pragma: no cover - environment dependent
        _load_error = e
        raise EngineUnavailable(f"cannot load {p}: {e}") from e
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError = missing export: loud
        fn.restype = res
        fn.argtypes = args
    if lib.rf_abi_version() != RF_ABI_VERSION:
        raise EngineUnavailable("librifraf_hip.so ABI version mismatch")
    if path is None:
        _lib = lib
    return lib


def host_dp_plan(n, m, bw, flags, ncins=None, ncdel=None, finite=None, stride_a=None, stride_b=None, **opts):
    """rf_host_dp_plan: rf_realign's launch planner for the jobs (n[k], m[k],
    bw[k], flags[k]) on the host alone (no context, no GPU).  ncins / ncdel
    default to 0 and finite to True (lean reads); stride_a / stride_b to the
    unpadded stride; opts are OPTIONS names (dp_lat=0, ...).  Returns (job,
    direction, launch index, score slot) per task in device order and the
    DpLaunch records in issue order."""
    nj = len(n)
    i32 = lambda a, fill: np.ascontiguousarray(np.full(nj, fill) if a is None else a, np.int32)
    flags = np.full(nj, flags) if np.isscalar(flags) else flags
    arrs = [i32(n, 0), i32(m, 0), i32(bw, 0), i32(flags, 0), i32(ncins, 0), i32(ncdel, 0),
            np.ascontiguousarray(np.ones(nj) if finite is None else finite, np.uint8),
            None if stride_a is None else i32(stride_a, 0), None if stride_b is None else i32(stride_b, 0)]
    keys = np.array([OPTIONS[k] for k in opts], np.int32)
    vals = np.array([opts[k] for k in opts], np.int32)
    out = [np.zeros(max(2 * nj, 1), np.int32) for _ in range(4)]
    rec = np.zeros((DP_LAUNCH_CAP, len(DpLaunch._fields)), np.int32)
    nt, nl = c_int32(), c_int32()
    rc = load().rf_host_dp_plan(nj, *(ptr(a) for a in arrs), len(keys), ptr(keys), ptr(vals),
                                *(ptr(a) for a in out), ctypes.byref(nt), DP_LAUNCH_CAP, ptr(rec), ctypes.byref(nl))
    if rc != 0:
        raise ValueError(f"rf_host_dp_plan: bad arguments ({rc})")
    return (*(a[:nt.value] for a in out), dp_launch_records(rec, nl.value))


def host_score_plan(n, m, bw, read_off, stride=None, finite=None, per_seq=False, empty_ok=True, **opts):
    """rf_host_score_plan: the scoring planner for reads (n[r], m[r], bw[r])
    in groups [read_off[g], read_off[g + 1]) on the host alone (no context, no
    GPU).  finite defaults to True, stride to the unpadded stride; opts are
    score_mode, score_kernel and lean_lds_kb by value.  Returns a ScorePlan."""
    nr, ng = len(n), len(read_off) - 1
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    fin = np.ascontiguousarray(np.ones(nr) if finite is None else finite, np.uint8)
    keys = np.array([OPTIONS[k] for k in opts], np.int32)
    vals = np.array([opts[k] for k in opts], np.int32)
    cap = int(sum(int(x) // 64 + 1 for x in m)) + 1   # no group has more items than its reads' 64-column chunks
    pick, split, items = np.zeros(3, np.int32), np.zeros(2, np.int32), np.zeros((cap, 2), np.int32)
    dense_off, split_off, ni = np.zeros(ng + 1, np.int64), np.zeros(max(ng, 1), np.int64), c_int32()
    rc = load().rf_host_score_plan(nr, ptr(i32(n)), ptr(i32(m)), ptr(i32(bw)), None if stride is None else ptr(i32(stride)),
                                   ptr(fin), ng, ptr(i32(read_off)), len(keys), ptr(keys), ptr(vals), int(per_seq),
                                   int(empty_ok), ptr(pick), ptr(split), cap, ptr(items), ctypes.byref(ni),
                                   ptr(dense_off), ptr(split_off))
    if rc != 0:
        raise ValueError(f"rf_host_score_plan: bad arguments ({rc})")
    return ScorePlan(SCORE_KERNELS[pick[0]], int(pick[1]), int(pick[2]), bool(split[0]), bool(split[1]),
                     [tuple(int(x) for x in it) for it in items[:ni.value]], dense_off.tolist(), split_off[:ng].tolist())


def host_band_bytes(n, m, bw, pad=False):
    """rf_host_band_bytes: the bytes one slot's A band plus B band take in the
    band arena for a read of n bases against a template of m at bandwidth bw,
    on the host alone (no context, no GPU).  pad: whether the realign call
    that fills them pads its bands (its widest band has H >= the band_pad
    option)."""
    v = int(load().rf_host_band_bytes(int(n), int(m), int(bw), int(bool(pad))))
    if v < 0:
        raise ValueError("rf_host_band_bytes: bad arguments")
    return v


def host_reserve_fit(budget):
    """rf_host_reserve_fit: the largest band_bytes for which rf_reserve on an
    engine with an empty band arena allocates at most `budget` bytes (no
    context, no GPU).  Raises ValueError for a budget below the smallest
    arena (2 MiB)."""
    v = int(load().rf_host_reserve_fit(int(budget)))
    if v < 0:
        raise ValueError("rf_host_reserve_fit: the budget is below the smallest band arena")
    return v


def host_score_chunks(kernel, split, nitems, max_reads, score_wgs=2048, seg_wgs=262144):
    """rf_host_score_chunks: (rchunk, grid_y) of a scorer launch of family
    `kernel` (a SCORE_KERNELS name) over nitems items of groups of at most
    max_reads reads, on the host alone (no context, no GPU); the options
    default as the engine's."""
    rchunk, grid_y = c_int32(), c_int32()
    rc = load().rf_host_score_chunks(SCORE_KERNELS.index(kernel), int(bool(split)), int(nitems), int(max_reads),
                                     int(score_wgs), int(seg_wgs), ctypes.byref(rchunk), ctypes.byref(grid_y))
    if rc != 0:
        raise ValueError(f"rf_host_score_chunks: bad arguments ({rc})")
    return rchunk.value, grid_y.value


PAIR_WIDE_MAX_H = 1 << 24   # RF_PAIR_WIDE_MAX_H: the widest band of the pair calls' wide tier
PAIR_WIDE_MODES = ("score", "trace", "count")   # rf_host_pair_wide_plan's modes, by value
PairWidePlan = namedtuple("PairWidePlan", "nwg ring_ld ring_bytes")


def host_pair_wide_plan(H, mode, budget):
    """rf_host_pair_wide_plan: the workgroups, the ring's row length and its
    bytes for a launch set's wide pairs of H[k] band rows in fill mode `mode`
    (a PAIR_WIDE_MODES name) within `budget` bytes of ring, on the host alone
    (no context, no GPU).  Python ints from the call's int64."""
    H = np.ascontiguousarray(H, np.int32)
    out = [c_int64(), c_int64(), c_int64()]
    rc = load().rf_host_pair_wide_plan(len(H), ptr(H), PAIR_WIDE_MODES.index(mode), int(budget),
                                       *(ctypes.byref(o) for o in out))
    if rc != 0:
        raise ValueError(f"rf_host_pair_wide_plan: bad arguments ({rc})")
    return PairWidePlan(*(o.value for o in out))


RF_CODES = 65536   # entries of the row codes' dictionary, per kind
# rf_host_row_codes' outputs: val3 is (codes, 4) -- match, mismatch, ins, 0 -- and val1 one del value per code
RowCodes = namedtuple("RowCodes", "coded finite records val3 val1 uncoded_reads")


def host_row_codes(bases, off, match, mismatch, ins, dele, uploads=None, flags=None, nthreads=1):
    """rf_host_row_codes: the row codes of rf_set_sequences' tables on the host
    alone (no context, no GPU).  uploads: the boundaries of the uploads in the
    sequence list (default one upload of them all); flags per upload: 1 starts
    a fresh dictionary, 2 undoes the upload's dictionary entries after it.
    Returns a RowCodes."""
    off = np.ascontiguousarray(off, np.int64)
    nseq = len(off) - 1
    up = np.ascontiguousarray([0, nseq] if uploads is None else uploads, np.int32)
    fl = np.ascontiguousarray(np.zeros(len(up) - 1) if flags is None else flags, np.uint8)
    f64 = [np.ascontiguousarray(a, np.float64) for a in (match, mismatch, ins, dele)]
    bases = np.ascontiguousarray(bases, np.uint8)
    coded, finite = np.zeros(max(nseq, 1), np.uint8), np.zeros(max(nseq, 1), np.uint8)
    rec = np.zeros(max(int(off[-1] - off[0]), 1), np.uint64)
    val3, val1, sizes = np.zeros((RF_CODES, 4)), np.zeros(RF_CODES), np.zeros(3, np.int64)
    rc = load().rf_host_row_codes(nseq, ptr(bases), ptr(off), *(ptr(a) for a in f64), len(up) - 1, ptr(up), ptr(fl),
                                  int(nthreads), ptr(coded), ptr(finite), ptr(rec), ptr(val3), ptr(val1), ptr(sizes))
    if rc != 0:
        raise ValueError(f"rf_host_row_codes: bad arguments ({rc})")
    return RowCodes(coded[:nseq].astype(bool), finite[:nseq].astype(bool), rec[:int(off[-1] - off[0])],
                    val3[:sizes[0]].copy(), val1[:sizes[1]].copy(), int(sizes[2]))


def host_upload_chunks(off, codes, stage_kb=262144, budget=0, cins_off=None, cdel_off=None):
    """rf_host_upload_chunks: the ends of the staging chunks of one upload by
    rf_set_sequences (codes False) or rf_set_sequences_codes (True) at the
    stage_kb option, or within `budget` bytes when that is positive."""
    off = np.ascontiguousarray(off, np.int64)
    i64 = lambda a: None if a is None else np.ascontiguousarray(a, np.int64)   # noqa: E731
    end, nc = np.zeros(max(len(off) - 1, 1), np.int32), c_int32()
    rc = load().rf_host_upload_chunks(len(off) - 1, ptr(off), ptr(i64(cins_off)), ptr(i64(cdel_off)), int(bool(codes)),
                                      int(stage_kb), int(budget), ptr(end), ctypes.byref(nc))
    if rc != 0:
        raise ValueError(f"rf_host_upload_chunks: bad arguments ({rc})")
    return end[:nc.value].tolist()


# the `source` byte of the candidate calls (include/rifraf_hip.h rf_candidates)
CAND_SOURCES = {"all": 0, "alignment": 1, "alignment_subs": 2, "subs": 3, "mask": 4}


class CandidateIO:
    """The arguments that rf_candidates, rf_candidates_table and
    rf_host_candidates share -- scores, sources, min_dist and the twelve
    output arguments -- for groups of rows[g] = m_g + 1 table rows, and the
    outputs read back as ScoredProposal lists.  cand_cap / chosen_cap: None
    gives every group room for all its 9 rows[g] slots, a number or one per
    group that many records, False no record arrays at all (counts only)."""

    def __init__(self, rows, scores, sources, min_dist, cand_cap=None, chosen_cap=None):
        self.rows = [int(r) for r in rows]
        G = self.G = len(self.rows)
        self.scores = np.ascontiguousarray(scores, np.float64).reshape(-1)
        src = [CAND_SOURCES.get(s, s) for s in sources]
        self.sources = np.ascontiguousarray(src, np.uint8).reshape(-1)
        if len(self.scores) != G or len(self.sources) != G:
            raise ValueError("one score and one source per group")
        self.min_dist = int(min_dist)
        self.counts = [np.zeros(max(G, 1), np.int32) for _ in range(2)]
        self.recs = []
        for cap in (cand_cap, chosen_cap):
            if cap is False:
                self.recs.append(None)
                continue
            caps = [9 * r for r in self.rows] if cap is None else (
                [int(cap)] * G if np.isscalar(cap) else [int(c) for c in cap])
            off = np.zeros(G + 1, np.int64)
            if G:
                np.cumsum(caps, out=off[1:])
            n = max(int(off[-1]), 1)
            self.recs.append((off, np.full(n, 255, np.uint8), np.full(n, -1, np.int32), np.full(n, 255, np.uint8),
                              np.full(n, np.nan)))

    def args(self):
        """score, source, [mask goes between them and min_dist in rf_candidates: see callers]"""
        out = []
        for cnt, rec in zip(self.counts, self.recs):
            out.append(ptr(cnt))
            out += [None] * 5 if rec is None else [ptr(a) for a in rec]
        return out

    def results(self, with_counts=False):
        from .proposals import Proposal, ScoredProposal
        lists = []
        for cnt, rec in zip(self.counts, self.recs):
            per = []
            for g in range(self.G):
                if rec is None:
                    per.append(None)
                    continue
                off, kind, pos, base, sc = rec
                a, n = int(off[g]), min(int(cnt[g]), int(off[g + 1] - off[g]))
                per.append([ScoredProposal(Proposal(int(kind[i]), int(pos[i]), int(base[i])), float(sc[i]))
                            for i in range(a, a + n)])
            lists.append(per)
        if with_counts:
            return [(lists[0][g], lists[1][g], int(self.counts[0][g]), int(self.counts[1][g])) for g in range(self.G)]
        return [(lists[0][g], lists[1][g]) for g in range(self.G)]


def pack_candidate_tables(cons, tables, masks=None):
    """Per-group consensus arrays, (m + 1, 9) tables and optional (m + 1, 9)
    masks (None entries allowed) as rf_candidates_table's flat arguments:
    (m, cons, cons_off, table, mask or None, rows)."""
    m = np.ascontiguousarray([len(c) for c in cons], np.int32)
    cons_off = np.zeros(len(cons) + 1, np.int64)
    np.cumsum(m, out=cons_off[1:])
    flat = np.ascontiguousarray(np.concatenate([np.asarray(c, np.uint8) for c in cons]) if len(cons)
                                else np.zeros(0), np.uint8)
    if len(flat) == 0:
        flat = np.zeros(1, np.uint8)
    rows = [int(x) + 1 for x in m]
    tabs = [np.asarray(t, np.float64).reshape(-1, 9) for t in tables]
    if [len(t) for t in tabs] != rows:
        raise ValueError("a table has m + 1 rows of 9")
    table = np.ascontiguousarray(np.concatenate(tabs) if tabs else np.zeros((1, 9)))
    mask = None
    if masks is not None and any(k is not None for k in masks):
        mask = np.ascontiguousarray(np.concatenate(
            [np.zeros((r, 9), np.uint8) if k is None else np.asarray(k, np.uint8).reshape(r, 9)
             for k, r in zip(masks, rows)]))
    return m, flat, cons_off, table, mask, rows


def host_candidates(cons, tables, scores, sources, min_dist, masks=None, cand_cap=None, chosen_cap=None,
                    with_counts=False):
    """rf_host_candidates: candidate selection and choose_candidates over
    dense tables on the host alone (no context, no GPU).  cons / tables /
    masks: one consensus, (m + 1, 9) table and (for sources 1, 2, 4) mask per
    group; sources: 0..4 or CAND_SOURCES names.  Returns per group
    (candidates, chosen) as ScoredProposal lists -- with_counts: also the true
    counts.  NaN in a proposal slot raises ArithmeticError."""
    m, flat, cons_off, table, mask, rows = pack_candidate_tables(cons, tables, masks)
    io = CandidateIO(rows, scores, sources, min_dist, cand_cap, chosen_cap)
    rc = load().rf_host_candidates(io.G, ptr(m), ptr(flat), ptr(cons_off), ptr(table), ptr(mask), ptr(io.scores),
                                   ptr(io.sources), io.min_dist, *io.args())
    if rc == -3:
        raise ArithmeticError("failed to compute a valid score")
    if rc != 0:
        raise ValueError(f"rf_host_candidates: bad arguments ({rc})")
    return io.results(with_counts)


class PairShifts:
    """The outputs of rf_pair_shifts and rf_host_shift_fix over n pairs:
    fixed_len, nprops and tally ((n, 5): the moves of each code 1..5), the
    corrected templates' bytes `fixed` at fixed_off, and the proposal records
    prop_kind / prop_pos / prop_base at prop_off.  fixed_caps: n + m of each
    pair (None: no corrected templates); prop_caps: the records each pair has
    room for (None: no records).  A failed pair has fixed_len = nprops = -1
    and tallies of -1, an ambiguous one fixed_len = -2."""
    __slots__ = ("n", "fixed", "fixed_off", "fixed_len", "nprops", "prop_off", "prop_kind", "prop_pos", "prop_base",
                 "tally")

    def __init__(self, n, fixed_caps=None, prop_caps=None):
        self.n = n
        self.fixed_len = np.full(max(n, 1), -1, np.int32)[:n]
        self.nprops = np.full(max(n, 1), -1, np.int32)[:n]
        self.tally = np.full((max(n, 1), 5), -1, np.int32)[:n]
        self.fixed = self.fixed_off = self.prop_off = self.prop_kind = self.prop_pos = self.prop_base = None
        if fixed_caps is not None:
            self.fixed_off = self._offsets(fixed_caps)
            self.fixed = np.full(max(int(self.fixed_off[-1]), 1), 255, np.uint8)
        if prop_caps is not None:
            self.prop_off = self._offsets(prop_caps)
            k = max(int(self.prop_off[-1]), 1)
            self.prop_kind, self.prop_pos = np.full(k, 255, np.uint8), np.full(k, -1, np.int32)
            self.prop_base = np.full(k, 255, np.uint8)

    def _offsets(self, caps):
        off = np.zeros(self.n + 1, np.int64)
        np.cumsum(np.broadcast_to(np.asarray(caps, np.int64).reshape(-1), (self.n,)), out=off[1:])
        return off

    def args(self):
        """The nine output arguments from `fixed` on, in the order of the C calls."""
        return [ptr(a) for a in (self.fixed, self.fixed_off, self.fixed_len, self.nprops, self.prop_off,
                                 self.prop_kind, self.prop_pos, self.prop_base, self.tally)]

    def fixed_seq(self, k):
        """The corrected template of pair k (uint8 base codes); None for a failed or an ambiguous pair."""
        ln = int(self.fixed_len[k])
        if ln < 0:
            return None
        o = int(self.fixed_off[k])
        return self.fixed[o:o + ln].copy()

    def proposals(self, k):
        """The records of pair k as Insertion / Deletion proposals (the first
        `capacity` of them); None for a failed pair."""
        from .proposals import Proposal
        if self.nprops[k] < 0:
            return None
        a = int(self.prop_off[k])
        n = min(int(self.nprops[k]), int(self.prop_off[k + 1]) - a)
        return [Proposal(int(self.prop_kind[i]), int(self.prop_pos[i]), int(self.prop_base[i])) for i in range(a, a + n)]

    def has_single_indels(self):
        """has_single_indels (model.jl:532-536) per pair: an insert or a delete among its moves (failed pairs: False)."""
        return (self.tally[:, 1] + self.tally[:, 2]) > 0


def host_shift_fix(moves, seqs, tpls, want_fixed=True, want_proposals=True, prop_cap=None):
    """rf_host_shift_fix: rf_pair_shifts' products from given moves on the
    host alone (no context, no GPU).  moves: one int8 array per pair in
    alignment order, None for a failed pair; seqs / tpls: the pairs' base
    arrays (the sequence is the reference, the template the consensus).
    prop_cap: records per pair, a number or one per pair (None: n + m).
    Returns a PairShifts."""
    n = len(moves)
    seqs = [np.asarray(s, np.uint8) for s in seqs]
    tpls = [np.asarray(t, np.uint8) for t in tpls]
    if len(seqs) != n or len(tpls) != n:
        raise ValueError("host_shift_fix: one sequence and one template per move list")
    nm = np.array([len(s) + len(t) for s, t in zip(seqs, tpls)], np.int64)
    r = PairShifts(n, nm if want_fixed else None, (nm if prop_cap is None else prop_cap) if want_proposals else None)
    cat = lambda xs, t: np.ascontiguousarray(np.concatenate([np.asarray(x, t) for x in xs] + [np.zeros(1, t)]), t)   # noqa: E731
    off = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)   # noqa: E731
    mvs = [np.zeros(0, np.int8) if mv is None else mv for mv in moves]
    nmoves = np.ascontiguousarray([-1 if mv is None else len(mv) for mv in moves] + [0], np.int32)
    rc = load().rf_host_shift_fix(n, ptr(cat(mvs, np.int8)), ptr(off(mvs)), ptr(nmoves), ptr(cat(seqs, np.uint8)),
                                  ptr(off(seqs)), ptr(cat(tpls, np.uint8)), ptr(off(tpls)), *r.args())
    if rc != 0:
        raise ValueError(f"rf_host_shift_fix: bad arguments ({rc})")
    return r


def ptr(a: np.ndarray | None):
    """Pointer to a contiguous numpy array (None -> NULL)."""
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"], "array must be C-contiguous"
    return a.ctypes.data_as(c_void_p)


__all__ = ["load", "ptr", "EngineUnavailable", "RF_FWD", "RF_BWD", "RF_SKEW", "RF_TRIM",
           "RF_BAND_A", "RF_BAND_B", "RF_ERR_NEED_HOST", "_SIGNATURES", "c_int8", "c_uint8"]
