#!/usr/bin/env python3
"""Time rf_score_dense_ref (the reads' dense fold + k_codon_dense) against the
list path it replaces in the quality pass with use_ref_for_qvs: rf_score over
all 8m + 4 proposals with the reference slot (the same fold + k_codon +
k_gather), on one GPU.

Shapes:
  c3_qv   the cluster of tests/test_workloads.py's
          test_c3_qv_with_reference_matches_oracle: 40 reads x 2,601 and the
          reference, consensus and bandwidths as a rifraf() run with
          use_ref_for_qvs leaves them (the reference at its final bandwidth)
  ref_bw9 / ref_bw72 / ref_bw288
          the same cluster with only the reference's bandwidth changed.  The
          reads stay in the group (rf_score_dense takes no empty group); their
          fold is the same work on both paths, and the codon kernels' own
          times (rf_last_codon_ms, rf_last_codon_dense_ms) are reported beside
          the calls' kernel totals.

Each path has an engine of its own, so that the growth of rf_device_bytes
over its first call is that path's; score_dense has sized the shared buffers
on both before.  The two paths run alternately in this one process:
`--warmup` untimed rounds, then `--repeats` timed ones.  Kernel times are the
engine's HIP-event figures (rf_last_timing, rf_last_codon_ms,
rf_last_codon_dense_ms); wall times are host clocks around the calls.  Every
compared slot must have the same bits before anything is reported.  No ratio
is expected in advance: the file records what ran.

    timeout -k 10 900 python scripts/score_dense_ref_timing.py
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rifraf.jl_amd"))


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def c3_qv_cluster():
    """The finished run's consensus, reads and reference (final bandwidths)."""
    from rifraf_amd import ErrorModel, RifrafParams, rifraf
    from rifraf_amd.engine import Engine
    from rifraf_amd.sample import sample_sequences
    rng = np.random.default_rng(33)
    ref, _, _, reads, _, phreds, _, _ = sample_sequences(
        40, 2601, error_rate=0.01, ref_error_rate=0.1, ref_errors=ErrorModel(10, 0, 0, 1, 1), rng=rng)
    eng = Engine(0)
    try:
        res = rifraf(reads, phreds, reference=ref, params=RifrafParams(seed=1, do_score=True, use_ref_for_qvs=True),
                     engine=eng)
    finally:
        eng.close()
    st = res.state
    return np.asarray(st.consensus, np.uint8), [st.sequences[int(i)] for i in st.batch_seqs], st.reference


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    nan = np.isnan(a) | np.isnan(b)
    return np.where(nan, np.isnan(a) & np.isnan(b), a.view(np.int64) == b.view(np.int64))


def run_case(name, cons, reads, ref, ref_bw, warmup, repeats):
    from rifraf_amd.engine import RF_BWD, RF_FWD, Engine
    from rifraf_amd.model import score_proposal_arrays
    from rifraf_amd.proposals import DEL, SUB
    m, R = len(cons), len(reads)
    kind, pos, base = score_proposal_arrays(m, cons)
    slot = np.where(kind == SUB, base, np.where(kind == DEL, 4, 5 + base)).astype(np.int64)
    p64 = pos.astype(np.int64)
    slots = np.arange(R, dtype=np.int32)
    engines = []
    for _ in range(2):
        e = Engine(0)
        e.set_sequences(0, list(reads) + [ref])
        e.set_templates(0, [cons])
        k = np.arange(R + 1)
        e.realign(k, k, 0, [s.bandwidth for s in reads] + [ref_bw], RF_FWD | RF_BWD)
        e.score_dense([slots])
        engines.append(e)
    el, ed = engines
    H = ed.geometry(R)[3]
    rec = {k: [] for k in ("list_kernel", "list_codon", "list_wall", "dense_kernel", "dense_codon", "dense_wall")}
    grow_list = grow_dense = None
    try:
        for it in range(warmup + repeats):
            b0 = el.device_bytes()
            t0 = time.perf_counter()
            tot = el.score([(slots, R, (kind, pos, base))])[0]
            w_list = time.perf_counter() - t0
            _, sc, ga = el.last_timing()
            cm = el.last_codon_ms()
            if grow_list is None:
                grow_list = el.device_bytes() - b0
            b0 = ed.device_bytes()
            t0 = time.perf_counter()
            dense = ed.score_dense_ref([slots], [R])[0]
            w_dense = time.perf_counter() - t0
            dsc = ed.last_timing()[1]
            dcm = ed.last_codon_dense_ms()
            if grow_dense is None:
                grow_dense = ed.device_bytes() - b0
            if not same_bits(dense[p64, slot], tot).all():
                raise SystemExit(f"{name}: rf_score_dense_ref and rf_score differ in "
                                 f"{int((~same_bits(dense[p64, slot], tot)).sum())} of {len(tot)} slots")
            if it >= warmup:
                for key, v in zip(rec, (sc + ga, cm, 1e3 * w_list, dsc, dcm, 1e3 * w_dense)):
                    rec[key].append(v)
    finally:
        for e in engines:
            e.close()
    out = {"case": name, "reads": R, "consensus_len": m, "reference_len": len(ref), "reference_bandwidth": int(ref_bw),
           "reference_band_rows": int(H), "proposals": int(len(kind)), "slots_identical": True,
           "warmup": warmup, "repeats": repeats,
           "list_kernel_ms": stats(rec["list_kernel"]), "list_codon_ms": stats(rec["list_codon"]),
           "list_wall_ms": stats(rec["list_wall"]),
           "dense_ref_kernel_ms": stats(rec["dense_kernel"]), "dense_ref_codon_ms": stats(rec["dense_codon"]),
           "dense_ref_wall_ms": stats(rec["dense_wall"]),
           "list_device_bytes_growth": int(grow_list), "dense_ref_device_bytes_growth": int(grow_dense),
           "list_newcols_scratch_bytes": int(32 * (len(ref) + 1) * len(kind))}
    out["codon_kernel_ratio_list_over_dense"] = out["list_codon_ms"]["median"] / out["dense_ref_codon_ms"]["median"]
    out["kernel_ratio_list_over_dense"] = out["list_kernel_ms"]["median"] / out["dense_ref_kernel_ms"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bandwidths", type=int, nargs="*", default=[9, 72, 288])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "score_dense_ref_timing.json"))
    args = ap.parse_args()
    cons, reads, ref = c3_qv_cluster()
    cases = [("c3_qv", ref.bandwidth)] + [(f"ref_bw{bw}", bw) for bw in args.bandwidths]
    results = []
    for name, bw in cases:
        r = run_case(name, cons, reads, ref, bw, args.warmup, args.repeats)
        print(json.dumps(r), flush=True)
        results.append(r)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"script": "scripts/score_dense_ref_timing.py", "device": "MI355X (gfx950)", "cases": results}, f,
                  indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
