#!/usr/bin/env python3
"""Time rf_pair_errors (the error count carried through the fill: no move
trace, no walk) against the path it replaces for callers that keep no moves,
rf_pair_align_smart without moves (trace fill + walk), on one GPU.

The two workloads of scripts/pair_align_timing.py that the README quotes:
  c4        62,500 pairs of the c4 read shape (1.5 kb, error rate 0.01) at
            bw 9, every read against its cluster's template, no doubling
  c5_smart  256 c5-shaped pairs (10 kb reads) doubling from bw 9 under the
            thresholds of pvalue 0.1

Per workload the two calls alternate in this one process on one engine:
`--warmup` untimed passes, then `--repeats` timed ones (at least five).  The
times are the engine's own HIP-event figures: rf_last_pair_align_ms (fill +
walk) for call A, rf_last_pair_errors_ms for call B.  Scores (bits), error
counts, bandwidths and rounds must be identical before anything is reported.
On c4 rf_pair_scores runs in the same passes as the floor: what the count
costs over the bare fill is reported, not judged.  rf_device_bytes growth is
taken on the first pass: call B runs first on the fresh engine, then call A
on top of it (the two share their descriptor and score buffers, so the sum
is what call A alone would have grown).

The direction is the only expectation: B's median kernel time below A's on
both workloads, and below A's fastest pass.  The file records what ran.

    timeout -k 10 900 python scripts/pair_errors_timing.py
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rifraf.jl_amd"))
sys.path.insert(0, os.path.join(REPO, "scripts"))

from pair_align_timing import stats, upload  # noqa: E402
from pair_scores_timing import make_clusters  # noqa: E402


def run(eng, name, clusters, seq, tpl, thr, max_doublings, warmup, repeats, floor):
    reads = upload(eng, clusters)
    npairs = len(seq)
    bws = np.full(npairs, 9, np.int32)
    lens = np.array([len(r) for r in reads])
    a_ms, a_fill, a_walk, b_ms, s_ms, a_wall, b_wall = [], [], [], [], [], [], []
    base = eng.device_bytes()
    grown = {}
    for it in range(warmup + repeats):
        t0 = time.perf_counter()
        b = eng.pair_errors(seq, tpl, bws, thr, max_doublings=max_doublings)
        tb = time.perf_counter() - t0
        kb = eng.last_pair_errors_ms()
        if it == 0:
            grown["pair_errors"] = eng.device_bytes() - base
        t0 = time.perf_counter()
        a = eng.pair_align_smart(seq, tpl, bws, thr, max_doublings=max_doublings, want_moves=False)
        ta = time.perf_counter() - t0
        f, w = eng.last_pair_align_ms()
        if it == 0:
            grown["pair_align_smart"] = eng.device_bytes() - base
        for x, y, what in zip(b, (a[0], a[2], a[3], a[4]), ("scores", "error counts", "bandwidths", "rounds")):
            if x.tobytes() != y.tobytes():
                raise SystemExit(f"{name}: {what} differ between rf_pair_errors and rf_pair_align_smart")
        if floor:
            sc = eng.pair_scores(seq, tpl, bws)
            ks = eng.last_pair_ms()
            if max_doublings == 0 and sc.tobytes() != b[0].tobytes():
                raise SystemExit(f"{name}: scores differ between rf_pair_errors and rf_pair_scores")
        if it >= warmup:
            a_ms.append(f + w)
            a_fill.append(f)
            a_walk.append(w)
            b_ms.append(kb)
            a_wall.append(ta * 1e3)
            b_wall.append(tb * 1e3)
            if floor:
                s_ms.append(ks)
    out = {"case": name, "pairs": npairs, "start_bandwidth": 9, "max_doublings": max_doublings,
           "read_len_mean": float(lens[seq].mean()), "rounds": int(b[3].max()),
           "final_bandwidths": {str(k): int(v) for k, v in zip(*np.unique(b[2], return_counts=True))},
           "nerrors_mean": float(b[1].mean()), "scores_nerrors_bandwidths_rounds_identical": True,
           "warmup": warmup, "repeats": repeats, "alternating": "B, A" + (", pair_scores" if floor else "") + " per pass",
           "pair_align_smart": {"kernel_ms": stats(a_ms), "fill_ms": stats(a_fill), "walk_ms": stats(a_walk),
                                "wall_ms": stats(a_wall), "device_bytes_grown": int(grown["pair_align_smart"])},
           "pair_errors": {"kernel_ms": stats(b_ms), "wall_ms": stats(b_wall),
                           "device_bytes_grown": int(grown["pair_errors"])},
           "errors_over_align_smart": float(np.median(b_ms) / np.median(a_ms)),
           "errors_median_below_align_smart_min": bool(np.median(b_ms) < min(a_ms))}
    if floor:
        out["pair_scores"] = {"kernel_ms": stats(s_ms)}
        out["errors_over_pair_scores"] = float(np.median(b_ms) / np.median(s_ms))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--case", choices=("c4", "c5_smart", "both"), default="both")
    ap.add_argument("--clusters", type=int, default=1250, help="c4: clusters of 50 reads (1250: 62,500 pairs)")
    ap.add_argument("--smart-pairs", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pair_errors_timing.json"))
    args = ap.parse_args()
    if args.repeats < 5:
        raise SystemExit("at least five timed passes")
    from rifraf_amd.engine import Engine
    from rifraf_amd.poisson import cquantile_poisson_many
    results = []
    for case in ("c4", "c5_smart"):
        if args.case not in (case, "both"):
            continue
        eng = Engine(0)   # a fresh engine per workload: its device_bytes growth is the workload's
        try:
            if case == "c4":
                clusters = make_clusters(args.clusters, 50, 1500, 0.01, 9, args.seed)
                seq = np.arange(50 * args.clusters, dtype=np.int32)
                tpl = seq // 50
                md = 0
            else:
                clusters = make_clusters(1, args.smart_pairs, 10000, 0.01, 9, args.seed + 2)
                seq = np.arange(args.smart_pairs, dtype=np.int32)
                tpl = np.zeros_like(seq)
                md = 5
            reads = [r for _, rs in clusters for r in rs]
            thr = np.asarray(cquantile_poisson_many([r.est_n_errors for r in reads], 0.1), np.float64)[seq]
            results.append(run(eng, case, clusters, seq, tpl, thr, md, args.warmup, args.repeats, case == "c4"))
            print(json.dumps(results[-1]), flush=True)
        finally:
            eng.close()
    if args.out:
        old = []
        if os.path.exists(args.out):
            old = [r for r in json.load(open(args.out))["results"] if r["case"] not in {x["case"] for x in results}]
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"tool": "scripts/pair_errors_timing.py", "device": "MI355X (gfx950)",
                       "results": old + results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
