#!/usr/bin/env python3
"""Time rf_pair_scores (the score-only forward pass) against the only other
way to get the same numbers, rf_realign(RF_FWD) into slots, on one GPU.

Two cases, each a list of (read, template) pairs scored by both paths:
  c4    62,500 pairs of the c4 read shape (clusters of 50 reads x 1.5 kb at
        error rate 0.01, bw 9; reads from rifraf_amd.sample as bench.py makes
        them), every read against its cluster's template
  long  one 10 kb class at bw 72: 1,024 pairs over 64 distinct reads

Per case the two paths run alternately in this one process: `--warmup`
untimed rounds, then `--repeats` timed ones; the kernel times are the
engine's own HIP-event figures (rf_last_pair_ms, rf_last_timing's dp_ms).
The two score vectors must be bitwise equal before anything is reported.
Prints one JSON line per case and writes them all to --out.

    timeout -k 10 600 python scripts/pair_scores_timing.py --case c4
    timeout -k 10 600 python scripts/pair_scores_timing.py --case long
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rifraf.jl_amd"))

FP64_VEC_TFLOPS = 78.6   # MI355X vector FP64 FMA peak; 5 non-FMA ops per cell (3 adds, 2 max): SURVEY.md §8(d)
VALU_CELLS_PER_S = FP64_VEC_TFLOPS / 2 / 5 * 1e12


def make_clusters(nclusters, nreads, length, error_rate, bw, seed):
    """bench.py's make_workload: clusters of reads sampled from a random template."""
    from rifraf_amd import ErrorModel, RifrafSequence, Scores
    from rifraf_amd.sample import MAX_PROB, MIN_PROB, random_seq, sample_from_template
    rng = np.random.default_rng(seed)
    scores = Scores.from_errors(ErrorModel(1.0, 2.0, 2.0, 0.0, 0.0))
    alpha = 0.1
    beta = alpha * (error_rate - MAX_PROB) / (MIN_PROB - error_rate)
    out = []
    for _ in range(nclusters):
        t = random_seq(length, rng)
        t_p = rng.beta(alpha, beta, size=length) * (MAX_PROB - MIN_PROB) + MIN_PROB
        reads = []
        for _ in range(nreads):
            s, _, ph, _, _ = sample_from_template(t, t_p, ErrorModel(1, 5, 5), 1.5, 3.0, 1.0, rng)
            reads.append(RifrafSequence(s, ph, bw, scores))
        out.append((t, reads))
    return out


def inband_cells(n, m, bw):
    """In-band cells of the (n+1) x (m+1) matrix (bandedarrays.jl row_range)."""
    j = np.arange(m + 1)
    lo = np.maximum(0, j - max(m - n, 0) - bw)
    hi = np.minimum(n, j + max(n - m, 0) + bw)
    return int(np.sum(hi - lo + 1))


def run_case(eng, name, clusters, seq_of_pair, tpl_of_pair, bw, warmup, repeats):
    from rifraf_amd.engine import RF_FWD
    reads = [r for _, rs in clusters for r in rs]
    for a in range(0, len(reads), 4096):
        eng.set_sequences(a, reads[a:a + 4096])
    eng.set_templates(0, [t for t, _ in clusters])
    npairs = len(seq_of_pair)
    slots = np.arange(npairs, dtype=np.int32)
    bws = np.full(npairs, bw, np.int32)
    lens = np.array([len(r) for r in reads])
    tlen = np.array([len(t) for t, _ in clusters])
    shapes, counts = np.unique(np.stack([lens[seq_of_pair], tlen[tpl_of_pair]], 1), axis=0, return_counts=True)
    cells = int(sum(c * inband_cells(int(n), int(m), bw) for (n, m), c in zip(shapes, counts)))
    pair_ms, fill_ms = [], []
    for it in range(warmup + repeats):
        a = eng.pair_scores(seq_of_pair, tpl_of_pair, bws)
        p = eng.last_pair_ms()
        b = eng.realign(slots, seq_of_pair, tpl_of_pair, bws, RF_FWD)
        f = eng.last_timing()[0]
        if not np.array_equal(a.view(np.int64), b.view(np.int64)):
            raise SystemExit(f"{name}: {int(np.sum(a.view(np.int64) != b.view(np.int64)))} of {npairs} "
                             "scores differ between rf_pair_scores and rf_realign")
        if it >= warmup:
            pair_ms.append(p)
            fill_ms.append(f)
    pm, fm = float(np.median(pair_ms)), float(np.median(fill_ms))
    return {"case": name, "pairs": npairs, "bandwidth": bw, "read_len_mean": float(lens[seq_of_pair].mean()),
            "template_len_mean": float(tlen[tpl_of_pair].mean()), "inband_cells": cells,
            "scores_bitwise_equal": True, "warmup": warmup, "repeats": repeats,
            "pair_scores_ms": {"median": pm, "min": float(min(pair_ms)), "max": float(max(pair_ms))},
            "realign_fwd_dp_ms": {"median": fm, "min": float(min(fill_ms)), "max": float(max(fill_ms))},
            "speedup_vs_fill": fm / pm,
            "pair_scores_cells_per_s": cells / (pm * 1e-3),
            "realign_fwd_cells_per_s": cells / (fm * 1e-3),
            "fp64_valu_ceiling_cells_per_s": VALU_CELLS_PER_S,
            "pair_scores_frac_of_valu_ceiling": cells / (pm * 1e-3) / VALU_CELLS_PER_S,
            "realign_fwd_frac_of_valu_ceiling": cells / (fm * 1e-3) / VALU_CELLS_PER_S}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--case", choices=("c4", "long", "both"), default="both")
    ap.add_argument("--clusters", type=int, default=1250, help="c4: clusters of 50 reads (1250: 62,500 pairs)")
    ap.add_argument("--long-pairs", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pair_scores_timing.json"))
    args = ap.parse_args()
    from rifraf_amd.engine import Engine
    eng = Engine(0)
    eng.set_option("dp_lat", 0)   # the throughput DP classes, as bench.py's step
    results = []
    try:
        if args.case in ("c4", "both"):
            t0 = time.time()
            clusters = make_clusters(args.clusters, 50, 1500, 0.01, 9, args.seed)
            print(f"c4: {args.clusters} clusters generated in {time.time() - t0:.1f} s", file=sys.stderr)
            seq = np.arange(50 * args.clusters, dtype=np.int32)
            results.append(run_case(eng, "c4", clusters, seq, seq // 50, 9, args.warmup, args.repeats))
            print(json.dumps(results[-1]), flush=True)
            eng.release_bands()
        if args.case in ("long", "both"):
            clusters = make_clusters(1, 64, 10000, 0.01, 72, args.seed + 1)
            seq = (np.arange(args.long_pairs) % 64).astype(np.int32)
            results.append(run_case(eng, "long", clusters, seq, np.zeros_like(seq), 72, args.warmup, args.repeats))
            print(json.dumps(results[-1]), flush=True)
    finally:
        eng.close()
    if args.out:
        old = []
        if os.path.exists(args.out):
            old = [r for r in json.load(open(args.out))["results"] if r["case"] not in {x["case"] for x in results}]
        with open(args.out, "w") as f:
            json.dump({"tool": "scripts/pair_scores_timing.py", "device": "MI355X (gfx950)",
                       "results": old + results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
