#!/usr/bin/env python3
"""Time rf_pair_align (fill with a 4-bit move trace, then the walk) against the
only other way to get the same alignments, rf_realign(RF_FWD) into slots +
rf_backtrace, on one GPU.

The two shapes of scripts/pair_scores_timing.py:
  c4    62,500 pairs of the c4 read shape (1.5 kb, error rate 0.01, bw 9),
        every read against its cluster's template
  long  one 10 kb class at bw 72: 1,024 pairs over 64 distinct reads

Per case the two paths run alternately in this one process: `--warmup`
untimed rounds, then `--repeats` timed ones; the kernel times are the engine's
own HIP-event figures (rf_last_pair_align_ms; rf_last_timing's dp_ms and
rf_last_backtrace_ms).  Moves, error counts and scores must be identical
before anything is reported.  Prints one JSON line per case and writes them
all to --out.  No ratio is expected in advance: the file records what ran.

    timeout -k 10 900 python scripts/pair_align_timing.py --case c4
    timeout -k 10 900 python scripts/pair_align_timing.py --case long
"""
import argparse
import json
import os
import sys
import time
from ctypes import byref, c_double

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rifraf.jl_amd"))
sys.path.insert(0, os.path.join(REPO, "scripts"))

from pair_scores_timing import inband_cells, make_clusters  # noqa: E402


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


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
    caps = lens[seq_of_pair] + tlen[tpl_of_pair]
    shapes, counts = np.unique(np.stack([lens[seq_of_pair], tlen[tpl_of_pair]], 1), axis=0, return_counts=True)
    cells = int(sum(c * inband_cells(int(n), int(m), bw) for (n, m), c in zip(shapes, counts)))
    before = eng.device_bytes()
    fill, walk, dp, bt = [], [], [], []
    trace_bytes = None
    for it in range(warmup + repeats):
        sc, mv, ne = eng.pair_align(seq_of_pair, tpl_of_pair, bws, caps=caps)
        f, w = eng.last_pair_align_ms()
        if trace_bytes is None:
            trace_bytes = eng.device_bytes() - before
        b = eng.realign(slots, seq_of_pair, tpl_of_pair, bws, RF_FWD)
        d = eng.last_timing()[0]
        mv2, ne2 = eng.backtrace(slots)
        t = c_double()
        eng.lib.rf_last_backtrace_ms(eng.ctx, byref(t))
        if not np.array_equal(sc.view(np.int64), b.view(np.int64)):
            raise SystemExit(f"{name}: scores differ between rf_pair_align and rf_realign")
        if not np.array_equal(ne, ne2):
            raise SystemExit(f"{name}: error counts differ between rf_pair_align and rf_backtrace")
        bad = [k for k in range(npairs) if mv[k] is None or not np.array_equal(mv[k], mv2[k])]
        if bad:
            raise SystemExit(f"{name}: moves of {len(bad)} of {npairs} pairs differ (first: pair {bad[0]})")
        if it >= warmup:
            fill.append(f)
            walk.append(w)
            dp.append(d)
            bt.append(t.value)
    new = np.array(fill) + np.array(walk)
    old = np.array(dp) + np.array(bt)
    return {"case": name, "pairs": npairs, "bandwidth": bw, "read_len_mean": float(lens[seq_of_pair].mean()),
            "template_len_mean": float(tlen[tpl_of_pair].mean()), "inband_cells": cells,
            "moves_nerrors_scores_identical": True, "warmup": warmup, "repeats": repeats,
            "pair_align_fill_ms": stats(fill), "pair_align_walk_ms": stats(walk), "pair_align_ms": stats(new),
            "realign_fwd_dp_ms": stats(dp), "backtrace_ms": stats(bt), "realign_backtrace_ms": stats(old),
            "speedup_vs_realign_backtrace": float(np.median(old) / np.median(new)),
            "fill_speedup_vs_realign": float(np.median(dp) / np.median(fill)),
            "walk_speedup_vs_backtrace": float(np.median(bt) / np.median(walk)),
            "pair_align_device_bytes": int(trace_bytes),
            "a_band_bytes": int(sum(c * (2 * bw + abs(int(n) - int(m)) + 1) * (int(m) + 1) * 8
                                    for (n, m), c in zip(shapes, counts)))}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--case", choices=("c4", "long", "both"), default="both")
    ap.add_argument("--clusters", type=int, default=1250, help="c4: clusters of 50 reads (1250: 62,500 pairs)")
    ap.add_argument("--long-pairs", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pair_align_timing.json"))
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
            json.dump({"tool": "scripts/pair_align_timing.py", "device": "MI355X (gfx950)",
                       "results": old + results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
