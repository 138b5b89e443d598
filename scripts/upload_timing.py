#!/usr/bin/env python3
"""Time the sequence uploads on their own, on one GPU: the wall milliseconds
of rf_set_sequences (host tables), rf_set_sequences_codes (Phred codes, tables
built on the device) and rf_set_sequences_codes_prep on a warm context.

Two shapes, Phred-coded reads without codon moves:
  c4  64 clusters x 50 reads x 1.5 kb, one upload (a wave of the c4 workload)
  c3  1,000 reads x 2.6 kb, one upload

Per shape the three calls run alternately in this one process over the same
ids: `--warmup` untimed rounds (arenas, staging and the dictionary are grown),
then `--repeats` timed ones.  These are host wall times: packing, coding and
copies included.  Prints one JSON line per shape and writes them all to --out.

    timeout -k 10 300 python scripts/upload_timing.py
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rifraf.jl_amd"))

SHAPES = {"c4": (64 * 50, 1500), "c3": (1000, 2600)}


def run_shape(eng, name, nreads, length, warmup, repeats, seed):
    from rifraf_amd import ErrorModel, RifrafSequence, Scores
    from rifraf_amd.errormodel import phred_to_log_p
    rng = np.random.default_rng(seed)
    scores = Scores.from_errors(ErrorModel(1.0, 2.0, 2.0, 0.0, 0.0))
    lens = length + rng.integers(-length // 50, length // 50 + 1, nreads)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    bases = rng.integers(0, 4, int(off[-1])).astype(np.uint8)
    phreds = rng.integers(5, 45, int(off[-1])).astype(np.int8)
    reads = [bases[off[k]:off[k + 1]] for k in range(nreads)]
    _, tabs = RifrafSequence.many_concat(reads, phred_to_log_p(phreds), off, 9, scores, phreds=phreds)
    p10 = np.power(10.0, tabs["lp_table"])
    with np.errstate(divide="ignore", invalid="ignore"):
        grid = np.ascontiguousarray(np.power(10.0, tabs["match_table"][None, :] - tabs["match_table"][:, None]))
    calls = {
        "set_sequences": lambda: eng.set_sequences_concat(0, bases, off, tabs["match"], tabs["mismatch"], tabs["ins"],
                                                          tabs["del"]),
        "set_sequences_codes": lambda: eng.set_sequences_codes(0, bases, off, tabs["code"], tabs["lp_table"],
                                                               tabs["match_table"], scores),
        "set_sequences_codes_prep": lambda: eng.set_sequences_codes(0, bases, off, tabs["code"], tabs["lp_table"],
                                                                    tabs["match_table"], scores, prep=(p10, grid)),
    }
    ms = {k: [] for k in calls}
    for it in range(warmup + repeats):
        for k, call in calls.items():
            t0 = time.perf_counter()
            if call() is False:
                raise SystemExit(f"{name}: {k} refused (row-code dictionary full)")
            if it >= warmup:
                ms[k].append((time.perf_counter() - t0) * 1e3)
    out = {"shape": name, "reads": nreads, "read_len_mean": float(lens.mean()), "positions": int(off[-1]),
           "warmup": warmup, "repeats": repeats}
    for k, v in ms.items():
        out[k + "_ms"] = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", choices=("c4", "c3", "both"), default="both")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from rifraf_amd.engine import Engine
    eng = Engine(0)
    results = []
    try:
        for name in ("c4", "c3"):
            if args.shape in (name, "both"):
                results.append(run_shape(eng, name, *SHAPES[name], args.warmup, args.repeats, args.seed))
                print(json.dumps(results[-1]), flush=True)
    finally:
        eng.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "scripts/upload_timing.py", "device": "MI355X (gfx950)", "results": results}, f,
                      indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
