#!/usr/bin/env python3
"""Time the wide tier of the pair calls (RF_OPT_PAIR_WIDE: bands past 5,114
rows, the ring in device memory) against the only other route to the same
numbers, on one GPU: rf_realign(RF_FWD | RF_SKEW) + rf_backtrace of the same
pairs into slots, whose FP64 bands live in the band arena.

Cases, all edit_distance's pairs (log p -1, ErrorModel(1, 1, 1), bandwidth
ceil(min(n, m) / 2), skewed):
  c5_64     64 reads of about 10 kb against their template
  c5_1024   1,024 such reads
  kb5_256   256 reads of about 5.2 kb against theirs

Route B (wide) is one rf_pair_errors call for all pairs.  Route A (slots)
runs in batches of `--slot-batch` pairs, the bands released in between, since
one 10 kb pair's band is about 0.4 GB; with `--slot-pairs` it runs on the
first that many pairs only and its time is scaled to the case (recorded as
such).  The error counts and score bits of the two routes must be identical
on the pairs both ran before anything is reported.  Per case the routes
alternate in this one process on one engine: `--warmup` untimed passes, then
`--repeats` timed ones; medians of the engine's own HIP-event times
(rf_last_timing's DP + rf_last_backtrace_ms for A, rf_last_pair_errors_ms for
B) and the device bytes each route grew by on a fresh engine.  No number is
expected; the file records what ran.

    timeout -k 10 1100 python scripts/pair_wide_timing.py
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rifraf.jl_amd"))
sys.path.insert(0, os.path.join(REPO, "scripts"))

from pair_align_timing import stats  # noqa: E402

CASES = {"c5_64": (64, 10000), "c5_1024": (1024, 10000), "kb5_256": (256, 5200)}


def make_pairs(npairs, length, seed):
    """edit_distance's sequences of `npairs` reads sampled from one template."""
    from rifraf_amd import ErrorModel, RifrafSequence, Scores
    from rifraf_amd.sample import random_seq
    rng = np.random.default_rng(seed)
    t = random_seq(length, rng)
    sc = Scores.from_errors(ErrorModel(1.0, 1.0, 1.0))
    seqs = []
    for _ in range(npairs):
        # an error rate of 0.01: substitutions 8 : insertions 1 : deletions 1
        s = t.copy()
        for i in rng.integers(0, length, rng.binomial(length, 0.008)):
            s[i] = (s[i] + rng.integers(1, 4)) % 4
        for _ in range(rng.binomial(length, 0.001)):
            s = np.insert(s, rng.integers(0, len(s) + 1), rng.integers(0, 4)).astype(np.uint8)
        for _ in range(rng.binomial(length, 0.001)):
            s = np.delete(s, rng.integers(0, len(s)))
        seqs.append(RifrafSequence(s, np.full(len(s), -1.0), int(math.ceil(min(len(s), length) * 0.5)), sc))
    return t, seqs


def slot_route(eng, ids, bws, batch):
    """rf_realign + rf_backtrace of pairs `ids` in batches -> (scores, nerrors, kernel ms)."""
    from rifraf_amd.engine import RF_FWD, RF_SKEW
    sc, ne, ms = [], [], 0.0
    for a in range(0, len(ids), batch):
        k = ids[a:a + batch]
        eng.release_bands()
        sc.append(eng.realign(np.arange(len(k)), k, np.zeros(len(k), np.int32), bws[k], RF_FWD | RF_SKEW))
        ms += eng.last_timing()[0]
        ne.append(eng.backtrace(np.arange(len(k)), want_moves=False)[1])
        ms += eng.last_backtrace_ms()
    return np.concatenate(sc), np.concatenate(ne), ms


def run(name, npairs, length, args):
    from rifraf_amd.engine import RF_SKEW, Engine
    t, seqs = make_pairs(npairs, length, args.seed)
    bws = np.array([s.bandwidth for s in seqs], np.int32)
    ids = np.arange(npairs, dtype=np.int32)
    nslot = min(npairs, args.slot_pairs) if args.slot_pairs else npairs
    rows = 2 * bws + np.abs(np.array([len(s) for s in seqs]) - length) + 1
    grown = {}
    for route in ("wide", "slots"):   # device bytes of each route alone, on a fresh engine
        eng = Engine(0)
        try:
            eng.set_sequences(0, seqs)
            eng.set_templates(0, [t])
            base = eng.device_bytes()
            if route == "wide":
                eng.set_option("pair_wide", 1)
                eng.pair_errors(ids, 0, bws, flags=RF_SKEW)
            else:
                slot_route(eng, ids[:min(nslot, args.slot_batch)], bws, args.slot_batch)
            grown[route] = eng.device_bytes() - base
        finally:
            eng.close()
    eng = Engine(0)
    a_ms, b_ms, a_wall, b_wall = [], [], [], []
    try:
        eng.set_sequences(0, seqs)
        eng.set_templates(0, [t])
        eng.set_option("pair_wide", 1)
        for it in range(args.warmup + args.repeats):
            t0 = time.perf_counter()
            b_sc, b_ne, _, _ = eng.pair_errors(ids, 0, bws, flags=RF_SKEW)
            tb = time.perf_counter() - t0
            kb = eng.last_pair_errors_ms()
            t0 = time.perf_counter()
            a_sc, a_ne, ka = slot_route(eng, ids[:nslot], bws, args.slot_batch)
            ta = time.perf_counter() - t0
            if a_sc.tobytes() != b_sc[:nslot].tobytes() or a_ne.tolist() != b_ne[:nslot].tolist():
                raise SystemExit(f"{name}: the two routes differ")
            if it >= args.warmup:
                a_ms.append(ka * npairs / nslot)
                b_ms.append(kb)
                a_wall.append(ta * 1e3 * npairs / nslot)
                b_wall.append(tb * 1e3)
    finally:
        eng.close()
    return {"case": name, "pairs": npairs, "template_len": length, "band_rows": {"min": int(rows.min()), "max": int(rows.max())},
            "nerrors_mean": float(b_ne.mean()), "scores_and_nerrors_identical": True,
            "warmup": args.warmup, "repeats": args.repeats, "alternating": "B (wide), A (slots) per pass",
            "slots": {"pairs_run": nslot, "scaled_to_all_pairs": nslot != npairs, "batch": args.slot_batch,
                      "kernel_ms": stats(a_ms), "wall_ms": stats(a_wall),
                      "device_bytes_grown_one_batch": int(grown["slots"])},
            "wide": {"kernel_ms": stats(b_ms), "wall_ms": stats(b_wall), "device_bytes_grown": int(grown["wide"])},
            "wide_over_slots": float(np.median(b_ms) / np.median(a_ms))}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--case", choices=tuple(CASES) + ("all",), default="all")
    ap.add_argument("--slot-batch", type=int, default=8, help="pairs per rf_realign call of the slot route")
    ap.add_argument("--slot-pairs", type=int, default=0, help="slot route on the first N pairs only, time scaled (0: all)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seed", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pair_wide_timing.json"))
    args = ap.parse_args()
    results = []
    for name, (npairs, length) in CASES.items():
        if args.case in (name, "all"):
            results.append(run(name, npairs, length, args))
            print(json.dumps(results[-1]), flush=True)
    if args.out:
        old = []
        if os.path.exists(args.out):
            old = [r for r in json.load(open(args.out))["results"] if r["case"] not in {x["case"] for x in results}]
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"tool": "scripts/pair_wide_timing.py", "device": "MI355X (gfx950)", "results": old + results},
                      f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
