#!/usr/bin/env python3
"""Time pairalign.correct_shifts_many through rf_pair_shifts (fill, walk, then
k_pa_fix making the corrected consensuses on the device; one shared reference
uploaded once) against the route it replaces: rf_pair_align with the moves
downloaded, one RifrafSequence table set uploaded per consensus, then
_single_indels + apply_proposals per pair on the host.

Two cases, one reference each, correct_shifts' default scores and bandwidth
(ceil(0.1 min(len))):
  c4    10,000 consensuses of 1.5 kb
  long  256 consensuses of 10 kb
A consensus is the reference with three substitutions and, at random, a
single insertion, a single deletion and an inserted or removed 3-base block.

Per case, in this one process: the new route `--warmup` untimed times and
`--repeats` timed ones (medians and ranges), the replaced route
`--parent-repeats` times.  The kernel times are the engine's HIP-event
figures (rf_last_pair_align_ms, rf_last_pair_shifts_ms); the bytes over PCIe
are computed from the sizes of what each route uploads and downloads (tables,
bases, descriptors left out on both sides).  The corrected consensuses of
both routes must be equal before anything is reported.  No ratio is expected
in advance: the file records what ran.

    timeout -k 10 900 python scripts/pair_shifts_timing.py --case c4
    timeout -k 10 900 python scripts/pair_shifts_timing.py --case long
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
from pair_text_timing import host_cpu  # noqa: E402


def make_case(n_cons, length, seed):
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, length).astype(np.uint8)
    cons = []
    for _ in range(n_cons):
        c = list(ref)
        for at in rng.integers(10, length - 10, 3):
            c[at] = (c[at] + 1 + int(rng.integers(0, 3))) % 4
        sites = sorted(rng.choice(np.arange(20, length - 20, 20), 3, replace=False).tolist(), reverse=True)
        if rng.random() < 0.5:
            c.insert(sites[0], int(rng.integers(0, 4)))
        if rng.random() < 0.5:
            del c[sites[1]]
        if rng.random() < 0.2:
            if rng.random() < 0.5:
                del c[sites[2]:sites[2] + 3]
            else:
                c[sites[2]:sites[2]] = rng.integers(0, 4, 3).tolist()
        cons.append(np.array(c, np.uint8))
    return ref, cons


def moves_route(eng, consensuses, reference, scores):
    """correct_shifts_many as it was before rf_pair_shifts: one table set per
    consensus, the moves to the host, the per-move loop."""
    from rifraf_amd import pairalign
    from rifraf_amd.engine import RF_SKEW
    from rifraf_amd.proposals import apply_proposals
    from rifraf_amd.rifrafsequences import RifrafSequence
    rs = []
    for c in consensuses:
        bw = int(math.ceil(min(len(c), len(reference)) * 0.1))
        rs.append(RifrafSequence(reference, np.full(len(reference), -1.0), bw, scores))
    k = np.arange(len(consensuses), dtype=np.int64)
    bws = np.array([s.bandwidth for s in rs], np.int64)
    _, moves, _ = pairalign._run(eng, rs, consensuses, k, k, bws, RF_SKEW, True)
    ms = eng.last_pair_align_ms()
    return [apply_proposals(c, pairalign._single_indels(mv, s.seq)) for c, s, mv in zip(consensuses, rs, moves)], ms


def table_bytes(n):
    """A sequence's upload: bases, four tables of n doubles (del: n + 1), two codon tables."""
    return n + 8 * (4 * n + 1) + 8 * 2 * max(n - 2, 0)


def run_case(eng, name, ref, cons, warmup, repeats, parent_repeats):
    from rifraf_amd import pairalign
    from rifraf_amd.errormodel import ErrorModel, Scores
    scores = Scores.from_errors(ErrorModel(10.0, 1e-5, 1e-5, 1.0, 1.0))
    n, npairs = len(ref), len(cons)
    mtot = int(sum(len(c) for c in cons))
    fill, walk, fix, wall = [], [], [], []
    new = None
    for it in range(warmup + repeats):
        t0 = time.perf_counter()
        new = pairalign.correct_shifts_many(cons, ref, engine=eng)
        t1 = time.perf_counter()
        if it >= warmup:
            f, w = eng.last_pair_align_ms()
            fill.append(f)
            walk.append(w)
            fix.append(eng.last_pair_shifts_ms())
            wall.append(t1 - t0)
    pfill, pwalk, pwall = [], [], []
    for it in range(parent_repeats):
        t0 = time.perf_counter()
        old, (f, w) = moves_route(eng, cons, ref, scores)
        pwall.append(time.perf_counter() - t0)
        pfill.append(f)
        pwalk.append(w)
        bad = [k for k, (a, b) in enumerate(zip(new, old)) if a.tolist() != b.tolist()]
        if bad:
            raise SystemExit(f"{name}: {len(bad)} corrected consensuses differ (first: pair {bad[0]})")
    changed = sum(len(a) != len(c) for a, c in zip(new, cons))
    return {"case": name, "pairs": npairs, "reference_len": n, "consensus_len_mean": mtot / npairs,
            "bandwidth": int(math.ceil(min(min(len(c) for c in cons), n) * 0.1)),
            "consensuses_changed_in_length": int(changed), "results_identical": True,
            "warmup": warmup, "repeats": repeats, "parent_repeats": parent_repeats,
            "pair_shifts": {"fill_ms": stats(fill), "walk_ms": stats(walk), "fix_ms": stats(fix),
                            "whole_call_s": stats(wall),
                            "pcie_up_bytes": table_bytes(n) + mtot,
                            "pcie_down_bytes": npairs * (8 + 8 + 7 * 4) + npairs * n + mtot},
            "moves_route": {"fill_ms": stats(pfill), "walk_ms": stats(pwalk), "fix_ms": None,
                            "whole_call_s": stats(pwall),
                            "pcie_up_bytes": npairs * table_bytes(n) + mtot,
                            "pcie_down_bytes": npairs * (8 + 8) + npairs * n + mtot},
            "speedup_whole_call": float(np.median(pwall) / np.median(wall)),
            "host_cpu": host_cpu()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--case", choices=("c4", "long", "both"), default="both")
    ap.add_argument("--c4-pairs", type=int, default=10000)
    ap.add_argument("--long-pairs", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-repeats", type=int, default=2)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pair_shifts_timing.json"))
    args = ap.parse_args()
    from rifraf_amd.engine import Engine
    eng = Engine(0)
    results = []
    try:
        for name, npairs, length in (("c4", args.c4_pairs, 1500), ("long", args.long_pairs, 10000)):
            if args.case in (name, "both"):
                ref, cons = make_case(npairs, length, args.seed)
                results.append(run_case(eng, name, ref, cons, args.warmup, args.repeats, args.parent_repeats))
                print(json.dumps(results[-1]), flush=True)
    finally:
        eng.close()
    if args.out:
        old = []
        if os.path.exists(args.out):
            old = [r for r in json.load(open(args.out))["results"] if r["case"] not in {x["case"] for x in results}]
        with open(args.out, "w") as f:
            json.dump({"tool": "scripts/pair_shifts_timing.py", "device": "MI355X (gfx950)",
                       "results": old + results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
