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

Two further measurements go to profiles/pair_align_smart_timing.json:

  --walk-ab   the same two cases, the 10 kb class at --ab-pairs further pair
        counts and c4-sized sets of shorter reads (--ab-short), with RF_OPT_PAIR_WALK 1 (k_pa_walk, one lane per pair) and
        2 (k_pa_walk_w, one wave per pair) alternating in the same protocol;
        for c4 and long the slot path's k_bt_win runs in the same rounds as
        the yardstick.  Moves and counts must be identical.  The automatic
        rule of RF_OPT_PAIR_WALK = 0 (pair_walk_wave in rifraf_hip.hip) is set
        from these numbers.
  --smart     256 c5-shaped pairs (10 kb reads, starting bandwidth 9,
        thresholds from pvalue 0.1): rf_pair_align_smart against the slot
        loop model.smart_forward_moves runs (rf_realign(RF_FWD) +
        rf_backtrace without moves per round), each on an engine of its own so
        that rf_device_bytes is that path's peak.  Final bandwidths, score
        bits and error counts must be equal; the times are a record.

    timeout -k 10 900 python scripts/pair_align_timing.py --walk-ab --case long
    timeout -k 10 900 python scripts/pair_align_timing.py --smart
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


def upload(eng, clusters):
    reads = [r for _, rs in clusters for r in rs]
    for a in range(0, len(reads), 4096):
        eng.set_sequences(a, reads[a:a + 4096])
    eng.set_templates(0, [t for t, _ in clusters])
    return reads


def run_walk_ab(eng, name, clusters, seq_of_pair, tpl_of_pair, bw, warmup, repeats, slots_too):
    """RF_OPT_PAIR_WALK 1 and 2 alternately (and the slot path's backtrace
    when slots_too), identical moves and counts required."""
    from rifraf_amd.engine import RF_FWD
    reads = upload(eng, clusters)
    npairs = len(seq_of_pair)
    slots = np.arange(npairs, dtype=np.int32)
    bws = np.full(npairs, bw, np.int32)
    lens = np.array([len(r) for r in reads])
    tlen = np.array([len(t) for t, _ in clusters])
    caps = lens[seq_of_pair] + tlen[tpl_of_pair]
    fill = {1: [], 2: []}
    walk = {1: [], 2: []}
    bt = []
    for it in range(warmup + repeats):
        got = {}
        for w in (1, 2):
            eng.set_option("pair_walk", w)
            got[w] = eng.pair_align(seq_of_pair, tpl_of_pair, bws, caps=caps)
            f, t = eng.last_pair_align_ms()
            if it >= warmup:
                fill[w].append(f)
                walk[w].append(t)
        if not np.array_equal(got[1][2], got[2][2]) or (got[1][2] < 0).any():
            raise SystemExit(f"{name}: error counts differ between the two walks")
        bad = [k for k in range(npairs) if not np.array_equal(got[1][1][k], got[2][1][k])]
        if bad:
            raise SystemExit(f"{name}: moves of {len(bad)} of {npairs} pairs differ between the two walks")
        if slots_too:
            eng.realign(slots, seq_of_pair, tpl_of_pair, bws, RF_FWD)
            _, ne2 = eng.backtrace(slots, want_moves=False)
            t = c_double()
            eng.lib.rf_last_backtrace_ms(eng.ctx, byref(t))
            if not np.array_equal(got[1][2], ne2):
                raise SystemExit(f"{name}: error counts differ between rf_pair_align and rf_backtrace")
            if it >= warmup:
                bt.append(t.value)
    eng.set_option("pair_walk", 0)
    out = {"case": name, "measurement": "walk_ab", "pairs": npairs, "bandwidth": bw,
           "n_plus_m_mean": float(caps.mean()), "moves_nerrors_identical": True, "warmup": warmup,
           "repeats": repeats, "fill_ms": stats(fill[1] + fill[2]), "walk_lane_ms": stats(walk[1]),
           "walk_wave_ms": stats(walk[2]), "wave_speedup_vs_lane": float(np.median(walk[1]) / np.median(walk[2]))}
    if slots_too:
        out["slot_backtrace_ms"] = stats(bt)
    return out


def slot_smart(eng, npairs, seqs, bws, thr, maxbw):
    """model.smart_forward_moves' loop over slots k = pair k against template 0."""
    from rifraf_amd.engine import RF_FWD
    bw = np.array(bws, np.int32)
    scores = np.empty(npairs)
    nerr = np.full(npairs, -1, np.int32)
    n_err = np.full(npairs, np.iinfo(np.int64).max)
    pending = np.arange(npairs, dtype=np.int32)
    dp_ms = bt_ms = 0.0
    rounds = 0
    while len(pending):
        rounds += 1
        scores[pending] = eng.realign(pending, seqs[pending], 0, bw[pending], RF_FWD)
        dp_ms += eng.last_timing()[0]
        _, ne = eng.backtrace(pending, want_moves=False)   # also for the pairs that stop at max_bw: nerrors is reported
        t = c_double()
        eng.lib.rf_last_backtrace_ms(eng.ctx, byref(t))
        bt_ms += t.value
        nerr[pending] = ne
        check = bw[pending] < maxbw[pending]
        old = n_err[pending]
        more = check & (ne > thr[pending]) & (ne < old)
        n_err[pending] = np.where(check, ne, old)
        pending = pending[more]
        bw[pending] = np.minimum(2 * bw[pending], maxbw[pending])
    return scores, nerr, bw, rounds, dp_ms, bt_ms


def run_smart(device, npairs, warmup, repeats, seed):
    from rifraf_amd.engine import Engine
    from rifraf_amd.poisson import cquantile_poisson_many
    clusters = make_clusters(1, npairs, 10000, 0.01, 9, seed)
    reads = clusters[0][1]
    m = len(clusters[0][0])
    seqs = np.arange(npairs, dtype=np.int32)
    bws = np.full(npairs, 9, np.int32)
    thr = np.asarray(cquantile_poisson_many([r.est_n_errors for r in reads], 0.1), np.float64)
    lens = np.array([len(r) for r in reads])
    maxbw = np.minimum(np.minimum(bws << 5, m), lens).astype(np.int32)
    res = {}
    for path in ("pair", "slot"):
        eng = Engine(device)
        eng.set_option("dp_lat", 0)
        try:
            upload(eng, clusters)
            base = eng.device_bytes()
            wall, k1, k2 = [], [], []
            for it in range(warmup + repeats):
                t0 = time.perf_counter()
                if path == "pair":
                    sc, _, ne, bw, rd = eng.pair_align_smart(seqs, 0, bws, thr, want_moves=False)
                    dt = time.perf_counter() - t0
                    a, b = eng.last_pair_align_ms()
                    rounds = int(rd.max())
                else:
                    sc, ne, bw, rounds, a, b = slot_smart(eng, npairs, seqs, bws, thr, maxbw)
                    dt = time.perf_counter() - t0
                if it >= warmup:
                    wall.append(dt * 1e3)
                    k1.append(a)
                    k2.append(b)
            res[path] = dict(scores=sc.copy(), nerr=np.asarray(ne).copy(), bw=np.asarray(bw).copy(), rounds=rounds,
                             wall_ms=stats(wall), fill_ms=stats(k1), walk_ms=stats(k2),
                             kernel_ms=stats(np.array(k1) + np.array(k2)), device_bytes=eng.device_bytes(),
                             device_bytes_grown=eng.device_bytes() - base)
        finally:
            eng.close()
    p, q = res["pair"], res["slot"]
    if not np.array_equal(p["bw"], q["bw"]):
        raise SystemExit("smart: final bandwidths differ between rf_pair_align_smart and the slot loop")
    if not np.array_equal(p["scores"].view(np.int64), q["scores"].view(np.int64)):
        raise SystemExit("smart: scores differ between rf_pair_align_smart and the slot loop")
    if not np.array_equal(p["nerr"], q["nerr"]):
        raise SystemExit("smart: error counts differ between rf_pair_align_smart and the slot loop")
    out = {"case": "c5_smart", "measurement": "smart", "pairs": npairs, "start_bandwidth": 9, "pvalue": 0.1,
           "read_len_mean": float(lens.mean()), "template_len": m,
           "final_bandwidths": {str(k): int(v) for k, v in zip(*np.unique(p["bw"], return_counts=True))},
           "rounds": p["rounds"], "bandwidths_scores_nerrors_identical": True, "warmup": warmup, "repeats": repeats}
    for name, r in (("pair_align_smart", p), ("slot_loop", q)):
        out[name] = {k: r[k] for k in ("wall_ms", "fill_ms", "walk_ms", "kernel_ms", "device_bytes",
                                       "device_bytes_grown")}
    return out


def write_out(path, results, key):
    old = []
    if os.path.exists(path):
        old = [r for r in json.load(open(path))["results"] if key(r) not in {key(x) for x in results}]
    with open(path, "w") as f:
        json.dump({"tool": "scripts/pair_align_timing.py", "device": "MI355X (gfx950)",
                   "results": old + results}, f, indent=1)
        f.write("\n")


def main_smart(args):
    from rifraf_amd.engine import Engine
    results = []
    if args.walk_ab:
        eng = Engine(0)
        eng.set_option("dp_lat", 0)
        try:
            if args.case in ("c4", "both"):
                clusters = make_clusters(args.clusters, 50, 1500, 0.01, 9, args.seed)
                seq = np.arange(50 * args.clusters, dtype=np.int32)
                results.append(run_walk_ab(eng, "c4", clusters, seq, seq // 50, 9, args.warmup, args.repeats, True))
                print(json.dumps(results[-1]), flush=True)
                eng.release_bands()
            for length in (args.ab_short if args.case in ("short", "both") else []):
                clusters = make_clusters(args.clusters, 50, length, 0.01, 9, args.seed + length)
                seq = np.arange(50 * args.clusters, dtype=np.int32)
                results.append(run_walk_ab(eng, f"short_{length}", clusters, seq, seq // 50, 9, args.warmup,
                                           args.repeats, False))
                print(json.dumps(results[-1]), flush=True)
            if args.case in ("long", "both"):
                clusters = make_clusters(1, 64, 10000, 0.01, 72, args.seed + 1)
                for npairs in sorted(set(args.ab_pairs + [args.long_pairs])):
                    seq = (np.arange(npairs) % 64).astype(np.int32)
                    name = "long" if npairs == args.long_pairs else f"long_{npairs}"
                    results.append(run_walk_ab(eng, name, clusters, seq, np.zeros_like(seq), 72, args.warmup,
                                               args.repeats, npairs == args.long_pairs))
                    print(json.dumps(results[-1]), flush=True)
        finally:
            eng.close()
    if args.smart:
        results.append(run_smart(0, args.smart_pairs, args.warmup, args.repeats, args.seed + 2))
        print(json.dumps(results[-1]), flush=True)
    if args.smart_out:
        write_out(args.smart_out, results, lambda r: (r["measurement"], r["case"]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--case", choices=("c4", "long", "short", "both"), default="both")
    ap.add_argument("--clusters", type=int, default=1250, help="c4: clusters of 50 reads (1250: 62,500 pairs)")
    ap.add_argument("--long-pairs", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pair_align_timing.json"))
    ap.add_argument("--walk-ab", action="store_true", help="RF_OPT_PAIR_WALK 1 against 2 instead of the default run")
    ap.add_argument("--ab-pairs", type=int, nargs="*", default=[16, 128, 4096],
                    help="--walk-ab: further pair counts of the 10 kb class")
    ap.add_argument("--ab-short", type=int, nargs="*", default=[50, 150, 400],
                    help="--walk-ab: read lengths of further c4-sized sets (clusters x 50 pairs at bw 9)")
    ap.add_argument("--smart", action="store_true", help="rf_pair_align_smart against the slot loop")
    ap.add_argument("--smart-pairs", type=int, default=256)
    ap.add_argument("--smart-out", default=os.path.join(REPO, "profiles", "pair_align_smart_timing.json"))
    args = ap.parse_args()
    if args.walk_ab or args.smart:
        return main_smart(args)
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
