#!/usr/bin/env python3
"""Time rf_score_dense_from against rf_score_dense, and the chunked driver
rifraf_amd.deep.dense_totals_chunked against one shot, on one GPU.

Shapes:
  c4_wave  256 clusters x 50 reads x 1,500 bases at bandwidth 9 (one wave of
           the c4 workload)
  c5_deep  one cluster of --c5-reads reads x 10,000 bases at bandwidth 9: the
           c5 shape with the read count cut from 5,000 to what this script's
           time allows (the default 500); the cut is recorded in the file

Part 1, continued against plain scoring (c4_wave, bands resident): per round
rf_score_dense, rf_score_dense_from(init = NULL) and rf_score_dense_from(init
= a table on the host), totals left on the device, alternately in this one
process: `--warmup` untimed rounds, then `--repeats` timed ones.  Kernel ms
are the engine's HIP-event figure (rf_last_timing's score_ms: scorer and fold,
without the upload of init); wall ms are host clocks around the calls, so the
upload of init shows there.  Both scorer modes run (fused: the kernels start
from init; split: k_reduce does).

Part 2, chunked against one shot (both shapes): dense_totals_chunked on a
fresh engine under band budgets that cut the deepest cluster into about 1, 2,
4 and 8 chunks: fill ms and score ms (HIP events, summed over the rounds), wall
s of the whole call (uploads, fills, scoring, downloads) and rf_device_bytes
afterwards (arenas never shrink: the peak).  Every table must have the bits of
the one-chunk run before anything is reported.  No ratio is expected in
advance: the file records what ran.

    timeout -k 10 900 python scripts/score_dense_from_timing.py
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


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    nan = np.isnan(a) | np.isnan(b)
    return bool(np.where(nan, np.isnan(a) & np.isnan(b), a.view(np.int64) == b.view(np.int64)).all())


def make_clusters(nclusters, nreads, length, bw, rng):
    """Templates and reads with about 1 % substitutions and 0.5 % indels each
    way, Phred 8..39 per base (finite tables: the lean scorers)."""
    from rifraf_amd import ErrorModel, RifrafSequence, Scores
    scores = Scores.from_errors(ErrorModel(1.0, 2.0, 2.0, 0.0, 0.0))
    tpls, reads = [], []
    for _ in range(nclusters):
        t = rng.integers(0, 4, length).astype(np.uint8)
        rs = []
        for _ in range(nreads):
            keep = rng.random(length) >= 0.005
            s = t[keep]
            ins = np.flatnonzero(rng.random(len(s)) < 0.005)
            s = np.insert(s, ins, rng.integers(0, 4, len(ins)).astype(np.uint8))
            sub = rng.random(len(s)) < 0.01
            s[sub] = (s[sub] + rng.integers(1, 4, int(sub.sum()))) % 4
            rs.append(RifrafSequence(s, rng.integers(8, 40, len(s)) / -10.0, bw, scores))
        tpls.append(t)
        reads.append(rs)
    return tpls, reads


def continued_vs_plain(tpls, reads, warmup, repeats):
    from rifraf_amd.engine import RF_BWD, RF_FWD, Engine, pack_groups
    e = Engine(0)
    out = {}
    try:
        flat = [r for rs in reads for r in rs]
        e.set_sequences(0, flat)
        e.set_templates(0, tpls)
        tpl = [c for c, rs in enumerate(reads) for _ in rs]
        k = np.arange(len(flat))
        e.realign(k, k, tpl, [r.bandwidth for r in flat], RF_FWD | RF_BWD)
        at, groups = 0, []
        for rs in reads:
            groups.append(np.arange(at, at + len(rs), dtype=np.int32))
            at += len(rs)
        pg = pack_groups(groups)
        rows = [len(t) + 1 for t in tpls]
        for mode in ("fused", "split"):
            e.set_option("score_mode", mode)
            plain = e.score_dense(pg, rows=rows)
            if not all(same_bits(a, b) for a, b in zip(e.score_dense_from(pg, None, rows=rows), plain)):
                raise SystemExit("rf_score_dense_from(init = NULL) differs from rf_score_dense")
            # init = the fold of each cluster's first half; then the second half continues it
            half = pack_groups([g[:len(g) // 2] for g in groups])
            rest = pack_groups([g[len(g) // 2:] for g in groups])
            init = e.score_dense(half, rows=rows)
            if not all(same_bits(a, b) for a, b in zip(e.score_dense_from(rest, init, rows=rows), plain)):
                raise SystemExit("the continued fold differs from the one-shot fold")
            launch = e.last_score_launch()
            rec = {k2: [] for k2 in ("dense_kernel", "dense_wall", "from_null_kernel", "from_null_wall",
                                     "from_init_kernel", "from_init_wall")}
            table = [np.array(t) for t in plain]     # a table of the call's layout (values do not matter for time)
            for it in range(warmup + repeats):
                row = []
                for call in (lambda: e.score_dense(pg, to_host=False),
                             lambda: e.score_dense_from(pg, None, to_host=False, rows=rows),
                             lambda: e.score_dense_from(pg, table, to_host=False, rows=rows)):
                    t0 = time.perf_counter()
                    call()
                    row += [e.last_timing()[1], 1e3 * (time.perf_counter() - t0)]
                if it >= warmup:
                    for key, v in zip(rec, row):
                        rec[key].append(v)
            out[mode] = {"kernel": launch.kernel, "split": launch.split,
                         "table_bytes": int(sum(rows) * 9 * 8), **{k2 + "_ms": stats(v) for k2, v in rec.items()}}
            out[mode]["init_cost_kernel_ms"] = (out[mode]["from_init_kernel_ms"]["median"]
                                                - out[mode]["dense_kernel_ms"]["median"])
        e.set_option("score_mode", "auto")
    finally:
        e.close()
    return out


def arena_budget(payload):
    """The smallest band_bytes whose arena holds `payload` bytes of bands
    (_lib.host_reserve_fit is monotone)."""
    from rifraf_amd import _lib
    lo, hi = 2 << 20, 2 * int(payload) + (4 << 20)
    while lo < hi:
        mid = (lo + hi) // 2
        if _lib.host_reserve_fit(mid) >= payload:
            hi = mid
        else:
            lo = mid + 1
    return lo


def chunked_vs_one_shot(name, tpls, reads, nchunks):
    from rifraf_amd.deep import dense_totals_chunked, read_band_bytes
    from rifraf_amd.engine import Engine
    C = len(tpls)
    deepest = max(sum(read_band_bytes(len(r), len(t), r.bandwidth, None) for r in rs) for t, rs in zip(tpls, reads))
    first, rows = None, []
    for k in nchunks:
        payload = C * (-(-deepest // k) + (1 << 16))
        budget = arena_budget(payload)
        e = Engine(0)
        try:
            st = {}
            t0 = time.perf_counter()
            tabs, _ = dense_totals_chunked(reads, tpls, band_bytes=budget, engine=e, stats=st)
            wall = time.perf_counter() - t0
            dev = e.device_bytes()
        finally:
            e.close()
        if first is None:
            first = tabs
        elif not all(same_bits(a, b) for a, b in zip(tabs, first)):
            raise SystemExit(f"{name}: {k} chunks differ from one chunk")
        row = {"case": name, "chunks_asked": k, "rounds": len(st["fill_ms"]), "band_budget_bytes": int(budget),
               "band_payload_bytes": int(payload),
               "round_band_bytes_max": int(max(st["round_band_bytes"])), "fill_ms": float(sum(st["fill_ms"])),
               "score_ms": float(sum(st["score_ms"])), "wall_s": wall, "device_bytes": int(dev),
               "tables_identical": True}
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--clusters", type=int, default=256)
    ap.add_argument("--c5-reads", type=int, default=500)
    ap.add_argument("--chunks", type=int, nargs="*", default=[1, 2, 4, 8])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "score_dense_from_timing.json"))
    args = ap.parse_args()
    rng = np.random.default_rng(4100)
    tpls, reads = make_clusters(args.clusters, 50, 1500, 9, rng)
    res = {"script": "scripts/score_dense_from_timing.py", "device": "MI355X (gfx950)",
           "c4_wave": {"clusters": args.clusters, "reads": 50, "length": 1500, "bandwidth": 9},
           "c5_deep": {"clusters": 1, "reads": args.c5_reads, "length": 10000, "bandwidth": 9,
                       "note": "the c5 shape with 5,000 reads cut to this count for the script's time"},
           "warmup": args.warmup, "repeats": args.repeats}
    res["continued_vs_plain"] = continued_vs_plain(tpls, reads, args.warmup, args.repeats)
    print(json.dumps(res["continued_vs_plain"]), flush=True)
    res["chunked"] = chunked_vs_one_shot("c4_wave", tpls, reads, args.chunks)
    t5, r5 = make_clusters(1, args.c5_reads, 10000, 9, rng)
    res["chunked"] += chunked_vs_one_shot("c5_deep", t5, r5, args.chunks)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
