#!/usr/bin/env python3
"""Time rf_pair_align_text (fill, walk, then k_pa_emit making the gapped texts
on the device) against the route it replaces for align_many: rf_pair_align
with the moves downloaded, then align.moves_to_aligned_seqs per pair on the
host.

The two shapes of scripts/pair_align_timing.py:
  c4    62,500 pairs of the c4 read shape (1.5 kb, error rate 0.01, bw 9),
        every read against its cluster's template
  long  one 10 kb class at bw 72: 1,024 pairs over 64 distinct reads

Per case, in this one process: `--warmup` untimed rounds, then `--repeats`
timed ones, medians reported.  A round is
  - one Engine.pair_align_text call for the texts with the sequences already
    uploaded, and the decoding of every pair's two strings (text_call_wall_s);
    its kernel times are the engine's HIP-event figures (rf_last_pair_align_ms,
    rf_last_pair_text_ms);
  - the replaced route on a sample of `--sample` pairs spread evenly over the
    case: Engine.pair_align with moves, then moves_to_aligned_seqs per pair,
    wall time scaled by pairs / sample (moves_route_wall_s_scaled).  The host
    loop is the bulk of it and is linear in the pairs; the sample size and the
    host CPU are recorded.
The strings of the sample must be equal on both routes before anything is
reported.  pairalign.align_many over the whole case (uploads included) is
timed once per case after the rounds (align_many_wall_s).  No ratio is expected
in advance: the file records what ran.

    timeout -k 10 900 python scripts/pair_text_timing.py --case c4
    timeout -k 10 900 python scripts/pair_text_timing.py --case long
"""
import argparse
import json
import os
import platform
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "rifraf.jl_amd"))
sys.path.insert(0, os.path.join(REPO, "scripts"))

from pair_align_timing import stats, upload  # noqa: E402
from pair_scores_timing import make_clusters  # noqa: E402


def host_cpu():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or platform.machine()


def run_case(eng, name, clusters, seq_of_pair, tpl_of_pair, bw, warmup, repeats, sample):
    from rifraf_amd import pairalign
    from rifraf_amd.align import moves_to_aligned_seqs
    reads = upload(eng, clusters)
    tpls = [t for t, _ in clusters]
    npairs = len(seq_of_pair)
    bws = np.full(npairs, bw, np.int32)
    lens = np.array([len(r) for r in reads])
    tlen = np.array([len(t) for t in tpls])
    caps = (lens[seq_of_pair] + tlen[tpl_of_pair], tlen[tpl_of_pair])
    pick = np.unique(np.linspace(0, npairs - 1, min(sample, npairs)).astype(np.int64))
    fill, walk, emit, text_wall, old_wall = [], [], [], [], []
    for it in range(warmup + repeats):
        t0 = time.perf_counter()
        _, r = eng.pair_align_text(seq_of_pair, tpl_of_pair, bws, caps=caps)
        texts = r.texts()
        t1 = time.perf_counter()
        f, w = eng.last_pair_align_ms()
        e = eng.last_pair_text_ms()
        t2 = time.perf_counter()
        _, mv, _ = eng.pair_align(seq_of_pair[pick], tpl_of_pair[pick], bws[pick],
                                  caps=caps[0][pick])
        old = [moves_to_aligned_seqs(m, tpls[int(j)], reads[int(i)].seq)
               for m, i, j in zip(mv, seq_of_pair[pick], tpl_of_pair[pick])]
        t3 = time.perf_counter()
        bad = [int(k) for k, o in zip(pick, old) if texts[int(k)] != o]
        if bad:
            raise SystemExit(f"{name}: texts of {len(bad)} of {len(pick)} sampled pairs differ (first: pair {bad[0]})")
        if it >= warmup:
            fill.append(f)
            walk.append(w)
            emit.append(e)
            text_wall.append(t1 - t0)
            old_wall.append((t3 - t2) * npairs / len(pick))
    pairs = np.stack([seq_of_pair, tpl_of_pair], 1)
    t0 = time.perf_counter()
    many = pairalign.align_many(reads, tpls, pairs=pairs, bandwidth=bw, engine=eng)
    many_wall = time.perf_counter() - t0
    if many != texts:
        raise SystemExit(f"{name}: align_many differs from pair_align_text")
    return {"case": name, "pairs": npairs, "bandwidth": bw, "read_len_mean": float(lens[seq_of_pair].mean()),
            "template_len_mean": float(tlen[tpl_of_pair].mean()),
            "aligned_len_mean": float(np.mean(r.aln_len)), "texts_identical_on_sample": True,
            "warmup": warmup, "repeats": repeats, "fill_ms": stats(fill), "walk_ms": stats(walk),
            "emit_ms": stats(emit), "emit_over_walk": float(np.median(emit) / np.median(walk)),
            "text_call_wall_s": stats(text_wall), "align_many_wall_s": many_wall,
            "moves_route_sample_pairs": int(len(pick)), "moves_route_wall_s_scaled": stats(old_wall),
            "speedup_text_call_vs_moves_route": float(np.median(old_wall) / np.median(text_wall)),
            "host_cpu": host_cpu()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--case", choices=("c4", "long", "both"), default="both")
    ap.add_argument("--clusters", type=int, default=1250, help="c4: clusters of 50 reads (1250: 62,500 pairs)")
    ap.add_argument("--long-pairs", type=int, default=1024)
    ap.add_argument("--sample", type=int, default=256, help="pairs the replaced route is timed on")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pair_text_timing.json"))
    args = ap.parse_args()
    from rifraf_amd.engine import Engine
    eng = Engine(0)
    results = []
    try:
        if args.case in ("c4", "both"):
            clusters = make_clusters(args.clusters, 50, 1500, 0.01, 9, args.seed)
            seq = np.arange(50 * args.clusters, dtype=np.int32)
            results.append(run_case(eng, "c4", clusters, seq, seq // 50, 9, args.warmup, args.repeats, args.sample))
            print(json.dumps(results[-1]), flush=True)
        if args.case in ("long", "both"):
            clusters = make_clusters(1, 64, 10000, 0.01, 72, args.seed + 1)
            seq = (np.arange(args.long_pairs) % 64).astype(np.int32)
            results.append(run_case(eng, "long", clusters, seq, np.zeros_like(seq), 72, args.warmup, args.repeats,
                                    args.sample))
            print(json.dumps(results[-1]), flush=True)
    finally:
        eng.close()
    if args.out:
        old = []
        if os.path.exists(args.out):
            old = [r for r in json.load(open(args.out))["results"] if r["case"] not in {x["case"] for x in results}]
        with open(args.out, "w") as f:
            json.dump({"tool": "scripts/pair_text_timing.py", "device": "MI355X (gfx950)",
                       "results": old + results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
