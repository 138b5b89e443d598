#!/usr/bin/env python3
"""Time candidate selection on the device (rf_candidates) against the host
sequence it replaces -- rf_alignment_proposals (mask download) + the mask
scan + rf_score (list upload, totals download) + the `total > score` filter +
choose_candidates -- on one GPU, at the C-ABI.

  c4     one wave of the c4 shape: --clusters x --reads reads of 1.5 kb at
         bandwidth 9, INIT with alignment proposals (source 1); the consensus
         of a cluster is its first read, as at the start of a run
  frame  one c3-shaped cluster (--frame-reads reads of 2.6 kb) in FRAME: a
         constant-quality codon reference in ref_slot and a seeded
         indel-correction mask (source 4)

Both paths run alternately in this one process: --warmup untimed rounds, then
--repeats timed ones.  Per call: wall time, process CPU time, bytes moved
over PCIe (counted from the arguments each call uploads and downloads) and
the engine's own kernel times.  The host path's scan, filter and sort are
numpy here and C++ in the native driver, so its CPU figure is an upper bound.
Chosen lists must be identical before anything is reported.  Writes --out.

    timeout -k 10 1100 python scripts/candidates_timing.py
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

from pair_scores_timing import make_clusters  # noqa: E402

ORDER = np.array([0, 1, 2, 3, 5, 6, 7, 8, 4])          # model._MASK_ORDER
KIND = np.array([0, 0, 0, 0, 1, 1, 1, 1, 2], np.uint8)
BASE = np.array([0, 1, 2, 3, 0, 1, 2, 3, 0], np.uint8)
ALL_ORDER = np.arange(9)                               # all_proposals: Sub, Del, Ins
ALL_KIND = np.array([0, 0, 0, 0, 2, 1, 1, 1, 1], np.uint8)
ALL_BASE = np.array([0, 1, 2, 3, 0, 0, 1, 2, 3], np.uint8)


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def choose(kind, pos, base, score, min_dist):
    order = np.argsort(-score, kind="stable")
    taken, out = [], []
    for i in order.tolist():
        p = int(pos[i])
        if any(abs(p - q) < min_dist for q in taken):
            continue
        taken.append(p)
        out.append((int(kind[i]), p, int(base[i]), float(score[i])))
    return out


def host_path(eng, groups, refs, rows, scores, min_dist, frame_mask):
    """Today's sequence; returns (chosen per group, PCIe bytes, kernel ms)."""
    G = len(groups)
    moved = 0
    row0 = np.concatenate([[0], np.cumsum(rows)])
    if frame_mask is None:
        masks = eng.alignment_proposals(groups, True)
        moved += sum(m.size for m in masks)
        bt = eng.last_backtrace_ms()
        sel = [np.nonzero(m[:, ORDER]) for m in masks]
        props = [(KIND[c], p.astype(np.int32), BASE[c]) for p, c in sel]
    else:
        bt = 0.0
        sel = [np.nonzero(frame_mask[row0[g]:row0[g + 1]][:, ALL_ORDER]) for g in range(G)]
        props = [(ALL_KIND[c], p.astype(np.int32), ALL_BASE[c]) for p, c in sel]
    tot = eng.score([(groups[g], refs[g], props[g]) for g in range(G)])
    moved += sum(6 * len(p[0]) + 8 * len(p[0]) for p in props)   # kind, pos, base up; totals down
    _, sc, ga = eng.last_timing()
    out = []
    for g in range(G):
        keep = tot[g] > scores[g]
        k, p, b = props[g]
        out.append(choose(k[keep], p[keep], b[keep], tot[g][keep], min_dist))
    return out, moved, bt + sc + ga


def device_path(eng, pg, refs, rows, scores, sources, min_dist, frame_mask, caps):
    masks = None
    if frame_mask is not None:
        row0 = np.concatenate([[0], np.cumsum(rows)])
        masks = [frame_mask[row0[g]:row0[g + 1]] for g in range(len(rows))]
    res = eng.candidates(pg, scores, sources, min_dist, ref_slots=refs if frame_mask is not None else None,
                         masks=masks, cand_cap=False, chosen_cap=caps)
    moved = (0 if frame_mask is None else frame_mask.size) + 8 * len(rows) + 16 * int(sum(caps))
    sel, cho = eng.last_candidates_ms()
    _, sc, _ = eng.last_timing()
    return [[(c.proposal.kind, c.proposal.pos, c.proposal.base, c.score) for c in ch] for _, ch in res], moved, \
        (sel, cho, eng.last_backtrace_ms() if frame_mask is None else 0.0, sc)


def measure(eng, name, groups, refs, rows, scores, sources, min_dist, frame_mask, warmup, repeats):
    from rifraf_amd.engine import pack_groups
    pg = pack_groups(groups)
    caps = [(r - 1) // min_dist + 1 for r in rows]
    rec = {k: [] for k in ("host_wall", "host_cpu", "dev_wall", "dev_cpu", "host_kernel", "sel", "cho", "dev_bt",
                           "dev_score")}
    for it in range(warmup + repeats):
        w0, c0 = time.perf_counter(), time.process_time()
        a, moved_h, hk = host_path(eng, groups, refs, rows, scores, min_dist, frame_mask)
        w1, c1 = time.perf_counter(), time.process_time()
        b, moved_d, (sel, cho, bt, sc) = device_path(eng, pg, refs, rows, scores, sources, min_dist, frame_mask, caps)
        w2, c2 = time.perf_counter(), time.process_time()
        if a != b:
            raise SystemExit(f"{name}: chosen lists differ between the host sequence and rf_candidates")
        if it >= warmup:
            for k, v in zip(rec, (w1 - w0, c1 - c0, w2 - w1, c2 - c1, hk, sel, cho, bt, sc)):
                rec[k].append(v * (1e3 if k.endswith(("wall", "cpu")) else 1.0))
    hw, dw = stats(rec["host_wall"]), stats(rec["dev_wall"])
    spread = max(hw["max"] - hw["min"], dw["max"] - dw["min"])
    return {"case": name, "groups": len(groups), "reads": int(sum(len(g) for g in groups)),
            "template_len_mean": float(np.mean(rows) - 1), "min_dist": min_dist, "warmup": warmup, "repeats": repeats,
            "chosen_identical": True, "chosen_per_group_mean": float(np.mean([len(x) for x in a])),
            "host_path": {"wall_ms": hw, "cpu_ms": stats(rec["host_cpu"]), "pcie_bytes": int(moved_h),
                          "kernel_ms": stats(rec["host_kernel"])},
            "rf_candidates": {"wall_ms": dw, "cpu_ms": stats(rec["dev_cpu"]), "pcie_bytes": int(moved_d),
                              "select_ms": stats(rec["sel"]), "choose_ms": stats(rec["cho"]),
                              "walks_ms": stats(rec["dev_bt"]), "dense_score_ms": stats(rec["dev_score"])},
            "wall_spread_ms": spread, "device_faster_by_more_than_spread": bool(hw["median"] - dw["median"] > spread)}


def c4_case(eng, args):
    from rifraf_amd.engine import RF_BWD, RF_FWD
    clusters = make_clusters(args.clusters, args.reads, 1500, 0.01, 9, 44)
    reads = [r for _, rs in clusters for r in rs]
    for a in range(0, len(reads), 4096):
        eng.set_sequences(a, reads[a:a + 4096])
    eng.set_templates(0, [rs[0].seq for _, rs in clusters])
    n = len(reads)
    slots = np.arange(n, dtype=np.int32)
    tpl = np.repeat(np.arange(args.clusters, dtype=np.int32), args.reads)
    a_end = eng.realign(slots, slots, tpl, np.full(n, 9, np.int32), RF_FWD | RF_BWD)
    groups = [slots[c * args.reads:(c + 1) * args.reads] for c in range(args.clusters)]
    scores = [float(a_end[g].sum()) for g in groups]
    rows = [len(rs[0].seq) + 1 for _, rs in clusters]
    return measure(eng, "c4_init_alignment_proposals", groups, [-1] * len(groups), rows, scores, [1] * len(groups),
                   15, None, args.warmup, args.repeats)


def frame_case(eng, args):
    from rifraf_amd import ErrorModel, RifrafSequence, Scores
    from rifraf_amd.engine import RF_BWD, RF_FWD
    from rifraf_amd.model import Stage, all_proposals
    from rifraf_amd.proposals import Deletion, Insertion
    (t, reads), = make_clusters(1, args.frame_reads, 2601, 0.01, 9, 45)
    cons = np.delete(np.asarray(reads[0].seq, np.uint8), 700)   # a frameshift against the reference
    ref = RifrafSequence(np.asarray(t, np.uint8), np.full(len(t), -1.0), 9,
                         Scores.from_errors(ErrorModel(10.0, 1e-5, 1e-5, 1.0, 1.0)))
    eng.release_bands()
    eng.set_sequences(0, reads + [ref])
    eng.set_templates(0, [cons])
    n = len(reads) + 1
    slots = np.arange(n, dtype=np.int32)
    a_end = eng.realign(slots, slots, 0, [s.bandwidth for s in reads + [ref]], RF_FWD | RF_BWD)
    mask = np.zeros((len(cons) + 1, 9), np.uint8)
    for p in all_proposals(Stage.FRAME, cons, True, [Insertion(700, 0), Deletion(1400)]):
        mask[p.pos, p.base if p.kind == 0 else 4 if p.kind == 2 else 5 + p.base] = 1
    return measure(eng, "c3_frame_seeded_mask", [slots[:-1]], [n - 1], [len(cons) + 1], [float(a_end.sum())], [4],
                   15, mask, args.warmup, args.repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clusters", type=int, default=256)
    ap.add_argument("--reads", type=int, default=50)
    ap.add_argument("--frame-reads", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "candidates_timing.json"))
    args = ap.parse_args()
    from rifraf_amd.engine import Engine
    eng = Engine(0)
    try:
        out = []
        for case in (c4_case, frame_case):
            out.append(case(eng, args))
            print(json.dumps(out[-1]), flush=True)
    finally:
        eng.close()
    with open(args.out, "w") as f:
        json.dump({"cases": out}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
