"""Dense totals of clusters of any depth inside a fixed band budget.

score_proposal's sum over a batch (model.jl:385-399) is a plain left fold in
read order, so it can be cut anywhere and continued exactly
(Engine.score_dense_from).  dense_totals_chunked cuts every cluster's reads
into consecutive chunks whose A and B bands fit a band budget, fills one chunk
per cluster and round into a fixed set of slots, and folds each round into the
running tables: the result has the bits of one realign + score_dense over all
the reads, while only one chunk's bands are ever resident.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .engine import RF_BAND_A, RF_BAND_B, RF_BWD, RF_FWD, Engine


def read_band_bytes(n, m, bw, pad):
    """_lib.host_band_bytes(n, m, bw, pad); pad None: the larger of the padded
    and the unpadded layout (a realign call decides the padding over all its
    jobs, and a padded row can be the shorter one)."""
    if pad is None:
        return max(_lib.host_band_bytes(n, m, bw, False), _lib.host_band_bytes(n, m, bw, True))
    return _lib.host_band_bytes(n, m, bw, pad)


def plan_read_chunks(ns, m, bws, budget_bytes, pad):
    """Cut reads 0..R-1 (ns[k] bases at bandwidth bws[k], template of m) into
    consecutive ranges (start, stop) whose bands fit budget_bytes, by
    read_band_bytes(n, m, bw, pad).  Greedy: each range takes every read that
    still fits, so no range could have taken the next one's first read.  A
    single read over the budget runs alone.  Pure: no engine, no GPU."""
    ns, bws = list(ns), list(bws)
    if len(ns) != len(bws):
        raise ValueError("one bandwidth per read")
    out, start, used = [], 0, 0
    for k, (n, bw) in enumerate(zip(ns, bws)):
        b = read_band_bytes(n, m, bw, pad)
        if k > start and used + b > budget_bytes:
            out.append((start, k))
            start, used = k, 0
        used += b
    if len(ns) > start:
        out.append((start, len(ns)))
    return out


def dense_totals_chunked(seqs_by_cluster, templates, bandwidths=None, band_bytes=1 << 30, references=None,
                         engine=None, stats=None):
    """The dense (m + 1, 9) totals of every cluster, with the bits of one
    realign + score_dense(_ref) over all its reads, inside a band budget.

    seqs_by_cluster: per cluster its RifrafSequences in batch order;
    templates: per cluster its consensus; bandwidths: per cluster one per read
    (None: each sequence's own); band_bytes: the budget for the band arena
    (at least 2 MiB, the smallest arena), what it holds of bands shared out
    evenly over the clusters; references: per cluster a
    RifrafSequence or None, its score added last (filled and passed with the
    cluster's last chunk); engine: an Engine whose sequences, templates and
    bands this call may replace (None: one on device 0, closed afterwards).

    Sequences and templates are uploaded once.  Per round: release_bands(),
    fill the next chunk of every cluster that still has reads into a fixed
    slot set (RF_FWD | RF_BWD), score_dense_from with the running tables; only
    those clusters are in the round's group list.  The band arena is reserved
    once, for the most bands whose arena -- with rf_reserve's guards and
    growth margin -- is no larger than band_bytes (_lib.host_reserve_fit), the
    chunks are planned against that, and the arena never grows past
    band_bytes unless a single read alone is larger than a cluster's share.
    stats: a dict that receives "plans" (per cluster its chunks),
    "round_band_bytes" (per round the capacities of the bands it filled, from
    rf_region_offsets), "fill_ms" and "score_ms" (kernel ms per round).
    Returns (tables, scores): per cluster the (m + 1, 9) table and the
    per-read A[end, end] (rescore!'s host fold takes the latter)."""
    C = len(seqs_by_cluster)
    if len(templates) != C or (references is not None and len(references) != C):
        raise ValueError("one template (and reference entry) per cluster")
    if any(len(s) == 0 for s in seqs_by_cluster):
        raise ValueError("a cluster without reads has no table")
    if bandwidths is None:
        bandwidths = [[s.bandwidth for s in seqs] for seqs in seqs_by_cluster]
    refs = list(references) if references is not None else [None] * C
    own = engine is None
    e = Engine(0) if own else engine
    try:
        # one upload: every cluster's reads, then the references
        first = np.zeros(C + 1, np.int64)
        np.cumsum([len(s) for s in seqs_by_cluster], out=first[1:])
        flat = [s for seqs in seqs_by_cluster for s in seqs]
        ref_seq = {}
        for c, r in enumerate(refs):
            if r is not None:
                ref_seq[c] = len(flat)
                flat.append(r)
        e.set_sequences(0, flat)
        e.set_templates(0, [np.asarray(t, np.uint8) for t in templates])
        # the chunks: each cluster's share of the budget, its reference's bands
        # counted against the last chunk
        pad = None if e.get_option("band_pad") > 0 else False
        fit = _lib.host_reserve_fit(band_bytes)     # what the arena holds when it is no larger than band_bytes
        share = fit // C
        plans = []
        for c in range(C):
            m = len(templates[c])
            room = share
            if refs[c] is not None:    # the reference's bands are resident beside the last chunk
                room -= read_band_bytes(len(refs[c]), m, refs[c].bandwidth, pad)
            plans.append(plan_read_chunks([len(s) for s in seqs_by_cluster[c]], m, bandwidths[c], room, pad))
        e.release_bands()
        e.reserve(fit)
        if stats is not None:
            stats.update(plans=plans, round_band_bytes=[], fill_ms=[], score_ms=[])
        width = [max(b - a for a, b in p) for p in plans]
        slot0 = np.zeros(C + 1, np.int64)
        np.cumsum([w + 1 for w in width], out=slot0[1:])      # the last slot of a cluster: its reference
        tables = [None] * C
        scores = [np.empty(len(s)) for s in seqs_by_cluster]
        rows = [len(t) + 1 for t in templates]
        for rnd in range(max(len(p) for p in plans)):
            live = [c for c in range(C) if rnd < len(plans[c])]
            e.release_bands()
            slots, seqs, tpls, bws, groups, ref_slots = [], [], [], [], [], []
            for c in live:
                a, b = plans[c][rnd]
                sl = np.arange(slot0[c], slot0[c] + (b - a), dtype=np.int32)
                groups.append(sl)
                slots += sl.tolist()
                seqs += range(int(first[c]) + a, int(first[c]) + b)
                tpls += [c] * (b - a)
                bws += [int(x) for x in bandwidths[c][a:b]]
                if refs[c] is not None and rnd == len(plans[c]) - 1:
                    rs = int(slot0[c] + width[c])
                    ref_slots.append(rs)
                    slots.append(rs)
                    seqs.append(ref_seq[c])
                    tpls.append(c)
                    bws.append(int(refs[c].bandwidth))
                else:
                    ref_slots.append(-1)
            got = e.realign(slots, seqs, tpls, bws, RF_FWD | RF_BWD)
            if stats is not None:
                stats["fill_ms"].append(e.last_timing()[0])
                stats["round_band_bytes"].append(sum(e.band_region(s, w)[1] for s in slots
                                                     for w in (RF_BAND_A, RF_BAND_B)))
            at = 0
            for c, sl, rs in zip(live, groups, ref_slots):
                a, b = plans[c][rnd]
                scores[c][a:b] = got[at:at + (b - a)]
                at += (b - a) + (1 if rs >= 0 else 0)
            init = None if rnd == 0 else [tables[c] for c in live]
            out = e.score_dense_from(groups, init, ref_slots if any(r >= 0 for r in ref_slots) else None,
                                     rows=[rows[c] for c in live])
            if stats is not None:
                stats["score_ms"].append(e.last_timing()[1])
            for c, t in zip(live, out):
                tables[c] = np.array(t)
        return tables, scores
    finally:
        if own:
            e.close()


__all__ = ["plan_read_chunks", "dense_totals_chunked", "read_band_bytes"]
