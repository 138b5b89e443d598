"""Score-only assignment of reads to templates (rf_pair_scores).

R x T grids of forward!(template, read)[end, end] (src/align.jl:155-179)
computed without bands or slots: which reference belongs to a cluster (the
ref-map.tsv the reference's command line asks the user for,
scripts/rifraf.jl:176-189), which consensus a read belongs to, which reads
are outliers.  The scores are bit-identical to the ones the banded fill
returns; only the fold over reads below runs on the host.
"""
from __future__ import annotations

import numpy as np

from .errormodel import ErrorModel, Scores, cap_phreds
from .rifrafsequences import RifrafSequence
from .types import DNASeq


def cross_scores(seqs, templates, bandwidth=None, engine=None, first_seq=0, first_tpl=0,
                 skew_matches=False, trim=False, bandwidth_pvalue=None, return_bandwidths=False,
                 max_doublings=5, carry_counts=False, wide=False):
    """(R, T) matrix of A[end, end] of every RifrafSequence against every
    template, in one engine call.  The sequences are uploaded as ids
    [first_seq, first_seq + R) and the templates as [first_tpl, first_tpl +
    T).  bandwidth=None uses each sequence's own.  bandwidth_pvalue=None
    scores every cell at that bandwidth (rf_pair_scores); a value starts
    there and doubles the band of each cell as smart_forward_moves!
    (model.jl:643-672) does (rf_pair_align_smart, no moves kept), without
    changing the sequences.  carry_counts: with a bandwidth_pvalue, the error
    counts that decide the doubling ride through the fills (rf_pair_errors:
    no move trace, no walk); the results are the same.  return_bandwidths:
    -> (scores, (R, T) int32 bandwidths the cells were scored at).
    wide: bands of more than pairalign.MAX_BAND_ROWS rows are not refused; the
    call runs with the engine's pair_wide option at 1 (the wide tier)."""
    from .align import default_engine
    from .engine import RF_SKEW, RF_TRIM
    from .pairalign import wide_tier
    e = engine or default_engine()
    seqs = list(seqs)
    templates = [DNASeq(t) for t in templates]
    R, T = len(seqs), len(templates)
    if R == 0 or T == 0:
        return (np.empty((R, T)), np.empty((R, T), np.int32)) if return_bandwidths else np.empty((R, T))
    e.set_sequences(first_seq, seqs)
    e.set_templates(first_tpl, templates)
    if bandwidth is None:
        bws = np.array([s.bandwidth for s in seqs], np.int32)[:, None]
    else:
        bws = np.full((R, 1), int(bandwidth), np.int32)
    flags = (RF_SKEW if skew_matches else 0) | (RF_TRIM if trim else 0)
    si, ti = first_seq + np.arange(R)[:, None], first_tpl + np.arange(T)[None, :]
    if bandwidth_pvalue is None:
        with wide_tier(e, wide):
            out = e.pair_scores(si, ti, bws, flags)
        return (out, np.broadcast_to(bws, (R, T)).astype(np.int32)) if return_bandwidths else out
    from .pairalign import MAX_BAND_ROWS, max_bandwidths, smart_inputs
    from .engine import RifrafError
    thr, fixed = smart_inputs(seqs, np.arange(R), bandwidth_pvalue)
    slen = np.array([len(s) for s in seqs], np.int64)[:, None]
    tlen = np.array([len(t) for t in templates], np.int64)[None, :]
    rows = 2 * max_bandwidths(bws, fixed[:, None], slen, tlen, max_doublings) + np.abs(slen - tlen) + 1
    if (rows > MAX_BAND_ROWS).any() and not wide:
        r, j = (int(x[0]) for x in np.nonzero(rows > MAX_BAND_ROWS))
        raise RifrafError(f"sequence {r}, template {j}: band of {int(rows[r, j])} rows at its largest bandwidth is "
                          f"wider than the {MAX_BAND_ROWS} the engine aligns without bands")
    with wide_tier(e, wide):
        if carry_counts:
            sc, _, out_bw, _ = e.pair_errors(si, ti, bws, thr[:, None], fixed=fixed[:, None],
                                             max_doublings=max_doublings, flags=flags)
        else:
            sc, _, _, out_bw, _ = e.pair_align_smart(si, ti, bws, thr[:, None], fixed=fixed[:, None],
                                                     max_doublings=max_doublings, flags=flags, want_moves=False)
    sc, out_bw = sc.reshape(R, T), out_bw.reshape(R, T)
    return (sc, out_bw) if return_bandwidths else sc


def fold_totals(scores) -> np.ndarray:
    """totals[j] = 0.0 + s[0, j] + ... + s[R-1, j]: the sequential left fold
    in read order (model.jl:389-397's order), not a pairwise sum."""
    scores = np.asarray(scores, np.float64)
    totals = np.zeros(scores.shape[1])
    for row in scores:
        totals = totals + row
    return totals


def first_maximum(totals) -> int:
    """Index of the first maximal total (ties go to the earliest)."""
    return int(np.argmax(np.asarray(totals)))


def choose_references(clusters, references, scores=None, bandwidth=9, phred_cap=None, engine=None,
                      bandwidth_pvalue=None, carry_counts=False, wide=False):
    """The reference of each cluster.  clusters: (dnaseqs, phreds) per
    cluster; references: bare base sequences.  Every read (with its Phred
    tables, capped at phred_cap if given) is aligned to every reference as
    the *template*; totals[j] is the left fold of the cluster's scores against
    reference j and the first maximum wins.  bandwidth_pvalue: as in
    cross_scores (None: every cell at `bandwidth`; a value: band doubling
    from there, so a read against a reference it fits badly is not
    under-scored); carry_counts and wide: as in cross_scores.
    -> [(index, totals)]."""
    if scores is None:
        scores = Scores.from_errors(ErrorModel(1.0, 2.0, 2.0))
    out = []
    for dnaseqs, phreds in clusters:
        if phred_cap is not None:
            phreds = [cap_phreds(p, phred_cap) for p in phreds]
        seqs = [RifrafSequence(s, np.asarray(p, np.int8), bandwidth, scores) for s, p in zip(dnaseqs, phreds)]
        totals = fold_totals(cross_scores(seqs, references, bandwidth=bandwidth, engine=engine,
                                           bandwidth_pvalue=bandwidth_pvalue, carry_counts=carry_counts,
                                           wide=wide))
        out.append((first_maximum(totals), totals))
    return out


__all__ = ["cross_scores", "choose_references", "fold_totals", "first_maximum"]
