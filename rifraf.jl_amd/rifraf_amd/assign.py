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
                 skew_matches=False, trim=False) -> np.ndarray:
    """(R, T) matrix of A[end, end] of every RifrafSequence against every
    template, in one engine call.  The sequences are uploaded as ids
    [first_seq, first_seq + R) and the templates as [first_tpl, first_tpl +
    T).  bandwidth=None uses each sequence's own."""
    from .align import default_engine
    from .engine import RF_SKEW, RF_TRIM
    e = engine or default_engine()
    seqs = list(seqs)
    templates = [DNASeq(t) for t in templates]
    R, T = len(seqs), len(templates)
    if R == 0 or T == 0:
        return np.empty((R, T))
    e.set_sequences(first_seq, seqs)
    e.set_templates(first_tpl, templates)
    if bandwidth is None:
        bws = np.array([s.bandwidth for s in seqs], np.int32)[:, None]
    else:
        bws = np.full((R, 1), int(bandwidth), np.int32)
    flags = (RF_SKEW if skew_matches else 0) | (RF_TRIM if trim else 0)
    return e.pair_scores(first_seq + np.arange(R)[:, None], first_tpl + np.arange(T)[None, :], bws, flags)


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


def choose_references(clusters, references, scores=None, bandwidth=9, phred_cap=None, engine=None):
    """The reference of each cluster.  clusters: (dnaseqs, phreds) per
    cluster; references: bare base sequences.  Every read (with its Phred
    tables, capped at phred_cap if given) is aligned to every reference as
    the *template*; totals[j] is the left fold of the cluster's scores against
    reference j and the first maximum wins.  -> [(index, totals)]."""
    if scores is None:
        scores = Scores.from_errors(ErrorModel(1.0, 2.0, 2.0))
    out = []
    for dnaseqs, phreds in clusters:
        if phred_cap is not None:
            phreds = [cap_phreds(p, phred_cap) for p in phreds]
        seqs = [RifrafSequence(s, np.asarray(p, np.int8), bandwidth, scores) for s, p in zip(dnaseqs, phreds)]
        totals = fold_totals(cross_scores(seqs, references, bandwidth=bandwidth, engine=engine))
        out.append((first_maximum(totals), totals))
    return out


__all__ = ["cross_scores", "choose_references", "fold_totals", "first_maximum"]
