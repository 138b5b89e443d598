"""Alignments of many pairs in one engine call (rf_pair_align,
rf_pair_align_text), and their error counts alone (rf_pair_errors).

The pairwise half of the reference's API over lists: align_moves / align
(src/align.jl:337-353), edit_distance (:253-260) and the loop of
scripts/correct_shifts.jl (:61-68, correct_shifts model.jl:1303-1316).  The
engine fills each pair with the scores on chip, keeps a 4-bit move per band
cell and walks it: no FP64 band, no slot.  align.py's one-pair functions and
model.correct_shifts keep their slot path; the results are the same.
Where only the gapped texts, the index maps (moves_to_indices, :322-335) or
the band tolerances (:262-284) are wanted, the engine makes them from the
moves on the device (Engine.pair_align_text) and the moves are not downloaded;
an engine without that call gets the moves and align.py's per-move loops.
The same holds for frameshift correction (rf_pair_shifts, Engine.pair_shifts):
correct_shifts_many, single_indel_proposals_many and has_single_indels_many.

A band of more than MAX_BAND_ROWS rows is refused here, before anything is
uploaded, as the engine refuses it.  wide=True on any function of this module
lifts that: the call runs with the engine's pair_wide option at 1
(RF_OPT_PAIR_WIDE: such pairs take the wide tier, its ring in device memory;
every other pair runs as before) and puts the option back afterwards.
"""
from __future__ import annotations

import contextlib
import math

import numpy as np

from .align import band_tolerance, moves_to_aligned_seqs, moves_to_indices
from .engine import RF_SKEW, RF_TRIM, RifrafError
from .errormodel import ErrorModel, Scores
from .poisson import cquantile_poisson_many
from .proposals import AmbiguousProposalsError, Deletion, Insertion, apply_proposals
from .rifrafsequences import RifrafSequence
from .types import DNASeq

MAX_BAND_ROWS = 160 * 1024 // 32 - 6   # DPW_LDS_H: the widest band a bandless pass holds in LDS
BANDWIDTH_PVALUE = 0.1                 # RifrafParams' default bandwidth_pvalue (model.py)


def _engine(engine):
    if engine is not None:
        return engine
    from .align import default_engine
    return default_engine()


@contextlib.contextmanager
def wide_tier(e, wide):
    """The engine's pair_wide option at 1 for the block if `wide`, and its
    previous value afterwards, also when the block raises."""
    if not wide:
        yield
        return
    old = e.set_option("pair_wide", 1)
    try:
        yield
    finally:
        e.set_option("pair_wide", old)


def _pairs(pairs, nseq, ntpl):
    if pairs is None:
        if nseq != ntpl:
            raise ValueError(f"{nseq} sequences and {ntpl} templates: give pairs=(sequence, template) indices")
        k = np.arange(nseq, dtype=np.int64)
        return k, k
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    if len(pairs) and (pairs.min() < 0 or pairs[:, 0].max() >= nseq or pairs[:, 1].max() >= ntpl):
        raise ValueError("pairs: index out of range")
    return pairs[:, 0], pairs[:, 1]


def max_bandwidths(bws, fixed, slen, tlen, max_doublings):
    """smart_forward_moves!' max_bandwidth (model.jl:648-651) per pair."""
    bws = np.asarray(bws, np.int64)
    grown = np.minimum(np.minimum(bws << int(max_doublings), tlen), slen)
    return np.where(np.asarray(fixed, bool), bws, grown)


def _upload(e, seqs, templates, si, ti, bws, smart, wide=False):
    """Checks the band every pair (si[k], ti[k]) needs -- with smart =
    (thresholds, fixed, max_doublings) the one at the largest bandwidth it can
    reach; not with `wide`, where the engine's own limits hold -- and uploads
    sequences and templates as ids 0.. of the engine.
    -> (sequence lengths, template lengths)."""
    slen = np.array([len(s) for s in seqs], np.int64)
    tlen = np.array([len(t) for t in templates], np.int64)
    top = bws if smart is None else max_bandwidths(bws, smart[1], slen[si], tlen[ti], smart[2])
    rows = 2 * top + np.abs(slen[si] - tlen[ti]) + 1
    over = np.nonzero(rows > MAX_BAND_ROWS)[0]
    if len(over) and not wide:
        k = int(over[0])
        at = "" if smart is None else f" at its largest bandwidth {int(top[k])}"
        raise RifrafError(f"pair {k} (sequence {int(si[k])}, template {int(ti[k])}): band of {int(rows[k])} rows"
                          f"{at} is wider than the {MAX_BAND_ROWS} the engine aligns without bands")
    e.set_sequences(0, seqs)
    e.set_templates(0, templates)
    return slen, tlen


def _run(e, seqs, templates, si, ti, bws, flags, want_moves, smart=None, text=None, wide=False):
    """One rf_pair_align call over pairs (si[k], ti[k]); sequences and
    templates are uploaded as ids 0.. of the engine.  smart = (thresholds,
    fixed, max_doublings): one rf_pair_align_smart call, and the band that
    must fit is the one at the largest bandwidth a pair can reach.  text =
    (want_text, want_indices, want_tolerance): one rf_pair_align_text call
    instead (len(si) > 0) -> (scores, engine.PairText)."""
    if len(si) == 0:
        empty = (np.empty(0), ([] if want_moves else None), np.empty(0, np.int32))
        return empty if smart is None else empty + (np.empty(0, np.int32), np.empty(0, np.int32))
    bws = np.broadcast_to(np.asarray(bws, np.int64), si.shape)
    slen, tlen = _upload(e, seqs, templates, si, ti, bws, smart, wide)
    with wide_tier(e, wide):
        return _run_call(e, si, ti, bws, flags, want_moves, smart, text, slen, tlen)


def _run_call(e, si, ti, bws, flags, want_moves, smart, text, slen, tlen):
    """_run's engine call."""
    if text is not None:
        thr, fixed, md = smart if smart is not None else (None, None, 0)
        return e.pair_align_text(si, ti, bws, thr, fixed=fixed, max_doublings=md, flags=flags, want_text=text[0],
                                 want_indices=text[1], want_tolerance=text[2], caps=(slen[si] + tlen[ti], tlen[ti]))
    if smart is None:
        return e.pair_align(si, ti, bws, flags, want_moves=want_moves, caps=slen[si] + tlen[ti])
    return e.pair_align_smart(si, ti, bws, smart[0], fixed=smart[1], max_doublings=smart[2], flags=flags,
                              want_moves=want_moves, caps=slen[si] + tlen[ti])


def align_moves_many(seqs, templates, pairs=None, bandwidth=None, skew_matches=False, trim=False, engine=None,
                     wide=False):
    """align_moves(templates[j], seqs[i]) (align.jl:337-344) for every (i, j)
    of `pairs` ((N, 2) indices; default k with k), in one engine call.
    bandwidth=None uses each sequence's own.  -> list of int8 move arrays in
    alignment order; None for a pair the reference raises on."""
    seqs = list(seqs)
    templates = [DNASeq(t) for t in templates]
    si, ti = _pairs(pairs, len(seqs), len(templates))
    if bandwidth is None:
        bws = np.array([s.bandwidth for s in seqs], np.int64)[si]
    else:
        bws = np.full(si.shape, int(bandwidth), np.int64)
    flags = (RF_SKEW if skew_matches else 0) | (RF_TRIM if trim else 0)
    _, moves, _ = _run(_engine(engine), seqs, templates, si, ti, bws, flags, True, wide=wide)
    return moves


def _products(seqs, templates, pairs, bandwidth, skew_matches, trim, engine, smart, text, wide=False):
    """The products text = (texts, indices, tolerances) of every pair, from
    one engine call: pair_align_text where the engine has it, else the moves
    and align.py's host functions.  smart: None, or (pvalue, max_doublings).
    -> ({"text": [...], "indices": [...], "tolerance": int32 array} of those
    asked for, final bandwidths); None / -1 for a pair the reference raises on."""
    seqs = list(seqs)
    templates = [DNASeq(t) for t in templates]
    si, ti = _pairs(pairs, len(seqs), len(templates))
    if bandwidth is None:
        bws = np.array([s.bandwidth for s in seqs], np.int64)[si]
    else:
        bws = np.full(si.shape, int(bandwidth), np.int64)
    if smart is not None:
        smart = smart_inputs(seqs, si, smart[0]) + (smart[1],)
    flags = (RF_SKEW if skew_matches else 0) | (RF_TRIM if trim else 0)
    e = _engine(engine)
    out = {}
    if len(si) and hasattr(e, "pair_align_text"):
        _, r = _run(e, seqs, templates, si, ti, bws, flags, False, smart=smart, text=text, wide=wide)
        if text[0]:
            out["text"] = r.texts()
        if text[1]:
            out["indices"] = [r.indices(k) for k in range(r.n)]
        if text[2]:
            out["tolerance"] = r.tolerance.copy()
        return out, r.bandwidths.copy()
    res = _run(e, seqs, templates, si, ti, bws, flags, True, smart=smart, wide=wide)
    moves, out_bw = res[1], (res[3] if smart is not None else bws.astype(np.int32))
    if text[0]:
        out["text"] = [None if mv is None else moves_to_aligned_seqs(mv, templates[int(j)], seqs[int(i)].seq)
                       for mv, i, j in zip(moves, si, ti)]
    if text[1]:
        out["indices"] = [None if mv is None else
                          np.array(moves_to_indices(mv, len(templates[int(j)]), len(seqs[int(i)])), np.int32)
                          for mv, i, j in zip(moves, si, ti)]
    if text[2]:
        out["tolerance"] = np.array([-1 if mv is None else
                                     band_tolerance(mv, len(seqs[int(i)]) + 1, len(templates[int(j)]) + 1, int(b))
                                     for mv, i, j, b in zip(moves, si, ti, out_bw)], np.int32)
    return out, out_bw


def align_many(seqs, templates, pairs=None, bandwidth=None, skew_matches=False, trim=False, engine=None, wide=False):
    """align (align.jl:346-353) per pair -> [(aligned t, aligned s)] with '-'
    gaps; None for a pair the reference raises on."""
    out, _ = _products(seqs, templates, pairs, bandwidth, skew_matches, trim, engine, None, (True, False, False),
                       wide)
    return out["text"]


def smart_inputs(seqs, si, pvalue):
    """(thresholds, fixed) of pairs whose sequences are seqs[si]: the
    cquantile(Poisson(est_n_errors), pvalue) of model.jl:661 and each
    sequence's bandwidth_fixed."""
    thr = np.asarray(cquantile_poisson_many([s.est_n_errors for s in seqs], pvalue), np.float64)
    fixed = np.array([bool(s.bandwidth_fixed) for s in seqs], bool)
    return thr[si], fixed[si]


def smart_align_moves_many(seqs, templates, pairs=None, pvalue=BANDWIDTH_PVALUE, max_doublings=5, bandwidth=None,
                           skew_matches=False, trim=False, engine=None, wide=False):
    """align_moves_many with smart_forward_moves!' band doubling
    (model.jl:643-672) per pair, in one engine call: the bandwidth (each
    sequence's own, or `bandwidth`) is where a pair starts.  The
    RifrafSequences are not changed -- one sequence may be in many pairs --
    so the bandwidths the pairs ended at are returned.
    -> (moves as align_moves_many's, int32 bandwidths)."""
    seqs = list(seqs)
    templates = [DNASeq(t) for t in templates]
    si, ti = _pairs(pairs, len(seqs), len(templates))
    if bandwidth is None:
        bws = np.array([s.bandwidth for s in seqs], np.int64)[si]
    else:
        bws = np.full(si.shape, int(bandwidth), np.int64)
    thr, fixed = smart_inputs(seqs, si, pvalue)
    flags = (RF_SKEW if skew_matches else 0) | (RF_TRIM if trim else 0)
    _, moves, _, out_bw, _ = _run(_engine(engine), seqs, templates, si, ti, bws, flags, True,
                                  smart=(thr, fixed, max_doublings), wide=wide)
    return moves, out_bw


def _count_inputs(seqs, templates, pairs, bandwidth):
    """The uploaded lists, the pair indices and the starting bandwidths of a
    counting call, built as smart_align_moves_many builds them."""
    seqs = list(seqs)
    templates = [DNASeq(t) for t in templates]
    si, ti = _pairs(pairs, len(seqs), len(templates))
    if bandwidth is None:
        bws = np.array([s.bandwidth for s in seqs], np.int64)[si]
    else:
        bws = np.full(si.shape, int(bandwidth), np.int64)
    return seqs, templates, si, ti, bws


def _errors(e, seqs, templates, si, ti, bws, flags, smart, wide=False):
    """One rf_pair_errors call over pairs (si[k], ti[k]).  smart: None or (thresholds, fixed, max_doublings).
    -> (scores, nerrors, bandwidths)."""
    if len(si) == 0:
        return np.empty(0), np.empty(0, np.int32), np.empty(0, np.int32)
    _upload(e, seqs, templates, si, ti, bws, smart, wide)
    thr, fixed, md = smart if smart is not None else (None, None, 0)
    with wide_tier(e, wide):
        sc, nerr, out_bw, _ = e.pair_errors(si, ti, bws, thr, fixed=fixed, max_doublings=md, flags=flags)
    return sc, nerr, out_bw


def count_errors_many(seqs, templates, pairs=None, bandwidth=None, skew_matches=True, engine=None, wide=False):
    """count_errors(templates[j], seqs[i]) (align.jl:247-250: the skewed
    alignment's count) for every (i, j) of `pairs`, in one engine call that
    keeps no moves (rf_pair_errors).  Arguments as align_moves_many's.
    -> int32 array; -1 for a pair the reference raises on."""
    seqs, templates, si, ti, bws = _count_inputs(seqs, templates, pairs, bandwidth)
    flags = RF_SKEW if skew_matches else 0
    return _errors(_engine(engine), seqs, templates, si, ti, bws, flags, None, wide)[1]


def smart_bandwidths_many(seqs, templates, pairs=None, pvalue=BANDWIDTH_PVALUE, max_doublings=5, bandwidth=None,
                          engine=None, wide=False):
    """The bandwidth smart_forward_moves! (model.jl:643-672) ends at for every
    pair, with the error count and the score of its last fill, in one engine
    call that keeps no moves (rf_pair_errors): the numbers of
    smart_align_moves_many for the same arguments.  The RifrafSequences are
    not changed.  -> (int32 bandwidths, int32 nerrors, scores)."""
    seqs, templates, si, ti, bws = _count_inputs(seqs, templates, pairs, bandwidth)
    thr, fixed = smart_inputs(seqs, si, pvalue)
    sc, nerr, out_bw = _errors(_engine(engine), seqs, templates, si, ti, bws, 0, (thr, fixed, max_doublings), wide)
    return out_bw, nerr, sc


def smart_align_many(seqs, templates, pairs=None, pvalue=BANDWIDTH_PVALUE, max_doublings=5, bandwidth=None,
                     skew_matches=False, trim=False, engine=None, wide=False):
    """align_many with smart_align_moves_many's band doubling
    -> ([(aligned t, aligned s)] with None for a pair the reference raises
    on, int32 bandwidths)."""
    out, out_bw = _products(seqs, templates, pairs, bandwidth, skew_matches, trim, engine, (pvalue, max_doublings),
                            (True, False, False), wide)
    return out["text"], out_bw


def align_indices_many(seqs, templates, pairs=None, pvalue=BANDWIDTH_PVALUE, max_doublings=0, bandwidth=None,
                       skew_matches=False, trim=False, engine=None, wide=False):
    """moves_to_indices (align.jl:322-335) of every pair's alignment: for
    each move that advances in the template, the 1-based sequence position
    reached (0 before the first sequence base).  A codon deletion covers
    three template bases with one entry, as in the reference.  max_doublings
    > 0 aligns with smart_align_many's band doubling, 0 (default) at the
    given bandwidth like align_many.  One engine call.
    -> list of int32 arrays; None for a pair the reference raises on."""
    out, _ = _products(seqs, templates, pairs, bandwidth, skew_matches, trim, engine,
                       (pvalue, max_doublings) if max_doublings else None, (False, True, False), wide)
    return out["indices"]


def band_tolerances(seqs, templates, pairs=None, pvalue=BANDWIDTH_PVALUE, max_doublings=0, bandwidth=None,
                    skew_matches=False, trim=False, engine=None, wide=False):
    """band_tolerance (align.jl:262-284) of every pair's alignment in the band
    of its last fill: how close the path comes to a band edge that is not the
    matrix's (len(seq) + 1 if the band is never such an edge).  Arguments as
    align_indices_many's.  One engine call.
    -> int32 array; -1 for a pair the reference raises on."""
    out, _ = _products(seqs, templates, pairs, bandwidth, skew_matches, trim, engine,
                       (pvalue, max_doublings) if max_doublings else None, (False, False, True), wide)
    return out["tolerance"]


def edit_distances(templates, seqs, engine=None, wide=False) -> np.ndarray:
    """edit_distance(templates[k], seqs[k]) (align.jl:253-260) for bare base
    sequences: log p = -1, ErrorModel(1, 1, 1), bandwidth ceil(min(m, n) / 2),
    skewed alignment, count_errors.  One engine call."""
    templates = [DNASeq(t) for t in templates]
    seqs = [DNASeq(s) for s in seqs]
    if len(templates) != len(seqs):
        raise ValueError("edit_distances: one template per sequence")
    scores = Scores.from_errors(ErrorModel(1.0, 1.0, 1.0))
    rs, bws = [], []
    for t, s in zip(templates, seqs):
        bw = int(math.ceil(min(len(t), len(s)) * 0.5))
        rs.append(RifrafSequence(s, np.full(len(s), -1.0), bw, scores))
        bws.append(bw)
    k = np.arange(len(seqs), dtype=np.int64)
    _, _, nerr = _run(_engine(engine), rs, templates, k, k, np.array(bws, np.int64), RF_SKEW, False, wide=wide)
    return nerr


def calibrate_phreds_many(seqs, phreds, consensus, engine=None) -> list:
    """calibrate_phreds (model.jl:1295-1300) of every read against one
    consensus: the error probabilities of its Phred values, scaled so that
    they sum to edit_distance(consensus, read).  The distances come from one
    rf_pair_errors call (edit_distance's sequences and bandwidths, RF_SKEW, no
    doubling; bands of any width, in the wide tier where they need it); the
    scaling is model.calibrate_phreds' on the host.
    -> one float64 array per read."""
    from .errormodel import phred_to_log_p
    seqs = [DNASeq(s) for s in seqs]
    phreds = list(phreds)
    if len(seqs) != len(phreds):
        raise ValueError("calibrate_phreds_many: one Phred array per sequence")
    consensus = DNASeq(consensus)
    if not seqs:
        return []
    scores = Scores.from_errors(ErrorModel(1.0, 1.0, 1.0))
    bws = np.array([int(math.ceil(min(len(consensus), len(s)) * 0.5)) for s in seqs], np.int64)
    rs = [RifrafSequence(s, np.full(len(s), -1.0), int(bw), scores) for s, bw in zip(seqs, bws)]
    si = np.arange(len(seqs), dtype=np.int64)
    _, nerr, _ = _errors(_engine(engine), rs, [consensus], si, np.zeros(len(seqs), np.int64), bws, RF_SKEW, None, True)
    out = []
    for k, phred in enumerate(phreds):
        if nerr[k] < 0:
            raise RifrafError(f"sequence {k}: new score is invalid")
        errors = np.power(10.0, phred_to_log_p(phred))
        out.append(errors * float(nerr[k]) / errors.sum())
    return out


def _single_indels(moves, refseq):
    """single_indel_proposals' walk (model.jl:538-562) over one move list."""
    out = []
    cons_idx = ref_idx = 0
    for mv in moves.tolist():
        if mv == 1:
            cons_idx += 1
            ref_idx += 1
        elif mv == 2:
            ref_idx += 1
            out.append(Insertion(cons_idx, int(refseq[ref_idx - 1])))
        elif mv == 3:
            cons_idx += 1
            out.append(Deletion(cons_idx))
        elif mv == 4:
            ref_idx += 3
        elif mv == 5:
            cons_idx += 3
    return out


def _shift_lists(fn, consensuses, references):
    """The consensuses and their references -- one for all (a list of one),
    or one per consensus -- as base arrays."""
    consensuses = [DNASeq(c) for c in consensuses]
    if isinstance(references, str) or (isinstance(references, np.ndarray) and references.ndim == 1):
        references = [references]
    references = [DNASeq(r) for r in references]
    if len(references) != 1 and len(references) != len(consensuses):
        raise ValueError(f"{fn}: one reference, or one per consensus")
    return consensuses, references


def _shift_moves(e, consensuses, references, log_p, bandwidth, scores, wide=False):
    """The skewed codon alignment of every consensus (template) against its
    reference (sequence) through pair_align: one RifrafSequence per pair,
    and the moves come to the host.  -> (sequences, moves), None for a
    failed pair's."""
    if len(references) == 1:
        references = references * len(consensuses)
    rs = []
    for c, r in zip(consensuses, references):
        bw = bandwidth if bandwidth >= 0 else int(math.ceil(min(len(c), len(r)) * 0.1))
        rs.append(RifrafSequence(r, np.full(len(r), log_p), bw, scores))
    k = np.arange(len(consensuses), dtype=np.int64)
    bws = np.array([s.bandwidth for s in rs], np.int64)
    _, moves, _ = _run(e, rs, consensuses, k, k, bws, RF_SKEW, True, wide=wide)
    return rs, moves


def _moves_or_raise(i, mv):
    if mv is None:
        raise RifrafError(f"pair {i}: new score is invalid")
    return mv


def _shifts(e, consensuses, seqs, si, bws, flags, want_fixed, want_proposals, wide=False):
    """One rf_pair_shifts call over the pairs (sequence seqs[si[k]], template
    consensuses[k]); a sequence that many pairs share is uploaded once.
    -> _lib.PairShifts."""
    ti = np.arange(len(consensuses), dtype=np.int64)
    slen, tlen = _upload(e, seqs, consensuses, si, ti, bws, None, wide)
    with wide_tier(e, wide):
        _, r = e.pair_shifts(si, ti, bws, flags, want_fixed=want_fixed, want_proposals=want_proposals,
                             caps=slen[si] + tlen[ti])
    return r


def _shift_sequences(consensuses, references, log_p, bandwidth, scores):
    """correct_shifts' sequences and bandwidths for rf_pair_shifts: the
    bandwidth of a pair travels beside it, so one reference is one sequence
    however many consensuses it meets.  -> (sequences, si, bws)."""
    n = len(consensuses)
    si = np.zeros(n, np.int64) if len(references) == 1 else np.arange(n, dtype=np.int64)
    bws = np.array([bandwidth if bandwidth >= 0 else int(math.ceil(min(len(c), len(references[int(i)])) * 0.1))
                    for c, i in zip(consensuses, si)], np.int64)
    # a RifrafSequence wants a bandwidth of its own; the call does not read it
    own = [int(bws.min())] if len(references) == 1 else bws.tolist()
    rs = [RifrafSequence(r, np.full(len(r), log_p), int(b), scores) for r, b in zip(references, own)]
    return rs, si, bws


def _raise_failed(r, ambiguous):
    """correct_shifts_many's exception for the first pair in order that has one."""
    bad = (r.fixed_len == -1) | (r.nprops == -1)
    if ambiguous:
        bad = bad | (r.fixed_len == -2)
    if bad.any():
        i = int(np.argmax(bad))
        if r.nprops[i] == -1:
            raise RifrafError(f"pair {i}: new score is invalid")
        raise AmbiguousProposalsError()


def correct_shifts_many(consensuses, references, log_p=-1.0, bandwidth=-1, scores=None, engine=None, wide=False):
    """correct_shifts (model.jl:1303-1316) of every consensus against its
    reference -- one reference for all, or one per consensus -- as the loop
    of scripts/correct_shifts.jl:61-68 does, in one engine call: the skewed
    codon alignment of single_indel_proposals (the reference is the
    sequence, the consensus the template), then apply_proposals.  The engine
    makes the corrected consensuses from the moves on the device
    (Engine.pair_shifts) and the moves are not downloaded; an engine without
    that call gets the moves and the per-move loop."""
    scores = scores or Scores.from_errors(ErrorModel(10.0, 1e-5, 1e-5, 1.0, 1.0))
    consensuses, references = _shift_lists("correct_shifts_many", consensuses, references)
    e = _engine(engine)
    if not consensuses:
        return []
    if not hasattr(e, "pair_shifts"):
        rs, moves = _shift_moves(e, consensuses, references, log_p, bandwidth, scores, wide)
        return [apply_proposals(c, _single_indels(_moves_or_raise(i, mv), s.seq))
                for i, (c, s, mv) in enumerate(zip(consensuses, rs, moves))]
    rs, si, bws = _shift_sequences(consensuses, references, log_p, bandwidth, scores)
    r = _shifts(e, consensuses, rs, si, bws, RF_SKEW, True, False, wide)
    _raise_failed(r, True)
    return [r.fixed_seq(k) for k in range(r.n)]


def single_indel_proposals_many(consensuses, references, log_p=-1.0, bandwidth=-1, scores=None, engine=None,
                                wide=False):
    """single_indel_proposals (model.jl:538-562) of every consensus against
    its reference: the Insertion / Deletion proposals that correct_shifts_many
    applies, in move order, from the same alignment and with the same
    arguments.  One engine call.  -> list of proposal lists."""
    scores = scores or Scores.from_errors(ErrorModel(10.0, 1e-5, 1e-5, 1.0, 1.0))
    consensuses, references = _shift_lists("single_indel_proposals_many", consensuses, references)
    e = _engine(engine)
    if not consensuses:
        return []
    if not hasattr(e, "pair_shifts"):
        rs, moves = _shift_moves(e, consensuses, references, log_p, bandwidth, scores, wide)
        return [_single_indels(_moves_or_raise(i, mv), s.seq) for i, (s, mv) in enumerate(zip(rs, moves))]
    rs, si, bws = _shift_sequences(consensuses, references, log_p, bandwidth, scores)
    r = _shifts(e, consensuses, rs, si, bws, RF_SKEW, False, True, wide)
    _raise_failed(r, False)
    return [r.proposals(k) for k in range(r.n)]


def has_single_indels_many(consensuses, refseqs, bandwidth=None, engine=None, wide=False):
    """has_single_indels (model.jl:532-536) of every consensus against its
    reference, a RifrafSequence -- one for all, or one per consensus: does
    the unskewed alignment (model.jl:534) hold a single insertion or
    deletion?  bandwidth=None uses each reference's own.  One engine call.
    -> bool array."""
    consensuses = [DNASeq(c) for c in consensuses]
    refseqs = [refseqs] if isinstance(refseqs, RifrafSequence) else list(refseqs)
    if len(refseqs) != 1 and len(refseqs) != len(consensuses):
        raise ValueError("has_single_indels_many: one reference, or one per consensus")
    n = len(consensuses)
    if n == 0:
        return np.zeros(0, bool)
    si = np.zeros(n, np.int64) if len(refseqs) == 1 else np.arange(n, dtype=np.int64)
    if bandwidth is None:
        bws = np.array([s.bandwidth for s in refseqs], np.int64)[si]
    else:
        bws = np.full(n, int(bandwidth), np.int64)
    e = _engine(engine)
    if not hasattr(e, "pair_shifts"):
        _, moves, _ = _run(e, refseqs, consensuses, si, np.arange(n, dtype=np.int64), bws, 0, True, wide=wide)
        return np.array([bool(((_moves_or_raise(i, mv) == 2) | (mv == 3)).any()) for i, mv in enumerate(moves)], bool)
    r = _shifts(e, consensuses, refseqs, si, bws, 0, False, False, wide)
    _raise_failed(r, False)
    return r.has_single_indels()


__all__ = ["align_moves_many", "align_many", "smart_align_moves_many", "smart_align_many", "align_indices_many",
           "band_tolerances", "edit_distances", "correct_shifts_many", "single_indel_proposals_many",
           "has_single_indels_many", "count_errors_many", "smart_bandwidths_many", "calibrate_phreds_many",
           "MAX_BAND_ROWS"]
