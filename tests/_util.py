"""Shared helpers for the parity tests (engine vs oracle)."""
import numpy as np

from rifraf_amd import ErrorModel, RifrafSequence, Scores
from rifraf_amd.proposals import DEL, INS, SUB
from rifraf_amd.sample import random_seq, sample_from_template

SEQ_SCORES = Scores.from_errors(ErrorModel(1.0, 2.0, 2.0, 0.0, 0.0))      # model.jl:98
REF_SCORES = Scores.from_errors(ErrorModel(10.0, 1e-1, 1e-1, 1.0, 1.0))   # model.jl:99


def make_read(template, rng, error_rate=0.02, bandwidth=9, scores=SEQ_SCORES,
              seq_errors=ErrorModel(1, 5, 5)):
    s, _, ph, _, _ = sample_from_template(template, np.full(len(template), error_rate), seq_errors,
                                          1.5, 1.0, 0.3, rng)
    if len(s) == 0:
        s, ph = template[:1].copy(), np.array([20], np.int8)
    return RifrafSequence(s, ph.astype(np.float64) / -10.0, bandwidth, scores)


def inband_mask(nrows, ncols, bw):
    """(H, ncols) boolean mask of the in-band data entries (row_range)."""
    H = 2 * bw + abs(nrows - ncols) + 1
    h_off = max(ncols - nrows, 0)
    v_off = max(nrows - ncols, 0)
    mask = np.zeros((H, ncols), bool)
    for j in range(1, ncols + 1):
        a = max(1, j - h_off - bw)
        b = min(j + v_off + bw, nrows)
        mask[a - j + h_off + bw: b - j + h_off + bw + 1, j - 1] = True
    return mask


def all_proposals_arrays(template):
    """STAGE_SCORE all_proposals (model.jl:401-456), no seeds, as arrays."""
    m = len(template)
    k, p, b = [INS] * 4, [0] * 4, [0, 1, 2, 3]
    for j in range(1, m + 1):
        for base in range(4):
            if template[j - 1] != base:
                k.append(SUB); p.append(j); b.append(base)
        k.append(DEL); p.append(j); b.append(0)
        for base in range(4):
            k.append(INS); p.append(j); b.append(base)
    return np.array(k, np.uint8), np.array(p, np.int32), np.array(b, np.uint8)


def dense_slot(kind, base):
    return np.where(kind == SUB, base, np.where(kind == DEL, 4, 5 + base))


def tie_template(m, rng, max_run=4):
    """A template of m bases in homopolymer runs of 1..max_run over two
    letters.  -> (bases, run lengths, the letter of each run)."""
    a, b = rng.choice(4, 2, replace=False)
    runs = []
    while sum(runs) < m:
        runs.append(min(int(rng.integers(1, max_run + 1)), m - sum(runs)))
    letters = [a if k % 2 == 0 else b for k in range(len(runs))]
    t = np.concatenate([np.full(r, c, np.uint8) for r, c in zip(runs, letters)])
    return t, runs, letters


def tie_read(runs, letters, n, rng, edits=0, spread=8):
    """A read of n bases made from a template's runs by shortening /
    lengthening runs one base at a time until it has n bases (for n == m one
    run is shortened and another lengthened); then `edits` times one run is
    shortened by 1..3 bases (as far as it has them) and another run lengthened
    by as many, at most `spread` runs away, so that the alignment leaves the
    diagonal by at most three and comes back soon: a lengthening by two puts two
    inserts at one template position, one by three is a codon."""
    m = sum(runs)
    rr = list(runs)
    if n == m and len(rr) > 1:
        k = int(rng.integers(0, len(rr)))
        rr[k] -= 1
        rr[(k + 1) % len(rr)] += 1
    while sum(rr) > n:
        k = int(rng.choice([i for i, r in enumerate(rr) if r > 0]))
        rr[k] -= 1
    while sum(rr) < n:
        rr[int(rng.integers(0, len(rr)))] += 1
    for _ in range(edits):
        k = int(rng.choice([i for i, r in enumerate(rr) if r > 0]))
        d = min(int(rng.integers(1, 4)), rr[k])
        rr[k] -= d
        rr[min(max(k + int(rng.integers(-spread, spread + 1)), 0), len(rr) - 1)] += d
    s = np.concatenate([np.full(r, c, np.uint8) for r, c in zip(rr, letters)])
    assert len(s) == n
    return s


def tie_pair(m, n, rng, max_run=4, edits=0, spread=8):
    """A template of homopolymer runs over two letters, and a read made from
    it by shortening / lengthening runs until it has n bases (for n == m one
    run is shortened and another lengthened): at a constant error_log_p the
    moves of the alignment tie all along the edited runs."""
    t, runs, letters = tie_template(m, rng, max_run)
    assert len(t) == m
    return t, tie_read(runs, letters, n, rng, edits, spread)


def assert_score_launch(engine, kernel=None, mode=None):
    """The engine's last scoring call ran the scorer `kernel` ("general",
    "seg", "ws") in `mode` ("fused", "split"); None: not checked.  The
    scorers and modes compute the same bits, so only this shows the routing."""
    launch = engine.last_score_launch()
    assert launch.items > 0 and launch.grid_y > 0, launch
    if kernel is not None:
        assert launch.kernel == kernel, launch
    if mode is not None:
        assert launch.split == (mode == "split"), launch


__all__ = ["make_read", "inband_mask", "all_proposals_arrays", "dense_slot", "random_seq",
           "SEQ_SCORES", "REF_SCORES", "assert_score_launch", "tie_template", "tie_read", "tie_pair"]
