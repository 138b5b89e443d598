"""Host side of rifraf_amd.assign (no GPU): the fold order and tie rule of
choose_references on hand-written score matrices, and the C-ABI declaration
of the score-only entry points."""
import os
import re

import numpy as np

from rifraf_amd import assign

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "rifraf_hip.h")


def test_fold_is_sequential_in_read_order():
    """0.0 + s_1 + ... + s_R from the left: with 1e16, 1.0, -1e16, 1.0 the
    left fold gives 1.0 (the first 1.0 is absorbed), a pairwise sum 0.0 and
    the exact sum 2.0."""
    col = np.array([1e16, 1.0, -1e16, 1.0])
    scores = np.stack([col, col[::-1], np.array([0.1, 0.2, 0.3, 0.4])], axis=1)
    totals = assign.fold_totals(scores)
    assert totals[0] == 1.0
    assert totals[1] == (((0.0 + 1.0) + -1e16) + 1.0) + 1e16 == 0.0
    assert totals[2] == ((0.0 + 0.1 + 0.2) + 0.3) + 0.4
    assert (col[0] + col[1]) + (col[2] + col[3]) == 0.0   # the pairwise order differs
    assert assign.fold_totals(np.zeros((0, 3))).tolist() == [0.0, 0.0, 0.0]


def test_first_maximum_wins_ties():
    assert assign.first_maximum([-3.0, -1.0, -1.0, -2.0]) == 1
    assert assign.first_maximum([-1.0, -1.0]) == 0
    assert assign.first_maximum([-np.inf, -5.0]) == 1


def test_choose_references_folds_engine_scores(monkeypatch):
    """choose_references = first_maximum(fold_totals(cross_scores)) per
    cluster, with the reads capped and the references as templates."""
    seen = []

    def fake_cross(seqs, templates, bandwidth=None, engine=None, **kw):
        seen.append(([s.phreds_max for s in seqs], len(templates), bandwidth, engine))
        return np.array([[-2.0, -1.0, -1.0]] * len(seqs)) * (1 + len(seen))

    class FakeSeq:
        def __init__(self, seq, phreds, bandwidth, scores):
            self.phreds_max = int(np.max(phreds))
            assert scores.mismatch < 0 and bandwidth == 7

    monkeypatch.setattr(assign, "cross_scores", fake_cross)
    monkeypatch.setattr(assign, "RifrafSequence", FakeSeq)
    reads = [np.array([0, 1, 2], np.uint8)] * 2
    phreds = [np.array([40, 10, 20], np.int8)] * 2
    res = assign.choose_references([(reads, phreds), (reads[:1], phreds[:1])], [b"x"] * 3, bandwidth=7,
                                   phred_cap=30, engine="E")
    assert [i for i, _ in res] == [1, 1]
    assert res[0][1].tolist() == [-8.0, -4.0, -4.0] and res[1][1].tolist() == [-6.0, -3.0, -3.0]
    assert seen == [([30, 30], 3, 7, "E"), ([30], 3, 7, "E")]


def test_header_declares_pair_scores():
    text = open(HEADER).read()
    assert re.search(r"^int rf_pair_scores\(rf_ctx \*ctx, int64_t npairs, const int32_t \*seq, "
                     r"const int32_t \*tpl,\s*const int32_t \*bw, int32_t flags, double \*out\);", text, re.M)
    assert re.search(r"^int rf_last_pair_ms\(const rf_ctx \*ctx, double \*ms\);", text, re.M)
    assert re.search(r"#define RF_ABI_VERSION 1\b", text)
    from rifraf_amd import _lib
    assert "rf_pair_scores" in _lib._SIGNATURES and "rf_last_pair_ms" in _lib._SIGNATURES
    import rifraf_amd
    assert rifraf_amd.cross_scores is assign.cross_scores
    assert rifraf_amd.choose_references is assign.choose_references
