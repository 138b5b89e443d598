"""The sequence uploads on the GPU (DESIGN.md §4 "Sequence uploads"): a refused
upload changes nothing, by either path and by the codes path's full
dictionary, and both paths stage an upload in several chunks to the same
tables.  Bit-exact against the CPU oracle and between the paths."""
import numpy as np
import pytest

import oracle
from _util import SEQ_SCORES, inband_mask, make_read, random_seq
from rifraf_amd import RifrafSequence, _lib
from rifraf_amd.engine import RF_BAND_A, RF_BAND_B, RF_BWD, RF_FWD, Engine
from rifraf_amd.errormodel import phred_to_log_p

pytestmark = pytest.mark.gpu
ptr = _lib.ptr
RF_ERR_ARG, RF_ERR_STATE = -1, -4


def code_tables():
    """lp, 10^lp, match per Phred code and the logsumexp grid (RifrafSequence.many_coded's)."""
    lp_t = phred_to_log_p(np.arange(256, dtype=np.uint8).view(np.int8))
    p10_t = np.power(10.0, lp_t)
    with np.errstate(divide="ignore", invalid="ignore"):
        match_t = np.log10(1.0 - p10_t)
        grid = np.ascontiguousarray(np.power(10.0, match_t[None, :] - match_t[:, None]))
    return lp_t, p10_t, match_t, grid


def assert_band_equal(got, exp_data, nrows, ncols, bw):
    mask = inband_mask(nrows, ncols, bw)
    g, x = got.data[mask], np.asarray(exp_data)[mask]
    bad = ~((g == x) | (np.isnan(g) & np.isnan(x)))
    assert not bad.any(), f"{bad.sum()} of {mask.sum()} in-band cells differ"


def check_bands(e, t, reads, slots, bw):
    """A and B bands of the slots against the oracle for `reads`."""
    for s, r in zip(slots, reads):
        assert_band_equal(e.download_band(s, RF_BAND_A), oracle.forward(t, r)[0], len(r) + 1, len(t) + 1, bw)
        assert_band_equal(e.download_band(s, RF_BAND_B), oracle.backward(t, r), len(r) + 1, len(t) + 1, bw)


@pytest.mark.parametrize("own", [False, True], ids=["others_coded", "would_reset"])
@pytest.mark.parametrize("path", ["tables", "codes"])
def test_refused_upload_changes_nothing(engine, path, own):
    """rf_set_sequences with a cins length of n - 3 on its second sequence, and
    rf_set_sequences_codes with an empty sequence in the middle, return
    RF_ERR_ARG and leave everything as it was: the bands filled from the named
    ids are still scored and walked to the same values, rf_code_stats is
    unchanged, and the ids still realign to the oracle.  others_coded: a
    fourth coded read stays valid on the session engine; would_reset: on an
    engine of its own the three ids are all there is, so an accepted call
    would have started a fresh dictionary."""
    e = Engine(0) if own else engine
    try:
        rng = np.random.default_rng(4040)
        t = random_seq(40, rng)
        reads = [make_read(t, rng, 0.05, 5) for _ in range(4)]
        sl, bw = np.arange(3), [5] * 3
        e.set_templates(0, [t])
        e.set_sequences(0, reads[:3] if own else reads)
        e.realign(sl, sl, 0, bw, RF_FWD | RF_BWD)
        dense = e.score_dense([sl])[0].copy()
        moves, nerr = e.backtrace(sl)
        stats = e.code_stats()
        lens = np.array([len(r) for r in reads[:3]], np.int64)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        bases = np.ascontiguousarray(np.concatenate([r.seq for r in reads[:3]]), np.uint8)
        if path == "tables":
            f = lambda name: np.ascontiguousarray(np.concatenate([getattr(r, name) for r in reads[:3]]))   # noqa: E731
            tabs = [f("match_scores"), f("mismatch_scores"), f("ins_scores"), f("del_scores")]
            cins_off = np.concatenate([[0], np.cumsum(lens - [2, 3, 2])]).astype(np.int64)
            cins = np.zeros(int(cins_off[-1]) + 1)
            rc = e.lib.rf_set_sequences(e.ctx, 0, 3, ptr(bases), ptr(off), *(ptr(a) for a in tabs), ptr(cins),
                                        ptr(cins_off), None, None)
            why = "inconsistent table lengths"
        else:
            lp_t, _, match_t, _ = code_tables()
            off[2] = off[1]                        # the middle sequence is empty
            codes = rng.integers(5, 45, len(bases)).astype(np.uint8)
            rc = e.lib.rf_set_sequences_codes(e.ctx, 0, 3, ptr(bases), ptr(off), ptr(codes), ptr(lp_t), ptr(match_t),
                                              float(SEQ_SCORES.mismatch), float(SEQ_SCORES.insertion),
                                              float(SEQ_SCORES.deletion))
            why = "empty sequence"
        assert rc == RF_ERR_ARG and why in e.lib.rf_last_error(e.ctx).decode()
        np.testing.assert_array_equal(e.score_dense([sl])[0], dense)
        moves2, nerr2 = e.backtrace(sl)
        for a, b in zip(moves, moves2):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(nerr, nerr2)
        assert e.code_stats() == stats
        e.realign(sl, sl, 0, bw, RF_FWD | RF_BWD)
        check_bands(e, t, reads[:3], sl, 5)
        np.testing.assert_array_equal(e.score_dense([sl])[0], dense)
    finally:
        if own:
            e.close()


def test_codes_upload_refused_by_full_dictionary():
    """67 reads x 1000 positions of continuous log probabilities fill the
    dictionary.  rf_set_sequences_codes of new Phreds for a read whose bands
    are filled then returns RF_ERR_STATE and changes nothing: rf_code_stats is
    as before and the read's bands still equal the oracle's for the old read;
    the tables upload the caller falls back to succeeds."""
    rng = np.random.default_rng(6767)
    L, bw = 1000, 9
    t = random_seq(L, rng)
    full = []
    for _ in range(67):
        r = make_read(t, rng, 0.01, bw)
        full.append(RifrafSequence(r.seq, -rng.uniform(0.5, 3.0, len(r.seq)), bw, SEQ_SCORES))
    old = make_read(t, rng, 0.01, bw)
    nb = old.seq.copy()
    nb[500:504] = (nb[500:504] + 1) % 4
    nph = rng.integers(8, 40, len(nb)).astype(np.int8)
    new = RifrafSequence(nb, nph, bw, SEQ_SCORES)
    lp_t, _, match_t, _ = code_tables()
    e = Engine(0)
    try:
        e.set_templates(0, [t])
        e.set_sequences(0, full)
        assert e.code_stats()["entries3"] == _lib.RF_CODES
        e.set_sequences(67, [old])
        e.realign([0], [67], 0, [bw], RF_FWD | RF_BWD)
        stats = e.code_stats()
        assert e.set_sequences_codes(67, nb, np.array([0, len(nb)], np.int64), nph.view(np.uint8), lp_t, match_t,
                                     SEQ_SCORES) is False
        assert "row-code dictionary full" in e.lib.rf_last_error(e.ctx).decode()
        assert e.code_stats() == stats
        e.score_dense([np.array([0])])                      # not stale: the refusal kept the read's version
        e.backtrace([0])
        check_bands(e, t, [old], [0], bw)
        e.realign([0], [67], 0, [bw], RF_FWD | RF_BWD)
        check_bands(e, t, [old], [0], bw)
        e.set_sequences(67, [new])
        e.realign([0], [67], 0, [bw], RF_FWD | RF_BWD)
        check_bands(e, t, [new], [0], bw)
    finally:
        e.close()


def test_both_paths_over_several_chunks(engine, opts):
    """40 reads of 300 bases, one of 600,000 and three of 300 at 16 KB of
    staging: the tables path stages them in many chunks and the codes path,
    whose chunk budget has a 1 MB floor, in three.  With and without prep the
    codes upload fills the same bands as the tables upload, and est / ucode /
    tsum equal rf_host_code_prep's values."""
    opts("stage_kb", 16)
    rng = np.random.default_rng(1616)
    lens = [300] * 40 + [600000] + [300] * 3
    reads = [rng.integers(0, 4, n).astype(np.uint8) for n in lens]
    for k in (1, 39, 41, 42, 43):                 # the reads whose bands are compared resemble the template
        reads[k] = reads[0].copy()
        reads[k][rng.integers(0, 300, 6)] = rng.integers(0, 4, 6)
    phreds = np.concatenate([rng.integers(5, 45, n).astype(np.int8) for n in lens])
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    assert len(_lib.host_upload_chunks(off, True, stage_kb=16)) == 3
    assert len(_lib.host_upload_chunks(off, False, stage_kb=16)) > 40
    allb, code = np.concatenate(reads), phreds.view(np.uint8)
    lp_t, p10_t, match_t, grid = code_tables()
    _, tabs = RifrafSequence.many_concat(reads, phred_to_log_p(phreds), off, 9, SEQ_SCORES, phreds=phreds)
    K = len(lens)
    est_h, ucode_h, lse_h = np.empty(K), np.empty(K, np.int32), np.empty(K)
    assert engine.lib.rf_host_code_prep(K, ptr(code), ptr(off), ptr(p10_t), ptr(match_t), ptr(grid), ptr(est_h),
                                        ptr(ucode_h), ptr(lse_h)) == 0
    ids, sl = np.array([0, 1, 39, 41, 42, 43]), np.arange(6)
    engine.set_templates(0, [reads[0]])
    bands = {}
    for path in ("tables", "codes", "prep"):
        if path == "tables":
            engine.set_sequences_concat(0, allb, off, tabs["match"], tabs["mismatch"], tabs["ins"], tabs["del"])
        else:
            got = engine.set_sequences_codes(0, allb, off, code, lp_t, match_t, SEQ_SCORES,
                                             prep=(p10_t, grid) if path == "prep" else None)
            assert got is not False
        if path == "prep":
            est, ucode, tsum = got
            lse = np.empty(K)
            assert engine.lib.rf_host_lse_finish(K, ptr(tsum), ptr(ucode), ptr(match_t), ptr(lse)) == 0
            np.testing.assert_array_equal(est.view(np.int64), est_h.view(np.int64))
            np.testing.assert_array_equal(ucode, ucode_h)
            np.testing.assert_array_equal(lse.view(np.int64), lse_h.view(np.int64))
        scores = engine.realign(sl, ids, 0, [9] * 6, RF_FWD | RF_BWD)
        bands[path] = [scores] + [engine.download_band(s, w).data.copy() for s in sl for w in (RF_BAND_A, RF_BAND_B)]
    for path in ("codes", "prep"):
        for a, b in zip(bands["tables"], bands[path]):
            np.testing.assert_array_equal(a, b)
