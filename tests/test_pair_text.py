"""rf_pair_align_text (k_pa_emit): the gapped texts, the template -> sequence
index map and the band tolerance of many pairs, made on the device from the
walk's moves.  The checker is host code: align.moves_to_aligned_seqs,
align.moves_to_indices and align.band_tolerance over the moves that
rf_pair_align / rf_pair_align_smart return for the same pairs (pinned to the
oracle by test_pair_align.py and test_pair_align_smart.py; the host functions
by test_pair_text_host.py).  Equality is exact everywhere.
"""
import numpy as np
import pytest

from _util import SEQ_SCORES, make_read, random_seq
from rifraf_amd import ErrorModel, RifrafSequence, Scores, pairalign
from rifraf_amd._lib import ptr
from rifraf_amd.align import band_tolerance, moves_to_aligned_seqs, moves_to_indices
from rifraf_amd.engine import RF_BWD, RF_FWD, RF_SKEW
from rifraf_amd.types import dna_str
from test_pair_align_smart_host import ALWAYS, NEVER, poisson_thresholds, smart_set

pytestmark = pytest.mark.gpu

CHUNK_EDGES = (1, 2, 63, 64, 65, 127, 128, 129, 193)
SHIFT_SCORES = Scores.from_errors(ErrorModel(10.0, 1e-5, 1e-5, 1.0, 1.0))   # correct_shifts_many's default


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def host_products(mv, t, s, bw):
    """(aligned t, aligned s, indices, tolerance) of one move list; None: an invalid pair."""
    if mv is None:
        return None
    return moves_to_aligned_seqs(mv, t, s.seq) + (moves_to_indices(mv, len(t), len(s)),
                                                  band_tolerance(mv, len(s) + 1, len(t) + 1, int(bw)))


def check_products(r, exp, what=None):
    """r: engine.PairText with all three products; exp: host_products per pair."""
    assert r.n == len(exp)
    for k, e in enumerate(exp):
        tag = k if what is None else what[k]
        if e is None:
            assert (r.aln_len[k], r.t2s_len[k], r.tolerance[k]) == (-1, -1, -1), tag
            assert r.text(k) is None and r.indices(k) is None
            continue
        assert r.text(k) == e[:2], (tag, r.text(k), e[:2])
        assert r.aln_len[k] == len(e[0]), tag
        assert r.indices(k).tolist() == e[2] and r.t2s_len[k] == len(e[2]), (tag, r.indices(k), e[2])
        assert r.tolerance[k] == e[3], (tag, r.tolerance[k], e[3])


def all_text(engine, ids_s, ids_t, bws, **kw):
    return engine.pair_align_text(ids_s, ids_t, bws, want_text=True, want_indices=True, want_tolerance=True, **kw)


def run_and_check(engine, seqs, tpls, bws, flags=0, what=None):
    """One pair_align and one pair_align_text call over pairs (k, k); every
    product against the host route.  -> (moves, PairText, expected)."""
    engine.set_sequences(0, seqs)
    engine.set_templates(0, tpls)
    ids = np.arange(len(seqs))
    bws = np.broadcast_to(np.asarray(bws), ids.shape)
    sc, moves, nerr = engine.pair_align(ids, ids, bws, flags)
    got_sc, r = all_text(engine, ids, ids, bws, flags=flags)
    assert bits(got_sc).tolist() == bits(sc).tolist()
    assert r.nerrors.tolist() == nerr.tolist()
    assert r.bandwidths.tolist() == bws.tolist() and (r.rounds == 1).all()
    exp = [host_products(mv, t, s, bw) for mv, t, s, bw in zip(moves, tpls, seqs, bws)]
    check_products(r, exp, what)
    return moves, r, exp


def same_text(a, b):
    for name in ("aln_len", "t2s_len", "tolerance", "nerrors", "bandwidths", "rounds"):
        assert getattr(a, name).tolist() == getattr(b, name).tolist(), name
    assert a.texts() == b.texts()
    for k in range(a.n):
        x, y = a.indices(k), b.indices(k)
        assert (x is None and y is None) or x.tolist() == y.tolist()


# ---------------------------------------------------------------------
# 1. chunk edges
# ---------------------------------------------------------------------
def edited(t, rng, nins, ndel):
    """t with nins single-base insertions and ndel single-base deletions, apart from each other."""
    s = list(t)
    spots = sorted(rng.choice(np.arange(1, max(len(t) - 1, 2)), size=min(nins + ndel, max(len(t) - 2, 1)),
                              replace=False).tolist(), reverse=True) if len(t) > 3 else []
    for q, p in enumerate(spots):
        if q < nins:
            s.insert(p, (s[p] + 2) % 4)
        else:
            del s[p]
    return np.array(s, np.uint8)


def chunk_edge_pairs():
    """Reads of a few indels against templates of 1..3 bases and of lengths
    around 32, 64, 96, 128 and 192: the move counts land on, below and above
    the multiples of 64 a lane chunk holds."""
    rng = np.random.default_rng(2601)
    seqs, tpls = [], []
    for m in (1, 2, 3, 31, 32, 33, 61, 62, 63, 64, 65, 95, 96, 97, 125, 126, 127, 128, 129, 190, 191, 192, 193):
        for nins, ndel in ((0, 0), (1, 0), (2, 1), (1, 2), (3, 0)):
            t = random_seq(m, rng)
            s = edited(t, rng, nins, ndel)
            seqs.append(RifrafSequence(s, np.full(len(s), -2.0), 6, SEQ_SCORES))
            tpls.append(t)
    return seqs, tpls


@pytest.mark.parametrize("walk", (1, 2))
def test_chunk_edges(engine, opts, walk):
    opts("pair_walk", walk)
    seqs, tpls = chunk_edge_pairs()
    moves, r, _ = run_and_check(engine, seqs, tpls, 6, what=[(len(s), len(t)) for s, t in zip(seqs, tpls)])
    counts = {len(mv) for mv in moves}
    assert set(CHUNK_EDGES) <= counts, sorted(set(CHUNK_EDGES) - counts)
    assert any((mv == 2).any() for mv in moves) and any((mv == 3).any() for mv in moves)
    assert engine.last_pair_text_ms() > 0


# ---------------------------------------------------------------------
# 2. codon moves across a lane-chunk boundary
# ---------------------------------------------------------------------
def codon_pairs():
    """correct_shifts_many's sequences (codon tables, skewed alignment): a
    90-base reference against consensuses with a 3-base block inserted (a
    codon deletion) or deleted (a codon insertion) so that the codon move is
    move number 62, 63, 64 or 65.  -> (seqs, tpls, (move number, code))."""
    rng = np.random.default_rng(2602)
    seqs, tpls, what = [], [], []
    for at in (62, 63, 64, 65):
        for code in (4, 5):
            while True:
                ref = random_seq(90, rng)
                blk = ref[at - 1:at + 2] if code == 4 else (ref[at - 1:at + 2] + 2) % 4
                # the block cannot slide: it differs from what precedes and follows it at a distance of 3
                if blk[2] != ref[at - 2] and blk[0] != (ref[at + 2] if code == 4 else ref[at - 1]):
                    break
            if code == 4:     # the consensus lacks three bases of the reference
                cons = np.concatenate([ref[:at - 1], ref[at + 2:]])
            else:             # the consensus has three bases more
                cons = np.concatenate([ref[:at - 1], blk, ref[at - 1:]])
            seqs.append(RifrafSequence(ref, np.full(len(ref), -1.0), 9, SHIFT_SCORES))
            tpls.append(cons.astype(np.uint8))
            what.append((at, code))
    return seqs, tpls, what


@pytest.mark.parametrize("walk", (1, 2))
def test_codon_moves_straddle_chunks(engine, opts, walk):
    opts("pair_walk", walk)
    seqs, tpls, what = codon_pairs()
    moves, r, exp = run_and_check(engine, seqs, tpls, 9, RF_SKEW, what)
    for mv, (at, code), e, t in zip(moves, what, exp, tpls):
        assert mv[at - 1] == code, (at, code, mv[at - 5:at + 4])
        assert e[0][at - 1:at + 2] == "---" if code == 4 else e[1][at - 1:at + 2] == "---"
        assert len(e[2]) == (len(t) - 2 if code == 5 else len(t))


# ---------------------------------------------------------------------
# 3. paths at the band edge
# ---------------------------------------------------------------------
def band_edge_pairs():
    """m = 120, bandwidth 6, reads 12 bases shorter (|n - m| > bw): a block
    insertion of w bases, then a block deletion of 12 + w.  After the
    insertion the path runs w diagonals towards the band's upper edge, 6
    away: w = 6 and 5 touch it or come within one row, w <= 3 stay inside.
    Last a 5 x 5 pair whose band of bandwidth 6 is the whole matrix."""
    rng = np.random.default_rng(2603)
    seqs, tpls = [], []
    for w in (0, 2, 3, 5, 6, 5, 6):
        t = random_seq(120, rng)
        s = np.concatenate([t[:30], (t[30:30 + w] + 1 + np.arange(w)) % 4, t[30:70], t[70 + 12 + w:]]).astype(np.uint8)
        assert len(s) == 108
        seqs.append(RifrafSequence(s, np.full(len(s), -2.0), 6, SEQ_SCORES))
        tpls.append(t)
    t = random_seq(5, rng)
    seqs.append(RifrafSequence(t.copy(), np.full(5, -2.0), 6, SEQ_SCORES))
    tpls.append(t)
    return seqs, tpls


def test_band_edge_paths(engine):
    seqs, tpls = band_edge_pairs()
    _, r, _ = run_and_check(engine, seqs, tpls, 6)
    tol = r.tolerance.tolist()
    assert any(x in (0, 1) for x in tol[:-1]), tol
    assert any(2 <= x < 109 for x in tol[:-1]), tol
    assert tol[-1] == len(seqs[-1]) + 1 == 6, tol


# ---------------------------------------------------------------------
# 4. launch sets
# ---------------------------------------------------------------------
def test_launch_sets(engine, opts):
    """7 pairs of 2,600 x ~2,600 at bandwidth 60: about 160 KB of trace each,
    1.1 MB in all, so pair_trace_mb = 1 splits them; pair_chunk = 3 makes
    three sets."""
    rng = np.random.default_rng(2604)
    tpls = [random_seq(2600, rng) for _ in range(7)]
    seqs = [make_read(t, rng, 0.03, 60) for t in tpls]
    words = [(((2 * 60 + abs(len(s) - len(t)) + 1 + 2 * len(t) + 1) // 2 + 15) // 16) *
             ((2 * 60 + abs(len(s) - len(t)) + 1 + 1) & ~1) for s, t in zip(seqs, tpls)]
    assert sum(words) * 8 > 1 << 20
    _, whole, _ = run_and_check(engine, seqs, tpls, 60)
    ids = np.arange(7)
    opts("pair_chunk", 3)
    same_text(all_text(engine, ids, ids, 60)[1], whole)
    opts("pair_chunk", 65536)
    opts("pair_trace_mb", 1)
    same_text(all_text(engine, ids, ids, 60)[1], whole)


# ---------------------------------------------------------------------
# 5. smart rounds
# ---------------------------------------------------------------------
def test_smart_rounds(engine):
    """smart_set's block-indel pairs from bandwidth 3 with max_doublings 5,
    under thresholds that keep doubling (ALWAYS), that stop every pair in
    round 1 (NEVER) and the Poisson ones, fixed pairs among them."""
    seqs, tpls, _, fixed = smart_set()
    n = len(seqs)
    idx = np.tile(np.arange(n), 3)
    thr = np.concatenate([np.full(n, ALWAYS), np.full(n, NEVER), poisson_thresholds(seqs)])
    engine.set_sequences(0, seqs)
    engine.set_templates(0, tpls)
    sc, moves, nerr, out_bw, rounds = engine.pair_align_smart(idx, idx, 3, thr, fixed=fixed[idx], max_doublings=5)
    got_sc, r = all_text(engine, idx, idx, 3, thresholds=thr, fixed=fixed[idx], max_doublings=5)
    assert bits(got_sc).tolist() == bits(sc).tolist()
    assert r.nerrors.tolist() == nerr.tolist()
    assert r.bandwidths.tolist() == out_bw.tolist() and r.rounds.tolist() == rounds.tolist()
    assert len(set(rounds.tolist())) >= 2 and (rounds[n:2 * n] == 1).all() and fixed.any()
    check_products(r, [host_products(mv, tpls[k], seqs[k], bw) for mv, k, bw in zip(moves, idx, out_bw)], idx)


# ---------------------------------------------------------------------
# 6. an invalid pair, argument errors, no products
# ---------------------------------------------------------------------
def raw_call(engine, n, ids, bw, thr, md, flags, sc=None, at=None, as_=None, aoff=None, alen=None, ix=None,
             ioff=None, ilen=None, tol=None, ne=None, ob=None, rd=None):
    return engine.lib.rf_pair_align_text(engine.ctx, n, ptr(ids), ptr(ids), ptr(bw), ptr(thr), None, md, flags,
                                         ptr(sc), ptr(at), ptr(as_), ptr(aoff), ptr(alen), ptr(ix), ptr(ioff),
                                         ptr(ilen), ptr(tol), ptr(ne), ptr(ob), ptr(rd))


def invalid_trio():
    """test_pair_align.test_invalid_pair_and_null_outputs' construction: the
    middle read has -Inf mismatch, insertion and deletion tables and meets a
    template of another base, so the reference raises on it."""
    rng = np.random.default_rng(2606)
    n = 9
    ninf = np.full(n, -np.inf)
    bad = RifrafSequence(np.zeros(n, np.uint8), np.full(n, -2.0), 3, SEQ_SCORES)
    bad.mismatch_scores, bad.ins_scores, bad.del_scores = ninf, ninf, np.full(n + 1, -np.inf)
    tg = [random_seq(n, rng), random_seq(n + 2, rng)]
    good = [make_read(t, rng, 0.1, 3) for t in tg]
    return [good[0], bad, good[1]], [tg[0], np.full(n, 1, np.uint8), tg[1]]


def test_invalid_pair_and_arguments(engine):
    seqs, tpls = invalid_trio()
    engine.set_sequences(0, seqs)
    engine.set_templates(0, tpls)
    ids = np.arange(3, dtype=np.int32)
    bw = np.full(3, 3, np.int32)
    sc, moves, nerr = engine.pair_align(ids, ids, bw)
    assert np.isnan(sc[1]) and moves[1] is None and moves[0] is not None and moves[2] is not None
    exp = [host_products(mv, t, s, 3) for mv, t, s in zip(moves, tpls, seqs)]
    caps = np.array([len(s) + len(t) for s, t in zip(seqs, tpls)], np.int64)
    aoff = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    ioff = np.concatenate([[0], np.cumsum([len(t) for t in tpls])]).astype(np.int64)

    def fresh():
        return dict(sc=np.full(3, 7.0), at=np.full(aoff[-1], 0x55, np.uint8), as_=np.full(aoff[-1], 0x55, np.uint8),
                    alen=np.full(3, 77, np.int32), ix=np.full(ioff[-1], 77, np.int32), ilen=np.full(3, 77, np.int32),
                    tol=np.full(3, 77, np.int32), ne=np.full(3, 77, np.int32), ob=np.full(3, 77, np.int32),
                    rd=np.full(3, 77, np.int32))

    def untouched(b):
        f = fresh()
        return all(np.array_equal(b[k], f[k]) for k in f)

    b = fresh()
    assert raw_call(engine, 3, ids, bw, None, 0, 0, aoff=aoff, ioff=ioff, **b) == 0   # threshold NULL, no doublings
    assert np.isnan(b["sc"][1]) and bits(b["sc"]).tolist() == bits(sc).tolist()
    assert b["alen"][1] == b["ilen"][1] == b["tol"][1] == b["ne"][1] == -1
    assert (b["at"][aoff[1]:aoff[2]] == 0x55).all() and (b["as_"][aoff[1]:aoff[2]] == 0x55).all()
    assert (b["ix"][ioff[1]:ioff[2]] == 77).all()
    for k in (0, 2):
        ln = b["alen"][k]
        assert b["at"][aoff[k]:aoff[k] + ln].tobytes().decode() == exp[k][0]
        assert b["as_"][aoff[k]:aoff[k] + ln].tobytes().decode() == exp[k][1]
        assert (b["at"][aoff[k] + ln:aoff[k + 1]] == 0x55).all()          # nothing past the text
        assert b["ix"][ioff[k]:ioff[k] + b["ilen"][k]].tolist() == exp[k][2]
        assert b["tol"][k] == exp[k][3] and b["ne"][k] == nerr[k]
    assert b["ob"].tolist() == [3, 3, 3] and b["rd"].tolist() == [1, 1, 1]
    assert engine.last_pair_text_ms() > 0
    # RF_FWD is implied and accepted
    b2 = fresh()
    assert raw_call(engine, 3, ids, bw, None, 0, RF_FWD, aoff=aoff, ioff=ioff, **b2) == 0
    assert all(np.array_equal(b[k], b2[k]) or k == "sc" for k in b) and bits(b["sc"]).tolist() == bits(b2["sc"]).tolist()

    # argument errors leave every output as it was
    thr = np.full(3, ALWAYS)
    for kw, md, flags, th in ((dict(as_=None, aoff=aoff, ioff=ioff), 0, 0, thr),          # aln_t without aln_s
                              (dict(aoff=None, ioff=ioff), 0, 0, thr),                    # text without aln_off
                              (dict(aoff=aoff, ioff=None), 0, 0, thr),                    # map without t2s_off
                              (dict(aoff=aoff, ioff=ioff), 1, 0, None),                   # NULL threshold, one doubling
                              (dict(aoff=aoff, ioff=ioff), 0, RF_BWD, thr),
                              (dict(aoff=aoff, ioff=ioff), 0, RF_FWD | RF_BWD, thr)):
        b = fresh()
        args = dict(b)
        args.update(kw)
        assert raw_call(engine, 3, ids, bw, th, md, flags, **args) == -1, (kw.keys(), md, flags)
        assert untouched(b)

    # no text, map or tolerance: rf_pair_align_smart, and no emit kernel
    s1, _, n1, bw1, r1 = engine.pair_align_smart(ids, ids, bw, thr, max_doublings=2, want_moves=False)
    b = fresh()
    assert raw_call(engine, 3, ids, bw, thr, 2, 0, sc=b["sc"], ne=b["ne"], ob=b["ob"], rd=b["rd"]) == 0
    assert bits(b["sc"]).tolist() == bits(s1).tolist() and b["ne"].tolist() == n1.tolist()
    assert b["ob"].tolist() == bw1.tolist() and b["rd"].tolist() == r1.tolist()
    assert engine.last_pair_text_ms() == 0.0
    fill, walk = engine.last_pair_align_ms()
    assert fill > 0 and walk >= 0


# ---------------------------------------------------------------------
# 7. no side effects
# ---------------------------------------------------------------------
def test_state_untouched(engine):
    rng = np.random.default_rng(2607)
    tpls = [random_seq(m, rng) for m in (80, 70, 95)]
    seqs = [make_read(tpls[0], rng, 0.03, 9) for _ in range(4)]
    engine.set_sequences(0, seqs)
    engine.set_templates(0, tpls)
    ids = np.arange(4)
    engine.realign(ids, ids, 0, 9, RF_FWD | RF_BWD)
    before = engine.score_dense([ids])[0].copy()
    geo = [engine.geometry(int(k)) for k in ids]
    slot_moves, _ = engine.backtrace(ids)
    si, ti = np.repeat(ids, 2), np.tile([1, 2], 4)
    _, moves, _ = engine.pair_align(si, ti, 9)
    _, r = all_text(engine, si, ti, 9)
    check_products(r, [host_products(mv, tpls[j], seqs[i], 9) for mv, i, j in zip(moves, si, ti)])
    grown = engine.device_bytes()
    _, r2 = all_text(engine, si, ti, 9)
    assert engine.device_bytes() == grown
    same_text(r, r2)
    assert before.tobytes() == engine.score_dense([ids])[0].tobytes()
    assert geo == [engine.geometry(int(k)) for k in ids]
    again, _ = engine.backtrace(ids)
    for a, b in zip(slot_moves, again):
        np.testing.assert_array_equal(a, b)


# ---------------------------------------------------------------------
# 8. the Python layer
# ---------------------------------------------------------------------
def test_python_layer(engine):
    """20 mixed pairs: lean and block-indel reads, one the reference raises
    on; every function against the per-pair host route over the moves."""
    set_seqs, set_tpls, _, _ = smart_set(seed=2608, npairs=16)
    bad_seqs, bad_tpls = invalid_trio()
    seqs, tpls = set_seqs[:17] + bad_seqs, set_tpls[:17] + bad_tpls
    assert len(seqs) == 20
    moves = pairalign.align_moves_many(seqs, tpls, engine=engine)
    assert sum(mv is None for mv in moves) == 1 and moves[18] is None
    exp = [host_products(mv, t, s, s.bandwidth) for mv, t, s in zip(moves, tpls, seqs)]
    assert pairalign.align_many(seqs, tpls, engine=engine) == [None if e is None else e[:2] for e in exp]
    idx = pairalign.align_indices_many(seqs, tpls, engine=engine)
    assert [None if x is None else x.tolist() for x in idx] == [None if e is None else e[2] for e in exp]
    assert all(x is None or x.dtype == np.int32 for x in idx)
    tol = pairalign.band_tolerances(seqs, tpls, engine=engine)
    assert tol.dtype == np.int32 and tol.tolist() == [-1 if e is None else e[3] for e in exp]
    # explicit pairs and a bandwidth
    pairs = [(3, 3), (0, 0), (19, 19), (18, 18)]
    mv = pairalign.align_moves_many(seqs, tpls, pairs=pairs, bandwidth=12, engine=engine)
    assert pairalign.align_many(seqs, tpls, pairs=pairs, bandwidth=12, engine=engine) == [
        None if m is None else moves_to_aligned_seqs(m, tpls[j], seqs[i].seq) for m, (i, j) in zip(mv, pairs)]
    # band doubling
    smoves, sbw = pairalign.smart_align_moves_many(seqs, tpls, engine=engine)
    sexp = [host_products(m, t, s, b) for m, t, s, b in zip(smoves, tpls, seqs, sbw)]
    texts, tbw = pairalign.smart_align_many(seqs, tpls, engine=engine)
    assert texts == [None if e is None else e[:2] for e in sexp] and tbw.tolist() == sbw.tolist()
    assert (sbw > np.array([s.bandwidth for s in seqs])).any()
    stol = pairalign.band_tolerances(seqs, tpls, max_doublings=5, engine=engine)
    assert stol.tolist() == [-1 if e is None else e[3] for e in sexp]
    sidx = pairalign.align_indices_many(seqs, tpls, max_doublings=5, engine=engine)
    assert [None if x is None else x.tolist() for x in sidx] == [None if e is None else e[2] for e in sexp]
    for (at, as_), t, s in ((e[:2], t, s) for e, t, s in zip(exp, tpls, seqs) if e is not None):
        assert at.replace("-", "") == dna_str(t) and as_.replace("-", "") == dna_str(s.seq)


def test_correct_shifts_many_unchanged(engine):
    kats = [("TTTT", "TTT", "TTT"), ("TT", "TTT", "TTT"), ("TTTACCC", "TTTCGC", "TTTCCC"),
            ("TTTAAACCC", "TTTCGC", "TTTAAACCC")]   # test/test_correct_shifts.jl:8-35
    got = pairalign.correct_shifts_many([c for c, _, _ in kats], [r for _, r, _ in kats], engine=engine)
    assert [dna_str(g) for g in got] == [e for _, _, e in kats]
