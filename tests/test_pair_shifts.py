"""rf_pair_shifts (k_pa_fix): the single-indel proposals, the corrected
template and the move tallies of many pairs, made on the device from the
walk's moves.  The checker is host code: rf_host_shift_fix over the moves
that rf_pair_align returns for the same pairs (pinned to the oracle by
test_pair_align.py; the host function to the Python restatement by
test_pair_shifts_host.py, which also holds the sweep's generator and shows
that it meets its coverage conditions).  Equality is exact everywhere.
"""
import numpy as np
import pytest

from rifraf_amd import AmbiguousProposalsError, DNASeq, RifrafSequence, _lib, model, pairalign
from rifraf_amd._lib import ptr
from rifraf_amd.engine import RF_BWD, RF_SKEW, RF_TRIM, Engine, RifrafError
from rifraf_amd.types import dna_str
from test_pair_align_host import SHIFT_KATS
from test_pair_shifts_host import (NOCODON_SCORES, SHIFT_SCORES, SWEEP_BW, assert_constructed, assert_sweep_coverage,
                                   constructed_pairs, invalid_reference, sweep_coverage, sweep_pairs)

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@pytest.fixture(scope="module")
def sweep():
    return sweep_pairs()


def same_shifts(a, b, what=None):
    """Two PairShifts with all products agree in every output."""
    assert a.n == b.n
    assert a.fixed_len.tolist() == b.fixed_len.tolist()
    assert a.nprops.tolist() == b.nprops.tolist()
    assert a.tally.tolist() == b.tally.tolist()
    for k in range(a.n):
        tag = k if what is None else what[k]
        assert a.proposals(k) == b.proposals(k), tag
        x, y = a.fixed_seq(k), b.fixed_seq(k)
        assert (x is None and y is None) or x.tolist() == y.tolist(), tag


def untouched_outside(r):
    """Nothing was written outside what the lengths and counts name."""
    for k in range(r.n):
        a, b = int(r.fixed_off[k]) + max(int(r.fixed_len[k]), 0), int(r.fixed_off[k + 1])
        assert (r.fixed[a:b] == 255).all(), k
        a, b = int(r.prop_off[k]) + max(int(r.nprops[k]), 0), int(r.prop_off[k + 1])
        assert (r.prop_kind[a:b] == 255).all() and (r.prop_pos[a:b] == -1).all() and (r.prop_base[a:b] == 255).all(), k


def all_shifts(engine, ids_s, ids_t, bws, flags, seqs, tpls):
    caps = np.array([len(seqs[int(i)]) + len(tpls[int(j)]) for i, j in zip(ids_s, ids_t)], np.int64)
    return engine.pair_shifts(ids_s, ids_t, bws, flags, want_fixed=True, want_proposals=True, caps=caps)


def run_and_check(engine, seqs, tpls, bw, flags, what=None):
    """One pair_align and one pair_shifts call over pairs (k, k); every
    output against host_shift_fix of the moves.  -> (moves, PairShifts)."""
    engine.set_sequences(0, seqs)
    engine.set_templates(0, tpls)
    ids = np.arange(len(seqs))
    sc, moves, _ = engine.pair_align(ids, ids, bw, flags)
    got_sc, r = all_shifts(engine, ids, ids, bw, flags, seqs, tpls)
    assert bits(got_sc).tolist() == bits(sc).tolist()
    exp = _lib.host_shift_fix(moves, [s.seq for s in seqs], tpls)
    same_shifts(r, exp, what)
    untouched_outside(r)
    return moves, r


# ---------------------------------------------------------------------
# 1. the sweep
# ---------------------------------------------------------------------
@pytest.mark.parametrize("flags", (RF_SKEW, 0, RF_SKEW | RF_TRIM))
@pytest.mark.parametrize("walk", (1, 2))
def test_sweep(engine, opts, sweep, walk, flags):
    opts("pair_walk", walk)
    seqs, tpls, what = sweep
    moves, r = run_and_check(engine, seqs, tpls, SWEEP_BW, flags, what)
    assert engine.last_pair_shifts_ms() > 0
    fill_ms, walk_ms = engine.last_pair_align_ms()
    assert fill_ms > 0 and walk_ms > 0
    if flags == RF_SKEW:
        assert_sweep_coverage(sweep_coverage(moves, seqs, tpls))
    assert r.has_single_indels().tolist() == [bool(((mv == 2) | (mv == 3)).any()) for mv in moves]


@pytest.mark.parametrize("walk", (1, 2))
def test_constructed_chunk_edges(engine, opts, walk):
    """A proposal or a codon move at move number 62..66, and a run of two
    inserts across moves 64 / 65 (the state carried between chunks)."""
    opts("pair_walk", walk)
    seqs, tpls, what = constructed_pairs()
    moves, r = run_and_check(engine, seqs, tpls, SWEEP_BW, RF_SKEW, what)
    assert_constructed(moves, what)
    assert r.fixed_len[-1] == -2 and r.nprops[-1] == 2
    # a single-base edit is undone, a codon move leaves the consensus as it is
    assert r.fixed_len[:-1].tolist() == [len(s) if code in (2, 3) else len(t)
                                         for s, t, (_, code) in zip(seqs[:-1], tpls[:-1], what[:-1])]


# ---------------------------------------------------------------------
# 2. other cases
# ---------------------------------------------------------------------
def test_kats(engine):
    cons = [DNASeq(c) for c, _, _ in SHIFT_KATS]
    refs = [DNASeq(r) for _, r, _ in SHIFT_KATS]
    got = pairalign.correct_shifts_many(cons, refs, engine=engine)
    assert [dna_str(g) for g in got] == [x for _, _, x in SHIFT_KATS]
    assert engine.last_pair_shifts_ms() > 0


def test_invalid_pair_between_neighbours(engine, sweep):
    seqs, tpls, _ = sweep
    bad = invalid_reference(9)
    seqs = [seqs[20], bad, seqs[21], bad, seqs[280]]
    tpls = [tpls[20], np.full(9, 1, np.uint8), tpls[21], np.full(12, 1, np.uint8), tpls[280]]
    moves, r = run_and_check(engine, seqs, tpls, SWEEP_BW, RF_SKEW)
    assert [mv is None for mv in moves] == [False, True, False, True, False]
    assert r.fixed_len[[1, 3]].tolist() == [-1, -1] and r.nprops[[1, 3]].tolist() == [-1, -1]
    assert (r.tally[[1, 3]] == -1).all() and (r.fixed_len[[0, 2]] >= 0).all()
    with pytest.raises(RifrafError, match="pair 1: new score is invalid"):
        pairalign._raise_failed(r, True)


def raw_shifts(engine, n, flags, r, scores, ids_s=None, ids_t=None, **nulls):
    ids_s = np.arange(n, dtype=np.int32) if ids_s is None else np.asarray(ids_s, np.int32)
    ids_t = np.arange(n, dtype=np.int32) if ids_t is None else np.asarray(ids_t, np.int32)
    bws = np.full(n, SWEEP_BW, np.int32)
    args = dict(fixed=r.fixed, fixed_off=r.fixed_off, fixed_len=r.fixed_len, nprops=r.nprops, prop_off=r.prop_off,
                prop_kind=r.prop_kind, prop_pos=r.prop_pos, prop_base=r.prop_base, tally=r.tally)
    args.update(nulls)
    return engine.lib.rf_pair_shifts(engine.ctx, n, ptr(ids_s), ptr(ids_t), ptr(bws), int(flags), ptr(scores),
                                     *(ptr(a) for a in args.values()))


def test_refusals_change_nothing(engine, sweep):
    seqs, tpls, _ = sweep
    seqs, tpls = seqs[30:36], tpls[30:36]
    engine.set_sequences(0, seqs)
    engine.set_templates(0, tpls)
    n = len(seqs)
    nm = [len(s) + len(t) for s, t in zip(seqs, tpls)]
    before = engine.device_bytes()
    cases = (dict(flags=RF_SKEW | RF_BWD), dict(flags=RF_SKEW, fixed_off=None), dict(flags=RF_SKEW, prop_off=None),
             dict(flags=RF_SKEW, prop_pos=None), dict(flags=RF_SKEW, ids_s=[0, 1, 2, 3, 4, 1 << 30]),   # an id no upload can have
             dict(flags=RF_SKEW, ids_t=[0, 1, -1, 3, 4, 5]), dict(flags=64))
    for kw in cases:
        r = _lib.PairShifts(n, nm, nm)
        scores = np.full(n, 7.5)
        rc = raw_shifts(engine, n, kw.pop("flags"), r, scores, **kw)
        assert rc == -1, kw   # RF_ERR_ARG
        assert (scores == 7.5).all() and (r.fixed == 255).all() and (r.fixed_len == -1).all(), kw
        assert (r.nprops == -1).all() and (r.prop_kind == 255).all() and (r.prop_pos == -1).all(), kw
        assert (r.tally == -1).all() and engine.device_bytes() == before, kw
    msg = engine.lib.rf_last_error(engine.ctx).decode()
    assert "rf_pair_shifts" in msg and "unknown flags" in msg


def test_device_bytes_bounded_by_the_launch_set():
    """On a fresh engine at pair_chunk 3: a 300-pair call leaves no more
    device memory behind than a 3-pair call.  The pairs are 12 kb, so one
    set's corrected templates (3 x 24 kB) and records are above the 64 KB a
    device buffer starts at, and a buffer sized by the 300 pairs instead of
    by the set would be 100 times the set's."""
    rng = np.random.default_rng(3104)
    seqs, tpls = [], []
    for k in range(3):
        ref = rng.integers(0, 4, 12000).astype(np.uint8)
        cons = list(ref)
        del cons[9000 + k]                         # an insertion
        cons.insert(5000 + 7 * k, int(ref[5000 + 7 * k] + 1) % 4)   # a deletion
        cons[2000] = (cons[2000] + 1) % 4
        seqs.append(RifrafSequence(ref, np.full(len(ref), -1.0), SWEEP_BW, SHIFT_SCORES))
        tpls.append(np.array(cons, np.uint8))
    assert 3 * min(len(s) + len(t) for s, t in zip(seqs, tpls)) > 1 << 16
    few = np.arange(3)
    many = np.tile(few, 100)
    eng = Engine(0)
    try:
        eng.set_option("pair_chunk", 3)
        eng.set_sequences(0, seqs)
        eng.set_templates(0, tpls)
        base = eng.device_bytes()
        sc3, r3 = all_shifts(eng, few, few, SWEEP_BW, RF_SKEW, seqs, tpls)
        after_three = eng.device_bytes()
        sc300, r300 = all_shifts(eng, many, many, SWEEP_BW, RF_SKEW, seqs, tpls)
        after_many = eng.device_bytes()
    finally:
        eng.close()
    # the set's buffers are real memory: moves, corrected templates, the records' bytes and positions
    assert after_three - base >= 3 * 24000 * (1 + 1 + 1 + 4)
    assert after_many <= after_three, (base, after_three, after_many)
    assert r3.nprops.tolist() == [2, 2, 2] and r3.fixed_len.tolist() == [12000] * 3
    assert bits(sc300).tolist() == np.tile(bits(sc3), 100).tolist()
    assert r300.fixed_len.tolist() == [12000] * 300 and r300.nprops.tolist() == [2] * 300
    for k in (0, 1, 2, 150, 299):
        assert r300.proposals(k) == r3.proposals(k % 3)
        assert r300.fixed_seq(k).tolist() == r3.fixed_seq(k % 3).tolist() == fixed_expected(seqs[k % 3], tpls[k % 3])


def fixed_expected(s, t):
    """The consensus with its single insertion and deletion undone: the reference but for the substitution."""
    out = s.seq.copy()
    out[2000] = t[2000]
    return out.tolist()


def test_launch_sets(engine, opts, sweep):
    seqs, tpls, what = sweep
    engine.set_sequences(0, seqs)
    engine.set_templates(0, tpls)
    ids = np.arange(len(seqs))
    sc, whole = all_shifts(engine, ids, ids, SWEEP_BW, RF_SKEW, seqs, tpls)
    opts("pair_chunk", 3)
    sc3, r3 = all_shifts(engine, ids, ids, SWEEP_BW, RF_SKEW, seqs, tpls)
    same_shifts(r3, whole, what)
    assert bits(sc3).tolist() == bits(sc).tolist()
    opts("pair_chunk", 65536)
    opts("pair_trace_mb", 1)
    sc1, r1 = all_shifts(engine, ids, ids, SWEEP_BW, RF_SKEW, seqs, tpls)
    same_shifts(r1, whole, what)
    assert bits(sc1).tolist() == bits(sc).tolist()


def test_capacity_and_sizing_calls(engine, sweep):
    """The first `capacity` records with the true count; without caps the
    engine sizes the buffers by a first call and returns the same."""
    seqs, tpls, what = sweep
    pick = [k for k, w in enumerate(what) if len(w) >= 3][:12]
    seqs, tpls = [seqs[k] for k in pick], [tpls[k] for k in pick]
    engine.set_sequences(0, seqs)
    engine.set_templates(0, tpls)
    ids = np.arange(len(seqs))
    _, full = all_shifts(engine, ids, ids, SWEEP_BW, RF_SKEW, seqs, tpls)
    assert (full.nprops >= 2).sum() >= 6
    _, cut = engine.pair_shifts(ids, ids, SWEEP_BW, RF_SKEW, want_fixed=False, want_proposals=True, prop_cap=1)
    assert cut.nprops.tolist() == full.nprops.tolist() and cut.fixed is None
    assert [cut.proposals(k) for k in ids] == [full.proposals(k)[:1] for k in ids]
    _, sized = engine.pair_shifts(ids, ids, SWEEP_BW, RF_SKEW, want_fixed=True, want_proposals=True)
    same_shifts(sized, full)
    assert int(sized.prop_off[-1]) == int(full.nprops.sum())


def test_all_products_null_is_pair_align_score(engine, sweep):
    seqs, tpls, _ = sweep
    seqs, tpls = seqs[:40], tpls[:40]
    engine.set_sequences(0, seqs)
    engine.set_templates(0, tpls)
    ids = np.arange(40)
    sc, _, _ = engine.pair_align(ids, ids, SWEEP_BW, RF_SKEW, want_moves=False)
    scores = np.empty(40)
    none = dict.fromkeys(("fixed", "fixed_off", "fixed_len", "nprops", "prop_off", "prop_kind", "prop_pos", "prop_base",
                          "tally"))
    assert raw_shifts(engine, 40, RF_SKEW, _lib.PairShifts(40), scores, **none) == 0
    assert bits(scores).tolist() == bits(sc).tolist()
    assert engine.last_pair_shifts_ms() == 0


# ---------------------------------------------------------------------
# 3. Python against model.py's one-pair functions
# ---------------------------------------------------------------------
def model_run(engine, consensus, refseq, scores):
    """model.correct_shifts' state and run for one pair."""
    run = model._Run(engine, 0)
    run.set_consensus(consensus)
    state = model.RifrafState(consensus=consensus, ref_scores=scores, reference=refseq, batch_fixed_size=0,
                              batch_size=0, base_batch_size=0, sequences=[], maxlen=0)
    engine.set_sequences(run.REF, [refseq])
    return state, run


def test_python_equals_model(engine, sweep):
    seqs, tpls, what = sweep
    pick = list(range(15, 45))
    cons = [tpls[k] for k in pick]
    refs = [seqs[k].seq for k in pick]
    for scores in (SHIFT_SCORES, NOCODON_SCORES):
        exp_props, exp_fixed, exp_has = [], [], []
        for c, r in zip(cons, refs):
            rs = RifrafSequence(r, np.full(len(r), -1.0), SWEEP_BW, scores)
            state, run = model_run(engine, c, rs, scores)
            exp_has.append(model.has_single_indels(state, run))
            state, run = model_run(engine, c, rs, scores)
            exp_props.append(model.single_indel_proposals(state, run))
            try:
                exp_fixed.append(model.correct_shifts(c, r, bandwidth=SWEEP_BW, scores=scores, engine=engine))
            except AmbiguousProposalsError:
                exp_fixed.append(None)
        props = pairalign.single_indel_proposals_many(cons, refs, bandwidth=SWEEP_BW, scores=scores, engine=engine)
        assert props == exp_props
        rss = [RifrafSequence(r, np.full(len(r), -1.0), SWEEP_BW, scores) for r in refs]
        assert pairalign.has_single_indels_many(cons, rss, engine=engine).tolist() == exp_has
        ok = [k for k, f in enumerate(exp_fixed) if f is not None]
        got = pairalign.correct_shifts_many([cons[k] for k in ok], [refs[k] for k in ok], bandwidth=SWEEP_BW,
                                            scores=scores, engine=engine)
        assert [g.tolist() for g in got] == [exp_fixed[k].tolist() for k in ok]
        if scores is NOCODON_SCORES:
            assert len(ok) < len(cons)
            with pytest.raises(AmbiguousProposalsError):
                pairalign.correct_shifts_many(cons, refs, bandwidth=SWEEP_BW, scores=scores, engine=engine)
    # one shared reference, the default bandwidth per pair
    ref = seqs[15].seq
    shared = [tpls[15], ref.copy(), ref[1:], ref[:-3], np.concatenate([ref[:20], ref[21:]])]
    got = pairalign.correct_shifts_many(shared, seqs[15].seq, engine=engine)
    exp = [model.correct_shifts(c, seqs[15].seq, engine=engine) for c in shared]
    assert [g.tolist() for g in got] == [x.tolist() for x in exp]
