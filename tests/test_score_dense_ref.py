"""rf_score_dense_ref (k_codon_dense): the dense table with the reference's
score added last in every slot, against two sources that must both agree
with it bit for bit -- engine.score over the list of all proposals with the
same reference slot (k_codon), and oracle.score_list with the reference's
bands.  Compared: every slot but the Sub / Del slots of p = 0 (asserted NaN)
and the consensus base's own Sub slot.

The codon reference is the one correct_shifts builds: constant
error_log_p = -1 and Scores.from_errors(ErrorModel(10, 1e-5, 1e-5, 1, 1)).
Its six tables hold one number each, so a table read one position off is
the same value; varying_reference (error_log_p = log10(U(0.01, 0.3)) per
position, every table different at every position) is the reference of the
second half of this file: the edge grid again, m at which 9 (m + 1) fills
its last workgroup, groups without a reference between groups with one,
tall and skewed bands, a frameshifted reference, the reads' scorers and
folds under the in-place add, and the reference changing from call to call
over one cached dense plan.
"""
import functools

import numpy as np
import pytest

import oracle
from _util import REF_SCORES, all_proposals_arrays, assert_score_launch, dense_slot, make_read, random_seq
from rifraf_amd import ErrorModel, RifrafSequence, Scores
from rifraf_amd._lib import ptr
from rifraf_amd.engine import RF_BWD, RF_FWD, Engine, RifrafError

pytestmark = pytest.mark.gpu

CODON = Scores.from_errors(ErrorModel(10.0, 1e-5, 1e-5, 1.0, 1.0))
PLAIN = Scores.from_errors(ErrorModel(1.0, 2.0, 2.0))
RF_ERR_ARG, RF_ERR_STATE = -1, -4

# m, n - m, bw: the i > 3 / j > 3 gates, Insertion(0, .), the just_a tail at
# pos >= m - 3, Deletion(m)'s shortcut, row ranges clipped at both ends
EDGES = [(m, dn, bw) for m in (1, 2, 3, 4, 5, 7, 12, 40) for dn in (-4, 0, 5) for bw in (1, 2, 3, 9)
         if m + dn >= 1]


def same(got, exp):
    """Bit equality (int64 views) on finite values, NaN only where both are."""
    got, exp = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(exp, np.float64)
    nan = np.isnan(got) | np.isnan(exp)
    return np.where(nan, np.isnan(got) & np.isnan(exp), got.view(np.int64) == exp.view(np.int64))


def dense_mask(t):
    mask = np.ones((len(t) + 1, 9), bool)
    mask[0, :5] = False                                                # p = 0 has no sub / del
    mask[np.arange(1, len(t) + 1), np.asarray(t, np.int64)] = False    # the consensus base's own slot
    return mask


def table(t, props, totals):
    """A proposal list's totals in the dense layout (NaN elsewhere)."""
    k, p, b = props
    out = np.full((len(t) + 1, 9), np.nan)
    out[p, dense_slot(k, b)] = totals
    return out


def reference(n, bw, rng, scores=CODON):
    return RifrafSequence(random_seq(n, rng), np.full(n, -1.0), bw, scores)


def varying_reference(n, bw, rng, scores, seq=None):
    """A reference whose tables differ at every position: error_log_p =
    log10(U(0.01, 0.3)) (random bases unless seq is given)."""
    seq = random_seq(n, rng) if seq is None else seq
    assert len(seq) == n
    return RifrafSequence(seq, np.log10(rng.uniform(0.01, 0.3, n)), bw, scores)


class Case:
    """One group: a template, 1-3 ordinary reads and a reference."""

    def __init__(self, t, reads, ref):
        self.t, self.reads, self.ref = t, reads, ref
        self.props = all_proposals_arrays(t)
        self._oracle = None

    def oracle_table(self):
        """Computed once: the cases that several tests share keep it."""
        if self._oracle is None:
            t, rs = self.t, self.reads
            tot = oracle.score_list(self.props, [oracle.forward(t, r)[0] for r in rs],
                                    [oracle.backward(t, r) for r in rs], rs, t,
                                    oracle.forward(t, self.ref)[0], oracle.backward(t, self.ref), self.ref,
                                    nthreads=1)
            self._oracle = table(t, self.props, tot)
        return self._oracle


def make_case(m, n, bw, rng, nreads, scores=CODON):
    t = random_seq(m, rng)
    reads = [make_read(t, rng, bandwidth=3) for _ in range(nreads)]
    return Case(t, reads, reference(n, bw, rng, scores))


def make_varying_case(m, n, bw, rng, nreads, scores=CODON, read_bw=3):
    t = random_seq(m, rng)
    reads = [make_read(t, rng, bandwidth=read_bw) for _ in range(nreads)]
    return Case(t, reads, varying_reference(n, bw, rng, scores))


def load(engine, cases):
    """Upload the cases (template c; sequences and slots: the reads of every
    case in turn, each followed by its reference) and fill every band.
    Returns per case (batch slots, reference slot)."""
    engine.release_bands()    # the session engine: no band of an earlier test in any slot
    seqs, tpl, ids = [], [], []
    for c, cs in enumerate(cases):
        at = len(seqs)
        seqs += cs.reads + [cs.ref]
        tpl += [c] * (len(cs.reads) + 1)
        ids.append((np.arange(at, at + len(cs.reads), dtype=np.int32), at + len(cs.reads)))
    engine.set_sequences(0, seqs)
    engine.set_templates(0, [cs.t for cs in cases])
    k = np.arange(len(seqs))
    engine.realign(k, k, tpl, [s.bandwidth for s in seqs], RF_FWD | RF_BWD)
    return ids


def check_cases(engine, cases, label, noref=()):
    """One rf_score_dense_ref call of all cases against the list path and the
    oracle.  The cases whose index is in noref are called with ref_slot -1
    (their reference is uploaded and unused): every slot of theirs has
    rf_score_dense's bits.  Returns load()'s slots."""
    ids = load(engine, cases)
    groups = [b for b, _ in ids]
    got = engine.score_dense_ref(groups, [-1 if c in noref else r for c, (_, r) in enumerate(ids)])
    lists = engine.score([(b, r, cs.props) for (b, r), cs in zip(ids, cases)])
    plain = engine.score_dense(groups) if noref else None
    for c, cs in enumerate(cases):
        mask = dense_mask(cs.t)
        key = (label, c, len(cs.t), len(cs.ref), cs.ref.bandwidth)
        if c in noref:
            assert same(got[c], plain[c]).all(), ("no reference",) + key
            continue
        assert np.isnan(got[c][0, :5]).all(), key
        exp = table(cs.t, cs.props, lists[c])
        assert same(got[c][mask], exp[mask]).all(), ("list path",) + key
        assert same(got[c][mask], cs.oracle_table()[mask]).all(), ("oracle",) + key
        assert np.isfinite(got[c][mask]).all(), key
    return ids


def test_edges(engine):
    """The whole edge grid as one call of 80 groups (n = m - 4 needs m >= 5)."""
    rng = np.random.default_rng(2701)
    cases = [make_case(m, m + dn, bw, rng, 1 + k % 3) for k, (m, dn, bw) in enumerate(EDGES)]
    assert len(cases) == 80
    check_cases(engine, cases, "edges")


def test_tall_bands(engine):
    """m = n = 150 at bandwidths 40 and 70: bands of 81 and 141 rows, taller
    than one and two waves."""
    rng = np.random.default_rng(2702)
    cases = [make_case(150, 150, bw, rng, 1) for bw in (40, 70)]
    ids = load(engine, cases)
    assert [engine.geometry(r)[3] for _, r in ids] == [81, 141]
    check_cases(engine, cases, "tall")


def test_reference_without_codon_tables(engine):
    """A reference built with ErrorModel(1, 2, 2): score_nocodon and
    seq_score_deletion, the list path's other branch."""
    rng = np.random.default_rng(2703)
    cases = [make_case(m, m + dn, bw, rng, 2, PLAIN) for m, dn, bw in ((3, 0, 1), (12, 5, 3), (40, -4, 9), (7, 0, 2))]
    assert all(len(cs.ref.codon_ins_scores) == 0 and len(cs.ref.codon_del_scores) == 0 for cs in cases)
    check_cases(engine, cases, "plain")


def invalid_case(rng):
    """n = m = 20 at bandwidth 2.  Reference row 10 has -Inf mismatch,
    insertion, deletion and codon scores, so a cell of that row is finite
    only where the template base equals the reference's.  The template
    carries that base in columns 8-12 -- every cell of the row inside the
    band -- so the fills are valid, and a proposal that brings another base
    into those columns is one the reference raises on."""
    n = 20
    ref = reference(n, 2, rng)
    ref.seq[9] = 1
    for f in ("mismatch_scores", "ins_scores", "del_scores", "codon_ins_scores", "codon_del_scores"):
        setattr(ref, f, np.array(getattr(ref, f), np.float64))
    ref.mismatch_scores[9] = ref.ins_scores[9] = ref.del_scores[10] = -np.inf
    ref.codon_del_scores[10] = ref.codon_ins_scores[7] = -np.inf
    t = np.full(n, 2, np.uint8)
    t[7:12] = 1
    return Case(t, [make_read(t, rng, bandwidth=3) for _ in range(2)], ref)


def test_invalid_slots(engine):
    """The NaN set equals the list path's: every proposal scored in a call of
    its own, NaN where rf_score raises "failed to compute a valid score";
    the oracle raises on the same proposals."""
    cs = invalid_case(np.random.default_rng(2704))
    (b, r), = load(engine, [cs])
    k, p, kb = cs.props
    tot = np.empty(len(k))
    for j in range(len(k)):
        try:
            tot[j] = engine.score([(b, r, (k[j:j + 1], p[j:j + 1], kb[j:j + 1]))])[0][0]
        except RifrafError as e:
            assert "failed to compute a valid score" in str(e)
            tot[j] = np.nan
    exp = table(cs.t, cs.props, tot)
    mask = dense_mask(cs.t)
    assert np.isnan(exp[mask]).any() and np.isfinite(exp[mask]).any()
    got = engine.score_dense_ref([b], [r])[0]
    assert same(got[mask], exp[mask]).all()
    # the oracle: the reads' fold, then the reference's score or its error
    A, B = oracle.forward(cs.t, cs.ref)[0], oracle.backward(cs.t, cs.ref)
    reads = oracle.cpu_pass(cs.t, cs.reads, nthreads=1)[0]
    for j in range(len(k)):
        sl = (p[j], dense_slot(k[j], kb[j]))
        try:
            e = reads[sl] + oracle.score_proposal(k[j], p[j], kb[j], A, B, cs.t, cs.ref)
        except oracle.OracleError:
            e = np.nan
        assert same(got[sl], e), (int(k[j]), int(p[j]), int(kb[j]))


def test_several_groups(engine):
    """Three groups of different m with ref_slot = [-1, r1, r2]: group 0 has
    rf_score_dense's bits, the others those of their own single-group calls."""
    rng = np.random.default_rng(2705)
    cases = [make_case(m, n, bw, rng, 2) for m, n, bw in ((9, 9, 3), (70, 66, 5), (23, 28, 4))]
    ids = load(engine, cases)
    groups = [b for b, _ in ids]
    got = engine.score_dense_ref(groups, [-1, ids[1][1], ids[2][1]])
    plain = engine.score_dense(groups)
    assert same(got[0], plain[0]).all()
    for c in (1, 2):
        mask = dense_mask(cases[c].t)
        alone = engine.score_dense_ref([groups[c]], [ids[c][1]])[0]
        assert same(got[c][mask], alone[mask]).all()
        assert same(got[c][mask], cases[c].oracle_table()[mask]).all()
        assert not same(got[c][mask], plain[c][mask]).any()    # the reference's score is in every slot
    none = engine.score_dense_ref(groups, [-1, -1, -1])
    for c in range(3):
        assert same(none[c], plain[c]).all()


def raw(engine, groups, refs, out=True):
    """rf_score_dense_ref's return code (refs None: a NULL ref_slot)."""
    slot_off = np.zeros(len(groups) + 1, np.int32)
    np.cumsum([len(g) for g in groups], out=slot_off[1:])
    slots = np.ascontiguousarray(np.concatenate(groups), np.int32)
    rows = sum(engine.geometry(int(g[0]))[1] for g in groups)
    buf = np.empty((rows, 9)) if out else None
    rp = None if refs is None else np.ascontiguousarray(refs, np.int32)
    return engine.lib.rf_score_dense_ref(engine.ctx, len(groups), ptr(slot_off), ptr(slots), ptr(rp), ptr(buf)), buf


def test_state_and_argument_errors(engine):
    """Refusals leave the context usable: a valid call follows each."""
    rng = np.random.default_rng(2706)
    cases = [make_case(12, 12, 3, rng, 2), make_case(12, 14, 3, rng, 1)]
    ids = load(engine, cases)
    (b0, r0), (b1, r1) = ids
    good = engine.score_dense_ref([b0], [r0])[0]

    def still_fine():
        rc, buf = raw(engine, [b0], [r0])
        assert rc == 0 and same(buf, good).all()

    assert raw(engine, [b0], None)[0] == RF_ERR_ARG                    # ref_slot = NULL
    still_fine()
    assert raw(engine, [b0], [10 ** 6])[0] == RF_ERR_ARG               # unknown reference slot
    still_fine()
    # a reference slot filled against another template id
    rc, _ = raw(engine, [b0], [r1])
    assert rc == RF_ERR_ARG and "different template" in engine.lib.rf_last_error(engine.ctx).decode()
    still_fine()
    # a reference slot with only its A band
    spare = r1 + 1
    engine.realign([spare], [r0], 0, [cases[0].ref.bandwidth], RF_FWD)
    rc, _ = raw(engine, [b0], [spare])
    assert rc == RF_ERR_STATE and "slot has no A/B bands" in engine.lib.rf_last_error(engine.ctx).decode()
    still_fine()
    # the template uploaded again after the fill
    engine.set_templates(0, [cases[0].t])
    rc, _ = raw(engine, [b0], [r0])
    assert rc == RF_ERR_STATE and "template changed" in engine.lib.rf_last_error(engine.ctx).decode()
    k = np.concatenate([b0, [r0]])
    engine.realign(k, k, 0, [s.bandwidth for s in cases[0].reads + [cases[0].ref]], RF_FWD | RF_BWD)
    still_fine()
    # out = NULL: the totals stay on the device
    assert raw(engine, [b0], [r0], out=False)[0] == 0
    still_fine()


def test_no_side_effects(engine):
    """rf_score_dense and the rf_score list path return the same bits before
    and after rf_score_dense_ref on the same slots."""
    rng = np.random.default_rng(2707)
    cs = make_case(33, 31, 4, rng, 3)
    (b, r), = load(engine, [cs])
    dense0 = engine.score_dense([b])[0].copy()
    list0 = engine.score([(b, r, cs.props)])[0].copy()
    got = engine.score_dense_ref([b], [r])[0].copy()
    dense1 = engine.score_dense([b])[0]
    list1 = engine.score([(b, r, cs.props)])[0]
    assert same(dense0, dense1).all() and same(list0, list1).all()
    assert same(engine.score_dense_ref([b], [r])[0], got).all()
    mask = dense_mask(cs.t)
    assert same(got[mask], table(cs.t, cs.props, list0)[mask]).all()
    assert engine.last_codon_dense_ms() > 0.0


def test_device_memory():
    """m = n = 600, 2 reads, bandwidth 9 on a fresh engine: after score_dense
    has sized the shared buffers, score_dense_ref may grow rf_device_bytes by
    less than 1/16 of 32 (n + 1) (8 m + 4) bytes -- the list path's newcols
    scratch for the same proposal set (its planner takes 4 (n + 1) doubles per
    proposal), about 92 MB here."""
    rng = np.random.default_rng(2708)
    m = n = 600
    cs = make_case(m, n, 9, rng, 2)
    e = Engine(0)
    try:
        (b, r), = load(e, [cs])
        e.score_dense([b])
        before = e.device_bytes()
        got = e.score_dense_ref([b], [r])[0]
        growth = e.device_bytes() - before
        bound = 32 * (n + 1) * (8 * m + 4) // 16
        print(f"rf_device_bytes growth {growth} B, bound {bound} B")
        assert growth < bound
        lists = e.score([(b, r, cs.props)])[0]
        mask = dense_mask(cs.t)
        assert same(got[mask], table(cs.t, cs.props, lists)[mask]).all()
    finally:
        e.close()


# ---------------------------------------------------------------------
# References whose tables differ at every position
# ---------------------------------------------------------------------

@pytest.mark.parametrize("scores", [CODON, REF_SCORES], ids=["CODON", "REF_SCORES"])
def test_varying_tables_edges(engine, scores):
    """The edge grid of test_edges with match, mismatch, insertion, deletion
    and codon tables that differ at every position, under the scores
    correct_shifts builds and the reference's default ones."""
    rng = np.random.default_rng(2711)
    cases = [make_varying_case(m, m + dn, bw, rng, 1 + k % 3, scores) for k, (m, dn, bw) in enumerate(EDGES)]
    assert len(cases) == 80
    check_cases(engine, cases, "varying edges")


def test_workgroup_edges(engine):
    """m = 62, 63, 64, 127, 128 (n = m + 2, bandwidth 5) in one call: 9 (m + 1)
    is 576 = 9 * 64 at m = 63 and 1152 = 18 * 64 at m = 127, so those groups'
    last workgroups have no idle lane and the next group starts on the very
    next workgroup; m one below and above leave 55 idle lanes and 9 used ones.
    Three groups with ref_slot -1 stand at the front, in the middle and at the
    end: they take no workgroup and no descriptor, and have rf_score_dense's
    bits."""
    rng = np.random.default_rng(2712)
    ms = [63, 62, 63, 30, 64, 127, 128, 128]
    noref = (0, 3, 7)
    assert 9 * (63 + 1) == 9 * 64 and 9 * (127 + 1) == 18 * 64
    cases = [make_varying_case(m, m + 2, 5, rng, 1 + k % 2) for k, m in enumerate(ms)]
    check_cases(engine, cases, "workgroup edges", noref)


def test_tall_and_skewed_bands_varying(engine):
    """Bands taller than one and two waves, and n far from m at a narrow band
    (|n - m| = 40 and 60 against bandwidths 9 and 30: the row ranges are
    clipped at both ends), with varying tables."""
    rng = np.random.default_rng(2713)
    shapes = [(150, 150, 40), (150, 150, 70), (120, 160, 9), (160, 120, 9), (200, 260, 30)]
    cases = [make_varying_case(m, n, bw, rng, 1) for m, n, bw in shapes]
    ids = check_cases(engine, cases, "tall and skewed")
    assert [engine.geometry(r)[3] for _, r in ids] == [81, 141, 59, 59, 121]


def test_frameshifted_reference(engine):
    """A template of 300 bases that is the reference with two single-base
    indels and a three-base insertion and deletion -- the consensus
    correct_shifts meets -- under varying tables.  By the oracle's backtrace
    alone the reference's alignment takes a codon insertion (move 4) and a
    codon deletion (move 5)."""
    rng = np.random.default_rng(2714)
    m = 300
    t = random_seq(m, rng)
    s = t
    for at, cut, add in ((240, 3, 0), (180, 0, 3), (120, 1, 0), (60, 0, 1)):   # back to front
        s = np.concatenate([s[:at], random_seq(add, rng), s[at + cut:]]).astype(np.uint8)
    ref = varying_reference(len(s), 9, rng, CODON, seq=s)
    _, moves = oracle.forward(t, ref, moves=True)
    walk = oracle.backtrace(moves, len(s) + 1, m + 1, ref.bandwidth)
    assert (walk == 4).any() and (walk == 5).any()
    cs = Case(t, [make_read(t, rng, bandwidth=9) for _ in range(2)], ref)
    check_cases(engine, [cs], "frameshifted")


@functools.lru_cache(maxsize=None)
def crossing_cases():
    """m = 260, three reads and a varying codon reference, all at bandwidth 9
    and all at bandwidth 25: shared by the legs of test_scorer_crossing."""
    rng = np.random.default_rng(2715)
    return [make_varying_case(260, n, bw, rng, 3, read_bw=bw) for n, bw in ((257, 9), (266, 25))]


@pytest.mark.parametrize("kern", ["general", "ws", "seg"])
@pytest.mark.parametrize("mode", ["fused", "split"])
def test_scorer_crossing(engine, opts, mode, kern):
    """The in-place add after each of the reads' scorers (k_score,
    k_score_ws, k_score_segl) and folds (fused; split, where k_reduce writes
    the totals last): one group of three reads per call."""
    opts("score_mode", mode)
    opts("score_kernel", kern)
    for cs in crossing_cases():
        check_cases(engine, [cs], f"crossing {mode} {kern}")
        assert_score_launch(engine, kern, mode)


def test_reference_follows_the_call(engine):
    """One batch and two reference slots (other sequences, bandwidths 3 and
    9) against the same template: calls with r1, r2, no reference and r1
    again.  The batch slot list is the same in every call, so the dense plan
    of the preceding rf_score_dense is reused throughout; each result is its
    own oracle table."""
    rng = np.random.default_rng(2716)
    t = random_seq(50, rng)
    reads = [make_read(t, rng, bandwidth=3) for _ in range(2)]
    refs = [varying_reference(48, 3, rng, CODON), varying_reference(53, 9, rng, REF_SCORES)]
    engine.release_bands()
    seqs = reads + refs
    engine.set_sequences(0, seqs)
    engine.set_templates(0, [t])
    k = np.arange(len(seqs))
    engine.realign(k, k, 0, [s.bandwidth for s in seqs], RF_FWD | RF_BWD)
    b, (r1, r2) = k[:2], k[2:]
    engine.score_dense([b], to_host=False)
    got = [engine.score_dense_ref([b], [r])[0] for r in (r1, r2, -1, r1)]
    mask = dense_mask(t)
    exp1, exp2 = (Case(t, reads, ref).oracle_table() for ref in refs)
    assert same(got[0][mask], exp1[mask]).all()
    assert same(got[1][mask], exp2[mask]).all()
    assert same(got[2][mask], oracle.cpu_pass(t, reads, nthreads=1)[0][mask]).all()
    assert same(got[3], got[0]).all()
    assert not same(got[0][mask], got[1][mask]).any() and not same(got[0][mask], got[2][mask]).any()
    for g in (got[0], got[1]):
        assert np.isnan(g[0, :5]).all()
