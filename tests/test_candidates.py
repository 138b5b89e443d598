"""Candidate selection on the device (k_cand_select, k_cand_choose).

rf_candidates_table against rf_host_candidates, field for field, on the
small cases of tests/test_candidates_host.py (ties and capacities included);
rf_candidates against today's host sequence -- rf_alignment_proposals +
mask_to_proposals (or all_proposals) + rf_score + the `total > score` filter +
choose_candidates -- with score bits, order, counts and chosen identical; its
refusals; and the native driver with RF_OPT_CAND_DEVICE 0 and 1."""
import numpy as np
import pytest

import test_candidates_host as H
from _util import make_read, random_seq
from rifraf_amd import ErrorModel, Scores
from rifraf_amd import _lib
from rifraf_amd._lib import ptr
from rifraf_amd.engine import RF_BWD, RF_FWD, RifrafError
from rifraf_amd.model import Stage, all_proposals, mask_to_proposals
from rifraf_amd.proposals import DEL, INS, Proposal, ScoredProposal, choose_candidates
from test_score_dense_ref import CODON, Case, load, reference

pytestmark = pytest.mark.gpu

RF_ERR_ARG, RF_ERR_STATE = -1, -4


# ------------------------------------------------ rf_candidates_table vs the host

def both(engine, groups, scores, sources, md, **kw):
    args = ([g[0] for g in groups], [g[1] for g in groups], scores, sources, md)
    kw = dict(masks=[g[2] for g in groups], with_counts=True, **kw)
    return engine.candidates_table(*args, **kw), _lib.host_candidates(*args, **kw)


def assert_same_results(got, exp):
    assert len(got) == len(exp)
    for (gc, gh, gnc, gnh), (ec, eh, enc, enh) in zip(got, exp):
        assert (gnc, gnh) == (enc, enh)
        for g, e in ((gc, ec), (gh, eh)):
            if e is None:
                assert g is None
            else:
                H.same(g, e)


def test_table_random(engine):
    """Every m and source of the host file as the groups of one call per
    min_dist (35 groups; pooled values, so ties everywhere)."""
    groups, sources = [], []
    for m in H.MS:
        for src in H.SOURCES:
            rng = np.random.default_rng(1000 * m + src)
            groups.append(H.random_group(rng, m, pool=bool((m + src) % 2)))
            sources.append(src)
    scores, totals = [0.0] * len(groups), []
    for md in (0, 1, 3, 15, 71):
        got, exp = both(engine, groups, scores, sources, md)
        assert_same_results(got, exp)
        totals.append(sum(r[3] for r in exp))
    assert totals[0] > totals[2] > totals[4] > 0   # the distance filter bites
    sel, cho = engine.last_candidates_ms()
    assert sel > 0.0 and cho > 0.0


def test_table_hand_made(engine):
    """The tie, extreme, NaN-elsewhere and several-group cases."""
    for _, grp, score, src, md, chosen in H.TIES:
        got, exp = both(engine, [grp], [score], [src], md)
        assert_same_results(got, exp)
        assert [c.proposal for c in got[0][1]] == chosen
    for _, groups, scores, sources, md, counts in H.EXTREMES:
        got, exp = both(engine, groups, scores, sources, md)
        assert_same_results(got, exp)
        assert [(r[2], r[3]) for r in got] == counts
    for _, grp, src, fatal in H.NANS:
        if not fatal:
            assert_same_results(*both(engine, [grp], [0.0], [src], 2))
    groups, scores, sources = H.several_groups()
    for md in (0, 3):
        got, exp = both(engine, groups, scores, sources, md)
        assert_same_results(got, exp)
        H.check_groups(engine.candidates_table, groups, scores, sources, md)


def test_table_nan_proposal_fails(engine):
    """NaN in a proposal slot: rf_score's code and message; the context goes on."""
    fatal = [c for c in H.NANS if c[3]]
    assert len(fatal) == 11
    for _, grp, src, _ in fatal:
        with pytest.raises(RifrafError, match="failed to compute a valid score"):
            engine.candidates_table([grp[0]], [grp[1]], [np.inf], [src], 2, masks=[grp[2]])
    grp = H.flat_group(6, fill=1.0)
    assert_same_results(*both(engine, [grp], [0.0], [0], 1))


@pytest.mark.parametrize("short", ("zero", "exact", "one_short", "counts_only", "chosen_only"))
def test_table_capacities(engine, short):
    H.test_capacities(short, run=engine.candidates_table)


def test_table_long_group(engine):
    """m = 1500 (53 rounds of 256 slots per scan, a bitmap of 47 words) with
    sparse candidates and a whole table of them."""
    rng = np.random.default_rng(8)
    cons, table, mask = H.random_group(rng, 1500, pool=False)
    sparse = (cons, table - 2.5, mask)
    got, exp = both(engine, [sparse, (cons, table, mask)], [0.0, 0.0], [1, 0], 15)
    assert_same_results(got, exp)
    assert 0 < exp[0][2] < 200 and exp[1][3] > 50


# ------------------------------------------------ rf_candidates vs today's path

PLAIN = Scores.from_errors(ErrorModel(1.0, 2.0, 2.0))


def todays_path(engine, slots, ref_slot, cons, score, source, md, mask=None):
    """(candidates, chosen) as get_candidates + choose_candidates give them."""
    if source in (1, 2):
        props = mask_to_proposals(engine.alignment_proposals([slots], source == 1)[0])
    elif source == 4:
        props = [p for p in all_proposals(Stage.INIT, cons, False) if mask[p.pos, H.slot_of(p)]]
    else:
        props = all_proposals(Stage.INIT if source == 0 else Stage.REFINE, cons, False)
    if not props:
        return [], []
    tot = engine.score([(slots, ref_slot, props)])[0]
    cands = [ScoredProposal(p, float(s)) for p, s in zip(props, tot) if s > score]
    return cands, choose_candidates(cands, md)


def off_consensus(t, rng, k):
    """t with k edits several bases apart (candidates exist against its reads)."""
    c = list(t)
    for pos in sorted(rng.choice(np.arange(3, len(t) - 3, 7), k, replace=False), reverse=True):
        kind = rng.integers(0, 3)
        if kind == 0:
            c[pos] = (c[pos] + 1) % 4
        elif kind == 1:
            c.insert(pos, int(rng.integers(0, 4)))
        else:
            del c[pos]
    return np.array(c, np.uint8)


@pytest.fixture(scope="module")
def clusters(engine):
    """Three clusters of 4-6 reads (m about 30, 64, 130; the first two with a
    consensus several edits off its reads' template) and a reference-guided
    one.  Slots and the state scores are computed once."""
    rng = np.random.default_rng(4242)
    cases = []
    for m, nr, edits in ((30, 4, 3), (64, 6, 5), (130, 5, 0)):
        t = random_seq(m, rng)
        reads = [make_read(t, rng, error_rate=0.04, bandwidth=9) for _ in range(nr)]
        cons = off_consensus(t, rng, edits) if edits else t
        cases.append(Case(cons, reads, reference(len(cons), 6, rng, CODON)))
    t = random_seq(45, rng)
    cons = off_consensus(t, rng, 3)
    cases.append(Case(cons, [make_read(t, rng, error_rate=0.03, bandwidth=9) for _ in range(4)],
                      reference(len(t), 6, rng, CODON)))
    ids = load(engine, cases)
    # state.score: the fold of A[end, end] over the batch (+ the reference in FRAME)
    scores = []
    for c, (b, r) in enumerate(ids):
        sl = np.concatenate([b, [r]]) if c == 3 else b
        bws = [s.bandwidth for s in (cases[c].reads + ([cases[c].ref] if c == 3 else []))]
        scores.append(float(np.sum(engine.realign(sl, sl, c, bws, RF_FWD | RF_BWD))))
    return cases, ids, scores


def seed_mask(cons, rng):
    """A FRAME mask: every substitution, indels around two seeds."""
    m = len(cons)
    seeds = [Proposal(INS, int(rng.integers(4, m - 4)), 1), Proposal(DEL, int(rng.integers(4, m - 4)), 0)]
    mask = np.zeros((m + 1, 9), np.uint8)
    for p in all_proposals(Stage.FRAME, cons, False, seeds):
        mask[p.pos, H.slot_of(p)] = 1
    return mask


@pytest.mark.parametrize("md", (0, 1, 15))
def test_candidates_match_todays_path(engine, clusters, md):
    cases, ids, scores = clusters
    rng = np.random.default_rng(9)
    fmask = seed_mask(cases[3].t, rng)
    seen = 0
    for source in (0, 1, 2, 3):
        groups = [b for b, _ in ids[:3]]
        got = engine.candidates(groups, scores[:3], [source] * 3, md, with_counts=True)
        for c in range(3):
            ec, eh = todays_path(engine, ids[c][0], -1, cases[c].t, scores[c], source, md)
            H.same(got[c][0], ec)
            H.same(got[c][1], eh)
            assert got[c][2:] == (len(ec), len(eh))
            seen += len(ec)
    assert seen > 20   # the off-by-several consensus has candidates
    # all four at once, each under a source of its own, the last with its reference and mask
    sources = [1, 0, 2, 4]
    got = engine.candidates([b for b, _ in ids], scores, sources, md, ref_slots=[-1, -1, -1, ids[3][1]],
                            masks=[None, None, None, fmask], with_counts=True)
    for c, src in enumerate(sources):
        ec, eh = todays_path(engine, ids[c][0], ids[c][1] if c == 3 else -1, cases[c].t, scores[c], src, md, fmask)
        H.same(got[c][0], ec)
        H.same(got[c][1], eh)
        assert got[c][2:] == (len(ec), len(eh))
    assert got[3][2] > 0
    # counts and chosen only
    few = engine.candidates([b for b, _ in ids], scores, sources, md, ref_slots=[-1, -1, -1, ids[3][1]],
                            masks=[None, None, None, fmask], cand_cap=False, with_counts=True)
    assert [(r[0], r[2], r[3]) for r in few] == [(None, r[2], r[3]) for r in got]
    for a, b in zip(few, got):
        H.same(a[1], b[1])


def raw(engine, groups, scores, sources, refs=None):
    slot_off = np.zeros(len(groups) + 1, np.int32)
    slot_off[1:] = np.cumsum([len(g) for g in groups])
    slots = np.ascontiguousarray(np.concatenate(groups), np.int32)
    io = _lib.CandidateIO([1] * len(groups), scores, sources, 3, cand_cap=False, chosen_cap=False)
    rp = None if refs is None else np.ascontiguousarray(refs, np.int32)
    rc = engine.lib.rf_candidates(engine.ctx, len(groups), ptr(slot_off), ptr(slots), ptr(rp), ptr(io.scores),
                                  ptr(io.sources), None, 3, *io.args())
    return rc, engine.lib.rf_last_error(engine.ctx).decode(), io.counts


def test_refusals(engine):
    """Unknown slots and stale bands are refused as rf_score_dense refuses
    them, and a refused call changes nothing: the same good call before and
    after gives the same records."""
    rng = np.random.default_rng(77)
    t = random_seq(40, rng)
    cs = Case(off_consensus(t, rng, 2), [make_read(t, rng, bandwidth=9) for _ in range(3)],
              reference(40, 6, rng, CODON))
    (b, r), = load(engine, [cs])
    good = engine.candidates([b], [-1e9], [1], 3, with_counts=True)
    assert good[0][2] > 0

    def dense_refusal(groups):
        pg = np.ascontiguousarray(np.concatenate(groups), np.int32)
        off = np.array([0, len(pg)], np.int32)
        return engine.lib.rf_score_dense(engine.ctx, 1, ptr(off), ptr(pg), None), \
            engine.lib.rf_last_error(engine.ctx).decode()

    def still_fine():
        again = engine.candidates([b], [-1e9], [1], 3, with_counts=True)
        assert_same_results(again, good)

    unknown = [np.array([b[0], 10 ** 6], np.int32)]
    rc, msg, _ = raw(engine, unknown, [0.0], [0])
    assert (rc, msg) == dense_refusal(unknown) and rc == RF_ERR_ARG and "unknown slot" in msg
    still_fine()
    rc, msg, _ = raw(engine, [b], [0.0], [0], refs=[10 ** 6])
    assert rc == RF_ERR_ARG and "unknown reference slot" in msg
    still_fine()
    rc, msg, _ = raw(engine, [b], [0.0], [7])
    assert rc == RF_ERR_ARG and "unknown source" in msg
    rc, msg, _ = raw(engine, [b], [0.0], [4])
    assert rc == RF_ERR_ARG and "needs a mask" in msg
    still_fine()
    # the template uploaded again after the fill: stale for every source
    engine.set_templates(0, [cs.t])
    for src in (0, 1, 3):
        rc, msg, _ = raw(engine, [b], [0.0], [src])
        assert (rc, msg) == dense_refusal([b]) and rc == RF_ERR_STATE and "template changed" in msg
    k = np.concatenate([b, [r]])
    engine.realign(k, k, 0, [s.bandwidth for s in cs.reads + [cs.ref]], RF_FWD | RF_BWD)
    still_fine()
    # a read uploaded again
    engine.set_sequences(int(b[0]), [cs.reads[0]])
    rc, msg, _ = raw(engine, [b], [0.0], [1])
    assert (rc, msg) == dense_refusal([b]) and rc == RF_ERR_STATE and "sequence changed" in msg
    engine.realign(k, k, 0, [s.bandwidth for s in cs.reads + [cs.ref]], RF_FWD | RF_BWD)
    still_fine()


# ------------------------------------------------ the native driver under key 35

def driver_clusters():
    from rifraf_amd.sample import sample_sequences
    out = []
    for seed in (1, 2, 3):
        rng = np.random.default_rng(seed)
        _, _, _, reads, _, phreds, _, _ = sample_sequences(8, 120, error_rate=0.03, rng=rng)
        out.append(dict(dnaseqs=reads, phreds=phreds))
    rng = np.random.default_rng(4)
    ref, _, _, reads, _, phreds, _, _ = sample_sequences(8, 120, error_rate=0.02, ref_error_rate=0.1,
                                                         ref_errors=ErrorModel(10, 0, 0, 1, 1), rng=rng)
    ref = np.asarray(ref, np.uint8)
    ref = np.concatenate([ref[:50], ref[51:90], [2], ref[90:]]).astype(np.uint8)   # a frameshift and its repair
    out.append(dict(dnaseqs=reads, phreds=phreds, reference=ref))
    return out


@pytest.mark.parametrize("pset", ("aligned", "all_proposals"))
def test_native_driver_same_under_both_values(engine, opts, pset):
    from rifraf_amd.batch import rifraf_batch
    from rifraf_amd.model import RifrafParams
    from test_sharded import assert_same_run, summary
    extra = dict(batch_size=0, batch_fixed=False) if pset == "aligned" else dict(
        batch_size=0, batch_fixed=False, do_alignment_proposals=False, max_iters=20)
    params = RifrafParams(scores=PLAIN, **extra)
    clusters = driver_clusters()
    runs = []
    for value in (0, 1):
        opts("cand_device", value)
        runs.append(rifraf_batch(clusters, params=params, engine=engine, native=True, device_qv=False))
    if pset == "aligned":
        assert any(r.state.stage_iterations[1] > 0 for r in runs[0])   # FRAME ran
    for a, b in zip(*runs):
        assert_same_run(summary(a), summary(b))
        assert list(a.state.stage_iterations) == list(b.state.stage_iterations)
        assert [len(s) for s in a.consensus_stages] == [len(s) for s in b.consensus_stages]
        assert [(s.bandwidth, s.bandwidth_fixed) for s in a.state.sequences] == \
            [(s.bandwidth, s.bandwidth_fixed) for s in b.state.sequences]
        if a.state.reference is not None and len(a.state.reference):
            assert (a.state.reference.bandwidth, a.state.n_ref_indel_mults) == \
                (b.state.reference.bandwidth, b.state.n_ref_indel_mults)
