"""Whole runs over tiny clusters: 1-6 reads of 1-15 bases, some with a
reference of 1-15 bases.  The clusters of test_batch.py and test_workloads.py
are sampled from one template at 1-5 % error with reads of 40-450 bases, so no
whole run there has a consensus of 1-3 bases, a read shorter than a codon,
candidates that tie, a random batch drawn from 2 or 3 reads, a reference
shorter than the band or a consensus that empties.  Here a fixed-seed
generator makes N_CLUSTERS such clusters, and the two drivers of
rifraf_batch on the HIP engine -- the native lockstep stage machine
(rf_rifraf_batch / rf_rifraf_batch_ref) and the Python stage machine behind
the hub -- are held to separate rifraf() runs on the CPU oracle engine, bit
for bit.

The oracle runs are made once per session (oracle_runs).  The tests that are
not marked `gpu` assert, from the oracle runs alone, that the generator
reaches what it is for; the counts they saw are the constants below.

A cluster whose accepted candidates remove every base of the consensus ends
with model.EMPTY_CONSENSUS under every driver.  Those
clusters are left out of the parity calls and run in a call of their own
(test_emptied_consensus_is_refused_and_leaves_no_state).
"""
import re

import numpy as np
import pytest

from test_batch import REF_PARAMS, _params, _same_batches
from test_sharded import QV_RTOL, assert_same_run, summary

SEED = 4
N_CLUSTERS = 300
CLASSES = ("edit", "unrelated", "tie")
REF_KINDS = ("short", "indel", "random")
MAX_READS, MAX_LEN = 6, 15

# name -> (RifrafParams overrides on test_batch._params(), reference clusters only)
PSETS = {
    "fixed_batch": (dict(max_iters=30), False),                                       # the default batch
    "all_reads": (dict(batch_size=0, batch_fixed=False, max_iters=30), False),
    "random_batch": (dict(batch_size=2, batch_fixed=False, batch_threshold=0.0, seed=5, max_iters=30), False),
    "max_iters3": (dict(max_iters=3), False),
    "throughput_qv": (dict(max_iters=30, **REF_PARAMS["throughput_qv"]), True),
    "random_refine": (dict(max_iters=30, **REF_PARAMS["random_refine"]), True),
}


# ---------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------
def _one_edit(base, rng):
    """A copy of `base` with one substitution, insertion or deletion that
    keeps its length within 1..MAX_LEN."""
    kinds = ["sub"] + (["ins"] if len(base) < MAX_LEN else []) + (["del"] if len(base) > 1 else [])
    kind = kinds[int(rng.integers(len(kinds)))]
    if kind == "ins":
        at = int(rng.integers(0, len(base) + 1))
        return np.concatenate([base[:at], [rng.integers(4)], base[at:]]).astype(np.uint8)
    at = int(rng.integers(0, len(base)))
    if kind == "del":
        return np.concatenate([base[:at], base[at + 1:]]).astype(np.uint8)
    out = base.copy()
    out[at] = (out[at] + rng.integers(1, 4)) % 4
    return out


def _runs(letters, rng):
    """Homopolymer runs over two letters, 1..MAX_LEN bases in all."""
    total = int(rng.integers(1, MAX_LEN + 1))
    runs = []
    while sum(runs) < total:
        runs.append(min(int(rng.integers(1, 5)), total - sum(runs)))
    return np.concatenate([np.full(r, letters[k % 2], np.uint8) for k, r in enumerate(runs)])


def generate(seed=SEED, n=N_CLUSTERS):
    """[(cluster kwargs of rifraf(), class, reference kind or None)].  The
    class cycles with the cluster index; every third group of three carries a
    reference, so a third of each class does.

    edit       copies of one base sequence with one edit each
    unrelated  reads drawn independently of each other
    tie        homopolymer runs over two letters at one Phred value, the
               reads one edit apart: candidates that tie exactly
               (test_small_geometry._tie_pair shows the idea)

    Phred values are 1..30: Phred 0 (match score -Inf) belongs to
    test_nonfinite_tiers.  References: `short` has 1-2 bases, `indel` is the
    cluster's base sequence (the first read of an `unrelated` cluster) with
    one insertion or deletion, so FRAME has work to do, `random` is unrelated
    to the reads."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        cls = CLASSES[i % len(CLASSES)]
        nreads = int(rng.integers(1, MAX_READS + 1))
        if cls == "tie":
            letters = rng.choice(4, 2, replace=False)
            base = _runs(letters, rng)
            reads = [base.copy() if k == 0 else _one_edit(base, rng) for k in range(nreads)]
            for r in reads:                      # an edit's new base stays within the two letters
                r[~np.isin(r, letters)] = letters[0]
            q = int(rng.integers(1, 31))
            phreds = [np.full(len(r), q, np.int8) for r in reads]
        else:
            base = rng.integers(0, 4, int(rng.integers(1, MAX_LEN + 1))).astype(np.uint8)
            if cls == "edit":
                reads = [_one_edit(base, rng) for _ in range(nreads)]
            else:
                reads = [rng.integers(0, 4, int(rng.integers(1, MAX_LEN + 1))).astype(np.uint8)
                         for _ in range(nreads)]
            phreds = [rng.integers(1, 31, len(r)).astype(np.int8) for r in reads]
        kw, ref_kind = dict(dnaseqs=reads, phreds=phreds), None
        if (i // len(CLASSES)) % 3 == 0:
            ref_kind = REF_KINDS[(i // (3 * len(CLASSES))) % len(REF_KINDS)]
            if ref_kind == "short":
                ref = rng.integers(0, 4, int(rng.integers(1, 3))).astype(np.uint8)
            elif ref_kind == "random":
                ref = rng.integers(0, 4, int(rng.integers(1, MAX_LEN + 1))).astype(np.uint8)
            else:
                stem = reads[0] if cls == "unrelated" else base
                ref = stem
                while len(ref) == len(stem):
                    ref = _one_edit(stem, rng)
            kw["reference"] = ref
        out.append((kw, cls, ref_kind))
    return out


_GENERATED = []


def clusters():
    if not _GENERATED:
        _GENERATED.extend(generate())
    return _GENERATED


def params_of(pset):
    p = _params()
    for k, v in PSETS[pset][0].items():
        setattr(p, k, v)
    return p


def members(pset):
    """Indices of the clusters a parameter set runs on."""
    return [i for i, (kw, _, _) in enumerate(clusters()) if "reference" in kw or not PSETS[pset][1]]


# ---------------------------------------------------------------------
# the oracle side: one rifraf() per cluster on OracleEngine, once per session
# ---------------------------------------------------------------------
class OracleRun:
    """result: the RifrafResult, or None where the run raised `error`;
    tied: handle_candidates calls whose best score two or more candidates
    share (the stable sort's order alone decides which is accepted)."""

    def __init__(self, result, error, tied):
        self.result, self.error, self.tied = result, error, tied
        self.summary = None if result is None else summary(result)


_ORACLE = {}


def oracle_runs(pset):
    """{cluster index: OracleRun} of a parameter set."""
    if pset in _ORACLE:
        return _ORACLE[pset]
    from oracle_engine import OracleEngine
    from rifraf_amd import model
    tied = [0]
    choose = model.choose_candidates

    def counting(candidates, min_dist):
        best = max(c.score for c in candidates)
        tied[0] += sum(c.score == best for c in candidates) >= 2
        return choose(candidates, min_dist)

    runs = {}
    model.choose_candidates = counting
    try:
        for i in members(pset):
            tied[0] = 0
            try:
                runs[i] = OracleRun(model.rifraf(params=params_of(pset), engine=OracleEngine(), **clusters()[i][0]),
                                    None, tied[0])
            except Exception as e:   # noqa: BLE001 -- the test asserts which errors these are
                runs[i] = OracleRun(None, e, tied[0])
    finally:
        model.choose_candidates = choose
    _ORACLE[pset] = runs
    return runs


def good(pset):
    return [i for i, r in oracle_runs(pset).items() if r.error is None]


def emptied(pset):
    return [i for i, r in oracle_runs(pset).items() if r.error is not None]


def coverage(pset):
    """What the oracle runs of a parameter set reach."""
    runs = oracle_runs(pset)
    ok = [(i, r.result) for i, r in runs.items() if r.error is None]
    return {
        "clusters": len(runs),
        "raised": len(runs) - len(ok),
        "consensus_len_1": sum(len(r.consensus) == 1 for _, r in ok),
        "consensus_len_le_3": sum(len(r.consensus) <= 3 for _, r in ok),
        "one_read": sum(len(clusters()[i][0]["dnaseqs"]) == 1 for i, _ in ok),
        "read_shorter_than_codon": sum(min(map(len, clusters()[i][0]["dnaseqs"])) < 3 for i, _ in ok),
        "three_reads": sum(len(clusters()[i][0]["dnaseqs"]) == 3 for i, _ in ok),   # random_batch draws 2 of them
        "frame": sum(r.state.stage_iterations[1] > 0 for _, r in ok),
        "penalty_increase": sum(r.state.n_ref_indel_mults >= 1 for _, r in ok),
        "refine": sum(r.state.stage_iterations[2] > 0 for _, r in ok),
        "unconverged": sum(not r.state.converged for _, r in ok),
        "batch_grew": sum(r.state.batch_size > r.state.base_batch_size for _, r in ok),
        "batch_below_reads": sum(len(r.state.batch_seqs) < len(clusters()[i][0]["dnaseqs"]) for i, r in ok),
        "tied_candidates": sum(runs[i].tied > 0 for i, _ in ok),
        "several_iterations": sum(sum(r.state.stage_iterations) > 1 for _, r in ok),
    }


# ---------------------------------------------------------------------
# what the generator reaches, from the oracle runs alone (no GPU)
# ---------------------------------------------------------------------
PER_CLASS = {"edit": 100, "unrelated": 100, "tie": 100}
PER_REF_KIND = {None: 198, "short": 36, "indel": 33, "random": 33}
# the clusters whose consensus empties (the only error of any oracle run), per
# parameter set: at most 1 % of the 300 and 2.9 % of the 102 with a reference
EMPTIED = {"fixed_batch": [153, 182, 261], "all_reads": [153, 182, 261], "random_batch": [153, 182],
           "max_iters3": [], "throughput_qv": [153, 182, 261], "random_refine": [153, 182, 261]}
MAX_RAISED_SHARE = 0.05
# coverage(pset) of the oracle runs with SEED; a test asserts at least half of
# each count it names, so a change of the generator that loses a condition
# fails while a different draw of the same kind passes
SEEN = {
    "fixed_batch": dict(consensus_len_1=16, consensus_len_le_3=62, one_read=50, read_shorter_than_codon=84,
                        three_reads=41, frame=72, penalty_increase=25, refine=72, unconverged=0, batch_grew=0,
                        batch_below_reads=41, tied_candidates=108, several_iterations=230),
    "all_reads": dict(consensus_len_1=16, consensus_len_le_3=61, one_read=50, read_shorter_than_codon=84,
                      three_reads=41, frame=70, penalty_increase=24, refine=70, unconverged=0, batch_grew=0,
                      batch_below_reads=0, tied_candidates=109, several_iterations=230),
    "random_batch": dict(consensus_len_1=18, consensus_len_le_3=64, one_read=50, read_shorter_than_codon=85,
                         three_reads=41, frame=73, penalty_increase=23, refine=73, unconverged=0, batch_grew=126,
                         batch_below_reads=111, tied_candidates=105, several_iterations=227),
    "max_iters3": dict(consensus_len_1=20, consensus_len_le_3=60, one_read=50, read_shorter_than_codon=87,
                       three_reads=42, frame=50, penalty_increase=23, refine=0, unconverged=128, batch_grew=0,
                       batch_below_reads=53, tied_candidates=91, several_iterations=233),
    "throughput_qv": dict(consensus_len_1=2, consensus_len_le_3=13, one_read=20, read_shorter_than_codon=26,
                          three_reads=10, frame=70, penalty_increase=24, refine=70, unconverged=0, batch_grew=0,
                          batch_below_reads=0, tied_candidates=53, several_iterations=90),
    "random_refine": dict(consensus_len_1=2, consensus_len_le_3=13, one_read=20, read_shorter_than_codon=26,
                          three_reads=10, frame=72, penalty_increase=25, refine=72, unconverged=0, batch_grew=0,
                          batch_below_reads=9, tied_candidates=54, several_iterations=90),
}
# the conditions each parameter set is there for, beyond those every set reaches
EVERY_SET = ("consensus_len_1", "consensus_len_le_3", "one_read", "read_shorter_than_codon", "three_reads", "frame",
             "penalty_increase", "tied_candidates", "several_iterations")
OWN = {"fixed_batch": ("refine", "batch_below_reads"), "all_reads": ("refine",),
       "random_batch": ("refine", "batch_grew", "batch_below_reads"), "max_iters3": ("unconverged",),
       "throughput_qv": ("refine",), "random_refine": ("refine", "batch_below_reads")}


def test_generator_shapes():
    """Clusters per class and per reference kind; no cluster above 6 reads or
    15 bases, reference included; no Phred 0; reads of 1 and 2 bases, one-read
    clusters and references shorter than a codon are there; the tie class is
    two letters at one Phred value; every cluster is within the native
    driver's scope."""
    from collections import Counter
    from rifraf_amd.batch import native_eligible
    cl = clusters()
    assert len(cl) == N_CLUSTERS
    assert Counter(c for _, c, _ in cl) == PER_CLASS
    assert Counter(k for _, _, k in cl) == PER_REF_KIND
    for kw, cls, kind in cl:
        assert 1 <= len(kw["dnaseqs"]) <= MAX_READS
        for s, p in zip(kw["dnaseqs"], kw["phreds"]):
            assert 1 <= len(s) <= MAX_LEN and len(p) == len(s) and p.min() >= 1 and s.max() <= 3
        if kind is not None:
            assert 1 <= len(kw["reference"]) <= (2 if kind == "short" else MAX_LEN)
        if cls == "tie":
            assert len(set(np.concatenate(kw["dnaseqs"]).tolist())) <= 2
            assert len(set(np.concatenate(kw["phreds"]).tolist())) == 1
    lens = Counter(len(s) for kw, _, _ in cl for s in kw["dnaseqs"])
    assert lens[1] >= 20 and lens[2] >= 20 and lens[MAX_LEN] >= 20
    assert Counter(len(kw["dnaseqs"]) for kw, _, _ in cl)[1] >= 30
    for pset in PSETS:
        assert native_eligible([cl[i][0] for i in members(pset)], params_of(pset)), pset


@pytest.mark.parametrize("pset", list(PSETS))
def test_oracle_runs_reach_what_the_generator_is_for(pset):
    """The oracle runs of each parameter set: at most 5 % of its clusters
    raise, every one of them model.EMPTY_CONSENSUS and nothing else (the
    clusters of EMPTIED); the rest reach at least half of every count of SEEN
    that the set is there for -- a final consensus of one base, one-read
    clusters, FRAME with a penalty increase, REFINE, accepted candidates whose
    best score is tied; a run that ends unconverged (max_iters3), a random
    batch below the read count that grows (random_batch)."""
    from rifraf_amd.engine import RifrafError
    from rifraf_amd.model import EMPTY_CONSENSUS
    runs = oracle_runs(pset)
    cov = coverage(pset)
    print(pset, cov)
    assert cov["clusters"] == len(members(pset)) == (102 if PSETS[pset][1] else N_CLUSTERS)
    for i in emptied(pset):
        e = runs[i].error
        assert type(e) is RifrafError and str(e) == EMPTY_CONSENSUS, (pset, i, repr(e))
    assert emptied(pset) == EMPTIED[pset]
    assert cov["raised"] <= MAX_RAISED_SHARE * cov["clusters"]
    for name in EVERY_SET + OWN[pset]:
        assert SEEN[pset][name] >= 2, (pset, name)              # the constant itself names a condition that is met
        assert cov[name] >= SEEN[pset][name] // 2, (pset, name, cov[name])
    if pset == "max_iters3":    # no run is long enough to empty its consensus or to reach REFINE
        assert cov["refine"] == 0
    # a consensus empties somewhere, in a tie cluster and in another one
    assert {clusters()[i][1] for ps in PSETS for i in EMPTIED[ps]} >= {"tie"}
    assert len({clusters()[i][1] for ps in PSETS for i in EMPTIED[ps]}) >= 2


# ---------------------------------------------------------------------
# the drivers on the HIP engine
# ---------------------------------------------------------------------
def assert_same_state(a, b, kw, what):
    """Beyond assert_same_run: the final batch in draw order and, with a
    reference, the penalty increases, the reference's error rate and
    bandwidth."""
    _same_batches(a, b)
    if "reference" in kw:
        assert a.state.n_ref_indel_mults == b.state.n_ref_indel_mults, what
        assert a.state.ref_error_rate == b.state.ref_error_rate or (
            np.isinf(a.state.ref_error_rate) and np.isinf(b.state.ref_error_rate)), what
        assert a.state.reference.bandwidth == b.state.reference.bandwidth, what


@pytest.mark.gpu
@pytest.mark.parametrize("pset", list(PSETS))
def test_native_and_hub_equal_oracle_runs(run_engine, pset):
    """One rifraf_batch call per driver over every cluster of the parameter
    set whose oracle run ends: the native driver with the host quality pass
    (device_qv=False) and the Python stage machine behind the hub, both on the
    HIP engine, against the oracle runs -- consensus at every iteration and
    stage, score bits, stage iterations, convergence, QVs, the final batch and
    the reference's record, bit for bit."""
    from rifraf_amd.batch import rifraf_batch
    idx = good(pset)
    cl = [clusters()[i][0] for i in idx]
    runs = oracle_runs(pset)
    hub = rifraf_batch(cl, params=params_of(pset), engine=run_engine, native=False)
    nat = rifraf_batch(cl, params=params_of(pset), engine=run_engine, native=True, device_qv=False)
    assert len(hub) == len(nat) == len(idx)
    for i, kw, h, n in zip(idx, cl, hub, nat):
        o = runs[i]
        try:
            assert_same_run(summary(n), summary(h))
            assert_same_run(summary(n), o.summary)
            assert_same_state(n, h, kw, "native / hub")
            assert_same_state(n, o.result, kw, "native / oracle")
        except AssertionError as e:
            raise AssertionError(f"{pset}: cluster {i} ({clusters()[i][1]}, reference {clusters()[i][2]}): {e}") from e


@pytest.mark.gpu
@pytest.mark.parametrize("pset", list(PSETS))
def test_device_qvs_within_project_tolerance(run_engine, pset):
    """The native driver's default quality pass (k_aln_sums / k_aln_marks /
    k_aln_fold and k_qv at consensus lengths 1..15) against the oracle runs:
    everything but the QVs bit for bit, the QVs within test_sharded's QV_RTOL
    / QV_ATOL."""
    from rifraf_amd.batch import rifraf_batch
    idx = good(pset)
    cl = [clusters()[i][0] for i in idx]
    runs = oracle_runs(pset)
    got = rifraf_batch(cl, params=params_of(pset), engine=run_engine, native=True)
    for i, kw, g in zip(idx, cl, got):
        try:
            assert_same_run(summary(g), runs[i].summary, qv_rtol=QV_RTOL)
            assert_same_state(g, runs[i].result, kw, "native / oracle")
        except AssertionError as e:
            raise AssertionError(f"{pset}: cluster {i}: {e}") from e


@pytest.mark.gpu
@pytest.mark.parametrize("pset", list(PSETS))
def test_native_same_under_both_cand_device_values(run_engine, opts, pset):
    """RF_OPT_CAND_DEVICE 0 (candidates chosen on the host) and 1 (k_cand_select
    / k_cand_choose over ragged groups of 1-6 slots): identical runs."""
    from rifraf_amd.batch import rifraf_batch
    idx = good(pset)
    cl = [clusters()[i][0] for i in idx]
    both = []
    for value in (0, 1):
        opts("cand_device", value)
        both.append(rifraf_batch(cl, params=params_of(pset), engine=run_engine, native=True, device_qv=False))
    for i, kw, a, b in zip(idx, cl, *both):
        try:
            assert_same_run(summary(a), summary(b))
            assert_same_state(a, b, kw, "cand_device 0 / 1")
            assert [(s.bandwidth, s.bandwidth_fixed) for s in a.state.sequences] == \
                [(s.bandwidth, s.bandwidth_fixed) for s in b.state.sequences]
        except AssertionError as e:
            raise AssertionError(f"{pset}: cluster {i}: {e}") from e


@pytest.mark.gpu
@pytest.mark.parametrize("native", [True, False], ids=["native", "hub"])
@pytest.mark.parametrize("pset", [p for p in PSETS if EMPTIED[p]])
def test_emptied_consensus_is_refused_and_leaves_no_state(run_engine, pset, native):
    """The clusters whose consensus empties, between two clusters that end, in
    one rifraf_batch call per driver: the call raises model.EMPTY_CONSENSUS
    (the host check stops the cluster before any template of length 0 is
    uploaded), and the next call on the same engine, with the two good
    clusters alone, gives the oracle's runs."""
    from rifraf_amd.batch import rifraf_batch
    from rifraf_amd.engine import RifrafError
    from rifraf_amd.model import EMPTY_CONSENSUS
    runs = oracle_runs(pset)
    ok = good(pset)
    with_ref = [i for i in ok if "reference" in clusters()[i][0]]
    pair = [with_ref[0], next(i for i in ok if i != with_ref[0])]
    mixed = [pair[0]] + EMPTIED[pset] + [pair[1]]
    kwargs = dict(params=params_of(pset), engine=run_engine, native=native, device_qv=False)
    with pytest.raises(RifrafError, match="^" + re.escape(EMPTY_CONSENSUS) + "$"):
        rifraf_batch([clusters()[i][0] for i in mixed], **kwargs)
    after = rifraf_batch([clusters()[i][0] for i in pair], **kwargs)
    for i, g in zip(pair, after):
        assert_same_run(summary(g), runs[i].summary)
        assert_same_state(g, runs[i].result, clusters()[i][0], "after the refused call")
