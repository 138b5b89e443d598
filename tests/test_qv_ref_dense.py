"""The quality pass with the reference (use_ref_for_qvs) through the dense
table: estimate_probs calls the engine's score_dense_ref when it has one and
the proposal list otherwise, with the same result."""
import numpy as np
import pytest

from rifraf_amd import ErrorModel, RifrafParams, RifrafSequence, Scores, rifraf
from rifraf_amd.engine import RifrafError
from rifraf_amd.model import RifrafState, _Run, estimate_probs, score_proposal_arrays
from rifraf_amd.proposals import DEL, SUB
from rifraf_amd.sample import random_seq, sample_sequences


class Counting:
    """An engine proxy that counts score_dense_ref calls."""

    def __init__(self, eng):
        self.e = eng
        self.dense_ref_calls = 0
        self.list_ref_calls = 0

    def __getattr__(self, name):
        return getattr(self.e, name)

    def score_dense_ref(self, groups, ref_slots, to_host=True, rows=None):
        self.dense_ref_calls += 1
        return self.e.score_dense_ref(groups, ref_slots, to_host, rows)


@pytest.mark.gpu
def test_qv_pass_with_reference_matches_oracle(engine):
    """A whole run with use_ref_for_qvs on the HIP engine and on the oracle
    engine: equal error_probs and aln_error_probs, and the HIP run took the
    dense route (no silent fallback to the list)."""
    from oracle_engine import OracleEngine
    rng = np.random.default_rng(41)
    ref, _, _, reads, _, phreds, _, _ = sample_sequences(
        8, 120, error_rate=0.01, ref_error_rate=0.1, ref_errors=ErrorModel(10, 0, 0, 1, 1), rng=rng)
    params = RifrafParams(seed=1, do_score=True, use_ref_for_qvs=True)
    proxy = Counting(engine)
    a = rifraf(reads, phreds, reference=ref, params=params, engine=proxy)
    b = rifraf(reads, phreds, reference=ref, params=params, engine=OracleEngine())
    assert not hasattr(OracleEngine, "score_dense_ref")
    np.testing.assert_array_equal(a.consensus, b.consensus)
    for f in ("sub", "dele", "ins"):
        np.testing.assert_array_equal(getattr(a.error_probs, f), getattr(b.error_probs, f), err_msg=f)
    np.testing.assert_array_equal(a.aln_error_probs, b.aln_error_probs)
    assert proxy.dense_ref_calls >= 1


# ---------------------------------------------------------------------
# routing, on a stand-in engine (no GPU)
# ---------------------------------------------------------------------
def slot_of(kind, base):
    return np.where(kind == SUB, base, np.where(kind == DEL, 4, 5 + base))


class ListOnly:
    """Scores a proposal list from a dense table, as rf_score gathers it."""

    def __init__(self, dense):
        self.dense = dense
        self.calls = []

    def score(self, groups, per_seq=False):
        (slots, ref, (kind, pos, base)), = groups
        self.calls.append(("score", list(slots), ref))
        tot = self.dense[pos.astype(np.int64), slot_of(kind.astype(np.int64), base.astype(np.int64))]
        if np.isnan(tot).any():
            raise RifrafError("failed to compute a valid score")
        return [tot]


class WithDense(ListOnly):
    def score_dense_ref(self, groups, ref_slots, to_host=True, rows=None):
        self.calls.append(("score_dense_ref", [list(g) for g in groups], list(ref_slots)))
        return [self.dense.copy()]


def stand_in_state(m, rng):
    cons = random_seq(m, rng)
    ref = RifrafSequence(random_seq(m, rng), np.full(m, -1.0), 3, Scores.from_errors(ErrorModel(10, 1e-1, 1e-1, 1, 1)))
    state = RifrafState(consensus=cons, ref_scores=None, reference=ref, batch_fixed_size=0, batch_size=2,
                        base_batch_size=2, sequences=[None, None], maxlen=0, score=-40.0, batch_seqs=[0, 1])
    dense = rng.uniform(-60.0, -45.0, (m + 1, 9))
    dense[0, :5] = np.nan
    return state, dense


def test_estimate_probs_routes_to_the_dense_call():
    rng = np.random.default_rng(42)
    state, dense = stand_in_state(17, rng)
    with_dense, list_only = WithDense(dense), ListOnly(dense)
    a = estimate_probs(state, _Run(with_dense, 2), True)
    b = estimate_probs(state, _Run(list_only, 2), True)
    assert with_dense.calls == [("score_dense_ref", [[0, 1]], [2])]
    assert list_only.calls == [("score", [0, 1], 2)]
    for f in ("sub", "dele", "ins"):
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)
    # without the reference the list path stays, whatever the engine has
    plain = WithDense(dense)
    c = estimate_probs(state, _Run(plain, 2), False)
    assert plain.calls == [("score", [0, 1], -1)]
    np.testing.assert_array_equal(c.sub, b.sub)
    # every proposal of the list reads a slot of the table
    kind, pos, base = score_proposal_arrays(17, state.consensus)
    assert len(kind) == 8 * 17 + 4


def test_nan_slots_on_the_dense_route():
    rng = np.random.default_rng(43)
    m = 11
    state, dense = stand_in_state(m, rng)
    own = dense.copy()
    own[np.arange(1, m + 1), np.asarray(state.consensus, np.int64)] = np.nan    # not proposals
    own[0, :5] = np.nan
    a = estimate_probs(state, _Run(WithDense(own), 2), True)
    b = estimate_probs(state, _Run(WithDense(dense), 2), True)
    for f in ("sub", "dele", "ins"):
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)
    for p, k in ((3, (int(state.consensus[2]) + 1) % 4), (5, 4), (0, 6), (m, 8)):
        bad = dense.copy()
        bad[p, k] = np.nan
        with pytest.raises(RifrafError, match="failed to compute a valid score"):
            estimate_probs(state, _Run(WithDense(bad), 2), True)
