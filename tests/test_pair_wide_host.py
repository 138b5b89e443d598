"""The wide tier of the pair calls (RF_OPT_PAIR_WIDE) without a GPU: the
option's key in its three places, the host plan function
(rf_host_pair_wide_plan) against a restatement, the Python layer's wide=True
over the stand-in engine of test_pair_align_host, and calibrate_phreds_many
against model.calibrate_phreds read by read."""
import os
import re

import numpy as np
import pytest

from _util import SEQ_SCORES, make_read, random_seq
from rifraf_amd import RifrafSequence, _lib, model, pairalign
from rifraf_amd.engine import RF_SKEW, RifrafError
from test_pair_align_host import StandInEngine, oracle_moves

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(REPO, "include", "rifraf_hip.h")).read()
MAX_H = 1 << 24


def test_option_in_sync():
    assert int(re.search(r"#define RF_OPT_PAIR_WIDE\s+(\d+)", HEADER).group(1)) == 36
    assert _lib.OPTIONS["pair_wide"] == 36
    assert int(re.search(r"#define RF_OPT_PAIR_RING_MB\s+(\d+)", HEADER).group(1)) == _lib.OPTIONS["pair_ring_mb"] == 37
    assert len(set(_lib.OPTIONS.values())) == len(_lib.OPTIONS)
    assert re.search(r"#define RF_PAIR_WIDE_MAX_H \(1 << 24\)", HEADER) and _lib.PAIR_WIDE_MAX_H == MAX_H
    assert int(re.search(r"#define RF_ABI_VERSION (\d+)", HEADER).group(1)) == 1
    # the engine's option names are _lib.OPTIONS (Engine.set_option / get_option look the key up there)
    import inspect
    from rifraf_amd.engine import Engine
    assert '_lib.OPTIONS[name]' in inspect.getsource(Engine.set_option)


def restated(H, mode, budget):
    """pair_wide_plan in Python integers."""
    ld = max(H) + 6
    one = 4 * ld * (12 if mode == "count" else 8)
    nwg = max(1, min(len(H), budget // one))
    return nwg, ld, nwg * one


H_LISTS = [[5115], [5115, 5116], [5114, 5115, 5116, 5117] * 5, [5115] * 1000, [7, 40, 300, 5115, 5200],
           [20001] * 64, [MAX_H], [MAX_H, 5115, MAX_H - 1], [MAX_H] * 40]
BUDGETS = [0, 1, 1 << 20, 256 << 20, (256 << 20) - 1, 1 << 40]


@pytest.mark.parametrize("mode", _lib.PAIR_WIDE_MODES)
def test_plan_matches_restatement(mode):
    for H in H_LISTS:
        for budget in BUDGETS:
            p = _lib.host_pair_wide_plan(H, mode, budget)
            assert tuple(p) == restated(H, mode, budget), (H[:4], mode, budget)
            assert 1 <= p.nwg <= len(H)
            # at most the budget's number of workgroups, and never more ring than max(budget, one ring)
            one = p.ring_bytes // p.nwg
            assert p.nwg == 1 or p.nwg * one <= budget
            assert p.ring_bytes <= max(budget, one)
            # the ring holds the widest pair: 4 anti-diagonals of H + 6 doubles, and as many int32 with the counts
            assert p.ring_ld == max(H) + 6
            assert one == 4 * (max(H) + 6) * 8 + (4 * (max(H) + 6) * 4 if mode == "count" else 0)
    # the byte count needs 64 bits: 40 rings of 2^24 rows
    p = _lib.host_pair_wide_plan([MAX_H] * 40, "count", 1 << 40)
    assert p.nwg == 40 and p.ring_bytes == 40 * 4 * (MAX_H + 6) * 12 > 1 << 34
    # budget 0 is one workgroup
    assert _lib.host_pair_wide_plan([5115] * 9, "score", 0).nwg == 1


def test_plan_refusals():
    ok = np.array([5115], np.int32)
    out = [_lib.c_int64() for _ in range(3)]
    refs = [_lib.ctypes.byref(o) for o in out]
    lib = _lib.load()
    assert lib.rf_host_pair_wide_plan(1, _lib.ptr(ok), 0, 1 << 20, *refs) == 0
    for H in ([MAX_H + 1], [5115, MAX_H + 1], [0], [-3]):
        with pytest.raises(ValueError):
            _lib.host_pair_wide_plan(H, "score", 1 << 20)
    assert lib.rf_host_pair_wide_plan(0, _lib.ptr(ok), 0, 1 << 20, *refs) != 0
    assert lib.rf_host_pair_wide_plan(1, None, 0, 1 << 20, *refs) != 0
    assert lib.rf_host_pair_wide_plan(1, _lib.ptr(ok), 3, 1 << 20, *refs) != 0
    assert lib.rf_host_pair_wide_plan(1, _lib.ptr(ok), -1, 1 << 20, *refs) != 0
    assert lib.rf_host_pair_wide_plan(1, _lib.ptr(ok), 0, -1, *refs) != 0
    assert lib.rf_host_pair_wide_plan(1, _lib.ptr(ok), 0, 1 << 20, None, refs[1], refs[2]) != 0


class OptionEngine(StandInEngine):
    """The stand-in engine with the option calls; records what pair_wide was
    during each pair_align."""

    def __init__(self, fail=False):
        super().__init__()
        self.options, self.seen, self.fail = {"pair_wide": 0}, [], fail

    def set_option(self, name, value):
        old = self.options[name]
        self.options[name] = value
        return old

    def pair_align(self, *a, **kw):
        self.seen.append(self.options["pair_wide"])
        if self.fail:
            raise RifrafError("stand-in failure")
        return super().pair_align(*a, **kw)


def wide_pair(rng, H=pairalign.MAX_BAND_ROWS + 1):
    """12 bases against 12 + H - 5 at bandwidth 2: H rows."""
    t = random_seq(12 + H - 5, rng)
    s = RifrafSequence(random_seq(12, rng), np.full(12, -2.0), 2, SEQ_SCORES)
    assert 2 * 2 + abs(12 - len(t)) + 1 == H
    return t, s


def test_wide_passes_the_band_check_and_restores():
    rng = np.random.default_rng(3601)
    t, s = wide_pair(rng)
    e = OptionEngine()
    with pytest.raises(RifrafError) as err:
        pairalign.align_moves_many([s], [t], engine=e)
    assert str(pairalign.MAX_BAND_ROWS) in str(err.value) and e.seen == []
    got = pairalign.align_moves_many([s], [t], engine=e, wide=True)
    np.testing.assert_array_equal(got[0], oracle_moves(t, s, 2))
    assert e.seen == [1] and e.options["pair_wide"] == 0
    # a previous value comes back, also after an exception
    e = OptionEngine(fail=True)
    e.options["pair_wide"] = 7
    with pytest.raises(RifrafError):
        pairalign.align_moves_many([s], [t], engine=e, wide=True)
    assert e.seen == [1] and e.options["pair_wide"] == 7
    # wide=False does not touch the option
    e = OptionEngine()
    e.options["pair_wide"] = 7
    pairalign.align_moves_many([s], [random_seq(14, rng)], engine=e)
    assert e.seen == [7] and e.options["pair_wide"] == 7
    assert pairalign.MAX_BAND_ROWS == 5114


class ErrorsEngine(StandInEngine):
    """pair_errors on the oracle (no doubling) beside the option calls."""

    def __init__(self):
        super().__init__()
        self.wide, self.seen = 0, []

    def set_option(self, name, value):
        assert name == "pair_wide"
        old, self.wide = self.wide, value
        return old

    def pair_errors(self, seqs, tpls, bws, thresholds=None, fixed=None, max_doublings=0, flags=0):
        assert thresholds is None and max_doublings == 0
        self.seen.append((self.wide, flags))
        sc, _, nerr = self.pair_align(seqs, tpls, bws, flags, want_moves=False)
        return sc, nerr, np.asarray(bws, np.int32), np.ones(len(nerr), np.int32)


def test_calibrate_phreds_many_equals_the_model():
    rng = np.random.default_rng(3602)
    cons = random_seq(60, rng)
    reads = [make_read(cons, rng, 0.1).seq for _ in range(5)] + [cons.copy(), random_seq(41, rng)]
    phreds = [rng.integers(3, 40, len(r)).astype(np.int8) for r in reads]
    e = ErrorsEngine()
    got = pairalign.calibrate_phreds_many(reads, phreds, cons, engine=e)
    assert e.seen == [(1, RF_SKEW)] and e.wide == 0
    assert e.calls[0][1] == [0] * len(reads)   # one consensus, uploaded once
    import math
    assert e.calls[0][2] == [int(math.ceil(min(len(cons), len(r)) * 0.5)) for r in reads]

    def edit_distance(t, s, scratch=None):
        rs = RifrafSequence(s, np.full(len(s), -1.0), int(math.ceil(min(len(t), len(s)) * 0.5)),
                            pairalign.Scores.from_errors(pairalign.ErrorModel(1.0, 1.0, 1.0)))
        import oracle
        return oracle.count_errors(oracle_moves(t, rs, rs.bandwidth, skew=True), t, s)

    import rifraf_amd.align as align_mod
    old = align_mod.edit_distance
    align_mod.edit_distance = edit_distance   # model.calibrate_phreds imports it at call time
    try:
        exp = [model.calibrate_phreds(r, p, cons) for r, p in zip(reads, phreds)]
    finally:
        align_mod.edit_distance = old
    assert len(got) == len(exp)
    for g, x in zip(got, exp):
        assert g.dtype == np.float64 and np.array_equal(g.view(np.int64), x.view(np.int64))
    assert got[5].sum() == 0.0   # the consensus itself: no errors
    assert pairalign.calibrate_phreds_many([], [], cons, engine=e) == []
    with pytest.raises(ValueError):
        pairalign.calibrate_phreds_many(reads, phreds[:2], cons, engine=e)
    import rifraf_amd
    assert rifraf_amd.calibrate_phreds_many is pairalign.calibrate_phreds_many
