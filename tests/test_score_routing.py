"""The scoring entry points' routing and refusals on the GPU.

1. One small launch on each side of the scorer choice (k_score_ws, the
   general k_score for a -Inf table entry, k_score_segl for wide bands),
   bit-exact against the oracle, with rf_last_score_launch naming the scorer.
2. The return code of every refusal of a slot, for each call that reads
   bands as an alignment.  The codes are those of the engine before the
   scoring planner was factored out, read from its source.
"""
import numpy as np
import pytest

import oracle
from _util import SEQ_SCORES, all_proposals_arrays, assert_score_launch, dense_slot, make_read, random_seq
from rifraf_amd import RifrafSequence
from rifraf_amd._lib import ptr
from rifraf_amd.engine import RF_BWD, RF_FWD, RifrafError

pytestmark = pytest.mark.gpu


def dense_mask(t):
    mask = np.ones((len(t) + 1, 9), bool)
    mask[0, :5] = False                       # p = 0 has no sub / del
    mask[np.arange(1, len(t) + 1), t] = False   # not a proposal
    return mask


def test_three_groups_on_each_side_of_the_scorer_choice(engine, opts):
    for k, v in (("score_kernel", "auto"), ("score_mode", "auto"), ("lean_lds_kb", 0), ("band_pad", 64)):
        opts(k, v)
    rng = np.random.default_rng(1027)
    tpls = [random_seq(L, rng) for L in (27, 33, 40)]
    counts = (1, 3, 2)
    tpl_of = np.repeat(np.arange(3), counts)
    n = len(tpl_of)
    groups = np.split(np.arange(n), np.cumsum(counts)[:-1])
    base = [make_read(tpls[c], rng, 0.04, 4) for c in tpl_of]
    lp = base[2].error_log_p.copy()
    lp[len(lp) // 2] = 0.0                    # Phred 0: match = -Inf
    inf = list(base)
    inf[2] = RifrafSequence(base[2].seq, lp, 4, SEQ_SCORES)
    assert np.isinf(inf[2].match_scores).any() and not any(np.isinf(r.match_scores).any() for r in base)
    wide = [RifrafSequence(r.seq, r.error_log_p, 18, SEQ_SCORES) for r in base]
    engine.release_bands()
    engine.set_templates(0, tpls)
    sl = np.arange(n)
    for reads, bw, kernel in ((base, 4, "ws"), (inf, 4, "general"), (wide, 18, "seg")):
        engine.set_sequences(0, reads)
        engine.realign(sl, sl, tpl_of, [bw] * n, RF_FWD | RF_BWD)
        got = engine.score_dense(groups)
        # 3 items (one per group) of at most 3 reads: split
        assert_score_launch(engine, kernel, "split")
        assert engine.last_score_launch().items == 3
        props = [all_proposals_arrays(t) for t in tpls]
        tots = engine.score([(groups[c], -1, props[c]) for c in range(3)])
        assert_score_launch(engine, kernel, "split")
        for c, t in enumerate(tpls):
            exp, _ = oracle.cpu_pass(t, [reads[i] for i in groups[c]], nthreads=1)
            mask = dense_mask(t)
            np.testing.assert_array_equal(got[c][mask], exp[mask], err_msg=f"{kernel} group {c}")
            k, p, b = props[c]
            np.testing.assert_array_equal(tots[c], exp[p, dense_slot(k, b)], err_msg=f"{kernel} group {c}")


# ---------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------
OK, ARG, STATE = 0, -1, -4
M = 30
GOOD, OTHER_TPL, NO_BANDS, FAILED, MIXED, TPL_REPLACED, SEQ_REPLACED, LAST = 0, 2, 3, 4, 5, 6, 7, 8
UNKNOWN = 1 << 30   # past every slot any test of the session's engine has filled
# fault: (the slot that has it, then the code of each call given that slot beside a good one).
# score, dense, dense_ref: as a batch slot; score_ref, dense_ref_ref: as the reference slot.
# rf_backtrace has no groups, rf_aln_error_sums' groups no template of their own (equal lengths
# pass), and both, like rf_alignment_proposals, read the A band alone: a B band of another
# alignment or of another template is nothing to them.
CALLS = ("score", "score_ref", "dense", "dense_ref", "dense_ref_ref", "backtrace", "alignment_proposals",
         "aln_error_sums")
CODES = {
    "unknown slot":            (UNKNOWN,      (STATE, STATE, ARG,   ARG,   ARG,   STATE, STATE, STATE)),
    "slot without bands":      (NO_BANDS,     (STATE, STATE, STATE, STATE, STATE, STATE, STATE, STATE)),
    "failed fill":             (FAILED,       (STATE, STATE, STATE, STATE, STATE, STATE, STATE, STATE)),
    "A and B of two reads":    (MIXED,        (STATE, STATE, STATE, STATE, STATE, OK,    OK,    OK)),
    "replaced template":       (TPL_REPLACED, (STATE, STATE, STATE, STATE, STATE, STATE, STATE, STATE)),
    "replaced sequence":       (SEQ_REPLACED, (STATE, STATE, STATE, STATE, STATE, STATE, STATE, STATE)),
    "two templates in a group": (OTHER_TPL,   (ARG,   ARG,   ARG,   ARG,   ARG,   OK,    ARG,   OK)),
}


@pytest.fixture(scope="module")
def faulty(engine):
    """Slots 0-8 of one engine state, one fault each (see the constants)."""
    rng = np.random.default_rng(733)
    tpls = [random_seq(M, rng) for _ in range(3)]
    reads = [make_read(tpls[0], rng, 0.04, 4) for _ in range(8)]
    wall = RifrafSequence(reads[7].seq, reads[7].error_log_p, 4, SEQ_SCORES)
    for f in ("match_scores", "mismatch_scores", "ins_scores"):
        tab = np.array(getattr(wall, f), np.float64)
        tab[len(tab) // 2] = -np.inf         # a row that cannot be entered: the fill raises
        setattr(wall, f, tab)
    reads[7] = wall
    engine.release_bands()
    engine.set_sequences(0, reads)
    engine.set_templates(0, tpls)
    both = RF_FWD | RF_BWD
    #            slot: seq, template
    fills = {GOOD: (0, 0), 1: (1, 0), OTHER_TPL: (2, 1), MIXED: (3, 0), TPL_REPLACED: (5, 2), SEQ_REPLACED: (6, 0),
             LAST: (1, 0)}
    slots = np.array(sorted(fills))
    engine.realign(slots, [fills[s][0] for s in slots], [fills[s][1] for s in slots], [4] * len(slots), both)
    with pytest.raises(RifrafError, match="new score is invalid"):
        engine.realign([FAILED], [7], 0, [4], both)
    engine.realign([MIXED], [4], 0, [4], RF_BWD)              # B of another read
    engine.set_templates(2, [random_seq(M, rng)])
    engine.set_sequences(6, [make_read(tpls[0], rng, 0.04, 4)])
    a_read = {s: reads[q] for s, (q, _) in fills.items()}     # the read of each slot's A band
    return a_read


def call(engine, name, x, a_read):
    """The return code of the call `name` with slot x beside the good ones."""
    lib, ctx = engine.lib, engine.ctx
    i32 = lambda *v: np.array(v, np.int32)
    as_ref = name in ("score_ref", "dense_ref_ref")
    group = i32(GOOD, 1) if as_ref else i32(GOOD, x)
    off, ref = i32(0, 2), i32(x if as_ref else -1)
    dense = np.zeros((M + 1) * 9)
    if name in ("score", "score_ref"):
        out = np.zeros(1)
        return lib.rf_score(ctx, 1, ptr(off), ptr(group), ptr(ref), ptr(np.array([0, 1], np.int64)),
                            ptr(np.array([1], np.uint8)), ptr(i32(0)), ptr(np.array([0], np.uint8)), ptr(out), None)
    if name == "dense":
        return lib.rf_score_dense(ctx, 1, ptr(off), ptr(group), ptr(dense))
    if name in ("dense_ref", "dense_ref_ref"):
        return lib.rf_score_dense_ref(ctx, 1, ptr(off), ptr(group), ptr(ref), ptr(dense))
    if name == "backtrace":
        return lib.rf_backtrace(ctx, 2, ptr(group), None, None, ptr(i32(0, 0)), ptr(i32(0, 0)))
    if name == "alignment_proposals":
        return lib.rf_alignment_proposals(ctx, 1, ptr(off), ptr(group), 1, ptr(np.zeros((M + 1) * 9, np.uint8)))
    assert name == "aln_error_sums"
    rs = [a_read.get(int(s), a_read[GOOD]) for s in group]
    keep = [(np.ascontiguousarray(r.seq, np.uint8), np.ascontiguousarray(r.match_scores, np.float64)) for r in rs]
    return lib.rf_aln_error_sums(ctx, 1, ptr(off), ptr(group), ptr(i32(M)),
                                 ptr(np.array([b.ctypes.data for b, _ in keep], np.uint64)),
                                 ptr(np.array([m.ctypes.data for _, m in keep], np.uint64)),
                                 ptr(i32(*(len(b) for b, _ in keep))), ptr(np.zeros((M, 4))))


@pytest.mark.parametrize("fault", list(CODES))
def test_refusal_codes(engine, faulty, fault):
    x, codes = CODES[fault]
    got = {name: call(engine, name, x, faulty) for name in CALLS}
    assert got == dict(zip(CALLS, codes))
    # the state is as it was: the good slots still score
    assert call(engine, "dense", 1, faulty) == OK
