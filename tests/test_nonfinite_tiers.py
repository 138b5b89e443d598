"""Non-finite score tables and raised fills in every kernel tier.

A read with one -Inf table entry (Phred 0, or an ErrorModel with a zero rate)
leaves every lean tier: its fills run in the general DP steps (k_dpx<true,
true>, k_dpr<NP> general, k_dp, k_dpm), its pairs in ps_gen_body and its
scoring in k_score.  The general tier is also the only one that can raise the
reference's "new score is invalid" (align.jl:105-110).  This module drives
each of those kernels with non-finite tables at the smallest shape that
reaches it, beside finite reads of the same class, and checks the engine's
state after a raise.

Every comparison is bit for bit against the oracle (NaN meets NaN).  What the
inputs are -- which ones fill, which ones raise, that every parity read is
non-finite -- is established from the oracle alone, on the CPU, before the
engine is touched (check_inputs).

A native wave in which exactly one cluster's fill raises cannot be built
within native_eligible's scope, so there is no test of it.  There every
read's tables come from its Phred scores and the one Scores object of the
call: mismatch, ins and del are lp + a score with lp finite, so a finite
Scores leaves every cell a finite way in (a Phred 0 only removes matches) and
no fill raises, and a Scores with a zero rate (-Inf) is refused for every
cluster alike by check_params ("scores must be between -Inf and 0.0") before
any fill (test_native_scope_has_no_raising_fill runs the candidates on the
CPU stage machine).  What a native wave does meet is non-finite reads in the
general tiers: test_native_wave_with_phred0_reads.
"""
import numpy as np
import pytest

import oracle
from _util import REF_SCORES, SEQ_SCORES, all_proposals_arrays, assert_score_launch, random_seq
from rifraf_amd import ErrorModel, RifrafSequence, Scores
from rifraf_amd.align import moves_to_aligned_seqs, moves_to_indices, moves_to_proposals_np
from rifraf_amd.engine import RF_BAND_A, RF_BAND_B, RF_BWD, RF_FWD, RF_SKEW, RF_TRIM, RifrafError
from rifraf_amd.errormodel import phred_to_log_p
from rifraf_amd.model import _add_base_distributions
from rifraf_amd.sample import sample_from_template
from test_gpu_parity import assert_band_equal, launched_tasks
from test_pair_scores import bits_equal, final_cell
from test_score_dense_ref import dense_mask, same, table
from test_sharded import QV_RTOL, assert_same_run, summary

pytestmark = pytest.mark.gpu

LP_TABLE = phred_to_log_p(np.arange(256, dtype=np.uint8).view(np.int8))
with np.errstate(divide="ignore", invalid="ignore"):
    MATCH_TABLE = np.log10(1.0 - np.power(10.0, LP_TABLE))
ZERO_INDEL = Scores.from_errors(ErrorModel(1.0, 0.0, 0.0, 1.0, 1.0))   # ins = del = -Inf everywhere
INVALID = "new score is invalid"
FILL_FAILED = "the last fill of this band failed"
DNS = (0, 3, -4)      # n - m of the reads of every call

# tier -> (options, m, bw): H = 2 bw + |n - m| + 1 over DNS
TIERS = {
    "dpx31": ({}, 40, 12),                   # H 25..29
    "dpx63": ({}, 80, 24),                   # H 49..53
    "dpx127": ({}, 140, 45),                 # H 91..95
    "dpr1": ({"dp_nl64": 0}, 40, 12),
    "dpr2": ({"dp_nl64": 0}, 80, 24),
    "dpr4": ({"dp_nl64": 0}, 140, 45),
    "dpr8": ({}, 260, 90),                   # H 181..185
    "dp64": ({"dp_np8": 0}, 260, 90),
    "dpring": ({}, 300, 135),                # H 271..275
    "dpm": ({"dp_mc": 1}, 2100, 1021),       # H 2043..2047
    "dpwide": ({"dp_mc": 0}, 2100, 1021),
}
H_RANGE = {"dpx31": (1, 31), "dpx63": (32, 63), "dpx127": (64, 127), "dpr1": (1, 31), "dpr2": (32, 63),
           "dpr4": (64, 127), "dpr8": (128, 255), "dp64": (128, 255), "dpring": (256, 300), "dpm": (2041, 2047),
           "dpwide": (2041, 2047)}
WIDE = ("dpm", "dpwide")
# tier -> the general kernel family (Engine.last_dp_launches: kernel, npi) that
# its non-lean fills run in: the non-finite reads', and every skew / trim fill
GENERAL_KERNELS = {"dpr", "dpx_codon", "dp64", "dpw_lds", "dpw_global", "dpm"}
TIER_KERNEL = {"dpx31": ("dpx_codon", 0), "dpx63": ("dpx_codon", 0), "dpx127": ("dpx_codon", 0),
               "dpr1": ("dpr", 0), "dpr2": ("dpr", 1), "dpr4": ("dpr", 2), "dpr8": ("dpr", 3),
               "dp64": ("dp64", 0), "dpring": ("dp64", 0), "dpm": ("dpm", 0), "dpwide": ("dpw_lds", 0)}
KINDS = ("phred0", "phred0-codes", "holes", "holes-codon")
FLAG_SETS = (RF_FWD | RF_BWD, RF_FWD | RF_SKEW, RF_FWD | RF_TRIM, RF_FWD | RF_SKEW | RF_TRIM)


def shape_seed(tier, kind):
    _, m, bw = TIERS[tier]
    return 7000 + 13 * m + bw + 101 * (KINDS + ("wall",)).index(kind)


# ---------------------------------------------------------------------
# 1. inputs
# ---------------------------------------------------------------------
def sampled(t, n, rng):
    """A read of exactly n bases made from the template (so matches matter),
    with its Phred scores (none of them 0)."""
    s, _, ph, _, _ = sample_from_template(t, np.full(len(t), 0.03), ErrorModel(1, 5, 5), 1.5, 1.0, 0.3, rng)
    s, ph = np.asarray(s, np.uint8), np.clip(np.asarray(ph, np.int64), 1, 60)
    if len(s) < n:
        k = n - len(s)
        s, ph = np.concatenate([s, random_seq(k, rng)]), np.concatenate([ph, np.full(k, 10)])
    return s[:n].copy(), ph[:n].astype(np.int8)


def own_tables(r):
    for f in ("match_scores", "mismatch_scores", "ins_scores", "del_scores", "codon_ins_scores",
              "codon_del_scores"):
        setattr(r, f, np.array(getattr(r, f), np.float64))
    return r


def pick(rng, n, frac, least=1, avoid=()):
    pool = np.setdiff1d(np.arange(n), np.asarray(avoid, np.int64))
    return rng.choice(pool, min(len(pool), max(least, int(round(frac * n)))), replace=False)


def holes_read(t, n, bw, rng, scores=SEQ_SCORES):
    """A finite read whose tables get -Inf insertions, deletions and
    mismatches (about 5 % each), and with codon tables a few -Inf codon
    entries.  The holes are placed so that every cell keeps a finite way in,
    in both directions: the first and the last column of a band are entered
    by insertions alone and its first and last row by deletions alone, so
    the rows that meet those columns keep their insertion scores (which
    leaves fewer than 5 % of the rows in the widest bands) and del_scores
    keeps its two ends; a cell on the band's lower edge has no deletion and
    one on its upper edge no insertion, so no row loses its mismatch
    together with its insertion or with a deletion beside it."""
    s, ph = sampled(t, n, rng)
    r = own_tables(RifrafSequence(s, ph, bw, scores))
    edge = bw + abs(n - len(t)) + 1
    ins = pick(rng, n, 0.05, avoid=np.r_[0:edge, n - edge:n])
    r.ins_scores[ins] = -np.inf
    mism = pick(rng, n, 0.05, avoid=ins)
    r.mismatch_scores[mism] = -np.inf
    r.del_scores[pick(rng, n + 1, 0.05, avoid=np.r_[0, n, mism, mism + 1])] = -np.inf
    if len(r.codon_ins_scores):
        r.codon_ins_scores[pick(rng, len(r.codon_ins_scores), 0.03)] = -np.inf
        r.codon_del_scores[pick(rng, len(r.codon_del_scores), 0.03)] = -np.inf
    return r


def wall_read(t, n, bw, rng, i0):
    """A holes read whose row i0 (0-based read position) cannot be entered:
    match = mismatch = ins = -Inf."""
    r = holes_read(t, n, bw, rng)
    r.match_scores[i0] = r.mismatch_scores[i0] = r.ins_scores[i0] = -np.inf
    return r


class Case:
    """One template with finite and non-finite reads of one H class, and the
    oracle's fills and walks of them, computed once (kept for the small
    tiers; the 2,100-base bands are recomputed per use)."""

    def __init__(self, tier, kind):
        _, m, bw = TIERS[tier]
        self.tier, self.kind, self.m, self.bw = tier, kind, m, bw
        rng = np.random.default_rng(shape_seed(tier, kind))
        self.t = random_seq(m, rng)
        self.coded = kind == "phred0-codes"
        dns = DNS
        fin = DNS     # finite reads beside them
        if kind.startswith("phred0"):
            raw = []
            for dn in dns:
                s, ph = sampled(self.t, m + dn, rng)
                ph[pick(rng, m + dn, 0.15)] = 0
                raw.append((s, ph))
            raw += [sampled(self.t, m + dn, rng) for dn in fin]
            self.off = np.zeros(len(raw) + 1, np.int64)
            np.cumsum([len(s) for s, _ in raw], out=self.off[1:])
            self.bases = np.concatenate([s for s, _ in raw])
            self.codes = np.concatenate([ph for _, ph in raw]).view(np.uint8)
            self.reads = [RifrafSequence(s, ph, bw, SEQ_SCORES) for s, ph in raw]
        else:
            sc = REF_SCORES if kind == "holes-codon" else SEQ_SCORES
            self.reads = [holes_read(self.t, m + dn, bw, rng, sc) for dn in dns]
            self.reads += [RifrafSequence(*sampled(self.t, m + dn, rng), bw, SEQ_SCORES) for dn in fin]
        self.nonfinite = list(range(len(dns)))
        self.keep = m < 1000
        self._memo = {}

    def upload(self, engine, first=0):
        if self.coded:
            assert engine.set_sequences_codes(first, self.bases, self.off, self.codes, LP_TABLE, MATCH_TABLE,
                                              SEQ_SCORES)
        else:
            engine.set_sequences(first, self.reads)

    def fwd(self, k, flags=0):
        """(A, moves, nerrors) of read k's forward fill."""
        key = ("f", k, flags & (RF_SKEW | RF_TRIM))
        if key in self._memo:
            return self._memo[key]
        r = self.reads[k]
        A, mv = oracle.forward(self.t, r, moves=True, skew=bool(flags & RF_SKEW), trim=bool(flags & RF_TRIM))
        w = oracle.backtrace(mv, len(r) + 1, self.m + 1, self.bw)
        out = (A, w, oracle.count_errors(w, self.t, r.seq))
        if self.keep:
            self._memo[key] = out
        return out

    def bwd(self, k):
        key = ("b", k)
        if key in self._memo:
            return self._memo[key]
        B = oracle.backward(self.t, self.reads[k])
        if self.keep:
            self._memo[key] = B
        return B


_CASES = {}


def case_of(tier, kind):
    """The case of a tier's shape; tiers of one shape share it."""
    _, m, bw = TIERS[tier]
    key = (m, bw, kind)
    if key not in _CASES:
        c = Case(tier, kind)
        check_inputs(c)
        _CASES[key] = c
    return _CASES[key]


def raises(fn):
    try:
        fn()
    except oracle.OracleError as e:
        assert str(e) == INVALID
        return True
    return False


def check_inputs(c):
    """From the oracle alone: every read has the tier's H, no parity read
    raises in any direction or flag set, and every non-finite read has a
    -Inf among match, mismatch, ins and del (S.finite is false), every
    other read none."""
    lo, hi = H_RANGE[c.tier]
    for k, r in enumerate(c.reads):
        H = 2 * c.bw + abs(len(r) - c.m) + 1
        assert lo <= H <= hi, (c.tier, H)
        tabs = np.concatenate([r.match_scores, r.mismatch_scores, r.ins_scores, r.del_scores])
        assert not np.isnan(tabs).any()
        assert np.isinf(tabs).any() == (k in c.nonfinite), (c.tier, c.kind, k)
        for fl in (0, RF_SKEW, RF_TRIM, RF_SKEW | RF_TRIM):     # an OracleError here fails the test
            c.fwd(k, fl)
        c.bwd(k)
    assert {len(r) - c.m for r in c.reads} == set(DNS)


class WallCase:
    """The raising inputs of a tier: a finite read, a wall read (row i0 near
    n / 2, near 3 n / 4 in the widest tiers) and a holes read, then a finite
    read for the slot the call does not name and a finite replacement for
    the wall's slot; `first_col`: the read that raises in the first column
    (insertions and deletions impossible, n = m + 1)."""

    def __init__(self, tier):
        _, m, bw = TIERS[tier]
        self.tier, self.m, self.bw = tier, m, bw
        rng = np.random.default_rng(shape_seed(tier, "wall"))
        self.t = random_seq(m, rng)
        n = m + 3
        self.i0 = (3 * n) // 4 if tier in WIDE else n // 2
        self.reads = [RifrafSequence(*sampled(self.t, m, rng), bw, SEQ_SCORES),
                      wall_read(self.t, n, bw, rng, self.i0),
                      holes_read(self.t, m - 4, bw, rng),
                      RifrafSequence(*sampled(self.t, m + 3, rng), bw, SEQ_SCORES),
                      RifrafSequence(*sampled(self.t, n, rng), bw, SEQ_SCORES)]
        s = np.concatenate([self.t, random_seq(1, rng)])
        self.first_col = RifrafSequence(s, np.full(len(s), -1.0), bw, ZERO_INDEL)
        self.good, self.wall, self.other, self.repl = (0, 2), 1, 3, 4
        lo, hi = H_RANGE[tier]
        for r in self.reads + [self.first_col]:
            assert lo <= 2 * bw + abs(len(r) - m) + 1 <= hi
        # the oracle: the wall raises in both directions, the first-column read
        # too; nothing else raises
        w = self.reads[self.wall]
        assert raises(lambda: oracle.forward(self.t, w)) and raises(lambda: oracle.backward(self.t, w))
        assert raises(lambda: oracle.forward(self.t, self.first_col))
        assert raises(lambda: oracle.backward(self.t, self.first_col))
        for k in (0, 2, 3, 4):
            assert not raises(lambda: oracle.forward(self.t, self.reads[k]))
            assert not raises(lambda: oracle.backward(self.t, self.reads[k]))


_WALLS = {}


def wall_of(tier):
    _, m, bw = TIERS[tier]
    if (m, bw) not in _WALLS:
        _WALLS[(m, bw)] = WallCase(tier)
    return _WALLS[(m, bw)]


def set_tier(opts, tier, pad=None):
    for k, v in TIERS[tier][0].items():
        opts(k, v)
    if pad is not None:
        opts("band_pad", pad)


def assert_tier_ran(engine, tier, general, lean):
    """The last rf_realign ran its `general` non-lean tasks in the tier's
    kernel and nowhere else, and its `lean` tasks (finite reads, no skew /
    trim) in lean kernels; above H 255 the tier's kernel takes those too."""
    got = launched_tasks(engine)
    wide = H_RANGE[tier][1] > 255
    non_lean = {k: c for k, c in got.items() if k[0] in GENERAL_KERNELS}
    assert non_lean == {TIER_KERNEL[tier]: general + (lean if wide else 0)}, (tier, got)
    assert sum(got.values()) - sum(non_lean.values()) == (0 if wide else lean), (tier, got)


def proposals_mask(t, walks, seqs):
    exp = np.zeros((len(t) + 1, 9), np.uint8)
    for w, s in zip(walks, seqs):
        k, p, b = moves_to_proposals_np(w, t, s.seq)
        exp[p, np.where(k == 0, b, np.where(k == 2, 4, 5 + b))] = 1
    return exp


def check_walks(engine, opts, t, reads, slots, walks):
    """rf_backtrace (4 waves and 1 per walk) and rf_alignment_proposals of
    `slots` against the oracle's walks (moves, nerrors)."""
    for nw in (4, 1):
        opts("bt_nw", nw)
        moves, nerr = engine.backtrace(slots)
        for k, (w, ne) in enumerate(walks):
            np.testing.assert_array_equal(moves[k], w, err_msg=f"slot {slots[k]} bt_nw {nw}")
            assert nerr[k] == ne, (slots[k], nw)
    mask = engine.alignment_proposals([np.asarray(slots, np.int32)], True)[0]
    np.testing.assert_array_equal(mask, proposals_mask(t, [w for w, _ in walks], reads))


# ---------------------------------------------------------------------
# 2. parity of the general tiers on non-finite tables
# ---------------------------------------------------------------------
PARITY = [(tier, kind) for tier in TIERS for kind in KINDS if tier not in WIDE or kind == "holes"]


@pytest.mark.parametrize("pad", [64, 1])
@pytest.mark.parametrize("tier,kind", PARITY)
def test_general_tier_parity(engine, opts, tier, kind, pad):
    """Bands, A[end, end], walks and proposal masks of three non-finite reads
    (n - m = 0, +3, -4) beside three finite reads of the same H class in one
    rf_realign: RF_FWD | RF_BWD, then forward fills with RF_SKEW, RF_TRIM
    and both (general for every read)."""
    c = case_of(tier, kind)
    set_tier(opts, tier, pad)
    c.upload(engine)
    engine.set_templates(0, [c.t])
    n = len(c.reads)
    sl = np.arange(n)
    for flags in FLAG_SETS:
        scores = engine.realign(sl, sl, 0, [c.bw] * n, flags)
        # three non-finite and three finite reads: lean only without skew / trim
        nf = len(c.nonfinite)
        assert_tier_ran(engine, tier, *((2 * nf, 2 * (n - nf)) if flags == RF_FWD | RF_BWD else (n, 0)))
        walks = []
        for k, r in enumerate(c.reads):
            A, w, ne = c.fwd(k, flags)
            assert_band_equal(engine.download_band(k, RF_BAND_A), A, len(r) + 1, c.m + 1, c.bw)
            assert bits_equal(scores[k:k + 1], [final_cell(A, len(r), c.m, c.bw)]), (k, flags)
            if flags & RF_BWD:
                assert_band_equal(engine.download_band(k, RF_BAND_B), c.bwd(k), len(r) + 1, c.m + 1, c.bw)
            walks.append((w, ne))
        check_walks(engine, opts, c.t, c.reads, list(range(n)), walks)


@pytest.mark.parametrize("how", ["marks", "one-launch", "host"])
@pytest.mark.parametrize("kind", ["phred0", "phred0-codes"])
def test_aln_error_sums_phred0(engine, opts, kind, how):
    """rf_aln_error_sums over Phred-0 reads, folded on the device in two
    launches and in one, and on the host: base_distribution summed in batch
    order over the oracle's walks.  Only row-coded reads are folded on the
    device: the "phred0" kind (uploaded as tables) takes the host fold under
    all three settings, and "phred0-codes" is what reaches k_aln_sums and
    k_aln_marks / k_aln_fold."""
    opts("aln_marks_min", 0 if how == "marks" else 128)
    opts("aln_sums_host", 1 if how == "host" else 0)
    for tier in ("dpx31", "dpx127"):
        c = case_of(tier, kind)
        c.upload(engine)
        engine.set_templates(0, [c.t])
        n = len(c.reads)
        sl = np.arange(n)
        engine.realign(sl, sl, 0, [c.bw] * n, RF_FWD | RF_BWD)
        exp = np.zeros((c.m, 4))
        _add_base_distributions(exp, [c.fwd(k)[1] for k in range(n)], c.reads)
        got = engine.aln_error_sums([sl.astype(np.int32)], [c.m], [c.reads])[0]
        assert same(got, exp).all(), (tier, kind, how)


# ---------------------------------------------------------------------
# 3. scoring with non-finite batch reads
# ---------------------------------------------------------------------
def oracle_scores(t, props, reads, As, Bs, ref=None):
    """(totals, per-read matrix) of a proposal list; a proposal the oracle
    raises on is NaN in both."""
    extra = () if ref is None else (oracle.forward(t, ref)[0], oracle.backward(t, ref), ref)
    try:
        return oracle.score_list(props, As, Bs, reads, t, *extra, per_seq=True, nthreads=1)
    except oracle.OracleError:
        pass
    k, p, b = props
    width = len(reads) + (ref is not None)
    tot, per = np.full(len(k), np.nan), np.full((len(k), width), np.nan)
    for j in range(len(k)):
        try:
            tot[j], per[j] = (x[0] for x in oracle.score_list((k[j:j + 1], p[j:j + 1], b[j:j + 1]), As, Bs, reads, t,
                                                              *extra, per_seq=True, nthreads=1))
        except oracle.OracleError:
            pass
    return tot, per


def check_list_scores(engine, group, ref_slot, props, tot, per):
    """rf_score of the proposals the oracle scores, totals and out_per_seq;
    the proposals it raises on make rf_score raise."""
    k, p, b = props
    ok = ~np.isnan(tot)
    got, mats = engine.score([(group, ref_slot, (k[ok], p[ok], b[ok]))], per_seq=True)
    assert same(got[0], tot[ok]).all()
    assert same(mats[0], per[ok]).all()
    if not ok.all():
        with pytest.raises(RifrafError, match="failed to compute a valid score"):
            engine.score([(group, ref_slot, (k[~ok], p[~ok], b[~ok]))])


@pytest.mark.parametrize("mode", ["fused", "split"])
@pytest.mark.parametrize("tier", ["dpx31", "dpx127", "dpring"])
def test_scoring_nonfinite_groups(engine, opts, tier, mode):
    """Groups with Phred-0 and holes reads among finite ones (k_score where
    finite tables would pick k_score_ws / k_score_segl): rf_score_dense,
    rf_score and rf_score_dense_ref (a finite codon reference, then a holes
    codon reference) against the oracle; then a finite-only group, which
    returns to the lean scorers."""
    opts("score_mode", mode)
    set_tier(opts, tier)
    p0 = case_of(tier, "phred0")
    m, bw = p0.m, p0.bw
    # batch reads: finite, Phred 0, finite, holes, Phred 0, finite (n - m: 0, +3, -4, 0, -4, +3);
    # references: slots 6, 7
    reads = [p0.reads[3], p0.reads[1], p0.reads[5], None, p0.reads[2], p0.reads[4]]
    rng = np.random.default_rng(shape_seed(tier, "holes") + 1)
    reads[3] = holes_read(p0.t, m, bw, rng)
    refs = [RifrafSequence(p0.reads[4].seq, p0.reads[4].error_log_p, bw, REF_SCORES),
            holes_read(p0.t, m + 3, bw, rng, REF_SCORES)]
    t = p0.t
    for r in reads + refs:
        assert not raises(lambda: oracle.forward(t, r)) and not raises(lambda: oracle.backward(t, r))
    assert [bool(np.isinf(np.concatenate([r.match_scores, r.mismatch_scores, r.ins_scores, r.del_scores])).any())
            for r in reads] == [False, True, False, True, True, False]
    assert np.isinf(np.concatenate([refs[1].ins_scores, refs[1].codon_ins_scores])).any()
    engine.release_bands()
    engine.set_sequences(0, reads + refs)
    engine.set_templates(0, [t])
    sl = np.arange(8)
    engine.realign(sl, sl, 0, [bw] * 8, RF_FWD | RF_BWD)
    As = [oracle.forward(t, r)[0] for r in reads]
    Bs = [oracle.backward(t, r) for r in reads]
    props = all_proposals_arrays(t)
    mask = dense_mask(t)
    # non-finite reads per group: 1 of 4, 2 of 5, 1 of 3, 2 of 3; the last group is finite only
    for group in ([0, 1, 2, 5], [0, 2, 3, 4, 5], [0, 4, 2], [1, 2, 3], [0, 2]):
        g = np.asarray(group, np.int32)
        rs = [reads[k] for k in group]
        tot, per = oracle_scores(t, props, rs, [As[k] for k in group], [Bs[k] for k in group])
        exp = table(t, props, tot)
        nfin = int(np.isfinite(exp[mask]).sum())
        print(f"{tier} {mode} group {group}: {nfin} of {int(mask.sum())} compared slots finite")
        assert 2 * nfin >= mask.sum()
        got = engine.score_dense([g])[0]
        assert_score_launch(engine, None if group == [0, 2] else "general", mode)
        assert same(got[mask], exp[mask]).all(), (tier, mode, group)
        check_list_scores(engine, g, -1, props, tot, per)
        if group == [0, 2]:
            continue
        for ref_slot in (6, 7):
            rtot, rper = oracle_scores(t, props, rs, [As[k] for k in group], [Bs[k] for k in group],
                                       refs[ref_slot - 6])
            rexp = table(t, props, rtot)
            nfin = int(np.isfinite(rexp[mask]).sum())
            print(f"{tier} {mode} group {group} reference {ref_slot}: {nfin} of {int(mask.sum())} compared slots "
                  f"finite")
            assert 2 * nfin >= mask.sum()
            got = engine.score_dense_ref([g], [ref_slot])[0]
            assert same(got[mask], rexp[mask]).all(), (tier, mode, group, ref_slot)
            check_list_scores(engine, g, ref_slot, props, rtot, rper)


# ---------------------------------------------------------------------
# 4. the same pairs without bands
# ---------------------------------------------------------------------
@pytest.mark.parametrize("walk", [1, 2])
@pytest.mark.parametrize("tier,kind", [(t, k) for t, k in PARITY if t not in ("dpr1", "dpr2", "dpr4", "dp64", "dpwide")])
def test_pairs_without_bands(engine, opts, tier, kind, walk):
    """rf_pair_scores, rf_pair_align and rf_pair_align_text (no doubling) of
    the parity reads and the tier's two raising reads: the bits, moves and
    counts of the banded fills, the host's texts and index maps of the
    oracle's moves; NaN / -1 / no bytes for the raising pairs, return 0."""
    opts("pair_walk", walk)
    c, w = case_of(tier, kind), wall_of(tier)
    # the parity reads as the kind uploads them (Phred codes: RF_TASK_CODED
    # pairs that are not finite), the two raising reads behind them as tables
    nc = len(c.reads)
    seqs = c.reads + [w.reads[w.wall], w.first_col]
    ours = (nc, nc + 1)      # the wall, the first-column read: on the wall case's template
    c.upload(engine)
    engine.set_sequences(nc, seqs[nc:])
    engine.set_templates(0, [c.t, w.t])
    ids = np.arange(len(seqs))
    tpl = np.array([1 if k in ours else 0 for k in ids])
    for flags in (0, RF_SKEW | RF_TRIM):
        exp, bad = {}, []
        for k in ids:
            if k in ours:
                try:
                    A, mv = oracle.forward(w.t, seqs[k], moves=True, skew=bool(flags), trim=bool(flags))
                except oracle.OracleError:
                    bad.append(k)
                    continue
                mv = oracle.backtrace(mv, len(seqs[k]) + 1, w.m + 1, w.bw)
                exp[k] = (final_cell(A, len(seqs[k]), w.m, w.bw), mv, oracle.count_errors(mv, w.t, seqs[k].seq))
            else:
                A, mv, ne = c.fwd(k, flags)
                exp[k] = (final_cell(A, len(seqs[k]), c.m, c.bw), mv, ne)
        assert ours[0] in bad and (flags or ours[1] in bad)
        sc = engine.pair_scores(ids, tpl, c.bw, flags)
        sc2, moves, nerr = engine.pair_align(ids, tpl, c.bw, flags)
        sc3, txt = engine.pair_align_text(ids, tpl, c.bw, max_doublings=0, flags=flags, want_indices=True)
        for k in ids:
            if k in bad:
                assert np.isnan(sc[k]) and np.isnan(sc2[k]) and np.isnan(sc3[k]), k
                assert moves[k] is None and nerr[k] == -1 and txt.text(k) is None and txt.indices(k) is None
                assert txt.nerrors[k] == -1
                continue
            s, mv, ne = exp[k]
            assert bits_equal([sc[k], sc2[k], sc3[k]], [s] * 3), (k, flags)
            np.testing.assert_array_equal(moves[k], mv)
            assert nerr[k] == ne and txt.nerrors[k] == ne
            assert txt.text(k) == moves_to_aligned_seqs(mv, w.t if k in ours else c.t, seqs[k].seq)
            assert txt.indices(k).tolist() == moves_to_indices(mv, c.m, len(seqs[k]))


# ---------------------------------------------------------------------
# 5. the raise, tier by tier, and the engine afterwards
# ---------------------------------------------------------------------
def refused(call, text=FILL_FAILED):
    with pytest.raises(RifrafError) as err:
        call()
    assert text in str(err.value), str(err.value)


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
@pytest.mark.parametrize("tier", list(TIERS))
def test_raise_and_state_after(engine, opts, tier, direction):
    """A wall job between good jobs of its class: the call raises, nothing it
    was to fill is readable until a later fill succeeds, slots it did not
    name stay current, the error does not leak into the next call, and the
    good jobs and the wall's slot refill."""
    w = wall_of(tier)
    set_tier(opts, tier)
    t, bw, m = w.t, w.bw, w.m
    flag = RF_FWD if direction == "fwd" else RF_BWD
    engine.release_bands()
    engine.set_sequences(0, w.reads)
    engine.set_templates(0, [t])
    # every slot current first: the good jobs, the replacement in the wall's slot, the slot left alone
    slots = np.array([0, 1, 2, 3], np.int32)
    engine.realign(slots, [0, w.repl, 2, w.other], 0, [bw] * 4, RF_FWD | RF_BWD)
    assert_tier_ran(engine, tier, 2, 6)       # the holes read's two fills in the tier's kernel
    ran = engine.last_dp_launches()
    fails = raises(lambda: (oracle.forward if direction == "fwd" else oracle.backward)(t, w.reads[w.wall]))
    assert fails
    # 1. the raise
    with pytest.raises(RifrafError, match=INVALID):
        engine.realign([0, 1, 2], [0, w.wall, 2], 0, [bw] * 3, flag)
    assert engine.last_dp_launches() == ran   # the launches of the last successful fill
    # 2. a failed fill leaves nothing readable
    props = all_proposals_arrays(t)
    good = np.array(w.good, np.int32)
    for s in (0, 1, 2):
        g = np.array([s], np.int32)
        rd = [w.reads[w.wall if s == 1 else s]]
        refused(lambda: engine.score([(g, -1, props)]))
        refused(lambda: engine.score_dense([g], rows=[m + 1]))
        refused(lambda: engine.qv_probs([g], [m], np.zeros(1)))
        if direction == "fwd":
            refused(lambda: engine.backtrace(g))
            refused(lambda: engine.alignment_proposals([g], True))
            refused(lambda: engine.aln_error_sums([g], [m], [rd]))
        # the cells are still there to look at
        which = RF_BAND_A if direction == "fwd" else RF_BAND_B
        assert engine.download_band(s, which).data.shape[1] == m + 1
    if direction == "bwd":
        # the A bands of the good jobs were not named: their walks still stand
        walks = []
        for s in w.good:
            _, mv = oracle.forward(t, w.reads[s], moves=True)
            wk = oracle.backtrace(mv, len(w.reads[s]) + 1, m + 1, bw)
            walks.append((wk, oracle.count_errors(wk, t, w.reads[s].seq)))
        check_walks(engine, opts, t, [w.reads[s] for s in w.good], list(w.good), walks)
    # 3. the error word does not leak: the slot the call did not name is current
    o = w.reads[w.other]
    Ao, mvo = oracle.forward(t, o, moves=True)
    if direction == "fwd" and tier not in WIDE:
        tot, _ = oracle_scores(t, props, [o], [Ao], [oracle.backward(t, o)])
        mask = dense_mask(t)
        assert same(engine.score_dense([[3]])[0][mask], table(t, props, tot)[mask]).all()
    else:
        wk = oracle.backtrace(mvo, len(o) + 1, m + 1, bw)
        moves, nerr = engine.backtrace([3])
        np.testing.assert_array_equal(moves[0], wk)
        assert nerr[0] == oracle.count_errors(wk, t, o.seq)
    # the good jobs alone: the fill succeeds and everything matches
    scores = engine.realign(good, good, 0, [bw] * 2, flag)
    refused(lambda: engine.score_dense([[1]], rows=[m + 1]))      # the wall's slot is still refused
    As, Bs, walks = [], [], []
    for k, s in enumerate(w.good):
        r = w.reads[s]
        A, mv = oracle.forward(t, r, moves=True)
        B = oracle.backward(t, r)
        assert_band_equal(engine.download_band(s, RF_BAND_A), A, len(r) + 1, m + 1, bw)
        assert_band_equal(engine.download_band(s, RF_BAND_B), B, len(r) + 1, m + 1, bw)
        h = max(m - len(r), 0) + bw
        assert bits_equal(scores[k:k + 1], [final_cell(A, len(r), m, bw) if direction == "fwd" else B[h, 0]])
        wk = oracle.backtrace(mv, len(r) + 1, m + 1, bw)
        walks.append((wk, oracle.count_errors(wk, t, r.seq)))
        As.append(A)
        Bs.append(B)
    check_walks(engine, opts, t, [w.reads[s] for s in w.good], list(w.good), walks)
    if tier not in WIDE:
        tot, per = oracle_scores(t, props, [w.reads[s] for s in w.good], As, Bs)
        mask = dense_mask(t)
        assert same(engine.score_dense([good])[0][mask], table(t, props, tot)[mask]).all()
        check_list_scores(engine, good, -1, props, tot, per)
    # 4. the wall's slot refilled with a finite read
    r = w.reads[w.repl]
    engine.realign([1], [w.repl], 0, [bw], flag)
    A, mv = oracle.forward(t, r, moves=True)
    B = oracle.backward(t, r)
    assert_band_equal(engine.download_band(1, RF_BAND_A), A, len(r) + 1, m + 1, bw)
    assert_band_equal(engine.download_band(1, RF_BAND_B), B, len(r) + 1, m + 1, bw)
    wk = oracle.backtrace(mv, len(r) + 1, m + 1, bw)
    check_walks(engine, opts, t, [r], [1], [(wk, oracle.count_errors(wk, t, r.seq))])
    if tier not in WIDE:
        tot, _ = oracle_scores(t, props, [r], [A], [B])
        mask = dense_mask(t)
        assert same(engine.score_dense([[1]])[0][mask], table(t, props, tot)[mask]).all()


@pytest.mark.parametrize("tier", [t for t in TIERS if t not in WIDE])
def test_first_column_raise_among_good_jobs(engine, opts, tier):
    """The read that raises in the first column (insertions and deletions
    impossible, n = m + 1; codon tables, so general in every tier) between
    two good jobs: forward and backward fills raise, and the bands are
    refused afterwards."""
    w = wall_of(tier)
    set_tier(opts, tier)
    engine.release_bands()
    engine.set_sequences(0, [w.reads[0], w.first_col, w.reads[2]])
    engine.set_templates(0, [w.t])
    for flag in (RF_FWD, RF_BWD, RF_FWD | RF_BWD):
        with pytest.raises(RifrafError, match=INVALID):
            engine.realign([0, 1, 2], [0, 1, 2], 0, [w.bw] * 3, flag)
    refused(lambda: engine.score_dense([[0, 2]], rows=[w.m + 1]))
    refused(lambda: engine.backtrace([2]))
    scores = engine.realign([0, 2], [0, 2], 0, [w.bw] * 2, RF_FWD | RF_BWD)
    for k, s in enumerate((0, 2)):
        A, _ = oracle.forward(w.t, w.reads[s])
        assert bits_equal(scores[k:k + 1], [final_cell(A, len(w.reads[s]), w.m, w.bw)])


def test_flag_after_raise_across_call_families(engine, opts):
    """rf_realign and every other call land the device's error flag in one
    pinned zone.  A raising rf_realign (the smallest wall case, m = 40)
    directly before each of rf_realign with a valid read, rf_backtrace,
    rf_score and rf_candidates_table: each returns 0 and the oracle's result
    (rf_candidates_table: its host restatement's).  Then the other way round:
    a raise landed by a call of the other families, followed by a clean
    rf_realign.  No test here has a walk that raises, so that raise is
    rf_candidates_table's NaN in a proposal slot.  test_raise_and_state_after
    already has a raising rf_realign followed by rf_backtrace or
    rf_score_dense on a slot the call did not name."""
    import test_candidates_host as CH
    from rifraf_amd import _lib
    from test_candidates import assert_same_results
    tier = "dpx31"
    w = wall_of(tier)
    set_tier(opts, tier)
    t, bw, m = w.t, w.bw, w.m
    engine.release_bands()
    engine.set_sequences(0, w.reads)
    engine.set_templates(0, [t])
    engine.realign([0, 1, 2, 3], [0, w.repl, 2, w.other], 0, [bw] * 4, RF_FWD | RF_BWD)

    def raise_in_realign():   # slot 1 named alone: the other slots stay current
        with pytest.raises(RifrafError, match=INVALID):
            engine.realign([1], [w.wall], 0, [bw], RF_FWD)

    o = w.reads[w.other]
    Ao, mvo = oracle.forward(t, o, moves=True)
    wk = oracle.backtrace(mvo, len(o) + 1, m + 1, bw)
    props = all_proposals_arrays(t)
    tot, per = oracle_scores(t, props, [o], [Ao], [oracle.backward(t, o)])
    assert not np.isnan(tot).any()
    grp = CH.flat_group(6, fill=1.0)
    cand = ([grp[0]], [grp[1]], [0.0], [0], 1)
    r = w.reads[w.repl]
    exp_repl = final_cell(oracle.forward(t, r)[0], len(r), m, bw)

    raise_in_realign()
    assert bits_equal(engine.realign([1], [w.repl], 0, [bw], RF_FWD), [exp_repl])
    raise_in_realign()
    moves, nerr = engine.backtrace([3])
    np.testing.assert_array_equal(moves[0], wk)
    assert nerr[0] == oracle.count_errors(wk, t, o.seq)
    raise_in_realign()
    check_list_scores(engine, np.array([3], np.int32), -1, props, tot, per)
    raise_in_realign()
    got = engine.candidates_table(*cand, masks=[grp[2]], with_counts=True)
    exp = _lib.host_candidates(*cand, masks=[grp[2]], with_counts=True)
    assert_same_results(got, exp)
    assert exp[0][3] > 0
    # the other way round
    _, bad, src, _ = next(c for c in CH.NANS if c[3])
    with pytest.raises(RifrafError, match="failed to compute a valid score"):
        engine.candidates_table([bad[0]], [bad[1]], [np.inf], [src], 2, masks=[bad[2]])
    assert bits_equal(engine.realign([1], [w.repl], 0, [bw], RF_FWD), [exp_repl])


# ---------------------------------------------------------------------
# 6. native waves
# ---------------------------------------------------------------------
def wave_clusters(rng, phred0, nclu=5, nreads=8, L=150, longer=2):
    """Reference-free clusters of equal-length reads, three substitutions
    each; cluster `longer` holds one read with an inserted base.  phred0:
    twenty Phred-0 positions in every read."""
    out = []
    for c in range(nclu):
        t = rng.integers(0, 4, L).astype(np.int8)
        reads, phreds = [], []
        for r in range(nreads):
            s = t.copy()
            for i in rng.integers(0, L, 3):
                s[i] = (s[i] + rng.integers(1, 4)) % 4
            p = rng.integers(8, 40, L).astype(np.int8)
            if c == longer and r == 3:
                s, p = np.insert(s, 70, 1).astype(np.int8), np.insert(p, 70, 20).astype(np.int8)
            if phred0:
                p[rng.integers(0, len(p), 20)] = 0
            reads.append(s)
            phreds.append(p)
        out.append(dict(dnaseqs=reads, phreds=phreds))
    return out


def test_native_scope_has_no_raising_fill():
    """The candidates for a wave with one raising cluster, on the CPU stage
    machine (OracleEngine): with a zero insertion, deletion or mismatch rate
    every cluster -- not only the one with a longer read -- is refused by
    check_params before any fill; with finite scores and Phred-0 reads no
    cluster raises."""
    from oracle_engine import OracleEngine
    from rifraf_amd.batch import native_eligible
    from rifraf_amd.model import RifrafParams, rifraf
    for em in (ErrorModel(1, 0, 0), ErrorModel(1, 0, 2), ErrorModel(1, 2, 0), ErrorModel(0, 1, 1)):
        params = RifrafParams(scores=Scores.from_errors(em), batch_size=0, batch_fixed=False, max_iters=3)
        clusters = wave_clusters(np.random.default_rng(5), False, nclu=3)
        assert native_eligible(clusters, params)
        for kw in clusters:
            with pytest.raises(RifrafError, match="scores must be between"):
                rifraf(params=params, engine=OracleEngine(), **kw)
    params = RifrafParams(scores=Scores.from_errors(ErrorModel(1, 2, 2)), batch_size=0, batch_fixed=False, max_iters=3)
    for kw in wave_clusters(np.random.default_rng(5), True, nclu=3):
        rifraf(params=params, engine=OracleEngine(), **kw)


def test_native_wave_with_phred0_reads(engine):
    """rf_rifraf_batch over clusters whose every read has Phred-0 positions
    (all fills and scoring in the general tiers) against the Python stage
    machine on the same engine: the same runs, quality pass included."""
    from rifraf_amd.batch import rifraf_batch
    from rifraf_amd.model import RifrafParams
    params = RifrafParams(scores=Scores.from_errors(ErrorModel(1, 2, 2)), batch_size=0, batch_fixed=False,
                          do_score=True, max_iters=20)
    clusters = wave_clusters(np.random.default_rng(6), True)
    hub = rifraf_batch(clusters, params=params, engine=engine, native=False)
    nat = rifraf_batch(clusters, params=params, engine=engine, native=True, device_qv=False)
    dqv = rifraf_batch(clusters, params=params, engine=engine, native=True)
    for a, b, c in zip(nat, hub, dqv):
        assert_same_run(summary(a), summary(b))
        assert_same_run(summary(c), summary(b), qv_rtol=QV_RTOL)
