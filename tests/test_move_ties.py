"""Exact move ties above the small sweep: every kernel that produces or
consumes moves, on inputs whose backtrace path runs through cells with tied
best candidates, against the CPU oracle.  The reference breaks such a tie in
the fixed order match, insert, delete, codon insert, codon delete with a
strict `>` (align.jl:77-104); a kernel that breaks it differently fills the
same band and the same A[end, end], so only the moves and what is derived
from them can show it.  Every assertion is equality of moves, integers or
score bits.

Inputs (fixed seeds; _util.tie_pair): templates of homopolymer runs of 1..6
bases over two letters, reads that copy the template with runs shortened and
lengthened by 1..3 bases, error_log_p = -1.0 everywhere.
  tie_seq    SEQ_SCORES, no codon tables
  tie_ref    REF_SCORES: codon tables, so a codon move ties with single moves
             (a run lengthened by three: the codon insert can sit anywhere in
             the run, so it ties with the match that slides it)
  tie_count  Scores(-2, -1/2, -1/2): mismatch = -3, insert = delete = -3/2,
             so mismatch == insert + delete exactly and tied paths differ in
             count_errors (a mismatch is one error, an insert and a delete two)

The conditions on the inputs (section 1) are CPU tests over the oracle alone:
a plain Python walk over the oracle's A band recomputes each on-path cell's
candidates, counts the tied ones, and walks again with the preference
reversed (last maximum wins).  The GPU tests (section 2) are marked `gpu`.
"""
import math

import numpy as np
import pytest

import oracle
from _util import REF_SCORES, SEQ_SCORES, tie_pair, tie_read, tie_template
from rifraf_amd import RifrafSequence, Scores, _lib
from rifraf_amd.align import band_tolerance, moves_to_aligned_seqs, moves_to_indices, moves_to_proposals_np
from rifraf_amd.engine import RF_BWD, RF_FWD, RF_SKEW
from test_pair_align_smart_host import ALWAYS, oracle_smart, poisson_thresholds

TIE_LP = -1.0
COUNT_SCORES = Scores(-2.0, -0.5, -0.5, -math.inf, -math.inf)
CLASS_SCORES = {"tie_seq": SEQ_SCORES, "tie_ref": REF_SCORES, "tie_count": COUNT_SCORES}
SEEDS = {"tie_seq": 3101, "tie_ref": 3102, "tie_count": 3103}
MAX_RUN = 6
PER_EDIT = {"tie_seq": 40, "tie_ref": 15, "tie_count": 40}   # template bases per edit
MIN_PATH_TIES = 8
# n == m pairs have no forced indel: the two halves of an edit lie up to this many runs apart, far enough
# that an insert and a delete cost less than a mismatch at every run boundary between them
LADDER_SPREAD = 24
LADDER_EDITS = {"tie_seq": 8, "tie_ref": 16, "tie_count": 8}   # at least this many edits per pair

# test_backtrace_windowed's multi-window shapes
BT_SHAPES = [(700, 9, 0), (400, 40, 30), (300, 120, -40), (260, 9, 60)]
BT_CLASSES = ("tie_seq", "tie_ref")
# the band heights on both sides of every fast-tier threshold of k_pa / k_pe (H = 2 bw + 1, n == m)
LADDER_BW = (15, 16, 31, 32, 63, 64, 127, 128)
# (m, n, bw) of the general-tier pairs: H = 271 and 291, n != m
GENERAL = ((300, 330, 120), (280, 250, 130))

OFFSETS = ((0, 0), (1, 1), (1, 0), (0, 1), (3, 0), (0, 3))   # align.jl:14-18
SINGLES = (1, 2, 3)   # match, insert, delete; 4 and 5 are the codon moves


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def read_of(s, bw, name):
    return RifrafSequence(s, np.full(len(s), TIE_LP), bw, CLASS_SCORES[name])


def tier_of(H, codon):
    """The trace tier of a pair: the fast classes by band height, "gen" above
    them and for every read with codon tables."""
    if codon or H > 255:
        return "gen"
    return next(h for h in (32, 64, 128, 255) if H <= h)


# ---------------------------------------------------------------------
# the Python walk
# ---------------------------------------------------------------------
def tie_walk(t, rs, A, bw, last=False):
    """backtrace over the oracle's A band alone: from (nrows, ncols) each
    cell's candidates are recomputed from the band and the read's tables
    (align.jl:50-112) and the first maximum in the order match, insert,
    delete, codon insert, codon delete is followed -- the last with `last`.
    -> (moves in alignment order, the tied codes of each on-path cell with
    two or more best candidates)."""
    s, n, m = rs.seq, len(rs.seq), len(t)
    nrows, ncols, H = n + 1, m + 1, A.shape[0]
    off = max(ncols - nrows, 0) + bw
    assert H == 2 * bw + abs(n - m) + 1
    ncins, ncdel = len(rs.codon_ins_scores), len(rs.codon_del_scores)

    def inband(i, j):
        return 1 <= i <= nrows and 1 <= j <= ncols and 0 <= i - j + off < H

    i, j = nrows, ncols
    out, ties = [], []
    while i > 1 or j > 1:
        seq_i = max(i - 1, 1)
        sb = s[i - 2] if i > 1 else -1
        tb = t[j - 2] if j > 1 else -1
        moves = [(1, rs.match_scores[seq_i - 1] if sb == tb else rs.mismatch_scores[seq_i - 1]),
                 (2, rs.ins_scores[seq_i - 1]), (3, rs.del_scores[i - 1])]
        if ncins > 0 and i > 3:
            moves.append((4, rs.codon_ins_scores[i - 4]))
        if ncdel > 0 and j > 3:
            moves.append((5, rs.codon_del_scores[i - 1]))
        cand = [(c, A[i - OFFSETS[c][0] - (j - OFFSETS[c][1]) + off, j - OFFSETS[c][1] - 1] + sc)
                for c, sc in moves if inband(i - OFFSETS[c][0], j - OFFSETS[c][1])]
        best = max(v for _, v in cand)
        assert best == A[i - j + off, j - 1], (i, j)
        tied = tuple(c for c, v in cand if v == best)
        if len(tied) > 1:
            ties.append(tied)
        mv = tied[-1] if last else tied[0]
        out.append(mv)
        i -= OFFSETS[mv][0]
        j -= OFFSETS[mv][1]
    return np.array(out[::-1], np.int8), ties


class Pair:
    """One (template, read, bandwidth) and, on first use, the oracle's
    results for it: A band, score bits, moves, count_errors, and both Python
    walks."""

    def __init__(self, t, rs, bw, tag):
        self.t, self.rs, self.bw, self.tag = t, rs, int(bw), tag
        self.n, self.m = len(rs.seq), len(t)
        self.H = 2 * self.bw + abs(self.n - self.m) + 1
        self._o = self._w = None

    def oracle(self, skew=False):
        """(A[end, end], moves, count_errors); the unskewed fill is kept."""
        if skew or self._o is None:
            A, mv = oracle.forward(self.t, self.rs, moves=True, skew=skew, bandwidth=self.bw)
            w = oracle.backtrace(mv, self.n + 1, self.m + 1, self.bw)
            res = (A[self.n - self.m + max(self.m - self.n, 0) + self.bw, self.m], w,
                   oracle.count_errors(w, self.t, self.rs.seq))
            if skew:
                return res
            self._o, self._A = res, A
        return self._o

    def walks(self):
        """((first-maximum moves, on-path ties), last-maximum moves)."""
        if self._w is None:
            self.oracle()
            self._w = (tie_walk(self.t, self.rs, self._A, self.bw), tie_walk(self.t, self.rs, self._A, self.bw, True)[0])
        return self._w


_MEMO = {}


def memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def bt_case(name, L, bw, skew):
    """One template of L bases and three reads of it, longer (skew > 0),
    shorter (skew < 0) or within two bases of it, one further edit per
    PER_EDIT template bases each."""
    def make():
        rng = np.random.default_rng(SEEDS[name] * 1000 + L + bw)
        t, runs, letters = tie_template(L, rng, MAX_RUN)
        pairs = []
        for _ in range(3):
            d = int(rng.integers(skew // 2, skew + 1)) if skew > 0 else \
                -int(rng.integers(-skew // 2, -skew + 1)) if skew < 0 else int(rng.integers(-2, 3))
            s = tie_read(runs, letters, L + d, rng, edits=L // PER_EDIT[name])
            pairs.append(Pair(t, read_of(s, bw, name), bw, (name, L, bw, skew, L + d)))
        return pairs
    return memo(("bt", name, L, bw, skew), make)


def ref_walk_case():
    """A reference against a consensus of m = 2600 at bandwidth 9."""
    def make():
        rng = np.random.default_rng(SEEDS["tie_ref"] * 1000 + 2600)
        t, s = tie_pair(2600, 2598, rng, MAX_RUN, edits=60)
        return [Pair(t, read_of(s, 9, "tie_ref"), 9, ("tie_ref", 2600, 9))]
    return memo("ref2600", make)


def ladder(name):
    """Two n == m pairs on each side of every fast-tier threshold (m = 3 H and
    2 H + 7, at most 600 and 451) and the two general-tier pairs."""
    def make():
        rng = np.random.default_rng(SEEDS[name] * 1000 + 1)
        pairs = []
        for bw in LADDER_BW:
            H = 2 * bw + 1
            for m in (min(3 * H, 600), min(2 * H + 7, 451)):
                t, s = tie_pair(m, m, rng, MAX_RUN, edits=max(LADDER_EDITS[name], m // PER_EDIT[name]),
                                spread=LADDER_SPREAD)
                pairs.append(Pair(t, read_of(s, bw, name), bw, (name, H, m, m)))
        for m, n, bw in GENERAL:
            t, s = tie_pair(m, n, rng, MAX_RUN, edits=8)
            pairs.append(Pair(t, read_of(s, bw, name), bw, (name, 2 * bw + abs(n - m) + 1, m, n)))
        return pairs
    return memo(("ladder", name), make)


def smart_cases():
    """The tie_count ladder under band doubling: every pair from bandwidth 1
    and from half its ladder bandwidth (one doubling lands in the pair's own
    tier) with a threshold every count is above, and from bandwidth 2 with
    the Poisson threshold.  An edit leaves the diagonal by up to three, so
    the narrow starts miss it and the count falls as the band doubles.
    -> (pairs, indices into them, starting bandwidths, thresholds)."""
    pairs = ladder("tie_count")
    n = len(pairs)
    idx = np.tile(np.arange(n), 3)
    bws = np.concatenate([np.full(n, 1), [max(p.bw // 2, 1) for p in pairs], np.full(n, 2)]).astype(np.int32)
    thr = np.concatenate([np.full(2 * n, ALWAYS), poisson_thresholds([p.rs for p in pairs])])
    return pairs, idx, bws, thr


def smart_expected():
    def make():
        pairs, idx, bws, thr = smart_cases()
        fills = {}
        return [oracle_smart(pairs[k].t, pairs[k].rs, int(bw), float(th), False, 5, fills, int(k))
                for k, bw, th in zip(idx, bws, thr)]
    return memo("smart", make)


# ---------------------------------------------------------------------
# 1. the inputs meet their conditions, by the oracle alone
# ---------------------------------------------------------------------
def kinds_of(ties):
    """The pairs (a, b), a < b, of move codes tied in some cell."""
    return {(a, b) for tied in ties for a in tied for b in tied if a < b}


def check_conditions(pairs):
    """(a) the Python walk is the oracle's backtrace and at least
    MIN_PATH_TIES of its cells are tied; (b) the reversed preference walks
    other moves.  -> (on-path ties per pair, tied kinds, moves that differ
    under the reversed rule per pair)."""
    counts, kinds, differ = [], set(), []
    for p in pairs:
        (first, ties), last = p.walks()
        np.testing.assert_array_equal(first, p.oracle()[1], err_msg=str(p.tag))
        assert len(ties) >= MIN_PATH_TIES, (p.tag, len(ties))
        assert first.tobytes() != last.tobytes(), (p.tag, "the reversed rule walks the same moves")
        counts.append(len(ties))
        kinds |= kinds_of(ties)
        k = min(len(first), len(last))
        differ.append(int((first[:k] != last[:k]).sum()) + abs(len(first) - len(last)))
    return counts, kinds, differ


SINGLE_KINDS = {(1, 2), (1, 3), (2, 3)}   # match / insert, match / delete, insert / delete


def assert_kinds(name, kinds):
    """Every pair of moves that can tie in the class is tied on some path.
    With codon tables a mismatch (-1.09) is far cheaper than an insert and a
    delete (-3.09 each), so no best path of tie_ref enters a cell by either of
    the two at the same value: there the insert / delete pair is replaced by
    each codon move against a single move."""
    if name == "tie_ref":
        need = {(1, 2), (1, 3)}
        assert any((a, 4) in kinds for a in SINGLES) and any((a, 5) in kinds for a in SINGLES), (name, sorted(kinds))
    else:
        need = SINGLE_KINDS
    assert need <= kinds, (name, sorted(need - kinds))


@pytest.mark.parametrize("name", BT_CLASSES)
def test_backtrace_inputs_tie(name):
    """Conditions (a) and (b) on the slots of test_backtrace_ties and, for
    tie_ref, the m = 2600 walk, by the oracle alone.  On-path tied cells per
    read (three reads per shape) and moves that differ under the reversed
    rule:
      tie_seq (700, 9, 0)      66, 79, 78     differ 48, 80, 66
              (400, 40, 30)    66, 98, 102           52, 76, 72
              (300, 120, -40)  63, 70, 66            44, 42, 54
              (260, 9, 60)     110, 111, 129         78, 98, 96
      tie_ref (700, 9, 0)      51, 60, 78            41, 57, 50
              (400, 40, 30)    20, 54, 37            19, 43, 26
              (300, 120, -40)  17, 26, 17            22, 18, 20
              (260, 9, 60)     16, 31, 42            18, 20, 29
              m = 2600         132                   89
    Tied kinds: tie_seq match / insert, match / delete, insert / delete;
    tie_ref match / insert, match / delete and both codon moves against each
    of match, insert and delete (and against each other)."""
    kinds = set()
    cases = [(sh, bt_case(name, *sh)) for sh in BT_SHAPES]
    if name == "tie_ref":
        cases.append(("m = 2600", ref_walk_case()))
    for sh, pairs in cases:
        counts, k, differ = check_conditions(pairs)
        print(f"{name} {sh}: on-path tied cells {counts}, moves differing under the reversed rule {differ}, "
              f"tied kinds {sorted(k)}")
        kinds |= k
    assert_kinds(name, kinds)


@pytest.mark.parametrize("name", list(SEEDS))
def test_ladder_inputs_tie(name):
    """Conditions (a) and (b) on the 18 pairs of the ladder, by the oracle
    alone; the pairs sit at H = 31, 33, 63, 65, 127, 129, 255, 257 (two each),
    271 and 291, with n + m on both sides of 512 (the wave walk's own
    threshold).  On-path tied cells / moves differing under the reversed rule:
      tie_seq    14 .. 99 (701 in all) / 14 .. 66
      tie_ref    8 .. 77 (540) / 8 .. 45
      tie_count  27 .. 91 (876) / 29 .. 96
    tie_count: count_errors differs under the reversed rule in all 18 pairs
    (e.g. H = 31: 21 against 26), so in every tier.  tie_seq: 18 pairs have
    two inserts at one template position (ambiguous for rf_pair_shifts);
    tie_ref has 228 codon moves on its paths."""
    pairs = ladder(name)
    assert [p.H for p in pairs[:16]] == [2 * bw + 1 for bw in LADDER_BW for _ in range(2)]
    assert all(p.H > 255 and p.n != p.m for p in pairs[16:])
    assert min(p.n + p.m for p in pairs) < 512 <= max(p.n + p.m for p in pairs)
    counts, kinds, differ = check_conditions(pairs)
    print(f"{name}: on-path tied cells {counts} ({sum(counts)}), moves differing under the reversed rule {differ}, "
          f"tied kinds {sorted(kinds)}")
    assert_kinds(name, kinds)
    if name == "tie_count":
        by_tier = {}
        for p in pairs:
            first, last = p.oracle()[2], oracle.count_errors(p.walks()[1], p.t, p.rs.seq)
            by_tier.setdefault(tier_of(p.H, False), []).append((first, last))
        print(f"{name}: count_errors (oracle, reversed rule) per tier {by_tier}")
        assert set(by_tier) == {32, 64, 128, 255, "gen"}
        for tier, c in by_tier.items():
            assert any(a != b for a, b in c), (tier, c)
    else:
        mvs = [p.oracle()[1] for p in pairs]
        r = _lib.host_shift_fix(mvs, [p.rs.seq for p in pairs], [p.t for p in pairs])
        ncodon = sum(int((mv >= 4).sum()) for mv in mvs)
        print(f"{name}: {int((r.fixed_len == -2).sum())} ambiguous pairs, {ncodon} codon moves")
        if name == "tie_seq":
            assert (r.fixed_len == -2).any(), "no pair with two inserts at one template position"
        else:
            assert ncodon > 0


def test_doubling_inputs_take_rounds():
    """Every tie_count pair started below its band takes at least two fills
    under smart_forward_moves! (the oracle's restatement): rounds 2 .. 5 from
    bandwidth 1, 2 from half the ladder bandwidth; the Poisson threshold adds
    stops below it after 1 .. 4."""
    pairs, idx, bws, thr = smart_cases()
    exp = smart_expected()
    n = len(pairs)
    rounds = [e.rounds for e in exp]
    print(f"rounds {rounds}, final bandwidths {[e.bw for e in exp]}, stops {sorted({e.why for e in exp})}")
    assert min(rounds[:2 * n]) >= 2 and max(rounds[:n]) >= 4
    assert {"stalled", "below"} <= {e.why for e in exp}
    # one doubling from half the ladder bandwidth ends in the pair's own tier
    assert [e.bw for e in exp[n:2 * n]] == [2 * (p.bw // 2) for p in pairs]


# ---------------------------------------------------------------------
# 2. the engine against the oracle
# ---------------------------------------------------------------------
def check_slots(engine, opts, pairs, win_kb, nw, pad):
    """The pairs (one template) into slots 0.. : rf_backtrace's moves and
    counts, rf_alignment_proposals with and without indels and
    rf_aln_error_sums (one launch, marks + fold, host fold) from the same
    slots, against the oracle's walks."""
    from rifraf_amd.model import _add_base_distributions
    t, seqs, n = pairs[0].t, [p.rs for p in pairs], len(pairs)
    sl = np.arange(n, dtype=np.int32)
    opts("band_pad", pad)
    engine.set_sequences(0, seqs)
    engine.set_templates(0, [t])
    sc = engine.realign(sl, sl, 0, [p.bw for p in pairs], RF_FWD | RF_BWD)
    assert bits(sc).tolist() == bits([p.oracle()[0] for p in pairs]).tolist()
    opts("bt_win_kb", win_kb)
    opts("bt_nw", nw)
    got, nerr = engine.backtrace(sl)
    for k, p in enumerate(pairs):
        np.testing.assert_array_equal(got[k], p.oracle()[1], err_msg=str(p.tag))
        assert nerr[k] == p.oracle()[2], (p.tag, nerr[k], p.oracle()[2])
    for do_indels in (True, False):
        exp = np.zeros((len(t) + 1, 9), np.uint8)
        for p in pairs:
            kk, pos, b = moves_to_proposals_np(p.oracle()[1], t, p.rs.seq)
            if not do_indels:
                keep = kk == 0
                kk, pos, b = kk[keep], pos[keep], b[keep]
            exp[pos, np.where(kk == 0, b, np.where(kk == 2, 4, 5 + b))] = 1
        np.testing.assert_array_equal(engine.alignment_proposals([sl], do_indels)[0], exp,
                                      err_msg=f"{pairs[0].tag} do_indels={do_indels}")
    exp = np.zeros((len(t), 4))
    _add_base_distributions(exp, [p.oracle()[1] for p in pairs], seqs)
    for how, option in (("one launch", None), ("marks + fold", ("aln_marks_min", 0)), ("host", ("aln_sums_host", 1))):
        if option:
            opts(*option)
        sums = engine.aln_error_sums([sl], [len(t)], [seqs])[0]
        assert sums.shape == exp.shape and bits(sums).tobytes() == bits(exp).tobytes(), (pairs[0].tag, how)
        if how != "host" and not seqs[0].do_codon_moves():
            # without the host tables only the device fold can answer: k_aln_sums / k_aln_marks + k_aln_fold ran
            dev = engine.aln_error_sums_ptr([sl], [len(t)], None, None, [p.n for p in pairs])
            assert dev is not None, "a read has no row codes: the device fold did not run"
            assert bits(dev[0]).tobytes() == bits(exp).tobytes(), (pairs[0].tag, how, "device fold")


@pytest.mark.gpu
@pytest.mark.parametrize("pad", [64, 1])
@pytest.mark.parametrize("nw", [4, 1])
@pytest.mark.parametrize("win_kb", [16, 32])
@pytest.mark.parametrize("L,bw,skew", BT_SHAPES)
@pytest.mark.parametrize("name", BT_CLASSES)
def test_backtrace_ties(engine, opts, name, L, bw, skew, win_kb, nw, pad):
    """k_bt_win over several LDS windows of 16 and 32 KB, on 4 waves and on
    one, padded and unpadded row strides, on reads whose path runs through
    tied cells all along (test_backtrace_inputs_tie), and the three consumers
    of its moves."""
    check_slots(engine, opts, bt_case(name, L, bw, skew), win_kb, nw, pad)


@pytest.mark.gpu
def test_reference_walk_ties(engine, opts):
    """A reference (codon tables) against a consensus of 2600 bases at
    bandwidth 9, one walk on 4 waves."""
    check_slots(engine, opts, ref_walk_case(), 32, 4, 64)


def upload_ladder(engine, pairs):
    engine.set_sequences(0, [p.rs for p in pairs])
    engine.set_templates(0, [p.t for p in pairs])
    return np.arange(len(pairs)), np.array([p.bw for p in pairs], np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("walk", (1, 2))
@pytest.mark.parametrize("name", list(SEEDS))
def test_pair_align_ties(engine, opts, name, walk):
    """rf_pair_align over the ladder in one call: the trace of every fast tier
    and of the general tier (k_pa, k_pa_gen) walked a lane per pair
    (k_pa_walk) and a wave per pair (k_pa_walk_w).  Moves, counts and score
    bits are the oracle's."""
    pairs = ladder(name)
    opts("pair_walk", walk)
    ids, bws = upload_ladder(engine, pairs)
    scores, moves, nerr = engine.pair_align(ids, ids, bws)
    assert bits(scores).tolist() == bits([p.oracle()[0] for p in pairs]).tolist()
    for k, p in enumerate(pairs):
        assert moves[k] is not None, p.tag
        np.testing.assert_array_equal(moves[k], p.oracle()[1], err_msg=str(p.tag))
        assert nerr[k] == p.oracle()[2], (p.tag, nerr[k], p.oracle()[2])
    counts = engine.pair_align(ids, ids, bws, want_moves=False)
    assert counts[2].tolist() == nerr.tolist()


@pytest.mark.gpu
def test_pair_counts_ties(engine):
    """rf_pair_errors (k_pe / k_pe_gen: the count carried in registers and in
    the int32 ring) over the tie_count ladder, where tied paths differ in
    count_errors: the counts are count_errors of the oracle's moves.  Then
    band doubling from below (smart_cases): scores, counts, final bandwidths
    and rounds of rf_pair_errors and of rf_pair_align_smart are the oracle's
    smart_forward_moves! restatement's, and each other's."""
    pairs = ladder("tie_count")
    ids, bws = upload_ladder(engine, pairs)
    got = engine.pair_errors(ids, ids, bws)
    assert bits(got[0]).tolist() == bits([p.oracle()[0] for p in pairs]).tolist()
    assert got[1].tolist() == [p.oracle()[2] for p in pairs]
    assert got[2].tolist() == bws.tolist() and (got[3] == 1).all()
    _, idx, start, thr = smart_cases()
    exp = smart_expected()
    errs = engine.pair_errors(idx, idx, start, thr, max_doublings=5)
    smart = engine.pair_align_smart(idx, idx, start, thr, max_doublings=5)
    for k, e in enumerate(exp):
        tag = (pairs[idx[k]].tag, int(start[k]), e.why)
        assert bits(errs[0][k]) == bits(e.score) == bits(smart[0][k]), tag
        assert (errs[1][k], errs[2][k], errs[3][k]) == (e.nerr, e.bw, e.rounds), (tag, errs[1][k], errs[2][k], errs[3][k], e)
        assert (smart[2][k], smart[3][k], smart[4][k]) == (e.nerr, e.bw, e.rounds), (tag, smart[2][k], smart[3][k], e)
        np.testing.assert_array_equal(smart[1][k], e.moves, err_msg=str(tag))


@pytest.mark.gpu
@pytest.mark.parametrize("walk", (1, 2))
@pytest.mark.parametrize("name", BT_CLASSES)
def test_pair_text_ties(engine, opts, name, walk):
    """rf_pair_align_text (k_pa_emit) over the ladder: the gapped texts,
    moves_to_indices and band_tolerance are the host functions' over the
    oracle's moves."""
    pairs = ladder(name)
    opts("pair_walk", walk)
    ids, bws = upload_ladder(engine, pairs)
    caps = (np.array([p.n + p.m for p in pairs]), np.array([p.m for p in pairs]))
    scores, r = engine.pair_align_text(ids, ids, bws, want_text=True, want_indices=True, want_tolerance=True, caps=caps)
    assert bits(scores).tolist() == bits([p.oracle()[0] for p in pairs]).tolist()
    assert r.nerrors.tolist() == [p.oracle()[2] for p in pairs]
    for k, p in enumerate(pairs):
        mv = p.oracle()[1]
        text = moves_to_aligned_seqs(mv, p.t, p.rs.seq)
        assert r.text(k) == text and r.aln_len[k] == len(text[0]), p.tag
        t2s = moves_to_indices(mv, p.m, p.n)
        assert r.indices(k).tolist() == t2s and r.t2s_len[k] == len(t2s), p.tag
        assert r.tolerance[k] == band_tolerance(mv, p.n + 1, p.m + 1, p.bw), p.tag


@pytest.mark.gpu
@pytest.mark.parametrize("flags", (0, RF_SKEW))
@pytest.mark.parametrize("walk", (1, 2))
@pytest.mark.parametrize("name", BT_CLASSES)
def test_pair_shifts_ties(engine, opts, name, walk, flags):
    """rf_pair_shifts (k_pa_fix) over the ladder, plain and skewed (what
    correct_shifts passes): the single-indel proposals, the corrected
    consensus, the ambiguity flag (fixed_len -2) and the tallies are
    rf_host_shift_fix's over the oracle's moves."""
    pairs = ladder(name)
    opts("pair_walk", walk)
    ids, bws = upload_ladder(engine, pairs)
    want = [p.oracle(skew=bool(flags & RF_SKEW)) for p in pairs]
    caps = np.array([p.n + p.m for p in pairs], np.int64)
    scores, r = engine.pair_shifts(ids, ids, bws, flags, want_fixed=True, want_proposals=True, caps=caps)
    assert bits(scores).tolist() == bits([w[0] for w in want]).tolist()
    exp = _lib.host_shift_fix([w[1] for w in want], [p.rs.seq for p in pairs], [p.t for p in pairs])
    assert r.fixed_len.tolist() == exp.fixed_len.tolist()
    assert r.nprops.tolist() == exp.nprops.tolist()
    assert r.tally.tolist() == exp.tally.tolist()
    for k, p in enumerate(pairs):
        assert r.proposals(k) == exp.proposals(k), p.tag
        x, y = r.fixed_seq(k), exp.fixed_seq(k)
        assert (x is None and y is None) or x.tolist() == y.tolist(), p.tag
    if name == "tie_seq" and flags == 0:
        assert (r.fixed_len == -2).any()
