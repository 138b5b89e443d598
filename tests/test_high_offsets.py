"""Every kernel family at arena offsets that do not fit in 32 bits.

Every kernel reaches its data through 64-bit offsets into three
bump-allocated arenas (bands and tables in doubles, bases in bytes).  The
product lives far above the 32-bit lines -- one native wave of 256 clusters is
about 14.8 GB of bands -- while every small-shape test of the suite runs in
the first few MB of each arena.  One `int` in an index expression is enough to
be wrong up there, and only a test that works up there would notice.

Band arena (`world`, its own Engine, about 18.5 GiB reserved):

  canaries  the probe set filled once at the bottom of the arena, compared
            with the oracle like any small test; every canary band's bits are
            kept
  filler    one call of its own: several thousand A bands of one 2,000-base
            pair (H 181, the lean fill the bench runs), 3.2 MB each, and one
            H 3 band whose length tunes `top` to 256 bytes, so that the
            filler ends half a band below 2^34 bytes
  probes    the probe set again, in the same call order: its first band
            straddles 2^31 doubles (16 GiB), every other one starts above it

Every probe result equals the oracle bit for bit and equals the canary result
of the same call; when all high work is done the canary bands are downloaded
again and must still hold their first bits.  A kernel that truncates an
offset to 32 bits in its writer and its reader alike computes right answers
while it overwrites the bottom of the arena: a probe's byte offset modulo 2^32
falls inside the canary area (asserted on the CPU from the layout plan), so
that last check is what catches it.

The engine has to prove where the regions lie: rf_region_offsets
(Engine.band_region / seq_regions) must return exactly the offsets that
plan_layout, a restatement of the engine's allocation rules (ARENA_GUARD,
256-byte regions, band_K x band_stride x 8 under RF_OPT_BAND_PAD's per-call
rule, seq_table_len), computes for the same calls.  The fixture asserts that
before any kernel result is looked at.

Table arena (`table_world`, a second Engine after the first is closed, about
5 GiB): twelve canary reads low, then one rf_set_sequences_codes call of
1,080 reads of 100,000 bases (k_tables builds 4.3 GB of tables on the device
from one byte per position), then the same twelve reads again above 2^32
bytes, six through rf_set_sequences (tables) and six through
rf_set_sequences_codes (row codes).  rf_realign (lean and general tier), every
pair kernel and the device fold of rf_aln_error_sums (its `rec` offsets point
into the table arena) are compared with the oracle and with the same call on
the low copies.

Left out, on purpose:
  - arena compaction of a region above 4 GiB.  rf_reserve sizes the band arena
    once, so it never grows here; compaction copies each region with one
    workgroup (k_scatter), and moving a 16 GiB arena is not a unit test.
  - tables above 2^31 doubles (16 GiB): four times what any workload holds,
    at a host-side cost nobody has measured.
  - the byte arena (bases and templates): it stays at a few hundred MB in
    every workload the project has.  The table filler's bases put the probe
    reads' bases above 100 MB, no further.

The tests of this module compare what the fixtures laid out; they can be
selected one by one.  test_canaries_survive reads the canaries back after the
fills, so it is last.
"""
import contextlib
import json
import math
import os
import time

import numpy as np
import pytest

import oracle
from _util import REF_SCORES, SEQ_SCORES, all_proposals_arrays, assert_score_launch, random_seq
from rifraf_amd import RifrafSequence, _lib
from rifraf_amd.align import band_tolerance, moves_to_aligned_seqs, moves_to_indices
from rifraf_amd.engine import RF_BAND_A, RF_BAND_B, RF_BWD, RF_FWD, RF_SKEW, Engine
from rifraf_amd.model import _add_base_distributions
from test_gpu_parity import SCORER_CONFIGS, assert_band_equal
from test_nonfinite_tiers import (DNS, LP_TABLE, MATCH_TABLE, TIERS, WIDE, case_of, oracle_scores, proposals_mask,
                                  sampled)
from test_pair_scores import bits_equal, final_cell
from test_score_dense_ref import CODON, dense_mask, make_varying_case, same, table

GIB = 1 << 30
LINE_DOUBLES = 1 << 31          # doubles: the band line, 16 GiB
LINE = LINE_DOUBLES * 8         # the same in bytes, 2^34
MEMORY_CAP = 32 * GIB           # peak rf_device_bytes of either engine

# ---------------------------------------------------------------------
# 1. the layout plan: the engine's allocation rules, restated
# ---------------------------------------------------------------------
ARENA_GUARD = 1 << 16
BAND_PAD_H = 64                 # RF_OPT_BAND_PAD's default


def align_up(x, a):
    return (x + a - 1) // a * a


def region_bytes(nbytes):
    return align_up(max(nbytes, 16), 256)


def band_rows(n, m, bw):
    return 2 * bw + abs(n - m) + 1


def band_stride(H, padded):
    half = (H + 1) >> 1
    return (half + 15) & ~15 if padded else half | 1


def seq_table_len(n, ncins=0, ncdel=0):
    return 4 * n + 1 + ncins + ncdel + n


class Layout:
    """The three arenas of a context that never moves a region: every id is
    uploaded at one size only and the band arena is reserved up front (a
    growth repacks the live regions in offset order, which leaves a
    bump-allocated arena without holes as it was)."""

    def __init__(self):
        self.top = {"band": ARENA_GUARD, "tabs": ARENA_GUARD, "bytes": ARENA_GUARD}
        self.band, self.tabs, self.bases, self.tpl = {}, {}, {}, {}
        self.n, self.m, self.geom = {}, {}, {}

    def _take(self, arena, table, key, nbytes):
        cap = region_bytes(nbytes)
        if key in table:
            assert table[key][1] >= cap, "a region that grows leaves a hole: not planned"
            return
        table[key] = (self.top[arena], cap)
        self.top[arena] += cap

    def sequences(self, first, lens, ncins=None, ncdel=None):
        """One upload call (any of the three) of ids first.."""
        for k, n in enumerate(lens):
            self.n[first + k] = n
            self._take("bytes", self.bases, first + k, n)
            self._take("tabs", self.tabs, first + k,
                       seq_table_len(n, ncins[k] if ncins else 0, ncdel[k] if ncdel else 0) * 8)

    def templates(self, ids, lens):
        for i, m in zip(ids, lens):
            self.m[i] = m
            self._take("bytes", self.tpl, i, m)

    def fill(self, jobs, flags=RF_FWD | RF_BWD, pad_h=BAND_PAD_H):
        """One rf_realign call: jobs of (slot, seq, tpl, bw).  All forward
        bands are laid out first, then all backward bands; the call pads every
        band when its widest reaches pad_h; a band whose partner holds the same
        alignment takes the partner's stride."""
        Hs = [band_rows(self.n[s], self.m[t], bw) for _, s, t, bw in jobs]
        padded = pad_h > 0 and max(Hs) >= pad_h
        for which, bit in ((RF_BAND_A, RF_FWD), (RF_BAND_B, RF_BWD)):
            if not flags & bit:
                continue
            for (slot, s, t, bw), H in zip(jobs, Hs):
                partner = self.geom.get((slot, 1 - which))
                P = partner[3] if partner and partner[:3] == (s, t, bw) else band_stride(H, padded)
                self.geom[(slot, which)] = (s, t, bw, P)
                self._take("band", self.band, (slot, which), (H + 2 * self.m[t]) * P * 8)


# ---------------------------------------------------------------------
# 2. the probe set
# ---------------------------------------------------------------------
class Cluster:
    """A template and its reads with the oracle's fills and walks (the
    interface of test_nonfinite_tiers.Case, for inputs that are not a tier's)."""

    def __init__(self, t, reads, bw):
        self.t, self.reads, self.bw, self.m = t, reads, bw, len(t)
        self.nonfinite = []
        self._memo = {}

    def upload(self, engine, first=0):
        engine.set_sequences(first, self.reads)

    def fwd(self, k, flags=0):
        if ("f", k) not in self._memo:
            r = self.reads[k]
            bw = self.bw or r.bandwidth
            A, mv = oracle.forward(self.t, r, moves=True, bandwidth=bw)
            w = oracle.backtrace(mv, len(r) + 1, self.m + 1, bw)
            self._memo[("f", k)] = (A, w, oracle.count_errors(w, self.t, r.seq))
        return self._memo[("f", k)]

    def bwd(self, k):
        if ("b", k) not in self._memo:
            self._memo[("b", k)] = oracle.backward(self.t, self.reads[k], bandwidth=self.bw or self.reads[k].bandwidth)
        return self._memo[("b", k)]


def long_reference():
    """test_dpx_long_reference_tasks' first shape: a 2,621-base codon
    reference against 2,600 columns at bw 9 (k_dpx<true, true>, H 40)."""
    m, dn, bw = 2600, 21, 9
    rng = np.random.default_rng(m + dn + 1000 * bw)
    t = random_seq(m, rng)
    s = t.copy()
    for _ in range(m // 200):
        p = int(rng.integers(0, len(s)))
        op = int(rng.integers(0, 3))
        if op == 0:
            s[p] = (s[p] + 1) % 4
        elif op == 1:
            s = np.concatenate([s[:p], random_seq(int(rng.integers(1, 4)), rng), s[p:]])
        else:
            s = np.concatenate([s[:p], s[p + int(rng.integers(1, 4)):]])
    s = s[:m + dn] if len(s) > m + dn else np.concatenate([s, random_seq(m + dn - len(s), rng)])
    return Cluster(t, [RifrafSequence(s, np.full(len(s), math.log10(0.1)), bw, REF_SCORES)], bw)


def reference_cluster():
    """Three reads and a codon reference whose tables differ at every
    position (test_score_dense_ref.make_varying_case), for k_codon,
    k_codon_dense and the candidates' reference term."""
    c = make_varying_case(45, 44, 6, np.random.default_rng(4518), 3, CODON, read_bw=9)
    cl = Cluster(c.t, c.reads + [c.ref], None)
    cl.case = c
    return cl


_CLUSTERS = {}


def cluster_of(key):
    """key: a tier of test_nonfinite_tiers.TIERS (three reads with Phred-0
    positions and three finite ones at n - m = 0, +3, -4, uploaded as Phred
    codes; the 2,100-base tiers: its "holes" reads, uploaded as tables),
    "longref" or "ref"."""
    if key not in _CLUSTERS:
        if key == "longref":
            _CLUSTERS[key] = long_reference()
        elif key == "ref":
            _CLUSTERS[key] = reference_cluster()
        else:
            _CLUSTERS[key] = case_of(key, "holes" if key in WIDE else "phred0-codes")
    return _CLUSTERS[key]


# (name, cluster, reads of it, options of the fill).  dp_lat is 0 as in
# conftest.py unless the probe says otherwise.  The first probe's first band is
# the one that straddles 2^31 doubles.
DP_PROBES = [
    ("np8", "dpr8", range(6), {"dp_wide": 0}),                  # lean k_dpr<8> + general k_dpr<8>
    ("wide64", "dpr8", range(6), {}),                           # lean 64-lane tasks
    ("np4", "dpr4", range(6), {"dp_wide": 0, "dp_nl64": 0}),
    ("wide32", "dpr4", range(6), {"dp_nl64": 0}),
    ("np2", "dpr2", range(6), {"dp_nl64": 0}),
    ("np1", "dpr1", range(6), {"dp_nl64": 0}),
    ("dp64", "dp64", range(6), {"dp_np8": 0}),                  # k_dp<64>
    ("dpring", "dpring", range(6), {}),                         # k_dp<64>, H 271..275
    ("dpx", "dpx63", range(6), {"dp_lat": 2048}),               # latency mode: k_dpx lean and non-lean
    ("dpx127", "dpx127", range(6), {"dp_lat": 2048}),
    ("longref", "longref", range(1), {}),                       # k_dpx's long-reference form
    ("dpm", "dpm", (0, 4), {"dp_mc": 1}),                       # k_dpm: slices across CUs
    ("dpwide", "dpwide", (0, 4), {"dp_mc": 0}),                 # the same bands, one workgroup each (k_dp)
    ("ref", "ref", range(4), {}),                               # reads + codon reference, for the readers
]
PROBE = {p[0]: p for p in DP_PROBES}

# what section 3 of the issue names, as (kernel family, npi or None) of the DP launch records
DP_FAMILIES = [("dpr_lean_pm", 0), ("dpr_lean_pm", 1), ("dpr_lean_pm", 2), ("dpr_lean_pm", 3),   # each lean k_dpr NP tier
               ("dpr", 0), ("dpr", 1), ("dpr", 2), ("dpr", 3),                           # the general k_dpr steps                                                          # the general k_dpr step
               ("dp64", None), ("dpw_lds", None),                                      # k_dp
               ("dpx_lean", None), ("dpx_codon", None),                                # k_dpx, latency mode
               ("dpm", None)]

# scoring probes: (cluster, reads of it): finite reads can take every scorer
SCORE_PROBE = ("np2", (3, 4, 5))
SCORE_KERNELS = ("general", "seg", "ws")
SCORE_CASES = [(k, mode) for k in SCORE_KERNELS for mode in ("fused", "split")]
assert {k for k, _ in SCORER_CONFIGS} >= set(SCORE_KERNELS)
BT_CASES = [(16, 4), (16, 1), (32, 4), (32, 1)]     # (bt_win_kb, bt_nw)
BT_PROBES = ("np8", "dpring", "longref")            # H 181 (one window), H 271, 5,200 moves (many windows)
# the other band readers of section 3 -> the test that runs them high
READERS = {"k_codon": "test_reference_scoring", "k_codon_dense": "test_reference_scoring",
           "k_bt_win": "test_backtrace", "k_bt_win+mask": "test_alignment_proposals",
           "k_aln_sums": "test_aln_error_sums", "k_aln_marks+k_aln_fold": "test_aln_error_sums",
           "k_qv": "test_qv_probs", "k_cand_select+k_cand_choose": "test_candidates",
           "rf_download_band": "test_dp_probe"}


def probe_reads(name):
    _, key, idx, _ = PROBE[name]
    return cluster_of(key), list(idx)


def probe_lengths(name):
    """(m, n per read) of a probe without building its inputs where a rule gives them."""
    _, key, idx, _ = PROBE[name]
    if key in TIERS:
        m = TIERS[key][1]
        return m, [m + (DNS + DNS)[k] for k in idx]
    c = cluster_of(key)
    return c.m, [len(c.reads[k]) for k in idx]


def probe_bw(name):
    _, key, idx, _ = PROBE[name]
    if key in TIERS:
        return [TIERS[key][2]] * len(idx)
    c = cluster_of(key)
    return [c.bw or c.reads[k].bandwidth for k in idx]


def cluster_tables(key):
    """Per read of a cluster: (n, codon insertion entries, codon deletion
    entries, finite tables).  A tier's reads: three with Phred-0 or -Inf
    entries, then three finite ones, none with codon tables."""
    if key in TIERS:
        m = TIERS[key][1]
        return [(m + d, 0, 0, k >= 3) for k, d in enumerate(DNS + DNS)]
    return [(len(r), len(r.codon_ins_scores), len(r.codon_del_scores), True) for r in cluster_of(key).reads]


FILL_N, FILL_BW = 2000, 90          # the filler pair: H 181, lean


class BandPlan:
    """Ids, slots and the planned layout of the band world, from lengths alone."""

    def __init__(self):
        L = self.layout = Layout()
        self.seq0, self.tpl, at = {}, {}, 0
        keys, tlens = [], []
        for _, key, _, _ in DP_PROBES:
            if key not in keys:
                keys.append(key)
        for i, key in enumerate(keys):
            name = next(p[0] for p in DP_PROBES if p[1] == key)
            m, _ = probe_lengths(name)
            tabs = cluster_tables(key)
            lens = [x[0] for x in tabs]
            L.sequences(at, lens, [x[1] for x in tabs], [x[2] for x in tabs])
            self.seq0[key], self.tpl[key] = at, i
            at += len(lens)
            tlens.append(m)
        L.templates(range(len(keys)), tlens)     # one rf_set_templates_ids call after the reads
        self.fill_seq, self.tune_seq = at, at + 1
        self.fill_tpl, self.tune_tpl = len(keys), len(keys) + 1
        # canaries
        self.lo, self.hi, slot = {}, {}, 0
        for name, key, idx, _ in DP_PROBES:
            self.lo[name] = list(range(slot, slot + len(idx)))
            slot += len(idx)
            L.fill(self.jobs(name, self.lo[name]))
        self.canary_top = L.top["band"]
        # filler: ends half a first band below the line
        first = self.probe_band_bytes(DP_PROBES[0][0], 0)
        target = LINE - align_up(first // 2, 256)
        fb = region_bytes((band_rows(FILL_N, FILL_N, FILL_BW) + 2 * FILL_N) * band_stride(181, True) * 8)
        self.nfill = (target - self.canary_top) // fb
        rest = target - self.canary_top - self.nfill * fb
        if rest < 768:
            self.nfill -= 1
            rest += fb
        self.tune_m = rest // 256 - 2      # H 3 padded: (3 + 2 m) 16 doubles in 256-byte regions
        L.sequences(self.fill_seq, [FILL_N])
        L.sequences(self.tune_seq, [self.tune_m])
        L.templates([self.fill_tpl, self.tune_tpl], [FILL_N, self.tune_m])
        self.fill_slots = list(range(slot, slot + self.nfill + 1))
        slot += self.nfill + 1
        L.fill(self.filler_jobs(), RF_FWD)
        self.filler_top = L.top["band"]
        for name, key, idx, _ in DP_PROBES:
            self.hi[name] = list(range(slot, slot + len(idx)))
            slot += len(idx)
            L.fill(self.jobs(name, self.hi[name]))
        self.reserve = L.top["band"] - ARENA_GUARD + (1 << 20)
        # rf_reserve on an empty arena (arena_grow_impl)
        cap = self.reserve + 2 * ARENA_GUARD
        self.band_cap = align_up(cap + cap // 8 + (1 << 20), 1 << 20)

    def jobs(self, name, slots):
        _, key, idx, _ = PROBE[name]
        return [(s, self.seq0[key] + k, self.tpl[key], bw) for s, k, bw in zip(slots, idx, probe_bw(name))]

    def filler_jobs(self):
        return ([(s, self.fill_seq, self.fill_tpl, FILL_BW) for s in self.fill_slots[:-1]] +
                [(self.fill_slots[-1], self.tune_seq, self.tune_tpl, 1)])

    def probe_band_bytes(self, name, k):
        m, ns = probe_lengths(name)
        Hs = [band_rows(n, m, bw) for n, bw in zip(ns, probe_bw(name))]
        return region_bytes((Hs[k] + 2 * m) * band_stride(Hs[k], max(Hs) >= BAND_PAD_H) * 8)

    def host_launches(self, name):
        """rf_host_dp_plan of the probe's call: the launches the engine must report."""
        _, key, idx, opts = PROBE[name]
        m, ns = probe_lengths(name)
        tabs = [cluster_tables(key)[k] for k in idx]
        P = [self.layout.geom[(s, RF_BAND_A)][3] for s in self.lo[name]]
        _, _, _, _, launches = _lib.host_dp_plan(
            ns, [m] * len(ns), probe_bw(name), RF_FWD | RF_BWD, ncins=[x[1] for x in tabs],
            ncdel=[x[2] for x in tabs], finite=[x[3] for x in tabs], stride_a=P, stride_b=P,
            **{"dp_lat": 0, **opts})
        return [(L.kernel, L.npi, L.pmi, L.first, L.count) for L in launches]


_PLAN = []


def band_plan():
    if not _PLAN:
        _PLAN.append(BandPlan())
    return _PLAN[0]


# ---------------------------------------------------------------------
# 3. CPU tests: the planned layout and the coverage
# ---------------------------------------------------------------------
def test_layout_rules_small():
    """plan_layout's rules on a hand-computed case: guard, 256-byte regions,
    forward bands before backward bands, the per-call padding rule and the
    partner stride."""
    L = Layout()
    L.sequences(0, [10, 100])
    L.templates([0], [10])
    assert L.tabs == {0: (65536, 512), 1: (66048, 4096)}        # 51 and 501 doubles
    assert L.bases == {0: (65536, 256), 1: (65792, 256)} and L.tpl == {0: (66048, 256)}
    L.fill([(0, 0, 0, 3)])                                       # H 7, P 5, K 27: 1,080 bytes
    assert L.band == {(0, 0): (65536, 1280), (0, 1): (66816, 1280)}
    L.fill([(1, 0, 0, 3), (2, 1, 0, 3)], RF_FWD)                 # H 97 pads the call: P 16 and 64
    assert 27 * 16 * 8 == 3456 and 117 * 64 * 8 == 59904         # regions: 3,584 and 59,904 bytes
    assert L.band[(1, 0)] == (68096, 3584) and L.band[(2, 0)] == (68096 + 3584, 59904)
    L.fill([(1, 0, 0, 3)], RF_BWD)                               # alone it would not pad: the partner's stride
    assert L.band[(1, 1)] == (68096 + 3584 + 59904, 3584)
    assert L.top["band"] == 68096 + 3584 + 59904 + 3584


def test_planned_layout_reaches_the_lines():
    p = band_plan()
    L = p.layout
    first = p.hi[DP_PROBES[0][0]][0]
    off, cap = L.band[(first, RF_BAND_A)]
    assert off == p.filler_top and off % 8 == 0
    # (a) the first probe band straddles 2^31 doubles, with room on both sides
    assert off // 8 < LINE_DOUBLES < (off + cap) // 8
    assert min(LINE - off, off + cap - LINE) >= cap // 4
    # (b) every other probe band starts above it; (c) its offset modulo 2^32 lies in the canary area
    others = [(s, w) for name in p.hi for s in p.hi[name] for w in (RF_BAND_A, RF_BAND_B) if (s, w) != (first, 0)]
    assert len(others) == 2 * sum(len(p[2]) for p in DP_PROBES) - 1
    for key in others:
        o, c = L.band[key]
        assert o // 8 > LINE_DOUBLES and o >= LINE
        assert ARENA_GUARD <= o % (1 << 32) and o % (1 << 32) + c <= p.canary_top, key
    # the straddling band's cells above the line land on the guard and the first canary band
    assert ARENA_GUARD < (off + cap) % (1 << 32) <= L.band[(p.lo[DP_PROBES[0][0]][0], 0)][0] + cap
    # every canary lies below 2^32 bytes, the filler in between
    assert p.canary_top < 1 << 30 and all(L.band[(s, w)][0] + L.band[(s, w)][1] <= p.canary_top
                                          for name in p.lo for s in p.lo[name] for w in (0, 1))
    assert p.nfill > 5000 and 1 <= p.tune_m < 13000
    assert L.band[(p.fill_slots[-1], 0)][1] == 256 * (p.tune_m + 2)
    # (d) memory: the reservation, the tables and scratch stay far below the cap
    assert p.band_cap + 2 * GIB < MEMORY_CAP and p.band_cap < 19 * GIB


def test_every_dp_family_has_a_probe():
    """From rf_host_dp_plan over the module's own probe list: every DP family
    the issue names is what some probe's call launches, so a probe that the
    engine runs as planned (asserted on the GPU) runs it high."""
    p = band_plan()
    seen = set()
    for name, key, idx, opts in DP_PROBES:
        for kernel, npi, _, _, count in p.host_launches(name):
            assert count > 0
            seen |= {(kernel, npi), (kernel, None)}
            if name == "longref":
                assert kernel == "dpx_codon"
    missing = [f for f in DP_FAMILIES if f not in seen]
    assert not missing, (missing, sorted(seen, key=str))
    # the lean wide tasks too, the product's default for H 64..255
    assert ("dpr_wide64", None) in seen and ("dpr_wide32", None) in seen
    # k_dpm and its one-workgroup form fill the same bands
    assert PROBE["dpm"][1:3] != PROBE["dpwide"][1:3] and TIERS["dpm"][1:] == TIERS["dpwide"][1:]
    assert PROBE["dpm"][3] == {"dp_mc": 1} and PROBE["dpwide"][3] == {"dp_mc": 0}


def score_plan(kern, mode, per_seq):
    name, idx = SCORE_PROBE
    m, ns = probe_lengths(name)
    ns = [ns[k] for k in idx]
    p = band_plan()
    P = [p.layout.geom[(p.lo[name][k], RF_BAND_A)][3] for k in idx]
    return _lib.host_score_plan(ns, [m] * len(ns), [probe_bw(name)[k] for k in idx], [0, len(ns)], stride=P,
                                per_seq=per_seq, empty_ok=per_seq,
                                score_kernel=_lib.OPTION_VALUES["score_kernel"][kern],
                                score_mode=_lib.OPTION_VALUES["score_mode"][mode])


def test_every_scorer_and_reader_has_a_probe():
    """From rf_host_score_plan: the scoring probe reaches k_score, k_score_ws
    and k_score_segl, each fused and split, through rf_score_dense and through
    rf_score with per-read output; and every other reader the issue names has
    its test in this module."""
    seen = set()
    for kern, mode in SCORE_CASES:
        for per_seq in (False, True):
            sp = score_plan(kern, mode, per_seq)
            seen.add((sp.kernel, sp.split_score if per_seq else sp.split_dense, per_seq))
    # rf_score with per-read output always runs split: the per-read values are the partials
    assert seen == ({(k, s, False) for k in SCORE_KERNELS for s in (False, True)} |
                    {(k, True, True) for k in SCORE_KERNELS})
    assert set(READERS) == {"k_codon", "k_codon_dense", "k_bt_win", "k_bt_win+mask", "k_aln_sums",
                            "k_aln_marks+k_aln_fold", "k_qv", "k_cand_select+k_cand_choose", "rf_download_band"}
    for test in READERS.values():
        assert callable(globals()[test]) and "gpu" in [m.name for m in globals()[test].pytestmark]
    assert set(BT_CASES) == {(kb, nw) for kb in (16, 32) for nw in (4, 1)}


# ---------------------------------------------------------------------
# 4. the band world
# ---------------------------------------------------------------------
_TIMES = {}


def record(key, value):
    """One GPU run's figures; written to the file the RIFRAF_HIGH_OFFSETS_TIMING
    environment variable names, if it is set (profiles/high_offsets_timing.json
    is from such a run)."""
    _TIMES[key] = value
    if os.environ.get("RIFRAF_HIGH_OFFSETS_TIMING"):
        with open(os.environ["RIFRAF_HIGH_OFFSETS_TIMING"], "w") as f:
            json.dump(_TIMES, f, indent=1, sort_keys=True)
            f.write("\n")


@pytest.fixture(autouse=True)
def _wall_time(request):
    t0 = time.perf_counter()
    yield
    if request.node.get_closest_marker("gpu"):
        record("test_s/" + request.node.name, round(time.perf_counter() - t0, 3))


@contextlib.contextmanager
def options(engine, **kw):
    old = {k: engine.set_option(k, v) for k, v in kw.items()}
    try:
        yield
    finally:
        for k, v in old.items():
            engine.set_option(k, v)


def band_bits(engine, slot, which):
    return engine.download_band(slot, which).data.view(np.int64).copy()


class World:
    pass


_BAND_WORLD = []


def close_band_world():
    """The two engines are never alive at once: the table world closes the
    band world's engine (its tests come first in the file) before it creates
    its own."""
    for w in _BAND_WORLD:
        if w.e.ctx:
            w.peak = max(w.peak, w.e.device_bytes())
            w.e.close()


@pytest.fixture(scope="module")
def world():
    """The band engine with canaries, filler and probes laid out and filled;
    the layout is checked against the plan before anything is compared."""
    p = band_plan()
    t_setup = time.perf_counter()
    e = Engine(0)
    w = World()
    w.e, w.p = e, p
    try:
        e.set_option("dp_lat", 0)
        for key, first in p.seq0.items():
            cluster_of(key).upload(e, first)
        e.set_templates_ids([p.tpl[k] for k in p.tpl], [cluster_of(k).t for k in p.tpl])
        rng = np.random.default_rng(1 << 34)
        t_fill = random_seq(FILL_N, rng)
        w.fill_read = RifrafSequence(*sampled(t_fill, FILL_N, rng), FILL_BW, SEQ_SCORES)
        t_tune = random_seq(p.tune_m, rng)
        tune_read = RifrafSequence(*sampled(t_tune, p.tune_m, rng), 1, SEQ_SCORES)
        e.set_sequences(p.fill_seq, [w.fill_read, tune_read])
        e.set_templates_ids([p.fill_tpl, p.tune_tpl], [t_fill, t_tune])
        w.t_fill = t_fill
        e.reserve(p.reserve)
        reserved = e.device_bytes()

        def fill(name, slots):
            jobs = p.jobs(name, slots)
            with options(e, **PROBE[name][3]):
                sc = e.realign([j[0] for j in jobs], [j[1] for j in jobs], [j[2] for j in jobs],
                               [j[3] for j in jobs], RF_FWD | RF_BWD)
                launches = [(L.kernel, L.npi, L.pmi, L.first, L.count) for L in e.last_dp_launches()]
            return sc.copy(), launches

        w.lo = {name: fill(name, p.lo[name]) for name, *_ in DP_PROBES}
        w.kept = {(s, which): band_bits(e, s, which) for name in p.lo for s in p.lo[name] for which in (0, 1)}
        jobs = p.filler_jobs()
        t0 = time.perf_counter()
        w.fill_scores = e.realign([j[0] for j in jobs], [j[1] for j in jobs], [j[2] for j in jobs],
                                  [j[3] for j in jobs], RF_FWD).copy()
        record("band_filler_fill_s", round(time.perf_counter() - t0, 3))
        record("band_filler_dp_ms", round(e.last_timing()[0], 3))
        record("band_filler_bands", len(jobs))
        record("band_filler_launches", [[L.kernel, L.npi, L.count] for L in e.last_dp_launches()])
        w.hi = {name: fill(name, p.hi[name]) for name, *_ in DP_PROBES}
        # the engine's own word on where everything lies
        # scratch (task descriptors, scores) grows by a few MB; a band arena that
        # grew would have been allocated again at 1.5 times its 18 GiB
        assert e.device_bytes() - reserved < GIB, "the band arena grew: regions moved"
        for key, (off, cap) in p.layout.band.items():
            assert e.band_region(*key) == (off, cap), key
        for i, (off, cap) in p.layout.tabs.items():
            assert e.seq_regions(i) == ((off, cap), p.layout.bases[i]), i
        w.peak = e.device_bytes()
        record("band_world_setup_s", round(time.perf_counter() - t_setup, 3))
        _BAND_WORLD.append(w)
        yield w
        close_band_world()
        record("band_engine_peak_device_bytes", w.peak)
    finally:
        e.close()


pytest_gpu = pytest.mark.gpu


def both(w, name, idx, fn):
    """fn(slots) on the canary slots and on the probe slots of reads `idx`
    of probe `name`: (low result, high result)."""
    lo = fn(np.asarray([w.p.lo[name][k] for k in idx], np.int32))
    hi = fn(np.asarray([w.p.hi[name][k] for k in idx], np.int32))
    return lo, hi


@pytest_gpu
def test_layout_matches_plan(world):
    """rf_region_offsets against the plan (asserted region by region in the
    fixture): one probe band straddles 2^31 doubles, the rest lie above, and
    the peak stays under the memory cap."""
    e, p = world.e, world.p
    first = p.hi[DP_PROBES[0][0]][0]
    off, cap = e.band_region(first, RF_BAND_A)
    assert off // 8 < LINE_DOUBLES < (off + cap) // 8
    for name in p.hi:
        for s in p.hi[name]:
            for which in (0, 1):
                if (s, which) != (first, 0):
                    assert e.band_region(s, which)[0] // 8 > LINE_DOUBLES
    assert e.band_region(p.fill_slots[-1])[0] + e.band_region(p.fill_slots[-1])[1] == off
    assert e.device_bytes() < MEMORY_CAP
    with pytest.raises(Exception):
        e.band_region(p.hi[DP_PROBES[-1][0]][-1] + 1)
    with pytest.raises(Exception):
        e.band_region(p.fill_slots[0], RF_BAND_B)      # the filler filled no B band
    with pytest.raises(Exception):
        e.seq_regions(p.tune_seq + 1)


@pytest_gpu
def test_filler_scores(world):
    """The filler's own results: every one of its bands ends in the oracle's
    A[end, end] (one 2,000-base forward fill on the CPU)."""
    A, _ = oracle.forward(world.t_fill, world.fill_read, bandwidth=FILL_BW)
    exp = final_cell(A, FILL_N, FILL_N, FILL_BW)
    assert bits_equal(world.fill_scores[:-1], np.full(world.p.nfill, exp))


@pytest_gpu
@pytest.mark.parametrize("name", [p[0] for p in DP_PROBES])
def test_dp_probe(world, name):
    """One probe's fill above the line: the launches are the planned family's,
    rf_download_band of A and B equals the oracle and the canary's bits, the
    scores equal the oracle's and the canary call's."""
    e, p = world.e, world.p
    c, idx = probe_reads(name)
    want = p.host_launches(name)
    assert world.lo[name][1] == want and world.hi[name][1] == want
    assert bits_equal(world.hi[name][0], world.lo[name][0])
    bws = probe_bw(name)
    for j, k in enumerate(idx):
        r = c.reads[k]
        A = c.fwd(k)[0]
        assert bits_equal(world.hi[name][0][j:j + 1], [final_cell(A, len(r), c.m, bws[j])]), (name, k)
        for which, exp in ((RF_BAND_A, A), (RF_BAND_B, c.bwd(k))):
            got = e.download_band(p.hi[name][j], which)
            assert_band_equal(got, exp, len(r) + 1, c.m + 1, bws[j])
            low = e.download_band(p.lo[name][j], which)
            assert_band_equal(low, exp, len(r) + 1, c.m + 1, bws[j])
            # every stored cell, the out-of-band ones included
            assert np.array_equal(got.data.view(np.int64), world.kept[(p.lo[name][j], which)]), (name, k, which)


def dense_expected(c, idx):
    reads = [c.reads[k] for k in idx]
    props = all_proposals_arrays(c.t)
    tot, per = oracle_scores(c.t, props, reads, [c.fwd(k)[0] for k in idx], [c.bwd(k) for k in idx])
    return props, tot, per


@pytest_gpu
@pytest.mark.parametrize("kern,mode", SCORE_CASES)
def test_scorers(world, kern, mode):
    """k_score, k_score_ws and k_score_segl, fused and split, through
    rf_score_dense and through rf_score with per-read output, on bands above
    the line; then k_score on the whole probe, Phred-0 reads included."""
    e = world.e
    name, idx = SCORE_PROBE
    c, _ = probe_reads(name)
    cases = [(idx, kern)] + ([(tuple(range(6)), "general")] if kern == "general" else [])
    for ids, want in cases:
        props, tot, per = dense_expected(c, ids)
        mask = dense_mask(c.t)
        with options(e, score_kernel=kern, score_mode=mode):
            def dense(slots):
                out = e.score_dense([slots])[0].copy()
                assert_score_launch(e, want, mode)
                return out

            def listed(slots):
                ok = ~np.isnan(tot)
                out = e.score([(slots, -1, tuple(a[ok] for a in props))], per_seq=True)
                assert_score_launch(e, want, "split")     # per-read output: the partials are the result
                return out[0][0], out[1][0]

            lo, hi = both(world, name, ids, dense)
            assert same(hi[mask], table(c.t, props, tot)[mask]).all() and same(hi, lo).all(), (kern, mode, ids)
            (lt, lp), (ht, hp) = both(world, name, ids, listed)
            ok = ~np.isnan(tot)
            assert same(ht, tot[ok]).all() and same(hp, per[ok]).all(), (kern, mode, ids)
            assert same(ht, lt).all() and same(hp, lp).all()


@pytest_gpu
def test_reference_scoring(world):
    """k_codon (rf_score with a reference slot) and k_codon_dense
    (rf_score_dense_ref) on a reference whose bands lie above the line."""
    e = world.e
    c = cluster_of("ref")
    exp = c.case.oracle_table()
    mask = dense_mask(c.t)

    def listed(slots):
        tot, per = e.score([(slots[:3], int(slots[3]), c.case.props)], per_seq=True)
        assert e.last_codon_ms() > 0
        return tot[0], per[0]

    def dense(slots):
        out = e.score_dense_ref([slots[:3]], [int(slots[3])])[0].copy()
        assert e.last_codon_dense_ms() > 0
        return out

    (lt, lp), (ht, hp) = both(world, "ref", range(4), listed)
    assert same(table(c.t, c.case.props, ht)[mask], exp[mask]).all()
    assert same(ht, lt).all() and same(hp, lp).all()
    lo, hi = both(world, "ref", range(4), dense)
    assert same(hi[mask], exp[mask]).all() and same(hi, lo).all()


@pytest_gpu
@pytest.mark.parametrize("win_kb,nw", BT_CASES)
def test_backtrace(world, win_kb, nw):
    """k_bt_win with 16 and 32 KB windows, on 4 waves and on 1 per walk."""
    e = world.e
    with options(e, bt_win_kb=win_kb, bt_nw=nw):
        for name in BT_PROBES:
            c, idx = probe_reads(name)
            (lm, le), (hm, he) = both(world, name, range(len(idx)), lambda s: e.backtrace(s))
            for j, k in enumerate(idx):
                _, walk, nerr = c.fwd(k)
                np.testing.assert_array_equal(hm[j], walk, err_msg=f"{name} read {k}")
                np.testing.assert_array_equal(hm[j], lm[j])
                assert he[j] == nerr == le[j]


@pytest_gpu
@pytest.mark.parametrize("do_indels", [True, False])
def test_alignment_proposals(world, do_indels):
    """k_bt_win marking the proposal mask, with and without indels."""
    e = world.e
    for name in ("np8", "np2"):
        c, idx = probe_reads(name)
        lo, hi = both(world, name, range(len(idx)), lambda s: e.alignment_proposals([s], do_indels)[0].copy())
        exp = proposals_mask(c.t, [c.fwd(k)[1] for k in idx], [c.reads[k] for k in idx])
        if not do_indels:
            exp[:, 4:] = 0
        np.testing.assert_array_equal(hi, exp)
        np.testing.assert_array_equal(hi, lo)


@pytest_gpu
@pytest.mark.parametrize("marks_min", [128, 0])
def test_aln_error_sums(world, marks_min):
    """The device folds of rf_aln_error_sums: k_aln_sums (aln_marks_min 128)
    and k_aln_marks + k_aln_fold (0).  The host tables are withheld, so a host
    fold would return None."""
    e = world.e
    for name in ("np2", "np8"):
        c, idx = probe_reads(name)
        with options(e, aln_marks_min=marks_min):
            lo, hi = both(world, name, range(len(idx)),
                          lambda s: e.aln_error_sums_ptr([s], [c.m], None, None, [len(c.reads[k]) for k in idx]))
        assert hi is not None and lo is not None, "a read has no row codes: the device fold did not run"
        exp = np.zeros((c.m, 4))
        _add_base_distributions(exp, [c.fwd(k)[1] for k in idx], [c.reads[k] for k in idx])
        assert same(hi[0], exp).all() and same(hi[0], lo[0]).all(), (name, marks_min)


@pytest_gpu
def test_qv_probs(world):
    """k_qv at test_small_geometry's 80-bit check and tolerance, and equal to
    the same call on the canaries bit for bit."""
    from test_small_geometry import check_qv_probs
    if np.finfo(np.longdouble).nmant < 63:
        pytest.skip("np.longdouble has fewer than 64 significand bits on this host")
    e, p = world.e, world.p
    name, idx = SCORE_PROBE
    c, _ = probe_reads(name)
    reads = [c.reads[k] for k in idx]
    out = {}
    for side, slots, scores in (("lo", p.lo[name], world.lo[name][0]), ("hi", p.hi[name], world.hi[name][0])):
        g = np.asarray([slots[k] for k in idx], np.int32)
        sc = {int(s): scores[k] for s, k in zip(g, idx)}
        check_qv_probs(e, [g], [c.t], [reads], sc)
        state = 0.0
        for s in g:
            state += float(sc[int(s)])
        out[side] = e.qv_probs([g], [c.m], [state])
    for a, b in zip(out["lo"][:3], out["hi"][:3]):
        assert same(a, b).all()


@pytest_gpu
@pytest.mark.parametrize("md", [0, 5])
def test_candidates(world, md):
    """k_cand_select and k_cand_choose behind the dense table, the reference
    term included, against the host filter and choose_candidates over the
    oracle's totals."""
    from rifraf_amd.model import Stage, all_proposals
    from rifraf_amd.proposals import ScoredProposal, choose_candidates
    import test_candidates_host as H
    e = world.e
    c = cluster_of("ref")
    exp_table = c.case.oracle_table()
    props = all_proposals(Stage.INIT, c.t, False)
    totals = [exp_table[q.pos, H.slot_of(q)] for q in props]
    score = float(np.sort(totals)[len(totals) // 2])          # half of the proposals are candidates
    cands = [ScoredProposal(q, float(s)) for q, s in zip(props, totals) if s > score]
    chosen = choose_candidates(cands, md)
    assert len(cands) > 20 and len(chosen) >= 1
    lo, hi = both(world, "ref", range(4), lambda s: e.candidates([s[:3]], [score], [0], md, ref_slots=[int(s[3])],
                                                                 with_counts=True)[0])
    for got in (lo, hi):
        H.same(got[0], cands)
        H.same(got[1], chosen)
        assert got[2:] == (len(cands), len(chosen))


@pytest_gpu
def test_canaries_survive(world):
    """After every fill and every reader above the line, the canary bands at
    the bottom of the arena still hold the bits of their first fill."""
    e = world.e
    assert len(world.kept) == 2 * sum(len(p[2]) for p in DP_PROBES)
    for (slot, which), bits in world.kept.items():
        assert np.array_equal(band_bits(e, slot, which), bits), (slot, which)
    assert e.device_bytes() < MEMORY_CAP


# ---------------------------------------------------------------------
# 5. the table world
# ---------------------------------------------------------------------
TAB_TIER = "dpr2"                   # m 80, bw 24: lean and general k_dpr<2>
TAB_FILL_N, TAB_FILL_READS = 100_000, 1080
TAB_LINE = 1 << 32


class TablePlan:
    """ids: 0..5 canary tables, 6..11 canary codes, 12..1091 the filler,
    then the same twelve reads as probes."""

    def __init__(self):
        m = TIERS[TAB_TIER][1]
        lens = [m + d for d in DNS + DNS]
        L = self.layout = Layout()
        L.sequences(0, lens)
        L.sequences(6, lens)
        self.fill0 = 12
        L.sequences(self.fill0, [TAB_FILL_N] * TAB_FILL_READS)
        self.hi = self.fill0 + TAB_FILL_READS
        L.sequences(self.hi, lens)
        L.sequences(self.hi + 6, lens)
        L.templates([0], [m])


def test_planned_tables_reach_the_line():
    p = TablePlan()
    L = p.layout
    assert all(L.tabs[i][0] + L.tabs[i][1] < 1 << 20 for i in range(12))
    assert all(L.tabs[p.hi + k][0] > TAB_LINE for k in range(12))
    assert L.tabs[p.hi][0] - TAB_LINE < 64 << 20                 # no more filler than the line needs
    assert all(L.bases[p.hi + k][0] > 100 << 20 for k in range(12))
    # the arena's growth margin of one eighth, the bases and the pair kernels' scratch
    assert L.top["tabs"] * 9 // 8 + L.top["bytes"] * 9 // 8 + GIB < 6 * GIB < MEMORY_CAP


@pytest.fixture(scope="module")
def table_world():
    p = TablePlan()
    c = case_of(TAB_TIER, "phred0-codes")
    close_band_world()
    t_setup = time.perf_counter()
    e = Engine(0)
    w = World()
    w.e, w.p, w.c = e, p, c
    try:
        e.set_option("dp_lat", 0)
        e.set_option("dp_nl64", 0)
        for first in (0, p.hi):
            if first:
                rng = np.random.default_rng(1 << 32)
                n = TAB_FILL_N * TAB_FILL_READS
                bases = rng.integers(0, 4, n, dtype=np.uint8)
                codes = rng.integers(1, 41, n, dtype=np.uint8)
                t0 = time.perf_counter()
                assert e.set_sequences_codes(p.fill0, bases, np.arange(TAB_FILL_READS + 1, dtype=np.int64) * TAB_FILL_N,
                                             codes, LP_TABLE, MATCH_TABLE, SEQ_SCORES)
                record("table_filler_upload_s", round(time.perf_counter() - t0, 3))
                del bases, codes
            e.set_sequences(first, c.reads)
            assert e.set_sequences_codes(first + 6, c.bases, c.off, c.codes, LP_TABLE, MATCH_TABLE, SEQ_SCORES)
        e.set_templates(0, [c.t])
        for i, (off, cap) in p.layout.tabs.items():
            if i < p.fill0 or i >= p.hi or i in (p.fill0, p.hi - 1):
                assert e.seq_regions(i) == ((off, cap), p.layout.bases[i]), i
        sl = np.arange(12)
        w.first_scores = e.realign(sl, sl, 0, [c.bw] * 12, RF_FWD | RF_BWD).copy()
        w.kept = {(s, which): band_bits(e, s, which) for s in range(12) for which in (0, 1)}
        record("table_world_setup_s", round(time.perf_counter() - t_setup, 3))
        yield w
        record("table_engine_peak_device_bytes", e.device_bytes())
    finally:
        e.close()


def pairs_both(w, fn):
    """fn(sequence ids) on the low copies and on the probes: twelve pairs each."""
    return fn(np.arange(12, dtype=np.int32)), fn(np.arange(w.p.hi, w.p.hi + 12, dtype=np.int32))


@pytest_gpu
def test_tables_high_realign(table_world):
    """rf_realign of the probe reads (tables and row codes above 2^32 bytes),
    lean and general tier in one call, against the oracle and the low copies."""
    w = table_world
    e, c, p = w.e, w.c, w.p
    for i in range(12):
        assert e.seq_regions(p.hi + i)[0][0] > TAB_LINE
    assert e.device_bytes() < MEMORY_CAP
    sl = np.arange(12, 24)
    sc = e.realign(sl, np.arange(p.hi, p.hi + 12), 0, [c.bw] * 12, RF_FWD | RF_BWD)
    kinds = {L.kernel for L in e.last_dp_launches()}
    assert "dpr" in kinds and kinds & {"dpr_lean", "dpr_lean_pm"}, kinds
    assert bits_equal(sc, w.first_scores)
    for i in range(12):
        k = i % 6
        r = c.reads[k]
        assert bits_equal(sc[i:i + 1], [final_cell(c.fwd(k)[0], len(r), c.m, c.bw)])
        for which, exp in ((RF_BAND_A, c.fwd(k)[0]), (RF_BAND_B, c.bwd(k))):
            got = e.download_band(12 + i, which)
            assert_band_equal(got, exp, len(r) + 1, c.m + 1, c.bw)
            assert np.array_equal(got.data.view(np.int64), w.kept[(i, which)])
    # the device fold of the alignment sums reads the row-code records of the coded probes
    for marks_min in (128, 0):
        with options(e, aln_marks_min=marks_min):
            got = e.aln_error_sums_ptr([np.arange(18, 24, dtype=np.int32)], [c.m], None, None,
                                       [len(r) for r in c.reads])
        assert got is not None
        exp = np.zeros((c.m, 4))
        _add_base_distributions(exp, [c.fwd(k)[1] for k in range(6)], c.reads)
        assert same(got[0], exp).all(), marks_min


@pytest_gpu
@pytest.mark.parametrize("walk", [1, 2])
def test_tables_high_pairs(table_world, walk):
    """The pair kernels on tables above 2^32 bytes, under both walks:
    rf_pair_scores, rf_pair_align, rf_pair_errors, rf_pair_align_smart,
    rf_pair_align_text and rf_pair_shifts against the oracle's fills and walks
    (the host functions over its moves) and the low copies."""
    w = table_world
    e, c = w.e, w.c
    m, bw = c.m, c.bw
    want = [c.fwd(i % 6) for i in range(12)]
    finals = [final_cell(A, len(c.reads[i % 6]), m, bw) for i, (A, _, _) in enumerate(want)]
    caps = np.array([len(c.reads[i % 6]) + m for i in range(12)], np.int64)
    with options(e, pair_walk=walk):
        lo, hi = pairs_both(w, lambda ids: e.pair_scores(ids, 0, bw))
        assert bits_equal(hi, finals) and bits_equal(hi, lo)
        lo, hi = pairs_both(w, lambda ids: e.pair_align(ids, 0, bw, caps=caps))
        assert bits_equal(hi[0], finals) and bits_equal(lo[0], finals)
        for i in range(12):
            np.testing.assert_array_equal(hi[1][i], want[i][1])
            np.testing.assert_array_equal(lo[1][i], want[i][1])
        assert hi[2].tolist() == [x[2] for x in want] == lo[2].tolist()
        lo, hi = pairs_both(w, lambda ids: e.pair_errors(ids, 0, bw))
        assert bits_equal(hi[0], finals) and hi[1].tolist() == [x[2] for x in want] == lo[1].tolist()
        # band doubling from bw 3: each pair's last fill is the oracle's at the bandwidth it ended on
        thr = np.zeros(12)
        lo, hi = pairs_both(w, lambda ids: e.pair_align_smart(ids, 0, 3, thr, max_doublings=3, caps=caps))
        le, he = pairs_both(w, lambda ids: e.pair_errors(ids, 0, 3, thr, max_doublings=3))
        assert (hi[4] > 1).any(), "no pair doubled its band"
        for i in range(12):
            r = c.reads[i % 6]
            try:
                A, mv = oracle.forward(c.t, r, moves=True, bandwidth=int(hi[3][i]))
            except oracle.OracleError:      # "new score is invalid" at that bandwidth: NaN, no moves
                assert math.isnan(hi[0][i]) and hi[1][i] is None and lo[1][i] is None and hi[2][i] == -1
                continue
            walk_exp = oracle.backtrace(mv, len(r) + 1, m + 1, int(hi[3][i]))
            assert bits_equal(hi[0][i:i + 1], [final_cell(A, len(r), m, int(hi[3][i]))])
            np.testing.assert_array_equal(hi[1][i], walk_exp)
            np.testing.assert_array_equal(lo[1][i], walk_exp)
            assert hi[2][i] == oracle.count_errors(walk_exp, c.t, r.seq)
        for a, b in ((hi[0], lo[0]), (hi[0], he[0]), (he[0], le[0])):
            assert bits_equal(a, b)
        for a, b in ((hi[2], he[1]), (hi[3], he[2]), (hi[4], he[3]), (hi[2], lo[2]), (hi[3], lo[3]), (hi[4], lo[4])):
            assert a.tolist() == b.tolist()
        lo, hi = pairs_both(w, lambda ids: e.pair_align_text(ids, 0, bw, want_text=True, want_indices=True,
                                                             want_tolerance=True, caps=(caps, np.full(12, m))))
        for sc, r in (lo, hi):
            assert bits_equal(sc, finals) and r.nerrors.tolist() == [x[2] for x in want]
            for i in range(12):
                s = c.reads[i % 6]
                assert r.text(i) == moves_to_aligned_seqs(want[i][1], c.t, s.seq)
                assert r.indices(i).tolist() == moves_to_indices(want[i][1], m, len(s))
                assert r.tolerance[i] == band_tolerance(want[i][1], len(s) + 1, m + 1, bw)
        for flags in (0, RF_SKEW):
            wf = [c.fwd(i % 6, flags) for i in range(12)]
            exp = _lib.host_shift_fix([x[1] for x in wf], [c.reads[i % 6].seq for i in range(12)], [c.t] * 12)
            lo, hi = pairs_both(w, lambda ids: e.pair_shifts(ids, 0, bw, flags, want_fixed=True, want_proposals=True,
                                                             caps=caps))
            for sc, r in (lo, hi):
                assert bits_equal(sc, [final_cell(x[0], len(c.reads[i % 6]), m, bw) for i, x in enumerate(wf)])
                assert r.fixed_len.tolist() == exp.fixed_len.tolist() and r.nprops.tolist() == exp.nprops.tolist()
                assert r.tally.tolist() == exp.tally.tolist()
                for i in range(12):
                    assert r.proposals(i) == exp.proposals(i)
                    x, y = r.fixed_seq(i), exp.fixed_seq(i)
                    assert (x is None and y is None) or x.tolist() == y.tolist()


@pytest_gpu
def test_tables_canaries_survive(table_world):
    """The low copies' bands, refilled after all work on the probes, equal
    their first fill: nothing wrote into the low tables."""
    w = table_world
    e, c = w.e, w.c
    sl = np.arange(12)
    sc = e.realign(sl, sl, 0, [c.bw] * 12, RF_FWD | RF_BWD)
    assert bits_equal(sc, w.first_scores)
    for (slot, which), bits in w.kept.items():
        assert np.array_equal(band_bits(e, slot, which), bits), (slot, which)
    assert e.device_bytes() < MEMORY_CAP
