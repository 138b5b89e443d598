// rifraf_dp_plan.h -- host-side launch planning of the DP fills (rf_realign,
// the pair calls): the task descriptor, the band geometry the planners test
// and the planners.  No HIP: a plain C++17 compiler takes it alone.  The
// routing rules are stated once in DESIGN.md §4 "DP launch planner".
#ifndef RIFRAF_DP_PLAN_H
#define RIFRAF_DP_PLAN_H

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../include/rifraf_hip.h"
#ifdef __HIPCC__
#define RF_HD __host__ __device__
#else
#define RF_HD
#endif

// band geometry (the layout is described in rifraf_hip.hip)
inline int band_rows(int n, int m, int bw) { return 2 * bw + std::abs(n - m) + 1; }
RF_HD inline int band_P(int H) { return ((H + 1) >> 1) | 1; }
// Row stride of a band as allocated: H >= pad_h (> 0) gives rows of a whole
// number of 128-B lines, so that the wide-band scorer's 32-diagonal segments
// read exactly one line per kappa row (k_score_segl); else the odd stride.
// rf_realign pads every band of a call whose widest band has H >=
// RF_OPT_BAND_PAD (pad_h 1 for the call), none otherwise.
inline int band_stride(int H, int pad_h)
{
    return (pad_h > 0 && H >= pad_h) ? (((H + 1) >> 1) + 15) & ~15 : band_P(H);
}
RF_HD inline int64_t band_K(int H, int m) { return (int64_t)H + 2 * (int64_t)m; }
// What a band takes in the band arena: K kappa rows of P doubles, in a region
// rounded as every arena region is (region_ensure).  rf_realign's bookkeeping
// and rf_host_band_bytes both come here.
inline int64_t band_payload_bytes(int H, int m, int P) { return band_K(H, m) * P * 8; }
inline int64_t region_bytes(int64_t bytes) { return (std::max<int64_t>(bytes, 16) + 255) / 256 * 256; }
// One band of an (n+1) x (m+1) alignment at bandwidth bw, padded (the call's
// RF_OPT_BAND_PAD decision) or not; A and B are alike
inline int64_t band_region_bytes(int n, int m, int bw, bool pad)
{
    const int H = band_rows(n + 1, m + 1, bw);
    return region_bytes(band_payload_bytes(H, m, band_stride(H, pad ? 1 : 0)));
}

// One DP fill task = (slot, direction).
struct alignas(16) DPTask {
    int64_t band;   // output band offset (doubles)
    int64_t sb;     // sequence bases offset (bytes)
    int64_t tab;    // sequence tables offset (doubles)
    int64_t tb;     // template bases offset (bytes)
    int32_t n, m, bw, H;
    int32_t c;      // h_off + bw
    int32_t ncins, ncdel;
    int32_t flags;  // 1 = reverse, 2 = skew, 4 = trim
    int32_t out_idx;
    int32_t klen;   // number of anti-diagonals K = H + 2m
    int32_t P;      // kappa row stride
    int32_t pad;
};

// DPTask.flags bit: the read carries row codes (rf_set_sequences) -- one
// 8-B record per read position i: bits 0-15 the code of (match, mismatch,
// ins)[i], 16-31 / 32-47 the codes of del[i] / del[i+1], 48-55 the base.
// Codes index the context's dictionary: RF_CODES entries of 4 doubles
// {match, mismatch, ins, 0}, then RF_CODES del values.
constexpr int RF_TASK_CODED = 1024;

// The kernels' band limits as the planners use them.  rifraf_hip.hip defines
// each beside its kernel (DPW_LDS_H, PS_FAST_H, PS_GEN64_H: the tests read
// them there) and asserts that the two agree.
constexpr int DP_LDS_H = 5114;     // widest band whose four-diagonal ring fits the LDS of k_dp<DPW_NT>
constexpr int DP_FAST_H = 255;     // widest band of the register kernels (k_dpr<8>, the 64-lane tasks, k_ps<2, 64>)
constexpr int DP_GEN64_H = 2040;   // widest band of a one-wave LDS ring (k_dp<64>, k_ps_gen<64>: ring < 64 KB)
constexpr int DP_COUNT_H = 3407;   // widest band whose score ring and int32 count ring fit 160 KiB (k_pe_gen): 48 (H + 6) B

RF_HD constexpr int dpl_pmax(int np, int lpt = 16) { return (lpt * np) | 1; }   // band_P(2*LPT*NP-1)
// stride classes of the lean DP launches: k_dpr<1 << npi, true, dpr_pm(npi, pmi)>
// takes the lean tasks of NP class npi with P <= dpr_pm (the largest is the
// class maximum 16 * NP | 1)
RF_HD constexpr int dpr_pm(int npi, int pmi)
{
    // NP = 1: P <= 17 (H <= 31); NP = 2: 17..33; NP = 4: 33..65; NP = 8: 65..129
    return npi == 0 ? 11 + 2 * pmi : npi == 1 ? 19 + 4 * pmi + (pmi == 3 ? 2 : 0) : (((16 << npi) * (pmi + 5)) / 8) | 1;
}
// PFIX: every task of the launch has row stride exactly PM (the host routes
// only such tasks to it), so the blocked interior's LDS offsets i * P are
// compile-time immediates instead of one address register per step.
#ifndef DPR_PFIX
#define DPR_PFIX 1
#endif

// k_dpm's slice geometry (profiles/r06p_exp_dpm.out, configs[2]'s band, ms per
// call): 1 pair per lane, hand-off every 32 steps 0.745; every 16 0.822; 2
// pairs per lane, every 32 1.064, every 64 0.984 (k_dpw: 3.35)
#ifndef DPM_NPL_
#define DPM_NPL_ 1
#endif
#ifndef DPM_B_
#define DPM_B_ 32
#endif
constexpr int DPM_NPL = DPM_NPL_;                 // pairs per lane
constexpr int DPM_B = DPM_B_;                     // anti-diagonals per hand-off
constexpr int DPM_OWN = 64 * DPM_NPL - DPM_B;     // pairs per slice
RF_HD constexpr int dpm_slices(int H) { return ((H + 1) / 2 + DPM_OWN - 1) / DPM_OWN; }
// A band's slices spin on each other, so they must be resident together:
// at most DPM_TASK_SLICES per band (an XCD holds 8 of these 20-KB workgroups
// per CU, 32 CUs: 256).  Workgroups of one launch dispatch in order, so the
// bands of one XCD become resident one after another (each waits only for
// earlier bands, which are whole); wider bands take k_dp.  Launches from
// other streams (a second engine) interleave with it, so one launch keeps
// to DPM_XCD_SLICES per XCD (more bands: further launches on its stream).
constexpr int DPM_TASK_SLICES = 160;
constexpr int DPM_XCD_SLICES = 64;

// k_dpm and k_dpx address a band with 32-bit buffer offsets
inline bool band_below_2g(const DPTask &t) { return (int64_t)t.klen * t.P * 8 < ((int64_t)1 << 31); }
// a k_dpx task: H <= 127 (lanes hold diagonal pairs) and a band below 2 GiB
// (DPX_NOSTORE past it)
inline bool dpx_fits(const DPTask &t) { return t.H <= 127 && band_below_2g(t); }

// k_dpr's lean condition: finite tables, no codon moves, no skew / trim
inline bool dp_lean(const DPTask &t, bool finite) { return t.ncins == 0 && t.ncdel == 0 && finite && !(t.flags & 6); }
// NP class of the register kernels: H <= 32 * (1 << npi) - 1
inline int dp_npi(int H) { return H <= 31 ? 0 : H <= 63 ? 1 : H <= 127 ? 2 : 3; }
// smallest stride class of NP class npi that holds stride P
inline int dp_pmi(int npi, int P)
{
    int pmi = 0;
    while (pmi < 3 && P > dpr_pm(npi, pmi))
        ++pmi;
    return pmi;
}

// fn(dir, k) for every fill of a call, the forward ones (dir 0) first; stops
// at fn's first error
template <class F>
int for_each_fill(int32_t njobs, const int32_t *jf, F fn)
{
    for (int dir = 0; dir < 2; ++dir)
        for (int32_t k = 0; k < njobs; ++k)
            if (jf[k] & (dir == 0 ? RF_FWD : RF_BWD))
                if (int e = fn(dir, k))
                    return e;
    return 0;
}

#ifndef DP_WIDE_DEFAULT
#define DP_WIDE_DEFAULT 3
#endif
// The options the planner reads (rf_set_option keys, include/rifraf_hip.h)
struct DpOpts {
    int dp_wide = DP_WIDE_DEFAULT;   // RF_OPT_DP_WIDE: lean H 128..255 in 64 lanes (bit 0), 64..127 in 32 (bit 1)
    int dp_psplit = -1;     // RF_OPT_DP_PSPLIT: lean stride-class split mask (-1 auto)
    int dp_np8 = 1;         // RF_OPT_DP_NP8: H 128..255 in k_dpr<8> (0: k_dp<64>)
    int dp_np8_lean = 1;    // RF_OPT_DP_NP8_LEAN: lean k_dpr<8> path
    int dp_streams = 1;     // RF_OPT_DP_STREAMS: DP classes on concurrent streams
    int dp_nl64 = 1024;     // RF_OPT_DP_NL64: at most this many non-lean H <= 127 tasks run in k_dpx
    int dp_mc = 1;          // RF_OPT_DP_MC: H > 2040 bands without codon moves in k_dpm (0: k_dp)
    int dp_pfit = 1;        // RF_OPT_DP_PFIT: lean NP >= 2 class launched at its tasks' stride class
    int dp_lat = 2048;      // RF_OPT_DP_LAT: at most this many lean H <= 127 tasks all run in one k_dpx launch
};

// The option of an rf_set_option key (NULL: not a planner option)
inline int *dp_opt(DpOpts &o, int32_t key)
{
    const struct { int32_t key; int *v; } t[] = {
        {RF_OPT_DP_WIDE, &o.dp_wide}, {RF_OPT_DP_PSPLIT, &o.dp_psplit}, {RF_OPT_DP_NP8, &o.dp_np8},
        {RF_OPT_DP_NP8_LEAN, &o.dp_np8_lean}, {RF_OPT_DP_STREAMS, &o.dp_streams}, {RF_OPT_DP_NL64, &o.dp_nl64},
        {RF_OPT_DP_MC, &o.dp_mc}, {RF_OPT_DP_PFIT, &o.dp_pfit}, {RF_OPT_DP_LAT, &o.dp_lat}};
    for (const auto &e : t)
        if (e.key == key)
            return e.v;
    return nullptr;
}

// The kernel family of a launch (RF_DPK_* of the C-ABI)
enum class DpKernel : int {
    Dpr = RF_DPK_DPR,                 // k_dpr<1 << npi, false>: general step, four 16-lane tasks per wave
    DprLean = RF_DPK_DPR_LEAN,        // k_dpr<1 << npi, true>
    DprLeanPm = RF_DPK_DPR_LEAN_PM,   // k_dpr<1 << npi, true, dpr_pm(npi, pmi)> (NP = 1: exact stride, PFIX)
    DprWide64 = RF_DPK_DPR_WIDE64,    // k_dpr<2, true, .., 64>: lean H 128..255, one 64-lane task per wave
    DprWide32 = RF_DPK_DPR_WIDE32,    // k_dpr<2, true, .., 32>: lean H 64..127, two 32-lane tasks per wave
    DpxCodon = RF_DPK_DPX_CODON,      // k_dpx<true, true>: few non-lean H <= 127 tasks, one per wave
    DpxLean = RF_DPK_DPX_LEAN,        // k_dpx<false, false>: latency mode, lean H <= 127
    Dp64 = RF_DPK_DP64,               // k_dp<64>: H <= 2040, one task per wave, LDS ring
    DpwLds = RF_DPK_DPW_LDS,          // k_dp<DPW_NT>: one task per block, LDS ring
    DpwGlobal = RF_DPK_DPW_GLOBAL,    // k_dp<DPW_NT>: the ring in global memory (a band past DP_LDS_H)
    Dpm = RF_DPK_DPM,                 // k_dpm: band slices across the CUs of an XCD
};
// few long tasks: such a launch cannot fill the GPU, its step latency is the time
inline bool dp_latency_bound(DpKernel k) { return k == DpKernel::DpxCodon || (k >= DpKernel::Dp64 && k <= DpKernel::Dpm); }

struct DpLaunch {
    DpKernel k;
    int npi, pmi;   // NP class (Dpr, DprLean, DprLeanPm) and stride class (DprLeanPm); else 0
    size_t at, n;   // its tasks: [at, at + n) of the device order
    int stream;     // -1: the main stream, else a side stream
    int hmax;       // Dp64, DpwLds, DpwGlobal: the widest band; Dpm: the most slices of a band
};

struct DpPlan {
    std::vector<DPTask> tasks;        // device order: class by class, each longest first
    std::vector<DpLaunch> launches;   // issue order, streams assigned
};

// Sorts the tasks of one rf_realign call (every (job, direction), forward
// first; finite[i]: task i's tables hold no -Inf) into launches.
inline DpPlan dp_plan(const std::vector<DPTask> &in, const std::vector<uint8_t> &finite, const DpOpts &o)
{
    // the classes in device order
    enum { CR = 0, CP = CR + 8, CW = CP + 16, CX = CW + 2, CL, C64, CG, CWM, NCLS };
    std::vector<uint32_t> cls[NCLS];   // indices into `in`
    // RF_OPT_DP_PSPLIT: bit npi set = lean class NP = 1 << npi splits by stride
    // (auto: NP = 1 alone, when it is at least half of the tasks: c4 DP -5..9 %)
    size_t n1 = 0, nlat = 0;
    for (size_t i = 0; i < in.size(); ++i) {
        n1 += in[i].H <= 31;
        nlat += dp_lean(in[i], finite[i]) && in[i].H <= 127;
    }
    const int psplit = o.dp_psplit >= 0 ? o.dp_psplit : (2 * n1 < in.size() ? 0 : 1);
    // latency mode (RF_OPT_DP_LAT): few lean tasks of H <= 127 cannot fill the
    // GPU, so all take the shortest step: one task per wave, one launch
    const bool latmode = nlat > 0 && nlat <= (size_t)std::max(o.dp_lat, 0);
    for (size_t i = 0; i < in.size(); ++i) {
        const DPTask &t = in[i];
        const int lean = dp_lean(t, finite[i]) ? 1 : 0;
        const int npi = dp_npi(t.H);
        const bool np8 = npi < 3 || (t.H <= 255 && o.dp_np8 && o.dp_np8_lean);
        // lean H 128..255 as one 64-lane task per wave, 64..127 as two 32-lane
        // tasks (the 16-lane NP = 4 / 8 kernels need > 256 registers)
        const int wide = npi == 3 && t.H <= 255 ? 0 : (npi == 2 ? 1 : -1);
        int c;
        if (lean && latmode && dpx_fits(t))
            c = CL;
        else if (lean && wide >= 0 && ((o.dp_wide >> wide) & 1))
            c = CW + wide;
        else if (lean && ((psplit >> npi) & 1) && np8 &&
                 !(npi == 0 && DPR_PFIX && (t.P < dpr_pm(0, 0) || t.P > dpr_pm(0, 3) || !(t.P & 1))))
            // NP = 1 stride classes take exactly P = 11, 13, 15, 17 (PFIX
            // kernels); other strides stay in the generic lean class
            c = CP + 4 * npi + dp_pmi(npi, t.P);
        else if (npi < 3)
            c = CR + 2 * npi + lean;
        else if (t.H <= 255 && o.dp_np8)
            c = CR + 6 + (o.dp_np8_lean ? lean : 0);
        else if (t.H <= DP_GEN64_H)
            c = C64;
        else if (t.ncins == 0 && t.ncdel == 0 && o.dp_mc && dpm_slices(t.H) <= DPM_TASK_SLICES && band_below_2g(t))
            c = CWM;   // k_dpm: across CUs, no codon moves (edit_distance's band)
        else
            c = CG;
        cls[c].push_back((uint32_t)i);
    }
    // few non-lean tasks of H <= 127 (the reference's codon DP: one long task
    // per call) run as one latency-bound task per wave (RF_OPT_DP_NL64)
    if (cls[CR].size() + cls[CR + 2].size() + cls[CR + 4].size() <= (size_t)std::max(o.dp_nl64, 0))
        for (int a = 0; a <= 2; ++a) {
            std::vector<uint32_t> keep;
            for (uint32_t i : cls[CR + 2 * a])
                (dpx_fits(in[i]) ? cls[CX] : keep).push_back(i);
            cls[CR + 2 * a].swap(keep);
        }
    // RF_OPT_DP_PFIT: a lean NP >= 2 class launched whole takes the smallest
    // stride class that holds its widest task (the flush stores a fixed
    // dpl_flush_stores(NP, PM) per lane: at PM = 33 c4's NP = 2 class, P <= 19,
    // rewrote 18 % of its bytes)
    if (o.dp_pfit)
        for (int a = 1; a <= 3; ++a) {
            std::vector<uint32_t> &c = cls[CR + 2 * a + 1];
            if (c.empty() || ((psplit >> a) & 1))
                continue;
            int pmax = 0;
            for (uint32_t i : c)
                pmax = std::max(pmax, in[i].P);
            std::vector<uint32_t> &to = cls[CP + 4 * a + dp_pmi(a, pmax)];
            to.insert(to.end(), c.begin(), c.end());
            c.clear();
        }
    // Each class is its own launch (merged launches and other splits measured
    // slower: DESIGN.md §4 "DP launch planner").
    DpPlan P;
    P.tasks.reserve(in.size());
    for (int c = 0; c < NCLS; ++c) {
        if (cls[c].empty())
            continue;
        if (c != CWM)   // longest first; k_dpm's launches take their bands in job order
            std::stable_sort(cls[c].begin(), cls[c].end(), [&](uint32_t x, uint32_t y) { return in[x].klen > in[y].klen; });
        static const DpKernel single[] = {DpKernel::DprWide64, DpKernel::DprWide32, DpKernel::DpxCodon, DpKernel::DpxLean,
                                          DpKernel::Dp64, DpKernel::DpwLds, DpKernel::Dpm};
        DpLaunch L{DpKernel::Dpr, 0, 0, P.tasks.size(), cls[c].size(), -1, 0};
        if (c < CP)
            L = {(c & 1) ? DpKernel::DprLean : DpKernel::Dpr, c >> 1, 0, L.at, L.n, -1, 0};
        else if (c < CW)
            L = {DpKernel::DprLeanPm, (c - CP) >> 2, (c - CP) & 3, L.at, L.n, -1, 0};
        else
            L.k = single[c - CW];
        for (uint32_t i : cls[c]) {
            if (c >= C64)
                L.hmax = std::max(L.hmax, c == CWM ? dpm_slices(in[i].H) : in[i].H);
            P.tasks.push_back(in[i]);
        }
        if (c == CG && L.hmax > DP_LDS_H)
            L.k = DpKernel::DpwGlobal;
        P.launches.push_back(L);
    }
    // The classes are independent (disjoint bands): the smaller ones run on
    // side streams beside the largest.  Latency-bound launches go first, on
    // the main stream (c3's codon DP once waited behind a read class on a
    // hardware queue that side streams share).
    std::vector<DpLaunch> &ls = P.launches;
    std::stable_partition(ls.begin(), ls.end(), [](const DpLaunch &L) { return dp_latency_bound(L.k); });
    size_t big = 0;
    if (!ls.empty() && !dp_latency_bound(ls[0].k))
        for (size_t i = 1; i < ls.size(); ++i)
            if (ls[i].n > ls[big].n)
                big = i;
    if (ls.size() > 1 && o.dp_streams) {
        int nside = 0;
        for (size_t i = 0; i < ls.size(); ++i)
            if (i != big)
                ls[i].stream = nside++ % 3;
    }
    return P;
}

// The wide tier of the pair calls (RF_OPT_PAIR_WIDE; k_ps_wide, k_pa_wide,
// k_pe_wide in rifraf_hip.hip): bands past DP_LDS_H, the four-anti-diagonal
// ring in device memory.  A pair is wide when its band has at least
// pair_wide_from(option) rows: never (0), from DP_LDS_H + 1 (1), or from v
// rows (v >= 2, the tests' knob; DP_LDS_H + 1 at the latest).
constexpr int PW_MAX_H = RF_PAIR_WIDE_MAX_H;   // widest band of the wide tier
constexpr int PW_RING_MB = 256;                // RF_OPT_PAIR_RING_MB's default
inline int pair_wide_from(int opt)
{
    return opt <= 0 ? std::numeric_limits<int>::max() : opt == 1 ? DP_LDS_H + 1 : std::min(opt, DP_LDS_H + 1);
}

// The launch of a set's wide class: npairs pairs (>= 1), the widest of hmax
// rows, in fill mode `count` (the int32 count ring behind the score ring) or
// not, within `budget` bytes of ring.  One workgroup holds a ring of 4 ring_ld
// doubles (and as many int32), ring_ld = hmax + 6; as many workgroups run as
// the budget holds rings, at least one and at most npairs, and loop over the
// pairs.  So the ring takes at most max(budget, one ring) bytes whatever
// npairs is.  Everything in int64.
struct PairWidePlan {
    int64_t nwg, ring_ld, ring_bytes;
};
inline PairWidePlan pair_wide_plan(int64_t npairs, int64_t hmax, bool count, int64_t budget)
{
    PairWidePlan p;
    p.ring_ld = hmax + 6;
    const int64_t one = 4 * p.ring_ld * (count ? 12 : 8);
    p.nwg = std::max<int64_t>(1, std::min(npairs, budget / one));
    p.ring_bytes = p.nwg * one;
    return p;
}

// The tasks of one launch set in their seven width classes, like rf_realign's:
// 0-2: H <= 31, 63, 127 as 16-lane tasks of 1, 2, 4 band-row pairs per lane;
// 3: H <= DP_FAST_H as 64-lane tasks of 2 (k_dpr's wide class: 8 pairs per
// lane in 16 lanes leave one wave per SIMD); 4, 5: the general tier in one
// wave (H <= DP_GEN64_H) or DPW_NT threads; 6: the wide tier, every pair of
// at least wide_from rows whatever class it would else take.
struct PairPlan {
    std::vector<DPTask> cls[7], all;   // all: the classes in order, each longest first
    size_t at[8];                      // class a is all[at[a] .. at[a + 1])
    int hmax[3];                       // widest band of classes 4, 5 and 6
    int wide_from = std::numeric_limits<int>::max();   // pair_wide_from(RF_OPT_PAIR_WIDE); clear() keeps it

    void clear()
    {
        for (auto &c : cls)
            c.clear();
        hmax[0] = hmax[1] = hmax[2] = 0;
    }
    void add(const DPTask &t, bool finite)
    {
        // fast tier: k_dpr's lean condition, bands that live in registers
        const int a = t.H >= wide_from ? 6
                      : dp_lean(t, finite) && t.H <= DP_FAST_H ? dp_npi(t.H) : (t.H <= DP_GEN64_H ? 4 : 5);
        cls[a].push_back(t);
        if (a >= 4)
            hmax[a - 4] = std::max(hmax[a - 4], t.H);
    }
    void finish()
    {
        all.clear();
        for (int a = 0; a < 7; ++a) {
            std::stable_sort(cls[a].begin(), cls[a].end(), [](const DPTask &x, const DPTask &y) { return x.klen > y.klen; });
            at[a] = all.size();
            all.insert(all.end(), cls[a].begin(), cls[a].end());
        }
        at[7] = all.size();
    }
};

// The move trace of a pair (the layout is described in rifraf_hip.hip):
// pa_blocks(klen) blocks of 16 periods, pa_hp(H) 64-bit words each
RF_HD inline int pa_hp(int H) { return (H + 1) & ~1; }
RF_HD inline int pa_blocks(int klen) { return (((klen + 1) >> 1) + 15) >> 4; }

// What one launch set of a pair call produces besides its scores
struct PairWants {
    bool trace;    // the fills write the move trace (rf_pair_scores: none, and nothing below)
    bool walk;     // the walk runs: nmoves and nerrors (with `count`: nerrors goes to the caller)
    bool get_mv;   // the moves go to the caller
    bool emit;     // k_pa_emit runs: aln_len, t2s_len and tolerance, and with
    bool want_txt, want_ix;   // ... these the two texts / the index maps
    bool count = false;   // rf_pair_errors: the fills carry nerrors (k_pe*); no trace, no walk, nothing else above
    bool fix = false;     // k_pa_fix runs: fixed_len, nprops and the tallies, and with
    bool want_fixed = false, want_rec = false;   // ... these the corrected templates / the proposal records
    bool want_mv() const { return get_mv || emit || fix; }   // the walk writes the moves
};

struct PairDims {
    int32_t n, m, bw;
};

// The end of the launch set that starts at list position p0 of npairs: at
// least one pair (a pair above the budget runs alone), then while there are
// fewer than `chunk` pairs and, with a trace, its 64-bit words stay within
// `budget` bytes.  dims(i): the PairDims of list position i.
template <class F>
int64_t pair_set_end(int64_t p0, int64_t npairs, int64_t chunk, bool trace, int64_t budget, F dims)
{
    if (!trace)
        return p0 + std::min(chunk, npairs - p0);
    int64_t cn = 0, words = 0;
    while (p0 + cn < npairs && cn < chunk) {
        const PairDims d = dims(p0 + cn);
        const int H = band_rows(d.n + 1, d.m + 1, d.bw);
        const int64_t w = (int64_t)pa_blocks(H + 2 * d.m) * pa_hp(H);
        if (cn > 0 && (words + w) * 8 > budget)
            break;
        words += w;
        ++cn;
    }
    return p0 + cn;
}

// One launch set: its tasks in launch order and, with a trace, where each
// pair's trace, moves (n + m bytes) and index map (m int32) start.
struct PairSet {
    int64_t cn = 0;
    PairPlan pl;
    std::vector<int64_t> mvoff, ixoff;   // per pair, in set order
    int64_t tr_at = 0, mv_total = 0, ix_total = 0;   // the totals: trace words, move bytes, map entries
    // k_pa_fix's proposal records (pair_set_records): cn + 1 offsets, the last the total
    std::vector<int64_t> proff;
    int64_t pr_total = 0;
};

// The device capacity of each pair's proposal records: cap(i) is what the
// caller gave pair i, and no pair has more proposals than its n + m moves.
template <class F>
void pair_set_records(PairSet &s, F cap)
{
    s.proff.assign((size_t)s.cn + 1, 0);
    for (int64_t i = 0; i < s.cn; ++i) {
        const int64_t slot = (i + 1 < s.cn ? s.mvoff[(size_t)i + 1] : s.mv_total) - s.mvoff[(size_t)i];
        s.proff[(size_t)i + 1] = s.proff[(size_t)i] + std::max<int64_t>(std::min(cap(i), slot), 0);
    }
    s.pr_total = s.proff[(size_t)s.cn];
}

// Fills `s` with the cn pairs of a set.  task(i, &finite): the DPTask of the
// set's pair i (out_idx i; no band, P or pad yet) and whether its tables are
// finite.
template <class F>
void pair_set_fill(PairSet &s, int64_t cn, bool trace, F task)
{
    s.cn = cn;
    s.pl.clear();
    s.mvoff.assign(trace ? (size_t)cn : 0, 0);
    s.ixoff.assign(trace ? (size_t)cn : 0, 0);
    s.tr_at = s.mv_total = s.ix_total = s.pr_total = 0;
    s.proff.clear();
    for (int64_t i = 0; i < cn; ++i) {
        bool finite = false;
        DPTask t = task(i, &finite);
        if (trace) {
            t.band = s.tr_at;             // the pair's trace: 64-bit words from the set's first
            t.P = pa_hp(t.H);             // words per 16-period block
            t.pad = pa_blocks(t.klen);    // blocks
            s.tr_at += (int64_t)t.pad * t.P;
            s.mvoff[(size_t)i] = s.mv_total;
            s.mv_total += t.n + t.m;
            s.ixoff[(size_t)i] = s.ix_total;
            s.ix_total += t.m;
        }
        s.pl.add(t, finite);
    }
    s.pl.finish();
}

// Where a set's downloads land in the pinned zone (bytes from its start,
// each part 16-byte aligned), and the device sizes that go with them.
// Scores, then nmoves and nerrors, then the moves; with k_pa_emit its
// lengths, the two texts (t, then s, mv_total bytes each) and the index maps.
struct PairLanding {
    size_t scores, counts;   // bytes: cn doubles at 0; 2 cn int32 behind them (cn with PairWants::count: nerrors alone)
    size_t mv_at, len_at, txt_at, ix_at;
    size_t lens;             // bytes: 3 cn int32 (aln_len, t2s_len, tolerance)
    size_t total;            // bytes of the zone
    size_t mv_dev, ix_dev;   // device bytes of the moves (and of each text) and of the index maps
    // k_pa_fix: its seven int32 per pair, the corrected templates (mv_total
    // bytes), the records' kind | base << 4 bytes (pr_total) and positions
    size_t fix_at, fixed_at, kb_at, pos_at;
    size_t fixes;            // bytes: 7 cn int32 (fixed_len, nprops, the five tallies)
    size_t kb_dev, pos_dev;  // device bytes of the two record arrays
};

inline PairLanding pair_landing(int64_t cn, int64_t mv_total, int64_t ix_total, const PairWants &w,
                                int64_t pr_total = 0)
{
    const auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    PairLanding L{};
    L.scores = sizeof(double) * (size_t)cn;
    L.total = L.scores;
    if (w.count) {
        L.counts = sizeof(int32_t) * (size_t)cn;
        L.total = L.scores + L.counts;
    }
    if (!w.trace)
        return L;
    L.counts = sizeof(int32_t) * 2 * (size_t)cn;
    L.lens = sizeof(int32_t) * 3 * (size_t)cn;
    L.mv_at = up16(L.scores + L.counts);
    L.len_at = up16(L.mv_at + (w.get_mv ? (size_t)mv_total : 0));
    L.txt_at = up16(L.len_at + (w.emit ? L.lens : 0));
    L.ix_at = up16(L.txt_at + (w.want_txt ? 2 * (size_t)mv_total : 0));
    L.total = L.ix_at + (w.want_ix ? sizeof(int32_t) * (size_t)ix_total : 0);
    L.mv_dev = (size_t)std::max<int64_t>(mv_total, 16);
    L.ix_dev = sizeof(int32_t) * (size_t)std::max<int64_t>(ix_total, 4);
    if (w.fix) {
        L.fixes = sizeof(int32_t) * 7 * (size_t)cn;
        L.fix_at = up16(L.total);
        L.fixed_at = up16(L.fix_at + L.fixes);
        L.kb_at = up16(L.fixed_at + (w.want_fixed ? (size_t)mv_total : 0));
        L.pos_at = up16(L.kb_at + (w.want_rec ? (size_t)pr_total : 0));
        L.total = L.pos_at + (w.want_rec ? sizeof(int32_t) * (size_t)pr_total : 0);
        L.kb_dev = (size_t)std::max<int64_t>(pr_total, 16);
        L.pos_dev = sizeof(int32_t) * (size_t)std::max<int64_t>(pr_total, 4);
    }
    return L;
}

// DPTask.flags' skew and trim bits of a call's RF_SKEW / RF_TRIM
inline int fill_flags(int flags) { return ((flags & RF_SKEW) ? 2 : 0) | ((flags & RF_TRIM) ? 4 : 0); }

#endif
