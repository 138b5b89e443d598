// rifraf_score_plan.h -- host-side launch planning of the dense scorers
// (rf_score, rf_score_dense and the calls built on it): the descriptors the
// kernels read, the choice of scorer and the group layout.  No HIP: a plain
// C++17 compiler takes it alone.  The rules are stated once in DESIGN.md §4
// "Scoring planner".
#ifndef RIFRAF_SCORE_PLAN_H
#define RIFRAF_SCORE_PLAN_H

#include "rifraf_dp_plan.h"

// One batch read of a scoring group.
struct alignas(16) ScoreRead {
    int64_t A, B;     // band offsets (doubles)
    int64_t sb, tab;  // sequence bases / tables
    int32_t n, bw, H, c;
    int32_t vb;       // v_off + bw
    int32_t P, K;
    int32_t flags;    // SR_CODED: row-code records follow the tables (no codon tables)
};
constexpr int SR_CODED = 1;

struct alignas(16) ScoreGroup {
    int64_t tb;         // template bases
    int64_t dense_off;  // totals [m+1][9]
    int64_t split_off;  // per-read partials base (split mode)
    int32_t r0, r1;     // reads [r0, r1) in the ScoreRead list
    int32_t m, pad;
};

struct alignas(8) WorkItem {
    int32_t group, p0;
};

constexpr int SCORE_C = 64;    // positions per work item

// Choice of dense scorer for one launch.
struct ScorePick {
    bool lean = false;
    bool seg = false;   // k_score_segl: wide bands (window too large for LDS), finite tables
    int lds = 0;    // lean: doubles of dynamic LDS; general: doubles per staged band
    int q() const { return 256; }   // k_score_ws chain columns per work item
    // columns per work item of the chosen scorer (k_score: 64)
    int cols() const { return lean ? q() : 64; }
    // the kernel family (RF_SCK_* of the C-ABI)
    int family() const { return lean ? RF_SCK_WS : seg ? RF_SCK_SEG : RF_SCK_GENERAL; }
};

// doubles of LDS a sub-pass over L lanes needs for a read of band height H

RF_HD inline int lean_need(int L, int H, int P)
{
    const int win = ((2 * L + H + 1) * P + 3) & ~1;   // kappa rows + alignment shift, even
    return 2 * win + (L + H + 1) * 6;
}

// k_score stages the kappa rows of a work item through LDS; size the
// per-band buffer for the 90th-percentile window (at most 24 KB per band,
// two bands per single-wave block), larger windows read in place.
inline int score_lds_elems(const std::vector<ScoreRead> &reads)
{
    if (reads.empty())
        return 0;
    std::vector<int> w;
    w.reserve(reads.size());
    for (const auto &R : reads)
        w.push_back((2 * SCORE_C + R.H) * R.P);
    const size_t q = (w.size() * 9) / 10;
    std::nth_element(w.begin(), w.begin() + q, w.end());
    return std::min(w[q], 24 * 1024 / 8);
}

// The options the planner reads (rf_set_option keys, include/rifraf_hip.h)
struct ScoreOpts {
    int score_mode = 0;     // RF_OPT_SCORE_MODE: 0 auto, 1 fused, 2 split
    int score_kernel = 0;   // RF_OPT_SCORE_KERNEL: 0 auto, 1 general, 2 seg, 3 ws (k_score_ws when it fits)
    int lean_lds_kb = 0;    // RF_OPT_LEAN_LDS_KB: k_score_ws LDS budget (0 = default 160 KB)
};

inline ScorePick pick_scorer(const ScoreOpts &o, const std::vector<ScoreRead> &reads, bool all_finite)
{
    ScorePick p;
    const bool force_general = o.score_kernel == 1;
    const bool force_seg = o.score_kernel == 2;
    if (all_finite && !force_general && !force_seg && !reads.empty()) {
        int need1 = 0;
        for (const auto &R : reads)
            need1 = std::max(need1, lean_need(1, R.H, R.P));
        // k_score_ws: 256 chain lanes + 256 loader lanes, one workgroup per CU
        // (measured at c4: 128 chain lanes (two workgroups per CU) +14 %,
        // 320 / 384 chain lanes +50 % scoring time)
        const int lds = std::max((o.lean_lds_kb > 0 ? o.lean_lds_kb : 160) * 1024 / 8, need1);
        // Round 5: a read whose 256-column window exceeds LDS runs in sub-
        // windows over a half (or less) of the chain lanes, the others idle;
        // when such reads hold most of the launch's cells, the segment scorer
        // (LDS independent of H) is faster -- configs[2]'s doubled bands
        // (bw 18, H ~ 37-51): 1.50 -> 0.65 ms per dense pass,
        // profiles/r05q_c3_score_kernel.jsonl
        double wide = 0.0, all = 0.0;
        for (const auto &R : reads) {
            const double w = (double)R.n * R.H;
            all += w;
            if (lean_need(256, R.H, R.P) > lds)
                wide += w;
        }
        if (lds <= 160 * 1024 / 8 && (o.score_kernel == 3 || !(2.0 * wide > all))) {
            p.lean = true;
            p.lds = lds;
            return p;
        }
    }
    // wide bands: the row-segment scorer (same chains, H-independent LDS)
    if (all_finite && !force_general && !reads.empty()) {
        p.seg = true;
        return p;
    }
    p.lds = score_lds_elems(reads);
    return p;
}

// work items: chunks of q consecutive positions of every group
inline std::vector<WorkItem> make_items(const std::vector<ScoreGroup> &groups, int q)
{
    std::vector<WorkItem> items;
    for (int g = 0; g < (int)groups.size(); ++g)
        if (groups[g].r1 > groups[g].r0)
            for (int p0 = 0; p0 <= groups[g].m; p0 += q)
                items.push_back({g, p0});
    return items;
}

// Split mode (one partial per read and k_reduce's ordered fold, instead of the
// in-kernel fold): too few (group, chunk) items to fill the chip, or the
// caller wants per-read scores.  RF_OPT_SCORE_MODE = fused | split overrides
// the choice (tests cover both), but per-read scores exist only in split mode.
inline bool score_split(int64_t nitems, int max_reads, int score_mode, bool per_seq)
{
    if (score_mode == 2 || per_seq)
        return true;
    return score_mode != 1 && nitems < 2048 && max_reads > 1;
}

// Reads per workgroup and grid.y of a scorer launch over nitems items of
// groups of at most max_reads reads.  Fused mode folds every read of a group
// in one workgroup (grid.y 1); the general scorer in split mode takes one read
// per workgroup.  The segment scorer and k_score_ws in split mode take rchunk
// consecutive reads of a group per workgroup: the segment scorer the fewest
// that keep the launch within seg_wgs workgroups (RF_OPT_SEG_WGS, a ceiling),
// k_score_ws the most that still leave score_wgs workgroups
// (RF_OPT_SCORE_WGS, a floor): enough reads per workgroup for the loaders'
// prefetch to overlap the chains, still one workgroup per CU at a time several
// times over.  An option below 1 counts as 1.
struct ScoreChunks {
    int rchunk = 1;
    unsigned grid_y = 1;
};

inline ScoreChunks score_chunks(int family, bool split, int64_t nitems, int64_t max_reads, int score_wgs, int seg_wgs)
{
    ScoreChunks c;
    if (!split)
        return c;
    c.grid_y = (unsigned)max_reads;
    if (family == RF_SCK_SEG) {
        const int64_t tgt = std::max(seg_wgs, 1);
        c.rchunk = (int)std::max<int64_t>(1, (nitems * max_reads + tgt - 1) / tgt);
    } else if (family == RF_SCK_WS) {
        c.rchunk = (int)std::max<int64_t>(1, (nitems * max_reads) / std::max(score_wgs, 1));
    } else {
        return c;
    }
    c.grid_y = (unsigned)((max_reads + c.rchunk - 1) / c.rchunk);
    return c;
}

// What the planner reads of one batch read and of one group
struct ScoreReadIn {
    int64_t A, B, sb, tab;   // bytes: the A and B bands', the sequence's bases' and tables' offsets
    int32_t n, m, bw, H, P;  // the bands' geometry and row stride
    bool finite, coded;      // no -Inf table entry; row codes and no codon tables
};
struct ScoreGroupIn {
    int32_t r0, r1;   // its reads in the ScoreReadIn list
    int32_t m;        // template length and bases offset
    int64_t tb;
};

struct ScorePlan {
    std::vector<ScoreRead> reads;
    std::vector<ScoreGroup> groups;
    std::vector<WorkItem> items;    // pick.cols() columns each
    std::vector<int64_t> gstart;    // dense_off of every group, then dense_total
    ScorePick pick;
    int max_reads = 0;
    int64_t items64 = 0;            // the 64-column items there would be: rf_score's count for score_split
    int64_t dense_total = 0, split_total = 0;
};

// Lays out the groups of one scoring call.  A group without reads gets no
// items, no dense span and no partials when empty_ok, else the call is
// refused (RF_ERR_ARG).
inline int score_plan(const std::vector<ScoreReadIn> &in, const std::vector<ScoreGroupIn> &gin, const ScoreOpts &o,
                      bool empty_ok, ScorePlan &P)
{
    P.groups.assign(gin.size(), ScoreGroup{});   // a plan that is planned again keeps its vectors' memory
    P.gstart.assign(gin.size() + 1, 0);
    P.reads.clear();
    P.reads.reserve(in.size());
    P.items.clear();
    P.max_reads = 0;
    P.items64 = P.dense_total = P.split_total = 0;
    bool all_finite = true;
    for (size_t g = 0; g < gin.size(); ++g) {
        const ScoreGroupIn &I = gin[g];
        if (I.r1 <= I.r0 && !empty_ok)
            return RF_ERR_ARG;
        for (int32_t r = I.r0; r < I.r1; ++r) {
            const ScoreReadIn &s = in[r];
            all_finite = all_finite && s.finite;
            ScoreRead R{};
            R.A = s.A / 8;
            R.B = s.B / 8;
            R.sb = s.sb;
            R.tab = s.tab / 8;
            R.n = s.n;
            R.bw = s.bw;
            R.H = s.H;
            R.c = std::max(s.m - s.n, 0) + s.bw;
            R.vb = std::max(s.n - s.m, 0) + s.bw;
            R.P = s.P;
            R.K = (int32_t)band_K(s.H, s.m);
            R.flags = s.coded ? SR_CODED : 0;
            P.reads.push_back(R);
        }
        ScoreGroup &G = P.groups[g];
        G.r0 = I.r0;
        G.r1 = I.r1;
        G.m = I.m;
        G.tb = I.tb;
        G.dense_off = P.gstart[g] = P.dense_total;
        if (I.r1 > I.r0) {
            const int64_t span = (int64_t)(G.m + 1) * 9;
            P.dense_total += span;
            G.split_off = P.split_total;
            P.split_total += span * (I.r1 - I.r0);
            P.items64 += G.m / 64 + 1;
            P.max_reads = std::max(P.max_reads, I.r1 - I.r0);
        }
    }
    P.gstart[gin.size()] = P.dense_total;
    P.pick = pick_scorer(o, P.reads, all_finite);
    P.items = make_items(P.groups, P.pick.cols());
    return 0;
}

#endif
