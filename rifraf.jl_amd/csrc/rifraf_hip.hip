// rifraf_hip.hip -- MI355X (gfx950) engine for the RIFRAF hot path.
//
// Kernels (all FP64 max-plus, bit-exact with the reference's evaluation
// order; no MFMA: the path has no dense contraction):
//   k_dpr       banded forward / reverse Viterbi fill (forward_moves!,
//               forward!, backward! = reverse forward + flip!), many tasks
//               per launch: 16-, 32- or 64-lane tasks, systolic DPP lanes
//               src/align.jl:50-112 (update), :114-179, :196-202
//   k_dpx       the same fill for a few long tasks (H <= 127), one
//               latency-bound task per wave (the reference's codon DP)
//   k_dpm / k_dp  very wide bands (edit_distance, align.jl:253-260): band
//               slices across the CUs of an XCD / one block per band
//   k_ps / k_ps_gen  score-only forward Viterbi of independent pairs
//               (rf_pair_scores): A[end,end] without a band; register tier
//               (k_dpr's systolic step, no stores) and LDS-ring tier (k_dp's)
//               src/align.jl:155-179
//   k_pa / k_pa_gen / k_pa_walk / k_pa_walk_w  alignments of independent pairs
//               (rf_pair_align): k_ps / k_ps_gen writing a 4-bit move per
//               cell, and a walk over the moves  src/align.jl:114-153,229-245
//   k_pe / k_pe_gen  k_ps / k_ps_gen carrying count_errors of the path into
//               each cell beside its score (rf_pair_errors): no trace, no walk
//               src/align.jl:240-250, src/model.jl:643-672
//   k_ps_wide / k_pa_wide / k_pe_wide  the three for bands past DPW_LDS_H
//               (RF_OPT_PAIR_WIDE): the ring of anti-diagonals in device memory
//   k_pa_emit   gapped texts, index maps and band tolerances from those moves
//               (rf_pair_align_text)  src/align.jl:262-311,322-335
//   k_pa_fix    frameshift correction from those moves (rf_pair_shifts): the
//               single-indel proposals, the corrected template, ambiguity
//               src/model.jl:538-562,1303-1316, src/proposals.jl:41-102
//   k_score_ws / k_score_segl / k_score
//               dense per-position proposal scoring of every batch read,
//               left-folded over the batch in batch order
//               src/model.jl:227-285 (seq_score_deletion, score_nocodon),
//               :385-399 (fold)
//   k_codon     codon-move scoring (reference sequence), one lane per
//               proposal  src/model.jl:287-383
//   k_codon_dense  the same score for every dense slot of a group, one lane
//               per slot, new columns in registers (rf_score_dense_ref)
//   k_reduce    ordered fold of per-read partials (split mode)
//   k_gather    proposal list -> totals (+ reference score, last)
//   k_bt_win    moves recomputed from the stored A band, backtrace +
//               count_errors (+ alignment_proposals' mask)
//               src/align.jl:229-245, src/model.jl:458-497
//   k_tables / k_code_prep / k_aln_* / k_qv  device setup and QV pass
//
// Host side: device arenas (sequences, templates, bands), descriptor
// upload, the C-ABI of include/rifraf_hip.h.

#include <hip/hip_runtime.h>
#include <sched.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <type_traits>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/rifraf_hip.h"
#include "rifraf_dp_plan.h"
#include "rifraf_score_plan.h"
#include "rifraf_seq_upload.h"
#include "rifraf_candidates.h"
#include "rifraf_shift_fix.h"

#define RF_INF (__builtin_inf())

// ---------------------------------------------------------------------
// Band storage on the device: anti-diagonal-major ("kappa-major")
//
//   d     = ii - jj + c    0-based data row of the reference layout
//                          (bandedarrays.jl:109-114), c = h_off + bw
//   kappa = d + 2*jj       anti-diagonal of cell (ii, jj)
//   element (d, jj) lives at band[kappa * P + (d >> 1)],
//   P = ceil(H/2) | 1 (odd row stride: the scorer's lanes read LDS at stride
//   2P; an even P measured 3 % slower scoring with no DP gain in a same-box
//   A/B, despite 4-16 % fewer band bytes), kappa in [0, K), K = H + 2m.
//
// A kappa row holds one anti-diagonal (all band rows d of one parity), so the
// DP fill stores every step as one contiguous run, and a window of columns
// is one contiguous block of rows for the scorer.  The reference's
// column-major `data` is produced on download (rf_download_band).
// ---------------------------------------------------------------------

typedef double dvec2 __attribute__((ext_vector_type(2)));

// Band stores of the DP fill: nontemporal (streamed once, read back by the
// scorer much later; measured ~5 % faster than plain stores on MI355X)
#ifndef RIFRAF_DP_PLAIN_STORES
#define DP_STORE(p, v) __builtin_nontemporal_store((v), (p))
#else
#define DP_STORE(p, v) (*(p) = (v))
#endif

__device__ __forceinline__ size_t bidx(int d, int jj, int P)
{
    return (size_t)(d + 2 * jj) * (size_t)P + (size_t)(d >> 1);
}

// ---------------------------------------------------------------------
// device-side descriptors
// ---------------------------------------------------------------------

// RF_CODES, row_code_off, seq_table_len: rifraf_seq_upload.h

// ScoreRead, ScoreGroup, WorkItem: rifraf_score_plan.h

struct alignas(16) CodonTask {
    int64_t A, B, sb, tab, tb;
    int64_t scratch;   // newcols scratch offset (doubles), 4 * (n+1)
    int32_t n, m, bw, H;
    int32_t ncins, ncdel;
    int32_t kind, pos, base;
    int32_t out_idx;
    int32_t P, pad;
};

struct alignas(16) BTTask {
    int64_t A, sb, tab, tb, out;
    int32_t n, m, bw, H;
    int32_t ncins, ncdel, flags, idx;
    int32_t P, pad;
    int64_t mask;   // k_bt_win with a proposal mask: byte offset of the cluster's (m+1) x 9 mask
};

// error word: first error code wins (atomicCAS)
__device__ __forceinline__ void set_err(int *err, int code)
{
    atomicCAS(err, 0, code);
}

// Order LDS traffic between the lanes of one wave: LDS instructions of a
// wave execute in issue order, so only the compiler has to be fenced.
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Workgroup barrier ordering LDS only: the fences name the local address
// space, so the wait before s_barrier is lgkmcnt(0) -- a wave's global
// stores in flight are not drained (vmcnt counts loads and stores alike).
__device__ __forceinline__ void lds_barrier()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// ---------------------------------------------------------------------
// k_dp: anti-diagonal wavefront DP fill
//
// Cell (ii, jj) depends on kappa-1 (insert: d-1, delete: d+1), kappa-2
// (match: d) and kappa-3 (codon insert d-3, codon delete d+3).  Lane q of a
// W-lane segment owns the pair of band rows {2q, 2q+1}; at anti-diagonal
// kappa it computes d = 2q + (kappa & 1), so every lane produces one cell per
// step (lanes loop over further pairs when H > 2W).  One task per segment,
// 64/W tasks per single-wave workgroup; the last four anti-diagonals live in
// an LDS ring padded with -Inf sentinels.  Out-of-band predecessors read
// -Inf, which never wins the strict '>' (align.jl:43) -- identical to the
// reference's inband() skip.  The candidates are evaluated in the
// reference's order with the same FP64 additions, so A/B are bit-identical
// to the scalar reference.  Each step's cells are one contiguous run of the
// kappa-major band; the reverse pass stores in flip!'ed position
// (bandedarrays.jl:176-198): kappa' = K-1-kappa, d' = H-1-d.
// ---------------------------------------------------------------------

// NT threads per block (64: one wave, 64 / W tasks; W = NT = DPW_NT: one task
// per block of DPW_NT / 64 waves -- the very wide bands of edit_distance,
// H ~ m, whose single task is latency-bound: more lanes per anti-diagonal and
// the ring in LDS (up to DPW_LDS_H) instead of global memory, round 4).
template <int W, bool GRING, int NT = 64>
__global__ void __launch_bounds__(NT)
k_dp(const DPTask *__restrict__ tasks, int ntasks, const uint8_t *__restrict__ bases,
     const double *__restrict__ tabs, double *__restrict__ bands,
     double *__restrict__ out_score, int *__restrict__ err, int ring_ld,
     double *__restrict__ gring)
{
    constexpr int SEGS = NT / W;
    constexpr bool BLOCK_SYNC = GRING || NT > 64;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int seg = threadIdx.x / W;
    const int q = threadIdx.x % W;
    const int tid = blockIdx.x * SEGS + seg;

    DPTask T = {};
    if (tid < ntasks)
        T = tasks[tid];
    double *ring = GRING ? gring + (size_t)blockIdx.x * 4 * ring_ld
                         : smem + (size_t)seg * 4 * ring_ld;
    for (int e = q; e < 4 * ring_ld; e += W)
        ring[e] = -RF_INF;
    int kmax = T.klen;
    for (int off = 32; off >= 1; off >>= 1)
        kmax = max(kmax, __shfl_xor(kmax, off));
    if (BLOCK_SYNC)
        __syncthreads();
    else
        wave_sync();

    const bool rev = T.flags & 1;
    const bool skew = T.flags & 2;
    const bool trim = T.flags & 4;
    const uint8_t *sbase = bases + T.sb;
    const uint8_t *tbase = bases + T.tb;
    const double *tb = tabs + T.tab;
    const double *t_match = tb;
    const double *t_mism = tb + T.n;
    const double *t_ins = tb + 2 * (size_t)T.n;
    const double *t_del = tb + 3 * (size_t)T.n;
    const double *t_cins = tb + 4 * (size_t)T.n + 1;
    const double *t_cdel = t_cins + T.ncins;
    double *band = bands + T.band;

    for (int k = 0; k < kmax; ++k) {
        if (k < T.klen) {
            const int par = k & 1;
            double *r0 = ring + (k & 3) * ring_ld + 3;
            const double *r1 = ring + ((k - 1) & 3) * ring_ld + 3;
            const double *r2 = ring + ((k - 2) & 3) * ring_ld + 3;
            const double *r3 = ring + ((k - 3) & 3) * ring_ld + 3;
            double *row = band + (size_t)(rev ? T.klen - 1 - k : k) * T.P;
            for (int pp = q;; pp += W) {
                const int d = 2 * pp + par;
                if (d >= T.H || d > k)
                    break;
                const int jj = (k - d) >> 1;
                double v = -RF_INF;
                if (jj <= T.m) {
                    const int ii = d + jj - T.c;
                    if (ii >= 0 && ii <= T.n) {
                        if (ii == 0 && jj == 0) {
                            v = 0.0;
                        } else {
                            // align.jl:64-76 score lookups
                            const int sb = ii >= 1 ? sbase[rev ? T.n - ii : ii - 1] : 4;
                            const int tbb = jj >= 1 ? tbase[rev ? T.m - jj : jj - 1] : 4;
                            const int ks = rev ? min(T.n - 1, T.n - ii) : max(ii - 1, 0);
                            const int kd = rev ? T.n - ii : ii;
                            double ms = (sb == tbb) ? t_match[ks] : t_mism[ks];
                            double is = t_ins[ks];
                            const double ds = t_del[kd];
                            if (skew && sb != tbb)
                                ms *= 0.99;
                            if (trim && (jj == 0 || jj == T.m))
                                is = 0.0;
                            // align.jl:77-104, strict '>' in reference order
                            double best = -RF_INF, s;
                            s = r2[d] + ms;
                            if (s > best) best = s;
                            s = r1[d - 1] + is;
                            if (s > best) best = s;
                            s = r1[d + 1] + ds;
                            if (s > best) best = s;
                            if (T.ncins > 0 && ii >= 3) {
                                const int ci = rev ? T.ncins - ii + 2 : ii - 3;
                                s = r3[d - 3] + t_cins[ci];
                                if (s > best) best = s;
                            }
                            if (T.ncdel > 0 && jj >= 3) {
                                s = r3[d + 3] + t_cdel[kd];
                                if (s > best) best = s;
                            }
                            if (best == -RF_INF)
                                set_err(err, 1);  // "new score is invalid"
                            v = best;
                        }
                        if (ii == T.n && jj == T.m && out_score)
                            out_score[T.out_idx] = v;
                    }
                }
                row[(rev ? T.H - 1 - d : d) >> 1] = v;
                r0[d] = v;
            }
        }
        // an LDS ring needs an LDS-only barrier (round 6: __syncthreads also
        // drained the step's band stores); the global ring needs the full one
        if (BLOCK_SYNC && GRING)
            __syncthreads();
        else if (BLOCK_SYNC)
            lds_barrier();
        else
            wave_sync();
    }
}
// widest band whose four-diagonal ring fits the LDS of k_dp<DPW_NT, false, DPW_NT>
constexpr int DPW_LDS_H = 160 * 1024 / 32 - 6;
// lanes of the very-wide-band task (edit_distance's band, H ~ m): each lane
// walks ceil(H/2 / DPW_NT) pairs per anti-diagonal, one dependent table /
// ring round trip each, so the step time falls with the lanes until the
// block barrier dominates (round 4: 256 -> 1024)
#ifndef DPW_NT
#define DPW_NT 1024
#endif

// ---------------------------------------------------------------------
// k_dpr: register-resident variant of k_dp for bands up to H <= 32*NP.
//
// Same recurrence, cell order and FP64 sums as k_dp; the anti-diagonals
// kappa-1..kappa-3 live in registers instead of an LDS ring.  Each task owns
// one 16-lane DPP row (4 tasks per wave); lane q holds band-row pairs
// q*NP .. q*NP+NP-1, and the only cross-lane traffic per step is the pair
// at each block edge, moved with DPP row shifts (v_mov_b32_dpp row_shr /
// row_shl).  Lanes outside the row read the -Inf "bound" value, i.e. an
// out-of-band predecessor, exactly like the ring's sentinels.
// ---------------------------------------------------------------------

template <int CTRL>
__device__ __forceinline__ double dpp_f64(double x)
{
    const long long b = __double_as_longlong(x);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp((int)0xFFF00000, (int)(b >> 32), CTRL, 0xF, 0xF, false);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
#define DPP_FROM_L1 0x111   // row_shr:1 -> value of lane q-1
#define DPP_FROM_L2 0x112   // row_shr:2 -> lane q-2
#define DPP_FROM_R1 0x101   // row_shl:1 -> lane q+1
#define DPP_FROM_R2 0x102   // row_shl:2 -> lane q+2
// Lanes per DP task: 16 (one DPP row, 4 tasks per wave), 32 (two tasks per
// wave) or 64 (the whole wave).  32 and 64 use wave_shr / wave_shl /
// wave_ror / wave_rol, the same moves across DPP rows.  With 32 lanes the
// wave shifts also cross the two tasks: lane 32 (31) would read lane 31's
// (32's) value where it should read its task's edge, so those lanes select
// the edge after the move (EDGE_FIX).  The rotations need no fix: the lanes
// they wrap between hold a task's top pairs, whose diagonals are >= H (the
// host's class bound), i.e. -Inf or masked, exactly as within a DPP row.
template <int LPT>
struct TaskLanes {
    static_assert(LPT == 16 || LPT == 32 || LPT == 64, "tasks are 16, 32 or 64 lanes");
    static constexpr int FROM_L1 = LPT >= 32 ? 0x138 : 0x111;   // lane q-1 (edge lane 0 reads `old`)
    static constexpr int FROM_R1 = LPT >= 32 ? 0x130 : 0x101;   // lane q+1 (edge lane LPT-1 reads `old`)
    static constexpr int ROT_L1 = LPT >= 32 ? 0x13C : 0x121;    // lane (q-1) mod LPT (or mod 64)
    static constexpr int ROT_R1 = LPT >= 32 ? 0x134 : 0x12F;    // lane (q+1) mod LPT (or mod 64)
    static constexpr bool EDGE_FIX = LPT == 32;
};

// Shift an int / double across the 16-lane DPP row (lanes outside the row
// read `bound`).
template <int CTRL>
__device__ __forceinline__ int dpp_i32(int x, int bound)
{
    return __builtin_amdgcn_update_dpp(bound, x, CTRL, 0xF, 0xF, false);
}
template <int CTRL>
__device__ __forceinline__ double dpp_f64_any(double x)
{
    const long long b = __double_as_longlong(x);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xF, 0xF, false);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}

// one {sub A, C, G, T, ins, del} record per read row i (align.jl:60-69)
__device__ __forceinline__ void lean_row(double *rec, int sbse, double mt, double mm, double ins, double del)
{
    double2 *r2 = (double2 *)rec;
    r2[0] = make_double2(sbse == 0 ? mt : mm, sbse == 1 ? mt : mm);
    r2[1] = make_double2(sbse == 2 ? mt : mm, sbse == 3 ? mt : mm);
    r2[2] = make_double2(ins, del);
}

// Per-row inputs of the recurrence (align.jl:64-76, :87-103): the read base
// and the score-table entries row ii uses, in forward or reverse indexing.
struct RowRec {
    int sb;
    double mt, mm, is, ds, ci, cd;
};

__device__ __forceinline__ RowRec load_row(const DPTask &T, bool rev, const uint8_t *sbase,
                                           const double *tb, int ii, bool codon)
{
    RowRec r;
    if (ii < 0 || ii > T.n) {
        r.sb = 4;
        r.mt = r.mm = r.is = r.ds = r.ci = r.cd = -RF_INF;
        return r;
    }
    r.sb = ii >= 1 ? sbase[rev ? T.n - ii : ii - 1] : 4;
    const int ks = rev ? min(T.n - 1, T.n - ii) : max(ii - 1, 0);
    const int kd = rev ? T.n - ii : ii;
    r.mt = tb[ks];
    r.mm = tb[T.n + ks];
    r.is = tb[2 * (size_t)T.n + ks];
    r.ds = tb[3 * (size_t)T.n + kd];
    r.ci = -RF_INF;
    r.cd = -RF_INF;
    if (codon) {
        const double *t_cins = tb + 4 * (size_t)T.n + 1;
        if (T.ncins > 0 && ii >= 3)
            r.ci = t_cins[rev ? T.ncins - ii + 2 : ii - 3];
        if (T.ncdel > 0)
            r.cd = t_cins[T.ncins + kd];
    }
    return r;
}

// A row record as loaded (no select applied yet: selecting right after the
// loads would make the wave wait for them at once) -- RowRec via row_val.
struct RawRow {
    int sb, fl;   // fl: bit 0 row in range, bit 1 base row (ii >= 1), bit 2 codon insert, bit 3 codon delete
    double mt, mm, is, ds, ci, cd;
};
__device__ __forceinline__ RawRow load_row_raw(const DPTask &T, bool rev, const uint8_t *sbase,
                                               const double *tb, int ii, bool codon)
{
    const bool in = ii >= 0 && ii <= T.n;
    const int ic = min(max(ii, 1), T.n);
    const int iz = min(max(ii, 0), T.n);
    // every index >= 0 also for a padding task (T = {}: n = 0), whose loads
    // read the first entries of the arenas and are discarded
    const int ks = max(rev ? min(T.n - 1, T.n - iz) : iz - 1, 0);
    const int kd = rev ? T.n - iz : iz;
    const int ci_i = rev ? T.ncins - iz + 2 : iz - 3;
    const int64_t ci_off = T.ncins > 0 ? 4 * (int64_t)T.n + 1 + min(max(ci_i, 0), T.ncins - 1) : ks;
    const int64_t cd_off = T.ncdel > 0 ? 4 * (int64_t)T.n + 1 + T.ncins + kd : ks;
    RawRow r;
    r.sb = sbase[max(rev ? T.n - ic : ic - 1, 0)];
    r.mt = tb[ks];
    r.mm = tb[T.n + ks];
    r.is = tb[2 * (size_t)T.n + ks];
    r.ds = tb[3 * (size_t)T.n + kd];
    r.ci = tb[ci_off];
    r.cd = tb[cd_off];
    r.fl = (in ? 1 : 0) | ((in && ii >= 1) ? 2 : 0) | ((codon && T.ncins > 0 && ii >= 3 && in) ? 4 : 0) |
           ((codon && T.ncdel > 0 && in) ? 8 : 0);
    return r;
}
__device__ __forceinline__ RowRec row_val(const RawRow &x)
{
    RowRec r;
    const bool in = x.fl & 1;
    r.sb = (x.fl & 2) ? x.sb : 4;
    r.mt = in ? x.mt : -RF_INF;
    r.mm = in ? x.mm : -RF_INF;
    r.is = in ? x.is : -RF_INF;
    r.ds = in ? x.ds : -RF_INF;
    r.ci = (x.fl & 4) ? x.ci : -RF_INF;
    r.cd = (x.fl & 8) ? x.cd : -RF_INF;
    return r;
}

// load_row without branches around its loads (the non-lean kernels): every
// load is issued at a clamped, valid index and the out-of-range values are
// selected afterwards, so each step issues the same loads on every path and
// hipcc's wait for them counts only the memory operations issued after them
// (a load in a branch makes the count path-dependent: vmcnt(0), i.e. a wait
// for every band store as well).  Same values as load_row.
__device__ __forceinline__ RowRec load_row_flat(const DPTask &T, bool rev, const uint8_t *sbase,
                                                const double *tb, int ii, bool codon)
{
    const bool in = ii >= 0 && ii <= T.n;
    const int ic = min(max(ii, 1), T.n);   // a valid read row for the base
    const int iz = min(max(ii, 0), T.n);
    // indices >= 0 for a padding task too (T = {}: n = 0; load_row_raw)
    const int ks = max(rev ? min(T.n - 1, T.n - iz) : iz - 1, 0);
    const int kd = rev ? T.n - iz : iz;
    const int sb = sbase[max(rev ? T.n - ic : ic - 1, 0)];
    const double mt = tb[ks], mm = tb[T.n + ks], is = tb[2 * (size_t)T.n + ks], ds = tb[3 * (size_t)T.n + kd];
    // codon tables (align.jl:87-98): t_cins has n - 2 entries, t_cdel n + 1;
    // a task without them reads the match table instead and discards it
    const double *t_cins = tb + 4 * (size_t)T.n + 1;
    const int ci_i = rev ? T.ncins - iz + 2 : iz - 3;
    const bool has_ci = codon && T.ncins > 0 && ii >= 3 && in;
    const bool has_cd = codon && T.ncdel > 0 && in;
    // one load each at a selected offset (no branch): a task without the
    // table reads its own match entry instead, never past its region
    const int64_t ci_off = T.ncins > 0 ? 4 * (int64_t)T.n + 1 + min(max(ci_i, 0), T.ncins - 1) : ks;
    const int64_t cd_off = T.ncdel > 0 ? 4 * (int64_t)T.n + 1 + T.ncins + kd : ks;
    const double ci = tb[ci_off], cd = tb[cd_off];
    (void)t_cins;
    RowRec r;
    r.sb = (in && ii >= 1) ? sb : 4;
    r.mt = in ? mt : -RF_INF;
    r.mm = in ? mm : -RF_INF;
    r.is = in ? is : -RF_INF;
    r.ds = in ? ds : -RF_INF;
    r.ci = has_ci ? ci : -RF_INF;
    r.cd = has_cd ? cd : -RF_INF;
    return r;
}

__device__ __forceinline__ int load_col(const DPTask &T, bool rev, const uint8_t *tbase, int jj)
{
    return (jj >= 1 && jj <= T.m) ? tbase[rev ? T.m - jj : jj - 1] : 4;
}
// load_col with its load issued unconditionally (load_row_flat)
__device__ __forceinline__ int load_col_flat(const DPTask &T, bool rev, const uint8_t *tbase, int jj)
{
    const int jc = min(max(jj, 1), max(T.m, 1));
    const int b = tbase[rev ? max(T.m - jc, 0) : jc - 1];
    return (jj >= 1 && jj <= T.m) ? b : 4;
}

// Row record of the lane above (row_shl:1 / wave_shl:1); lane LPT-1 receives `edge`.
template <int LPT = 16>
__device__ __forceinline__ RowRec row_from_above(const RowRec &x, const RowRec &edge, bool codon)
{
    constexpr int C = TaskLanes<LPT>::FROM_R1;
    RowRec r;
    r.sb = __builtin_amdgcn_update_dpp(edge.sb, x.sb, C, 0xF, 0xF, false);
    auto sh = [](double v, double e) {
        constexpr int C = TaskLanes<LPT>::FROM_R1;
        const long long b = __double_as_longlong(v), eb = __double_as_longlong(e);
        const int lo = __builtin_amdgcn_update_dpp((int)eb, (int)b, C, 0xF, 0xF, false);
        const int hi = __builtin_amdgcn_update_dpp((int)(eb >> 32), (int)(b >> 32), C, 0xF, 0xF, false);
        return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
    };
    r.mt = sh(x.mt, edge.mt);
    r.mm = sh(x.mm, edge.mm);
    r.is = sh(x.is, edge.is);
    r.ds = sh(x.ds, edge.ds);
    if (TaskLanes<LPT>::EDGE_FIX && (threadIdx.x & (LPT - 1)) == LPT - 1) {
        r.sb = edge.sb;
        r.mt = edge.mt;
        r.mm = edge.mm;
        r.is = edge.is;
        r.ds = edge.ds;
    }
    if (codon) {
        r.ci = sh(x.ci, edge.ci);
        r.cd = sh(x.cd, edge.cd);
    } else {
        r.ci = r.cd = -RF_INF;
    }
    return r;
}

// ---------------------------------------------------------------------
// k_dpr: register-resident, systolic variant of k_dp for H <= 32*NP.
//
// Same recurrence and cell values as k_dp.  Each task owns one 16-lane DPP
// row (4 tasks per wave); lane q holds band-row pairs q*NP .. q*NP+NP-1.
// With pp = q*NP + r the cell of pair pp at anti-diagonal kappa is
//   row ii = pp + ceil(kappa/2) - c,   column jj = floor(kappa/2) - pp,
// so at odd steps every pair moves down one read row and at even steps one
// template column.  The anti-diagonals kappa-1..kappa-3, the per-row score
// tables and the template base all move systolically through registers: a
// pair takes the row record of the pair above it and the column base of the
// pair before it (DPP row_shl / row_shr); the DPP "old" operand hands lane 15
// its prefetched row and lane 0 its new column.  Out-of-row DPP sources read
// -Inf, i.e. an out-of-band predecessor, exactly like the ring's sentinels.
// The loop is unrolled over (even, odd) anti-diagonals so the parity is
// static.  The cell value of the reference's strict-'>' candidate chain
// (align.jl:43, :77-104) is the maximum of the candidates, and FP64 max of
// the same sums is exact (no NaN, no signed zero among candidates), so
// fmax yields bit-identical cells; the move is recomputed in k_bt_win
// with the strict order.
// ---------------------------------------------------------------------

// FLAT (the non-lean kernels): no branch around a store -- a cell outside
// the band goes to the sink -- the final cell's score is kept in a register
// (`fval` / `fset`, stored once after the loop) and the error flag is
// collected in `eflag` and raised once after the loop, so every step issues
// the same memory operations on every path (load_row_flat).
template <int NP, int PAR, int LPT = 16, bool FLAT = false>
__device__ __forceinline__ void dpr_step(const DPTask &T, int q, int k, bool codon, bool rev,
                                         bool skew, bool trim, double (&v1)[NP], double (&v2)[NP],
                                         double (&v3)[NP], const RowRec (&row)[NP],
                                         const int (&col)[NP], double *__restrict__ band,
                                         double *__restrict__ out_score, int *__restrict__ err,
                                         double *__restrict__ sink = nullptr, int *eflag = nullptr,
                                         double *fval = nullptr, int *fset = nullptr)
{
    // block-edge neighbours at kappa-1 (every lane shifts: uniform control flow)
    double E1;
    if (PAR == 0)
        E1 = dpp_f64<TaskLanes<LPT>::FROM_L1>(v1[NP - 1]);   // (d-1) of pair 0 = lane q-1's last pair
    else
        E1 = dpp_f64<TaskLanes<LPT>::FROM_R1>(v1[0]);        // (d+1) of the last pair = lane q+1's pair 0
    double L3a = -RF_INF, L3b = -RF_INF, R3a = -RF_INF, R3b = -RF_INF;
    // (32- and 64-lane tasks are lean: no codon moves; few long non-lean
    // tasks run in k_dpx, the rest as 16-lane tasks here)
    if (LPT == 16 && codon) {
        if (NP == 1) {
            L3a = dpp_f64<DPP_FROM_L1>(v3[0]);
            L3b = dpp_f64<DPP_FROM_L2>(v3[0]);
            R3a = dpp_f64<DPP_FROM_R1>(v3[0]);
            R3b = dpp_f64<DPP_FROM_R2>(v3[0]);
        } else {
            L3a = dpp_f64<DPP_FROM_L1>(v3[NP - 1]);
            L3b = dpp_f64<DPP_FROM_L1>(v3[NP > 1 ? NP - 2 : 0]);
            R3a = dpp_f64<DPP_FROM_R1>(v3[0]);
            R3b = dpp_f64<DPP_FROM_R1>(v3[NP > 1 ? 1 : 0]);
        }
    }
    const bool live = k < T.klen;
    double *orow = band + (size_t)(rev ? T.klen - 1 - k : k) * T.P;
    double nv[NP];
#pragma unroll
    for (int r = 0; r < NP; ++r) {
        const int d = 2 * (q * NP + r) + PAR;
        const int jj = (k - d) >> 1;
        const int ii = d + jj - T.c;
        const bool stored = live && d < T.H && d <= k;
        const bool valid = stored && jj <= T.m && ii >= 0 && ii <= T.n;
        const RowRec &R = row[r];
        const int tbb = col[r];
        double ms = (R.sb == tbb) ? R.mt : R.mm;
        double is = R.is;
        if (skew && R.sb != tbb)
            ms *= 0.99;
        if (trim && (jj == 0 || jj == T.m))
            is = 0.0;
        // insert (d-1, kappa-1) and delete (d+1, kappa-1)
        const double x_ins = PAR ? v1[r] : (r > 0 ? v1[r > 0 ? r - 1 : 0] : E1);
        const double x_del = PAR ? (r < NP - 1 ? v1[r < NP - 1 ? r + 1 : 0] : E1) : v1[r];
        double best = fmax(fmax(v2[r] + ms, x_ins + is), x_del + R.ds);
        if (codon) {
            if (ii >= 3) {   // codon insert: d-3 at kappa-3 = pair q*NP + r - 2 + PAR
                const int idx = r - 2 + PAR;
                const double y = idx >= 0 ? v3[idx >= 0 ? idx : 0] : (idx == -1 ? L3a : L3b);
                best = fmax(best, y + R.ci);
            }
            if (jj >= 3) {   // codon delete: d+3 at kappa-3 = pair q*NP + r + 1 + PAR
                const int idx = r + 1 + PAR;
                const double y = idx < NP ? v3[idx < NP ? idx : 0] : (idx == NP ? R3a : R3b);
                best = fmax(best, y + R.cd);
            }
        }
        const bool origin = ii == 0 && jj == 0;
        const double v = valid ? (origin ? 0.0 : best) : -RF_INF;
        if (FLAT) {
            *eflag |= (valid && !origin && best == -RF_INF) ? 1 : 0;   // "new score is invalid"
            const bool fin = valid && ii == T.n && jj == T.m;
            *fval = fin ? v : *fval;
            *fset |= fin ? 1 : 0;
            *(stored ? orow + ((rev ? T.H - 1 - d : d) >> 1) : sink + 2 * q) = v;
        } else {
            if (valid && !origin && best == -RF_INF)
                set_err(err, 1);  // "new score is invalid"
            if (valid && ii == T.n && jj == T.m && out_score)
                out_score[T.out_idx] = v;
            if (stored)
                orow[(rev ? T.H - 1 - d : d) >> 1] = v;
        }
        nv[r] = v;
    }
#pragma unroll
    for (int r = 0; r < NP; ++r) {
        v3[r] = v2[r];
        v2[r] = v1[r];
        v1[r] = nv[r];
    }
}

// Whole-row DPP rotate of an f64 (no "old" operand: every lane has a source).
template <int CTRL>
__device__ __forceinline__ double dpp_rot_f64(double x)
{
    const long long b = __double_as_longlong(x);
    const int lo = __builtin_amdgcn_mov_dpp((int)b, CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_mov_dpp((int)(b >> 32), CTRL, 0xF, 0xF, false);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
#define DPP_ROT_L1 0x121   // row_ror:1  -> lane (q-1) mod 16
#define DPP_ROT_R1 0x12F   // row_ror:15 -> lane (q+1) mod 16

// One anti-diagonal of the lean interior (LEAN kernels, kappa in [klo, khi]):
// no codon / skew / trim, and every cell of an active diagonal is inside the
// matrix, so the per-cell range checks, the origin and A[end,end] cases of
// dpr_step drop out.  Inactive diagonals (d >= H, or no cell in the matrix)
// get lb = -Inf, which keeps them at -Inf exactly like dpr_step's masking
// (x + 0.0 == x for every cell value: no cell is -0.0).  The block-edge
// neighbour comes from a row *rotate*: the lane it wraps from holds diagonal
// 32*NP-1 >= H (host guarantees H <= 32*NP-1), i.e. -Inf.  Lean tasks have
// finite match/mismatch/ins/del tables, so every in-band cell is finite (each
// has an in-band predecessor chain to the origin) and the "new score is
// invalid" check (align.jl:105-107) cannot fire here; the general steps keep it.
// (An XOR swizzle of the lean blocks' LDS band rows, removing the 4-way bank
// conflicts of the NP = 8 cell stores, was bit-exact but slower at c5:
// 30.2 -> 32.0 ms DP-only, profiles/r02_exp_dp_swz.json.)
template <int NP>
__device__ __forceinline__ dvec2 dpl_rd2(const double *R, int u)   // u even
{
    return *(const dvec2 *)(R + u);
}

template <int NP, int PAR, int LPT = 16>
__device__ __forceinline__ void dpl_step(double (&v1)[NP], double (&v2)[NP], const RowRec (&row)[NP],
                                         const int (&col)[NP], const double (&lb)[NP],
                                         const bool (&st)[NP], double *Rb, int u0, int ostep)
{
    const double E1 = PAR == 0 ? dpp_rot_f64<TaskLanes<LPT>::ROT_L1>(v1[NP - 1])
                               : dpp_rot_f64<TaskLanes<LPT>::ROT_R1>(v1[0]);
    double nv[NP];
#pragma unroll
    for (int r = 0; r < NP; ++r) {
        const RowRec &R = row[r];
        const double ms = (R.sb == col[r]) ? R.mt : R.mm;
        const double x_ins = PAR ? v1[r] : (r > 0 ? v1[r > 0 ? r - 1 : 0] : E1);
        const double x_del = PAR ? (r < NP - 1 ? v1[r < NP - 1 ? r + 1 : 0] : E1) : v1[r];
        // (round 3: the mask on the insert / delete inputs instead of the cell,
        // and the exchanged value entering the max last, were no faster)
        nv[r] = fmax(fmax(v2[r] + ms, x_ins + R.is), x_del + R.ds) + lb[r];
        if (st[r])
            Rb[u0 + r * ostep] = nv[r];
    }
#pragma unroll
    for (int r = 0; r < NP; ++r) {
        v2[r] = v1[r];
        v1[r] = nv[r];
    }
}

// Blocked lean interior: per task an LDS slice of DPL_B edge records (the
// row entering lane 15 and the column entering lane 0 per period) and
// 2*DPL_B kappa rows of band output, flushed as one contiguous chunk.
#ifndef DPL_BLOCK
#define DPL_BLOCK 16
#endif
// periods per block (<= 16: one edge record per lane); NP = 2, 4 take 8 and NP = 8
// takes 4 (measured: NP = 2/4 at 16 need 280/430 VGPRs -> one wave per SIMD), so
// that a 4-task workgroup's LDS slices (rows of up to 129 doubles) leave
// several waves per CU
#ifndef DPL_B64
#define DPL_B64 8   // periods per block of the 64-lane tasks
#endif
__host__ __device__ constexpr int dpl_b(int np, int lpt = 16)
{
    return lpt >= 32 ? DPL_B64 : (np >= 8 ? 4 : (np >= 2 ? 8 : DPL_BLOCK));
}
#ifndef DPL_SPREAD
#define DPL_SPREAD 1   // NP = 1 lean flush spread over the next block's periods
#endif
#define DPL_SPREAD_ON(np, lpt) (DPL_SPREAD && (np) == 1 && (lpt) == 16)
#ifndef DPR_WPE1
#define DPR_WPE1 1   // minimum waves per SIMD requested for the NP = 1 kernels
#endif
struct alignas(16) EdgeRec {
    double mt, mm, is, ds;
    int sb, col, pad0, pad1;
};
// carry slots on either side of a task's band-output rows: a flush writes
// whole 128-B lines only and carries the partial line into the next block
constexpr int DPL_CARRY = 16;
__host__ __device__ constexpr int dpl_task_bytes(int np, int pm, int lpt = 16)
{
    return (int)(dpl_b(np, lpt) * sizeof(EdgeRec)) + (2 * dpl_b(np, lpt) * pm + 2 * DPL_CARRY + 8) * 8;
}
__host__ __device__ constexpr int dpl_task_bytes(int np) { return dpl_task_bytes(np, dpl_pmax(np)); }
// 16-B stores per lane of one flush: at most 2*DPL_B*P + DPL_CARRY doubles
__host__ __device__ constexpr int dpl_flush_stores(int np, int pm, int lpt = 16)
{
    return (dpl_b(np, lpt) * pm + DPL_CARRY / 2 + lpt - 1) / lpt;
}
extern __shared__ __attribute__((aligned(16))) char dpl_smem[];

// PM: the largest band row stride P of the launch's tasks (default: the
// class maximum).  The lean flush issues a fixed dpl_flush_stores(NP, PM)
// 16-B stores per lane (a static count, so hipcc's wait for the next edge
// load is vmcnt(FL) rather than vmcnt(0)); lanes past a block's end repeat
// its last pair.  For NP = 1 the host splits the lean class by P (11, 13,
// 15, 17), so a c4 task with P = 11 issues 12 stores per lane per block
// instead of 18.
#ifndef DPR_WPE64
#define DPR_WPE64 2   // minimum waves per SIMD requested for the 64-lane kernels
#endif
// PFIX (DPR_PFIX, rifraf_dp_plan.h): every task of the launch has stride PM
template <int NP, bool LEAN, int PM, int LPT, bool PFIX>
__device__ __forceinline__ void dpr_body(const int blk, const DPTask *__restrict__ tasks, int ntasks,
                                         const uint8_t *__restrict__ bases, const double *__restrict__ tabs,
                                         double *__restrict__ bands, double *__restrict__ out_score,
                                         int *__restrict__ err, double *__restrict__ sink,
                                         const double *__restrict__ lut)
{
    constexpr int DPL_B = dpl_b(NP, LPT);
    const int q = threadIdx.x & (LPT - 1);
    const int tid = blk * (64 / LPT) + threadIdx.x / LPT;
    DPTask T = {};
    if (tid < ntasks)
        T = tasks[tid];
    int kmax = T.klen;
    for (int off = 32; off >= 1; off >>= 1)
        kmax = max(kmax, __shfl_xor(kmax, off));
    kmax = __builtin_amdgcn_readfirstlane(kmax);
    const bool codon = LEAN ? false : __any(T.ncins > 0 || T.ncdel > 0);   // wave-uniform
    const bool rev = T.flags & 1;
    const bool skew = LEAN ? false : (T.flags & 2);
    const bool trim = LEAN ? false : (T.flags & 4);
    const uint8_t *sbase = bases + T.sb;
    const uint8_t *tbase = bases + T.tb;
    const double *tb = tabs + T.tab;
    double *band = bands + T.band;

    double v1[NP], v2[NP], v3[NP];
    RowRec row[NP];
    int col[NP];
#pragma unroll
    for (int r = 0; r < NP; ++r) {
        v1[r] = -RF_INF;
        v2[r] = -RF_INF;
        v3[r] = -RF_INF;
        const int pp = q * NP + r;
        row[r] = load_row(T, rev, sbase, tb, pp - T.c, codon);   // kappa = 0
        col[r] = load_col(T, rev, tbase, -pp);
    }
    const int top = LPT * NP - 1;
    // general steps of the non-lean kernels: branch-free loads and stores
    // (load_row_flat, dpr_step<FLAT>), so hipcc waits for a prefetched
    // load without draining the band stores issued after it
    constexpr bool FLAT = !LEAN;
    auto lrow = [&](int ii, bool cod) {
        return FLAT ? load_row_flat(T, rev, sbase, tb, ii, cod) : load_row(T, rev, sbase, tb, ii, cod);
    };
    auto lcol = [&](int jj) { return FLAT ? load_col_flat(T, rev, tbase, jj) : load_col(T, rev, tbase, jj); };
    int eflag = 0;
    double fval = 0.0;   // FLAT: the final cell's score (the lane that computes it)
    int fset = 0;
    double *gsink = sink + 64 * (threadIdx.x >> 4);   // 32 doubles per 16-lane row of the wave
    if (FLAT) {
        // Non-lean kernels (codon moves, skew / trim, non-finite tables; e.g. the
        // reference's codon DP, often a single long task per launch, whose
        // period is shorter than a load's latency): the edge row entering lane
        // 15 at odd steps and the column base entering lane 0 at even steps are
        // loaded QD periods ahead into QD static slots (the loop is unrolled
        // over QD periods, so no slot is moved between registers), and their
        // selects run at use; stores and loads are branch-free (dpr_step<FLAT>),
        // so every wait counts only the operations issued after its load.
        constexpr int QD = 4;
        RawRow nq[QD];
        int cq[QD];
        bool cv[QD];
#pragma unroll
        for (int j = 0; j < QD; ++j) {
            nq[j] = load_row_raw(T, rev, sbase, tb, top + 1 + j - T.c, codon);   // period j's edge row
            const int jj = 1 + j;                                                // column of period 1 + j
            cq[j] = tbase[rev ? max(T.m - min(max(jj, 1), max(T.m, 1)), 0) : min(max(jj, 1), max(T.m, 1)) - 1];
            cv[j] = jj >= 1 && jj <= T.m;
        }
        for (int k0 = 0; k0 < kmax; k0 += 2 * QD) {
#pragma unroll
            for (int j = 0; j < QD; ++j) {
                const int k = k0 + 2 * j;
                if (k >= kmax)
                    break;
                if (k > 0) {
                    // even step: lane 0 receives column k/2, from slot (k/2 - 1) mod QD
                    const int cs = (j + QD - 1) % QD;   // static after unrolling
                    const int edge = cv[cs] ? cq[cs] : 4;
                    const int jn = k / 2 + QD;
                    const int jc = min(max(jn, 1), max(T.m, 1));
                    cq[cs] = tbase[rev ? max(T.m - jc, 0) : jc - 1];
                    cv[cs] = jn >= 1 && jn <= T.m;
                    int from = __builtin_amdgcn_update_dpp(edge, col[NP - 1], TaskLanes<LPT>::FROM_L1, 0xF, 0xF,
                                                           false);
                    if (TaskLanes<LPT>::EDGE_FIX && q == 0)
                        from = edge;
#pragma unroll
                    for (int r = NP - 1; r > 0; --r)
                        col[r] = col[r - 1];
                    col[0] = from;
                }
                dpr_step<NP, 0, LPT, true>(T, q, k, codon, rev, skew, trim, v1, v2, v3, row, col, band, out_score,
                                           err, gsink, &eflag, &fval, &fset);
                if (k + 1 < kmax) {
                    // odd step: rows advance; lane 15 receives period k/2's row (slot j)
                    const RowRec up = row_from_above<LPT>(row[0], row_val(nq[j]), codon);
#pragma unroll
                    for (int r = 0; r < NP - 1; ++r)
                        row[r] = row[r + 1];
                    row[NP - 1] = up;
                    nq[j] = load_row_raw(T, rev, sbase, tb, top + k / 2 + 1 + QD - T.c, codon);
                    dpr_step<NP, 1, LPT, true>(T, q, k + 1, codon, rev, skew, trim, v1, v2, v3, row, col, band,
                                               out_score, err, gsink, &eflag, &fval, &fset);
                }
            }
        }
        if (eflag)
            set_err(err, 1);  // "new score is invalid"
        if (fset && out_score)
            out_score[T.out_idx] = fval;
        return;
    }
    // lean kernels: the edge row / column of the next period (one ahead)
    constexpr int QD = 1;
    RowRec nq[QD];
    int cq[QD];
    nq[0] = lrow(top + 1 - T.c, codon);   // enters at kappa = 1
    cq[0] = lcol(1);                      // enters at kappa = 2

    // Lean interior [klo, khi]: the kappa range in which every cell of every
    // active diagonal of the wave's four tasks is inside the matrix, minus the
    // origin and the final cell.  Diagonal d holds cells jj in
    // [max(0, c-d), min(m, n+c-d)], i.e. kappa in [d + 2 jlo, d + 2 jhi].
    int klo = INT_MAX, khi = -1;
    double lb[2][NP];
    bool st[2][NP];
    if (LEAN) {
        int lo = 0, hi = INT_MAX;
        bool ok = true;
#pragma unroll
        for (int par = 0; par < 2; ++par)
#pragma unroll
            for (int r = 0; r < NP; ++r) {
                const int d = 2 * (q * NP + r) + par;
                const int jlo = max(0, T.c - d), jhi = min(T.m, T.n + T.c - d);
                const bool a = tid < ntasks && d < T.H && jlo <= jhi;
                st[par][r] = tid < ntasks && d < T.H;
                lb[par][r] = a ? 0.0 : -RF_INF;
                if (a) {
                    lo = max(lo, d + 2 * jlo);
                    hi = min(hi, d + 2 * jhi);
                }
            }
        if (tid < ntasks) {
            lo = max(lo, T.c + 1);
            hi = min(hi, T.klen - 2);
            ok = T.c <= T.m;   // diagonal 0 holds cells: edge rows stay >= 1
        }
        for (int off = 32; off >= 1; off >>= 1) {
            lo = max(lo, __shfl_xor(lo, off));
            hi = min(hi, __shfl_xor(hi, off));
        }
        if (__all(ok)) {
            klo = __builtin_amdgcn_readfirstlane((lo + 1) & ~1);   // wave-uniform: scalar loop
            khi = __builtin_amdgcn_readfirstlane(hi);
        }
    }
    // whole blocks of the interior; the remainder runs as general steps
    const int nblk = (LEAN && khi >= klo) ? (khi - klo + 1) / (2 * DPL_B) : 0;

    for (int k = 0; k < kmax; k += 2) {
        if (LEAN && k == klo && nblk > 0) {
            // ---- blocked lean interior: DPL_B periods (2*DPL_B anti-diagonals)
            // per block, inputs and outputs staged in this task's LDS slice
            const int P = PFIX ? PM : T.P;
            const int t = threadIdx.x / LPT;
            EdgeRec *ein = reinterpret_cast<EdgeRec *>(dpl_smem + t * dpl_task_bytes(NP, PM, LPT));
            // line-aligned flushes: `fl` is the band position (doubles from the
            // band start, which is 256-B aligned) up to which (forward) or down
            // from which (reverse) the interior has been written.  A block's
            // first position g0 is even forward (even kappa x any P) but can be
            // odd in reverse (odd H): `ob` is shifted by g0's parity so that LDS
            // and global 16-B pairs line up.
            const int blk = 2 * DPL_B * P;
            const ptrdiff_t g00 = (ptrdiff_t)(rev ? T.klen - 2 * DPL_B - k : k) * P;
            ptrdiff_t fl = g00 + (rev ? blk : 0);
            // rows region R; slot u of R holds the band value at position
            // g0 + (u - ub) of the block
            double *R = reinterpret_cast<double *>(dpl_smem + t * dpl_task_bytes(NP, PM, LPT) + DPL_B * sizeof(EdgeRec));
            const int ub = DPL_CARRY + (int)(g00 & 1);
            // this lane's LDS slot per parity; a block's 2*DPL_B rows are the
            // contiguous global chunk (reverse: flipped rows)
            const int sl0 = rev ? (T.H - 1 - 2 * q * NP) >> 1 : q * NP;
            const int sl1 = rev ? (T.H - 2 - 2 * q * NP) >> 1 : q * NP;
            const int ostep = rev ? -1 : 1;
            const int top_c = LPT * NP - T.c;
            // Edge records.  A task whose read has row codes (DPTask flag
            // RF_TASK_CODED) reads one 8-B code record per row from HBM and the
            // table values from the context's code dictionary (L2-resident),
            // instead of 4 table doubles per row; the values are the same
            // doubles.  The code record of a block is loaded one block before
            // its dictionary entries, so neither load's wait covers the
            // block's own band stores.
            const bool coded = T.flags & RF_TASK_CODED;
            const uint64_t *codes = (const uint64_t *)(tb + row_code_off(T.n, T.ncins, T.ncdel));
            auto edge_ks = [&](int kb) {   // lane q < DPL_B: the period kb + 2q edge row (clamped: see dpl_step)
                const int kk = kb + 2 * min(q, DPL_B - 1);
                const int ii = max(1, min(top_c + (kk >> 1), T.n));
                return rev ? T.n - ii : ii - 1;
            };
            auto code_load = [&](int kb) -> uint64_t { return coded ? codes[edge_ks(kb)] : 0; };
            auto edge_load = [&](int kb, uint64_t rec) {
                EdgeRec e;
                const int kk = kb + 2 * min(q, DPL_B - 1);
                const int ks = edge_ks(kb);
                const int kd = rev ? ks : ks + 1;
                if (coded) {
                    const double *l3 = lut + 4 * (int)(rec & 0xffff);
                    const dvec2 mt_mm = *(const dvec2 *)l3;
                    e.mt = mt_mm.x;
                    e.mm = mt_mm.y;
                    e.is = l3[2];
                    e.ds = lut[4 * RF_CODES + (int)((rec >> (rev ? 16 : 32)) & 0xffff)];
                    e.sb = (int)(rec >> 48) & 0xff;
                } else {
                    e.sb = sbase[ks];
                    e.mt = tb[ks];
                    e.mm = tb[T.n + ks];
                    e.is = tb[2 * (size_t)T.n + ks];
                    e.ds = tb[3 * (size_t)T.n + kd];
                }
                const int jj = max(1, min(kk >> 1, T.m));
                e.col = tbase[rev ? T.m - jj : jj - 1];
                return e;
            };
            EdgeRec pend = edge_load(k, code_load(k));
            if (q < DPL_B)
                ein[q] = pend;
            pend = edge_load(k + 2 * DPL_B, code_load(k + 2 * DPL_B));
            uint64_t pcode = code_load(k + 4 * DPL_B);
            // spread flush (NP = 1): a block's flush stores are read from LDS
            // into registers at the block end and issued one per period during
            // the next block, so the store stream stays steady instead of one
            // burst per block that stalls the issuing wave behind the memory
            // pipeline.  Before the first block the pending set is the sink.
            constexpr int FL = dpl_flush_stores(NP, PM, LPT);
            constexpr int FLS = DPL_SPREAD_ON(NP, LPT) ? FL : 1;
            dvec2 pv[FLS];
            dvec2 *pg = (dvec2 *)sink;
            int pnu = 0;
            bool preal = false;
#pragma unroll
            for (int j = 0; j < FLS; ++j)
                pv[j] = dvec2{0.0, 0.0};
            if (!DPL_SPREAD_ON(NP, LPT)) {
                // as many stores behind this load as the loop puts behind its
                // own (to the sink), so that hipcc's wait for `pend` is vmcnt(FL)
                // on every path into the loop, not vmcnt(0)
                dvec2 *g = (dvec2 *)sink;
                const dvec2 z = {0.0, 0.0};
#pragma unroll
                for (int j = 0; j < FL; ++j)
                    g[q + LPT * j] = z;
            }
            wave_sync();
            for (int b = 0; b < nblk; ++b) {
                // edge records are LDS broadcasts read one period ahead: a read
                // issued right before its use exposes the full LDS latency on
                // every step (the DP chain has nothing else to issue meanwhile)
                EdgeRec E = ein[0];
#pragma unroll
                for (int p = 0; p < DPL_B; ++p) {
                    EdgeRec En;
                    if (p + 1 < DPL_B)
                        En = ein[p + 1];
                    if (DPL_SPREAD_ON(NP, LPT)) {
#pragma unroll
                        for (int j = p; j < FLS; j += DPL_B) {
                            const int e = preal ? min(q + LPT * j, pnu - 1) : q + LPT * j;
                            DP_STORE(pg + e, pv[j]);
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    {   // even step: column k/2 enters lane 0
                        int from = __builtin_amdgcn_update_dpp(E.col, col[NP - 1], TaskLanes<LPT>::FROM_L1, 0xF, 0xF, false);
                        if (TaskLanes<LPT>::EDGE_FIX && q == 0)
                            from = E.col;
#pragma unroll
                        for (int r = NP - 1; r > 0; --r)
                            col[r] = col[r - 1];
                        col[0] = from;
                    }
                    const int i0 = rev ? 2 * DPL_B - 1 - 2 * p : 2 * p;
                    dpl_step<NP, 0, LPT>(v1, v2, row, col, lb[0], st[0], R, ub + i0 * P + sl0, ostep);
                    {   // odd step: rows advance; lane 15 receives the edge row
                        RowRec e;
                        e.sb = E.sb;
                        e.mt = E.mt;
                        e.mm = E.mm;
                        e.is = E.is;
                        e.ds = E.ds;
                        const RowRec up = row_from_above<LPT>(row[0], e, false);
#pragma unroll
                        for (int r = 0; r < NP - 1; ++r)
                            row[r] = row[r + 1];
                        row[NP - 1] = up;
                    }
                    const int i1 = rev ? 2 * DPL_B - 2 - 2 * p : 2 * p + 1;
                    dpl_step<NP, 1, LPT>(v1, v2, row, col, lb[1], st[1], R, ub + i1 * P + sl1, ostep);
                    if (p + 1 < DPL_B)
                        E = En;
                }
                wave_sync();
                // next block's edges (loaded one block ago) -> LDS (harmless past
                // the last block: ein is not read again)
                if (q < DPL_B)
                    ein[q] = pend;
                // the block after next: issued BEFORE this block's stores.  vmcnt
                // is one in-order counter for loads and stores, so a load issued
                // after the stores could only be waited for by draining them
                // (clamped rows: past the interior it reads valid, unused rows)
                pend = edge_load(k + 4 * DPL_B, pcode);
                pcode = code_load(k + 6 * DPL_B);
                // flush: the block's 2*DPL_B kappa rows are one contiguous run of the
                // band [g0, g0 + blk).  Only whole 128-B lines are written (a partial
                // line would leave L2 as a partial HBM write): the part past the last
                // full line is carried into the next block (LDS slots before /
                // after `ob`); the last block writes everything.  A fixed number of
                // 16-B stores per lane (lanes past the end repeat the last pair;
                // tasks past ntasks write the sink) keeps hipcc's wait for the next
                // edge load at vmcnt(FL) instead of draining these stores.
                {
                    const ptrdiff_t g0 = (ptrdiff_t)(rev ? T.klen - 2 * DPL_B - k : k) * P;
                    const bool last = b + 1 == nblk;
                    ptrdiff_t lo, hi;
                    if (!rev) {
                        lo = fl;
                        hi = last ? g0 + blk : ((g0 + blk) & ~(ptrdiff_t)15);
                        fl = hi;
                    } else {
                        hi = fl;
                        lo = last ? g0 : ((g0 + 15) & ~(ptrdiff_t)15);
                        fl = lo;
                    }
                    // whole 16-B pairs [lo2, hi2); an odd end (reverse, odd g0: only
                    // the first and last blocks) is one 8-B store
                    const ptrdiff_t lo2 = (lo + 1) & ~(ptrdiff_t)1, hi2 = hi & ~(ptrdiff_t)1;
                    const int nu = (int)((hi2 - lo2) >> 1);
                    // padding tasks (T = {}: nu = 0) write slots [0, 16*FL) of
                    // the sink -- never index -1
                    const bool task_real = tid < ntasks;
                    const bool real = task_real && nu > 0;
                    dvec2 *g = real ? (dvec2 *)(band + lo2) : (dvec2 *)sink;
                    const int u2 = ub + (int)(lo2 - g0);   // even
                    if (DPL_SPREAD_ON(NP, LPT)) {
#pragma unroll
                        for (int j = 0; j < FLS; ++j)
                            pv[j] = dpl_rd2<NP>(R, u2 + 2 * (real ? min(q + LPT * j, nu - 1) : 0));
                        pg = g;
                        pnu = nu;
                        preal = real;
                        if (last) {   // nothing follows: write the last block now
#pragma unroll
                            for (int j = 0; j < FLS; ++j) {
                                const int e = real ? min(q + LPT * j, nu - 1) : q + LPT * j;
                                DP_STORE(g + e, pv[j]);
                            }
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < FL; ++j) {
                            const int e = real ? min(q + LPT * j, nu - 1) : q + LPT * j;
                            DP_STORE(g + e, dpl_rd2<NP>(R, u2 + 2 * (real ? e : 0)));
                        }
                    }
                    if (task_real && q == 0 && (lo & 1))
                        band[lo] = R[ub + (int)(lo - g0)];
                    if (task_real && q == 1 && (hi & 1))
                        band[hi - 1] = R[ub + (int)(hi - 1 - g0)];
                    // carry the unwritten partial line (fewer than 16 doubles: one
                    // pass of the task's lanes) next to the next block's rows
                    if (!rev) {
                        const int c = (int)(g0 + blk - fl), src = (int)(fl - g0);
                        if (q < c)
                            R[ub + src - blk + q] = R[ub + src + q];
                    } else {
                        const int c = (int)(fl - g0);
                        if (q < c)
                            R[ub + blk + q] = R[ub + q];
                    }
                }
                wave_sync();
                k += 2 * DPL_B;
            }
            // back to the general steps: the edge row and column they expect
            // (lean kernels only, QD = 1)
            nq[0] = lrow(top + k / 2 + 1 - T.c, false);
            cq[0] = lcol(k / 2);
            if (k >= kmax)
                break;
        }
        if (k > 0) {
            // even step: columns advance; lane 0 receives column k/2
            const int edge = cq[0];
#pragma unroll
            for (int j = 0; j + 1 < QD; ++j)
                cq[j] = cq[j + 1];
            cq[QD - 1] = lcol(k / 2 + QD);
            int from = __builtin_amdgcn_update_dpp(edge, col[NP - 1], TaskLanes<LPT>::FROM_L1, 0xF, 0xF, false);
            if (TaskLanes<LPT>::EDGE_FIX && q == 0)
                from = edge;
#pragma unroll
            for (int r = NP - 1; r > 0; --r)
                col[r] = col[r - 1];
            col[0] = from;
        }
        dpr_step<NP, 0, LPT, FLAT>(T, q, k, codon, rev, skew, trim, v1, v2, v3, row, col, band, out_score, err,
                                   gsink, &eflag, &fval, &fset);
        if (k + 1 < kmax) {
            // odd step: rows advance; lane 15 receives the prefetched row
            const RowRec up = row_from_above<LPT>(row[0], nq[0], codon);
#pragma unroll
            for (int r = 0; r < NP - 1; ++r)
                row[r] = row[r + 1];
            row[NP - 1] = up;
#pragma unroll
            for (int j = 0; j + 1 < QD; ++j)
                nq[j] = nq[j + 1];
            nq[QD - 1] = lrow(top + (k + 2) / 2 + QD - T.c, codon);
            dpr_step<NP, 1, LPT, FLAT>(T, q, k + 1, codon, rev, skew, trim, v1, v2, v3, row, col, band,
                                       out_score, err, gsink, &eflag, &fval, &fset);
        }
    }
    if (FLAT && eflag)
        set_err(err, 1);  // "new score is invalid"
}

template <int NP, bool LEAN, int PM = dpl_pmax(NP), int LPT = 16, bool PFIX = false>
__global__ void __launch_bounds__(64)
__attribute__((amdgpu_waves_per_eu(LPT >= 32 ? DPR_WPE64 : (NP == 1 ? DPR_WPE1 : 1))))
k_dpr(const DPTask *__restrict__ tasks, int ntasks, const uint8_t *__restrict__ bases,
      const double *__restrict__ tabs, double *__restrict__ bands,
      double *__restrict__ out_score, int *__restrict__ err, double *__restrict__ sink,
      const double *__restrict__ lut)
{
    dpr_body<NP, LEAN, PM, LPT, PFIX>(blockIdx.x, tasks, ntasks, bases, tabs, bands, out_score, err, sink, lut);
}

// ---------------------------------------------------------------------
// k_ps / k_ps_gen (rf_pair_scores) and k_pa / k_pa_gen / k_pa_walk
// (rf_pair_align): forward Viterbi of many independent (sequence, template)
// pairs without FP64 bands.
//
// The fill is A[n+1, m+1] of forward! (align.jl:155-179, cell rule :50-112),
// one double out per pair: only the anti-diagonals kappa-1 and kappa-2
// (kappa-3 with codon moves) stay live.  Same candidates and FP64 sums as
// k_dpr / k_dp, so the value is the one rf_realign(RF_FWD) writes to
// out_score, bit for bit.  Each tier is one body (ps_body, ps_gen_body) that
// every entry point runs: k_ps* in mode PS_SCORE, k_pa* in PS_TRACE, k_pe* in
// PS_COUNT (MODE below; TRACE and COUNT name the two that add something).
//
// ps_body<NP, LPT, TRACE> (fast tier): the lean condition of k_dpr -- no
// codon tables, finite tables, no skew / trim -- and H <= 2*LPT*NP - 1 <=
// PS_FAST_H.  Four 16-lane tasks per wave (NP = 1, 2, 4: H <= 31, 63, 127) or
// one 64-lane task (NP = 2: H <= 255); the anti-diagonals, row records and
// template bases move systolically by DPP exactly as in k_dpr (dpr_step /
// dpl_step without their stores).  The lean interior takes its edge records
// (the row entering lane 15, the column entering lane 0) from a PS_B-period
// LDS block that the task's lanes load one block ahead, one record per lane,
// from the row codes + dictionary or the tables; that block (768 B per task)
// is the kernel's only LDS, and with no band stores nothing else waits on
// memory.  Finite tables make every in-band cell finite (dpl_step's note),
// so "new score is invalid" cannot fire in this tier.  The final cell is
// kept in a register (fval / fset) and stored once after the loop.
//
// ps_gen_body<NT, NPP, TRACE> (general tier): everything else up to
// H <= DPW_LDS_H -- codon tables, RF_SKEW, RF_TRIM, -Inf table entries, wide
// bands -- as k_dp's LDS-ring recurrence with the band stores removed, one
// pair per workgroup of NT threads; thread q owns the diagonal pairs q,
// q + NT, ... (NPP of them at most).  A pair with an invalid cell
// (align.jl:105-110) gets NaN; its neighbours are untouched and no error
// word is raised.
//
// What TRACE adds (forward_moves!, align.jl:114-153): each cell's move --
// the first candidate that is strictly greater, in the order match, insert,
// delete, codon insert, codon delete (align.jl:77-104) -- goes into a 4-bit
// trace.  The score stays the fmax value (fast tier) or the strict-> chain
// (general tier) of the same expression, so out[] holds the same bits.
// Trace of one pair: cell (d, jj) has kappa = d + 2 jj and period
// p = kappa >> 1; its move is nibble p & 15 of the 64-bit word
// tr[(p >> 4) * HP + d], HP = H rounded up to even (pa_hp), for
// pa_blocks(klen) blocks of 16 periods.  A lane gathers the 16 periods of a
// diagonal it owns in a register pair and the lanes of a task store the HP
// words of a block as one contiguous run of 16-B vector stores; every word
// of every block is stored, cells outside the DP as 0 (TRACE_NONE).  In the
// fast tier the lean interior then starts at a multiple of 32 anti-diagonals
// (2 without the trace), so one PS_B-period block is one trace word per
// diagonal and words are flushed at block ends only; the border steps flush
// after every 16th period.  In the general tier the loop over a thread's
// diagonal pairs is unrolled, so their open words stay in registers.
//
// What COUNT adds (k_pe*, rf_pair_errors): count_errors (align.jl:240-245) of
// the path into each cell, an int32 beside its score.  The path into a cell
// is the path into the predecessor its move names, so
//   count[cell] = count[predecessor] + cost(move),
// cost = s[i] != t[j] for a match, 1 for an insertion or a deletion, 3 for a
// codon move (what k_pa_walk adds per step), and the final cell's count
// comes out with A[end, end]: no trace, no walk.  The move is chosen as
// TRACE chooses it and the score expressions are unchanged, so out[] holds
// the same bits.  Fast tier: count registers e1 / e2 beside v1 / v2, moved
// by the same DPP shifts; a masked or out-of-matrix diagonal carries some
// count that nothing selects (its score is -Inf).  General tier: an int32
// ring of the same four anti-diagonals behind the score ring, 48 (H + 6) B
// in all, which fits the LDS up to PE_LDS_H (the host sends wider bands
// through k_pa_gen and the walk); a pair with an invalid cell gets -1.
//
// k_pa_walk (backtrace + count_errors, align.jl:229-245): one lane per pair,
// from (n, m) to (0, 0), reading trace nibbles in place (a word serves up to
// 16 consecutive matches: they stay on one diagonal) and the two base strings
// for the mismatch count.  At most n + m steps; TRACE_NONE, an unknown code,
// a cell off the band or a step that would leave the matrix ends the walk
// with nmoves = nerrors = -1.  Moves are written end-aligned in the pair's
// n + m slot like k_bt_win's.  NaN pairs are not walked.
// ---------------------------------------------------------------------
constexpr int PS_B = 16;           // periods per edge-record block of the fast tier (one record per lane)
constexpr int PS_FAST_H = 255;     // widest band of the fast tier (k_ps<2, 64>)
constexpr int PS_GEN64_H = 2040;   // widest band of the one-wave general tier (ring < 64 KB); above: DPW_NT threads
static_assert(DPW_LDS_H == DP_LDS_H && PS_FAST_H == DP_FAST_H && PS_GEN64_H == DP_GEN64_H, "rifraf_dp_plan.h's limits");
constexpr int PS_CHUNK = 65536;    // pairs per launch set of rf_pair_scores (RF_OPT_PAIR_CHUNK's default)
constexpr int PA_TRACE_MB = 1024;  // RF_OPT_PAIR_TRACE_MB's default
// diagonal pairs per thread of the general tier: 2 NT NPP >= pa_hp(widest band of the tier)
constexpr int PA_NPP64 = (PS_GEN64_H + 1 + 127) / 128;
constexpr int PA_NPPW = (DPW_LDS_H + 1 + 2 * DPW_NT - 1) / (2 * DPW_NT);
// The fill modes of ps_body / ps_gen_body: the score alone (k_ps*), with the
// move trace (k_pa*), with the error count carried per cell (k_pe*)
constexpr int PS_SCORE = 0, PS_TRACE = 1, PS_COUNT = 2;
// widest band whose score ring (4 x 8 B) and count ring (4 x 4 B) of H + 6 entries fit the 160 KiB of LDS
constexpr int PE_LDS_H = 160 * 1024 / 48 - 6;
static_assert(PE_LDS_H == DP_COUNT_H && 48 * (PE_LDS_H + 6) <= 160 * 1024 && 48 * (PE_LDS_H + 7) > 160 * 1024,
              "rifraf_dp_plan.h's DP_COUNT_H");
constexpr int PE_NPPW = (PE_LDS_H + 1 + 2 * DPW_NT - 1) / (2 * DPW_NT);
#ifndef PS_COUNT_GRP
#define PS_COUNT_GRP PS_B   // periods unrolled per pass of the lean interior with the count
#endif

// dpr_step without codon moves, skew / trim and stores (borders of the
// matrix).  TRACE: the cell's move (strict '>' in reference order) goes into
// nibble (k >> 1) & 15 of w
template <int NP, int PAR, int LPT, int MODE>
__device__ __forceinline__ void ps_step(const DPTask &T, int q, int k, double (&v1)[NP], double (&v2)[NP],
                                        const RowRec (&row)[NP], const int (&col)[NP], double &fval, int &fset,
                                        uint64_t (&w)[NP], int (&e1)[NP], int (&e2)[NP], int &fcnt)
{
    constexpr bool TRACE = MODE == PS_TRACE, COUNT = MODE == PS_COUNT;
    const double E1 = PAR == 0 ? dpp_f64<TaskLanes<LPT>::FROM_L1>(v1[NP - 1])
                               : dpp_f64<TaskLanes<LPT>::FROM_R1>(v1[0]);
    int C1 = 0;   // COUNT: the count that moves with E1
    if constexpr (COUNT)
        C1 = PAR == 0 ? dpp_i32<TaskLanes<LPT>::FROM_L1>(e1[NP - 1], 0) : dpp_i32<TaskLanes<LPT>::FROM_R1>(e1[0], 0);
    const bool live = k < T.klen;
    double nv[NP];
    int ne[NP];
#pragma unroll
    for (int r = 0; r < NP; ++r) {
        const int d = 2 * (q * NP + r) + PAR;
        const int jj = (k - d) >> 1;
        const int ii = d + jj - T.c;
        const bool valid = live && d < T.H && d <= k && jj <= T.m && ii >= 0 && ii <= T.n;
        const RowRec &R = row[r];
        const double ms = (R.sb == col[r]) ? R.mt : R.mm;
        const double x_ins = PAR ? v1[r] : (r > 0 ? v1[r > 0 ? r - 1 : 0] : E1);
        const double x_del = PAR ? (r < NP - 1 ? v1[r < NP - 1 ? r + 1 : 0] : E1) : v1[r];
        const double cm = v2[r] + ms, ci = x_ins + R.is, cd = x_del + R.ds;
        const double best = fmax(fmax(cm, ci), cd);
        const bool org = ii == 0 && jj == 0;
        const double v = valid ? (org ? 0.0 : best) : -RF_INF;
        if constexpr (TRACE) {
            int mv = 0;
            double b = -RF_INF;
            if (cm > b) { b = cm; mv = 1; }
            if (ci > b) { b = ci; mv = 2; }
            if (cd > b) { mv = 3; }
            mv = (valid && !org) ? mv : 0;
            w[r] |= (uint64_t)mv << (4 * ((k >> 1) & 15));
        }
        const bool fin = valid && ii == T.n && jj == T.m;
        if constexpr (COUNT) {
            // the count of the chosen predecessor plus the move's cost, chosen as TRACE chooses the move
            const int c_ins = PAR ? e1[r] : (r > 0 ? e1[r > 0 ? r - 1 : 0] : C1);
            const int c_del = PAR ? (r < NP - 1 ? e1[r < NP - 1 ? r + 1 : 0] : C1) : e1[r];
            int c = 0;
            double b = -RF_INF;
            if (cm > b) { b = cm; c = e2[r] + (R.sb == col[r] ? 0 : 1); }
            if (ci > b) { b = ci; c = c_ins + 1; }
            if (cd > b) { c = c_del + 1; }
            c = (valid && !org) ? c : 0;
            fcnt = fin ? c : fcnt;
            ne[r] = c;
        }
        fval = fin ? v : fval;
        fset |= fin ? 1 : 0;
        nv[r] = v;
    }
#pragma unroll
    for (int r = 0; r < NP; ++r) {
        v2[r] = v1[r];
        v1[r] = nv[r];
        if constexpr (COUNT) {
            e2[r] = e1[r];
            e1[r] = ne[r];
        }
    }
}

// dpl_step without its LDS stores (the lean interior).  TRACE: the move goes
// into nibble p (a constant once unrolled) of a 4-period accumulator: two
// compares and selects on the candidates; a masked diagonal (-Inf) carries 0.
// COUNT: the same two compares select the predecessor's count plus the move's
// cost; a masked diagonal carries some count, which no cell selects (its score is -Inf)
template <int NP, int PAR, int LPT, int MODE>
__device__ __forceinline__ void ps_lean_step(double (&v1)[NP], double (&v2)[NP], const RowRec (&row)[NP],
                                             const int (&col)[NP], const double (&lb)[NP], uint32_t (&w)[NP],
                                             const int p, int (&e1)[NP], int (&e2)[NP])
{
    constexpr bool TRACE = MODE == PS_TRACE, COUNT = MODE == PS_COUNT;
    const double E1 = PAR == 0 ? dpp_rot_f64<TaskLanes<LPT>::ROT_L1>(v1[NP - 1])
                               : dpp_rot_f64<TaskLanes<LPT>::ROT_R1>(v1[0]);
    int C1 = 0;
    if constexpr (COUNT)
        C1 = PAR == 0 ? __builtin_amdgcn_mov_dpp(e1[NP - 1], TaskLanes<LPT>::ROT_L1, 0xF, 0xF, false)
                      : __builtin_amdgcn_mov_dpp(e1[0], TaskLanes<LPT>::ROT_R1, 0xF, 0xF, false);
    double nv[NP];
    int ne[NP];
#pragma unroll
    for (int r = 0; r < NP; ++r) {
        const RowRec &R = row[r];
        const double ms = (R.sb == col[r]) ? R.mt : R.mm;
        const double x_ins = PAR ? v1[r] : (r > 0 ? v1[r > 0 ? r - 1 : 0] : E1);
        const double x_del = PAR ? (r < NP - 1 ? v1[r < NP - 1 ? r + 1 : 0] : E1) : v1[r];
        const double cm = v2[r] + ms, ci = x_ins + R.is, cd = x_del + R.ds;
        const double t = fmax(cm, ci);
        nv[r] = fmax(t, cd) + lb[r];
        if constexpr (TRACE) {
            int mv = ci > cm ? 2 : 1;
            mv = cd > t ? 3 : mv;
            mv = nv[r] == -RF_INF ? 0 : mv;
            w[r] |= (uint32_t)mv << (4 * p);
        }
        if constexpr (COUNT) {
            const int c_ins = PAR ? e1[r] : (r > 0 ? e1[r > 0 ? r - 1 : 0] : C1);
            const int c_del = PAR ? (r < NP - 1 ? e1[r < NP - 1 ? r + 1 : 0] : C1) : e1[r];
            int c = ci > cm ? c_ins + 1 : e2[r] + (R.sb == col[r] ? 0 : 1);
            ne[r] = cd > t ? c_del + 1 : c;
        }
    }
#pragma unroll
    for (int r = 0; r < NP; ++r) {
        v2[r] = v1[r];
        v1[r] = nv[r];
        if constexpr (COUNT) {
            e2[r] = e1[r];
            e1[r] = ne[r];
        }
    }
}

template <int NP, int LPT, int MODE>
__device__ __forceinline__ void ps_body(const DPTask *__restrict__ tasks, int ntasks,
                                        const uint8_t *__restrict__ bases, const double *__restrict__ tabs,
                                        double *__restrict__ out, const double *__restrict__ lut,
                                        uint64_t *__restrict__ trace, int32_t *__restrict__ cnt)
{
    constexpr bool TRACE = MODE == PS_TRACE, COUNT = MODE == PS_COUNT;
    // 16 lanes per task, or the whole wave (wave_shr / wave_shl moves: no edge fix, TaskLanes)
    static_assert(LPT == 16 || LPT == 64, "fast-tier tasks are 16 or 64 lanes");
    __shared__ EdgeRec s_edge[64 / LPT][PS_B];
    const int q = threadIdx.x & (LPT - 1);
    const int t = threadIdx.x / LPT;
    const int tid = blockIdx.x * (64 / LPT) + t;
    DPTask T = {};   // a padding task: pad (its trace blocks) = 0, nothing stored
    if (tid < ntasks)
        T = tasks[tid];
    int kmax = T.klen;
    for (int off = 32; off >= 1; off >>= 1)
        kmax = max(kmax, __shfl_xor(kmax, off));
    kmax = __builtin_amdgcn_readfirstlane(kmax);
    const uint8_t *sbase = bases + T.sb;
    const uint8_t *tbase = bases + T.tb;
    const double *tb = tabs + T.tab;

    double v1[NP], v2[NP];
    RowRec row[NP];
    int col[NP];
    uint64_t w[2][NP];   // TRACE: the open trace words of diagonals 2 (q NP + r) + par
    int e1[NP], e2[NP];  // COUNT: the error counts of the paths into v1's and v2's cells
#pragma unroll
    for (int r = 0; r < NP; ++r) {
        v1[r] = -RF_INF;
        v2[r] = -RF_INF;
        e1[r] = e2[r] = 0;
        if constexpr (TRACE)
            w[0][r] = w[1][r] = 0;
        const int pp = q * NP + r;
        row[r] = load_row(T, false, sbase, tb, pp - T.c, false);   // kappa = 0
        col[r] = load_col(T, false, tbase, -pp);
    }
    const int top = LPT * NP - 1;
    RowRec nq = load_row(T, false, sbase, tb, top + 1 - T.c, false);   // enters at kappa = 1
    int cq = load_col(T, false, tbase, 1);                             // enters at kappa = 2
    double fval = 0.0;   // the final cell's score (the lane that computes it)
    int fset = 0;
    int fcnt = 0;        // COUNT: and its path's error count
    // TRACE: block b of the task's trace, diagonals 2 (q NP + r), + 1 as one 16-B store
    auto flush = [&](int b) {
        uint64_t *trp = trace + T.band;
#pragma unroll
        for (int r = 0; r < NP; ++r) {
            const int d = 2 * (q * NP + r);
            if (b < T.pad && d < T.P)
                *(ulonglong2 *)(trp + (size_t)b * T.P + d) = make_ulonglong2(w[0][r], w[1][r]);
            w[0][r] = w[1][r] = 0;
        }
    };

    // lean interior [klo, khi] of the wave's tasks (dpr_body); with the trace klo is at a word boundary
    constexpr int KLO_ALIGN = TRACE ? 2 * PS_B : 2;
    int klo = INT_MAX, khi = -1;
    double lb[2][NP];
    {
        int lo = 0, hi = INT_MAX;
        bool ok = true;
#pragma unroll
        for (int par = 0; par < 2; ++par)
#pragma unroll
            for (int r = 0; r < NP; ++r) {
                const int d = 2 * (q * NP + r) + par;
                const int jlo = max(0, T.c - d), jhi = min(T.m, T.n + T.c - d);
                const bool a = tid < ntasks && d < T.H && jlo <= jhi;
                lb[par][r] = a ? 0.0 : -RF_INF;
                if (a) {
                    lo = max(lo, d + 2 * jlo);
                    hi = min(hi, d + 2 * jhi);
                }
            }
        if (tid < ntasks) {
            lo = max(lo, T.c + 1);
            hi = min(hi, T.klen - 2);
            ok = T.c <= T.m;   // diagonal 0 holds cells: edge rows stay >= 1
        }
        for (int off = 32; off >= 1; off >>= 1) {
            lo = max(lo, __shfl_xor(lo, off));
            hi = min(hi, __shfl_xor(hi, off));
        }
        if (__all(ok)) {
            klo = __builtin_amdgcn_readfirstlane((lo + KLO_ALIGN - 1) & ~(KLO_ALIGN - 1));
            khi = __builtin_amdgcn_readfirstlane(hi);
        }
    }
    const int nblk = khi >= klo ? (khi - klo + 1) / (2 * PS_B) : 0;
    int open_blk = -1;   // TRACE: the trace block the border steps have written into, not flushed yet

    for (int k = 0; k < kmax; k += 2) {
        if (k == klo && nblk > 0) {
            // TRACE: (k - 2) & 31 == 30, the border steps flushed their last block
            EdgeRec *ein = s_edge[t];
            const int top_c = LPT * NP - T.c;
            const bool coded = T.flags & RF_TASK_CODED;
            const uint64_t *codes = (const uint64_t *)(tb + row_code_off(T.n, T.ncins, T.ncdel));
            const int ql = min(q, PS_B - 1);
            auto edge_ks = [&](int kb) {   // lane q < PS_B: the edge row of period kb / 2 + q (clamped; masked by lb)
                const int ii = max(1, min(top_c + (kb >> 1) + ql, T.n));
                return ii - 1;
            };
            auto code_load = [&](int kb) -> uint64_t { return coded ? codes[edge_ks(kb)] : 0; };
            auto edge_load = [&](int kb, uint64_t rec) {
                EdgeRec e;
                const int ks = edge_ks(kb);
                if (coded) {
                    const double *l3 = lut + 4 * (int)(rec & 0xffff);
                    const dvec2 mt_mm = *(const dvec2 *)l3;
                    e.mt = mt_mm.x;
                    e.mm = mt_mm.y;
                    e.is = l3[2];
                    e.ds = lut[4 * RF_CODES + (int)((rec >> 32) & 0xffff)];
                    e.sb = (int)(rec >> 48) & 0xff;
                } else {
                    e.sb = sbase[ks];
                    e.mt = tb[ks];
                    e.mm = tb[T.n + ks];
                    e.is = tb[2 * (size_t)T.n + ks];
                    e.ds = tb[3 * (size_t)T.n + ks + 1];
                }
                const int jj = max(1, min((kb >> 1) + ql, T.m));
                e.col = tbase[jj - 1];
                e.pad0 = e.pad1 = 0;
                return e;
            };
            {
                const EdgeRec first = edge_load(k, code_load(k));
                if (q < PS_B)
                    ein[q] = first;
            }
            EdgeRec pend = edge_load(k + 2 * PS_B, code_load(k + 2 * PS_B));
            uint64_t pcode = code_load(k + 4 * PS_B);
            wave_sync();
            // Periods unrolled per pass of the block: all 16 without the trace.  With it 4 (at
            // 16 the scheduler hoists every period's row / column moves and match selects and
            // runs out of registers); their moves gather in 16 bits and join the trace word once.
            // COUNT keeps all 16 (registers: DESIGN.md §4 "Error counts carried through the fill").
            constexpr int GRP = TRACE ? 4 : (COUNT ? PS_COUNT_GRP : PS_B);
            for (int b = 0; b < nblk; ++b) {
                EdgeRec E = ein[0];
#pragma unroll 1
                for (int p0 = 0; p0 < PS_B; p0 += GRP) {
                    uint32_t acc[2][NP];
                    if constexpr (TRACE) {
#pragma unroll
                        for (int r = 0; r < NP; ++r)
                            acc[0][r] = acc[1][r] = 0;
                    }
#pragma unroll
                    for (int j = 0; j < GRP; ++j) {
                        const EdgeRec En = ein[min(p0 + j + 1, PS_B - 1)];   // one period ahead (LDS latency)
                        {   // even step: column k/2 enters lane 0
                            const int from = __builtin_amdgcn_update_dpp(E.col, col[NP - 1], TaskLanes<LPT>::FROM_L1,
                                                                         0xF, 0xF, false);
#pragma unroll
                            for (int r = NP - 1; r > 0; --r)
                                col[r] = col[r - 1];
                            col[0] = from;
                        }
                        ps_lean_step<NP, 0, LPT, MODE>(v1, v2, row, col, lb[0], acc[0], j, e1, e2);
                        {   // odd step: rows advance; lane 15 receives the edge row
                            RowRec e;
                            e.sb = E.sb;
                            e.mt = E.mt;
                            e.mm = E.mm;
                            e.is = E.is;
                            e.ds = E.ds;
                            e.ci = e.cd = -RF_INF;
                            const RowRec up = row_from_above<LPT>(row[0], e, false);
#pragma unroll
                            for (int r = 0; r < NP - 1; ++r)
                                row[r] = row[r + 1];
                            row[NP - 1] = up;
                        }
                        ps_lean_step<NP, 1, LPT, MODE>(v1, v2, row, col, lb[1], acc[1], j, e1, e2);
                        E = En;
                    }
                    if constexpr (TRACE) {
#pragma unroll
                        for (int r = 0; r < NP; ++r) {
                            w[0][r] |= (uint64_t)acc[0][r] << (4 * p0);
                            w[1][r] |= (uint64_t)acc[1][r] << (4 * p0);
                        }
                    }
                }
                if constexpr (TRACE)
                    flush(k >> 5);   // the block's 16 periods are one trace word per diagonal
                wave_sync();
                if (q < PS_B)
                    ein[q] = pend;   // the next block's records, loaded one block ago
                pend = edge_load(k + 4 * PS_B, pcode);
                pcode = code_load(k + 6 * PS_B);
                wave_sync();
                k += 2 * PS_B;
            }
            // back to the general steps: the edge row and column they expect
            nq = load_row(T, false, sbase, tb, top + k / 2 + 1 - T.c, false);
            cq = load_col(T, false, tbase, k / 2);
            if (k >= kmax)
                break;
        }
        if (k > 0) {
            // even step: columns advance; lane 0 receives column k/2
            const int edge = cq;
            cq = load_col(T, false, tbase, k / 2 + 1);
            const int from = __builtin_amdgcn_update_dpp(edge, col[NP - 1], TaskLanes<LPT>::FROM_L1, 0xF, 0xF, false);
#pragma unroll
            for (int r = NP - 1; r > 0; --r)
                col[r] = col[r - 1];
            col[0] = from;
        }
        if constexpr (TRACE)
            open_blk = k >> 5;
        ps_step<NP, 0, LPT, MODE>(T, q, k, v1, v2, row, col, fval, fset, w[0], e1, e2, fcnt);
        if (k + 1 < kmax) {
            // odd step: rows advance; lane 15 receives the prefetched row
            const RowRec up = row_from_above<LPT>(row[0], nq, false);
#pragma unroll
            for (int r = 0; r < NP - 1; ++r)
                row[r] = row[r + 1];
            row[NP - 1] = up;
            nq = load_row(T, false, sbase, tb, top + (k + 2) / 2 + 1 - T.c, false);
            ps_step<NP, 1, LPT, MODE>(T, q, k + 1, v1, v2, row, col, fval, fset, w[1], e1, e2, fcnt);
        }
        if constexpr (TRACE)
            if ((k & 31) == 30) {
                flush(open_blk);
                open_blk = -1;
            }
    }
    if constexpr (TRACE)
        if (open_blk >= 0)
            flush(open_blk);
    if (fset) {
        out[T.out_idx] = fval;
        if constexpr (COUNT)
            cnt[T.out_idx] = fcnt;
    }
}

template <int NP, int LPT = 16>
__global__ void __launch_bounds__(64)
k_ps(const DPTask *__restrict__ tasks, int ntasks, const uint8_t *__restrict__ bases,
     const double *__restrict__ tabs, double *__restrict__ out, const double *__restrict__ lut)
{
    ps_body<NP, LPT, PS_SCORE>(tasks, ntasks, bases, tabs, out, lut, nullptr, nullptr);
}

template <int NP, int LPT = 16>
__global__ void __launch_bounds__(64)
k_pa(const DPTask *__restrict__ tasks, int ntasks, const uint8_t *__restrict__ bases,
     const double *__restrict__ tabs, double *__restrict__ out, const double *__restrict__ lut,
     uint64_t *__restrict__ trace)
{
    ps_body<NP, LPT, PS_TRACE>(tasks, ntasks, bases, tabs, out, lut, trace, nullptr);
}

template <int NP, int LPT = 16>
__global__ void __launch_bounds__(64)
k_pe(const DPTask *__restrict__ tasks, int ntasks, const uint8_t *__restrict__ bases,
     const double *__restrict__ tabs, double *__restrict__ out, const double *__restrict__ lut,
     int32_t *__restrict__ cnt)
{
    ps_body<NP, LPT, PS_COUNT>(tasks, ntasks, bases, tabs, out, lut, nullptr, cnt);
}

template <int NT, int NPP, int MODE>
__device__ __forceinline__ void ps_gen_body(const DPTask *__restrict__ tasks, const uint8_t *__restrict__ bases,
                                            const double *__restrict__ tabs, double *__restrict__ out,
                                            uint64_t *__restrict__ trace, int32_t *__restrict__ cnt, int ring_ld)
{
    constexpr bool TRACE = MODE == PS_TRACE, COUNT = MODE == PS_COUNT;
    extern __shared__ __attribute__((aligned(16))) double ps_ring[];
    const int q = threadIdx.x;
    const DPTask T = tasks[blockIdx.x];
    double *ring = ps_ring;
    int *cring = (int *)(ps_ring + 4 * ring_ld);   // COUNT: the counts of the same four anti-diagonals
    for (int e = q; e < 4 * ring_ld; e += NT) {
        ring[e] = -RF_INF;
        if constexpr (COUNT)
            cring[e] = 0;
    }
    auto sync = [] {
        if (NT > 64)
            lds_barrier();
        else
            wave_sync();
    };
    sync();
    const bool skew = T.flags & 2;
    const bool trim = T.flags & 4;
    const uint8_t *sbase = bases + T.sb;
    const uint8_t *tbase = bases + T.tb;
    const double *tb = tabs + T.tab;
    const double *t_match = tb;
    const double *t_mism = tb + T.n;
    const double *t_ins = tb + 2 * (size_t)T.n;
    const double *t_del = tb + 3 * (size_t)T.n;
    const double *t_cins = tb + 4 * (size_t)T.n + 1;
    const double *t_cdel = t_cins + T.ncins;
    bool bad = false;    // "new score is invalid" in a cell of this lane
    double fval = 0.0;   // the final cell (the lane that computes it)
    bool fset = false;
    int fcnt = 0;        // COUNT: the error count of the final cell's path
    uint64_t w0[NPP], w1[NPP];   // TRACE: open trace words of diagonals 2 (q + u NT), + 1
    if constexpr (TRACE) {
#pragma unroll
        for (int u = 0; u < NPP; ++u)
            w0[u] = w1[u] = 0;
    }
    const int nu = min(NPP, (T.H + 2 * NT - 1) / (2 * NT));   // diagonal pairs per thread in use (uniform)
    // with the trace the loop over them is unrolled, so w0 / w1 stay in registers
    constexpr int UNROLL = TRACE ? NPP : 1;

    for (int k = 0; k < T.klen; ++k) {
        const int par = k & 1;
        double *r0 = ring + (k & 3) * ring_ld + 3;
        const double *r1 = ring + ((k - 1) & 3) * ring_ld + 3;
        const double *r2 = ring + ((k - 2) & 3) * ring_ld + 3;
        const double *r3 = ring + ((k - 3) & 3) * ring_ld + 3;
        int *c0 = cring + (k & 3) * ring_ld + 3;
        const int *c1 = cring + ((k - 1) & 3) * ring_ld + 3;
        const int *c2 = cring + ((k - 2) & 3) * ring_ld + 3;
        const int *c3 = cring + ((k - 3) & 3) * ring_ld + 3;
#pragma unroll UNROLL
        for (int u = 0; u < NPP; ++u) {
            const int d = 2 * (q + u * NT) + par;
            if (u >= nu || d >= T.H || d > k) {
                // d grows with u, so nothing follows: leave the rolled loop; the unrolled one
                // stays straight-line (a jump out of it costs k_pa_gen<64> five times the SGPR spills)
                if constexpr (TRACE)
                    continue;
                else
                    break;
            }
            const int jj = (k - d) >> 1;
            double v = -RF_INF;
            int mv = 0;   // dead without TRACE
            int ce = 0;   // COUNT: the count of the chosen predecessor plus the move's cost
            if (jj <= T.m) {
                const int ii = d + jj - T.c;
                if (ii >= 0 && ii <= T.n) {
                    if (ii == 0 && jj == 0) {
                        v = 0.0;
                    } else {
                        // align.jl:64-76 score lookups
                        const int sb = ii >= 1 ? sbase[ii - 1] : 4;
                        const int tbb = jj >= 1 ? tbase[jj - 1] : 4;
                        const int ks = max(ii - 1, 0);
                        double ms = (sb == tbb) ? t_match[ks] : t_mism[ks];
                        double is = t_ins[ks];
                        const double ds = t_del[ii];
                        if (skew && sb != tbb)
                            ms *= 0.99;
                        if (trim && (jj == 0 || jj == T.m))
                            is = 0.0;
                        // align.jl:77-104, strict '>' in reference order
                        double best = -RF_INF, s;
                        s = r2[d] + ms;
                        if (s > best) { best = s; mv = 1; }
                        s = r1[d - 1] + is;
                        if (s > best) { best = s; mv = 2; }
                        s = r1[d + 1] + ds;
                        if (s > best) { best = s; mv = 3; }
                        if (T.ncins > 0 && ii >= 3) {
                            s = r3[d - 3] + t_cins[ii - 3];
                            if (s > best) { best = s; mv = 4; }
                        }
                        if (T.ncdel > 0 && jj >= 3) {
                            s = r3[d + 3] + t_cdel[ii];
                            if (s > best) { best = s; mv = 5; }
                        }
                        bad = bad || best == -RF_INF;   // "new score is invalid"
                        v = best;
                        if constexpr (COUNT) {
                            // count_errors (align.jl:240-245) of the path into the cell, as k_pa_walk counts it
                            switch (mv) {
                            case 1: ce = c2[d] + (sb != tbb ? 1 : 0); break;
                            case 2: ce = c1[d - 1] + 1; break;
                            case 3: ce = c1[d + 1] + 1; break;
                            case 4: ce = c3[d - 3] + 3; break;
                            case 5: ce = c3[d + 3] + 3; break;
                            default: break;
                            }
                        }
                    }
                    if (ii == T.n && jj == T.m) {
                        fval = v;
                        fset = true;
                        fcnt = ce;
                    }
                }
            }
            r0[d] = v;
            if constexpr (COUNT)
                c0[d] = ce;
            if constexpr (TRACE) {
                const uint64_t nib = (uint64_t)mv << (4 * ((k >> 1) & 15));
                w0[u] |= par ? 0 : nib;
                w1[u] |= par ? nib : 0;
            }
        }
        if constexpr (TRACE)
            if ((k & 31) == 31 || k == T.klen - 1) {
                // 16 periods done (or the last): the block's HP words, 16 B per thread and diagonal pair
                uint64_t *blk = trace + T.band + (size_t)(k >> 5) * T.P;
#pragma unroll
                for (int u = 0; u < NPP; ++u) {
                    const int d = 2 * (q + u * NT);
                    if (d < T.P)
                        *(ulonglong2 *)(blk + d) = make_ulonglong2(w0[u], w1[u]);
                    w0[u] = w1[u] = 0;
                }
            }
        sync();
    }
    // the pair's flag through the ring (no longer read): NaN for a pair the
    // reference raises on
    if (q == 0)
        ring[0] = 0.0;
    sync();
    if (bad)
        ring[0] = 1.0;
    sync();
    if (fset) {
        const bool raised = ring[0] != 0.0;
        out[T.out_idx] = raised ? __builtin_nan("") : fval;
        if constexpr (COUNT)
            cnt[T.out_idx] = raised ? -1 : fcnt;
    }
}

template <int NT>
__global__ void __launch_bounds__(NT)
k_ps_gen(const DPTask *__restrict__ tasks, const uint8_t *__restrict__ bases,
         const double *__restrict__ tabs, double *__restrict__ out, int ring_ld)
{
    ps_gen_body<NT, NT == 64 ? PA_NPP64 : PA_NPPW, PS_SCORE>(tasks, bases, tabs, out, nullptr, nullptr, ring_ld);
}

template <int NT, int NPP>
__global__ void __launch_bounds__(NT)
k_pa_gen(const DPTask *__restrict__ tasks, const uint8_t *__restrict__ bases,
         const double *__restrict__ tabs, double *__restrict__ out, uint64_t *__restrict__ trace, int ring_ld)
{
    ps_gen_body<NT, NPP, PS_TRACE>(tasks, bases, tabs, out, trace, nullptr, ring_ld);
}

template <int NT>
__global__ void __launch_bounds__(NT)
k_pe_gen(const DPTask *__restrict__ tasks, const uint8_t *__restrict__ bases,
         const double *__restrict__ tabs, double *__restrict__ out, int32_t *__restrict__ cnt, int ring_ld)
{
    ps_gen_body<NT, NT == 64 ? PA_NPP64 : PE_NPPW, PS_COUNT>(tasks, bases, tabs, out, nullptr, cnt, ring_ld);
}

// ps_wide_body<MODE> (wide tier, RF_OPT_PAIR_WIDE): ps_gen_body's recurrence
// for bands past DPW_LDS_H -- the same candidates in the same order, the same
// strict '>' and FP64 sums, so the same bits, moves and counts -- with the
// ring of four anti-diagonals in device memory, as k_dp<W, true, NT> keeps
// it: one workgroup of DPW_NT threads per pair, thread q the diagonal pairs
// q, q + DPW_NT, ... in a rolled loop (no bound on H but PW_MAX_H), a full
// __syncthreads() per anti-diagonal (it orders the workgroup's global
// stores).  The launch has nwg workgroups (pair_wide_plan: what the ring
// budget holds) and workgroup b takes the pairs b, b + nwg, ... of the class,
// which is sorted longest first; its ring is 4 ring_ld doubles at
// gring + 4 ring_ld b and, with COUNT, as many int32 behind the nwg score
// rings.  Before each pair the workgroup writes the 4 (H + 6) entries that the
// pair reads -- -Inf and count 0 -- so nothing of the pair before is seen.
// TRACE: a thread owns more diagonals than registers hold open words, so the
// pair's trace is zeroed first (every word of every block is stored, cells
// outside the DP as TRACE_NONE) and each cell ORs its nibble into its word in
// place; a word belongs to one thread.  The pair's "new score is invalid" flag
// is a word of LDS, the kernel's only LDS.
// gfx950 (-Rpass-analysis=kernel-resource-usage): DESIGN.md §4 "Wide tier".
template <int MODE>
__device__ __forceinline__ void ps_wide_body(const DPTask *__restrict__ tasks, int ntasks,
                                             const uint8_t *__restrict__ bases, const double *__restrict__ tabs,
                                             double *__restrict__ out, uint64_t *trace, int32_t *__restrict__ cnt,
                                             double *gring, int ring_ld)
{
    constexpr bool TRACE = MODE == PS_TRACE, COUNT = MODE == PS_COUNT;
    constexpr int NT = DPW_NT;
    __shared__ int raised;
    const int q = threadIdx.x;
    double *ring = gring + (size_t)blockIdx.x * 4 * ring_ld;
    int *cring = (int *)(gring + (size_t)gridDim.x * 4 * ring_ld) + (size_t)blockIdx.x * 4 * ring_ld;
    for (int t = blockIdx.x; t < ntasks; t += gridDim.x) {
        const DPTask T = tasks[t];
        const int ld = T.H + 6;   // <= ring_ld
        for (int e = q; e < 4 * ld; e += NT) {
            ring[e] = -RF_INF;
            if constexpr (COUNT)
                cring[e] = 0;
        }
        // the pair's trace from the thread's first diagonal on (a pointer in vector registers)
        uint64_t *tr = TRACE ? trace + T.band + 2 * q : nullptr;
        if constexpr (TRACE) {
            // fewer than 2^31 words: the host refuses a longer trace (pair_band_fault)
            const unsigned words = (unsigned)T.pad * (unsigned)T.P;
            for (unsigned e = q; e < words; e += NT)
                tr[(int)e - 2 * q] = 0;
        }
        if (q == 0)
            raised = 0;
        __syncthreads();
        const uint8_t *sbase = bases + T.sb;
        const uint8_t *tbase = bases + T.tb;
        const double *tb = tabs + T.tab;
        // the tables by offset from tb and the ring rows by offset from ring / cring:
        // one scalar register each where a pointer takes two
        const size_t nn = (size_t)T.n;
        bool bad = false;    // "new score is invalid" in a cell of this thread
        double fval = 0.0;   // the final cell (the thread that computes it)
        bool fset = false;
        int fcnt = 0;        // COUNT: the error count of the final cell's path

        for (int k = 0; k < T.klen; ++k) {
            const int par = k & 1;
            const int o0 = (k & 3) * ld + 3, o1 = ((k - 1) & 3) * ld + 3;
            const int o2 = ((k - 2) & 3) * ld + 3, o3 = ((k - 3) & 3) * ld + 3;
            for (int pp = q;; pp += NT) {
                const int d = 2 * pp + par;
                if (d >= T.H || d > k)
                    break;
                const int jj = (k - d) >> 1;
                double v = -RF_INF;
                int mv = 0;   // dead in PS_SCORE
                int ce = 0;   // COUNT: the count of the chosen predecessor plus the move's cost
                const int ii = d + jj - T.c;
                if (jj <= T.m && ii >= 0 && ii <= T.n) {
                    if (ii == 0 && jj == 0) {
                        v = 0.0;
                    } else {
                        // align.jl:64-76 score lookups
                        const int sb = ii >= 1 ? sbase[ii - 1] : 4;
                        const int tbb = jj >= 1 ? tbase[jj - 1] : 4;
                        const int ks = max(ii - 1, 0);
                        double ms = tb[(sb == tbb ? 0 : nn) + ks];
                        double is = tb[2 * nn + ks];
                        const double ds = tb[3 * nn + ii];
                        if ((T.flags & 2) && sb != tbb)
                            ms *= 0.99;
                        if ((T.flags & 4) && (jj == 0 || jj == T.m))
                            is = 0.0;
                        // align.jl:77-104, strict '>' in reference order
                        double best = -RF_INF, s;
                        s = ring[o2 + d] + ms;
                        if (s > best) { best = s; mv = 1; }
                        s = ring[o1 + d - 1] + is;
                        if (s > best) { best = s; mv = 2; }
                        s = ring[o1 + d + 1] + ds;
                        if (s > best) { best = s; mv = 3; }
                        if (T.ncins > 0 && ii >= 3) {
                            s = ring[o3 + d - 3] + tb[4 * nn + 1 + (ii - 3)];
                            if (s > best) { best = s; mv = 4; }
                        }
                        if (T.ncdel > 0 && jj >= 3) {
                            s = ring[o3 + d + 3] + tb[4 * nn + 1 + T.ncins + ii];
                            if (s > best) { best = s; mv = 5; }
                        }
                        bad = bad || best == -RF_INF;   // "new score is invalid"
                        v = best;
                        if constexpr (COUNT) {
                            // count_errors (align.jl:240-245) of the path into the cell, as k_pa_walk counts it
                            switch (mv) {
                            case 1: ce = cring[o2 + d] + (sb != tbb ? 1 : 0); break;
                            case 2: ce = cring[o1 + d - 1] + 1; break;
                            case 3: ce = cring[o1 + d + 1] + 1; break;
                            case 4: ce = cring[o3 + d - 3] + 3; break;
                            case 5: ce = cring[o3 + d + 3] + 3; break;
                            default: break;
                            }
                        }
                    }
                    if (ii == T.n && jj == T.m) {
                        fval = v;
                        fset = true;
                        fcnt = ce;
                    }
                }
                ring[o0 + d] = v;
                if constexpr (COUNT)
                    cring[o0 + d] = ce;
                if constexpr (TRACE)
                    if (mv != 0)
                        tr[(k >> 5) * T.P + (d - 2 * q)] |= (uint64_t)mv << (4 * ((k >> 1) & 15));
            }
            __syncthreads();
        }
        // NaN for a pair the reference raises on; the flag is reset before the next pair
        if (bad)
            raised = 1;
        __syncthreads();
        if (fset) {
            const bool nan = raised != 0;
            const int oi = tasks[t].out_idx;
            out[oi] = nan ? __builtin_nan("") : fval;
            if constexpr (COUNT)
                cnt[oi] = nan ? -1 : fcnt;
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(DPW_NT)
k_ps_wide(const DPTask *__restrict__ tasks, int ntasks, const uint8_t *__restrict__ bases,
          const double *__restrict__ tabs, double *__restrict__ out, double *gring, int ring_ld)
{
    ps_wide_body<PS_SCORE>(tasks, ntasks, bases, tabs, out, nullptr, nullptr, gring, ring_ld);
}

__global__ void __launch_bounds__(DPW_NT)
k_pa_wide(const DPTask *__restrict__ tasks, int ntasks, const uint8_t *__restrict__ bases,
          const double *__restrict__ tabs, double *__restrict__ out, uint64_t *trace, double *gring, int ring_ld)
{
    ps_wide_body<PS_TRACE>(tasks, ntasks, bases, tabs, out, trace, nullptr, gring, ring_ld);
}

__global__ void __launch_bounds__(DPW_NT)
k_pe_wide(const DPTask *__restrict__ tasks, int ntasks, const uint8_t *__restrict__ bases,
          const double *__restrict__ tabs, double *__restrict__ out, int32_t *__restrict__ cnt, double *gring,
          int ring_ld)
{
    ps_wide_body<PS_COUNT>(tasks, ntasks, bases, tabs, out, nullptr, cnt, gring, ring_ld);
}

__global__ void __launch_bounds__(64)
k_pa_walk(const DPTask *__restrict__ tasks, int ntasks, const uint8_t *__restrict__ bases,
          const double *__restrict__ scores, const uint64_t *__restrict__ trace, int8_t *__restrict__ moves,
          const int64_t *__restrict__ moves_off, int32_t *__restrict__ nmoves, int32_t *__restrict__ nerr)
{
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= ntasks)
        return;
    const DPTask T = tasks[t];
    const int n = T.n, m = T.m, H = T.H, HP = T.P, c = T.c, nb = T.pad;
    const uint8_t *s = bases + T.sb;
    const uint8_t *tt = bases + T.tb;
    const uint64_t *tr = trace + T.band;
    int8_t *o = moves ? moves + moves_off[T.out_idx] : nullptr;
    int ii = n, jj = m, cnt = 0, errs = 0;
    bool ok = !(scores[T.out_idx] != scores[T.out_idx]);   // NaN: the reference raised, no walk
    int key = -1;
    uint64_t word = 0;
    for (int step = 0; ok && step < n + m && (ii > 0 || jj > 0); ++step) {
        const int d = ii - jj + c, kap = ii + jj + c;
        const int p = kap >> 1, b = p >> 4;
        if ((unsigned)d >= (unsigned)H || b >= nb) {
            ok = false;
            break;
        }
        const int kk = b * HP + d;
        if (kk != key) {
            word = tr[kk];
            key = kk;
        }
        const int mv = (int)(word >> (4 * (p & 15))) & 15;
        const int di = (mv == 1 || mv == 2) ? 1 : (mv == 4 ? 3 : 0);
        const int dj = (mv == 1 || mv == 3) ? 1 : (mv == 5 ? 3 : 0);
        if (mv < 1 || mv > 5 || ii < di || jj < dj) {
            ok = false;
            break;
        }
        const bool mis = mv == 1 && s[ii - 1] != tt[jj - 1];
        errs += (mv >= 2 || mis) ? 1 : 0;
        errs += mv >= 4 ? 2 : 0;
        if (o)
            o[n + m - 1 - cnt] = (int8_t)mv;
        ++cnt;
        ii -= di;
        jj -= dj;
    }
    ok = ok && ii == 0 && jj == 0;
    nmoves[T.out_idx] = ok ? cnt : -1;
    nerr[T.out_idx] = ok ? errs : -1;
}

// k_pa_walk with one wave per pair (RF_OPT_PAIR_WALK), for launches of few
// long walks: same inputs, trace format, outputs and termination rules.  The
// walk state (ii, jj, counts) is wave-uniform.  The lanes hold a window of the
// trace: the words of up to 64 diagonals d0 .. d0 + 63 of the current
// 16-period block (one coalesced load, masked at HP: only words the fill
// wrote) and the same diagonals of the block before it, which is loaded while
// the current one is walked and moves up when the walk crosses the block
// edge inside the window.  A step takes the current diagonal's word from its
// lane (readlane).  A run of matches stays on one diagonal and inside one
// word: its length comes from the word's nibbles with one count of leading
// zeros, the run is one step, and its lanes store the move bytes and load
// the two bases each; the comparison is taken one run later, per lane, so no
// step waits for those loads, and the lanes' mismatch counts are summed once
// after the walk.  Every other move is one uniform step.  Each iteration
// takes at least one move, so n + m iterations bound the loop as they bound
// k_pa_walk's.
constexpr int PAW_NW = 4;   // waves (pairs) per workgroup
__global__ void __launch_bounds__(64 * PAW_NW)
k_pa_walk_w(const DPTask *__restrict__ tasks, int ntasks, const uint8_t *__restrict__ bases,
            const double *__restrict__ scores, const uint64_t *__restrict__ trace, int8_t *__restrict__ moves,
            const int64_t *__restrict__ moves_off, int32_t *__restrict__ nmoves, int32_t *__restrict__ nerr)
{
    const int lane = threadIdx.x & 63;
    const int t = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * PAW_NW + (threadIdx.x >> 6)));
    if (t >= ntasks)
        return;
    const DPTask &T = tasks[t];
    const int n = T.n, m = T.m, H = T.H, HP = T.P, c = T.c, nb = T.pad, oi = T.out_idx;
    const uint8_t *s = bases + T.sb;
    const uint8_t *tt = bases + T.tb;
    const uint64_t *tr = trace + T.band;
    int8_t *o = moves ? moves + moves_off[oi] : nullptr;
    int ii = n, jj = m, cnt = 0, errs = 0;
    bool ok = !(scores[oi] != scores[oi]);   // NaN: the reference raised, no walk
    int wb = -2, d0 = 0;            // the window: block wb (and wb - 1), diagonals d0 + lane
    uint64_t wcur = 0, wprev = 0;
    int ps = 0, pt = 0, lerr = 0;   // this lane's bases of the last run, its mismatches so far
    for (int it = 0; ok && it < n + m && (ii > 0 || jj > 0); ++it) {
        const int d = ii - jj + c, kap = ii + jj + c;
        const int p = kap >> 1, b = p >> 4;
        if ((unsigned)d >= (unsigned)H || b >= nb) {
            ok = false;
            break;
        }
        if (b != wb || (unsigned)(d - d0) >= 64u) {
            const bool up = b == wb - 1 && (unsigned)(d - d0) < 64u;
            if (!up)
                d0 = max(d - 32, 0);
            const bool in = d0 + lane < HP;
            wcur = up ? wprev : (in ? tr[(size_t)b * HP + d0 + lane] : 0);
            wprev = (b > 0 && in) ? tr[(size_t)(b - 1) * HP + d0 + lane] : 0;
            wb = b;
        }
        const int sl = __builtin_amdgcn_readfirstlane(d - d0);
        const uint32_t wlo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)wcur, sl);
        const uint32_t whi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(wcur >> 32), sl);
        const uint64_t word = ((uint64_t)whi << 32) | wlo;
        const int q = p & 15;
        const int mv = (int)(word >> (4 * q)) & 15;
        if (mv == 1) {
            // nibbles q, q - 1, ... that are 1: the shifted-in low nibbles are 0 and end the run at nibble 0
            const uint64_t y = (word << (4 * (15 - q))) ^ 0x1111111111111111ull;
            const int run = y ? __builtin_clzll(y) >> 2 : 16;
            const int r = min(run, min(ii, jj));
            if (r == 0) {   // a match that would leave the matrix
                ok = false;
                break;
            }
            lerr += ps != pt ? 1 : 0;
            ps = pt = 0;
            if (lane < r) {
                ps = s[ii - 1 - lane];
                pt = tt[jj - 1 - lane];
                if (o)
                    o[n + m - 1 - cnt - lane] = 1;
            }
            cnt += r;
            ii -= r;
            jj -= r;
        } else {
            const int di = mv == 2 ? 1 : (mv == 4 ? 3 : 0);
            const int dj = mv == 3 ? 1 : (mv == 5 ? 3 : 0);
            if (mv < 2 || mv > 5 || ii < di || jj < dj) {
                ok = false;
                break;
            }
            errs += mv >= 4 ? 3 : 1;
            if (o && lane == 0)
                o[n + m - 1 - cnt] = (int8_t)mv;
            ++cnt;
            ii -= di;
            jj -= dj;
        }
    }
    lerr += ps != pt ? 1 : 0;
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1)
        lerr += __shfl_xor(lerr, w, 64);
    ok = ok && ii == 0 && jj == 0;
    if (lane == 0) {
        nmoves[oi] = ok ? cnt : -1;
        nerr[oi] = ok ? errs + lerr : -1;
    }
}

// k_pa_emit (rf_pair_align_text): what a caller makes of a pair's moves, on
// the moves the walk left in device memory.  One wave per pair; the lanes take
// 64 consecutive moves, in alignment order.  A lane's move gives (di, dj)
// (offset_forward, align.jl:20-23), its width in the text (3 for the codon
// moves, else 1) and whether it advances j; the four go through one inclusive
// wave scan packed in bytes (a chunk sums to at most 3 * 64 per field), on
// top of the running totals of the chunks before.  With i, j after its move a
// lane writes
//   - its 1 or 3 bytes of both gapped texts, "ACGT-" (moves_to_aligned_seqs,
//     align.jl:286-311), from the start of the pair's n + m slot;
//   - i into the template -> sequence map if dj > 0: j only grows, so that is
//     the reference's j > last_j, and a codon deletion pushes once
//     (moves_to_indices, align.jl:322-335);
//   - nothing for band_tolerance (align.jl:262-284), but keeps the minimum
//     distance of its cell (i + 1, j + 1) to the band's row_range where that
//     range is cut by the band and not by the matrix; lane 0 starts from cell
//     (1, 1), the value starts at nrows, and the lanes' minima meet once after
//     the loop.
// Any of the three products may be off (NULL).  lens: aln_len, t2s_len and
// tolerance, ntasks of each; a pair the walk gave up (-1) gets -1 in all three
// and no bytes.
// types.dna_str's letter of a base code: the arenas hold what the caller
// uploaded, 0..3 by the ABI's convention; 4 is the host's gap letter
__device__ __forceinline__ uint8_t pa_char(uint8_t b) { return b < 4 ? (uint8_t)"ACGT"[b] : (uint8_t)'-'; }

__global__ void __launch_bounds__(64 * PAW_NW)
k_pa_emit(const DPTask *__restrict__ tasks, int ntasks, const uint8_t *__restrict__ bases,
          const int8_t *__restrict__ moves, const int64_t *__restrict__ moves_off,
          const int32_t *__restrict__ nmoves, uint8_t *__restrict__ aln_t, uint8_t *__restrict__ aln_s,
          int32_t *__restrict__ t2s, const int64_t *__restrict__ t2s_off, int32_t *__restrict__ lens)
{
    const int lane = threadIdx.x & 63;
    const int t = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * PAW_NW + (threadIdx.x >> 6)));
    if (t >= ntasks)
        return;
    const DPTask &T = tasks[t];
    const int n = T.n, m = T.m, bw = T.bw, oi = T.out_idx;
    const int cnt = nmoves[oi];
    if (cnt < 0) {
        if (lane < 3)
            lens[(size_t)lane * ntasks + oi] = -1;
        return;
    }
    const uint8_t *s = bases + T.sb;
    const uint8_t *tt = bases + T.tb;
    const int64_t slot = moves_off[oi];
    const int8_t *mvs = moves + slot + (n + m - cnt);   // end-aligned by the walk
    uint8_t *at = aln_t ? aln_t + slot : nullptr;
    uint8_t *as = aln_t ? aln_s + slot : nullptr;
    int32_t *ix = t2s ? t2s + t2s_off[oi] : nullptr;
    const int nrows = n + 1, hoff = max(m - n, 0), voff = max(n - m, 0);
    // |i - start| where start > 1, |i - stop| where stop < nrows, else nrows (row_range, bandedarrays.jl:133-137)
    auto edge = [&](int i, int j) {
        const int start = max(1, j - hoff - bw), stop = min(j + voff + bw, nrows);
        const int a = start > 1 ? abs(i - start) : nrows, b = stop < nrows ? abs(i - stop) : nrows;
        return min(a, b);
    };
    int tol = lane == 0 ? edge(1, 1) : nrows;
    int bi = 0, bj = 0, bo = 0, bk = 0;   // i, j, text bytes and map entries of the chunks before
    for (int x0 = 0; x0 < cnt; x0 += 64) {
        const bool on = x0 + lane < cnt;
        const int mv = on ? mvs[x0 + lane] : 0;
        const int di = (mv == 1 || mv == 2) ? 1 : (mv == 4 ? 3 : 0);
        const int dj = (mv == 1 || mv == 3) ? 1 : (mv == 5 ? 3 : 0);
        const int w = mv >= 4 ? 3 : (mv >= 1 ? 1 : 0);
        int sc = di | (dj << 8) | (w << 16) | ((dj > 0 ? 1 : 0) << 24);
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(sc, d, 64);
            sc += lane >= d ? up : 0;
        }
        const int i = bi + (sc & 255), j = bj + ((sc >> 8) & 255);
        const int o = bo + ((sc >> 16) & 255) - w, k = bk + ((sc >> 24) & 255);
        if (on) {
            if (at) {
                if (mv <= 3) {
                    at[o] = mv == 2 ? '-' : pa_char(tt[j - 1]);
                    as[o] = mv == 3 ? '-' : pa_char(s[i - 1]);
                } else {
#pragma unroll
                    for (int u = 0; u < 3; ++u) {
                        at[o + u] = mv == 4 ? '-' : pa_char(tt[j - 3 + u]);
                        as[o + u] = mv == 5 ? '-' : pa_char(s[i - 3 + u]);
                    }
                }
            }
            if (ix && dj > 0)
                ix[k - 1] = i;
            tol = min(tol, edge(i + 1, j + 1));
        }
        const int tot = __builtin_amdgcn_readlane(sc, 63);
        bi += tot & 255;
        bj += (tot >> 8) & 255;
        bo += (tot >> 16) & 255;
        bk += (tot >> 24) & 255;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
        tol = min(tol, __shfl_xor(tol, d, 64));
    if (lane == 0) {
        lens[oi] = bo;
        lens[(size_t)ntasks + oi] = bk;
        lens[2 * (size_t)ntasks + oi] = tol;
    }
}

// k_pa_fix (rf_pair_shifts): correct_shifts (model.jl:1303-1316) from a
// pair's moves, on the moves the walk left in device memory.  The sequence s
// (rows) is the reference, the template t the consensus.  Shape and scan are
// k_pa_emit's: one wave per pair, the lanes take 64 consecutive moves in
// alignment order, and (di, dj), the bases the move adds to the corrected
// template and whether it proposes go through one inclusive wave scan packed
// in bytes (a chunk sums to at most 3 * 64 per field) on top of the running
// totals.  The per-move rules are rifraf_shift_fix.h's, which the host
// restatement (rf_host_shift_fix) shares.  With i, j after its move:
//   - single_indel_proposals (model.jl:538-562): an insert (2) is
//     Insertion(j, s[i - 1]), a delete (3) is Deletion(j), in move order; the
//     other moves propose nothing.  The first `capacity` records of a pair are
//     stored, nprops is the true count.
//   - apply_proposals(t, proposals) (proposals.jl:80-102) is the
//     concatenation, per move, of: match t[j - 1]; insert s[i - 1]; delete and
//     codon insert nothing; codon delete t[j - 3 .. j - 1].  Why: j never
//     decreases along the moves and Deletion(p) is made by the move that
//     brings j to p, Insertion(p, b) by a later move at j = p, so move order
//     is already the order apply_proposals sorts to (by pos, deletions first).
//     It copies t[next .. pos - 1], then a deletion skips t[pos]; an insertion
//     at pos > 0 without a deletion there emits t[pos], b; after a deletion at
//     pos, or at pos = 0, it emits b alone; next = pos + 1, and the tail
//     follows.  So every template base is emitted exactly once, in order,
//     unless a Deletion names it, and b comes right behind the bases up to
//     t[pos].  Per move that is the same text: each template position belongs
//     to exactly one j-advancing move (a match or a codon delete emits it, a
//     delete drops it), and an insert emits s[i - 1] when the bases up to t[j]
//     are out (or dropped) -- before the first base at j = 0, after t[j] if it
//     was kept, in its place if the move before deleted it.  A move adds at
//     most di + dj bases, so the length is at most n + m.
//   - are_ambiguous (proposals.jl:41-56): the deletions' positions are
//     distinct (each takes a new j), so the set is ambiguous exactly when two
//     inserts share a j, i.e. an insert whose previous insert has the same j
//     (no move between them advanced j; a codon insert does not).  A lane
//     finds the insert before it by a ballot, or in the j of the last insert
//     of the chunks before (last_ins).  fixed_len is then -2; the proposals
//     and tallies are reported all the same.
// out: fixed_len, nprops and the counts of the move codes 1..5, ntasks of
// each; a pair the walk gave up (-1) gets -1 in all seven and no bytes or
// records.  fixed and the records (rec_kb = kind | base << 4, rec_pos) may be
// off (NULL); rec_off holds ntasks + 1 offsets.  No LDS, no atomics.
__global__ void __launch_bounds__(64 * PAW_NW)
k_pa_fix(const DPTask *__restrict__ tasks, int ntasks, const uint8_t *__restrict__ bases,
         const int8_t *__restrict__ moves, const int64_t *__restrict__ moves_off,
         const int32_t *__restrict__ nmoves, uint8_t *__restrict__ fixed, uint8_t *__restrict__ rec_kb,
         int32_t *__restrict__ rec_pos, const int64_t *__restrict__ rec_off, int32_t *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int t = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * PAW_NW + (threadIdx.x >> 6)));
    if (t >= ntasks)
        return;
    const DPTask &T = tasks[t];
    const int n = T.n, m = T.m, oi = T.out_idx;
    const int cnt = nmoves[oi];
    if (cnt < 0) {
        if (lane < 2 + SF_TALLIES)
            out[(size_t)lane * ntasks + oi] = -1;
        return;
    }
    const uint8_t *s = bases + T.sb;
    const uint8_t *tt = bases + T.tb;
    const int64_t slot = moves_off[oi];
    const int8_t *mvs = moves + slot + (n + m - cnt);   // end-aligned by the walk
    uint8_t *fx = fixed ? fixed + slot : nullptr;
    const int64_t r0 = rec_kb ? rec_off[oi] : 0;
    const int cap = rec_kb ? (int)(rec_off[oi + 1] - r0) : 0;
    int bi = 0, bj = 0, bo = 0, bk = 0;   // i, j, corrected bases and proposals of the chunks before
    int last_ins = -1;                    // j of the last insert of the chunks before
    bool amb = false;
    int tl[SF_TALLIES] = {0, 0, 0, 0, 0};
    for (int x0 = 0; x0 < cnt; x0 += 64) {
        const bool on = x0 + lane < cnt;
        const int mv = on ? mvs[x0 + lane] : 0;
        const int w = sf_width(mv), pr = sf_proposes(mv) ? 1 : 0;
        int sc = sf_di(mv) | (sf_dj(mv) << 8) | (w << 16) | (pr << 24);
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(sc, d, 64);
            sc += lane >= d ? up : 0;
        }
        const int i = bi + (sc & 255), j = bj + ((sc >> 8) & 255);
        const int o = bo + ((sc >> 16) & 255) - w, k = bk + ((sc >> 24) & 255) - pr;
        if (fx) {
            if (mv == 1)
                fx[o] = tt[j - 1];
            else if (mv == 2)
                fx[o] = s[i - 1];
            else if (mv == 5) {
#pragma unroll
                for (int u = 0; u < 3; ++u)
                    fx[o + u] = tt[j - 3 + u];
            }
        }
        if (rec_kb && pr && k < cap) {
            rec_kb[r0 + k] = (uint8_t)(mv == 2 ? SF_INS | (s[i - 1] << 4) : SF_DEL);
            rec_pos[r0 + k] = j;
        }
        const uint64_t insm = __ballot(mv == 2);
        const uint64_t below = insm & ((1ull << lane) - 1);
        const int jp = __shfl(j, below ? 63 - __builtin_clzll(below) : lane, 64);
        amb = amb || __ballot(mv == 2 && j == (below ? jp : last_ins)) != 0;
        if (insm)
            last_ins = __builtin_amdgcn_readlane(j, __builtin_amdgcn_readfirstlane(63 - __builtin_clzll(insm)));
#pragma unroll
        for (int c = 0; c < SF_TALLIES; ++c)
            tl[c] += __popcll(__ballot(mv == c + 1));
        const int tot = __builtin_amdgcn_readlane(sc, 63);
        bi += tot & 255;
        bj += (tot >> 8) & 255;
        bo += (tot >> 16) & 255;
        bk += (tot >> 24) & 255;
    }
    if (lane == 0) {
        out[oi] = amb ? -2 : bo;
        out[(size_t)ntasks + oi] = bk;
#pragma unroll
        for (int c = 0; c < SF_TALLIES; ++c)
            out[(size_t)(2 + c) * ntasks + oi] = tl[c];
    }
}

// ---------------------------------------------------------------------
// k_dpm: very wide bands without codon moves across several CUs (round 6;
// edit_distance's band, align.jl:253-260: bw = ceil(min(m, n) / 2), H ~ m,
// configs[2]: H = 2,624, one band per call).  Round 5 ran such a band in
// one 1024-thread workgroup (k_dpw: a barrier per anti-diagonal, issue-bound
// on one CU, 3.35 ms per call).  Here the band is cut into slices of DPM_OWN
// band-row pairs, one single-wave workgroup each (no barrier per step),
// which meet only every DPM_B anti-diagonals:
//   - the wave holds 64 * DPM_NPL consecutive pairs: its slice and DPM_B / 2
//     pairs (DPM_B diagonals) of each neighbouring slice.  After a hand-off
//     every pair holds exact values; in the next DPM_B steps a wrong value
//     enters at the wave's outer edges (their outer neighbours are unknown)
//     and spreads inward one diagonal per step, so it never reaches the
//     slice before the next hand-off refreshes the halo pairs;
//   - the kappa-1 values of neighbouring diagonals move between lanes by DPP
//     (wave_shr / wave_shl), within a lane in registers;
//   - row records and template bases come from LDS rings, filled 64 rows /
//     columns at a time one chunk of 64 periods ahead; the rings carry a
//     mirrored tail, so a lane's ring index is its constant plus the
//     period's scalar one (no wrap per read);
//   - a cell is a fixed sequence of selects: its validity is a per-lane
//     range of periods, its store a buffer store whose offset is per-lane
//     (lanes outside the slice or the band get an offset past the band and
//     the range check drops the store); the origin, the final cell and a
//     last period without its odd step are separate (EDGE) periods;
//   - a wave computes only its compute phase, the periods at which some
//     pair it holds is in the DP; before and after, its cells are -Inf
//     stores (configs[2]: 2,602 of the band's 7,826 anti-diagonals);
//   - hand-off through the band itself: the host fills each band with an
//     all-ones pattern (a NaN no sum produces) before the launch; the slice
//     stores every in-band cell it owns (write-through, sc1) and a wave
//     takes its halo pairs' last two values where they are in the DP by
//     polling those cells (sc1 loads, 64-bit single-copy atomic) until none
//     holds the pattern -- one round trip, no flag and no store drain
//     (bounded: error 4 rather than a hang);
//   - a band's slices run on one XCD (workgroup i runs on XCD i % 8), the
//     bands of a launch spread over the eight.
// Same candidates, FP64 sums and strict-'>' values as k_dp: bit-identical;
// cells left of the DP (jj < 0) are stored as -Inf, which k_dp leaves out.
// ---------------------------------------------------------------------
// DPM_NPL / DPM_B / DPM_OWN, dpm_slices and the slice limits: rifraf_dp_plan.h
constexpr int DPM_RING = 512;                     // staged rows / columns (8 blocks of 64)
constexpr int DPM_RINGX = DPM_RING + 64 * DPM_NPL;   // + the mirrored tail
constexpr int DPM_SPIN = 1 << 22;                 // polls before error 4
constexpr unsigned DPM_NOSTORE = 0x80000000u;     // past every band (K * P * 8 < 2^31)
constexpr long long DPM_UNSET = -1;               // the fill pattern of a band not yet stored
constexpr int DPM_SC1 = 16;                       // buffer-store cache policy: sc1 (write-through)
static_assert(DPM_OWN > 0 && (DPM_B / 2) % DPM_NPL == 0 && 128 % DPM_B == 0, "slice geometry");

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ double ld_sc1(const double *p)
{
    return __longlong_as_double(
        (long long)__hip_atomic_load((unsigned long long *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

template <bool TRIM>
__global__ void __launch_bounds__(64)
k_dpm(const DPTask *__restrict__ tasks, int ntasks, int G, const uint8_t *__restrict__ bases,
      const double *__restrict__ tabs, double *__restrict__ bands, double *__restrict__ out_score,
      int *__restrict__ err)
{
    // workgroup i runs on XCD i % 8: task t takes XCD t % 8, its slice g
    // the workgroups 8 ((t / 8) G + g) + t % 8
    const int row = blockIdx.x >> 3, task = (row / G) * 8 + (blockIdx.x & 7), g = row % G;
    if (task >= ntasks)
        return;
    const DPTask T = tasks[task];
    const int npairs = (T.H + 1) >> 1;
    const int Gt = dpm_slices(T.H);
    if (g >= Gt)
        return;
    const int q = threadIdx.x;
    const bool rev = T.flags & 1, skew = T.flags & 2, trim = TRIM && (T.flags & 4);
    const uint8_t *sbase = bases + T.sb;
    const uint8_t *tbase = bases + T.tb;
    const double *tb = tabs + T.tab;
    double *band = bands + T.band;
    const int K = T.klen, H = T.H;
    const int own_lo = g * DPM_OWN, own_hi = min(own_lo + DPM_OWN, npairs);
    const int pb = own_lo - DPM_B / 2;           // the pair of lane 0, r = 0
    const __amdgpu_buffer_rsrc_t brs =
        __builtin_amdgcn_make_buffer_rsrc(band, 0, (int)((int64_t)K * T.P * 8), 0x00020000);
    __shared__ dvec2 s_rec[2 * DPM_RINGX];      // {mt, mm}, {is, ds} per read row
    __shared__ uint8_t s_sb[DPM_RINGX], s_col[DPM_RINGX];
    // pair pp = pb + x at period P reads read row x + P + par + rbase and
    // template column P + 64 DPM_NPL - 1 - x + cbase: ring entries
    // (x + P + par) and (P + 64 DPM_NPL - 1 - x), blocks of 64 entries
    const int rbase = pb - T.c, cbase = -(pb + 64 * DPM_NPL - 1);
    static_assert(64 * (DPM_NPL + 2) <= DPM_RING, "ring holds the chunk's blocks and the next");
    // a block's loads are held raw until it is put in LDS a chunk later (a
    // select right after them would make hipcc wait for them at once; k_dpx)
    struct Blk {
        RawRow r;
        int col;
        bool colok;
    };
    auto blk_load = [&](int b) {
        Blk x;
        x.r = load_row_raw(T, rev, sbase, tb, rbase + 64 * b + q, false);
        const int jj = cbase + 64 * b + q;
        const int jc = min(max(jj, 1), max(T.m, 1));
        x.col = tbase[rev ? max(T.m - jc, 0) : jc - 1];
        x.colok = jj >= 1 && jj <= T.m;
        return x;
    };
    auto blk_put = [&](int b, const Blk &x) {
        const RowRec rr = row_val(x.r);
        const dvec2 m2{rr.mt, skew ? rr.mm * 0.99 : rr.mm}, i2{rr.is, rr.ds};
        const int i = ((64 * b) & (DPM_RING - 1)) + q;
        s_rec[2 * i] = m2;
        s_rec[2 * i + 1] = i2;
        s_sb[i] = (uint8_t)rr.sb;
        s_col[i] = (uint8_t)(x.colok ? x.col : 4);
        if (i < DPM_RINGX - DPM_RING) {          // the mirrored tail
            s_rec[2 * (i + DPM_RING)] = m2;
            s_rec[2 * (i + DPM_RING) + 1] = i2;
            s_sb[i + DPM_RING] = (uint8_t)rr.sb;
            s_col[i + DPM_RING] = (uint8_t)(x.colok ? x.col : 4);
        }
    };
    // per pair and parity: the periods at which the cell is in the DP
    // (d <= k, jj <= m, 0 <= ii <= n: P in [lo, lo + span]), the store offset
    int lo[2][DPM_NPL];
    unsigned span[2][DPM_NPL], vo[2][DPM_NPL];
    bool own[DPM_NPL];
#pragma unroll
    for (int r = 0; r < DPM_NPL; ++r) {
        const int pp = pb + q * DPM_NPL + r;
        own[r] = pp >= own_lo && pp < own_hi;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int d = 2 * pp + a;
            const bool inb = pp >= 0 && d < H;
            const int l = max(pp, T.c - pp - a), h = min(pp + T.m, T.n + T.c - pp - a);
            const bool ok = inb && l <= h;
            lo[a][r] = ok ? l : (1 << 30);
            span[a][r] = ok ? (unsigned)(h - l) : 0u;
            vo[a][r] = (inb && own[r]) ? 8u * (unsigned)((rev ? H - 1 - d : d) >> 1) : DPM_NOSTORE;
        }
    }
    const int porg = T.c >> 1;                       // the origin (ii = jj = 0): pair c / 2, step c
    const int kfin = T.n + T.m + T.c;                // the final cell (ii = n, jj = m)
    // the wave's compute phase [Pa, Pb]: every pair it holds (slice and halo)
    // is outside the DP before Pa and after Pb, i.e. -Inf there -- those
    // periods are stores of -Inf only (for configs[2]'s band, the ~2,600 of
    // 7,826 anti-diagonals before the origin and after the final cell)
    int la = 1 << 30, hb = -1;
#pragma unroll
    for (int r = 0; r < DPM_NPL; ++r)
#pragma unroll
        for (int a = 0; a < 2; ++a)
            if (lo[a][r] != (1 << 30)) {
                la = min(la, lo[a][r]);
                hb = max(hb, lo[a][r] + (int)span[a][r]);
            }
    for (int o = 32; o > 0; o >>= 1) {
        la = min(la, __shfl_xor(la, o));
        hb = max(hb, __shfl_xor(hb, o));
    }
    const int Pa = __builtin_amdgcn_readfirstlane(la), Pb = __builtin_amdgcn_readfirstlane(hb);
    const int NPER = (K + 1) >> 1;                   // periods: steps 2P, 2P + 1 < K
    const unsigned dso = 8u * (unsigned)(rev ? -T.P : T.P);   // band row step in bytes
    const unsigned so_base = 8u * (unsigned)((rev ? K - 1 : 0) * T.P);
    auto so_of = [&](int P) { return so_base + (unsigned)(2 * P) * dso; };
    // a period outside the compute phase: -Inf in every in-band cell the slice owns
    auto blank = [&](int P) {
        const unsigned so0 = so_of(P);
#pragma unroll
        for (int r = 0; r < DPM_NPL; ++r) {
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, -RF_INF), brs, vo[0][r], so0, DPM_SC1);
            if (2 * P + 1 < K)
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, -RF_INF), brs, vo[1][r], so0 + dso,
                                                      DPM_SC1);
        }
    };
    double vev[DPM_NPL], vod[DPM_NPL];
    // a pair's row record for its even step is the record its odd step read
    // one period earlier (read row pp + P - c either way): carried here
    dvec2 rmt[DPM_NPL], ris[DPM_NPL];
    int rsb[DPM_NPL];
    uint64_t bad[DPM_NPL];                       // lanes with a valid cell of -Inf
    Blk pend;
    if (Pa <= Pb) {
        // chunk t0 of Pa: blocks t0 .. t0 + DPM_NPL in the ring, t0 + DPM_NPL + 1 loading
        const int t0 = Pa >> 6;
        for (int b = t0; b <= t0 + DPM_NPL; ++b)
            blk_put(b, blk_load(b));
        pend = blk_load(t0 + DPM_NPL + 1);
        wave_sync();
    }
#pragma unroll
    for (int r = 0; r < DPM_NPL; ++r) {
        vev[r] = vod[r] = -RF_INF;
        bad[r] = 0;
        const int ri = q * DPM_NPL + r + (Pa & (DPM_RING - 1));
        rmt[r] = s_rec[2 * ri];
        ris[r] = s_rec[2 * ri + 1];
        rsb[r] = s_sb[ri];
    }
    // one period P of the compute phase: the even step 2P and the odd step
    // 2P + 1.  The LDS reads of both (the period's template bases, the odd
    // step's row records) are issued first.  EDGE: the period may hold the
    // origin, the final cell or no odd step (K odd).
    auto period = [&](auto EDGEC, const int P) {
        constexpr bool EDGE = decltype(EDGEC)::value;
        const bool odd_too = !EDGE || 2 * P + 1 < K;
        const unsigned so0 = so_of(P);
        const int s = P & (DPM_RING - 1);
        const int ir = q * DPM_NPL + 1 + s, ic = s + 64 * DPM_NPL - 1 - q * DPM_NPL;
        int tbb[DPM_NPL];
        dvec2 omt[DPM_NPL], ois[DPM_NPL];
        int osb[DPM_NPL];
#pragma unroll
        for (int r = 0; r < DPM_NPL; ++r) {
            tbb[r] = s_col[ic - r];
            omt[r] = s_rec[2 * (ir + r)];
            ois[r] = s_rec[2 * (ir + r) + 1];
            osb[r] = s_sb[ir + r];
        }
        auto cells = [&](auto PARC, const dvec2 (&mt)[DPM_NPL], const dvec2 (&is2)[DPM_NPL], const int (&sbr)[DPM_NPL]) {
            constexpr int par = decltype(PARC)::value;
            const int k = 2 * P + par;
            const unsigned so = par ? so0 + dso : so0;
            // the neighbouring pair's kappa - 1 value across the lane edge
            // (lanes 0 and 63 hold halo pairs or pairs outside the band: what
            // they receive there is never a slice's value)
            const double nbL = par ? 0.0 : dpp_rot_f64<TaskLanes<64>::FROM_L1>(vod[DPM_NPL - 1]);
            const double nbR = par ? dpp_rot_f64<TaskLanes<64>::FROM_R1>(vev[0]) : 0.0;
            double nv[DPM_NPL];
            bool val[DPM_NPL];
#pragma unroll
            for (int r = 0; r < DPM_NPL; ++r) {
                const double a2 = par ? vod[r] : vev[r];
                const double a1l = par ? vev[r] : (r > 0 ? vod[r > 0 ? r - 1 : 0] : nbL);
                const double a1r = par ? (r < DPM_NPL - 1 ? vev[r < DPM_NPL - 1 ? r + 1 : 0] : nbR) : vod[r];
                const double ms = sbr[r] == tbb[r] ? mt[r].x : mt[r].y;
                double is = is2[r].x;
                if (TRIM) {
                    const int jj = P - (pb + q * DPM_NPL + r);
                    is = (trim && (jj == 0 || jj == T.m)) ? 0.0 : is;
                }
                // align.jl:77-104: the maximum of the candidates
                const double best = fmax(fmax(a2 + ms, a1l + is), a1r + is2[r].y);
                val[r] = (unsigned)(P - lo[par][r]) <= span[par][r];
                nv[r] = val[r] ? best : -RF_INF;
            }
            if (EDGE && k == T.c) {
#pragma unroll
                for (int r = 0; r < DPM_NPL; ++r)
                    nv[r] = (pb + q * DPM_NPL + r == porg && val[r]) ? 0.0 : nv[r];
            }
#pragma unroll
            for (int r = 0; r < DPM_NPL; ++r) {
                // "new score is invalid"
                bad[r] |= __builtin_amdgcn_ballot_w64(nv[r] == -RF_INF) & __builtin_amdgcn_ballot_w64(val[r]);
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, nv[r]), brs, vo[par][r], so,
                                                      DPM_SC1);
                if (par)
                    vod[r] = nv[r];
                else
                    vev[r] = nv[r];
            }
            if (EDGE && k == kfin && out_score) {
#pragma unroll
                for (int r = 0; r < DPM_NPL; ++r)
                    if (own[r] && val[r] && pb + q * DPM_NPL + r == P - T.m)
                        out_score[T.out_idx] = nv[r];
            }
        };
        cells(std::integral_constant<int, 0>{}, rmt, ris, rsb);
        if (odd_too)
            cells(std::integral_constant<int, 1>{}, omt, ois, osb);
#pragma unroll
        for (int r = 0; r < DPM_NPL; ++r) {
            rmt[r] = omt[r];
            ris[r] = ois[r];
            rsb[r] = osb[r];
        }
    };
    // ---- hand-off after period P: the halo pairs' values at steps 2P (even
    // diagonal) and 2P + 1 (odd), polled from their owners' cells where the
    // cell is in the DP (an owner computes every such cell; -Inf elsewhere)
    auto hand_off = [&](const int P) {
        const unsigned so0 = so_of(P);
        bool pe[DPM_NPL], po[DPM_NPL];
        const double *ae[DPM_NPL], *ao[DPM_NPL];
#pragma unroll
        for (int r = 0; r < DPM_NPL; ++r) {
            pe[r] = !own[r] && (unsigned)(P - lo[0][r]) <= span[0][r];
            po[r] = !own[r] && (unsigned)(P - lo[1][r]) <= span[1][r];
            const int pp = pb + q * DPM_NPL + r, de = 2 * pp, dod = 2 * pp + 1;
            ae[r] = band + (pe[r] ? (so0 >> 3) + ((rev ? H - 1 - de : de) >> 1) : 0);
            ao[r] = band + (po[r] ? ((so0 + dso) >> 3) + ((rev ? H - 1 - dod : dod) >> 1) : 0);
        }
        double he[DPM_NPL], ho[DPM_NPL];
        for (int spins = 0;; ++spins) {
#pragma unroll
            for (int r = 0; r < DPM_NPL; ++r) {
                he[r] = ld_sc1(ae[r]);
                ho[r] = ld_sc1(ao[r]);
            }
            __builtin_amdgcn_s_waitcnt(0);
            int wait = 0;
#pragma unroll
            for (int r = 0; r < DPM_NPL; ++r)
                wait |= ((int)pe[r] & (int)(__double_as_longlong(he[r]) == DPM_UNSET)) |
                        ((int)po[r] & (int)(__double_as_longlong(ho[r]) == DPM_UNSET));
            if (__builtin_amdgcn_ballot_w64(wait != 0) == 0)
                break;
            if (spins >= DPM_SPIN)
                return false;   // a neighbouring slice never arrived
            __builtin_amdgcn_s_sleep(2);
        }
#pragma unroll
        for (int r = 0; r < DPM_NPL; ++r) {
            if (own[r])
                continue;
            vev[r] = pe[r] ? he[r] : -RF_INF;
            vod[r] = po[r] ? ho[r] : -RF_INF;
        }
        // nothing of the hand-off left in flight: a register still pending at
        // the loop head would make hipcc wait vmcnt(0) -- every band store --
        // once per period
        __builtin_amdgcn_s_waitcnt(0);
        return true;
    };
    // chunk refill at P = 64 t (t > t0), the period, the hand-off every DPM_B steps
    auto body = [&](auto EDGEC, const int P) {
        if ((P & 63) == 0 && P != Pa) {          // chunk t: rows / columns of block t + DPM_NPL
            const int t = P >> 6;
            __builtin_amdgcn_s_waitcnt(0);       // after a hand-off: nothing left in flight
            blk_put(t + DPM_NPL, pend);
            pend = blk_load(t + DPM_NPL + 1);
            wave_sync();
        }
        period(EDGEC, P);
        const int kn = 2 * P + 2;                // steps done
        return !(kn % DPM_B == 0 && P < Pb) || hand_off(P);
    };
    // the compute phase first (its hand-offs pace the neighbours), in runs of
    // plain periods between the special ones
    const int psp[3] = {porg, kfin >> 1, (K & 1) ? NPER - 1 : INT_MAX};
    bool ok = true;
    for (int P = Pa; P <= Pb && ok;) {
        int stop = Pb + 1;
        for (int i = 0; i < 3; ++i)
            if (psp[i] >= P && psp[i] < stop)
                stop = psp[i];
        for (; P < stop && ok; ++P)
            ok = body(std::false_type{}, P);
        if (P <= Pb && ok) {
            ok = body(std::true_type{}, P);
            ++P;
        }
    }
    if (!ok) {
        set_err(err, 4);
        return;
    }
    for (int P = 0; P < min(Pa, NPER); ++P)
        blank(P);
    for (int P = max(Pb + 1, Pa <= Pb ? 0 : NPER); P < NPER; ++P)
        blank(P);
    bool e = false;
#pragma unroll
    for (int r = 0; r < DPM_NPL; ++r)
        e = e || (own[r] && ((bad[r] >> q) & 1));
    if (e)
        set_err(err, 1);
}

// ---------------------------------------------------------------------
// k_dpx: latency-bound non-lean tasks (round 5).
//
// The reference's codon DP (align.jl:77-104 with codon moves; skew_matches
// for single_indel_proposals, model.jl:538-562) is one task of ~5,000
// anti-diagonals per call: nothing else runs beside it, so its time is the
// step latency of one wave, i.e. the instructions one step issues.  k_dpr's
// general step moved every row record through the lanes (7 DPP moves per
// value and period), took the codon neighbours by two wave shifts each and
// waited for its edge loads with vmcnt(0) -- ~900 cycles per anti-diagonal
// (profiles/r05a_kernel_stats_c3.csv).  Here one task owns a single-wave
// workgroup, lane q holds the diagonal pair {2q, 2q+1} (H <= 127), and
//   - the row records {match, mismatch (x 0.99 under skew), ins, del,
//     codon ins, codon del, base} and the template bases are staged in LDS
//     rings of 256 rows / columns, 64 at a time, loaded a block ahead:
//     lane q reads row P + q + par - c and column P - q at period P (one
//     LDS read set per period instead of the systolic moves);
//   - every anti-diagonal's values go to a 4-row LDS ring as well, so the
//     codon neighbours (d -/+ 3 at kappa - 3) are two LDS reads at an
//     immediate offset; only the insert / delete neighbour at kappa - 1
//     (on the step-to-step chain) is a DPP wave shift;
//   - interior steps (every active diagonal inside the matrix, codon moves
//     allowed, no trim column) carry no range checks: inactive diagonals
//     get -Inf by an additive mask, as in the lean kernels.
// Same candidates, same FP64 sums and the same strict-'>' value (the max of
// the candidates; no NaN, no -0.0) as k_dpr / k_dp, stored in the same
// kappa-major positions (reverse: flipped), so bands, scores and errors are
// bit-identical.
// ---------------------------------------------------------------------
constexpr int DPX_W = 72;       // doubles per LDS band row: 2 pad | 64 lanes | 6 pad (-Inf)
#ifndef DPX_STAGE
#define DPX_STAGE 1   // interior rows staged in LDS, four per contiguous flush
#endif
#ifndef DPX_FL16
#define DPX_FL16 1    // the flush in 16-B stores when the run is 16-B aligned
#endif
constexpr int DPX_RING = 256;   // staged rows / columns: 4 blocks of 64
struct DpxStage {
    RawRow r;
    int col;
    bool colok;
};

constexpr unsigned DPX_NOSTORE = 0x80000000u;   // buffer offset past any band: the store is dropped

template <int PAR, bool FAST, bool CODON, bool CHECK>
__device__ __forceinline__ double dpx_cell(const DPTask &T, bool trim, int d, int ii, int jj, double v1,
                                           double v2, double xn, double yci, double ycd, const dvec2 &mtmm,
                                           const dvec2 &isds, const dvec2 &cicd, int sb, int tbb, double lbv,
                                           uint64_t actm, uint64_t &emask, int &eflag, double &fval, int &fset)
{
    const double ms = sb == tbb ? mtmm.x : mtmm.y;   // mismatch staged x 0.99 under skew (align.jl:70-72)
    const double x_ins = PAR ? v1 : xn;               // (d-1, kappa-1)
    const double x_del = PAR ? xn : v1;               // (d+1, kappa-1)
    if (FAST) {
        // candidates off the step-to-step chain first, the kappa-1 pair last
        const double t = CODON ? fmax(fmax(v2 + ms, yci + cicd.x), ycd + cicd.y) : v2 + ms;
        const double best = fmax(t, fmax(x_ins + isds.x, x_del + isds.y));
        if (CHECK)
            emask |= __ballot(best == -RF_INF) & actm;   // "new score is invalid" (active diagonals)
        return best + lbv;
    }
    const bool valid = d < T.H && jj >= 0 && jj <= T.m && ii >= 0 && ii <= T.n;
    const double is = (trim && (jj == 0 || jj == T.m)) ? 0.0 : isds.x;   // align.jl:74-76
    double best = fmax(fmax(v2 + ms, x_ins + is), x_del + isds.y);
    if (CODON) {
        const double cd = jj >= 3 ? cicd.y : -RF_INF;       // codon delete needs j > 3
        best = fmax(fmax(best, yci + cicd.x), ycd + cd);   // cicd.x is -Inf unless i > 3 (staged)
    }
    const bool origin = ii == 0 && jj == 0;
    const double v = valid ? (origin ? 0.0 : best) : -RF_INF;
    eflag |= (valid && !origin && best == -RF_INF) ? 1 : 0;
    const bool fin = valid && ii == T.n && jj == T.m;
    fval = fin ? v : fval;
    fset |= fin ? 1 : 0;
    return v;
}

// CODON: the task may have codon moves (ring of the last four anti-diagonals
// in LDS); CHECK: the interior raises "new score is invalid" (non-finite
// tables).  <false, false> takes the latency-mode lean tasks (finite tables,
// no codon / skew / trim, RF_OPT_DP_LAT), <true, true> every other task.
template <bool CODON, bool CHECK>
__global__ void __launch_bounds__(128)
k_dpx(const DPTask *__restrict__ tasks, int ntasks, const uint8_t *__restrict__ bases,
      const double *__restrict__ tabs, double *__restrict__ bands, double *__restrict__ out_score,
      int *__restrict__ err)
{
    __shared__ dvec2 s_mtmm[DPX_RING], s_isds[DPX_RING], s_cicd[CODON ? DPX_RING : 1];
    __shared__ int s_sb[DPX_RING], s_col[DPX_RING];
    __shared__ double s_band[CODON ? 4 * DPX_W : 1];
    // DPX_STAGE: the interior's four rows of a pair of periods, staged here
    // and written as one contiguous run (P <= 65)
    // (lean tasks only: the reference's single codon task, latency-bound on
    // one wave, ran 0.43 -> 0.61 ms with it; 1,000 lean reads 0.52 -> 0.49 ms,
    // profiles/r05bt_exp_dpx_stage.jsonl)
    constexpr bool STAGE = DPX_STAGE && !CODON;
    __shared__ __attribute__((aligned(16))) double s_out[STAGE ? 4 * 72 : 1];
    // wave 0 fills the band; wave 1 stages the edge records (round 5: its
    // loads' waits are its own, so the filling wave never waits on vmcnt,
    // which would drain its band stores too)
    const int q = threadIdx.x & 63;
    const bool loader = threadIdx.x >= 64;
    const DPTask T = tasks[blockIdx.x];   // one task per workgroup
    const bool rev = T.flags & 1, skew = T.flags & 2, trim = T.flags & 4;
    const bool codon = CODON && (T.ncins > 0 || T.ncdel > 0);
    const uint8_t *sbase = bases + T.sb;
    const uint8_t *tbase = bases + T.tb;
    const double *tb = tabs + T.tab;
    const int K = T.klen;
    // band stores through a buffer resource: a lane that stores nothing at a
    // step gets an offset past the band (dropped by the range check), so no
    // step changes exec for its store (the host keeps K * P * 8 < 2^31)
    const __amdgpu_buffer_rsrc_t brs =
        __builtin_amdgcn_make_buffer_rsrc(bands + T.band, 0, (int)((int64_t)K * T.P * 8), 0x00020000);
    if (CODON && !loader)
        for (int e = q; e < 4 * DPX_W; e += 64)
            s_band[e] = -RF_INF;

    // block b: rows R = P + q + par in [64b, 64b + 64) (read row R - c) and
    // columns J = P - q + 64 in [64b, 64b + 64) (template column J - 64)
    // A block's loads are held raw (load_row_raw) until the block is put in
    // LDS a chunk later, and their range selects (and the skew factor) are
    // applied there: a select right after the loads made hipcc wait for them
    // at once, draining every band store in flight (vmcnt counts both).
    auto stage_load = [&](int b) {
        DpxStage s;
        s.r = load_row_raw(T, rev, sbase, tb, 64 * b + q - T.c, codon);
        const int jj = 64 * b + q - 64;
        const int jc = min(max(jj, 1), max(T.m, 1));
        s.col = tbase[rev ? max(T.m - jc, 0) : jc - 1];
        s.colok = jj >= 1 && jj <= T.m;
        return s;
    };
    auto stage_put = [&](int b, const DpxStage &s) {
        const int i = (64 * b + q) & (DPX_RING - 1);
        const RowRec r = row_val(s.r);
        s_mtmm[i] = dvec2{r.mt, skew ? r.mm * 0.99 : r.mm};
        s_isds[i] = dvec2{r.is, r.ds};
        if (CODON)
            s_cicd[i] = dvec2{r.ci, r.cd};
        s_sb[i] = r.sb;
        s_col[i] = s.colok ? s.col : 4;
    };

    // interior [klo, khi]: every diagonal with cells in the matrix has its
    // cell inside the matrix (with i, j > 3: codon moves open) and j in
    // 1..m-1 (trim off); the origin and the final cell lie outside it
    double lb[2];
    bool act[2];
    // kappa of (0, 0) + 1, and at least H: every band diagonal has d <= kappa
    // (stored); kappa of (n, m) - 1
    int lo = max(T.c + 1, T.H), hi = T.n + T.c + T.m - 1;
    bool ok = true;
#pragma unroll
    for (int par = 0; par < 2; ++par) {
        const int d = 2 * q + par;
        const int mlo = max(0, T.c - d), mhi = min(T.m, T.n + T.c - d);
        act[par] = d < T.H && mlo <= mhi;
        lb[par] = act[par] ? 0.0 : -RF_INF;
        if (act[par]) {
            const int jlo = CODON ? max(3, T.c + 3 - d) : max(trim ? 1 : 0, T.c - d);
            const int jhi = min(T.m - (trim ? 1 : 0), T.n + T.c - d);
            ok = ok && jlo <= jhi;
            lo = max(lo, d + 2 * jlo);
            hi = min(hi, d + 2 * jhi);
        }
    }
    for (int off = 32; off >= 1; off >>= 1) {
        lo = max(lo, __shfl_xor(lo, off));
        hi = min(hi, __shfl_xor(hi, off));
    }
    const int klo = __builtin_amdgcn_readfirstlane(__all(ok) ? lo : INT_MAX);
    const int khi = __builtin_amdgcn_readfirstlane(hi);

    const int npairs = (K + 3) >> 2;
    if (loader) {
        // blocks 0-2 before the fill starts; block t + 3 during chunk t (ring
        // slot of block t - 1, which chunk t no longer reads), one barrier
        // per chunk boundary 1 .. nch - 1
        stage_put(0, stage_load(0));
        stage_put(1, stage_load(1));
        stage_put(2, stage_load(2));
        lds_barrier();
        const int nch = (npairs + 31) >> 5;
        for (int t = 0; t + 1 < nch; ++t) {
            stage_put(t + 3, stage_load(t + 3));
            lds_barrier();
        }
        return;
    }
    lds_barrier();

    // per parity: byte offset of this lane's band element in a kappa row
    // (reverse: flipped), or past the band when the row does not hold it
    const unsigned vo0 = 2 * q < T.H ? 8u * (unsigned)(rev ? (T.H - 1 - 2 * q) >> 1 : q) : DPX_NOSTORE;
    const unsigned vo1 = 2 * q + 1 < T.H ? 8u * (unsigned)(rev ? (T.H - 2 - 2 * q) >> 1 : q) : DPX_NOSTORE;
    const unsigned rowb = 8u * (unsigned)T.P;
    const uint64_t actm0 = __ballot(act[0]), actm1 = __ballot(act[1]);
    double v1 = -RF_INF, v2 = -RF_INF;
    uint64_t emask = 0;
    int eflag = 0, fset = 0;
    double fval = 0.0;
    // Records of a pair of periods (2u, 2u + 1): rows R = 2u + q (c), 2u + q + 1
    // (a), 2u + q + 2 (b) and columns J = 2u - q + 64, + 1.  Pair u reads the
    // records of pair u + 1 (rows 2u + q + 3, + 4 and the next columns) into
    // set u mod 3; its own a / b are set u - 1 and its c is the b of set u - 2.
    // The loop runs three pairs per iteration with the sets rotated by name,
    // so no record moves between registers (round 5: the one-pair loop copied
    // 17 registers per pair at its end, ~4 of the ~22 instructions per step).
    struct Rec {
        dvec2 mtmm, isds, cicd;
        int sb;
    };
    auto rec_ld = [&](int r) {
        Rec x;
        x.mtmm = s_mtmm[r];
        x.isds = s_isds[r];
        x.cicd = CODON ? s_cicd[r] : dvec2{0.0, 0.0};
        x.sb = s_sb[r];
        return x;
    };
    Rec A0, B0, A1, B1, A2, B2;
    int C00 = 0, C01 = 0, C10 = 0, C11 = 0, C20, C21;
    B1 = rec_ld(q);              // set -2: b = row q
    A2 = rec_ld(q + 1);          // set -1: rows q + 1, q + 2, columns 64 - q, 65 - q
    B2 = rec_ld(q + 2);
    C20 = s_col[(64 - q) & (DPX_RING - 1)];
    C21 = s_col[(65 - q) & (DPX_RING - 1)];
    A0 = A1 = B0 = A2;           // (defined before their first load)
    // the codon neighbours of the next step, read one step ahead (kappa = 0:
    // ring row 1, still -Inf)
    double cy_ci = CODON ? s_band[DPX_W + 2 + q - 2] : 0.0, cy_cd = CODON ? s_band[DPX_W + 2 + q + 1] : 0.0;
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    using I3 = std::integral_constant<int, 3>;
    using BT = std::integral_constant<bool, true>;
    using BF = std::integral_constant<bool, false>;
    // byte offset of kappa row 4u (reverse: K - 1 - 4u), advanced once per
    // pair of periods (the per-step select and multiply off the loop)
    const int drow = rev ? -(int)rowb : (int)rowb;
    unsigned rob = rev ? rowb * (unsigned)(K - 1) : 0u;
    auto pair = [&](const int u, const Rec &c, const Rec &a, const Rec &b, const int col0, const int col1, Rec &na,
                    Rec &nb, int &ncol0, int &ncol1) {
        if ((u & 31) == 0 && u > 0)   // chunk t = u / 32 (64 periods): block t + 2 is in
            lds_barrier();
        // the next pair's records (rows <= 2u + 67: block t + 2 at most, in LDS)
        na = rec_ld((2 * u + q + 3) & (DPX_RING - 1));
        nb = rec_ld((2 * u + q + 4) & (DPX_RING - 1));
        ncol0 = s_col[(2 * u - q + 66) & (DPX_RING - 1)];
        ncol1 = s_col[(2 * u - q + 67) & (DPX_RING - 1)];
        // four steps kappa = 4u + s: (period, parity) = (2u, 0), (2u, 1), (2u+1, 0), (2u+1, 1)
        auto step = [&](auto FASTC, auto PARC, auto SC, int per, const Rec &r, int col) {
            constexpr bool FAST = decltype(FASTC)::value;
            constexpr int PAR = decltype(PARC)::value, S = decltype(SC)::value;
            const int k = 4 * u + S;
            if (!FAST && k >= K)
                return;
            // the kappa - 1 neighbour by a wave rotate: lane 0 (63) receives the
            // value of diagonal 127 (0 at kappa - 1 into diagonal 127), and
            // diagonal 127 >= H is -Inf / masked (the host sends H <= 127 only)
            const double xn = PAR ? dpp_rot_f64<TaskLanes<64>::ROT_R1>(v1) : dpp_rot_f64<TaskLanes<64>::ROT_L1>(v1);
            // codon neighbours at kappa - 3: d - 3 / d + 3 = lanes q - 2 / q + 1
            // (even), q - 1 / q + 2 (odd); this step's were read one step ago,
            // the next step's (ring row kappa - 2, the other parity) now
            const double yci = cy_ci, ycd = cy_cd;
            if (CODON) {
                const double *rr = s_band + ((S + 2) & 3) * DPX_W + 2 + q;
                cy_ci = rr[PAR ? -2 : -1];
                cy_cd = rr[PAR ? 1 : 2];
            }
            const int d = 2 * q + PAR;
            const int jj = per - q, ii = per + q + PAR - T.c;
            const double v = dpx_cell<PAR, FAST, CODON, CHECK>(T, trim, d, ii, jj, v1, v2, xn, yci, ycd, r.mtmm,
                                                               r.isds, r.cicd, r.sb, col, lb[PAR],
                                                               PAR ? actm1 : actm0, emask, eflag, fval, fset);
            if (CODON) {
                s_band[S * DPX_W + 2 + q] = v;
                // other lanes read this row two and three steps on: keep hipcc
                // from hoisting those reads above the write (the three-pair loop
                // body gives it the room; LDS is in order within the wave)
                wave_sync();
            }
            const unsigned ro = rob + (unsigned)(S * drow);   // = rowb * (rev ? K - 1 - k : k)
            const unsigned vo = PAR ? vo1 : vo0;
            if (STAGE && FAST) {
                if (vo != DPX_NOSTORE)
                    s_out[(rev ? 3 - S : S) * T.P + (int)(vo >> 3)] = v;
            } else {
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), brs,
                                                      (FAST || d <= k) ? vo + ro : DPX_NOSTORE, 0, 0);
            }
            v2 = v1;
            v1 = v;
        };
        if (4 * u >= klo && 4 * u + 3 <= khi) {
            step(BT{}, I0{}, I0{}, 2 * u, c, col0);
            step(BT{}, I1{}, I1{}, 2 * u, a, col0);
            step(BT{}, I0{}, I2{}, 2 * u + 1, a, col1);
            step(BT{}, I1{}, I3{}, 2 * u + 1, b, col1);
            if (STAGE) {
                // rows 4u .. 4u + 3 (reverse: K - 4 - 4u .. K - 1 - 4u) are one
                // run of 4P doubles.  A 16-B aligned run (forward always; reverse
                // when K is even) goes out as 16-B stores of consecutive lanes,
                // a fixed DPX_FL16 per lane (4P <= 260 doubles: 130 pairs),
                // lanes past the run at an offset past the band; else 8-B
                // stores in a loop (round 6: the loop issued ~30 instructions
                // per pair of periods)
                wave_sync();
                const unsigned base = rev ? rob - 3u * rowb : rob;
                const int n = 4 * T.P;
                if (DPX_FL16 && (base & 15u) == 0) {
                    const dvec2 *s2 = reinterpret_cast<const dvec2 *>(s_out);
                    const int n2 = n >> 1;
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const int t = q + 64 * j;
                        const dvec2 v = s2[min(t, n2 - 1)];
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), brs,
                                                               t < n2 ? base + 16u * (unsigned)t : DPX_NOSTORE, 0,
                                                               0);
                    }
                } else {
                    for (int t = q; t < n; t += 64)
                        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, s_out[t]), brs,
                                                              base + 8u * (unsigned)t, 0, 0);
                }
                wave_sync();
            }
        } else {
            step(BF{}, I0{}, I0{}, 2 * u, c, col0);
            step(BF{}, I1{}, I1{}, 2 * u, a, col0);
            step(BF{}, I0{}, I2{}, 2 * u + 1, a, col1);
            step(BF{}, I1{}, I3{}, 2 * u + 1, b, col1);
        }
        rob += (unsigned)(4 * drow);
    };
    int u = 0;
    for (; u + 3 <= npairs; u += 3) {
        pair(u, B1, A2, B2, C20, C21, A0, B0, C00, C01);
        pair(u + 1, B2, A0, B0, C00, C01, A1, B1, C10, C11);
        pair(u + 2, B0, A1, B1, C10, C11, A2, B2, C20, C21);
    }
    if (u < npairs)
        pair(u, B1, A2, B2, C20, C21, A0, B0, C00, C01);
    if (u + 1 < npairs)
        pair(u + 1, B2, A0, B0, C00, C01, A1, B1, C10, C11);
    (void)ntasks;
    if (eflag || emask)
        set_err(err, 1);  // "new score is invalid"
    if (fset && out_score)
        out_score[T.out_idx] = fval;
}

// ---------------------------------------------------------------------
// k_score: dense proposal scoring of batch reads (no codon moves)
//
// One lane per consensus position p in [0, m].  For a read it evaluates
// every proposal anchored at p -- Substitution(p, b) (4 bases, the one equal
// to the consensus base is never requested), Deletion(p), Insertion(p, b) --
// from A columns p-1 and p and B column p (0-based), exactly as
// score_nocodon (model.jl:242-285) and seq_score_deletion (:227-236) do,
// with new columns built in the reference's update order.  The per-read
// results are left-folded over the group's reads in batch order
// (model.jl:389-393).  Output slots: 0-3 sub A,C,G,T; 4 del; 5-8 ins A,C,G,T.
// A failed update ("new score is invalid") or a -Inf sum ("failed to compute
// a valid score") is reported as NaN in that slot.
//
// The A/B kappa rows covering the 64 positions of a work item are one
// contiguous block; it is staged through LDS with coalesced loads when it
// fits (the common narrow band), otherwise read in place.
// ---------------------------------------------------------------------

// Accessor of a band window: rows [k0, ...) of a kappa-major band.
struct BandWin {
    const double *base;
    int k0, P;
    __device__ __forceinline__ double at(int d, int jj) const
    {
        return base[(size_t)(d + 2 * jj - k0) * P + (d >> 1)];
    }
};

// HALF 0: Substitution(p, b) chains + Deletion(p)  -> out[0..4]
// HALF 1: Insertion(p, b) chains                     -> out[5..8]
// (two waves of one workgroup share the staged A/B window).
// update() of a new column (align.jl:50-112) keeps the first strictly-best
// of {match, insert, delete}; its value is the FP64 max of the three sums
// (no NaN / signed zero among candidates), and the sums are formed from the
// same operands as the reference, so fmax is bit-exact.  A chain that hits
// -Inf ("new score is invalid") is detected by the running minimum.
template <int HALF>
__device__ __forceinline__ void score_half(int p, int m, const ScoreRead &R,
                                           const uint8_t *__restrict__ s,
                                           const double *__restrict__ tb,
                                           const BandWin A, const BandWin B, double out[5])
{
    const int n = R.n, c = R.c, vb = R.vb;
    const double *t_match = tb;
    const double *t_mism = tb + n;
    const double *t_ins = tb + 2 * (size_t)n;
    const double *t_del = tb + 3 * (size_t)n;
    const double qnan = __builtin_nan("");
    // row ranges (bandedarrays.jl:133-137), 0-based rows
    const int s0 = max(0, p - c), s1 = min(p + vb, n);             // rows(p): new Sub col, B col p
    double prev[4], acc[4], mn[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        prev[b] = -RF_INF;
        acc[b] = -RF_INF;
        mn[b] = RF_INF;
    }
    if (HALF == 0) {
        if (p < 1) {
#pragma unroll
            for (int k = 0; k < 5; ++k)
                out[k] = qnan;
            return;
        }
        const int d0 = max(0, p - 1 - c), d1 = min(p - 1 + vb, n);  // rows(p-1): A col p-1
        double del_acc = -RF_INF;
        // A(p-1, ii) in band iff ii in rows(p-1)
        double am1_prev = (s0 - 1 >= d0) ? A.at(s0 - 1 - (p - 1) + c, p - 1) : -RF_INF;
        for (int ii = s0; ii <= s1; ++ii) {
            const double am1 = (ii <= d1) ? A.at(ii - (p - 1) + c, p - 1) : -RF_INF;
            const double b0 = B.at(ii - p + c, p);
            const int sb = ii >= 1 ? s[ii - 1] : 4;
            const int ks = max(ii - 1, 0);
            const double dm = am1_prev + t_match[ks];     // match predecessor (i-1, p)
            const double dx = am1_prev + t_mism[ks];      //   ... mismatching base
            const double is = t_ins[ks];
            const double dl = am1 + t_del[ii];            // delete predecessor (i, p)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const double best = fmax(fmax(sb == b ? dm : dx, prev[b] + is), dl);
                mn[b] = fmin(mn[b], best);
                prev[b] = best;
                acc[b] = fmax(acc[b], best + b0);     // summax, util.jl:40-48
            }
            if (ii <= d1)
                del_acc = fmax(del_acc, am1 + b0);    // seq_score_deletion, model.jl:227-236
            am1_prev = am1;
        }
#pragma unroll
        for (int b = 0; b < 4; ++b)
            out[b] = (mn[b] == -RF_INF || acc[b] == -RF_INF) ? qnan : acc[b];
        out[4] = del_acc;
    } else {
        const int pI = min(p + 1, m);                                // new Ins col's row range
        const int i0 = max(0, pI - c), i1 = min(pI + vb, n);
        // A(p, ii) in band iff ii in rows(p)
        double a0_prev = (i0 - 1 >= s0) ? A.at(i0 - 1 - p + c, p) : -RF_INF;
        for (int ii = i0; ii <= i1; ++ii) {
            const bool in_s = ii <= s1;
            const double a0 = in_s ? A.at(ii - p + c, p) : -RF_INF;
            const double b0 = in_s ? B.at(ii - p + c, p) : -RF_INF;
            const int sb = ii >= 1 ? s[ii - 1] : 4;
            const int ks = max(ii - 1, 0);
            const double dm = a0_prev + t_match[ks];
            const double dx = a0_prev + t_mism[ks];
            const double is = t_ins[ks];
            const double dl = a0 + t_del[ii];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const double best = fmax(fmax(sb == b ? dm : dx, prev[b] + is), dl);
                mn[b] = fmin(mn[b], best);
                prev[b] = best;
                acc[b] = fmax(acc[b], best + b0);
            }
            a0_prev = a0;
        }
#pragma unroll
        for (int b = 0; b < 4; ++b)
            out[b] = (mn[b] == -RF_INF || acc[b] == -RF_INF) ? qnan : acc[b];
    }
}

// One workgroup = 2 waves x 64 lanes: lane l of wave h handles position
// p0 + l, wave 0 the Substitution/Deletion proposals, wave 1 the
// Insertions.  grid.x = work items (group, chunk of SCORE_C positions);
// grid.y = read index in split mode.  Fused mode folds all reads of the
// group in batch order.  lds_elems: doubles the dynamic LDS holds per band.
// INIT (fused launches of rf_score_dense_from): the fold continues from the
// totals already in `dense` instead of starting at 0.0.  A compile-time
// flag: the <false> instance has the code the kernel had without it.
template <bool INIT>
__global__ void __launch_bounds__(128)
k_score(const WorkItem *__restrict__ items, const ScoreGroup *__restrict__ groups,
        const ScoreRead *__restrict__ reads, const uint8_t *__restrict__ bases,
        const double *__restrict__ tabs, const double *__restrict__ bands,
        double *__restrict__ dense, double *__restrict__ split, int split_mode, int lds_elems)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const WorkItem w = items[blockIdx.x];
    const ScoreGroup G = groups[w.group];
    const int lane = threadIdx.x & 63;
    const int half = threadIdx.x >> 6;
    const int p = w.p0 + lane;
    int r0 = G.r0, r1 = G.r1;
    if (split_mode) {
        r0 = G.r0 + blockIdx.y;
        if (r0 >= G.r1)
            return;
        r1 = r0 + 1;
    }
    double tot[5];
#pragma unroll
    for (int k = 0; k < 5; ++k)
        tot[k] = 0.0;
    if (INIT && !split_mode && p <= G.m) {
        // the lane's own slots of the resident table, once, before the reads
        const double *src = dense + G.dense_off + (size_t)p * 9 + (half ? 5 : 0);
#pragma unroll
        for (int k = 0; k < 5; ++k)
            if (k < 4 || half == 0)
                tot[k] = src[k];
    }
    double *sA = smem;
    double *sB = smem + lds_elems;
    const int k0 = 2 * (w.p0 - 1);                    // window's first kappa row
    for (int r = r0; r < r1; ++r) {
        const ScoreRead R = reads[r];
        const double *A = bands + R.A;
        const double *B = bands + R.B;
        const bool stage = (2 * SCORE_C + R.H) * R.P <= lds_elems;
        double sc[5];
        if (stage) {
            // contiguous kappa rows -> LDS, coalesced, 16 loads in flight per lane
            const int kbeg = max(k0, 0);
            const int kend = min(k0 + 2 * SCORE_C + R.H, R.K);
            const int nel = (kend - kbeg) * R.P;
            const int off = (kbeg - k0) * R.P;
            const double *ga = A + (size_t)kbeg * R.P;
            const double *gb = B + (size_t)kbeg * R.P;
            for (int e0 = 0; e0 < nel; e0 += 128 * 8) {
                double ra[8], rb[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int e = e0 + u * 128 + threadIdx.x;
                    if (e < nel) {
                        ra[u] = ga[e];
                        rb[u] = gb[e];
                    }
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int e = e0 + u * 128 + threadIdx.x;
                    if (e < nel) {
                        sA[off + e] = ra[u];
                        sB[off + e] = rb[u];
                    }
                }
            }
            __syncthreads();
            if (p <= G.m) {
                if (half == 0)
                    score_half<0>(p, G.m, R, bases + R.sb, tabs + R.tab, BandWin{sA, k0, R.P},
                                  BandWin{sB, k0, R.P}, sc);
                else
                    score_half<1>(p, G.m, R, bases + R.sb, tabs + R.tab, BandWin{sA, k0, R.P},
                                  BandWin{sB, k0, R.P}, sc);
            }
            __syncthreads();
        } else if (p <= G.m) {
            if (half == 0)
                score_half<0>(p, G.m, R, bases + R.sb, tabs + R.tab, BandWin{A, 0, R.P},
                              BandWin{B, 0, R.P}, sc);
            else
                score_half<1>(p, G.m, R, bases + R.sb, tabs + R.tab, BandWin{A, 0, R.P},
                              BandWin{B, 0, R.P}, sc);
        }
        if (p <= G.m) {
#pragma unroll
            for (int k = 0; k < 5; ++k)
                tot[k] += sc[k];
        }
    }
    if (p > G.m)
        return;
    double *dst = split_mode ? split + G.split_off + ((size_t)blockIdx.y * (G.m + 1) + p) * 9
                             : dense + G.dense_off + (size_t)p * 9;
    if (half == 0) {
#pragma unroll
        for (int k = 0; k < 5; ++k)
            dst[k] = tot[k];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            dst[5 + k] = tot[k];
    }
}

// split mode: ordered fold over reads, one lane per (group position slot).
// INIT (rf_score_dense_from): the fold starts from the slot's value already
// in `dense` -- the first add is init + v[0] -- instead of 0.0.
template <bool INIT>
__global__ void k_reduce(const ScoreGroup *__restrict__ groups, int ngroups,
                         const int64_t *__restrict__ gstart, int64_t total,
                         const double *__restrict__ split, double *__restrict__ dense)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total)
        return;
    // find group (gstart: prefix of (m+1)*9 per group; empty groups skipped)
    int lo = 0, hi = ngroups - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (gstart[mid] <= e)
            lo = mid;
        else
            hi = mid - 1;
    }
    const ScoreGroup G = groups[lo];
    const int64_t local = e - gstart[lo];
    const int64_t stride = (int64_t)(G.m + 1) * 9;
    const double *src = split + G.split_off + local;
    const int nr = G.r1 - G.r0;
    // the left fold in read order (model.jl:389-393); 16 partials are loaded
    // before they are added, so each lane keeps 16 streaming loads in flight
    double acc = INIT ? dense[G.dense_off + local] : 0.0;
    int r = 0;
    for (; r + 16 <= nr; r += 16) {
        double v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u)
            v[u] = __builtin_nontemporal_load(src + (int64_t)(r + u) * stride);
#pragma unroll
        for (int u = 0; u < 16; ++u)
            acc += v[u];
    }
    for (; r < nr; ++r)
        acc += __builtin_nontemporal_load(src + (int64_t)r * stride);
    dense[G.dense_off + local] = acc;
}

// ---------------------------------------------------------------------
// Lean dense scoring (k_score_ws, k_score_segl): one new-column chain per lane
//
// A new column built from A column a (0-based) with base b over the rows of
// column min(a+1, m) serves two proposals (model.jl:250-270):
//   Substitution(a+1, b)  acol = a+1 (1-based) -> summax with B column a+1
//   Insertion(a, b)       acol = a+1 (1-based) -> summax with B column a
// (same A column, same rows, same base: the chains are identical), and the
// lane also folds Deletion(a+1) = max_i A(i, a) + B(i, a+1) (model.jl:227-236).
// So lane a writes slots 5-8 of position a and slots 0-4 of position a+1.
//
// Eligible when every read of the launch has finite match / mismatch / ins /
// del tables (the lean DP condition): then every in-band A and B cell is
// finite, a new column can never hold -Inf, and the reference's "new score
// is invalid" check cannot fire; an empty summax still reports NaN.
//
// Per read, the kappa rows of the work item's columns (one contiguous block
// per band) are staged in LDS with 16-B loads -- the next read's block is
// prefetched into VGPRs while the current one is scored -- and the per-row tables are staged once as {sub A,C,G,T, ins, del} records
// (sub_b = match if the read base is b, else mismatch), so the inner loop is
// LDS reads + FP64 max-plus only.  A read whose window exceeds the LDS budget
// is processed in sub-passes over fewer lanes.  Work items are remapped so
// that consecutive chunks of one group run on the same XCD (shared L2 for the
// H overlapping kappa rows of neighbouring chunks).
// ---------------------------------------------------------------------

// v_max_f64 without the NaN-quieting self-max hipcc adds in front of every
// fmax whose operand is a loop-carried value; the operands here are never NaN
// (finite tables, finite in-band cells, -Inf sentinels), so the result is
// the same FP64 maximum.
__device__ __forceinline__ double vmax(double a, double b)
{
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}


// One row of the four new-column chains of a lane (score_nocodon's update
// over MATCH / INSERT / DELETE, model.jl:262-270, then summax's running max
// against B, util.jl:40-48): best_k = max(aprev + sub_k, prev_k + ins, dl),
// accI_k = max(accI_k, best_k + bI), accS_k = max(accS_k, best_k + bS).
// Issued phase by phase across the four chains, so that no FP64 op waits on
// the op issued right before it (measured: about 1 % faster than chain by
// chain at c5, the same values).
__device__ __forceinline__ void chain_row(double aprev, const double (&sub)[4], double ins, double dl, double bI,
                                          double bS, double (&prev)[4], double (&accI)[4], double (&accS)[4])
{
    double x[4], y[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        x[k] = aprev + sub[k];
        y[k] = prev[k] + ins;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        x[k] = vmax(x[k], y[k]);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        prev[k] = vmax(x[k], dl);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        x[k] = prev[k] + bI;
        y[k] = prev[k] + bS;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        accI[k] = vmax(accI[k], x[k]);
        accS[k] = vmax(accS[k], y[k]);
    }
}

// Geometry of one staged (read, lanes [la0, la1]) window.
struct LeanWin {
    int kw0, shift, n16, win;   // kappa rows from kw0, 16-B chunks per band, doubles per band slot
    int t0, t1;                 // table rows
};

__device__ __forceinline__ LeanWin lean_win(const ScoreRead &R, int m, int la0, int la1)
{
    LeanWin w;
    w.kw0 = 2 * la0;
    const int kw1 = min(2 * (la1 + 1) + R.H, R.K);
    w.shift = (w.kw0 * R.P) & 1;
    w.n16 = (w.shift + (kw1 - w.kw0) * R.P + 1) >> 1;
    w.win = (2 * w.n16 + 1) & ~1;
    w.t0 = max(0, min(la0 + 1, m) - R.c);
    w.t1 = min(min(la1 + 1, m) + R.vb, R.n);
    return w;
}


// Synchronous staging of a window (bands and tables through VGPRs).
template <int Q>
__device__ __forceinline__ void lean_stage(const ScoreRead &R, const LeanWin &w, int tid,
                                           const double *__restrict__ bands, const double *__restrict__ tabs,
                                           const uint8_t *__restrict__ bases, double *sA, double *sB, double *sT)
{
    // plain 16-B loads + ds_write (no LDS-DMA: a global_load_lds anywhere in
    // the kernel makes hipcc wait vmcnt(0) before every LDS read, which would
    // drain the cross-read prefetch at the start of each chain)
    const dvec2 *ga = (const dvec2 *)(bands + R.A + (size_t)w.kw0 * R.P - w.shift);
    const dvec2 *gb = (const dvec2 *)(bands + R.B + (size_t)w.kw0 * R.P - w.shift);
    dvec2 *la = (dvec2 *)sA, *lb = (dvec2 *)sB;
    for (int e0 = 0; e0 < w.n16; e0 += 4 * Q) {
        dvec2 va[4], vb[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = e0 + u * Q + tid;
            if (e < w.n16) {
                va[u] = ga[e];
                vb[u] = gb[e];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = e0 + u * Q + tid;
            if (e < w.n16) {
                la[e] = va[u];
                lb[e] = vb[u];
            }
        }
    }
    const int n = R.n;
    const double *tm = tabs + R.tab;
    const uint8_t *sq = bases + R.sb;
    for (int e = tid; e <= w.t1 - w.t0; e += Q) {
        const int i = w.t0 + e;
        const int ks = max(i - 1, 0);
        lean_row(sT + 6 * e, i >= 1 ? sq[i - 1] : 4, tm[ks], tm[n + ks], tm[2 * (size_t)n + ks],
                 tm[3 * (size_t)n + i]);
    }
}

// One new-column chain (lane column a) over the staged window; accumulates
// into the lane's totals.  Row values are software-pipelined one row ahead.
__device__ __forceinline__ void lean_chain(const ScoreRead &R, const LeanWin &w, int a, int m,
                                           const double *sA, const double *sB, const double *sT,
                                           double tI[4], double tS[4], double &tD)
{
    const int c = R.c, vb = R.vb, P = R.P;
    const int jn = min(a + 1, m);
    const int i0 = max(0, jn - c);
    const int i1 = min(jn + vb, R.n);
    const int ilast = min(i1, a + vb);                  // last row of rows(a)
    int d = i0 - a + c;
    int idx = w.shift + (d + 2 * a - w.kw0) * P + (d >> 1);
    double aprev = (d >= 1 && i0 >= 1) ? sA[idx - P - 1 + (d & 1)] : -RF_INF;
    // B(i, a+1) sits at idx + P - 1 + (d & 1); the last column (a = m) has no
    // Substitution(m+1): it reads B(i, a) there and masks the sum to -Inf
    const bool hasS = a < m;
    const int sofs = hasS ? P - 1 : 0;
    const int sodd = hasS ? 1 : 0;
    const double smask = hasS ? 0.0 : -RF_INF;
    const double *tr = sT + 6 * (i0 - w.t0);
    double prev[4], accI[4], accS[4], dd = -RF_INF;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        prev[k] = -RF_INF;
        accI[k] = -RF_INF;
        accS[k] = -RF_INF;
    }
    double ac = sA[idx], bI = sB[idx], bSr = sB[idx + sofs + (sodd & d)];
    double2 u0 = ((const double2 *)tr)[0], u1 = ((const double2 *)tr)[1], u2 = ((const double2 *)tr)[2];
    for (int i = i0; i <= ilast; ++i) {
        // next row's operands (row ilast + 1 is the peeled row below)
        idx += P + (d & 1);
        ++d;
        tr += 6;
        const double acn = sA[idx], bIn = sB[idx], bSn = sB[idx + sofs + (sodd & d)];
        const double2 v0 = ((const double2 *)tr)[0], v1 = ((const double2 *)tr)[1],
                      v2 = ((const double2 *)tr)[2];
        const double bS = bSr + smask;
        const double sub[4] = {u0.x, u0.y, u1.x, u1.y};
        const double dl = ac + u2.y;
        const double dsum = ac + bS;
        chain_row(aprev, sub, u2.x, dl, bI, bS, prev, accI, accS);
        dd = vmax(dd, dsum);
        aprev = ac;
        ac = acn;
        bI = bIn;
        bSr = bSn;
        u0 = v0;
        u1 = v1;
        u2 = v2;
    }
    if (i1 > ilast) {
        // last row of the new column lies below A/B column a's band (a < m)
        const double sub[4] = {u0.x, u0.y, u1.x, u1.y};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            accS[k] = vmax(accS[k], vmax(aprev + sub[k], prev[k] + u2.x) + bSr);
    }
    const double qnan = __builtin_nan("");
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        tI[k] += accI[k] == -RF_INF ? qnan : accI[k];
        tS[k] += accS[k] == -RF_INF ? qnan : accS[k];
    }
    tD += dd;
}

// lean_chain for an interior lane of a read with row stride exactly PT (the
// c4 strides 11..17): a < m, a >= c and a + 1 + vb <= n, so the chain runs
// diagonals d = 1 .. H-1 of column a and then the peeled row d = H.  Over two
// rows (d odd, then even) the window index advances by 2 PT + 1, so with the
// stride a template constant every LDS operand of a row pair is at an
// immediate offset from one pointer per array: the per-row index arithmetic
// of lean_chain (about 15 of its 51 VALU ops per row) drops out.  Same
// operands, same FP64 ops in the same order: the same values.
#ifndef WS_UNROLL
#define WS_UNROLL 2   // lean_chain_fix row pairs per loop iteration
#endif
template <int PT>
__device__ __forceinline__ void lean_chain_fix(const ScoreRead &R, const LeanWin &w, int a, const double *sA,
                                               const double *sB, const double *sT, double tI[4], double tS[4],
                                               double &tD)
{
    const int idx0 = w.shift + (1 + 2 * a - w.kw0) * PT;   // d = 1
    const double *pa = sA + idx0, *pb = sB + idx0;
    const double *pt = sT + 6 * (a + 1 - R.c - w.t0);
    double aprev = pa[-PT];
    double prev[4], accI[4], accS[4], dd = -RF_INF;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        prev[k] = -RF_INF;
        accI[k] = -RF_INF;
        accS[k] = -RF_INF;
    }
    // one row: A / B at offset o, B(i, a+1) at offset os, table record at t
    auto row = [&](int o, int os, int t) {
        const double ac = pa[o], bI = pb[o], bS = pb[os];
        const double2 u0 = *(const double2 *)(pt + t), u1 = *(const double2 *)(pt + t + 2),
                      u2 = *(const double2 *)(pt + t + 4);
        const double sub[4] = {u0.x, u0.y, u1.x, u1.y};
        const double dl = ac + u2.y;
        const double dsum = ac + bS;
        chain_row(aprev, sub, u2.x, dl, bI, bS, prev, accI, accS);
        dd = vmax(dd, dsum);
        aprev = ac;
    };
    const int nrows = R.c + R.vb;   // i0 = a + 1 - c .. ilast = a + vb
    // WS_UNROLL row pairs per iteration: hipcc issues an iteration's LDS
    // reads at its top and waits for the first ones at once, so each
    // iteration exposes one LDS round trip; two pairs halve that per row
    int u = 0;
    if (WS_UNROLL > 1) {
        for (; u + WS_UNROLL <= (nrows >> 1); u += WS_UNROLL) {
#pragma unroll
            for (int k = 0; k < WS_UNROLL; ++k) {    // pair k: offsets + k (2 PT + 1)
                const int o = k * (2 * PT + 1);
                row(o, o + PT, 12 * k);                   // d odd
                row(o + PT + 1, o + 2 * PT, 12 * k + 6);  // d even
            }
            pa += WS_UNROLL * (2 * PT + 1);
            pb += WS_UNROLL * (2 * PT + 1);
            pt += 12 * WS_UNROLL;
        }
    }
    for (; u < (nrows >> 1); ++u) {
        row(0, PT, 0);                        // d odd
        row(PT + 1, 2 * PT, 6);               // d even
        pa += 2 * PT + 1;
        pb += 2 * PT + 1;
        pt += 12;
    }
    // the last odd row (H even), then the peeled row d = H below column a's band
    const bool odd_tail = nrows & 1;
    if (odd_tail)
        row(0, PT, 0);
    const double bSr = odd_tail ? pb[2 * PT] : pb[PT];
    const double *tp = pt + (odd_tail ? 6 : 0);
    const double2 u0 = *(const double2 *)tp, u1 = *(const double2 *)(tp + 2), u2 = *(const double2 *)(tp + 4);
    const double sub[4] = {u0.x, u0.y, u1.x, u1.y};
#pragma unroll
    for (int k = 0; k < 4; ++k)
        accS[k] = vmax(accS[k], vmax(aprev + sub[k], prev[k] + u2.x) + bSr);
    const double qnan = __builtin_nan("");
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        tI[k] += accI[k] == -RF_INF ? qnan : accI[k];
        tS[k] += accS[k] == -RF_INF ? qnan : accS[k];
    }
    tD += dd;
}

// Whether every chain lane of this wave is interior for read R (lean_chain_fix).
__device__ __forceinline__ bool ws_wave_interior(const ScoreRead &R, int a, int m)
{
    return __all(a < m && a >= R.c && a + 1 + R.vb <= R.n);
}

#ifndef WS_PFIX
#define WS_PFIX 2   // interior waves of reads with stride 11..17 (1) / 11..25 (2) run lean_chain_fix
#endif
// lean_chain, or lean_chain_fix<P> when the wave is interior and P is a c4 stride
__device__ __forceinline__ void lean_chain_any(const ScoreRead &R, const LeanWin &w, int a, int m, const double *sA,
                                               const double *sB, const double *sT, double tI[4], double tS[4],
                                               double &tD)
{
    if (WS_PFIX && ws_wave_interior(R, a, m)) {
        switch (R.P) {
        case 11: lean_chain_fix<11>(R, w, a, sA, sB, sT, tI, tS, tD); return;
        case 13: lean_chain_fix<13>(R, w, a, sA, sB, sT, tI, tS, tD); return;
        case 15: lean_chain_fix<15>(R, w, a, sA, sB, sT, tI, tS, tD); return;
        case 17: lean_chain_fix<17>(R, w, a, sA, sB, sT, tI, tS, tD); return;
#if WS_PFIX > 1
        // doubled bands (bw 18 after smart_forward_moves!, H 37..51)
        case 19: lean_chain_fix<19>(R, w, a, sA, sB, sT, tI, tS, tD); return;
        case 21: lean_chain_fix<21>(R, w, a, sA, sB, sT, tI, tS, tD); return;
        case 23: lean_chain_fix<23>(R, w, a, sA, sB, sT, tI, tS, tD); return;
        case 25: lean_chain_fix<25>(R, w, a, sA, sB, sT, tI, tS, tD); return;
#endif
        default: break;
        }
    }
    lean_chain(R, w, a, m, sA, sB, sT, tI, tS, tD);
}

__device__ __forceinline__ void wg_barrier()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// ---------------------------------------------------------------------
// k_score_ws: the lean scorer with wave specialization (the default)
//
// 512 threads: waves 0-3 are the chain waves (256 chain columns per work
// item, totals in their VGPRs); waves 4-7 are loader waves that hold the
// NEXT read's window and table rows in their own VGPRs while the chain waves
// score the current read from LDS, then write it to LDS between two
// barriers.  The two roles run separate loops (so the loaders' registers
// never constrain the chains) that meet at the same s_barrier sequence:
// two barriers per read, or per sub-pass of a read too wide for the
// prefetch (staged synchronously by the loaders).
// ---------------------------------------------------------------------


#ifndef WS_NPF
#define WS_NPF 19
#endif
#ifndef WS_CODES
#define WS_CODES 1   // loaders read row-coded reads' tables through the code dictionary
#endif

// INIT (fused launches of rf_score_dense_from): the chain waves' totals start
// from the values already in `dense` instead of 0.0 (a compile-time flag).
template <int NPF, int Q, bool INIT = false>
__global__ void __launch_bounds__(2 * Q)
k_score_ws(const WorkItem *__restrict__ items, const ScoreGroup *__restrict__ groups,
           const ScoreRead *__restrict__ reads, const uint8_t *__restrict__ bases,
           const double *__restrict__ tabs, const double *__restrict__ bands,
           double *__restrict__ dense, double *__restrict__ split, int split_mode, int lds_elems,
           const double *__restrict__ lut, int rchunk)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int nb = gridDim.x, b = blockIdx.x;
    const int xq = nb >> 3, xr = nb & 7, x = b & 7;
    const int item = x * xq + min(x, xr) + (b >> 3);
    const WorkItem wi = items[item];
    const ScoreGroup G = groups[wi.group];
    const int m = G.m;
    const int a0 = wi.p0;
    const int la1f = min(a0 + Q - 1, m);
    int r0 = G.r0, r1 = G.r1;
    if (split_mode & 1) {
        // split mode: rchunk consecutive reads per workgroup (round 5: one
        // read per workgroup left a small cluster's launch -- configs[2]'s
        // 1,000 reads x 11 items -- without the loaders' prefetch overlap),
        // each read's own partial written, k_reduce folds them in order
        r0 = G.r0 + blockIdx.y * rchunk;
        if (r0 >= G.r1)
            return;
        r1 = min(r0 + rchunk, G.r1);
    }
    // same decision in both roles (block-uniform)
    auto fast = [&](const ScoreRead &R, const LeanWin &w) {
        return lean_need(Q, R.H, R.P) <= lds_elems && w.n16 <= NPF * Q && w.t1 - w.t0 < 2 * Q;
    };
    auto sub_L = [&](const ScoreRead &R) {
        int L = Q;
        while (L > 1 && lean_need(L, R.H, R.P) > lds_elems)
            L >>= 1;
        return L;
    };
    // Work units: a read whose whole window fits LDS and the loaders'
    // registers is one unit of Q columns; a wider one is split into sub-
    // windows of L columns that fit LDS (sub_L).  Units stream through the
    // same register prefetch as whole reads whenever a unit's window fits the
    // loaders' registers (doubled bands, P 19..25, at L = Q / 2), otherwise
    // they are staged synchronously.  Both roles walk the same sequence.
    struct Unit {
        int r, s0, L;
    };
    auto unit_first = [&](int r) {
        Unit u{r, 0, Q};
        if (r < r1) {
            const ScoreRead R = reads[r];
            if (!fast(R, lean_win(R, m, a0, la1f)))
                u.L = sub_L(R);
        }
        return u;
    };
    auto unit_next = [&](const Unit &u) {
        const int s0 = u.s0 + u.L;
        if (s0 < Q && a0 + s0 <= m)
            return Unit{u.r, s0, u.L};
        return unit_first(u.r + 1);
    };
    auto unit_win = [&](const ScoreRead &R, const Unit &u) {
        return lean_win(R, m, a0 + u.s0, min(a0 + u.s0 + u.L - 1, m));
    };
    auto unit_pf = [&](const ScoreRead &R, const Unit &u, const LeanWin &w) {   // register-prefetched
        return lean_need(u.L, R.H, R.P) <= lds_elems && w.n16 <= NPF * Q && w.t1 - w.t0 < 2 * Q;
    };
    if (threadIdx.x >= Q) {
        // =========================== loader waves ===========================
        const int lt = threadIdx.x - Q;
        dvec2 pa[NPF], pb[NPF];
        double pm[2], px[2], pn[2], pd[2];
        int ps[2];
        auto issue = [&](const ScoreRead &R2, const LeanWin &w2) {
            const double *tm = tabs + R2.tab;
            const int n2 = R2.n;
            // Row-coded reads (SR_CODED): one 8-B code record per row from HBM
            // (issued first, so that the wait for them leaves the band loads in
            // flight) and the values from the context's L2-resident dictionary
            // -- the same doubles as the tables (rf_set_sequences), 8 instead of
            // 33 B per row.  Record of position ks: triple code | del[ks] code
            // << 16 | del[ks+1] code << 32 | base << 48.
            const bool coded = (R2.flags & SR_CODED) && lut != nullptr;
            uint64_t rc[2];
            if (coded) {
                const uint64_t *rec = (const uint64_t *)(tm + row_code_off(n2, 0, 0));
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const int i = min(w2.t0 + lt + k * Q, w2.t1);
                    rc[k] = rec[max(i - 1, 0)];
                }
            }
            const dvec2 *ga = (const dvec2 *)(bands + R2.A + (size_t)w2.kw0 * R2.P - w2.shift);
            const dvec2 *gb = (const dvec2 *)(bands + R2.B + (size_t)w2.kw0 * R2.P - w2.shift);
#pragma unroll
            for (int u = 0; u < NPF; ++u) {
                // predicated: chunks past the window are neither loaded nor
                // committed (the commit's `e < n16` test)
                const int e = u * Q + lt;
                if (e < w2.n16) {
                    pa[u] = ga[e];
                    pb[u] = gb[e];
                }
            }
            if (coded) {
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const int i = min(w2.t0 + lt + k * Q, w2.t1);
                    const double *l3 = lut + 4 * (size_t)(rc[k] & 0xffff);
                    pm[k] = l3[0];
                    px[k] = l3[1];
                    pn[k] = l3[2];
                    pd[k] = lut[4 * (size_t)RF_CODES + ((rc[k] >> (i == 0 ? 16 : 32)) & 0xffff)];
                    ps[k] = (int)((rc[k] >> 48) & 0xff);
                }
            } else {
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const int i = min(w2.t0 + lt + k * Q, w2.t1);
                    const int ks = max(i - 1, 0);
                    pm[k] = tm[ks];
                    px[k] = tm[n2 + ks];
                    pn[k] = tm[2 * (size_t)n2 + ks];
                    pd[k] = tm[3 * (size_t)n2 + i];
                    ps[k] = bases[R2.sb + ks];
                }
            }
        };
        bool held = false;   // the registers hold the unit
        for (Unit u = unit_first(r0); u.r < r1;) {
            const ScoreRead R = reads[u.r];
            const LeanWin w = unit_win(R, u);
            const Unit nx = unit_next(u);
            if (unit_pf(R, u, w)) {
                if (!held)
                    issue(R, w);
                dvec2 *sA = (dvec2 *)smem;
                dvec2 *sB = (dvec2 *)(smem + w.win);
                double *sT = smem + 2 * w.win;
#pragma unroll
                for (int k = 0; k < NPF; ++k) {
                    const int e = k * Q + lt;
                    if (e < w.n16) {
                        sA[e] = pa[k];
                        sB[e] = pb[k];
                    }
                }
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const int e = lt + k * Q;
                    const int i = w.t0 + e;
                    if (i <= w.t1)
                        lean_row(sT + 6 * e, i >= 1 ? ps[k] : 4, pm[k], px[k], pn[k], pd[k]);
                }
                wg_barrier();                        // unit ready
                held = false;
                if (nx.r < r1) {
                    const ScoreRead R2 = reads[nx.r];
                    const LeanWin w2 = unit_win(R2, nx);
                    if (unit_pf(R2, nx, w2)) {
                        issue(R2, w2);
                        held = true;
                    }
                }
                wg_barrier();                        // chains of the unit done
            } else {
                lean_stage<Q>(R, w, lt, bands, tabs, bases, smem, smem + w.win, smem + 2 * w.win);
                wg_barrier();
                wg_barrier();
                held = false;
            }
            u = nx;
        }
        return;
    }
    // ============================ chain waves =============================
    const int tid = threadIdx.x;
    const int a = a0 + tid;
    double tI[4], tS[4], tD = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        tI[k] = 0.0;
        tS[k] = 0.0;
    }
    if (INIT && !(split_mode & 1) && a <= m) {
        // the slots this lane emits (5-8 of position a, 0-4 of a + 1): one
        // run of 9 doubles per lane, consecutive across the wave, read once
        // before the first read's barrier
        const double *src = dense + G.dense_off + (size_t)a * 9;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            tI[k] = src[5 + k];
        if (a < m) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                tS[k] = src[9 + k];
            tD = src[13];
        }
    }
    const double qnan = __builtin_nan("");
    // one position's 9 totals (fused: the group's fold; split: read r's
    // partial, 0.0 + its own sums, and the running values restart at 0.0)
    auto emit = [&](double *base) {
        double *dst = base + (size_t)a * 9;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            dst[5 + k] = tI[k];
        if (a < m) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                dst[9 + k] = tS[k];
            dst[13] = tD;
        }
        if (a == 0) {
#pragma unroll
            for (int k = 0; k < 5; ++k)
                dst[k] = qnan;
        }
    };
    for (Unit u = unit_first(r0); u.r < r1;) {
        const ScoreRead R = reads[u.r];
        const LeanWin w = unit_win(R, u);
        wg_barrier();                                // unit ready
        if (tid >= u.s0 && tid < u.s0 + u.L && a <= m)
            lean_chain_any(R, w, a, m, smem, smem + w.win, smem + 2 * w.win, tI, tS, tD);
        wg_barrier();                                // chains of the unit done
        const Unit nx = unit_next(u);
        if ((split_mode & 1) && nx.r != u.r && a <= m) {
            emit(split + G.split_off + (size_t)(u.r - G.r0) * (m + 1) * 9);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                tI[k] = 0.0;
                tS[k] = 0.0;
            }
            tD = 0.0;
        }
        u = nx;
    }
    if (a > m || (split_mode & 1))
        return;
    emit(dense + G.dense_off);
}

// ---------------------------------------------------------------------
// k_score_segl: the wide-band scorer over line-aligned band rows (default)
//
// Same chains, operands, order and FP64 max-plus as k_score_ws's lean_chain
// (identical results).  Segments are 32 band diagonals [D, D+32) with D a
// multiple of 32, so a kappa row's piece of a segment is elements
// [D/2, D/2 + 16): exactly one 128-B line when the band's rows are padded to
// whole lines (band_stride, P % 16 == 0; band regions are 256-B aligned) --
// no line is shared by two segments, so each is fetched once.  Bands with the
// odd stride (H below RF_OPT_BAND_PAD) take 9 pair-aligned 16-B chunks per
// row instead.  The wave's 65 columns [a0, a0+64] touch kappa rows
// [D + 2*a0, D + 2*a0 + 160).
//
// LDS holds the segment transposed: slot (d - D + 1) * 65 + (a - a0) for
// d in [D-1, D+32) (row 0 is the previous segment's last diagonal), so lane
// a's operands at step d -- A(d, a), B(d, a), B(d-1, a+1) -- are one
// consecutive 512-B run per wave-instruction at an immediate offset, and the
// table records of read row i = a - c + d (three 16-B arrays) likewise.
// The next segment's lines are loaded into registers while this one is
// scored.
// ---------------------------------------------------------------------
#ifndef SEGL_UNROLL
#define SEGL_UNROLL 32
#endif
// an interior wave's last segment runs the unrolled steps over rows staged as
// -Inf past the peel row when it holds at least this many rows (fewer: the
// generic loop, which costs more per step but runs only the real rows)
#ifndef SEGL_MASKED_MIN
#define SEGL_MASKED_MIN 20
#endif
#define SEGL_FENCE() __builtin_amdgcn_sched_barrier(0)
// A kappa row's piece of a segment is one 128-B line.  (Half-line segments
// of 16 diagonals -- 55 % of the LDS, two waves per SIMD -- were bit-exact but
// slower at c5: 30.6 ms at one wave per SIMD, 40.6 ms at two with spills,
// against 27.9 ms; profiles/r02_exp_segl16.json.)
template <int S_>
struct SeglGeo {
    static_assert(S_ == 32, "segments of 32 diagonals");
    static constexpr int S = S_;        // diagonals per segment
    static constexpr int LS = 65;       // LDS row: columns a0 .. a0+64
    static constexpr int NRW = S + 1;   // LDS rows: d = D-1 .. D+S-1
    static constexpr int NROW = S + 128;   // kappa rows per segment
    static constexpr int CPR = S / 4;      // 16-B chunks of a row piece (S/2 doubles), aligned rows
    static constexpr int RPI = 64 / CPR;   // rows per wave-wide load
    static constexpr int NUA = NROW * CPR / 64;          // chunks per lane and band, aligned rows
    static constexpr int NC = CPR + 1;                   // pair-aligned chunks per row, odd stride
    static constexpr int NUG = (NROW * NC + 63) / 64;
    static constexpr int NT = S + 65;   // table rows: i - ib in [0, S + 65)
};

#ifndef SEGL_WPE
#define SEGL_WPE 1
#endif
// INIT (fused launches of rf_score_dense_from): the lane's totals start from
// the values already in `dense` instead of 0.0 (a compile-time flag).
template <int SEGS, bool INIT = false>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SEGL_WPE)))
k_score_segl(const WorkItem *__restrict__ items, const ScoreGroup *__restrict__ groups,
             const ScoreRead *__restrict__ reads, const uint8_t *__restrict__ bases,
             const double *__restrict__ tabs, const double *__restrict__ bands,
             double *__restrict__ dense, double *__restrict__ split, int split_mode, int rchunk)
{
    using Gm = SeglGeo<SEGS>;
    constexpr int S = Gm::S, LS = Gm::LS, NUA = Gm::NUA, NUG = Gm::NUG, NT = Gm::NT;
    constexpr int CPR = Gm::CPR, RPI = Gm::RPI, NC = Gm::NC;

    constexpr int SL = (Gm::NRW * LS + 1) & ~1;   // doubles per band slice (16-B multiple)
    __shared__ __attribute__((aligned(16))) double sA[SL];
    __shared__ __attribute__((aligned(16))) double sB[SL];
    __shared__ __attribute__((aligned(16))) dvec2 sT0[NT], sT1[NT], sT2[NT];
    const int nx = gridDim.x;
    const int lin = blockIdx.x + nx * blockIdx.y, ncell = nx * gridDim.y;
    const int xq = ncell >> 3, xr = ncell & 7, x = lin & 7;
    const int cell = x * xq + min(x, xr) + (lin >> 3);
    const int bx = cell % nx, by = cell / nx;
    const WorkItem wi = items[bx];
    const ScoreGroup G = groups[wi.group];
    const int m = G.m;
    const int a0 = wi.p0;
    const int tid = threadIdx.x;
    const int a = a0 + tid;
    const bool active = a <= m;
    int r0 = G.r0, r1 = G.r1;
    if (split_mode & 1) {
        r0 = G.r0 + by * rchunk;
        if (r0 >= G.r1)
            return;
        r1 = min(r0 + rchunk, G.r1);
    }
    const bool hasS = a < m;
    const double smask = hasS ? 0.0 : -RF_INF;
    const bool wave_s = __all(hasS);   // every lane has a Substitution column
    double tI[4], tS[4], tD = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        tI[k] = 0.0;
        tS[k] = 0.0;
    }
    if (INIT && !(split_mode & 1) && active) {
        // the slots this lane writes at the end (5-8 of position a, 0-4 of
        // a + 1): 9 doubles per lane, consecutive across the wave, read once
        const double *src = dense + G.dense_off + (size_t)a * 9;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            tI[k] = src[5 + k];
        if (hasS) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                tS[k] = src[9 + k];
            tD = src[13];
        }
    }
    const bool all_act = __all(active) && wave_s;
    // aligned-row loader lane roles: row r8 + RPI j, 16-B chunk cc8 of the row piece
    const int r8 = tid / CPR, cc8 = tid % CPR, p8 = r8 & 1;
    // per-read geometry: wave-uniform fields plus the lane's diagonal range
    struct RG {
        const double *gA;
        const double *tm;
        const uint8_t *sq;
        int64_t dB;
        int c, P, K, n;
        int dfirst, dlast;           // this lane's chain rows as band diagonals
        bool peel;
        int dlo, dhi, dfmax, dlmin;  // wave-wide
        bool uni;                    // every lane active with the same [dfirst, dlast] and peel
    };
    auto setup = [&](int r, RG &g) {
        const ScoreRead R = reads[r];
        g.c = R.c;
        g.P = R.P;
        g.K = R.K;
        g.n = R.n;
        g.gA = bands + R.A;
        g.dB = R.B - R.A;
        g.tm = tabs + R.tab;
        g.sq = bases + R.sb;
        const int jn = min(a + 1, m);
        const int i0 = max(0, jn - g.c);
        const int i1 = min(jn + R.vb, g.n);
        const int ilast = min(i1, a + R.vb);
        g.dfirst = i0 - a + g.c;
        g.dlast = ilast - a + g.c;
        g.peel = i1 > ilast;
        int dlo = active ? g.dfirst : INT_MAX, dhi = active ? g.dlast + (g.peel ? 1 : 0) : -1;
        int dfmax = active ? g.dfirst : INT_MAX, dlmin = active ? g.dlast : -1;
        for (int off = 32; off >= 1; off >>= 1) {
            dlo = min(dlo, __shfl_xor(dlo, off));
            dhi = max(dhi, __shfl_xor(dhi, off));
            dfmax = max(dfmax, __shfl_xor(dfmax, off));
            dlmin = min(dlmin, __shfl_xor(dlmin, off));
        }
        g.dlo = __builtin_amdgcn_readfirstlane(dlo);
        g.dhi = __builtin_amdgcn_readfirstlane(dhi);
        g.dfmax = __builtin_amdgcn_readfirstlane(dfmax);
        g.dlmin = __builtin_amdgcn_readfirstlane(dlmin);
        // interior waves: every lane has the same chain rows [dfirst, dlast]
        // and a peel row dlast + 1 (uniform), so the first and last segments
        // of the read can run the unrolled steps too (see chains)
        g.uni = all_act && __all(g.dfirst == g.dlo && g.dlast == g.dlmin && g.peel);
    };
    // one segment's registers: its band lines, table rows and (a read's
    // first segment) LDS row 0
    struct SegSet {
        dvec2 ra[NUA], rb[NUA];
        double tmt[2], tmm[2], tin[2], tdl[2];
        int tsb[2];
        double z0a, z0b, z1a, z1b;
    };
    // loads of segment D of read g (registers only)
    auto load_seg = [&](SegSet &X, const RG &g, int D, bool first) {
        const int kb = D + 2 * a0, eh = D >> 1;
        if ((g.P & 15) == 0) {
#pragma unroll
            for (int j = 0; j < NUA; ++j) {
                const int kap = min(kb + r8 + RPI * j, g.K - 1);
                const int64_t o = (int64_t)kap * g.P + eh + 2 * cc8;
                X.ra[j] = *(const dvec2 *)(g.gA + o);
                X.rb[j] = *(const dvec2 *)(g.gA + g.dB + o);
            }
        }
        if (first && D > 0) {
            // diagonal D-1 of columns a0 .. a0+64 (the previous segment's last row)
            const int kap = min(D - 1 + 2 * a, g.K - 1);
            const int64_t o = (int64_t)kap * g.P + ((D - 1) >> 1);
            X.z0a = g.gA[o];
            X.z0b = g.gA[g.dB + o];
            if (tid == 0) {
                const int kap1 = min(D - 1 + 2 * (a0 + 64), g.K - 1);
                const int64_t o1 = (int64_t)kap1 * g.P + ((D - 1) >> 1);
                X.z1a = g.gA[o1];
                X.z1b = g.gA[g.dB + o1];
            }
        }
        const int ib = a0 - g.c + D;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = min(max(ib + tid + 64 * u, 0), g.n);
            const int ks = max(i - 1, 0);
            X.tsb[u] = g.sq[ks];   // read row 0 (the gap) is selected at the store
            X.tmt[u] = g.tm[ks];
            X.tmm[u] = g.tm[g.n + ks];
            X.tin[u] = g.tm[2 * (size_t)g.n + ks];
            X.tdl[u] = g.tm[3 * (size_t)g.n + i];
        }
    };
    auto store_seg = [&](const SegSet &X, const RG &g, int D) {
        if ((g.P & 15) == 0) {
            // an interior wave's last segment: rows past the peel row (d >
            // dlast + 1 in A, d > dlast in B beyond column a) read -Inf, so the
            // unrolled steps past the chain's end leave it unchanged (chains)
            const int dm = (g.uni && D > 0 && g.dlmin + 1 < D + S && g.dlmin + 1 - D >= SEGL_MASKED_MIN)
                               ? g.dlmin + 1 - D : INT_MAX;
#pragma unroll
            for (int j = 0; j < NUA; ++j) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int ddl = 4 * cc8 + 2 * h + p8;       // d - D
                    const int col = (r8 + RPI * j - ddl) >> 1;  // a - a0
                    const double v = h ? X.ra[j].y : X.ra[j].x, w = h ? X.rb[j].y : X.rb[j].x;
                    const int l = (ddl + 1) * LS + col;
                    // rows S..127 always land in [0, 64]; the parallelogram's
                    // first / last S rows hold cells of the neighbouring items
                    if ((j * RPI >= S && (j + 1) * RPI <= 128) || (col >= 0 && col <= 64)) {
                        sA[l] = v;
                        sB[l] = w;
                    }
                }
            }
            if (dm != INT_MAX) {
                // LDS rows dm + 1 .. S (diagonals D + dm ..) of both bands: -Inf
                for (int e = tid; e < (S - dm) * LS; e += 64) {
                    const int l = (dm + 1) * LS + e;
                    sA[l] = -RF_INF;
                    sB[l] = -RF_INF;
                }
            }
        } else {
            // odd-stride rows (narrow bands in a wide launch): NC pair-aligned
            // chunks per row, loaded here in groups of 4 (not prefetched)
            const int kb = D + 2 * a0, eh = D >> 1;
#pragma unroll 1
            for (int j0 = 0; j0 < NUG; j0 += 4) {
                dvec2 ga[4], gb[4];
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const int t = min(tid + 64 * (j0 + jj), Gm::NROW * NC - 1);
                    const int rr = t / NC, cc = t - NC * rr;
                    const int kap = min(kb + rr, g.K - 1);
                    const int o = ((kap * g.P + eh) & ~1) + 2 * cc;
                    ga[jj] = *(const dvec2 *)(g.gA + o);
                    gb[jj] = *(const dvec2 *)(g.gA + g.dB + o);
                }
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const int t = tid + 64 * (j0 + jj);
                    const int rr = t / NC, cc = t - NC * rr;
                    const int sh = (kb + rr + eh) & 1;   // P odd
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int xl = 2 * cc + h - sh;
                        const int ddl = 2 * xl + (rr & 1);
                        const int col = (rr - ddl) >> 1;
                        if (t < Gm::NROW * NC && xl >= 0 && xl < S / 2 && col >= 0 && col <= 64) {
                            const int l = (ddl + 1) * LS + col;
                            sA[l] = h ? ga[jj].y : ga[jj].x;
                            sB[l] = h ? gb[jj].y : gb[jj].x;
                        }
                    }
                }
            }
            // nothing of this path stays in flight: hipcc's wait analysis
            // merges paths, and a load it saw pending here would make it
            // drain the next segment's prefetch before the chains
            __builtin_amdgcn_s_waitcnt(0);
        }
        const int ib = a0 - g.c + D;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int t = tid + 64 * u;
            if (t < NT) {
                const int sb = ib + t >= 1 ? X.tsb[u] : 4;
                const double mt = X.tmt[u], mm = X.tmm[u];
                sT0[t] = dvec2{sb == 0 ? mt : mm, sb == 1 ? mt : mm};
                sT1[t] = dvec2{sb == 2 ? mt : mm, sb == 3 ? mt : mm};
                sT2[t] = dvec2{X.tin[u], X.tdl[u]};
            }
        }
    };
    // a wave with no column (every a > m) writes nothing; any other wave has
    // rows in every read (each band column holds at least one row)
    if (!__any(active))
        return;
    double prev[4], accI[4], accS[4], dd = -RF_INF;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        prev[k] = -RF_INF;
        accI[k] = -RF_INF;
        accS[k] = -RF_INF;
    }
    // the chains of segment D of read g (operands from LDS)
    auto chains = [&](const RG &g, int D) {
        const int c = g.c, dfirst = g.dfirst, dlast = g.dlast;
        const int dfmax = g.dfmax, dlmin = g.dlmin;
        const bool peel = g.peel;
        if (active) {
            const int lo = max(D, dfirst), hi = min(D + S - 1, dlast);
            const double a0v = sA[min(max(lo - D, 0), S) * LS + tid];   // unconditional read, then select
            double aprev = (lo <= hi && lo >= 1 && a - c + lo >= 1) ? a0v : -RF_INF;
            const double *pA = sA + LS + tid;    // row 1 = diagonal D
            const double *pB = sB + LS + tid;
            const double *pS = sB + tid + 1;     // B(d-1, a+1): row d - D, column + 1
            const dvec2 *q0 = sT0 + tid, *q1 = sT1 + tid, *q2 = sT2 + tid;
            // operands of step s; the next step's are read from LDS while this
            // one is scored (software pipeline: a read right before its use
            // exposes the LDS latency on every step at one wave per SIMD)
            struct Ops {
                double ac, bI, bs;
                dvec2 u0, u1, u2;
            };
            auto ld = [&](int s) {
                Ops o;
                o.ac = pA[s * LS];
                o.bI = pB[s * LS];
                o.bs = pS[s * LS];   // in range for every lane
                o.u0 = q0[s];
                o.u1 = q1[s];
                o.u2 = q2[s];
                return o;
            };
            // ALLS: every lane has a Substitution column (hasS; smask = 0)
            auto step = [&](const Ops &o, auto alls) {
                const double bS = ((decltype(alls)::value || hasS) ? o.bs : o.bI) + smask;
                const double sub[4] = {o.u0.x, o.u0.y, o.u1.x, o.u1.y};
                const double dl = o.ac + o.u2.y;
                const double dsum = o.ac + bS;
                chain_row(aprev, sub, o.u2.x, dl, o.bI, bS, prev, accI, accS);
                dd = vmax(dd, dsum);
                aprev = o.ac;
            };
            // unrolled steps s0 .. shi (wave-uniform) of the segment; s0 = 0 or 1
            // the unrolled steps 0 .. S-1 (one copy of the body: instruction
            // cache); skip0 -- a read's first segment in an interior wave,
            // whose chains start at diagonal 1 -- only takes row 0 as the next
            // step's MATCH predecessor (a scalar branch on the first step)
            auto run = [&](bool skip0) {
                Ops cur = ld(0);
#pragma unroll SEGL_UNROLL
                for (int s = 0; s < S; ++s) {
                    const Ops nxt = ld(s + 1 < S ? s + 1 : s);
                    // keep the reads ahead of this step's chain (hipcc's scheduler
                    // otherwise sinks them next to their use); the arithmetic may
                    // still move across (a full sched_barrier costs hazard nops)
                    SEGL_FENCE();
                    if (s == 0 && skip0)
                        aprev = a - c >= 0 ? cur.ac : -RF_INF;   // diagonal 0: read row a - c
                    else
                        step(cur, std::true_type{});
                    cur = nxt;
                }
            };
            // every lane scores all 32 diagonals (no peel inside: dlast >= D+31);
            // all_act includes wave_s, so the bS select is the identity
            const bool full = all_act && dfmax <= D && dlmin >= D + S - 1;
            // interior wave, first segment of the read (round 4): every lane's
            // chain covers diagonals 1 .. S-1 of it
            const bool first_u = g.uni && D == 0 && dfirst == 1 && dlast + 1 >= S && (g.P & 15) == 0;
            // interior wave, last segment with at least SEGL_MASKED_MIN rows
            // (round 4): the rows past the peel row were stored as -Inf
            // (store_seg), so all S unrolled steps give the chain's rows up to
            // dlast, then the peel row dlast + 1 exactly as below (max(x, -Inf)
            // = x; B(dlast, a + 1) is the peel's operand), and leave the state
            // unchanged afterwards
            const bool last_u = g.uni && D > 0 && dlast + 1 < D + S && dlast + 1 - D >= SEGL_MASKED_MIN &&
                                (g.P & 15) == 0;
            if (full || first_u || last_u) {
                run(__builtin_amdgcn_readfirstlane((int)first_u) != 0);   // one call site: one body
            } else {
                const int slo = max(lo - D, 0), shi = hi - D;
                if (slo <= shi) {
                    Ops cur = ld(slo);
                    for (int s = slo; s <= shi; ++s) {
                        const Ops nxt = ld(s < shi ? s + 1 : s);
                        SEGL_FENCE();
                        step(cur, std::false_type{});
                        cur = nxt;
                    }
                }
                const int dp = dlast + 1;
                if (peel && dp >= D && dp < D + S) {
                    // last row of the new column lies below A/B column a's band (a < m)
                    const int sp = dp - D;
                    const double ap = sA[sp * LS + tid];
                    const double bSr = sB[sp * LS + tid + 1];
                    const dvec2 u0 = sT0[tid + sp], u1 = sT1[tid + sp], u2 = sT2[tid + sp];
                    const double sub[4] = {u0.x, u0.y, u1.x, u1.y};
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        accS[k] = vmax(accS[k], vmax(ap + sub[k], prev[k] + u2.x) + bSr);
                }
            }
        }
    };
    // read r's totals (after its last segment) and fresh chain state
    auto finish = [&](int r) {
        if (active) {
            const double qnan = __builtin_nan("");
            if (split_mode & 1) {
                double *dst = split + G.split_off + ((size_t)(r - G.r0) * (m + 1) + a) * 9;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    dst[5 + k] = accI[k] == -RF_INF ? qnan : accI[k];
                if (a < m) {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        dst[9 + k] = accS[k] == -RF_INF ? qnan : accS[k];
                    dst[13] = dd;
                }
                if (a == 0) {
#pragma unroll
                    for (int k = 0; k < 5; ++k)
                        dst[k] = qnan;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    tI[k] += accI[k] == -RF_INF ? qnan : accI[k];
                    tS[k] += accS[k] == -RF_INF ? qnan : accS[k];
                }
                tD += dd;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            prev[k] = -RF_INF;
            accI[k] = -RF_INF;
            accS[k] = -RF_INF;
        }
        dd = -RF_INF;
    };
    // Reads and their segments as one stream: the register prefetch always
    // holds the next segment(s) -- this read's next, or the next read's
    // first -- so no read starts on an exposed load.
    struct Pos {
        int r, D;
        RG g;
    };
    auto first_of = [&](const RG &g) { return g.dlo & ~(S - 1); };
    auto adv = [&](Pos &p) {
        if (p.D + S > p.g.dhi) {
            ++p.r;
            if (p.r < r1) {
                setup(p.r, p.g);
                p.D = first_of(p.g);
            }
        } else {
            p.D += S;
        }
    };
    // one segment: X holds its loads; afterwards X holds the next segment's
    auto step = [&](SegSet &X, Pos &cur) {
        const int D = cur.D;
        const bool first = D == first_of(cur.g);
        wave_sync();   // previous segment's chains are done with LDS
        // LDS row 0 = diagonal D-1: the previous segment's row 32, or prefetched
        if (first) {
            if (D > 0) {
                sA[tid] = X.z0a;
                sB[tid] = X.z0b;
                if (tid == 0) {
                    sA[64] = X.z1a;
                    sB[64] = X.z1b;
                }
            }
        } else {
            const double va = sA[S * LS + tid], vbv = sB[S * LS + tid];
            const double va6 = sA[S * LS + 64], vb6 = sB[S * LS + 64];
            sA[tid] = va;
            sB[tid] = vbv;
            if (tid == 0) {
                sA[64] = va6;
                sB[64] = vb6;
            }
        }
        store_seg(X, cur.g, D);
        wave_sync();
        Pos ahead = cur;
        if (ahead.r < r1)
            adv(ahead);
        if (ahead.r < r1)
            load_seg(X, ahead.g, ahead.D, ahead.D == first_of(ahead.g));
        chains(cur.g, D);
        if (D + S > cur.g.dhi)
            finish(cur.r);
        cur = ahead;
    };
    Pos cur;
    cur.r = r0;
    if (r0 < r1) {
        setup(r0, cur.g);
        cur.D = first_of(cur.g);
    }
    SegSet X0;
    if (r0 < r1)
        load_seg(X0, cur.g, cur.D, true);
    while (cur.r < r1)
        step(X0, cur);
    if (!active || (split_mode & 1))
        return;
    const double qnan = __builtin_nan("");
    double *dst = dense + G.dense_off + (size_t)a * 9;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        dst[5 + k] = tI[k];
    if (a < m) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            dst[9 + k] = tS[k];
        dst[13] = tD;
    }
    if (a == 0) {
#pragma unroll
        for (int k = 0; k < 5; ++k)
            dst[k] = qnan;
    }
}

// ---------------------------------------------------------------------
// k_codon: codon-move scoring, one lane per proposal (model.jl:302-383)
// ---------------------------------------------------------------------

struct Geo {
    int n, m, bw, H, P, c;
    __device__ __forceinline__ bool inband(int ii, int jj) const
    {
        // 0-based cell (ii, jj) of an (n+1) x (m+1) band (bandedarrays.jl:151-157)
        if (ii < 0 || jj < 0 || ii > n || jj > m)
            return false;
        const int d = ii - jj + c;
        return d >= 0 && d < H;
    }
    __device__ __forceinline__ double get(const double *band, int ii, int jj) const
    {
        return band[bidx(ii - jj + c, jj, P)];
    }
    __device__ __forceinline__ void rows(int jj, int &a, int &b) const
    {
        a = max(0, jj - max(m - n, 0) - bw);
        b = min(jj + max(n - m, 0) + bw, n);
    }
};

// align.jl:50-112 with newcols / acol (1-based i, j like the reference)
__device__ bool update_nc(const Geo &g, const double *A, const double *nc, int ncld, int acol,
                          int i, int j, int s_base, int t_base, const double *tb, int ncins,
                          int ncdel, double &out)
{
    const int n = g.n, ncols = g.m + 1;
    const int seq_i = max(i - 1, 1);
    const int del_i = i;
    const double ms = (s_base == t_base) ? tb[seq_i - 1] : tb[n + seq_i - 1];
    const double is = tb[2 * n + seq_i - 1];
    const double ds = tb[3 * n + del_i - 1];
    const double *t_cins = tb + 4 * n + 1;
    const double *t_cdel = t_cins + ncins;
    double best = -RF_INF;
    int mv = 0;
    auto helper = [&](double msc, int move, int a, int b) {
        const int pi = i - a, pj = j - b;
        const int rc = min(pj, ncols);
        if (g.inband(pi - 1, rc - 1)) {
            const double v = (acol < 1 || pj <= acol) ? g.get(A, pi - 1, pj - 1)
                                                      : nc[(size_t)(pi - 1) + (size_t)ncld * (pj - acol - 1)];
            const double sc = v + msc;
            if (sc > best) {
                best = sc;
                mv = move;
            }
        }
    };
    helper(ms, 1, 1, 1);
    helper(is, 2, 1, 0);
    helper(ds, 3, 0, 1);
    if (ncins > 0 || ncdel > 0) {
        if (ncins > 0 && i > 3)
            helper(t_cins[i - 3 - 1], 4, 3, 0);
        if (ncdel > 0 && j > 3)
            helper(t_cdel[del_i - 1], 5, 0, 3);
    }
    out = best;
    return best != -RF_INF && mv != 0;
}

// equal_ranges((imn,imx), row_range(B, bj)) then summax (1-based rows);
// acolvals indexed by absolute 1-based row
__device__ double summax_nc(const Geo &g, const double *acolvals, int imn, int imx,
                            const double *B, int bj)
{
    int bs, be;
    g.rows(bj - 1, bs, be);
    bs += 1;
    be += 1;
    const int lo = max(imn, bs), hi = min(imx, be);
    double r = -RF_INF;
    for (int i = lo; i <= hi; ++i) {
        const double x = acolvals[i - 1] + g.get(B, i - 1, bj - 1);
        r = (i == lo) ? x : fmax(r, x);
    }
    return r;
}

__global__ void k_codon(const CodonTask *__restrict__ tasks, int ntasks,
                        const uint8_t *__restrict__ bases, const double *__restrict__ tabs,
                        const double *__restrict__ bands, double *__restrict__ scratch,
                        double *__restrict__ out)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntasks)
        return;
    const CodonTask T = tasks[t];
    const double qnan = __builtin_nan("");
    const double *A = bands + T.A;
    const double *B = bands + T.B;
    const uint8_t *s = bases + T.sb;
    const uint8_t *cons = bases + T.tb;
    const double *tb = tabs + T.tab;
    double *nc = scratch + T.scratch;
    Geo g;
    g.n = T.n;
    g.m = T.m;
    g.bw = T.bw;
    g.H = T.H;
    g.P = T.P;
    g.c = max(T.m - T.n, 0) + T.bw;
    const int n = T.n, m = T.m;
    const int nrows = n + 1, ncols = m + 1;
    const int kind = T.kind, pos = T.pos;

    if (T.ncins == 0 && T.ncdel == 0) {
        // score_nocodon on a single sequence (model.jl:242-285)
        double result = qnan;
        if (kind == 2) {
            // seq_score_deletion: summax(A col pos, B col pos+1) (model.jl:227-236)
            int as, ae, bs, be;
            g.rows(pos - 1, as, ae);
            g.rows(pos, bs, be);
            const int lo = max(as, bs), hi = min(ae, be);
            double r = -RF_INF;
            for (int i = lo; i <= hi; ++i) {
                const double x = g.get(A, i, pos - 1) + g.get(B, i, pos);
                r = (i == lo) ? x : fmax(r, x);
            }
            result = r;
        } else {
            const int acol = pos + (kind == 0 ? 0 : 1);
            const int new_acol = acol + 1;
            int amin, amax;
            g.rows(min(new_acol, ncols) - 1, amin, amax);
            amin += 1;
            amax += 1;
            bool ok = true;
            for (int i = amin; i <= amax && ok; ++i) {
                const int sb = i > 1 ? s[i - 2] : 4;
                double v;
                ok = update_nc(g, A, nc, nrows, acol, i, new_acol, sb, T.base, tb, 0, 0, v);
                nc[i - 1] = v;
            }
            if (ok) {
                const double sc = summax_nc(g, nc, amin, amax, B, pos + 1);
                result = (sc == -RF_INF) ? qnan : sc;
            }
        }
        out[T.out_idx] = result;
        return;
    }

    // codon path (model.jl:310-383)
    const int acol = pos + (kind == 1 ? 0 : -1) + 1;
    const int first_bcol = acol + (kind == 1 ? 1 : 2);
    const int last_bcol = first_bcol + 2;
    if (kind == 2 && acol == ncols - 1) {
        out[T.out_idx] = g.get(A, nrows - 1, ncols - 2);
        return;
    }
    const bool just_a = last_bcol >= ncols;
    const int n_after = !just_a ? 3 : m - pos;
    const int n_new_bases = kind == 2 ? 0 : 1;
    if (n_new_bases == 0 && n_after == 0) {
        out[T.out_idx] = qnan;
        return;
    }
    const int n_new = n_new_bases + n_after;
    int sub[8];
    int nsub = 0;
    if (kind != 2)
        sub[nsub++] = T.base;
    const int stop = min(pos + 1 + n_after - 1, m);
    for (int k = pos + 1; k <= stop && nsub < 8; ++k)
        sub[nsub++] = cons[k - 1];
    if (nsub < n_new) {
        out[T.out_idx] = qnan;
        return;
    }
    bool ok = true;
    for (int j = 1; j <= n_new && ok; ++j) {
        const int range_col = min(acol + j, ncols);
        int amin, amax;
        g.rows(range_col - 1, amin, amax);
        amin += 1;
        amax += 1;
        for (int i = amin; i <= amax && ok; ++i) {
            const int sb = i > 1 ? s[i - 2] : 4;
            double v;
            ok = update_nc(g, A, nc, nrows, acol, i, acol + j, sb, sub[j - 1], tb, T.ncins,
                           T.ncdel, v);
            nc[(size_t)(i - 1) + (size_t)nrows * (j - 1)] = v;
        }
    }
    if (!ok) {
        out[T.out_idx] = qnan;
        return;
    }
    if (just_a) {
        out[T.out_idx] = nc[(size_t)(nrows - 1) + (size_t)nrows * (n_new - 1)];
        return;
    }
    double best = -RF_INF;
    for (int j = 1; j <= 3; ++j) {
        const int new_j = n_new - 3 + j;
        int imn, imx;
        g.rows(min(acol + new_j, ncols) - 1, imn, imx);
        imn += 1;
        imx += 1;
        const int bj = first_bcol + j - 1;
        if (bj > ncols) {
            best = qnan;
            break;
        }
        const double sc = summax_nc(g, nc + (size_t)nrows * (new_j - 1), imn, imx, B, bj);
        if (sc > best)
            best = sc;
    }
    out[T.out_idx] = (best == -RF_INF) ? qnan : best;
}

// ---------------------------------------------------------------------
// k_codon_dense: k_codon's score for every dense slot of a group, one lane
// per slot, no per-proposal scratch and no per-proposal descriptor
// (rf_score_dense_ref).
//
// In update_nc, new column j at row i reads column j at rows i-1 and i-3,
// column j-1 at rows i and i-1 and column j-3 at row i (a column of A for
// j <= 3, new column 1 for j = 4).  So the up-to-four new columns advance row
// by row together, each with its last four rows in registers (h[j][0..3] =
// rows i .. i-3), column 1 first; the closing summax against B accumulates
// as the rows pass (ascending, first value then fmax, as summax_nc).  Every
// candidate, gate and addition is k_codon's, in k_codon's order, so the
// result has k_codon's bits; k_codon stops at the first failed update where
// this kernel goes on and reports NaN at the end.
//
// Lane order is the dense table's: slot = p * 9 + k, so the nine lanes of a
// position read the same A / B cells and table rows.  The lane adds its
// score to the reads' total in place (total + s_ref).  Sub / Del of p = 0 get
// NaN; the consensus base's own Sub slot is left as the scorer wrote it.
// ---------------------------------------------------------------------

// one per group that has a reference slot, ordered by blk0
struct alignas(16) CodonDenseGroup {
    int64_t A, B, sb, tab, tb;   // the reference's bands, bases and tables; template bases
    int64_t dense_off;           // the group's totals [m+1][9]
    int32_t n, m, bw, H;
    int32_t ncins, ncdel, P;
    int32_t blk0;                // first workgroup of the group
};

__device__ __forceinline__ double codon_dense_sref(const Geo &g, const double *__restrict__ A,
                                                   const double *__restrict__ B,
                                                   const uint8_t *__restrict__ s,
                                                   const uint8_t *__restrict__ cons,
                                                   const double *__restrict__ tb, int ncins, int ncdel,
                                                   int kind, int pos, int base)
{
    const double qnan = __builtin_nan("");
    const int n = g.n, m = g.m;
    const int nrows = n + 1, ncols = m + 1;
    int acol, n_new, n_new_bases = 1, nsum, bj0;
    if (ncins == 0 && ncdel == 0) {
        // score_nocodon on a single sequence (model.jl:242-285)
        if (kind == 2) {
            // seq_score_deletion: summax(A col pos, B col pos+1) (model.jl:227-236)
            int as, ae, bs, be;
            g.rows(pos - 1, as, ae);
            g.rows(pos, bs, be);
            const int lo = max(as, bs), hi = min(ae, be);
            double r = -RF_INF;
            for (int i = lo; i <= hi; ++i) {
                const double x = g.get(A, i, pos - 1) + g.get(B, i, pos);
                r = (i == lo) ? x : fmax(r, x);
            }
            return r;
        }
        acol = pos + (kind == 0 ? 0 : 1);
        n_new = 1;
        nsum = 1;
        bj0 = pos + 1;
    } else {
        // codon path (model.jl:310-383)
        acol = pos + (kind == 1 ? 0 : -1) + 1;
        const int first_bcol = acol + (kind == 1 ? 1 : 2);
        const int last_bcol = first_bcol + 2;
        if (kind == 2 && acol == ncols - 1)
            return g.get(A, nrows - 1, ncols - 2);
        const bool just_a = last_bcol >= ncols;
        const int n_after = !just_a ? 3 : m - pos;
        n_new_bases = kind == 2 ? 0 : 1;
        if (n_new_bases == 0 && n_after == 0)
            return qnan;
        n_new = n_new_bases + n_after;
        // sub_consensus: the proposal's base, then the consensus after pos
        if (n_new_bases + min(n_after, m - pos) < n_new || n_new > 4)
            return qnan;
        nsum = just_a ? 0 : 3;
        bj0 = first_bcol;
    }

    // per new column (0-based j here; update_nc's column is acol + j + 1)
    double h[4][4], r[4];
    int amin[4], amax[4], slo[4], shi[4], bjc[4], subb[4];
    int imin = INT_MAX, imax = 0;
    bool nob = false;   // a B column past the band's last (k_codon: NaN)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            h[j][q] = -RF_INF;
        r[j] = -RF_INF;
        amin[j] = 1;
        amax[j] = 0;
        slo[j] = 1;
        shi[j] = 0;
        bjc[j] = 0;
        subb[j] = 4;
        if (j < n_new) {
            int a, b;
            g.rows(min(acol + j + 1, ncols) - 1, a, b);
            amin[j] = a + 1;
            amax[j] = b + 1;
            imin = min(imin, amin[j]);
            imax = max(imax, amax[j]);
            subb[j] = j < n_new_bases ? base : cons[pos + j - n_new_bases];
            const int sidx = j - (n_new - nsum);   // >= 0: summed with B column bj0 + sidx
            if (sidx >= 0) {
                const int bj = bj0 + sidx;
                if (bj > ncols) {
                    nob = true;
                } else {
                    int bs, be;
                    g.rows(bj - 1, bs, be);
                    slo[j] = max(amin[j], bs + 1);
                    shi[j] = min(amax[j], be + 1);
                    bjc[j] = bj;
                }
            }
        }
    }

    const double *t_cins = tb + 4 * (size_t)n + 1;
    const double *t_cdel = t_cins + ncins;
    bool bad = false;
    double last = -RF_INF;   // the last new column at the band's last row (just_a)
    for (int i = imin; i <= imax; ++i) {
        // align.jl:50-112, 1-based row i as update_nc
        const int seq_i = max(i - 1, 1);
        const int sb = i > 1 ? s[i - 2] : 4;
        const double t_m = tb[seq_i - 1];
        const double t_x = tb[n + seq_i - 1];
        const double is = tb[2 * n + seq_i - 1];
        const double ds = tb[3 * n + i - 1];
        const double cis = (ncins > 0 && i > 3) ? t_cins[i - 3 - 1] : 0.0;
        const double cds = ncdel > 0 ? t_cdel[i - 1] : 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < n_new) {
                h[j][3] = h[j][2];
                h[j][2] = h[j][1];
                h[j][1] = h[j][0];
                h[j][0] = -RF_INF;
                if (i >= amin[j] && i <= amax[j]) {
                    const int jabs = acol + j + 1;
                    const int cself = min(jabs, ncols) - 1;       // 0-based range columns
                    const int cprev = min(jabs - 1, ncols) - 1;
                    const double ms = (sb == subb[j]) ? t_m : t_x;
                    double best = -RF_INF;
                    if (g.inband(i - 2, cprev)) {                 // match
                        double v;
                        if (j == 0)
                            v = g.get(A, i - 2, jabs - 2);
                        else
                            v = h[j > 0 ? j - 1 : 0][1];
                        const double sc = v + ms;
                        if (sc > best)
                            best = sc;
                    }
                    if (g.inband(i - 2, cself)) {                 // insert
                        const double sc = h[j][1] + is;
                        if (sc > best)
                            best = sc;
                    }
                    if (g.inband(i - 1, cprev)) {                 // delete
                        double v;
                        if (j == 0)
                            v = g.get(A, i - 1, jabs - 2);
                        else
                            v = h[j > 0 ? j - 1 : 0][0];
                        const double sc = v + ds;
                        if (sc > best)
                            best = sc;
                    }
                    if (ncins > 0 && i > 3 && g.inband(i - 4, cself)) {   // codon insert
                        const double sc = h[j][3] + cis;
                        if (sc > best)
                            best = sc;
                    }
                    if (ncdel > 0 && jabs > 3 && g.inband(i - 1, min(jabs - 3, ncols) - 1)) {   // codon delete
                        double v;
                        if (j < 3)
                            v = g.get(A, i - 1, jabs - 4);
                        else
                            v = h[0][0];
                        const double sc = v + cds;
                        if (sc > best)
                            best = sc;
                    }
                    h[j][0] = best;
                    bad = bad || best == -RF_INF;
                    if (bjc[j] > 0 && i >= slo[j] && i <= shi[j]) {
                        const double x = best + g.get(B, i - 1, bjc[j] - 1);
                        r[j] = (i == slo[j]) ? x : fmax(r[j], x);
                    }
                    if (j == n_new - 1 && i == nrows)
                        last = best;
                }
            }
        }
    }
    if (bad)
        return qnan;
    if (ncins == 0 && ncdel == 0)
        return r[0] == -RF_INF ? qnan : r[0];
    if (nsum == 0)
        return last;
    if (nob)
        return qnan;
    double best = -RF_INF;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (bjc[j] > 0 && r[j] > best)
            best = r[j];
    return best == -RF_INF ? qnan : best;
}

__global__ void __launch_bounds__(64)
k_codon_dense(const CodonDenseGroup *__restrict__ groups, int ngroups,
              const uint8_t *__restrict__ bases, const double *__restrict__ tabs,
              const double *__restrict__ bands, double *__restrict__ dense)
{
    // the group of this workgroup: the last descriptor with blk0 <= blockIdx.x
    int glo = 0, ghi = ngroups - 1;
    while (glo < ghi) {
        const int mid = (glo + ghi + 1) >> 1;
        if (groups[mid].blk0 <= (int)blockIdx.x)
            glo = mid;
        else
            ghi = mid - 1;
    }
    const CodonDenseGroup G = groups[glo];
    const int idx = ((int)blockIdx.x - G.blk0) * 64 + (int)threadIdx.x;
    if (idx >= 9 * (G.m + 1))
        return;
    const int p = idx / 9, k = idx - 9 * p;
    const int kind = k < 4 ? 0 : (k == 4 ? 2 : 1);
    const int base = k < 4 ? k : (k == 4 ? 0 : k - 5);
    double *dst = dense + G.dense_off + idx;
    const uint8_t *cons = bases + G.tb;
    if (kind != 1 && p == 0) {
        *dst = __builtin_nan("");
        return;
    }
    if (kind == 0 && cons[p - 1] == base)
        return;   // the consensus base's own slot: not a proposal
    Geo g;
    g.n = G.n;
    g.m = G.m;
    g.bw = G.bw;
    g.H = G.H;
    g.P = G.P;
    g.c = max(G.m - G.n, 0) + G.bw;
    const double sref = codon_dense_sref(g, bands + G.A, bands + G.B, bases + G.sb, cons, tabs + G.tab,
                                         G.ncins, G.ncdel, kind, p, base);
    *dst = *dst + sref;
}

// totals for the proposal list: reads fold (dense) + reference score last
__global__ void k_gather(int64_t nprops, const int32_t *__restrict__ pgroup,
                         const uint8_t *__restrict__ kind, const int32_t *__restrict__ pos,
                         const uint8_t *__restrict__ base, const ScoreGroup *__restrict__ groups,
                         const int32_t *__restrict__ has_reads, const double *__restrict__ dense,
                         const double *__restrict__ refscore, const int32_t *__restrict__ has_ref,
                         double *__restrict__ out, int *__restrict__ err)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nprops)
        return;
    const int g = pgroup[k];
    const ScoreGroup G = groups[g];
    const int kd = kind[k];
    const int slot = kd == 0 ? base[k] : (kd == 2 ? 4 : 5 + base[k]);
    double tot = 0.0;
    if (has_reads[g])
        tot = dense[G.dense_off + (size_t)pos[k] * 9 + slot];
    if (has_ref[g])
        tot += refscore[k];
    if (tot != tot)
        set_err(err, 3);  // failed to compute a valid score / new score is invalid
    out[k] = tot;
}

// ---------------------------------------------------------------------
// k_bt_win: backtrace + count_errors (align.jl:229-245), one wave per
// alignment, from LDS windows (round 4: codon moves and any band height too --
// the reference's codon alignment and edit_distance's wide bands).
//
// The walk is sequential, so the wave parallelises it across a "box" of the
// cells it can reach next: from the current cell (ii0, jj0) lane l computes
// the move of cell (ii0 - di, jj0 - dj), di = l / 3, dj = di - (l % 3 - 1),
// i.e. the 3 band diagonals around the walk's diagonal for 21 steps
// (63 cells).  Each move is the first strictly-best candidate over the
// stored A values (align.jl:77-104, the same FP64 sums as the forward fill),
// so it equals the trace band's move.  The walk then follows the box with
// one v_readlane per move (the move, the mismatch flag and the read base
// packed in one dword) until it leaves the box, and a new box is computed
// at the cell reached.
//
// Operands come from LDS: a window of kappa rows [klo, khi] of the A band,
// restricted to the elements [e0, e0 + wd) around the walk's diagonal
// (whole rows when P <= BTW_WD), and windows of the table rows and bases.
// The walk only moves to lower kappa; a window is re-staged below when a
// box would leave it.  Staging issues every load of a window before the
// first LDS write (one memory latency per window, not one per element).
// With a mask, the walk also marks the proposals its alignment implies
// (moves_to_proposals, model.jl:458-480; the set union does not depend on
// the walk direction).
// Codon moves (align.jl:77-104, TRACE_CODON_INSERT / _DELETE) reach cells
// 3 diagonals off the walk's: the windows then extend 2 more kappa rows,
// diagonals and table rows, the box evaluates the two codon candidates after
// the three others (the same strict-> order), and a codon move leaves the box
// (|u| = 3), so the next box starts at the cell it reaches.
// ---------------------------------------------------------------------
// The box's walk is ranked in parallel (pointer doubling over the 63
// cells' successors) instead of one readlane step per move (round 4:
// backtrace 19.8 -> 8.0 ms, alignment proposals 36.9 -> 12.9 ms per 512 e2e
// clusters, bit-exact, profiles/r04ab_btw_rank.txt; the sequential walk is
// in git history).
// elements staged per kappa row (the walk's box needs 3 -- 5 with codon
// moves -- around its diagonal): 8 holds twice the kappa rows of 16 in the
// same LDS, so windows are re-staged half as often: with the ranked walk,
// backtrace 8.1 -> 6.9 ms and alignment proposals 12.8 -> 10.7 ms per 512
// e2e clusters (profiles/r04ad_btw_window.txt); a 32-KB window is slower
#ifndef BTW_WD_ELEMS
#define BTW_WD_ELEMS 8
#endif
// window loads in flight per lane (one memory round trip per chunk)
#ifndef BTW_CHUNK
#define BTW_CHUNK 16
#endif
constexpr int BTW_WD = BTW_WD_ELEMS;   // staged elements per kappa row when P > BTW_WD (>= 6: codon boxes)
constexpr int BTW_T = 256;     // staged table rows / template bases per window

// NW > 1 (round 6): a launch of few walks (the reference's, edit_distance's:
// one latency-bound walk each) gives each walk NW waves and a box of
// 3 x (21 NW) cells; the rank's successor tables go through LDS with a block
// barrier per round (8 rounds for 252 cells) and the results are broadcast
// through LDS.  A box then carries ~4x the moves for ~2x the round latency.
constexpr int BTW_FEW = 64;    // launches of at most this many walks take NW = 4

template <int BTW_A, int NW = 1>   // doubles of the A window (4096: 32 KB, 2048: 16 KB); waves per walk
__global__ void __launch_bounds__(64 * NW)
k_bt_win(const BTTask *__restrict__ tasks, const uint8_t *__restrict__ bases, const double *__restrict__ tabs,
         const double *__restrict__ bands, int8_t *__restrict__ moves, int32_t *__restrict__ nmoves,
         int32_t *__restrict__ nerr, int *__restrict__ err, uint8_t *__restrict__ mask, int do_indels)
{
    constexpr int NT = 64 * NW;                         // threads: box cells + the sink
    constexpr int BD = 21 * NW - 1;                     // box depth: cells di = 0 .. BD (3 diagonals)
    constexpr int TT = NW == 1 ? BTW_T : 2 * BTW_T;     // staged table rows / template bases
    constexpr int RB = NW == 1 ? 6 : (NW == 2 ? 7 : 8); // doubling rounds: log2(NT)
    static_assert(NW == 1 || NW == 2 || NW == 4, "1, 2 or 4 waves per walk");
    constexpr int NX = NW > 1 ? NT : 1;                 // LDS rank arrays (NW > 1 only)
    __shared__ double sA[BTW_A];
    __shared__ double sTm[TT], sTx[TT], sTi[TT], sTd[TT];
    __shared__ double sTci[TT], sTcd[TT];   // codon tables (codon alignments only)
    __shared__ uint8_t sS[TT], sTt[TT];
    __shared__ int sJ[2][NX], sPk[NX], sMv[NX], sNi[NX], sNj[NX], sCnt[NW];
    const BTTask T = tasks[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    auto bsync = [&]() {
        if constexpr (NW == 1)
            wave_sync();
        else
            __syncthreads();
    };
    const double *A = bands + T.A;
    const uint8_t *s = bases + T.sb;
    const uint8_t *tt = bases + T.tb;
    const double *tb = tabs + T.tab;
    const int n = T.n, m = T.m, H = T.H, P = T.P;
    const int c = max(m - n, 0) + T.bw;
    const int K = H + 2 * m;
    const bool skew = T.flags & 2, trim = T.flags & 4;
    const bool cod = T.ncins > 0 || T.ncdel > 0;
    const int wd = min(P, cod ? max(BTW_WD, 6) : BTW_WD);   // codon boxes need 5 elements around the walk
    const int W = BTW_A / wd;                          // kappa rows per window (>= 256)
    const int ext = cod ? 2 : 0;                       // codon predecessors: 2 more rows / diagonals
    const double *t_cins = tb + 4 * (size_t)n + 1;     // cins[ii - 3], ncins = n - 2 entries
    const double *t_cdel = t_cins + T.ncins;           // cdel[ii], ncdel = n + 1 entries
    int8_t *out = moves + T.out;
    uint8_t *mk = mask ? mask + T.mask : nullptr;
    // this thread's box cell offsets
    const int bdi = tid / 3, bdj = bdi - (tid % 3 - 1);
    const bool blane = tid < 3 * (BD + 1);
    int ii = n, jj = m, cnt = 0, errs = 0;
    int klo = -1, e0 = 0;                              // A window: rows [klo, klo + W), elements [e0, e0 + wd)
    int q0 = -1, r0 = -1;                              // table rows [q0, q0 + BTW_T), bases [r0, r0 + BTW_T)
    int failed = 0;
    while ((ii > 0 || jj > 0) && !failed) {
        // ---- windows for the box at (ii, jj)
        const int kap0 = ii + jj + c;                  // kappa of the current cell
        const int d0 = ii - jj + c;
        const int klo_need = max(kap0 - 2 * BD - 3 - ext, 0);
        const int elo = max(d0 - 2 - ext, 0) >> 1, ehi = min(d0 + 2 + ext, H - 1) >> 1;
        if (klo < 0 || klo_need < klo || elo < e0 || ehi >= e0 + wd) {
            const int khi = min(kap0 - 1, K - 1);
            klo = max(0, khi - W + 1);
            e0 = min(max((d0 >> 1) - wd / 2, 0), P - wd);
            const int nrow = khi - klo + 1, na = nrow * wd;
            bsync();                                   // every thread is done with the old window
            if (wd == 8 && na == BTW_A) {
                // a whole window of 8-element rows (the common case): thread =
                // NT / 8 rows x 8 columns per u, so each load is the previous
                // one's address plus NT / 8 rows and each LDS slot an immediate
                // offset (round 6: the generic loop spent ~10 instructions per
                // element)
                const double *src = A + (size_t)(klo + (tid >> 3)) * P + e0 + (tid & 7);
                const size_t step = (size_t)(NT / 8) * P;
                for (int u0 = 0; u0 < BTW_A / NT; u0 += BTW_CHUNK) {
                    double v[BTW_CHUNK];
#pragma unroll
                    for (int u = 0; u < BTW_CHUNK; ++u)
                        v[u] = src[(size_t)(u0 + u) * step];
#pragma unroll
                    for (int u = 0; u < BTW_CHUNK; ++u)
                        sA[tid + NT * (u0 + u)] = v[u];
                }
            } else {
                // element t = row * wd + col, t = tid + NT u: incremental row / col
                const int qr = NT / wd, rr = NT % wd;
                int row = tid / wd, col = tid % wd;
                for (int u0 = 0; u0 < BTW_A / NT; u0 += BTW_CHUNK) {
                    double v[BTW_CHUNK];
                    int rw = row, cl = col;
#pragma unroll
                    for (int u = 0; u < BTW_CHUNK; ++u) {   // issue all loads of the chunk
                        const int t = tid + NT * (u0 + u);
                        v[u] = t < na ? A[(size_t)(klo + rw) * P + e0 + cl] : 0.0;
                        rw += qr;
                        cl += rr;
                        if (cl >= wd) {
                            cl -= wd;
                            ++rw;
                        }
                    }
#pragma unroll
                    for (int u = 0; u < BTW_CHUNK; ++u) {
                        const int t = tid + NT * (u0 + u);
                        if (t < na)
                            sA[t] = v[u];
                    }
                    row = rw;
                    col = cl;
                    if (NT * (u0 + BTW_CHUNK) >= na)      // thread 0 holds the chunk's lowest t
                        break;
                }
            }
            bsync();
        }
        const int qlo_need = max(ii - BD - 1 - ext, 0), rlo_need = max(jj - BD - 2, 0);
        if (q0 < 0 || qlo_need < q0 || rlo_need < r0 || ii > q0 + TT - 1 || max(jj - 1, 0) > r0 + TT - 1) {
            q0 = max(0, ii - TT + 1);                  // del index ii .. ; ks = ii - 1 ..
            r0 = max(0, max(jj - 1, 0) - TT + 1);
            bsync();
            constexpr int NU = TT / NT;
            double vm[NU], vx[NU], vi[NU], vd[NU];
            int vs[NU], vt[NU];
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int q = q0 + tid + NT * u;
                const int ks = min(q, n - 1);
                const int qd = min(q, n);
                vm[u] = tb[ks];
                vx[u] = tb[n + ks];
                vi[u] = tb[2 * (size_t)n + ks];
                vd[u] = tb[3 * (size_t)n + qd];
                vs[u] = q < n ? s[q] : 4;
                const int r = r0 + tid + NT * u;
                vt[u] = r < m ? tt[r] : 4;
            }
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int e = tid + NT * u;
                sTm[e] = vm[u];
                sTx[e] = vx[u];
                sTi[e] = vi[u];
                sTd[e] = vd[u];
                sS[e] = (uint8_t)vs[u];
                sTt[e] = (uint8_t)vt[u];
            }
            if (cod) {
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    const int q = q0 + tid + NT * u;
                    vm[u] = T.ncins > 0 ? t_cins[min(q, T.ncins - 1)] : 0.0;
                    vx[u] = T.ncdel > 0 ? t_cdel[min(q, T.ncdel - 1)] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    sTci[tid + NT * u] = vm[u];
                    sTcd[tid + NT * u] = vx[u];
                }
            }
            bsync();
        }
        // ---- box: the move of cell (ci, cj), packed mv | mismatch << 3 | read base << 4.
        // Branch-free: every LDS read is issued at a selected (valid) index and
        // masked after, so the box is one LDS round trip (round 6; the guarded
        // reads were exec-mask branches and three dependent round trips).
        int pack = 0;
        {
            const int ci = ii - bdi, cj = jj - bdj;
            const int dc = ci - cj + c, kap = ci + cj + c;   // the cell's diagonal and kappa
            const bool valid = blane & (bdj >= 0) & (ci >= 0) & (cj >= 0) & ((ci | cj) != 0) &
                               ((unsigned)dc < (unsigned)H);
            // predecessors in the band: (ci-1, cj-1) diagonal dc, (ci-1, cj) dc-1, (ci, cj-1) dc+1
            const bool in1 = valid & (ci >= 1) & (cj >= 1), in2 = valid & (ci >= 1) & (dc >= 1),
                       in3 = valid & (cj >= 1) & (dc + 1 < H);
            // indices masked to 0 off the band (an and, not a select: hipcc
            // turns selects of computed indices into exec-mask branches)
            const int row1 = (kap - 2 - klo) * wd - e0, row2 = row1 + wd;
            const int a1i = (row1 + (dc >> 1)) & -(int)in1;
            const int a2i = (row2 + ((dc - 1) >> 1)) & -(int)in2;
            const int a3i = (row2 + ((dc + 1) >> 1)) & -(int)in3;
            const double a1 = sA[a1i], a2 = sA[a2i], a3 = sA[a3i];
            const int ks = (max(ci - 1, 0) - q0) & -(int)valid;
            const int kd = (ci - q0) & -(int)valid;
            const bool hs = valid & (ci >= 1), ht = valid & (cj >= 1);
            const int sbr = sS[(ci - 1 - q0) & -(int)hs], tbr = sTt[(cj - 1 - r0) & -(int)ht];
            const double tm = sTm[ks], tx = sTx[ks], ti = sTi[ks], ds = sTd[kd];
            // every read issued before the selects (else hipcc sinks a load
            // into a branch of its own or after another's wait)
            asm volatile("" ::"v"(tm), "v"(tx), "v"(ti), "v"(ds), "v"(a1), "v"(a2), "v"(a3), "v"(sbr), "v"(tbr));
            const int sb = hs ? sbr : 4, tbb = ht ? tbr : 4;
            const bool mis = sb != tbb;
            const double ms = mis ? (skew ? tx * 0.99 : tx) : tm;
            const double is = (trim & ((cj == 0) | (cj == m))) ? 0.0 : ti;
            double best = -RF_INF, x;
            int mv = 0;
            x = a1 + ms;
            if (in1 && x > best) { best = x; mv = 1; }
            x = a2 + is;
            if (in2 && x > best) { best = x; mv = 2; }
            x = a3 + ds;
            if (in3 && x > best) { best = x; mv = 3; }
            if (cod) {
                // TRACE_CODON_INSERT from (ci - 3, cj), TRACE_CODON_DELETE from (ci, cj - 3)
                const bool in4 = valid & (T.ncins > 0) & (ci >= 3) & (dc >= 3);
                const bool in5 = valid & (T.ncdel > 0) & (cj >= 3) & (dc + 3 < H);
                const int row3 = row1 - wd;
                const double a4 = sA[(row3 + ((dc - 3) >> 1)) & -(int)in4];
                const double a5 = sA[(row3 + ((dc + 3) >> 1)) & -(int)in5];
                x = a4 + sTci[(ci - 3 - q0) & -(int)in4];
                if (in4 && x > best) { best = x; mv = 4; }
                x = a5 + sTcd[kd];
                if (in5 && x > best) { best = x; mv = 5; }
            }
            pack = valid ? (mv | (mis ? 8 : 0) | (sb << 4)) : 0;
        }
        // ---- walk the box by ranking its cells in parallel: J0 = each box
        // cell's successor lane (or the sink, lane 63: leaves the box, reaches
        // (0, 0), or no move), J_r = J0^(2^r) by pointer doubling; lane k then
        // finds the k-th cell of the walk from lane 1 (the current cell) by
        // the binary digits of k, and emits the k-th move.  Round r applies
        // J_r to the lane's cell and squares J_r with two independent
        // permutes (round 6: 6 dependent permute rounds instead of 11).  The
        // same moves, marks, error counts and failure points as the
        // sequential walk (git history).
        {
            constexpr int SINK = NT - 1;
            const int mv0 = pack & 7;
            const int bu = tid % 3 - 1;
            const int ndi = bdi + (int)((mv0 == 1) | (mv0 == 2));
            const int nu = bu + (int)(mv0 == 2) - (int)(mv0 == 3);
            const bool inbox = (mv0 >= 1 && mv0 <= 3) && ndi <= BD && nu >= -1 && nu <= 1;
            const int ti = ii - ndi, tj = jj - (ndi - nu);
            int J = (blane && inbox && (ti > 0 || tj > 0)) ? ndi * 3 + nu + 1 : SINK;
            if (tid == SINK)
                J = SINK;
            int cell = 1;   // thread k: the k-th cell of the walk
            int pk;
            if constexpr (NW == 1) {
#pragma unroll
                for (int r = 0; r < RB; ++r) {
                    const int nx = __builtin_amdgcn_ds_bpermute(cell << 2, J);
                    if (r < RB - 1)
                        J = __builtin_amdgcn_ds_bpermute(J << 2, J);
                    cell = ((lane >> r) & 1) ? nx : cell;
                }
                pk = __builtin_amdgcn_ds_bpermute(cell << 2, pack);
            } else {
                // the same rounds through LDS (two tables, a block barrier each)
                sPk[tid] = pack;
                sJ[0][tid] = J;
                bsync();
#pragma unroll
                for (int r = 0; r < RB; ++r) {
                    const int nx = sJ[r & 1][cell];
                    if (r < RB - 1) {
                        J = sJ[r & 1][J];
                        sJ[(r + 1) & 1][tid] = J;
                    }
                    cell = ((tid >> r) & 1) ? nx : cell;
                    bsync();
                }
                pk = sPk[cell];
            }
            // cells reached; a cell with no move (mv 0) ends the walk in failure
            const bool visited = cell != SINK;
            const int mvk = pk & 7;
            const int cdi = cell / 3, cdu = cell % 3 - 1;
            const int ci = ii - cdi, cj = jj - (cdi - cdu);
            // the cell after this move
            const int di = (mvk == 1 || mvk == 2) ? 1 : (mvk == 4 ? 3 : 0);
            const int dj = (mvk == 1 || mvk == 3) ? 1 : (mvk == 5 ? 3 : 0);
            int nvis;
            bool nomove_last;
            if constexpr (NW == 1) {
                nvis = __popcll(__ballot(visited));
                nomove_last = __builtin_amdgcn_readlane(mvk, max(nvis - 1, 0)) == 0;
            } else {
                const int cw = __popcll(__ballot(visited));
                if (lane == 0)
                    sCnt[wv] = cw;
                sMv[tid] = mvk;
                sNi[tid] = ci - di;
                sNj[tid] = cj - dj;
                bsync();
                nvis = 0;
#pragma unroll
                for (int w = 0; w < NW; ++w)
                    nvis += sCnt[w];
                nomove_last = sMv[max(nvis - 1, 0)] == 0;
            }
            int nmv = nomove_last ? nvis - 1 : nvis;
            bool fail_now = nomove_last;
            if (cnt + nmv > n + m) {   // the sequential walk's cnt >= n + m check
                nmv = n + m - cnt;
                fail_now = true;
            }
            const bool emit = tid < nmv;
            const int ksb = pk >> 4;
            const bool mism = pk & 8;
            // the forward step of this move ends at (ci, cj) (moves_to_proposals):
            // a mismatch marks (cj, read base), an insertion (cj, 5 + base), a
            // deletion (cj, 4) -- one store, its slot selected (no branches)
            const bool mark = emit && mk && ((mvk == 1 && mism) || (do_indels && (mvk == 2 || mvk == 3)));
            const int slot9 = cj * 9 + (mvk == 1 ? ksb : (mvk == 2 ? 5 + ksb : 4));
            if (emit)
                out[n + m - 1 - (cnt + tid)] = (int8_t)mvk;
            if (mark)
                mk[(size_t)slot9] = 1;
            // count_errors: 1 per mismatch or indel, 3 per codon move (this
            // wave's threads; the waves' sums are added at the end)
            errs += __popcll(__ballot(emit && (mvk >= 2 || mism))) + 2 * __popcll(__ballot(emit && mvk >= 4));
            if (nmv > 0) {
                if constexpr (NW == 1) {
                    ii = __builtin_amdgcn_readlane(ci - di, nmv - 1);
                    jj = __builtin_amdgcn_readlane(cj - dj, nmv - 1);
                } else {
                    ii = sNi[nmv - 1];
                    jj = sNj[nmv - 1];
                }
            }
            cnt += nmv;
            if (fail_now) {
                if (tid == 0)
                    set_err(err, 2);  // failed to find a move
                failed = 1;
            }
        }
    }
    if constexpr (NW > 1) {
        bsync();
        if (lane == 0)
            sCnt[wv] = errs;
        bsync();
        errs = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w)
            errs += sCnt[w];
    }
    if (tid == 0) {
        nmoves[T.idx] = cnt;
        nerr[T.idx] = errs;
    }
}

// ---------------------------------------------------------------------
// k_aln_sums: alignment_error_probs's per-column sums (model.jl:817-840)
// on the device, from the backtrace moves already there (k_bt_win).  One workgroup per group (cluster); its reads are walked in
// batch order, one read at a time: the 256 threads take 256 consecutive
// moves, a block prefix sum of the (read, consensus) steps gives each move's
// (i, j), and a MATCH move adds base_distribution(s[i], match[i]) to column
// j: out[j][b] += (b == s[i] ? match[i] : errlp(match[i])).  A read matches a
// column at most once, and a barrier separates the reads, so every column
// receives the same FP64 additions in the same order as the host loop
// (rf_aln_error_sums).  errlp = log10(1 - 10^ilp) - log10(3) is evaluated on
// the host (libm) once per row-code dictionary entry; the read's row-code
// record gives its entry and base.
// ---------------------------------------------------------------------
struct alignas(16) AlnSumRead {
    int64_t mv;    // moves slot (bytes in the backtrace move buffer; moves end-aligned in n + m)
    int64_t rec;   // row-code records (doubles offset into the table arena)
    int32_t n, m, idx, pad;
};
struct alignas(16) AlnSumGroup {
    int64_t out;   // doubles offset of the group's m x 4 sums
    int32_t r0, r1, m, pad;
};

__global__ void __launch_bounds__(256) k_aln_sums(const AlnSumGroup *__restrict__ groups,
                                                  const AlnSumRead *__restrict__ reads,
                                                  const double *__restrict__ tabs, const int8_t *__restrict__ moves,
                                                  const int32_t *__restrict__ nmoves, const double *__restrict__ lut,
                                                  const double *__restrict__ errlut, double *__restrict__ out)
{
    __shared__ int wsum[4];
    const AlnSumGroup G = groups[blockIdx.x];
    double *o = out + G.out;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int e = tid; e < 4 * G.m; e += 256)
        o[e] = 0.0;
    __syncthreads();
    for (int r = G.r0; r < G.r1; ++r) {
        const AlnSumRead R = reads[r];
        const int cnt = nmoves[R.idx];
        const int8_t *mv = moves + R.mv + (R.n + R.m - cnt);
        const uint64_t *rec = (const uint64_t *)(tabs + R.rec);
        int ci = 0, cj = 0;   // read / consensus positions consumed before this tile (block-uniform)
        for (int b0 = 0; b0 < cnt; b0 += 256) {
            const int e = b0 + tid;
            const int v = e < cnt ? mv[e] : 0;
            // align.jl OFFSETS: MATCH (1,1), INSERT (1,0), DELETE (0,1), CODON_INSERT (3,0), CODON_DELETE (0,3)
            const int di = (v == 1 || v == 2) ? 1 : (v == 4 ? 3 : 0);
            const int dj = (v == 1 || v == 3) ? 1 : (v == 5 ? 3 : 0);
            // a tile moves (i, j) by at most 3 * 256 each: 16-bit fields of one
            // int hold the tile's prefix sums; the carry across tiles is two ints
            const int x = di | (dj << 16);
            int inc = x;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int y = __shfl_up(inc, off);
                if (lane >= off)
                    inc += y;
            }
            if (lane == 63)
                wsum[w] = inc;
            __syncthreads();
            int before = 0;
            for (int k = 0; k < w; ++k)
                before += wsum[k];
            const int tile = wsum[0] + wsum[1] + wsum[2] + wsum[3];
            __syncthreads();   // wsum is rewritten by the next tile
            if (v == 1) {
                const int ex = before + inc - x;
                const int i = ci + (ex & 0xffff), j = cj + (ex >> 16);
                const uint64_t rc = rec[i];
                const int code = (int)(rc & 0xffff), sb = (int)(rc >> 48) & 0xff;
                const double ilp = lut[4 * code], el = errlut[code];
                double *p = o + (size_t)j * 4;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    p[q] += q == sb ? ilp : el;
            }
            ci += tile & 0xffff;
            cj += tile >> 16;
        }
        __syncthreads();   // this read's additions precede the next read's
    }
}

// Groups with many reads (c3: one cluster of 1,000 reads) leave k_aln_sums
// one workgroup walking every read in turn (16.6 ms per call at c3, round 4
// profile).  There the sums run in two launches instead: k_aln_marks, one
// wave per read, writes each MATCH move's row-code entry and base into a
// (read, column) record; k_aln_fold, one lane per (group, column), adds the
// records of the column's reads in batch order -- the same FP64 additions in
// the same order per column as k_aln_sums and the host loop.
__global__ void __launch_bounds__(64) k_aln_marks(const AlnSumGroup *__restrict__ groups, int ngroups,
                                                  const AlnSumRead *__restrict__ reads,
                                                  const int64_t *__restrict__ rbase,
                                                  const double *__restrict__ tabs, const int8_t *__restrict__ moves,
                                                  const int32_t *__restrict__ nmoves, uint32_t *__restrict__ marks)
{
    const int r = blockIdx.x, lane = threadIdx.x;
    const AlnSumRead R = reads[r];
    const int cnt = nmoves[R.idx];
    const int8_t *mv = moves + R.mv + (R.n + R.m - cnt);
    const uint64_t *rec = (const uint64_t *)(tabs + R.rec);
    uint32_t *row = marks + rbase[r];   // this read's m records
    int ci = 0, cj = 0;
    for (int b0 = 0; b0 < cnt; b0 += 64) {
        const int e = b0 + lane;
        const int v = e < cnt ? mv[e] : 0;
        const int di = (v == 1 || v == 2) ? 1 : (v == 4 ? 3 : 0);
        const int dj = (v == 1 || v == 3) ? 1 : (v == 5 ? 3 : 0);
        const int x = di | (dj << 16);   // a tile moves (i, j) by at most 3 * 64 each
        int inc = x;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int y = __shfl_up(inc, off);
            if (lane >= off)
                inc += y;
        }
        if (v == 1) {
            const int ex = inc - x;
            const int i = ci + (ex & 0xffff), j = cj + (ex >> 16);
            const uint64_t rc = rec[i];
            row[j] = (uint32_t)(rc & 0xffff) | ((uint32_t)((rc >> 48) & 0xff) << 16) | 0x80000000u;
        }
        const int tile = __shfl(inc, 63);
        ci += tile & 0xffff;
        cj += tile >> 16;
    }
}

__global__ void __launch_bounds__(256) k_aln_fold(const AlnSumGroup *__restrict__ groups, int ngroups,
                                                  const int64_t *__restrict__ gcol, const int64_t *__restrict__ gbase,
                                                  const uint32_t *__restrict__ marks, const double *__restrict__ lut,
                                                  const double *__restrict__ errlut, double *__restrict__ out,
                                                  int64_t ncols)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ncols)
        return;
    int lo = 0, hi = ngroups - 1;   // the group whose columns hold e
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (gcol[mid] <= e)
            lo = mid;
        else
            hi = mid - 1;
    }
    const AlnSumGroup G = groups[lo];
    const int j = (int)(e - gcol[lo]);
    const uint32_t *col = marks + gbase[lo] + j;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int r = 0; r < G.r1 - G.r0; ++r) {
        const uint32_t rc = col[(int64_t)r * G.m];
        if (rc & 0x80000000u) {
            const int code = (int)(rc & 0xffff), sb = (int)((rc >> 16) & 0xff);
            const double ilp = lut[4 * code], el = errlut[code];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                acc[q] += q == sb ? ilp : el;
        }
    }
    double *o = out + G.out + (int64_t)j * 4;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        o[q] = acc[q];
}

// ---------------------------------------------------------------------
// k_scatter: one staged upload -> per-object device regions (a block per
// segment), so a batch upload is one H2D copy instead of one per object.
// ---------------------------------------------------------------------
struct alignas(16) Segment {
    int64_t src, dst, len;   // bytes
    int64_t pad;
};

__global__ void k_scatter(const Segment *__restrict__ segs, const uint8_t *__restrict__ src,
                          uint8_t *__restrict__ dst)
{
    const Segment S = segs[blockIdx.x];
    if ((S.src | S.dst | S.len) % 8 == 0) {
        const uint64_t *a = reinterpret_cast<const uint64_t *>(src + S.src);
        uint64_t *b = reinterpret_cast<uint64_t *>(dst + S.dst);
        for (int64_t e = threadIdx.x; e < S.len / 8; e += blockDim.x)
            b[e] = a[e];
    } else {
        for (int64_t e = threadIdx.x; e < S.len; e += blockDim.x)
            dst[S.dst + e] = src[S.src + e];
    }
}

// ---------------------------------------------------------------------
// k_tables: RifrafSequence tables (rifrafsequences.jl:19-82, no codon
// moves) and row-code records of phred-coded reads, built on the device
// from one byte per position (rf_set_sequences_codes).  Per code c the host
// passes lp[c], match[c] (its own libm values), and the dictionary ids of
// the (match, mismatch, ins) triple and of the del value lp[c] + s_del:
//   mismatch = lp + s_mis, ins = lp + s_ins,
//   del[0] = lp[0] + s_del, del[n] = lp[n-1] + s_del,
//   del[i] = max(lp[i-1], lp[i]) + s_del,
// the same FP64 additions and maximum as the host constructor, so the same
// bits.  One block per sequence.
// ---------------------------------------------------------------------
struct alignas(16) CodeSeq {
    int64_t tab;    // doubles offset of the sequence's tables
    int64_t src;    // byte offset of its codes / bases in the staged upload
    int32_t n, pad0;
    int64_t pad1;
};
struct alignas(16) CodeLut {   // per Phred code
    double lp, match;
    int32_t id3, id1;
    int32_t pad0, pad1;
};

__global__ void __launch_bounds__(256) k_tables(const CodeSeq *__restrict__ seqs, const uint8_t *__restrict__ codes,
                                                const uint8_t *__restrict__ bases, const CodeLut *__restrict__ lut,
                                                double s_mis, double s_ins, double s_del, double *__restrict__ tabs)
{
    const CodeSeq S = seqs[blockIdx.x];
    const int n = S.n;
    const uint8_t *cd = codes + S.src;
    const uint8_t *bs = bases + S.src;
    double *t = tabs + S.tab;
    uint64_t *rec = (uint64_t *)(t + row_code_off(n, 0, 0));
    for (int i = threadIdx.x; i <= n; i += blockDim.x) {
        const CodeLut L = lut[cd[min(i, n - 1)]];
        // del[i] and its dictionary id: the neighbour with the larger lp
        int idd;
        double dv;
        if (i == 0 || i == n) {
            dv = L.lp + s_del;
            idd = L.id1;
        } else {
            const CodeLut Lp = lut[cd[i - 1]];
            const double l = Lp.lp, r = L.lp;
            dv = (r > l ? r : l) + s_del;
            idd = r > l ? L.id1 : Lp.id1;
        }
        t[3 * (size_t)n + i] = dv;
        if (i < n) {
            t[i] = L.match;
            t[n + i] = L.lp + s_mis;
            t[2 * (size_t)n + i] = L.lp + s_ins;
        }
        // records need del[i] and del[i+1]: written by position i with the next id
        if (i < n) {
            int idn;
            if (i + 1 == n) {
                idn = L.id1;
            } else {
                const CodeLut Ln = lut[cd[i + 1]];
                idn = Ln.lp > L.lp ? Ln.id1 : L.id1;
            }
            rec[i] = (uint64_t)(uint32_t)L.id3 | ((uint64_t)(uint32_t)idd << 16) | ((uint64_t)(uint32_t)idn << 32) |
                     ((uint64_t)bs[i] << 48);
        }
    }
}

// Per-read setup values of the native driver from the staged Phred codes
// (round 5: formerly rf_host_code_prep's per-position host pass, which
// bounded a rank held to 2 host cores): one thread per sequence,
//   est[k]   = est_n_errors = sum(10^lp) in Julia 0.6's order
//              (rifrafsequences.jl:19-82, base/reduce.jl mapreduce_impl:
//              sequential below 1,024 elements, else pairwise halves);
//   ucode[k] = the code of the first maximal match score;
//   tsum[k]  = sum_i 10^(match[c_i] - match[ucode]) sequentially -- the
//              host finishes logsumexp10 = log10(tsum) + max with libm
//              (rf_host_lse_finish), so the initial consensus (model.jl:
//              575-579) is the one the host pass picks.
// The same table entries and the same FP64 additions in the same order as
// rf_host_code_prep: bit-identical.
constexpr int PREP_STACK = 40;
// sum_{i = lo..hi} tab[c[i]] left to right (the same additions in the same
// order as one loop), with eight entries loaded ahead of their additions:
// from LDS each element was two dependent round trips on lane 0's chain
__device__ __forceinline__ double prep_seq_sum(const uint8_t *c, const double *tab, int64_t lo, int64_t hi)
{
    double a = tab[c[lo]];
    int64_t i = lo + 1;
    for (; i + 8 <= hi + 1; i += 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u)
            v[u] = tab[c[i + u]];
#pragma unroll
        for (int u = 0; u < 8; ++u)
            a += v[u];
    }
    for (; i <= hi; ++i)
        a += tab[c[i]];
    return a;
}

__device__ double prep_julia_sum(const uint8_t *c, const double *p10, int64_t lo0, int64_t hi0)
{
    // explicit-stack post-order of the pairwise split (no device recursion)
    int64_t slo[PREP_STACK], shi[PREP_STACK];
    double sleft[PREP_STACK];
    int sst[PREP_STACK];
    int sp = 0;
    slo[0] = lo0;
    shi[0] = hi0;
    sst[0] = 0;
    double ret = 0.0;
    while (true) {
        const int64_t lo = slo[sp], hi = shi[sp];
        if (lo + 1024 > hi) {   // leaf: sequential
            ret = prep_seq_sum(c, p10, lo, hi);
            if (--sp < 0)
                return ret;
            continue;
        }
        const int64_t mid = (lo + hi) >> 1;
        if (sst[sp] == 0) {
            sst[sp] = 1;
            ++sp;
            slo[sp] = lo;
            shi[sp] = mid;
            sst[sp] = 0;
        } else if (sst[sp] == 1) {
            sleft[sp] = ret;
            sst[sp] = 2;
            ++sp;
            slo[sp] = mid + 1;
            shi[sp] = hi;
            sst[sp] = 0;
        } else {
            ret = sleft[sp] + ret;
            if (--sp < 0)
                return ret;
        }
    }
}

// One wave per sequence (round 5): the wave stages the sequence's codes in
// LDS with coalesced loads, and lane 0 runs the sequential sums from LDS (a
// thread per sequence read its codes one byte load at a time, dependent
// chains of global loads: 1.2 ms for configs[2]'s 1,000 reads).  The sums
// and their order are unchanged.
constexpr int CP_MAX = 32768;   // codes staged in LDS (longer sequences: read in place)
__global__ void __launch_bounds__(64) k_code_prep(const CodeSeq *__restrict__ seqs, int nseq,
                                                  const uint8_t *__restrict__ codes, const double *__restrict__ tabs3,
                                                  const double *__restrict__ grid, double *__restrict__ est,
                                                  int32_t *__restrict__ ucode, double *__restrict__ tsum)
{
    __shared__ double p10[256], mt[256], gr[256];
    __shared__ __attribute__((aligned(16))) uint8_t sc[CP_MAX];
    __shared__ int s_uc;
    for (int i = threadIdx.x; i < 256; i += 64) {
        p10[i] = tabs3[i];
        mt[i] = tabs3[256 + i];
    }
    const int k = blockIdx.x;
    if (k >= nseq)
        return;
    const CodeSeq S = seqs[k];
    const int64_t n = S.n;
    const uint8_t *cg = codes + S.src;
    if (n <= CP_MAX)
        for (int64_t i = threadIdx.x; i < n; i += 64)
            sc[i] = cg[i];
    __syncthreads();
    const uint8_t *c = n <= CP_MAX ? (const uint8_t *)sc : cg;
    // ucode: the code at the first position whose match score is maximal
    // (the sequential `if (mt[c_i] > mt[uc]) uc = c_i` scan), by a wave
    // reduction of (maximum, first position)
    {
        double best = -RF_INF;
        int64_t at = INT64_MAX;
        for (int64_t i = threadIdx.x; i < n; i += 64) {
            const double v = mt[c[i]];
            if (v > best) {   // strided: a lane's first maximum is its smallest position
                best = v;
                at = i;
            }
        }
        for (int off = 32; off >= 1; off >>= 1) {
            const double ob = __shfl_xor(best, off);
            const int64_t oa = __shfl_xor(at, off);
            if (ob > best || (ob == best && oa < at)) {
                best = ob;
                at = oa;
            }
        }
        if (threadIdx.x == 0) {
            const int uc = c[at == INT64_MAX ? 0 : at];
            est[k] = n <= 1024 ? prep_seq_sum(c, p10, 0, n - 1) : prep_julia_sum(c, p10, 0, n - 1);
            ucode[k] = uc;
            s_uc = uc;
        }
    }
    __syncthreads();
    const int uc = s_uc;
    for (int i = threadIdx.x; i < 256; i += 64)
        gr[i] = grid[(size_t)uc * 256 + i];
    __syncthreads();
    if (threadIdx.x == 0)
        tsum[k] = prep_seq_sum(c, gr, 0, n - 1);
}

// ---------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------

namespace {

// Every arena keeps ARENA_GUARD bytes before its first region and after its
// last: k_score_seg's LDS-DMA staging reads whole 16-B chunks of band rows
// and table rows, which may start up to one row before a region or end past
// it (values never used); the guards keep those reads inside the allocation.
constexpr int64_t ARENA_GUARD = 1 << 16;

struct Region {
    int64_t off = -1;  // bytes
    int64_t cap = 0;
};

struct Arena {
    char *d = nullptr;
    int64_t cap = 0, top = 0;
};

struct SeqObj {
    bool valid = false;
    bool finite = false;   // match / mismatch / ins / del tables hold no -Inf (lean DP eligible)
    bool coded = false;    // row codes written after the tables (RF_TASK_CODED)
    int32_t n = 0, ncins = 0, ncdel = 0;
    uint64_t version = 0;   // bumped by every upload of this id (tables, codes, codes_prep)
    Region bases, tabs;
};

struct TplObj {
    bool valid = false;
    int32_t m = 0;
    uint64_t version = 0;
    Region bases;
};

struct Band {
    bool valid = false;
    // the last fill this band was planned for raised (RF_ERR_NUMERIC): the
    // geometry stands and rf_download_band returns the cells, but no call
    // reads them as an alignment until a later fill of the band succeeds
    bool failed = false;
    int32_t seq = -1, tpl = -1, bw = 0, n = 0, m = 0, H = 0, flags = 0;
    int32_t P = 0;   // kappa row stride (band_stride at the fill)
    uint64_t tplver = 0;
    uint64_t seqver = 0;   // SeqObj::version at the fill
    Region r;
};

struct Slot {
    Band a, b;
};

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};

// The context's device buffers (rf_ctx::scratch), each named for what it
// holds.  Every buffer grows on demand (ensure_buf, upload) and is freed by
// rf_destroy.  All work on them is issued to the context's stream (launch_dp's
// side streams fork from it and join it again before launch_dp returns), and
// every exported call waits for that stream before it returns, so two calls
// never have work in flight at once: a buffer with two users (X_OR_Y) holds
// one content at a time, in stream order.  A new user takes a new enumerator.
// A call that lands results or the error flag in the pinned zone waits in
// land_wait, behind its last launch and copy (the landing helpers, below).
// The calls that wait elsewhere, with a stream_wait of their own: realign_run
// (the flag's copy goes first) and rf_score (its pageable per-read downloads
// follow the flag's copy); the calls whose results go straight to the caller
// -- score_dense_impl, rf_score_dense_ref, rf_internal_aln_sums_dev (before
// its check_err) and rf_qv_probs; pair_download, for every set; and the
// uploads: tables_chunk and set_sequences_codes_impl after every chunk,
// rf_set_templates*.  An entry point that returned with work in flight would
// have to take buffers of its own, and a context serves one call at a time.
enum Buf : int {
    BUF_SCORE_ITEMS,    // rf_score: WorkItem
    BUF_SCORE_GROUPS,   // rf_score: ScoreGroup
    // rf_score: ScoreRead | rf_alignment_proposals: the proposal mask its walks mark
    BUF_READS_OR_MASK,
    // The backtrace's moves (n + m bytes per slot, at BTTask::out) and its
    // counts (nmoves, then nerrors, per slot): sized by build_bt_tasks,
    // written by launch_backtraces' k_bt_win, read by rf_backtrace's downloads
    // and by rf_internal_aln_sums_dev's k_aln_marks / k_aln_sums.  Writer and
    // reader run inside the same exported call (rf_backtrace,
    // rf_alignment_proposals, rf_aln_error_sums, rf_qv_probs), on the stream.
    // | rf_score: CodonTask (moves) and its proposal block -- pgroup, pos,
    // kind, base, the per-group flags and gstart (counts).
    BUF_MOVES_OR_CTASKS,
    BUF_COUNTS_OR_PROPS,
    // Segment of the sequence and template uploads (scatter_staged, for
    // tables_chunk, set_sequences_codes_impl and rf_set_templates*);
    // tables_chunk uses it twice and waits for the stream in between | rf_score: its work block
    // (dense totals, split partials, k_codon's columns and outputs, totals)
    BUF_SEGS_OR_WORK,
    // tables_chunk: the staged tables | set_sequences_codes_impl: CodeSeq;
    // each waits for the stream after every chunk
    BUF_TABS_OR_CSEQS,
    // the staged bases of the sequence and template uploads (with
    // set_sequences_codes_impl, the codes behind them) | launch_dp: the sink the
    // lean kernels' padding tasks store to (written, never read)
    BUF_BYTES_OR_SINK,
    BUF_DP_TASKS,    // rf_realign: DPTask in device order; kept while rf_ctx::rplan is valid
    BUF_DP_SCORES,   // rf_realign: two scores per job
    // launch_dp: k_dp's global anti-diagonal ring (DpwLds / DpwGlobal launches)
    // | score_dense_impl: the split partials k_reduce folds
    BUF_RING_OR_SPLIT,
    // score_dense_impl: WorkItem, ScoreGroup, ScoreRead and gstart; kept while rf_ctx::dplan is valid
    BUF_DENSE_ITEMS,
    BUF_DENSE_GROUPS,
    BUF_DENSE_READS,
    BUF_DENSE_GSTART,
    // The dense totals, (m + 1) x 9 per group at dplan's dense_off: written by
    // score_dense_impl, then folded into by rf_score_dense_ref's k_codon_dense
    // or read by rf_qv_probs' k_qv -- inside the exported call that ran
    // score_dense_impl, on the stream.
    BUF_DENSE_TOTALS,
    BUF_BT_TASKS,     // launch_backtraces: BTTask
    BUF_ALN_READS,    // rf_internal_aln_sums_dev: AlnSumRead
    BUF_ALN_GROUPS,   // rf_internal_aln_sums_dev: AlnSumGroup
    // The alignment sums, m x 4 per group: written by rf_internal_aln_sums_dev
    // (k_aln_fold / k_aln_sums), downloaded by it or read by rf_qv_probs' k_qv
    // -- inside the rf_qv_probs call that ran it, on the stream.
    BUF_ALN_SUMS,
    BUF_CODE_LUTS,   // set_sequences_codes_impl: CodeLut (code_tables)
    // rf_internal_aln_sums_dev's two-launch path: the reads' mark offsets, the
    // groups' column and mark offsets, the marks
    BUF_ALN_READ_BASE,
    BUF_ALN_GROUP_COL,
    BUF_ALN_GROUP_BASE,
    BUF_ALN_MARKS,
    BUF_QV_GROUPS,   // rf_qv_probs: QvGroup
    BUF_QV_OUT,      // rf_qv_probs: pos, ins and aln probabilities, the groups' error codes
    BUF_CODE_PREP,   // rf_set_sequences_codes_prep: p10 | match tables, the grid, est / tsum / ucode
    // one launch set of the pair calls (pair_run): DPTask and scores; the move
    // trace, the moves, their offsets, and the counts (nmoves, then nerrors)
    BUF_PAIR_TASKS,
    BUF_PAIR_SCORES,
    BUF_PAIR_TRACE,
    BUF_PAIR_MOVES,
    BUF_PAIR_MOVE_OFF,
    BUF_PAIR_COUNTS,
    BUF_CODON_GROUPS,   // rf_score_dense_ref: CodonDenseGroup
    // k_pa_emit's products for one launch set: the two texts, the index maps,
    // their offsets, and aln_len / t2s_len / tolerance
    BUF_PAIR_TEXT_T,
    BUF_PAIR_TEXT_S,
    BUF_PAIR_INDEX,
    BUF_PAIR_INDEX_OFF,
    BUF_PAIR_LENGTHS,
    // k_pa_fix's products for one launch set: the corrected templates, the
    // proposal records (kind | base << 4, pos) with their offsets, and
    // fixed_len / nprops / the five tallies
    BUF_PAIR_FIXED,
    BUF_PAIR_PROP_KB,
    BUF_PAIR_PROP_POS,
    BUF_PAIR_PROP_OFF,
    BUF_PAIR_FIX_OUT,
    // The candidate calls (cand_run, which waits for the stream after its
    // downloads).  The proposal mask of rf_candidates, (m + 1) x 9 bytes per
    // group at dplan's dense_off: the caller's rows of source 4, marked on top
    // by the walks of sources 1 and 2, read by k_cand_select / k_cand_choose
    // and never downloaded | rf_candidates_table: the caller's mask
    BUF_CAND_MASK,
    BUF_CAND_GROUPS,   // CandGroup
    // the counts (ncand, then nchosen, per group), the chosen records, the
    // candidate records: one download
    BUF_CAND_OUT,
    BUF_CAND_TABLE,    // rf_candidates_table: the caller's table
    BUF_CAND_CONS,     // rf_candidates_table: the caller's consensus bases
    // the wide pair class of one launch set (RF_OPT_PAIR_WIDE): its workgroups'
    // rings of four anti-diagonals, the scores and behind them k_pe_wide's counts
    BUF_PAIR_RING,
    BUF_COUNT
};

// The context's timing events (rf_ctx::ev), each named for the point on the
// stream that it marks.  A call records its marks around its launches and
// reads the time between two of them (mark_ms) after its stream wait.  A new
// point takes a new enumerator.
enum Ev : int {
    EV_DP_BEGIN,   // rf_realign: around launch_dp
    EV_DP_END,
    EV_SCORER_BEGIN,   // rf_score and score_dense_impl: before the scorer (and k_reduce)
    EV_CODON_BEGIN,    // rf_score: before k_codon
    EV_SCORER_END,     // after the scorer and k_codon; rf_score's k_gather begins here
    EV_GATHER_END,     // rf_score: after k_gather
    EV_WALKS_BEGIN,    // launch_backtraces: around k_bt_win (and its descriptor upload)
    EV_WALKS_END,
    EV_CODON_DENSE_BEGIN,   // rf_score_dense_ref: around k_codon_dense
    EV_CODON_DENSE_END,
    EV_PAIR_FILL_BEGIN,   // a launch set of the pair calls: the fills, the walk, k_pa_emit
    EV_PAIR_FILL_END,
    EV_PAIR_WALK_END,
    EV_PAIR_EMIT_END,
    EV_PAIR_FIX_END,      // ... or k_pa_fix, from EV_PAIR_WALK_END
    EV_PAIR_ERRORS_BEGIN,   // a launch set of rf_pair_errors: around the counting fills (k_pe*)
    EV_PAIR_ERRORS_END,
    EV_CAND_SELECT_BEGIN,   // cand_run: k_cand_select, then k_cand_choose
    EV_CAND_CHOOSE_BEGIN,
    EV_CAND_CHOOSE_END,
    EV_COUNT
};

}  // namespace

// Host worker threads: OMP_NUM_THREADS when set (the GPU box's CPU share),
// else the machine's, at most 16, and never more than the CPUs this thread
// may run on (sched_getaffinity, read per call: a rank pinned to its share of
// the host's cores -- e.g. 2 of 16 at 8 ranks -- gets that many workers).
// Shared with rifraf_batch.cpp (C++ linkage, not part of the C-ABI).
int rf_internal_host_threads()
{
    static const int cap = [] {
        const char *v = std::getenv("OMP_NUM_THREADS");
        int t = (v && *v) ? std::atoi(v) : (int)std::thread::hardware_concurrency();
        return std::max(1, std::min(t, 16));
    }();
    cpu_set_t cs;
    CPU_ZERO(&cs);
    if (sched_getaffinity(0, sizeof(cs), &cs) == 0)
        return std::max(1, std::min(cap, (int)CPU_COUNT(&cs)));
    return cap;
}

namespace {
inline int host_threads() { return rf_internal_host_threads(); }
// parallel_for, CodeDict: rifraf_seq_upload.h.  The context's dictionary with
// its device copies: `lut` (RF_CODES x 4 triple doubles, then RF_CODES del
// doubles, filled by send_dictionary) and `errlut` (CodeDict::errv).
struct DevCodeDict : CodeDict {
    DevBuf lut, errlut;
};

// Tuning options (rf_set_option keys, include/rifraf_hip.h).  Every option
// selects between bit-identical code paths; defaults come from the RIFRAF_*
// environment once, at rf_create, and never from a hot path.
// The launch planners' options are DpOpts (rifraf_dp_plan.h) and ScoreOpts
// (rifraf_score_plan.h).
struct Opts : DpOpts, ScoreOpts {
    int band_pad_h = 64;    // RF_OPT_BAND_PAD: a realign call whose widest band has H >= this gets
                            // 128-B-line rows for all its bands (0: never, 1: always)
    int bt_win_kb = 16;     // RF_OPT_BT_WIN_KB: k_bt_win A window (16 or 32 KB of LDS)
    int stage_kb = 262144;  // RF_OPT_STAGE_KB: rf_set_sequences staging chunk (KB of tables)
    int aln_sums_host = 0;  // RF_OPT_ALN_SUMS_HOST: 1 = rf_aln_error_sums folds the moves on the host
    int aln_marks_min = 128;   // RF_OPT_ALN_MARKS_MIN: device QV sums in two launches above this many reads per group
    int sync_block = 2;     // RF_OPT_SYNC_BLOCK: 1 host waits yield / sleep instead of spinning; 2 (default)
                            // auto: when the waiting thread may run on fewer than 4 CPUs
    int score_wgs = 2048;   // RF_OPT_SCORE_WGS: split-mode k_score_ws takes reads in chunks so that about
                            // this many workgroups remain
    int seg_wgs = 262144;   // RF_OPT_SEG_WGS: split-mode k_score_segl takes reads in chunks so that about
                            // this many workgroups remain
    int bt_nw = 4;          // RF_OPT_BT_NW: waves per walk in launches of at most BTW_FEW walks (4 or 1)
    int pair_chunk = PS_CHUNK;   // RF_OPT_PAIR_CHUNK: pairs per launch set of rf_pair_scores / rf_pair_align
    int pair_trace_mb = PA_TRACE_MB;   // RF_OPT_PAIR_TRACE_MB: MB of move trace per launch set of rf_pair_align
    int pair_walk = 0;                 // RF_OPT_PAIR_WALK: 0 auto, 1 k_pa_walk (lane per pair), 2 k_pa_walk_w (wave per pair)
    int cand_device = 0;    // RF_OPT_CAND_DEVICE: 1 = the native driver selects and chooses candidates with rf_candidates
    int pair_wide = 0;      // RF_OPT_PAIR_WIDE: 0 bands past DPW_LDS_H refused, 1 in the wide tier, v >= 2 also every band of >= v rows
    int pair_ring_mb = PW_RING_MB;   // RF_OPT_PAIR_RING_MB: MB of the wide tier's rings per launch set (0: one workgroup)
};

}  // namespace

struct rf_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t side[3] = {};   // concurrent DP class launches (fork/join on `stream`)
    hipEvent_t ev[EV_COUNT] = {};   // by Ev: the point on the stream each marks
    hipEvent_t fork = nullptr, join[3] = {};
    std::string err;
    Arena bytes_arena;  // sequence + template bases
    Arena tab_arena;    // sequence tables
    Arena band_arena;   // A / B bands
    DevCodeDict codes;  // row-code dictionary (RF_TASK_CODED)
    std::vector<SeqObj> seqs;
    std::vector<TplObj> tpls;
    std::vector<Slot> slots;
    uint64_t tpl_counter = 0;
    uint64_t seq_counter = 0;
    uint64_t layout_gen = 1;   // bumped whenever a device offset / length may change
    int64_t arena_grows = 0;   // arena_grow calls and their wall seconds (RIFRAF_BATCH_TIMING)
    double arena_grow_s = 0.0;
    // bumped by every call that changes sequences, templates or band metadata:
    // a plan validated at the current epoch with the same job / slot list
    // needs no per-slot validation again
    uint64_t state_epoch = 1;
    DevBuf scratch[BUF_COUNT];   // by Buf: what each holds, and who shares it
    // pinned host staging for sequence uploads (pageable H2D copies of a few
    // MB took ~14 ms per cluster upload on the box: page locking per call)
    void *pinned = nullptr;
    size_t pinned_bytes = 0;
    // pinned ring for the per-call descriptor uploads (upload()): the runtime
    // stages a pageable H2D copy through a blit of its own
    void *up = nullptr;
    size_t up_bytes = 0, up_off = 0;
    // pinned landing zone for every call's downloads (ensure_landing): the
    // error flag at 0, results from HDN_RES
    void *hdn = nullptr;
    size_t hdn_bytes = 0;
    DevBuf grow_segs;   // compaction descriptors (arena_grow may run inside other uploads)
    int *d_err = nullptr;
    double dp_ms = 0, score_ms = 0, gather_ms = 0, bt_ms = 0;
    double codon_ms = 0;        // k_codon of the last rf_score (inside score_ms)
    double codon_dense_ms = 0;  // k_codon_dense of the last rf_score_dense_ref (inside score_ms)
    double pair_ms = 0;         // kernels of the last rf_pair_scores
    double pa_fill_ms = 0, pa_walk_ms = 0;   // fills / walks of the last rf_pair_align
    double pa_emit_ms = 0;                   // k_pa_emit of the last rf_pair_align_text
    double pa_fix_ms = 0;                    // k_pa_fix of the last rf_pair_shifts
    double pe_ms = 0;                        // kernels of the last rf_pair_errors
    double cand_select_ms = 0, cand_choose_ms = 0;   // k_cand_select / k_cand_choose of the last candidate call
    hipEvent_t ev_block = nullptr;   // blocking-sync event (RF_OPT_SYNC_BLOCK)
    Opts opt;
    uint64_t opt_gen = 0;      // bumped by rf_set_option (scorer plan key)
    std::vector<BTTask> bt_win;   // backtrace descriptors of the last launch
    // host-side plan caches: a repeated call with identical arguments and an
    // unchanged layout reuses the uploaded descriptors (steady-state loops)
    struct {
        bool valid = false;
        uint64_t gen = 0;
        uint64_t val_epoch = 0;   // state_epoch at which the job list was last validated
        std::vector<int32_t> slot, seq, tpl, bw, flags;   // flags: per job (rf_realign_jobs)
        DpPlan dp;   // host copy of the uploaded descriptors, and their launches
    } rplan;
    std::vector<DpLaunch> last_dp;   // launches of the last successful rf_realign (rf_last_dp_launches)
    std::vector<int32_t> jflags;   // rf_realign: the call's flags for every job
    struct {
        bool valid = false;
        uint64_t gen = 0;
        uint64_t val_epoch = 0;   // state_epoch at which the slot list was last validated
        std::vector<int32_t> slot_off, slots;
        int ngroups = 0;
        uint64_t opt_gen = 0;
        // host copy of the uploaded descriptors: alive until the uploads it
        // sources have completed (hipMemcpyAsync from pageable memory)
        ScorePlan plan;
    } dplan;
    int32_t last_score[RF_SCL_FIELDS] = {};   // the last successful scoring call's launch (rf_last_score_launch)
};

namespace {

const char *numeric_message(int code)
{
    switch (code) {
    case 1: return "new score is invalid";
    case 2: return "failed to find a move";
    case 3: return "failed to compute a valid score";
    case 4: return "internal error: a band slice's neighbour never arrived (k_dpm)";
    default: return "numeric error";
    }
}

int fail(rf_ctx *ctx, int code, const std::string &msg)
{
    if (ctx)
        ctx->err = msg;
    return code;
}

// A band filled from a sequence id that was uploaded again since: its cells
// belong to the old content (and length), the id's tables and bases to the new.
bool seq_stale(const rf_ctx *ctx, const Band &b)
{
    return b.seq < 0 || b.seq >= (int32_t)ctx->seqs.size() || ctx->seqs[b.seq].version != b.seqver;
}

// The refusal of a band whose last fill raised (Band::failed).
const char *const FILL_FAILED = "the last fill of this band failed";

#define HIPCHK(ctx, call)                                                          \
    do {                                                                           \
        hipError_t e_ = (call);                                                    \
        if (e_ != hipSuccess)                                                      \
            return fail((ctx), RF_ERR_HIP,                                         \
                        std::string(#call ": ") + hipGetErrorString(e_));          \
    } while (0)

int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

// The host's wait for the context's stream.  HIP's stream synchronize spins
// on the completion signal; with RF_OPT_SYNC_BLOCK the thread yields its core
// and then sleeps between polls of an event instead, so a rank held to a
// 2-core share leaves the core to its other host work (quality pass, table
// setup, another engine's thread) while its kernels run.  (Round 6: a
// blocking-sync hipEventSynchronize kept the waiting thread on its core --
// the native stage machine's thread CPU time equalled its wall time,
// profiles/r06e_e2e_phases.out.)  2: auto, block when this thread may run on
// fewer than 4 CPUs.
bool host_blocks(const rf_ctx *ctx)
{
    if (ctx->opt.sync_block == 2) {
        cpu_set_t cs;
        return sched_getaffinity(0, sizeof(cs), &cs) == 0 && CPU_COUNT(&cs) < 4;
    }
    return ctx->opt.sync_block == 1;
}

hipError_t stream_wait(rf_ctx *ctx)
{
    if (!ctx->ev_block || !host_blocks(ctx))
        return hipStreamSynchronize(ctx->stream);
    hipError_t e = hipEventRecord(ctx->ev_block, ctx->stream);
    if (e != hipSuccess)
        return e;
    const auto t0 = std::chrono::steady_clock::now();
    while ((e = hipEventQuery(ctx->ev_block)) == hipErrorNotReady) {
        if (std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(200))
            sched_yield();
        else
            std::this_thread::sleep_for(std::chrono::microseconds(30));
    }
    return e;
}

// before a device-to-host copy into host memory that may be pageable (HIP
// then copies through a staging buffer and spins until the stream reaches
// the copy): a blocking host waits for the stream first, so the copy is
// short
hipError_t pre_d2h(rf_ctx *ctx)
{
    return host_blocks(ctx) ? stream_wait(ctx) : hipSuccess;
}

// a context buffer as an array of T
template <class T>
T *dev(const rf_ctx *ctx, Buf b)
{
    return (T *)ctx->scratch[b].p;
}

int ensure_buf(rf_ctx *ctx, DevBuf &b, size_t bytes)
{
    if (b.cap >= bytes)
        return 0;
    if (b.p) {
        HIPCHK(ctx, stream_wait(ctx));
        HIPCHK(ctx, hipFree(b.p));
    }
    size_t cap = std::max<size_t>(bytes + bytes / 4, 1 << 16);
    HIPCHK(ctx, hipMalloc(&b.p, cap));
    b.cap = cap;
    return 0;
}

#ifndef RF_UP_RING
#define RF_UP_RING (32 << 20)   // bytes of the pinned upload ring (0: pageable copies)
#endif
// `bytes` of the pinned upload ring for one H2D copy on the context's stream
// (*h = nullptr: too large for the ring, copy from pageable memory)
int ring_take(rf_ctx *ctx, size_t bytes, char **h)
{
    *h = nullptr;
    if (RF_UP_RING <= 0 || bytes > (size_t)RF_UP_RING / 4)
        return 0;
    if (!ctx->up) {
        if (hipHostMalloc(&ctx->up, RF_UP_RING, hipHostMallocDefault) != hipSuccess)
            return fail(ctx, RF_ERR_HIP, "pinned upload ring allocation failed");
        ctx->up_bytes = RF_UP_RING;
        ctx->up_off = 0;
    }
    const size_t need = (bytes + 255) & ~(size_t)255;
    if (ctx->up_off + need > ctx->up_bytes) {
        // every copy out of the ring is on this stream: once it drains, the
        // ring is free again
        HIPCHK(ctx, stream_wait(ctx));
        ctx->up_off = 0;
    }
    *h = (char *)ctx->up + ctx->up_off;
    ctx->up_off += need;
    return 0;
}

// H2D copy of host memory into a context buffer, through the pinned ring when
// it fits; else `src` sources the copy until the call's stream wait
int upload(rf_ctx *ctx, DevBuf &b, const void *src, size_t bytes)
{
    if (int e = ensure_buf(ctx, b, std::max<size_t>(bytes, 16)))
        return e;
    if (!bytes)
        return 0;
    char *h;
    if (int e = ring_take(ctx, bytes, &h))
        return e;
    if (h)
        std::memcpy(h, src, bytes);
    HIPCHK(ctx, hipMemcpyAsync(b.p, h ? (const void *)h : src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return 0;
}

template <class T>
int upload(rf_ctx *ctx, DevBuf &b, const std::vector<T> &v)
{
    return upload(ctx, b, v.data(), v.size() * sizeof(T));
}

// Collect every live region of an arena, for compaction.
void live_regions(rf_ctx *ctx, Arena *a, std::vector<Region *> &out)
{
    out.clear();
    if (a == &ctx->bytes_arena) {
        for (auto &s : ctx->seqs)
            if (s.bases.off >= 0) out.push_back(&s.bases);
        for (auto &t : ctx->tpls)
            if (t.bases.off >= 0) out.push_back(&t.bases);
    } else if (a == &ctx->tab_arena) {
        for (auto &s : ctx->seqs)
            if (s.tabs.off >= 0) out.push_back(&s.tabs);
    } else {
        for (auto &s : ctx->slots) {
            if (s.a.r.off >= 0) out.push_back(&s.a.r);
            if (s.b.r.off >= 0) out.push_back(&s.b.r);
        }
    }
}

// Grow (and compact) an arena so that `need` more bytes fit at the top.
// `skip` is a region about to be rewritten: its content is not preserved.
int arena_grow_impl(rf_ctx *ctx, Arena &a, int64_t need, Region *skip);
int arena_grow(rf_ctx *ctx, Arena &a, int64_t need, Region *skip)
{
    const auto t0 = std::chrono::steady_clock::now();
    const int e = arena_grow_impl(ctx, a, need, skip);
    ctx->arena_grow_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    ++ctx->arena_grows;
    return e;
}

// The capacity an arena of old_cap bytes gets when `want` bytes of regions
// must fit: the guards, half as much again as before at least, and a margin
// of an eighth plus 1 MiB, in whole MiB.  rf_host_reserve_fit inverts it.
static int64_t arena_capacity(int64_t want, int64_t old_cap)
{
    const int64_t cap = std::max<int64_t>(want + 2 * ARENA_GUARD, (int64_t)(old_cap * 1.5));
    return align_up(cap + cap / 8 + (1 << 20), 1 << 20);
}

int arena_grow_impl(rf_ctx *ctx, Arena &a, int64_t need, Region *skip)
{
    std::vector<Region *> regs;
    live_regions(ctx, &a, regs);
    int64_t live = 0;
    for (auto *r : regs)
        if (r != skip)
            live += r->cap;
    const int64_t cap = arena_capacity(live + need, a.cap);
    char *d = nullptr;
    HIPCHK(ctx, hipMalloc((void **)&d, cap));
    std::sort(regs.begin(), regs.end(), [](Region *x, Region *y) { return x->off < y->off; });
    // compaction = one scatter launch (one block per live region), not one
    // copy dispatch per region: a batch upload that grows an arena log(N)
    // times would otherwise issue O(N log N) tiny copies
    std::vector<Segment> segs;
    segs.reserve(regs.size());
    int64_t top = ARENA_GUARD;   // guard bytes before the first region
    for (auto *r : regs) {
        if (r == skip) {
            r->off = -1;
            r->cap = 0;
            continue;
        }
        if (r->cap > 0)
            segs.push_back({r->off, top, r->cap, 0});
        r->off = top;
        top += r->cap;
    }
    if (!segs.empty()) {
        if (int e = upload(ctx, ctx->grow_segs, segs))
            return e;
        hipLaunchKernelGGL(k_scatter, dim3((unsigned)segs.size()), dim3(256), 0, ctx->stream,
                           (const Segment *)ctx->grow_segs.p, (const uint8_t *)a.d, (uint8_t *)d);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, stream_wait(ctx));
    if (a.d)
        HIPCHK(ctx, hipFree(a.d));
    a.d = d;
    a.cap = cap;
    a.top = top;
    ++ctx->layout_gen;
    return 0;
}

int region_ensure(rf_ctx *ctx, Arena &a, Region &r, int64_t bytes)
{
    bytes = region_bytes(bytes);
    if (r.off >= 0 && r.cap >= bytes)
        return 0;
    if (a.top + bytes + ARENA_GUARD > a.cap)
        if (int e = arena_grow(ctx, a, bytes, &r))
            return e;
    r.off = a.top;
    r.cap = bytes;
    a.top += bytes;
    ++ctx->layout_gen;
    return 0;
}

// The landing zone: every call's downloads land in ctx->hdn (pinned: a
// pageable D2H copy is staged by the runtime through a blit and a wait of its
// own), the error flag at offset 0 and the results from HDN_RES.  A call
// sizes the zone (ensure_landing), queues its results (land) and the flag
// (land_flag) behind its kernels, waits for the stream once, reads the flag
// (check_landed) and copies the results out (landed).  Offsets are bytes from
// HDN_RES; a call with several parts keeps each 16-byte aligned.
// pre_d2h goes before the copies of every call but realign_run, whose copies
// all go to pinned memory and which never called it.
constexpr size_t HDN_RES = 16;
int ensure_landing(rf_ctx *ctx, size_t bytes)
{
    const size_t want = HDN_RES + bytes;
    if (ctx->hdn_bytes >= want)
        return 0;
    if (ctx->hdn) {
        HIPCHK(ctx, stream_wait(ctx));
        (void)hipHostFree(ctx->hdn);
    }
    ctx->hdn = nullptr;
    ctx->hdn_bytes = 0;
    const size_t sz = std::max<size_t>(want + want / 4, 1 << 20);
    if (hipHostMalloc(&ctx->hdn, sz, hipHostMallocDefault) != hipSuccess)
        return fail(ctx, RF_ERR_HIP, "pinned download buffer allocation failed");
    ctx->hdn_bytes = sz;
    return 0;
}

// the landed bytes at offset `at`, as an array of T
template <class T>
const T *landed(const rf_ctx *ctx, size_t at = 0)
{
    return (const T *)((const char *)ctx->hdn + HDN_RES + at);
}

// queue the download of `bytes` at `src` on the device to offset `at`
hipError_t land(rf_ctx *ctx, size_t at, const void *src, size_t bytes)
{
    return hipMemcpyAsync((char *)ctx->hdn + HDN_RES + at, src, bytes, hipMemcpyDeviceToHost, ctx->stream);
}

// queue the error flag's copy
hipError_t land_flag(rf_ctx *ctx)
{
    return hipMemcpyAsync(ctx->hdn, ctx->d_err, sizeof(int), hipMemcpyDeviceToHost, ctx->stream);
}

// the end of a call's stream work: the flag behind everything queued so far,
// then the call's one wait
hipError_t land_wait(rf_ctx *ctx)
{
    const hipError_t e = land_flag(ctx);
    return e != hipSuccess ? e : stream_wait(ctx);
}

// after the wait: the landed error flag; a raised one is cleared on the device
int check_landed(rf_ctx *ctx)
{
    const int h = *(const int *)ctx->hdn;
    if (h) {
        int z = 0;
        HIPCHK(ctx, hipMemcpy(ctx->d_err, &z, sizeof(int), hipMemcpyHostToDevice));
        return fail(ctx, RF_ERR_NUMERIC, numeric_message(h));
    }
    return 0;
}

// the whole call end of a call that lands nothing but the flag
int check_err(rf_ctx *ctx)
{
    if (int e = ensure_landing(ctx, 0))
        return e;
    HIPCHK(ctx, pre_d2h(ctx));
    HIPCHK(ctx, land_wait(ctx));
    return check_landed(ctx);
}

// milliseconds between two marks of the stream, after the wait (0 if the query fails)
double mark_ms(const rf_ctx *ctx, Ev a, Ev b)
{
    float ms = 0;
    return hipEventElapsedTime(&ms, ctx->ev[a], ctx->ev[b]) == hipSuccess ? ms : 0.0;
}

int env_int(const char *name, int dflt)
{
    const char *v = std::getenv(name);
    return (v && *v) ? std::atoi(v) : dflt;
}

// option defaults from the environment (rf_create only)
void load_env_opts(Opts &o)
{
    if (const char *k = std::getenv("RIFRAF_SCORE_KERNEL"))
        o.score_kernel = !std::strcmp(k, "general") ? 1 : !std::strcmp(k, "seg") ? 2 : !std::strcmp(k, "ws") ? 3 : 0;
    if (const char *m = std::getenv("RIFRAF_SCORE_MODE"))
        o.score_mode = !std::strcmp(m, "fused") ? 1 : !std::strcmp(m, "split") ? 2 : 0;
    o.lean_lds_kb = env_int("RIFRAF_LEAN_LDS_KB", o.lean_lds_kb);
    o.dp_psplit = env_int("RIFRAF_DP_PSPLIT", o.dp_psplit);
    o.dp_np8 = env_int("RIFRAF_DP_NO_NP8", 0) ? 0 : 1;
    o.dp_np8_lean = env_int("RIFRAF_DP_NP8_LEAN", o.dp_np8_lean);
    o.dp_streams = env_int("RIFRAF_DP_STREAMS", o.dp_streams);
    o.bt_win_kb = env_int("RIFRAF_BT_WIN_KB", o.bt_win_kb);
    o.band_pad_h = env_int("RIFRAF_BAND_PAD", o.band_pad_h);
    o.dp_wide = env_int("RIFRAF_DP_WIDE", o.dp_wide);
    o.aln_sums_host = env_int("RIFRAF_ALN_SUMS_HOST", o.aln_sums_host);
    o.sync_block = env_int("RIFRAF_SYNC_BLOCK", o.sync_block);
    o.dp_nl64 = env_int("RIFRAF_DP_NL64", o.dp_nl64);
    o.dp_lat = env_int("RIFRAF_DP_LAT", o.dp_lat);
    o.score_wgs = env_int("RIFRAF_SCORE_WGS", o.score_wgs);
    o.seg_wgs = env_int("RIFRAF_SEG_WGS", o.seg_wgs);
    o.dp_pfit = env_int("RIFRAF_DP_PFIT", o.dp_pfit);
    o.dp_mc = env_int("RIFRAF_DP_MC", o.dp_mc);
    o.bt_nw = env_int("RIFRAF_BT_NW", o.bt_nw);
    o.pair_trace_mb = env_int("RIFRAF_PAIR_TRACE_MB", o.pair_trace_mb);
    o.pair_walk = env_int("RIFRAF_PAIR_WALK", o.pair_walk);
    o.cand_device = env_int("RIFRAF_CAND_DEVICE", o.cand_device);
}

// Launches the picked scorer over nitems items (split: partials of gy reads,
// rchunk of them per workgroup); returns the launch's grid.y.  from (fused
// launches of rf_score_dense_from): the fold continues from the totals
// already in `dense` (the INIT instantiations); a split launch writes
// partials as ever and k_reduce<true> takes the initial value
unsigned launch_scorer(rf_ctx *ctx, const ScorePick &pk, unsigned nitems, unsigned gy, const WorkItem *items,
                   const ScoreGroup *groups, const ScoreRead *reads, double *dense, double *split,
                   bool from = false)
{
    const uint8_t *d_bases = (const uint8_t *)ctx->bytes_arena.d;
    const double *d_tabs = (const double *)ctx->tab_arena.d;
    const double *d_bands = (const double *)ctx->band_arena.d;
    int sm = split ? 1 : 0;
    dim3 grid(nitems, gy);
    // split: gy is the launch's max_reads (score_chunks, csrc/rifraf_score_plan.h)
    const ScoreChunks ch = score_chunks(pk.family(), sm != 0, nitems, gy, ctx->opt.score_wgs, ctx->opt.seg_wgs);
    if (sm)
        grid.y = ch.grid_y;
    if (from && !sm) {
        if (pk.seg) {
            hipLaunchKernelGGL((k_score_segl<32, true>), grid, dim3(64), 0, ctx->stream, items, groups, reads, d_bases,
                               d_tabs, d_bands, dense, split, sm, ch.rchunk);
        } else if (!pk.lean) {
            hipLaunchKernelGGL(k_score<true>, grid, dim3(128), 2 * pk.lds * 8, ctx->stream, items, groups, reads,
                               d_bases, d_tabs, d_bands, dense, split, sm, pk.lds);
        } else {
            hipLaunchKernelGGL((k_score_ws<WS_NPF, 256, true>), grid, dim3(512), pk.lds * 8, ctx->stream, items,
                               groups, reads, d_bases, d_tabs, d_bands, dense, split, sm, pk.lds,
                               WS_CODES ? (const double *)ctx->codes.lut.p : nullptr, ch.rchunk);
        }
        return grid.y;
    }
    if (pk.seg) {
        hipLaunchKernelGGL(k_score_segl<32>, grid, dim3(64), 0, ctx->stream, items, groups, reads, d_bases, d_tabs,
                           d_bands, dense, split, sm, ch.rchunk);
    } else if (!pk.lean) {
        hipLaunchKernelGGL(k_score<false>, grid, dim3(128), 2 * pk.lds * 8, ctx->stream, items, groups, reads,
                           d_bases, d_tabs, d_bands, dense, split, sm, pk.lds);
    } else {
        hipLaunchKernelGGL((k_score_ws<WS_NPF, 256>), grid, dim3(512), pk.lds * 8, ctx->stream, items,
                           groups, reads, d_bases, d_tabs, d_bands, dense, split, sm, pk.lds,
                           WS_CODES ? (const double *)ctx->codes.lut.p : nullptr, ch.rchunk);
    }
    return grid.y;
}

void note_score_launch(rf_ctx *ctx, const ScorePick &pk, bool split, size_t nitems, unsigned gy)
{
    const int32_t rec[RF_SCL_FIELDS] = {pk.family(), split ? 1 : 0, (int32_t)nitems, (int32_t)gy};
    std::copy(rec, rec + RF_SCL_FIELDS, ctx->last_score);
}

// Why slot s cannot be scored (NULL: it can): A and B both filled, neither
// fill failed, both for one alignment at one row stride, and neither the
// template nor the sequence replaced since
const char *score_band_fault(const rf_ctx *ctx, int32_t s)
{
    if (s < 0 || s >= (int32_t)ctx->slots.size())
        return "unknown slot";
    const Slot &S = ctx->slots[s];
    if (!S.a.valid || !S.b.valid)
        return "slot has no A/B bands";
    if (S.a.failed || S.b.failed)
        return FILL_FAILED;
    if (S.a.seq != S.b.seq || S.a.tpl != S.b.tpl || S.a.bw != S.b.bw || S.a.tplver != S.b.tplver ||
        S.a.m != S.b.m || S.a.seqver != S.b.seqver || S.a.n != S.b.n)
        return "A and B bands were computed for different alignments";
    if (S.a.P != S.b.P)
        return "A and B bands have different row strides";
    if (ctx->tpls[S.a.tpl].version != S.a.tplver)
        return "template changed since the bands were computed";
    if (seq_stale(ctx, S.a))
        return "sequence changed since the bands were computed";
    return nullptr;
}

// Why the A band of slot s cannot be walked (NULL: it can): the calls that
// read A alone (backtraces, alignment sums)
const char *a_band_fault(const rf_ctx *ctx, int32_t s)
{
    if (s < 0 || s >= (int32_t)ctx->slots.size() || !ctx->slots[s].a.valid)
        return "slot has no A band";
    const Band &b = ctx->slots[s].a;
    if (b.failed)
        return FILL_FAILED;
    if (seq_stale(ctx, b))
        return "sequence changed since the bands were computed";
    if (ctx->tpls[b.tpl].version != b.tplver)
        return "template changed since the A band was computed";
    return nullptr;
}

// The fields that CodonTask, CodonDenseGroup and BTTask share, from a checked
// slot's bands and the sequence and template they were filled for
template <class D>
D slot_desc(const rf_ctx *ctx, int32_t s)
{
    const Band &A = ctx->slots[s].a;
    const SeqObj &S = ctx->seqs[A.seq];
    D t{};
    t.A = A.r.off / 8;
    if constexpr (!std::is_same_v<D, BTTask>)
        t.B = ctx->slots[s].b.r.off / 8;
    t.sb = S.bases.off;
    t.tab = S.tabs.off / 8;
    t.tb = ctx->tpls[A.tpl].bases.off;
    t.n = A.n;
    t.m = A.m;
    t.bw = A.bw;
    t.H = A.H;
    t.ncins = S.ncins;
    t.ncdel = S.ncdel;
    t.P = A.P;
    return t;
}

// The batch slots [k0, k1) of one scoring group, checked in slot order (an
// unknown slot is `unknown`, RF_ERR_STATE in rf_score and RF_ERR_ARG in the
// dense calls); tpl: the group's template, -1 before its first slot.  Appends
// the planner's records of the slots to `in` unless that is NULL.
int score_group_slots(rf_ctx *ctx, const char *fn, int unknown, const int32_t *slots, int32_t k0, int32_t k1,
                      int32_t &tpl, std::vector<ScoreReadIn> *in)
{
    for (int32_t k = k0; k < k1; ++k) {
        const int32_t s = slots[k];
        if (s < 0 || s >= (int32_t)ctx->slots.size())
            return fail(ctx, unknown, std::string(fn) + ": unknown slot");
        if (const char *why = score_band_fault(ctx, s))
            return fail(ctx, RF_ERR_STATE, std::string(fn) + ": " + why);
        const Band &A = ctx->slots[s].a;
        const SeqObj &S = ctx->seqs[A.seq];
        if (S.ncins > 0 || S.ncdel > 0)
            return fail(ctx, RF_ERR_ARG, "error model cannot allow codon indels");
        if (tpl >= 0 && A.tpl != tpl)
            return fail(ctx, RF_ERR_ARG, std::string(fn) + ": batch slots use different templates");
        tpl = A.tpl;
        if (in)
            in->push_back({A.r.off, ctx->slots[s].b.r.off, S.bases.off, S.tabs.off, A.n, A.m, A.bw, A.H, A.P,
                           S.finite, S.coded});
    }
    return 0;
}

}  // namespace

// rf_last_error text for the host stage machine in rifraf_batch.cpp (same
// library, C++ linkage, not part of the C-ABI)
int rf_internal_fail(rf_ctx *ctx, int code, const char *msg)
{
    return fail(ctx, code, msg ? msg : "");
}

extern "C" {

int rf_abi_version(void) { return RF_ABI_VERSION; }

int rf_create(int device, rf_ctx **out)
{
    if (!out)
        return RF_ERR_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return RF_ERR_HIP;
    if (device < 0 || device >= ndev)
        return RF_ERR_ARG;
    rf_ctx *ctx = new rf_ctx();
    ctx->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc((void **)&ctx->d_err, sizeof(int)) != hipSuccess ||
        hipMemset(ctx->d_err, 0, sizeof(int)) != hipSuccess) {
        delete ctx;
        return RF_ERR_HIP;
    }
    load_env_opts(ctx->opt);
    for (auto &e : ctx->ev)
        (void)hipEventCreate(&e);
    (void)hipEventCreateWithFlags(&ctx->ev_block, hipEventBlockingSync | hipEventDisableTiming);
    (void)hipEventCreateWithFlags(&ctx->fork, hipEventDisableTiming);
    for (int i = 0; i < 3; ++i) {
        (void)hipStreamCreateWithFlags(&ctx->side[i], hipStreamNonBlocking);
        (void)hipEventCreateWithFlags(&ctx->join[i], hipEventDisableTiming);
    }
    // the lean scorer may use up to the whole 160 KiB LDS of a CU, and so may
    // the block-wide DP's ring
    (void)hipFuncSetAttribute((const void *)k_score_ws<WS_NPF, 256>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void *)k_score_ws<WS_NPF, 256, true>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void *)k_dp<DPW_NT, false, DPW_NT>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void *)k_ps_gen<DPW_NT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    (void)hipFuncSetAttribute((const void *)k_pe_gen<64>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              48 * (PS_GEN64_H + 6));
    (void)hipFuncSetAttribute((const void *)k_pe_gen<DPW_NT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              48 * (PE_LDS_H + 6));
    (void)hipFuncSetAttribute((const void *)k_pa_gen<DPW_NT, PA_NPPW>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    *out = ctx;
    return 0;
}

int rf_destroy(rf_ctx *ctx)
{
    if (!ctx)
        return 0;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (Arena *a : {&ctx->bytes_arena, &ctx->tab_arena, &ctx->band_arena})
        if (a->d)
            (void)hipFree(a->d);
    for (auto &b : ctx->scratch)
        if (b.p)
            (void)hipFree(b.p);
    if (ctx->grow_segs.p)
        (void)hipFree(ctx->grow_segs.p);
    if (ctx->codes.lut.p)
        (void)hipFree(ctx->codes.lut.p);
    if (ctx->codes.errlut.p)
        (void)hipFree(ctx->codes.errlut.p);
    if (ctx->pinned)
        (void)hipHostFree(ctx->pinned);
    if (ctx->up)
        (void)hipHostFree(ctx->up);
    if (ctx->hdn)
        (void)hipHostFree(ctx->hdn);
    if (ctx->d_err)
        (void)hipFree(ctx->d_err);
    for (auto &e : ctx->ev)
        if (e)
            (void)hipEventDestroy(e);
    if (ctx->ev_block)
        (void)hipEventDestroy(ctx->ev_block);
    for (int i = 0; i < 3; ++i) {
        if (ctx->side[i]) {
            (void)hipStreamSynchronize(ctx->side[i]);
            (void)hipStreamDestroy(ctx->side[i]);
        }
        if (ctx->join[i])
            (void)hipEventDestroy(ctx->join[i]);
    }
    if (ctx->fork)
        (void)hipEventDestroy(ctx->fork);
    (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return 0;
}

const char *rf_last_error(const rf_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

static int *opt_slot(rf_ctx *ctx, int32_t key)
{
    Opts &o = ctx->opt;
    switch (key) {
    case RF_OPT_SCORE_MODE: return &o.score_mode;
    case RF_OPT_SCORE_KERNEL: return &o.score_kernel;
    case RF_OPT_LEAN_LDS_KB: return &o.lean_lds_kb;
    case RF_OPT_BT_WIN_KB: return &o.bt_win_kb;
    case RF_OPT_STAGE_KB: return &o.stage_kb;
    case RF_OPT_BAND_PAD: return &o.band_pad_h;
    case RF_OPT_ALN_SUMS_HOST: return &o.aln_sums_host;
    case RF_OPT_ALN_MARKS_MIN: return &o.aln_marks_min;
    case RF_OPT_SYNC_BLOCK: return &o.sync_block;
    case RF_OPT_SCORE_WGS: return &o.score_wgs;
    case RF_OPT_SEG_WGS: return &o.seg_wgs;
    case RF_OPT_BT_NW: return &o.bt_nw;
    case RF_OPT_PAIR_CHUNK: return &o.pair_chunk;
    case RF_OPT_PAIR_TRACE_MB: return &o.pair_trace_mb;
    case RF_OPT_PAIR_WALK: return &o.pair_walk;
    case RF_OPT_CAND_DEVICE: return &o.cand_device;
    case RF_OPT_PAIR_WIDE: return &o.pair_wide;
    case RF_OPT_PAIR_RING_MB: return &o.pair_ring_mb;
    default: return dp_opt(o, key);   // the DP launch planner's
    }
}

int rf_set_option(rf_ctx *ctx, int32_t key, int32_t value)
{
    if (!ctx)
        return RF_ERR_ARG;
    int *s = opt_slot(ctx, key);
    if (!s)
        return fail(ctx, RF_ERR_ARG, "rf_set_option: unknown option");
    if (*s != value) {
        *s = value;
        ++ctx->opt_gen;
        ctx->rplan.valid = false;   // DP class split depends on options
    }
    return 0;
}

int rf_get_option(rf_ctx *ctx, int32_t key, int32_t *value)
{
    if (!ctx || !value)
        return RF_ERR_ARG;
    int *s = opt_slot(ctx, key);
    if (!s)
        return fail(ctx, RF_ERR_ARG, "rf_get_option: unknown option");
    *value = *s;
    return 0;
}

int rf_reserve(rf_ctx *ctx, int64_t band_bytes)
{
    if (!ctx || band_bytes < 0)
        return RF_ERR_ARG;
    (void)hipSetDevice(ctx->device);
    if (ctx->band_arena.cap - ctx->band_arena.top >= band_bytes + ARENA_GUARD)
        return 0;   // room already: nothing moves, cached plans stay valid
    ++ctx->state_epoch;   // regions move (arena_grow also bumps layout_gen)
    return arena_grow(ctx, ctx->band_arena, band_bytes, nullptr);
}

int rf_release_bands(rf_ctx *ctx)
{
    if (!ctx)
        return RF_ERR_ARG;
    (void)hipSetDevice(ctx->device);
    HIPCHK(ctx, stream_wait(ctx));   // no launch still reads or writes a band
    for (auto &s : ctx->slots)
        for (Band *b : {&s.a, &s.b}) {
            b->valid = false;
            b->failed = false;
            b->r.off = -1;
            b->r.cap = 0;
        }
    ctx->band_arena.top = ARENA_GUARD;
    ++ctx->layout_gen;
    ++ctx->state_epoch;
    return 0;
}

int rf_code_stats(const rf_ctx *ctx, int64_t *entries3, int64_t *entries1, int64_t *uncoded_reads,
                  int64_t *resets)
{
    if (!ctx)
        return RF_ERR_ARG;
    if (entries3)
        *entries3 = (int64_t)ctx->codes.t3.size();
    if (entries1)
        *entries1 = (int64_t)ctx->codes.d1.size();
    if (uncoded_reads)
        *uncoded_reads = ctx->codes.uncoded_reads;
    if (resets)
        *resets = ctx->codes.resets;
    return 0;
}

int64_t rf_device_bytes(const rf_ctx *ctx)
{
    if (!ctx)
        return 0;
    int64_t t = ctx->bytes_arena.cap + ctx->tab_arena.cap + ctx->band_arena.cap;
    for (auto &b : ctx->scratch)
        t += (int64_t)b.cap;
    return t;
}

// ---------------------------------------------------------------------
// Sequence uploads (DESIGN.md §4 "Sequence uploads").  rf_set_sequences and
// rf_set_sequences_codes(_prep) are one list of steps, each written once:
//   upload_check      the arguments and lengths: every RF_ERR_ARG comes from
//                     here, before anything changes
//   fresh_dictionary  a new code dictionary when nothing outside the ids is coded
//   upload_begin      epoch, records, versions, one growth per arena, regions
//   per chunk (chunk_end): ensure_pinned, the path's own staging and launches,
//                     scatter_staged for the bases, and a stream_wait, since the
//                     next chunk reuses the staging and descriptor buffers
//   send_dictionary   new dictionary entries to the device
//   upload_finish     valid, layout_gen
// The host work that touches no device is rifraf_seq_upload.h's.
// ---------------------------------------------------------------------

static int upload_check(rf_ctx *ctx, const char *who, bool pointers, int32_t first, int32_t nseq, const int64_t *off,
                        const int64_t *cins_off, const int64_t *cdel_off)
{
    if (!ctx || first < 0 || nseq < 0 || !pointers)
        return fail(ctx, RF_ERR_ARG, std::string(who) + ": bad arguments");
    for (int32_t k = 0; k < nseq; ++k) {
        const int64_t n = off[k + 1] - off[k];
        const int64_t nci = cins_off ? cins_off[k + 1] - cins_off[k] : 0;
        const int64_t ncd = cdel_off ? cdel_off[k + 1] - cdel_off[k] : 0;
        if (n < 1)
            return fail(ctx, RF_ERR_ARG, std::string(who) + ": empty sequence");
        if ((nci != 0 && nci != n - 2) || (ncd != 0 && ncd != n + 1))
            return fail(ctx, RF_ERR_ARG, std::string(who) + ": inconsistent table lengths");
    }
    return 0;
}

// a fresh code dictionary when no coded sequence outside this upload is
// still valid (nothing references the old codes)
static void fresh_dictionary(rf_ctx *ctx, int32_t first, int32_t nseq)
{
    for (size_t k = 0; k < ctx->seqs.size(); ++k) {
        const bool outside = (int64_t)k < first || (int64_t)k >= (int64_t)first + nseq;
        if (outside && ctx->seqs[k].valid && ctx->seqs[k].coded)
            return;
    }
    if (!(ctx->codes.t3.empty() && ctx->codes.d1.empty()))
        ctx->codes.reset();
}

// The first state change of an upload (the lengths have been checked).  Bands
// filled from these ids are stale from here on, also when the upload fails
// later; until upload_finish the ids are not valid.
static int upload_begin(rf_ctx *ctx, int32_t first, int32_t nseq, const int64_t *off, const int64_t *cins_off,
                        const int64_t *cdel_off)
{
    (void)hipSetDevice(ctx->device);
    ++ctx->state_epoch;
    if ((int64_t)first + nseq > (int64_t)ctx->seqs.size())
        ctx->seqs.resize(first + nseq);
    // each arena grows at most once for the whole upload
    int64_t need_b = 0, need_t = 0;
    for (int32_t k = 0; k < nseq; ++k) {
        SeqObj &S = ctx->seqs[first + k];
        S.version = ++ctx->seq_counter;
        S.valid = false;
        S.n = (int32_t)(off[k + 1] - off[k]);
        S.ncins = (int32_t)(cins_off ? cins_off[k + 1] - cins_off[k] : 0);
        S.ncdel = (int32_t)(cdel_off ? cdel_off[k + 1] - cdel_off[k] : 0);
        const int64_t bb = align_up(std::max<int64_t>(S.n, 16), 256);
        const int64_t tb = align_up(std::max<int64_t>(seq_table_len(S.n, S.ncins, S.ncdel) * 8, 16), 256);
        if (!(S.bases.off >= 0 && S.bases.cap >= bb)) need_b += bb;
        if (!(S.tabs.off >= 0 && S.tabs.cap >= tb)) need_t += tb;
    }
    if (ctx->bytes_arena.top + need_b + ARENA_GUARD > ctx->bytes_arena.cap)
        if (int e = arena_grow(ctx, ctx->bytes_arena, need_b, nullptr)) return e;
    if (ctx->tab_arena.top + need_t + ARENA_GUARD > ctx->tab_arena.cap)
        if (int e = arena_grow(ctx, ctx->tab_arena, need_t, nullptr)) return e;
    // regions (a growth moves earlier regions: offsets are read after this loop)
    for (int32_t k = 0; k < nseq; ++k) {
        SeqObj &S = ctx->seqs[first + k];
        if (int e = region_ensure(ctx, ctx->bytes_arena, S.bases, S.n)) return e;
        if (int e = region_ensure(ctx, ctx->tab_arena, S.tabs, seq_table_len(S.n, S.ncins, S.ncdel) * 8)) return e;
    }
    return 0;
}

static void upload_finish(rf_ctx *ctx, int32_t first, int32_t nseq)
{
    for (int32_t k = 0; k < nseq; ++k)
        ctx->seqs[first + k].valid = true;
    ++ctx->layout_gen;
}

// ctx->pinned holds `bytes`: the host staging of one chunk
static int ensure_pinned(rf_ctx *ctx, size_t bytes)
{
    if (ctx->pinned_bytes >= bytes)
        return 0;
    if (ctx->pinned)
        (void)hipHostFree(ctx->pinned);
    ctx->pinned = nullptr;
    ctx->pinned_bytes = 0;
    const size_t want = std::max(bytes + bytes / 2, (size_t)1 << 22);
    if (hipHostMalloc(&ctx->pinned, want, hipHostMallocDefault) != hipSuccess)
        return fail(ctx, RF_ERR_HIP, "sequence upload: pinned staging allocation failed");
    ctx->pinned_bytes = want;
    return 0;
}

// new code-dictionary entries to the device, one H2D copy per kind
static int send_dictionary(rf_ctx *ctx)
{
    DevCodeDict &D = ctx->codes;
    if (int e = ensure_buf(ctx, D.lut, (size_t)RF_CODES * 5 * 8)) return e;
    const size_t n3 = D.t3v.size() / 4, n1 = D.d1v.size();
    if (n3 > D.up3)
        HIPCHK(ctx, hipMemcpyAsync((double *)D.lut.p + 4 * D.up3, D.t3v.data() + 4 * D.up3, (n3 - D.up3) * 32,
                                   hipMemcpyHostToDevice, ctx->stream));
    if (n1 > D.up1)
        HIPCHK(ctx, hipMemcpyAsync((double *)D.lut.p + 4 * (size_t)RF_CODES + D.up1, D.d1v.data() + D.up1,
                                   (n1 - D.up1) * 8, hipMemcpyHostToDevice, ctx->stream));
    D.up3 = n3;
    D.up1 = n1;
    return 0;
}

// One k_scatter launch: the segments of the staged bytes in `src` to their
// places in arena `a`.  The descriptors go through BUF_SEGS_OR_WORK, which the
// stream must have read before the next call of this (the callers' waits).
static int scatter_staged(rf_ctx *ctx, const std::vector<Segment> &sg, Buf src, Arena &a)
{
    if (int e = upload(ctx, ctx->scratch[BUF_SEGS_OR_WORK], sg)) return e;
    hipLaunchKernelGGL(k_scatter, dim3((unsigned)sg.size()), dim3(256), 0, ctx->stream,
                       dev<const Segment>(ctx, BUF_SEGS_OR_WORK), dev<const uint8_t>(ctx, src), (uint8_t *)a.d);
    return 0;
}

// One chunk of rf_set_sequences, sequences [k0, k1) of the call: their tables
// and bases packed into pinned memory and coded there (code_rows), one H2D
// copy each, and a scatter each to the regions.
static int tables_chunk(rf_ctx *ctx, int32_t first, int32_t k0, int32_t k1, const uint8_t *bases, const int64_t *off,
                        const double *match, const double *mismatch, const double *ins, const double *del,
                        const double *cins, const int64_t *cins_off, const double *cdel, const int64_t *cdel_off)
{
    const int32_t nseq = k1 - k0;
    const int64_t nb = off[k1] - off[k0];
    std::vector<Segment> sb(nseq), st(nseq);
    int64_t nt = 0;
    for (int32_t k = 0; k < nseq; ++k) {
        const SeqObj &S = ctx->seqs[first + k0 + k];
        const int64_t len = seq_table_len(S.n, S.ncins, S.ncdel);
        st[k] = {nt * 8, S.tabs.off, len * 8, 0};
        sb[k] = {off[k0 + k] - off[k0], S.bases.off, S.n, 0};
        nt += len;
    }
    if (int e = ensure_pinned(ctx, (size_t)nt * 8 + (size_t)nb)) return e;
    double *host_tabs = (double *)ctx->pinned;
    uint8_t *host_bases = (uint8_t *)ctx->pinned + (size_t)nt * 8;
    std::vector<RowSeq> rs(nseq);
    for (int32_t k = 0; k < nseq; ++k) {
        const SeqObj &S = ctx->seqs[first + k0 + k];
        rs[k] = {host_tabs + st[k].src / 8, bases + off[k0 + k], S.n, S.ncins, S.ncdel, false, false};
    }
    // the host work per position (staging copies, the finiteness test, the
    // row codes) runs on host threads, one per MB of tables
    const int nth = (int)std::max<int64_t>(1, std::min<int64_t>(host_threads(), (nt + (1 << 20) - 1) >> 20));
    code_rows(ctx->codes, rs.data(), nseq, nth, [&](int32_t k) {
        const int32_t kg = k0 + k;   // index into the caller's arrays
        pack_tables(rs[k], match + off[kg], mismatch + off[kg], ins + off[kg], del + off[kg] + kg,
                    rs[k].nci ? cins + cins_off[kg] : nullptr, rs[k].ncd ? cdel + cdel_off[kg] : nullptr);
    });
    for (int32_t k = 0; k < nseq; ++k) {
        ctx->seqs[first + k0 + k].finite = rs[k].finite;
        ctx->seqs[first + k0 + k].coded = rs[k].coded;
    }
    if (int e = send_dictionary(ctx)) return e;
    if (int e = ensure_buf(ctx, ctx->scratch[BUF_TABS_OR_CSEQS], (size_t)nt * 8)) return e;
    if (int e = ensure_buf(ctx, ctx->scratch[BUF_BYTES_OR_SINK], (size_t)std::max<int64_t>(nb, 16))) return e;
    std::memcpy(host_bases, bases + off[k0], nb);
    HIPCHK(ctx, hipMemcpyAsync(ctx->scratch[BUF_TABS_OR_CSEQS].p, host_tabs, nt * 8, hipMemcpyHostToDevice,
                               ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->scratch[BUF_BYTES_OR_SINK].p, host_bases, nb, hipMemcpyHostToDevice, ctx->stream));
    if (int e = scatter_staged(ctx, st, BUF_TABS_OR_CSEQS, ctx->tab_arena)) return e;
    HIPCHK(ctx, stream_wait(ctx));   // between the two uses of BUF_SEGS_OR_WORK
    if (int e = scatter_staged(ctx, sb, BUF_BYTES_OR_SINK, ctx->bytes_arena)) return e;
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, stream_wait(ctx));   // after the chunk: the next one reuses the pinned staging and all three buffers
    return 0;
}

// A refusal (RF_ERR_ARG) leaves the context as it was: see upload_check.
int rf_set_sequences(rf_ctx *ctx, int32_t first, int32_t nseq, const uint8_t *bases,
                     const int64_t *off, const double *match, const double *mismatch,
                     const double *ins, const double *del, const double *cins,
                     const int64_t *cins_off, const double *cdel, const int64_t *cdel_off)
{
    if (int e = upload_check(ctx, "rf_set_sequences", nseq <= 0 || (bases && off && match && mismatch && ins && del),
                             first, nseq, off, cins_off, cdel_off))
        return e;
    fresh_dictionary(ctx, first, nseq);
    if (int e = upload_begin(ctx, first, nseq, off, cins_off, cdel_off)) return e;
    // chunks of at most RF_OPT_STAGE_KB of tables: a bounded pinned staging
    // buffer and device scratch, whatever the size of the upload
    const int64_t budget = tables_stage_budget(ctx->opt.stage_kb);
    for (int32_t k0 = 0, k1; k0 < nseq; k0 = k1) {
        k1 = chunk_end(k0, nseq, budget, [&](int32_t k) {
            const SeqObj &S = ctx->seqs[first + k];
            return tables_stage_bytes(S.n, S.ncins, S.ncdel);
        });
        if (int e = tables_chunk(ctx, first, k0, k1, bases, off, match, mismatch, ins, del, cins, cins_off, cdel,
                                 cdel_off))
            return e;
    }
    upload_finish(ctx, first, nseq);
    return 0;
}

// The codes path's per-code values: which codes occur, the four table values
// of each and whether they are finite, and the device's CodeLut.
struct CodeTables {
    bool present[256] = {};
    bool fin[256];
    std::vector<CodeLut> lut = std::vector<CodeLut>(256);
};

// The 256-entry LUT of an upload of N positions: the table values by the
// RifrafSequence constructor's FP64 adds, and the dictionary codes of the
// codes present.  RF_ERR_STATE when the dictionary cannot hold them: the
// entries this call added are dropped again (the caller then uploads host
// tables; codes no sequence uses must not crowd out later uploads).
static int code_tables(rf_ctx *ctx, int64_t N, const uint8_t *codes, const double *lp_t, const double *match_t,
                       double s_mis, double s_ins, double s_del, CodeTables &T)
{
    {
        // one byte store per position (~0.5 ns): threads from 512 K positions
        // (c3's 2.6 M: 1.3 ms on one thread)
        const int nth = (int)std::max<int64_t>(1, std::min<int64_t>(host_threads(), (N >> 19) + 1));
        std::vector<std::array<uint8_t, 256>> pr(nth);
        parallel_for(nth, [&](int t) {
            pr[t].fill(0);
            for (int64_t i = N * t / nth; i < N * (t + 1) / nth; ++i)
                pr[t][codes[i]] = 1;
        });
        for (int t = 0; t < nth; ++t)
            for (int c = 0; c < 256; ++c)
                T.present[c] = T.present[c] || pr[t][c];
    }
    CodeDict &D = ctx->codes;
    const CodeDict::Mark mark = D.mark();
    for (int c = 0; c < 256; ++c) {
        const double mt = match_t[c], mm = lp_t[c] + s_mis, is = lp_t[c] + s_ins, dl = lp_t[c] + s_del;
        T.fin[c] = std::isfinite(mt) && std::isfinite(mm) && std::isfinite(is) && std::isfinite(dl);
        T.lut[c] = {lp_t[c], mt, 0, 0, 0, 0};
        if (!T.present[c])
            continue;
        T.lut[c].id3 = D.insert3(CodeDict::key3(mt, mm, is));
        T.lut[c].id1 = D.insert1(CodeDict::bits(dl));
        if (T.lut[c].id3 < 0 || T.lut[c].id1 < 0) {
            D.undo(mark);
            return fail(ctx, RF_ERR_STATE, "rf_set_sequences_codes: row-code dictionary full");
        }
    }
    return 0;
}

// Refusals leave the context as it was: RF_ERR_ARG (upload_check) and the
// full dictionary's RF_ERR_STATE (code_tables; a dictionary that
// fresh_dictionary has just emptied holds any 256 codes, so the refusal meets
// one that was kept).
static int set_sequences_codes_impl(rf_ctx *ctx, int32_t first, int32_t nseq, const uint8_t *bases,
                                    const int64_t *off, const uint8_t *codes, const double *lp_t,
                                    const double *match_t, double s_mis, double s_ins, double s_del,
                                    const double *p10_t, const double *grid, double *est, int32_t *ucode,
                                    double *tsum)
{
    const bool prep = p10_t != nullptr;
    if (int e = upload_check(ctx, "rf_set_sequences_codes", nseq <= 0 || (bases && off && codes && lp_t && match_t),
                             first, nseq, off, nullptr, nullptr))
        return e;
    const int64_t N = nseq > 0 ? off[nseq] - off[0] : 0;
    fresh_dictionary(ctx, first, nseq);
    CodeTables T;
    if (int e = code_tables(ctx, N, nseq > 0 ? codes + off[0] : codes, lp_t, match_t, s_mis, s_ins, s_del, T)) return e;
    if (int e = upload_begin(ctx, first, nseq, off, nullptr, nullptr)) return e;
    if (int e = send_dictionary(ctx)) return e;
    if (int e = upload(ctx, ctx->scratch[BUF_CODE_LUTS], T.lut)) return e;
    // prep (rf_set_sequences_codes_prep): p10 | match tables, the 256 x 256
    // grid, then est / tsum (nseq doubles each) and ucode (nseq ints)
    const size_t prep_tab = 512 * 8, prep_grid = 65536 * 8, prep_out = (size_t)std::max(nseq, 1) * 20;
    if (prep) {
        if (int e = ensure_buf(ctx, ctx->scratch[BUF_CODE_PREP], prep_tab + prep_grid + prep_out)) return e;
        // the two tables and the grid as one copy out of the pinned ring
        char *h;
        if (int e = ring_take(ctx, prep_tab + prep_grid, &h)) return e;
        if (h) {
            std::memcpy(h, p10_t, 256 * 8);
            std::memcpy(h + 256 * 8, match_t, 256 * 8);
            std::memcpy(h + prep_tab, grid, prep_grid);
            HIPCHK(ctx, hipMemcpyAsync(ctx->scratch[BUF_CODE_PREP].p, h, prep_tab + prep_grid, hipMemcpyHostToDevice,
                                       ctx->stream));
        } else {
            HIPCHK(ctx, hipMemcpyAsync(ctx->scratch[BUF_CODE_PREP].p, p10_t, 256 * 8, hipMemcpyHostToDevice,
                                       ctx->stream));
            HIPCHK(ctx, hipMemcpyAsync(dev<char>(ctx, BUF_CODE_PREP) + 256 * 8, match_t, 256 * 8,
                                       hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(ctx, hipMemcpyAsync(dev<char>(ctx, BUF_CODE_PREP) + prep_tab, grid, prep_grid,
                                       hipMemcpyHostToDevice, ctx->stream));
        }
    }
    double *d_est = (double *)(dev<char>(ctx, BUF_CODE_PREP) + prep_tab + prep_grid);
    double *d_tsum = d_est + std::max(nseq, 1);
    int32_t *d_ucode = (int32_t *)(d_tsum + std::max(nseq, 1));
    // chunks of sequences: bases + codes staged in pinned memory, one H2D,
    // the bases scattered to their regions, the tables built in place
    const int64_t budget = codes_stage_budget(ctx->opt.stage_kb);
    for (int32_t k0 = 0, k1; k0 < nseq; k0 = k1) {
        k1 = chunk_end(k0, nseq, budget, [&](int32_t k) { return codes_stage_bytes(off[k + 1] - off[k]); });
        const int64_t nb = off[k1] - off[k0];
        if (int e = ensure_pinned(ctx, (size_t)(2 * nb))) return e;
        uint8_t *hb = (uint8_t *)ctx->pinned, *hc = hb + nb;
        std::memcpy(hb, bases + off[k0], nb);
        std::memcpy(hc, codes + off[k0], nb);
        std::vector<CodeSeq> cs(k1 - k0);
        std::vector<Segment> sg(k1 - k0);
        for (int32_t k = k0; k < k1; ++k) {
            const SeqObj &S = ctx->seqs[first + k];
            cs[k - k0] = {S.tabs.off / 8, off[k] - off[k0], S.n, 0, 0};
            sg[k - k0] = {off[k] - off[k0], S.bases.off, S.n, 0};
        }
        if (int e = ensure_buf(ctx, ctx->scratch[BUF_BYTES_OR_SINK], (size_t)std::max<int64_t>(2 * nb, 16))) return e;
        HIPCHK(ctx, hipMemcpyAsync(ctx->scratch[BUF_BYTES_OR_SINK].p, hb, 2 * nb, hipMemcpyHostToDevice, ctx->stream));
        // every copy of the chunk before its first launch
        if (int e = upload(ctx, ctx->scratch[BUF_TABS_OR_CSEQS], cs)) return e;
        if (int e = scatter_staged(ctx, sg, BUF_BYTES_OR_SINK, ctx->bytes_arena)) return e;
        hipLaunchKernelGGL(k_tables, dim3(k1 - k0), dim3(256), 0, ctx->stream,
                           dev<const CodeSeq>(ctx, BUF_TABS_OR_CSEQS),
                           dev<const uint8_t>(ctx, BUF_BYTES_OR_SINK) + nb, dev<const uint8_t>(ctx, BUF_BYTES_OR_SINK),
                           dev<const CodeLut>(ctx, BUF_CODE_LUTS), s_mis, s_ins, s_del, (double *)ctx->tab_arena.d);
        if (prep)
            hipLaunchKernelGGL(k_code_prep, dim3(k1 - k0), dim3(64), 0, ctx->stream,
                               dev<const CodeSeq>(ctx, BUF_TABS_OR_CSEQS), k1 - k0,
                               dev<const uint8_t>(ctx, BUF_BYTES_OR_SINK) + nb,
                               dev<const double>(ctx, BUF_CODE_PREP),
                               (const double *)(dev<char>(ctx, BUF_CODE_PREP) + prep_tab), d_est + k0, d_ucode + k0,
                               d_tsum + k0);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, stream_wait(ctx));   // after the chunk: the next one reuses the pinned staging and all three buffers
    }
    // finiteness per sequence (lean DP / scorer eligibility): every sequence
    // is finite when every code present is; else one pass per sequence
    bool all_fin = true;
    for (int c = 0; c < 256; ++c)
        all_fin = all_fin && (!T.present[c] || T.fin[c]);
    if (all_fin) {
        for (int32_t k = 0; k < nseq; ++k)
            ctx->seqs[first + k].finite = true;
    } else {
        const int nth = (int)std::max<int64_t>(1, std::min<int64_t>(host_threads(), (N >> 19) + 1));
        parallel_for(nth, [&](int t) {
            for (int32_t k = (int32_t)((int64_t)nseq * t / nth); k < (int32_t)((int64_t)nseq * (t + 1) / nth); ++k) {
                bool f = true;
                for (int64_t i = off[k]; i < off[k + 1] && f; ++i)
                    f = T.fin[codes[i]];
                ctx->seqs[first + k].finite = f;
            }
        });
    }
    for (int32_t k = 0; k < nseq; ++k)
        ctx->seqs[first + k].coded = true;
    upload_finish(ctx, first, nseq);
    if (prep && nseq > 0) {
        // est | tsum | ucode are contiguous on the device: one copy into the
        // pinned landing zone
        const size_t ob = (size_t)std::max(nseq, 1) * 20;
        if (int e = ensure_landing(ctx, ob)) return e;
        HIPCHK(ctx, pre_d2h(ctx));
        HIPCHK(ctx, land(ctx, 0, d_est, ob));
        HIPCHK(ctx, stream_wait(ctx));
        const char *hl = landed<char>(ctx);
        const size_t ns = (size_t)std::max(nseq, 1);
        std::memcpy(est, hl, (size_t)nseq * 8);
        std::memcpy(tsum, hl + ns * 8, (size_t)nseq * 8);
        std::memcpy(ucode, hl + ns * 16, (size_t)nseq * 4);
    }
    return 0;
}

int rf_set_sequences_codes(rf_ctx *ctx, int32_t first, int32_t nseq, const uint8_t *bases, const int64_t *off,
                           const uint8_t *codes, const double *lp_t, const double *match_t, double s_mis,
                           double s_ins, double s_del)
{
    return set_sequences_codes_impl(ctx, first, nseq, bases, off, codes, lp_t, match_t, s_mis, s_ins, s_del, nullptr,
                                    nullptr, nullptr, nullptr, nullptr);
}

int rf_set_sequences_codes_prep(rf_ctx *ctx, int32_t first, int32_t nseq, const uint8_t *bases, const int64_t *off,
                                const uint8_t *codes, const double *lp_t, const double *match_t, double s_mis,
                                double s_ins, double s_del, const double *p10_t, const double *grid, double *est,
                                int32_t *ucode, double *tsum)
{
    if (!ctx || (nseq > 0 && (!p10_t || !grid || !est || !ucode || !tsum)))
        return fail(ctx, RF_ERR_ARG, "rf_set_sequences_codes_prep: bad arguments");
    return set_sequences_codes_impl(ctx, first, nseq, bases, off, codes, lp_t, match_t, s_mis, s_ins, s_del, p10_t,
                                    grid, est, ucode, tsum);
}

int rf_set_templates(rf_ctx *ctx, int32_t first, int32_t ntpl, const uint8_t *bases,
                     const int64_t *off)
{
    if (!ctx || first < 0 || ntpl < 0 || (ntpl > 0 && (!bases || !off)))
        return fail(ctx, RF_ERR_ARG, "rf_set_templates: bad arguments");
    std::vector<int32_t> ids(ntpl);
    for (int32_t k = 0; k < ntpl; ++k)
        ids[k] = first + k;
    return rf_set_templates_ids(ctx, ntpl, ids.data(), bases, off);
}

int rf_set_templates_ids(rf_ctx *ctx, int32_t ntpl, const int32_t *ids, const uint8_t *bases,
                         const int64_t *off)
{
    if (!ctx || ntpl < 0 || (ntpl > 0 && (!ids || !bases || !off)))
        return fail(ctx, RF_ERR_ARG, "rf_set_templates: bad arguments");
    (void)hipSetDevice(ctx->device);
    ++ctx->state_epoch;
    int32_t top = 0;
    for (int32_t k = 0; k < ntpl; ++k) {
        if (ids[k] < 0)
            return fail(ctx, RF_ERR_ARG, "rf_set_templates: bad arguments");
        top = std::max(top, ids[k] + 1);
    }
    if ((int64_t)top > (int64_t)ctx->tpls.size())
        ctx->tpls.resize(top);
    for (int32_t k = 0; k < ntpl; ++k) {
        TplObj &T = ctx->tpls[ids[k]];
        const int64_t m = off[k + 1] - off[k];
        if (m < 1)
            return fail(ctx, RF_ERR_ARG, "rf_set_templates: empty template");
        if (int e = region_ensure(ctx, ctx->bytes_arena, T.bases, m))
            return e;
        if (T.m != (int32_t)m)
            ++ctx->layout_gen;
        T.m = (int32_t)m;
        T.version = ++ctx->tpl_counter;
        T.valid = true;
    }
    if (ntpl > 0) {
        // offsets are read after every region_ensure (arena growth moves regions)
        std::vector<Segment> sg(ntpl);
        for (int32_t k = 0; k < ntpl; ++k)
            sg[k] = {off[k] - off[0], ctx->tpls[ids[k]].bases.off, off[k + 1] - off[k], 0};
        const int64_t nb = off[ntpl] - off[0];
        if (int e = ensure_buf(ctx, ctx->scratch[BUF_BYTES_OR_SINK], (size_t)std::max<int64_t>(nb, 16))) return e;
        HIPCHK(ctx, hipMemcpyAsync(ctx->scratch[BUF_BYTES_OR_SINK].p, bases + off[0], nb, hipMemcpyHostToDevice,
                                   ctx->stream));
        if (int e = scatter_staged(ctx, sg, BUF_BYTES_OR_SINK, ctx->bytes_arena)) return e;
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, stream_wait(ctx));
    return 0;
}

static int realign_run(rf_ctx *ctx, int32_t njobs, const int32_t *slot, const int32_t *seq, const int32_t *tpl,
                       const int32_t *bw, const int32_t *jf, double *out_score);

// rf_realign / rf_realign_jobs.  A call that gets past its argument checks and
// then fails -- the reference's error() (RF_ERR_NUMERIC), an allocation, a HIP
// error -- leaves no band behind that reads as filled: the reference's
// error() leaves no state, so every band the call named, the good jobs' too,
// is refused by the read-back calls until a later fill succeeds.  The plan is
// dropped, so that fill plans again (and clears the mark); the epoch moves for
// the scorers' validation skip.
static int realign_impl(rf_ctx *ctx, int32_t njobs, const int32_t *slot, const int32_t *seq, const int32_t *tpl,
                        const int32_t *bw, const int32_t *jf, double *out_score)
{
    const int e = realign_run(ctx, njobs, slot, seq, tpl, bw, jf, out_score);
    if (e == 0 || e == RF_ERR_ARG)   // RF_ERR_ARG: refused before anything was planned
        return e;
    for (int32_t k = 0; k < njobs; ++k) {
        if (slot[k] < 0 || slot[k] >= (int32_t)ctx->slots.size())
            continue;
        Slot &S = ctx->slots[slot[k]];
        if ((jf[k] & RF_FWD) && S.a.valid)
            S.a.failed = true;
        if ((jf[k] & RF_BWD) && S.b.valid)
            S.b.failed = true;
    }
    ctx->rplan.valid = false;
    ++ctx->state_epoch;
    return e;
}

// The DPTask of one alignment, the single place one is filled (no slot, no
// band: the caller adds those); fl: 1 = reverse, 2 = skew, 4 = trim
static DPTask pair_task(const SeqObj &S, const TplObj &T, int bw, int fl, int32_t out_idx)
{
    DPTask t{};
    t.sb = S.bases.off;
    t.tab = S.tabs.off / 8;
    t.tb = T.bases.off;
    t.n = S.n;
    t.m = T.m;
    t.bw = bw;
    t.H = band_rows(S.n + 1, T.m + 1, bw);
    t.c = std::max(T.m - S.n, 0) + bw;
    t.ncins = S.ncins;
    t.ncdel = S.ncdel;
    t.flags = fl | (S.coded ? RF_TASK_CODED : 0);
    t.out_idx = out_idx;
    t.klen = t.H + 2 * t.m;
    return t;
}

// The task of fill (dir, k) of an rf_realign call of njobs jobs into a band at
// `band` (doubles) with row stride P.  Skew and trim are the forward fill's;
// forward scores win out_score when both directions run.
static DPTask realign_task(const SeqObj &S, const TplObj &T, int bw, int jf, int dir, int32_t k, int32_t njobs,
                           int64_t band, int P)
{
    const int fl = dir == 1 ? 1 : fill_flags(jf);
    DPTask t = pair_task(S, T, bw, fl, (dir == 0 || !(jf & RF_FWD)) ? k : njobs + k);
    t.band = band;
    t.P = P;
    return t;
}

static int realign_check(rf_ctx *ctx, int32_t njobs, const int32_t *slot, const int32_t *seq, const int32_t *tpl,
                         const int32_t *bw)
{
    for (int32_t k = 0; k < njobs; ++k) {
        if (slot[k] < 0 || seq[k] < 0 || seq[k] >= (int32_t)ctx->seqs.size() || !ctx->seqs[seq[k]].valid ||
            tpl[k] < 0 || tpl[k] >= (int32_t)ctx->tpls.size() || !ctx->tpls[tpl[k]].valid)
            return fail(ctx, RF_ERR_ARG, "rf_realign: unknown slot / sequence / template");
        if (bw[k] < 1)
            return fail(ctx, RF_ERR_ARG, "bandwidth must be positive");
    }
    return 0;
}

static Band &job_band(rf_ctx *ctx, int32_t slot, int dir) { return dir == 0 ? ctx->slots[slot].a : ctx->slots[slot].b; }

// An identical job list on an unchanged layout: the descriptors on the device
// are still exact; only the band bookkeeping (template / sequence version) moves
static void realign_restamp(rf_ctx *ctx, int32_t njobs, const int32_t *slot, const int32_t *seq, const int32_t *tpl,
                            const int32_t *jf)
{
    bool changed = false;
    for_each_fill(njobs, jf, [&](int dir, int32_t k) {
        Band &b = job_band(ctx, slot[k], dir);
        const uint64_t v = ctx->tpls[tpl[k]].version, sv = ctx->seqs[seq[k]].version;
        changed = changed || b.tplver != v || b.seqver != sv;
        b.tplver = v;
        b.seqver = sv;
        return 0;
    });
    if (changed)
        ++ctx->state_epoch;
}

// Band bookkeeping of a new job list: every band's region, stride and metadata
static int realign_bands(rf_ctx *ctx, int32_t njobs, const int32_t *slot, const int32_t *seq, const int32_t *tpl,
                         const int32_t *bw, const int32_t *jf)
{
    ++ctx->state_epoch;   // band metadata changes below
    int32_t maxslot = -1;
    for (int32_t k = 0; k < njobs; ++k)
        maxslot = std::max(maxslot, slot[k]);
    if (maxslot >= (int32_t)ctx->slots.size())
        ctx->slots.resize(maxslot + 1);
    bool moved = false;   // a band now describes another alignment
    // RF_OPT_BAND_PAD: a call whose widest band reaches the threshold lays out
    // all its bands with line-padded rows (the wide-band scorer reads them a
    // line per row); narrower calls (c4-like) keep the odd stride, which the
    // window scorer k_score_ws stages in fewer passes
    int hmax_call = 0;
    for (int32_t k = 0; k < njobs; ++k)
        hmax_call = std::max(hmax_call, band_rows(ctx->seqs[seq[k]].n + 1, ctx->tpls[tpl[k]].m + 1, bw[k]));
    const bool pad_call = ctx->opt.band_pad_h > 0 && hmax_call >= ctx->opt.band_pad_h;
    const int e = for_each_fill(njobs, jf, [&](int dir, int32_t k) {
        const SeqObj &S = ctx->seqs[seq[k]];
        const TplObj &T = ctx->tpls[tpl[k]];
        Band &b = job_band(ctx, slot[k], dir);
        const int H = band_rows(S.n + 1, T.m + 1, bw[k]);
        // A and B of one alignment share a row stride: every scorer reads
        // both bands with one P, and the two are often filled by different
        // calls (forward_moves with band doubling, then backward!) that
        // may differ in pad_call
        const Band &o = job_band(ctx, slot[k], 1 - dir);
        const bool partner = o.valid && o.seq == seq[k] && o.tpl == tpl[k] && o.bw == bw[k] &&
                             o.n == S.n && o.m == T.m && o.H == H && o.tplver == T.version &&
                             o.seqver == S.version;
        const int P = partner ? o.P : band_stride(H, pad_call ? 1 : 0);
        if (int e = region_ensure(ctx, ctx->band_arena, b.r, band_payload_bytes(H, T.m, P)))
            return e;
        moved = moved || !b.valid || b.seq != seq[k] || b.tpl != tpl[k] || b.bw != bw[k] ||
                b.n != S.n || b.m != T.m || b.H != H || b.P != P;
        b.P = P;
        b.valid = true;
        b.failed = false;
        b.seq = seq[k];
        b.tpl = tpl[k];
        b.bw = bw[k];
        b.n = S.n;
        b.m = T.m;
        b.H = H;
        b.flags = dir == 0 ? (jf[k] & (RF_SKEW | RF_TRIM)) : 0;
        b.tplver = T.version;
        b.seqver = S.version;
        return 0;
    });
    if (e)
        return e;
    // scorer descriptors (rf_score_dense's plan) hold band geometry and
    // sequence offsets: a band that now describes another read, template or
    // bandwidth invalidates them even when its region did not move
    if (moved)
        ++ctx->layout_gen;
    return 0;
}

// The call's tasks sorted into launches (dp_plan, rifraf_dp_plan.h).  Band
// offsets are only final after every allocation (arena growth moves them), so
// this follows realign_bands.
static DpPlan realign_plan(rf_ctx *ctx, int32_t njobs, const int32_t *slot, const int32_t *seq, const int32_t *tpl,
                           const int32_t *bw, const int32_t *jf)
{
    std::vector<DPTask> tasks;
    std::vector<uint8_t> finite;
    tasks.reserve(2 * (size_t)njobs);
    finite.reserve(2 * (size_t)njobs);
    for_each_fill(njobs, jf, [&](int dir, int32_t k) {
        const SeqObj &S = ctx->seqs[seq[k]];
        const Band &b = job_band(ctx, slot[k], dir);
        tasks.push_back(realign_task(S, ctx->tpls[tpl[k]], bw[k], jf[k], dir, k, njobs, b.r.off / 8, b.P));
        finite.push_back(S.finite);
        return 0;
    });
    return dp_plan(tasks, finite, ctx->opt);
}

// k_dpm runs a launch's bands in chunks: at most DPM_XCD_SLICES slices per
// XCD per launch, the launches in sequence on one stream.  A launch's bands
// become resident in order, but two launches from different streams
// interleave, so each keeps to a share of an XCD (four such launches fit at
// once)
static int dpm_chunk(int gm) { return 8 * std::max(1, DPM_XCD_SLICES / gm); }

// Grid, block and dynamic LDS of a launch (k_dpm: of its first chunk)
struct DpGeom { unsigned grid, block; size_t lds; };
static DpGeom dp_geom(const DpLaunch &L)
{
    const unsigned n = (unsigned)L.n;
    switch (L.k) {
    case DpKernel::Dpr: return {(n + 3) / 4, 64, 0};
    case DpKernel::DprLean: return {(n + 3) / 4, 64, 4 * (size_t)dpl_task_bytes(1 << L.npi)};
    case DpKernel::DprLeanPm: return {(n + 3) / 4, 64, 4 * (size_t)dpl_task_bytes(1 << L.npi, dpr_pm(L.npi, L.pmi))};
    case DpKernel::DprWide64: return {n, 64, (size_t)dpl_task_bytes(2, dpl_pmax(2, 64), 64)};
    case DpKernel::DprWide32: return {(n + 1) / 2, 64, 2 * (size_t)dpl_task_bytes(2, dpl_pmax(2, 32), 32)};
    case DpKernel::DpxCodon:
    case DpKernel::DpxLean: return {n, 128, 0};
    case DpKernel::Dp64: return {n, 64, 4 * (size_t)(L.hmax + 6) * 8};   // the LDS ring: 4 anti-diagonals
    case DpKernel::DpwLds: return {n, DPW_NT, 4 * (size_t)(L.hmax + 6) * 8};
    case DpKernel::DpwGlobal: return {n, DPW_NT, 0};
    case DpKernel::Dpm: return {8 * ((std::min(n, (unsigned)dpm_chunk(L.hmax)) + 7) / 8) * L.hmax, 64, 0};
    }
    return {0, 0, 0};
}

// The k_dpr instance of a 16-lane launch
using DprFn = void (*)(const DPTask *, int, const uint8_t *, const double *, double *, double *, int *, double *,
                       const double *);
static DprFn dpr_kernel(const DpLaunch &L)
{
#define KP(a, b) k_dpr<1 << (a), true, dpr_pm(a, b), 16, (a) == 0 && DPR_PFIX>
#define KP4(a) KP(a, 0), KP(a, 1), KP(a, 2), KP(a, 3)
    static const DprFn whole[4][2] = {{k_dpr<1, false>, k_dpr<1, true>}, {k_dpr<2, false>, k_dpr<2, true>},
                                      {k_dpr<4, false>, k_dpr<4, true>}, {k_dpr<8, false>, k_dpr<8, true>}};
    static const DprFn pm[4][4] = {{KP4(0)}, {KP4(1)}, {KP4(2)}, {KP4(3)}};
#undef KP4
#undef KP
    return L.k == DpKernel::DprLeanPm ? pm[L.npi][L.pmi] : whole[L.npi][L.k == DpKernel::DprLean];
}

// The launches of a plan whose tasks are in BUF_DP_TASKS, scores into d_out.
// The side streams fork from the context's stream and join it again.
static int launch_dp(rf_ctx *ctx, const DpPlan &plan, double *d_out)
{
    const DPTask *d_tasks = dev<const DPTask>(ctx, BUF_DP_TASKS);
    const uint8_t *d_bases = (const uint8_t *)ctx->bytes_arena.d;
    const double *d_tabs = (const double *)ctx->tab_arena.d;
    double *d_bands = (double *)ctx->band_arena.d;
    const double *d_lut = (const double *)ctx->codes.lut.p;
    // the lean kernels' padding-task sink
    if (int e = ensure_buf(ctx, ctx->scratch[BUF_BYTES_OR_SINK], 4 * (size_t)dpl_task_bytes(4)))
        return e;
    bool fork = false;
    for (const DpLaunch &L : plan.launches) {
        fork = fork || L.stream >= 0;
        if (L.k == DpKernel::DpwLds || L.k == DpKernel::DpwGlobal)   // the global ring (sized for either)
            if (int e = ensure_buf(ctx, ctx->scratch[BUF_RING_OR_SPLIT], L.n * 4 * (size_t)(L.hmax + 6) * 8))
                return e;
    }
    if (fork)
        HIPCHK(ctx, hipEventRecord(ctx->fork, ctx->stream));
    std::vector<int> used_side;
    for (const DpLaunch &L : plan.launches) {
        hipStream_t st = ctx->stream;
        if (L.stream >= 0) {
            st = ctx->side[L.stream];
            if (std::find(used_side.begin(), used_side.end(), L.stream) == used_side.end()) {
                HIPCHK(ctx, hipStreamWaitEvent(st, ctx->fork, 0));
                used_side.push_back(L.stream);
            }
        }
        const int n = (int)L.n;
        const DPTask *tk = d_tasks + L.at;
        const DpGeom g = dp_geom(L);
        const int ld = L.hmax + 6;   // k_dp's ring: doubles per anti-diagonal
        switch (L.k) {
        case DpKernel::Dpr:
        case DpKernel::DprLean:
        case DpKernel::DprLeanPm:
            hipLaunchKernelGGL(dpr_kernel(L), dim3(g.grid), dim3(g.block), g.lds, st, tk, n, d_bases, d_tabs, d_bands,
                               d_out, ctx->d_err, dev<double>(ctx, BUF_BYTES_OR_SINK), d_lut);
            break;
        case DpKernel::DpxCodon:
        case DpKernel::DpxLean:
            hipLaunchKernelGGL((L.k == DpKernel::DpxCodon ? k_dpx<true, true> : k_dpx<false, false>), dim3(g.grid),
                               dim3(g.block), 0, st, tk, n, d_bases, d_tabs, d_bands, d_out, ctx->d_err);
            break;
        case DpKernel::DprWide64:
        case DpKernel::DprWide32: {
            const DprFn fn = L.k == DpKernel::DprWide64 ? k_dpr<2, true, dpl_pmax(2, 64), 64> : k_dpr<2, true, dpl_pmax(2, 32), 32>;
            hipLaunchKernelGGL(fn, dim3(g.grid), dim3(g.block), g.lds, st, tk, n, d_bases, d_tabs, d_bands, d_out,
                               ctx->d_err, dev<double>(ctx, BUF_BYTES_OR_SINK), d_lut);
            break;
        }
        case DpKernel::Dp64:
            hipLaunchKernelGGL((k_dp<64, false>), dim3(g.grid), dim3(g.block), g.lds, st, tk, n, d_bases, d_tabs,
                               d_bands, d_out, ctx->d_err, ld, nullptr);
            break;
        case DpKernel::Dpm: {
            // one workgroup per slice, a band's slices on one XCD; each band is
            // filled with the not-yet-stored pattern first (the slices poll
            // their halo cells)
            const int gm = L.hmax, per = dpm_chunk(gm);
            for (int c0 = 0; c0 < n; c0 += per) {
                const int nc = std::min(per, n - c0);
                bool trim = false;
                for (int i = c0; i < c0 + nc; ++i) {
                    const DPTask &t = plan.tasks[L.at + i];
                    trim = trim || (t.flags & 4);
                    HIPCHK(ctx, hipMemsetAsync(d_bands + t.band, 0xFF, (size_t)t.klen * t.P * 8, st));
                }
                hipLaunchKernelGGL(trim ? k_dpm<true> : k_dpm<false>, dim3((unsigned)(8 * ((nc + 7) / 8) * gm)),
                                   dim3(64), 0, st, tk + c0, nc, gm, d_bases, d_tabs, d_bands, d_out, ctx->d_err);
            }
            break;
        }
        case DpKernel::DpwLds:
        case DpKernel::DpwGlobal: {
            const bool gring = L.k == DpKernel::DpwGlobal;
            hipLaunchKernelGGL((gring ? k_dp<DPW_NT, true, DPW_NT> : k_dp<DPW_NT, false, DPW_NT>), dim3(g.grid),
                               dim3(g.block), g.lds, st, tk, n, d_bases, d_tabs, d_bands, d_out, ctx->d_err, ld,
                               gring ? dev<double>(ctx, BUF_RING_OR_SPLIT) : nullptr);
            break;
        }
        }
    }
    for (int si : used_side) {
        HIPCHK(ctx, hipEventRecord(ctx->join[si], ctx->side[si]));
        HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->join[si], 0));
    }
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

static int realign_run(rf_ctx *ctx, int32_t njobs, const int32_t *slot, const int32_t *seq, const int32_t *tpl,
                       const int32_t *bw, const int32_t *jf, double *out_score)
{
    if (!ctx || njobs < 0 || (njobs > 0 && (!slot || !seq || !tpl || !bw || !jf)))
        return fail(ctx, RF_ERR_ARG, "rf_realign: bad arguments");
    for (int32_t k = 0; k < njobs; ++k)
        if (!(jf[k] & (RF_FWD | RF_BWD)))
            return fail(ctx, RF_ERR_ARG, "rf_realign: need RF_FWD and/or RF_BWD");
    (void)hipSetDevice(ctx->device);
    auto &P = ctx->rplan;
    const size_t nb = sizeof(int32_t) * (size_t)njobs;
    const bool same = P.valid && P.gen == ctx->layout_gen &&
                      P.slot.size() == (size_t)njobs && (njobs == 0 ||
                      (!std::memcmp(P.slot.data(), slot, nb) && !std::memcmp(P.seq.data(), seq, nb) &&
                       !std::memcmp(P.tpl.data(), tpl, nb) && !std::memcmp(P.bw.data(), bw, nb) &&
                       !std::memcmp(P.flags.data(), jf, nb)));
    // the same job list, validated with nothing changed since: its checks and
    // its band bookkeeping would come out the same
    const bool fresh = same && P.val_epoch == ctx->state_epoch;
    if (!fresh)
        if (int e = realign_check(ctx, njobs, slot, seq, tpl, bw))
            return e;
    if (same) {
        if (!fresh) {
            realign_restamp(ctx, njobs, slot, seq, tpl, jf);
            P.val_epoch = ctx->state_epoch;
        }
    } else {
        P.valid = false;
        if (int e = realign_bands(ctx, njobs, slot, seq, tpl, bw, jf))
            return e;
        P.dp = realign_plan(ctx, njobs, slot, seq, tpl, bw, jf);
        if (int e = upload(ctx, ctx->scratch[BUF_DP_TASKS], P.dp.tasks))
            return e;
        P.valid = true;
        P.gen = ctx->layout_gen;
        P.val_epoch = ctx->state_epoch;
        P.flags.assign(jf, jf + njobs);
        P.slot.assign(slot, slot + njobs);
        P.seq.assign(seq, seq + njobs);
        P.tpl.assign(tpl, tpl + njobs);
        P.bw.assign(bw, bw + njobs);
    }
    if (int e = ensure_buf(ctx, ctx->scratch[BUF_DP_SCORES], sizeof(double) * 2 * std::max(njobs, 1)))
        return e;
    double *d_out = dev<double>(ctx, BUF_DP_SCORES);
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_DP_BEGIN], ctx->stream));
    if (int e = launch_dp(ctx, P.dp, d_out))
        return e;
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_DP_END], ctx->stream));
    // the error flag, then the scores, into the landing zone: one wait
    const size_t ob = (out_score && njobs > 0) ? sizeof(double) * njobs : 0;
    if (int e = ensure_landing(ctx, ob))
        return e;
    HIPCHK(ctx, land_flag(ctx));
    if (ob)
        HIPCHK(ctx, land(ctx, 0, d_out, ob));
    HIPCHK(ctx, stream_wait(ctx));
    // the scores and the time go out whether or not a fill raised
    if (ob)
        std::memcpy(out_score, landed<double>(ctx), ob);
    ctx->dp_ms = mark_ms(ctx, EV_DP_BEGIN, EV_DP_END);
    if (int e = check_landed(ctx))
        return e;
    ctx->last_dp = P.dp.launches;
    return 0;
}

// Kernel id, class indices, tasks, stream and launch geometry of a launch, as
// the RF_DPL_FIELDS int32 of the C-ABI
static void dp_launch_record(const DpLaunch &L, int32_t *out)
{
    const DpGeom g = dp_geom(L);
    const int32_t rec[RF_DPL_FIELDS] = {(int32_t)L.k, L.npi, L.pmi, (int32_t)L.at, (int32_t)L.n,
                                        L.stream, (int32_t)g.grid, (int32_t)g.block, (int32_t)g.lds};
    std::copy(rec, rec + RF_DPL_FIELDS, out);
}

int rf_last_dp_launches(const rf_ctx *ctx, int32_t cap, int32_t *launches, int32_t *nlaunches)
{
    if (!ctx || !nlaunches || cap < 0 || (cap > 0 && !launches) || ctx->last_dp.size() > (size_t)cap)
        return RF_ERR_ARG;
    *nlaunches = (int32_t)ctx->last_dp.size();
    for (size_t i = 0; i < ctx->last_dp.size(); ++i)
        dp_launch_record(ctx->last_dp[i], launches + i * RF_DPL_FIELDS);
    return 0;
}

int rf_region_offsets(const rf_ctx *ctx, int32_t slot, int32_t which, int32_t seq, int64_t *band, int64_t *tabs,
                      int64_t *bases)
{
    if (!ctx || (slot < 0 && seq < 0))
        return RF_ERR_ARG;
    // every refusal comes before the first write
    const Band *b = nullptr;
    if (slot >= 0) {
        if (!band || slot >= (int32_t)ctx->slots.size() || (which != RF_BAND_A && which != RF_BAND_B))
            return RF_ERR_ARG;
        b = which == RF_BAND_A ? &ctx->slots[slot].a : &ctx->slots[slot].b;
        if (b->r.off < 0)
            return RF_ERR_ARG;
    }
    const SeqObj *S = nullptr;
    if (seq >= 0) {
        if (!tabs || !bases || seq >= (int32_t)ctx->seqs.size() || !ctx->seqs[seq].valid)
            return RF_ERR_ARG;
        S = &ctx->seqs[seq];
    }
    if (b) {
        band[0] = b->r.off;
        band[1] = b->r.cap;
    }
    if (S) {
        tabs[0] = S->tabs.off;
        tabs[1] = S->tabs.cap;
        bases[0] = S->bases.off;
        bases[1] = S->bases.cap;
    }
    return 0;
}

int rf_host_dp_plan(int32_t njobs, const int32_t *n, const int32_t *m, const int32_t *bw, const int32_t *flags,
                    const int32_t *ncins, const int32_t *ncdel, const uint8_t *finite, const int32_t *stride_a,
                    const int32_t *stride_b, int32_t nopt, const int32_t *opt_key, const int32_t *opt_val,
                    int32_t *task_job, int32_t *task_dir, int32_t *task_launch, int32_t *task_out,
                    int32_t *ntasks, int32_t launch_cap, int32_t *launches, int32_t *nlaunches)
{
    if (njobs < 0 || nopt < 0 || launch_cap < 0 || !ntasks || !nlaunches || (launch_cap > 0 && !launches) ||
        (nopt > 0 && (!opt_key || !opt_val)) ||
        (njobs > 0 && (!n || !m || !bw || !flags || !ncins || !ncdel || !finite || !task_job || !task_dir ||
                       !task_launch || !task_out)))
        return RF_ERR_ARG;
    DpOpts o;
    for (int32_t i = 0; i < nopt; ++i) {
        int *v = dp_opt(o, opt_key[i]);
        if (!v)
            return RF_ERR_ARG;
        *v = opt_val[i];
    }
    for (int32_t k = 0; k < njobs; ++k) {
        // H, K = H + 2 m and K P 8 in range: a stride holds its row pairs and is no wider than a band's
        const int64_t H = 2 * (int64_t)bw[k] + std::abs((int64_t)n[k] - m[k]) + 1;
        if (n[k] < 0 || m[k] < 0 || bw[k] < 1 || ncins[k] < 0 || ncdel[k] < 0 || !(flags[k] & (RF_FWD | RF_BWD)) ||
            H + 2 * (int64_t)m[k] > INT32_MAX / 2)
            return RF_ERR_ARG;
        for (const int32_t *stride : {stride_a, stride_b})
            if (stride && (stride[k] < (H + 1) / 2 || stride[k] > (H + 1) / 2 + 16))
                return RF_ERR_ARG;
    }
    std::vector<DPTask> tasks;
    std::vector<uint8_t> fin;
    for_each_fill(njobs, flags, [&](int dir, int32_t k) {
        SeqObj S;
        TplObj T;
        S.n = n[k];
        S.ncins = ncins[k];
        S.ncdel = ncdel[k];
        T.m = m[k];
        const int32_t *stride = dir == 0 ? stride_a : stride_b;
        const int P = stride ? stride[k] : band_P(band_rows(S.n + 1, T.m + 1, bw[k]));
        tasks.push_back(realign_task(S, T, bw[k], flags[k], dir, k, njobs, k, P));   // band: the job, for the report
        fin.push_back(finite[k]);
        return 0;
    });
    const DpPlan plan = dp_plan(tasks, fin, o);
    if (plan.launches.size() > (size_t)launch_cap)
        return RF_ERR_ARG;
    *ntasks = (int32_t)plan.tasks.size();
    *nlaunches = (int32_t)plan.launches.size();
    for (size_t i = 0; i < plan.launches.size(); ++i) {
        const DpLaunch &L = plan.launches[i];
        dp_launch_record(L, launches + i * RF_DPL_FIELDS);
        for (size_t j = L.at; j < L.at + L.n; ++j) {
            task_job[j] = (int32_t)plan.tasks[j].band;
            task_dir[j] = plan.tasks[j].flags & 1;
            task_launch[j] = (int32_t)i;
            task_out[j] = plan.tasks[j].out_idx;
        }
    }
    return 0;
}

int rf_realign(rf_ctx *ctx, int32_t njobs, const int32_t *slot, const int32_t *seq,
               const int32_t *tpl, const int32_t *bw, int32_t flags, double *out_score)
{
    if (!ctx || njobs < 0)
        return fail(ctx, RF_ERR_ARG, "rf_realign: bad arguments");
    ctx->jflags.assign((size_t)njobs, flags);
    return realign_impl(ctx, njobs, slot, seq, tpl, bw, ctx->jflags.data(), out_score);
}

int rf_realign_jobs(rf_ctx *ctx, int32_t njobs, const int32_t *slot, const int32_t *seq, const int32_t *tpl,
                    const int32_t *bw, const int32_t *flags, double *out_score)
{
    return realign_impl(ctx, njobs, slot, seq, tpl, bw, flags, out_score);
}

// ---- rf_pair_scores / rf_pair_align: the checks, the launch plan and the fill launches they share ----

// The refusal of a band that no pair kernel holds.  k: the pair (-1:
// rf_pair_scores, which names none); mb: the bandwidth after the last
// doubling (-1: the call's own).  Both are indices / bandwidths the checks
// have found non-negative, so a negative value can only mean "not named".
enum class PairCall { Scores, Align, Errors };   // rf_pair_scores | rf_pair_align* | rf_pair_errors

static std::string band_too_wide(const std::string &fn, int64_t H, int64_t k, int64_t mb = -1)
{
    return fn + ": band of " + std::to_string(H) + " rows" +
           (mb >= 0 ? " at the largest bandwidth " + std::to_string(mb) : std::string()) +
           (k >= 0 ? " (pair " + std::to_string(k) + ")" : std::string()) + " is wider than the " +
           std::to_string(DPW_LDS_H) + (k >= 0 ? " a bandless" : " a score-only") + " pass holds in LDS";
}

// The band check of one pair: H rows (at bandwidth mb where that is not the
// call's own) against template length m.  Without RF_OPT_PAIR_WIDE the LDS
// limit; with it the wide tier's limits (include/rifraf_hip.h).  Empty: fits.
static std::string pair_band_fault(const rf_ctx *ctx, const std::string &fn, PairCall call, int64_t H, int64_t m,
                                   int64_t k, int64_t mb = -1)
{
    const bool align = call != PairCall::Scores;
    if (H <= DPW_LDS_H)
        return {};
    if (ctx->opt.pair_wide <= 0)
        return band_too_wide(fn, H, align ? k : -1, mb);
    const std::string who = fn + ": band of " + std::to_string(H) + " rows (pair " + std::to_string(k) + ")";
    if (H > PW_MAX_H)
        return who + " is wider than the " + std::to_string(PW_MAX_H) + " the wide tier takes";
    if (H + 2 * m > INT32_MAX)
        return who + ": H + 2 m does not fit 32 bits";
    // the lane walk indexes a pair's trace words with 32 bits
    if (call == PairCall::Align && (int64_t)pa_blocks((int)(H + 2 * m)) * pa_hp((int)H) > INT32_MAX)
        return who + ": its move trace has 2^31 words or more";
    return {};
}

// Argument, flag and per-pair checks.  `fn` names the entry point in the
// messages; `outs_ok` is its check of its own output pointers; `call` gives
// the wording (rf_pair_errors takes rf_pair_align's) and the timers that are
// reset.
static int pair_check(rf_ctx *ctx, const std::string &fn, PairCall call, bool outs_ok, int64_t npairs,
                      const int32_t *seq, const int32_t *tpl, const int32_t *bw, int32_t flags)
{
    const bool align = call != PairCall::Scores;
    if (!(ctx && npairs >= 0 && (npairs == 0 || (seq && tpl && bw)) && outs_ok))
        return fail(ctx, RF_ERR_ARG, fn + ": bad arguments");
    if (flags & RF_BWD)
        return fail(ctx, RF_ERR_ARG,
                    fn + ": RF_BWD is not supported (forward " + (align ? "alignments" : "scores") + " only)");
    if (flags & ~(RF_FWD | RF_SKEW | RF_TRIM))
        return fail(ctx, RF_ERR_ARG, fn + ": unknown flags");
    (void)hipSetDevice(ctx->device);
    if (call == PairCall::Errors)
        ctx->pe_ms = 0;
    else if (align)
        ctx->pa_fill_ms = ctx->pa_walk_ms = ctx->pa_emit_ms = ctx->pa_fix_ms = 0;
    else
        ctx->pair_ms = 0;
    for (int64_t k = 0; k < npairs; ++k) {
        if (seq[k] < 0 || seq[k] >= (int32_t)ctx->seqs.size() || !ctx->seqs[seq[k]].valid || tpl[k] < 0 ||
            tpl[k] >= (int32_t)ctx->tpls.size() || !ctx->tpls[tpl[k]].valid)
            return fail(ctx, RF_ERR_ARG, fn + ": unknown sequence / template");
        if (bw[k] < 1)
            return fail(ctx, RF_ERR_ARG, "bandwidth must be positive");
        const int64_t H = 2 * (int64_t)bw[k] + std::abs((int64_t)ctx->seqs[seq[k]].n - ctx->tpls[tpl[k]].m) + 1;
        const std::string why = pair_band_fault(ctx, fn, call, H, ctx->tpls[tpl[k]].m, k);
        if (!why.empty())
            return fail(ctx, RF_ERR_ARG, why);
    }
    return 0;
}

// The wide class of a plan under the context's ring budget (RF_OPT_PAIR_RING_MB)
static PairWidePlan pair_wide_ring(const rf_ctx *ctx, const PairPlan &pl, bool count)
{
    return pair_wide_plan((int64_t)pl.cls[6].size(), pl.hmax[2], count,
                          (int64_t)std::max(ctx->opt.pair_ring_mb, 0) << 20);
}

// The fill launches of a plan whose tasks are in BUF_PAIR_TASKS: k_pa* into
// the trace d_tr, k_pe* with the counts d_cnt (bands up to DP_COUNT_H; never
// both), k_ps* with neither.
static int pair_fill(rf_ctx *ctx, const PairPlan &pl, double *d_out, uint64_t *d_tr, int32_t *d_cnt)
{
    const DPTask *d_tasks = dev<const DPTask>(ctx, BUF_PAIR_TASKS);
    const uint8_t *d_bases = (const uint8_t *)ctx->bytes_arena.d;
    const double *d_tabs = (const double *)ctx->tab_arena.d;
    const double *d_lut = (const double *)ctx->codes.lut.p;
    using KsFn = void (*)(const DPTask *, int, const uint8_t *, const double *, double *, const double *);
    using KaFn = void (*)(const DPTask *, int, const uint8_t *, const double *, double *, const double *, uint64_t *);
    const KsFn ks[4] = {k_ps<1>, k_ps<2>, k_ps<4>, k_ps<2, 64>};
    const KaFn ka[4] = {k_pa<1>, k_pa<2>, k_pa<4>, k_pa<2, 64>};
    using KeFn = void (*)(const DPTask *, int, const uint8_t *, const double *, double *, const double *, int32_t *);
    const KeFn ke[4] = {k_pe<1>, k_pe<2>, k_pe<4>, k_pe<2, 64>};
    for (int a = 0; a < 4; ++a)
        if (const int n = (int)pl.cls[a].size()) {
            const int tpw = a == 3 ? 1 : 4;
            const dim3 grid((n + tpw - 1) / tpw);
            if (d_tr)
                hipLaunchKernelGGL(ka[a], grid, dim3(64), 0, ctx->stream, d_tasks + pl.at[a], n, d_bases, d_tabs,
                                   d_out, d_lut, d_tr);
            else if (d_cnt)
                hipLaunchKernelGGL(ke[a], grid, dim3(64), 0, ctx->stream, d_tasks + pl.at[a], n, d_bases, d_tabs,
                                   d_out, d_lut, d_cnt);
            else
                hipLaunchKernelGGL(ks[a], grid, dim3(64), 0, ctx->stream, d_tasks + pl.at[a], n, d_bases, d_tabs,
                                   d_out, d_lut);
        }
    for (int g = 0; g < 2; ++g)
        if (const unsigned n = (unsigned)pl.cls[4 + g].size()) {
            const int ld = pl.hmax[g] + 6;   // the LDS ring: 4 anti-diagonals of ld doubles
            const size_t lds = 4 * (size_t)ld * 8;
            const DPTask *tk = d_tasks + pl.at[4 + g];
            if (d_cnt) {
                // the count ring behind the score ring: 4 anti-diagonals of ld int32
                if (g == 0)
                    hipLaunchKernelGGL(k_pe_gen<64>, dim3(n), dim3(64), lds + lds / 2, ctx->stream, tk, d_bases,
                                       d_tabs, d_out, d_cnt, ld);
                else
                    hipLaunchKernelGGL(k_pe_gen<DPW_NT>, dim3(n), dim3(DPW_NT), lds + lds / 2, ctx->stream, tk,
                                       d_bases, d_tabs, d_out, d_cnt, ld);
            } else if (g == 0 && d_tr)
                hipLaunchKernelGGL((k_pa_gen<64, PA_NPP64>), dim3(n), dim3(64), lds, ctx->stream, tk, d_bases,
                                   d_tabs, d_out, d_tr, ld);
            else if (g == 0)
                hipLaunchKernelGGL(k_ps_gen<64>, dim3(n), dim3(64), lds, ctx->stream, tk, d_bases, d_tabs, d_out, ld);
            else if (d_tr)
                hipLaunchKernelGGL((k_pa_gen<DPW_NT, PA_NPPW>), dim3(n), dim3(DPW_NT), lds, ctx->stream, tk,
                                   d_bases, d_tabs, d_out, d_tr, ld);
            else
                hipLaunchKernelGGL(k_ps_gen<DPW_NT>, dim3(n), dim3(DPW_NT), lds, ctx->stream, tk, d_bases, d_tabs,
                                   d_out, ld);
        }
    if (const int n = (int)pl.cls[6].size()) {
        // the wide tier: the workgroups the ring budget holds loop over the class (BUF_PAIR_RING: pair_stage)
        const PairWidePlan wp = pair_wide_ring(ctx, pl, d_cnt != nullptr);
        const DPTask *tk = d_tasks + pl.at[6];
        double *d_ring = dev<double>(ctx, BUF_PAIR_RING);
        const dim3 grid((unsigned)wp.nwg);
        if (d_tr)
            hipLaunchKernelGGL(k_pa_wide, grid, dim3(DPW_NT), 0, ctx->stream, tk, n, d_bases, d_tabs, d_out, d_tr,
                               d_ring, (int)wp.ring_ld);
        else if (d_cnt)
            hipLaunchKernelGGL(k_pe_wide, grid, dim3(DPW_NT), 0, ctx->stream, tk, n, d_bases, d_tabs, d_out, d_cnt,
                               d_ring, (int)wp.ring_ld);
        else
            hipLaunchKernelGGL(k_ps_wide, grid, dim3(DPW_NT), 0, ctx->stream, tk, n, d_bases, d_tabs, d_out, d_ring,
                               (int)wp.ring_ld);
    }
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

int rf_host_pair_wide_plan(int64_t npairs, const int32_t *H, int32_t mode, int64_t budget, int64_t *nwg,
                           int64_t *ring_ld, int64_t *ring_bytes)
{
    if (npairs < 1 || !H || mode < PS_SCORE || mode > PS_COUNT || budget < 0 || !nwg || !ring_ld || !ring_bytes)
        return RF_ERR_ARG;
    int32_t hmax = 0;
    for (int64_t k = 0; k < npairs; ++k) {
        if (H[k] < 1 || H[k] > PW_MAX_H)
            return RF_ERR_ARG;
        hmax = std::max(hmax, H[k]);
    }
    const PairWidePlan p = pair_wide_plan(npairs, hmax, mode == PS_COUNT, budget);
    *nwg = p.nwg;
    *ring_ld = p.ring_ld;
    *ring_bytes = p.ring_bytes;
    return 0;
}

int rf_last_pair_ms(const rf_ctx *ctx, double *ms)
{
    if (!ctx || !ms)
        return RF_ERR_ARG;
    *ms = ctx->pair_ms;
    return 0;
}

// Which walk a launch set takes: RF_OPT_PAIR_WALK, or with 0 (auto) the rule
// measured by scripts/pair_align_timing.py --walk-ab (DESIGN.md §4,
// profiles/pair_align_smart_timing.json): the wave walk from a mean n + m of
// PAW_MIN_NM.  62,500 pairs at bw 9: n + m = 60, 120, 301 -> the lane walk is
// faster (wave / lane time 1.80, 1.50, 1.14); 802, 3,006 -> the wave walk
// (0.86, 0.57).  At n + m = 20,037 the wave walk took 0.10-0.14 of the lane
// walk's time for 16, 128, 1,024 and 4,096 pairs alike, so the number of
// pairs does not enter the rule.
constexpr int PAW_MIN_NM = 512;
static bool pair_walk_wave(const rf_ctx *ctx, int64_t cn, int64_t mv_total)
{
    if (ctx->opt.pair_walk != 0)
        return ctx->opt.pair_walk == 2;
    return mv_total >= (int64_t)PAW_MIN_NM * cn;
}

struct PairText {   // rf_pair_align_text's outputs, each NULL or indexed by the pair's own k
    uint8_t *aln_t, *aln_s;
    const int64_t *aln_off;
    int32_t *aln_len, *t2s;
    const int64_t *t2s_off;
    int32_t *t2s_len, *tolerance;
    bool any() const { return aln_t || aln_len || t2s || t2s_len || tolerance; }
};

struct PairFix {   // rf_pair_shifts' outputs, each NULL or indexed by the pair's own k
    uint8_t *fixed;
    const int64_t *fixed_off;
    int32_t *fixed_len, *nprops;
    const int64_t *prop_off;
    uint8_t *prop_kind;
    int32_t *prop_pos;
    uint8_t *prop_base;
    int32_t *tally;
    bool any() const { return fixed || fixed_len || nprops || prop_kind || tally; }
};

// The pairs of one pair_run and where their results go.  List position i is
// pair at(i); seq, tpl, bw and every output are indexed by the pair's own k.
struct PairIo {
    int64_t nidx;
    const int64_t *idx;   // NULL: the pairs 0 .. nidx - 1
    const int32_t *seq, *tpl, *bw;
    int fl;               // fill_flags of the call
    double *out_score;
    int8_t *moves;
    const int64_t *moves_off;
    int32_t *nmoves, *nerrors;
    const PairText *tx;   // may be NULL
    bool errors = false;  // rf_pair_errors: counts carried by the fills, kernel time to its own timer
    const PairFix *fx = nullptr;   // rf_pair_shifts: k_pa_fix's products
    int64_t at(int64_t i) const { return idx ? idx[i] : i; }
};
// sees a pair's k, score, nmoves and nerrors; says whether its moves and texts go to the caller
using PairEnded = std::function<bool(int64_t, double, int32_t, int32_t)>;

// Step 1 of a launch set: its descriptors on the device, room for its products
static int pair_stage(rf_ctx *ctx, const PairSet &s, const PairLanding &L, const PairWants &w)
{
    DevBuf *b = ctx->scratch;
    if (int e = upload(ctx, b[BUF_PAIR_TASKS], s.pl.all))
        return e;
    if (int e = ensure_buf(ctx, b[BUF_PAIR_SCORES], L.scores))
        return e;
    if (w.trace)
        if (int e = ensure_buf(ctx, b[BUF_PAIR_TRACE], (size_t)std::max<int64_t>(s.tr_at, 2) * 8))
            return e;
    if (w.walk && w.want_mv()) {
        if (int e = ensure_buf(ctx, b[BUF_PAIR_MOVES], L.mv_dev))
            return e;
        if (int e = upload(ctx, b[BUF_PAIR_MOVE_OFF], s.mvoff))
            return e;
    }
    if (w.walk || w.count)
        if (int e = ensure_buf(ctx, b[BUF_PAIR_COUNTS], L.counts))
            return e;
    if (!s.pl.cls[6].empty())
        if (int e = ensure_buf(ctx, b[BUF_PAIR_RING], (size_t)pair_wide_ring(ctx, s.pl, w.count).ring_bytes))
            return e;
    if (w.want_txt) {
        if (int e = ensure_buf(ctx, b[BUF_PAIR_TEXT_T], L.mv_dev))
            return e;
        if (int e = ensure_buf(ctx, b[BUF_PAIR_TEXT_S], L.mv_dev))
            return e;
    }
    if (w.want_ix) {
        if (int e = ensure_buf(ctx, b[BUF_PAIR_INDEX], L.ix_dev))
            return e;
        if (int e = upload(ctx, b[BUF_PAIR_INDEX_OFF], s.ixoff))
            return e;
    }
    if (w.emit)
        if (int e = ensure_buf(ctx, b[BUF_PAIR_LENGTHS], L.lens))
            return e;
    if (w.fix)
        if (int e = ensure_buf(ctx, b[BUF_PAIR_FIX_OUT], L.fixes))
            return e;
    if (w.want_fixed)
        if (int e = ensure_buf(ctx, b[BUF_PAIR_FIXED], L.mv_dev))
            return e;
    if (w.want_rec) {
        if (int e = ensure_buf(ctx, b[BUF_PAIR_PROP_KB], L.kb_dev))
            return e;
        if (int e = ensure_buf(ctx, b[BUF_PAIR_PROP_POS], L.pos_dev))
            return e;
        if (int e = upload(ctx, b[BUF_PAIR_PROP_OFF], s.proff))
            return e;
    }
    return ensure_landing(ctx, L.total);
}

// Step 2: the fills, then with a trace the walk (k_pa_walk_w or k_pa_walk by
// pair_walk_wave) and k_pa_emit or k_pa_fix over the moves the walk left.  With
// PairWants::count the fills are the set's only kernels, between marks of
// their own.
static int pair_launch(rf_ctx *ctx, const PairSet &s, const PairWants &w)
{
    const int64_t cn = s.cn;
    const uint8_t *d_bases = (const uint8_t *)ctx->bytes_arena.d;
    const DPTask *d_tasks = dev<const DPTask>(ctx, BUF_PAIR_TASKS);
    double *d_out = dev<double>(ctx, BUF_PAIR_SCORES);
    uint64_t *d_tr = w.trace ? dev<uint64_t>(ctx, BUF_PAIR_TRACE) : nullptr;
    int8_t *d_mv = w.want_mv() ? dev<int8_t>(ctx, BUF_PAIR_MOVES) : nullptr;
    const int64_t *d_mvoff = dev<const int64_t>(ctx, BUF_PAIR_MOVE_OFF);
    int32_t *d_cnt = dev<int32_t>(ctx, BUF_PAIR_COUNTS);
    HIPCHK(ctx, hipEventRecord(ctx->ev[w.count ? EV_PAIR_ERRORS_BEGIN : EV_PAIR_FILL_BEGIN], ctx->stream));
    if (int e = pair_fill(ctx, s.pl, d_out, d_tr, w.count ? d_cnt : nullptr))
        return e;
    HIPCHK(ctx, hipEventRecord(ctx->ev[w.count ? EV_PAIR_ERRORS_END : EV_PAIR_FILL_END], ctx->stream));
    if (!w.trace)
        return 0;
    if (w.walk) {
        if (pair_walk_wave(ctx, cn, s.mv_total))
            hipLaunchKernelGGL(k_pa_walk_w, dim3((unsigned)((cn + PAW_NW - 1) / PAW_NW)), dim3(64 * PAW_NW), 0,
                               ctx->stream, d_tasks, (int)cn, d_bases, (const double *)d_out,
                               (const uint64_t *)d_tr, d_mv, d_mvoff, d_cnt, d_cnt + cn);
        else
            hipLaunchKernelGGL(k_pa_walk, dim3((unsigned)((cn + 63) / 64)), dim3(64), 0, ctx->stream, d_tasks,
                               (int)cn, d_bases, (const double *)d_out, (const uint64_t *)d_tr, d_mv, d_mvoff,
                               d_cnt, d_cnt + cn);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_PAIR_WALK_END], ctx->stream));
    if (w.emit) {
        hipLaunchKernelGGL(k_pa_emit, dim3((unsigned)((cn + PAW_NW - 1) / PAW_NW)), dim3(64 * PAW_NW), 0,
                           ctx->stream, d_tasks, (int)cn, d_bases, (const int8_t *)d_mv, d_mvoff,
                           (const int32_t *)d_cnt, w.want_txt ? dev<uint8_t>(ctx, BUF_PAIR_TEXT_T) : nullptr,
                           w.want_txt ? dev<uint8_t>(ctx, BUF_PAIR_TEXT_S) : nullptr,
                           w.want_ix ? dev<int32_t>(ctx, BUF_PAIR_INDEX) : nullptr,
                           dev<const int64_t>(ctx, BUF_PAIR_INDEX_OFF), dev<int32_t>(ctx, BUF_PAIR_LENGTHS));
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipEventRecord(ctx->ev[EV_PAIR_EMIT_END], ctx->stream));
    }
    if (w.fix) {   // never with emit: its time runs from EV_PAIR_WALK_END
        hipLaunchKernelGGL(k_pa_fix, dim3((unsigned)((cn + PAW_NW - 1) / PAW_NW)), dim3(64 * PAW_NW), 0,
                           ctx->stream, d_tasks, (int)cn, d_bases, (const int8_t *)d_mv, d_mvoff,
                           (const int32_t *)d_cnt, w.want_fixed ? dev<uint8_t>(ctx, BUF_PAIR_FIXED) : nullptr,
                           w.want_rec ? dev<uint8_t>(ctx, BUF_PAIR_PROP_KB) : nullptr,
                           w.want_rec ? dev<int32_t>(ctx, BUF_PAIR_PROP_POS) : nullptr,
                           dev<const int64_t>(ctx, BUF_PAIR_PROP_OFF), dev<int32_t>(ctx, BUF_PAIR_FIX_OUT));
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipEventRecord(ctx->ev[EV_PAIR_FIX_END], ctx->stream));
    }
    return 0;
}

// Step 3: the set's products into the pinned landing zone, and the wait
static int pair_download(rf_ctx *ctx, const PairSet &s, const PairLanding &L, const PairWants &w)
{
    const size_t mv = (size_t)s.mv_total;
    auto get = [&](size_t at, Buf b, size_t bytes) { return land(ctx, at, ctx->scratch[b].p, bytes); };
    HIPCHK(ctx, get(0, BUF_PAIR_SCORES, L.scores));
    if (w.walk || w.count)
        HIPCHK(ctx, get(L.scores, BUF_PAIR_COUNTS, L.counts));
    if (w.walk && w.get_mv && mv > 0)
        HIPCHK(ctx, get(L.mv_at, BUF_PAIR_MOVES, mv));
    if (w.emit)
        HIPCHK(ctx, get(L.len_at, BUF_PAIR_LENGTHS, L.lens));
    if (w.want_txt && mv > 0) {
        HIPCHK(ctx, get(L.txt_at, BUF_PAIR_TEXT_T, mv));
        HIPCHK(ctx, get(L.txt_at + mv, BUF_PAIR_TEXT_S, mv));
    }
    if (w.want_ix && s.ix_total > 0)
        HIPCHK(ctx, get(L.ix_at, BUF_PAIR_INDEX, sizeof(int32_t) * (size_t)s.ix_total));
    if (w.fix)
        HIPCHK(ctx, get(L.fix_at, BUF_PAIR_FIX_OUT, L.fixes));
    if (w.want_fixed && mv > 0)
        HIPCHK(ctx, get(L.fixed_at, BUF_PAIR_FIXED, mv));
    if (w.want_rec && s.pr_total > 0) {
        HIPCHK(ctx, get(L.kb_at, BUF_PAIR_PROP_KB, (size_t)s.pr_total));
        HIPCHK(ctx, get(L.pos_at, BUF_PAIR_PROP_POS, sizeof(int32_t) * (size_t)s.pr_total));
    }
    HIPCHK(ctx, stream_wait(ctx));
    return 0;
}

// Step 4: the landed products to the caller's arrays, for the set's pairs
// io.at(p0 ..), and the kernel times
static void pair_collect(rf_ctx *ctx, const PairIo &io, int64_t p0, const PairSet &s, const PairLanding &L,
                         const PairWants &w, const PairEnded &ended)
{
    const int64_t cn = s.cn;
    const char *h = landed<char>(ctx);
    const double *sc = landed<double>(ctx);
    const int32_t *cnt = landed<int32_t>(ctx, L.scores);
    const int32_t *len = landed<int32_t>(ctx, L.len_at);   // aln_len, t2s_len, tolerance: cn of each
    const int32_t *fix = landed<int32_t>(ctx, L.fix_at);   // fixed_len, nprops, the five tallies: cn of each
    const PairText *tx = io.tx;
    for (int64_t i = 0; i < cn; ++i) {
        const int64_t k = io.at(p0 + i);
        if (io.out_score)
            io.out_score[k] = sc[i];
        if (!w.walk)
            continue;
        // the walk's counts are nmoves, then nerrors; the counting fills leave nerrors alone
        const int32_t nmv = w.count ? -1 : cnt[i], nerr = w.count ? cnt[i] : cnt[cn + i];
        if (io.nmoves)
            io.nmoves[k] = nmv;
        if (io.nerrors)
            io.nerrors[k] = nerr;
        if (ended && !ended(k, sc[i], nmv, nerr))
            continue;
        if (w.get_mv && cnt[i] > 0) {   // the walk leaves the moves at the end of the pair's n + m slot
            const int64_t slot = (i + 1 < cn ? s.mvoff[(size_t)i + 1] : s.mv_total) - s.mvoff[(size_t)i];
            std::memcpy(io.moves + io.moves_off[k], h + L.mv_at + s.mvoff[(size_t)i] + slot - cnt[i], (size_t)cnt[i]);
        }
        if (w.fix) {   // k_pa_fix writes the corrected template from the start of the slot
            const PairFix *fx = io.fx;
            const int32_t fl = fix[i], np = fix[cn + i];
            if (fx->fixed_len)
                fx->fixed_len[k] = fl;
            if (fx->nprops)
                fx->nprops[k] = np;
            for (int c = 0; fx->tally && c < SF_TALLIES; ++c)
                fx->tally[k * SF_TALLIES + c] = fix[(2 + c) * cn + i];
            if (w.want_fixed && fl > 0)
                std::memcpy(fx->fixed + fx->fixed_off[k], h + L.fixed_at + s.mvoff[(size_t)i], (size_t)fl);
            if (w.want_rec) {   // the first `capacity` records; a failed pair (-1) has none
                const int64_t r0 = s.proff[(size_t)i], nr = std::min<int64_t>(np, s.proff[(size_t)i + 1] - r0);
                const uint8_t *kb = (const uint8_t *)h + L.kb_at + r0;
                const int32_t *pos = (const int32_t *)(h + L.pos_at) + r0;
                for (int64_t r = 0; r < nr; ++r) {
                    fx->prop_kind[fx->prop_off[k] + r] = kb[r] & 15;
                    fx->prop_base[fx->prop_off[k] + r] = kb[r] >> 4;
                    fx->prop_pos[fx->prop_off[k] + r] = pos[r];
                }
            }
        }
        if (!w.emit)
            continue;
        const int32_t al = len[i], il = len[cn + i];
        if (tx->aln_len)
            tx->aln_len[k] = al;
        if (tx->t2s_len)
            tx->t2s_len[k] = il;
        if (tx->tolerance)
            tx->tolerance[k] = len[2 * cn + i];
        if (w.want_txt && al > 0) {   // k_pa_emit writes the texts from the start of the slot
            std::memcpy(tx->aln_t + tx->aln_off[k], h + L.txt_at + s.mvoff[(size_t)i], (size_t)al);
            std::memcpy(tx->aln_s + tx->aln_off[k], h + L.txt_at + s.mv_total + s.mvoff[(size_t)i], (size_t)al);
        }
        if (w.want_ix && il > 0)
            std::memcpy(tx->t2s + tx->t2s_off[k], h + L.ix_at + sizeof(int32_t) * (size_t)s.ixoff[(size_t)i],
                        sizeof(int32_t) * (size_t)il);
    }
    if (w.count) {
        ctx->pe_ms += mark_ms(ctx, EV_PAIR_ERRORS_BEGIN, EV_PAIR_ERRORS_END);
        return;
    }
    if (io.errors) {   // its pairs above DP_COUNT_H: the trace fill and the walk
        ctx->pe_ms += mark_ms(ctx, EV_PAIR_FILL_BEGIN, EV_PAIR_WALK_END);
        return;
    }
    if (!w.trace) {
        ctx->pair_ms += mark_ms(ctx, EV_PAIR_FILL_BEGIN, EV_PAIR_FILL_END);
        return;
    }
    ctx->pa_fill_ms += mark_ms(ctx, EV_PAIR_FILL_BEGIN, EV_PAIR_FILL_END);
    ctx->pa_walk_ms += mark_ms(ctx, EV_PAIR_FILL_END, EV_PAIR_WALK_END);
    if (w.emit)
        ctx->pa_emit_ms += mark_ms(ctx, EV_PAIR_WALK_END, EV_PAIR_EMIT_END);
    if (w.fix)
        ctx->pa_fix_ms += mark_ms(ctx, EV_PAIR_WALK_END, EV_PAIR_FIX_END);
}

// The launch sets of a pair call: the pairs of `io` in sets of at most
// RF_OPT_PAIR_CHUNK pairs and, with w.trace, RF_OPT_PAIR_TRACE_MB of trace
// (pair_set_end), so one set's buffers (BUF_PAIR_*) are all the device memory
// a call needs, whatever its size.  Within a set the pairs are sorted into
// width classes, longest first.  `ended` (may be empty) sees a pair's score
// and counts and says whether its moves and k_pa_emit's products go to the
// caller; without it every pair's do.
static int pair_sets(rf_ctx *ctx, const PairIo &io, const PairWants &w, const PairEnded &ended)
{
    const int64_t chunk = std::max(ctx->opt.pair_chunk, 1);
    const int64_t budget = (int64_t)std::max(ctx->opt.pair_trace_mb, 1) << 20;   // bytes of trace per set
    PairSet s;
    s.pl.wide_from = pair_wide_from(ctx->opt.pair_wide);
    for (int64_t p0 = 0; p0 < io.nidx; p0 += s.cn) {
        const int64_t p1 = pair_set_end(p0, io.nidx, chunk, w.trace, budget, [&](int64_t i) {
            const int64_t k = io.at(i);
            return PairDims{ctx->seqs[io.seq[k]].n, ctx->tpls[io.tpl[k]].m, io.bw[k]};
        });
        pair_set_fill(s, p1 - p0, w.trace, [&](int64_t i, bool *finite) {
            const int64_t k = io.at(p0 + i);
            const SeqObj &S = ctx->seqs[io.seq[k]];
            *finite = S.finite;
            return pair_task(S, ctx->tpls[io.tpl[k]], io.bw[k], io.fl, (int32_t)i);
        });
        if (w.want_rec)
            pair_set_records(s, [&](int64_t i) {
                const int64_t k = io.at(p0 + i);
                return io.fx->prop_off[k + 1] - io.fx->prop_off[k];
            });
        const PairLanding L = pair_landing(s.cn, s.mv_total, s.ix_total, w, s.pr_total);
        if (int e = pair_stage(ctx, s, L, w))
            return e;
        if (int e = pair_launch(ctx, s, w))
            return e;
        if (int e = pair_download(ctx, s, L, w))
            return e;
        pair_collect(ctx, io, p0, s, L, w, ended);
    }
    return 0;
}

// The body of every pair call (one round of rf_pair_align_smart).  Without
// `trace` (rf_pair_scores) the fills are k_ps*, score-only, and nothing
// follows them.  `walk`: run the walk (counts, and moves where asked for);
// with io.tx, k_pa_emit then runs over the moves (with io.fx, k_pa_fix),
// which are downloaded only if io.moves asks for them.
//
// With io.errors (rf_pair_errors) the pairs whose band is within DP_COUNT_H
// (and the wide tier's, RF_OPT_PAIR_WIDE) run first, in sets of their own, through the counting fills (k_pe*): no
// trace, no walk, sets by the chunk alone.  The pairs above it follow through
// the trace fill and the walk.
static int pair_run(rf_ctx *ctx, const PairIo &io, bool trace, bool walk, const PairEnded &ended)
{
    if (!io.errors) {
        const bool emit = walk && io.tx && io.tx->any();
        PairWants w{trace, walk, io.moves != nullptr, emit, emit && io.tx->aln_t, emit && io.tx->t2s};
        w.fix = walk && io.fx && io.fx->any();
        w.want_fixed = w.fix && io.fx->fixed;
        w.want_rec = w.fix && io.fx->prop_kind;
        return pair_sets(ctx, io, w, ended);
    }
    std::vector<int64_t> part[2];   // the pairs that carry their count | that take the trace
    for (int64_t i = 0; i < io.nidx; ++i) {
        const int64_t k = io.at(i);
        const int H = band_rows(ctx->seqs[io.seq[k]].n + 1, ctx->tpls[io.tpl[k]].m + 1, io.bw[k]);
        // a wide pair (RF_OPT_PAIR_WIDE) carries its count in k_pe_wide, whatever its width
        part[H > DP_COUNT_H && H < pair_wide_from(ctx->opt.pair_wide)].push_back(k);
    }
    for (int g = 0; g < 2; ++g) {
        if (part[g].empty())
            continue;
        PairIo sub = io;
        sub.nidx = (int64_t)part[g].size();
        sub.idx = part[g].data();
        PairWants w{g == 1, walk, false, false, false, false};
        w.count = g == 0;
        if (int e = pair_sets(ctx, sub, w, ended))
            return e;
    }
    return 0;
}

// Score-only forward pass of independent pairs (k_ps / k_ps_gen).  Reads the
// sequence and template arenas only: no slot, no band, no band bookkeeping.
int rf_pair_scores(rf_ctx *ctx, int64_t npairs, const int32_t *seq, const int32_t *tpl, const int32_t *bw,
                   int32_t flags, double *out)
{
    if (int e = pair_check(ctx, "rf_pair_scores", PairCall::Scores, npairs == 0 || out, npairs, seq, tpl, bw, flags))
        return e;
    const PairIo io{npairs, nullptr, seq, tpl, bw, fill_flags(flags), out, nullptr, nullptr, nullptr, nullptr, nullptr};
    return pair_run(ctx, io, false, false, nullptr);
}

// Alignments of independent pairs from a 4-bit move trace (k_pa / k_pa_gen,
// then k_pa_walk or k_pa_walk_w).  Like rf_pair_scores it reads the sequence
// and template arenas only.
int rf_pair_align(rf_ctx *ctx, int64_t npairs, const int32_t *seq, const int32_t *tpl, const int32_t *bw,
                  int32_t flags, double *out_score, int8_t *moves, const int64_t *moves_off, int32_t *nmoves,
                  int32_t *nerrors)
{
    if (int e = pair_check(ctx, "rf_pair_align", PairCall::Align, !moves == !moves_off, npairs, seq, tpl, bw, flags))
        return e;
    const PairIo io{npairs, nullptr, seq, tpl, bw, fill_flags(flags),
                    out_score, moves, moves_off, nmoves, nerrors, nullptr};
    return pair_run(ctx, io, true, moves || nmoves || nerrors, nullptr);
}

// rf_pair_align whose products are k_pa_fix's: single_indel_proposals
// (model.jl:538-562) and correct_shifts (model.jl:1303-1316) of each pair.
// The moves stay on the device.
int rf_pair_shifts(rf_ctx *ctx, int64_t npairs, const int32_t *seq, const int32_t *tpl, const int32_t *bw,
                   int32_t flags, double *out_score, uint8_t *fixed, const int64_t *fixed_off, int32_t *fixed_len,
                   int32_t *nprops, const int64_t *prop_off, uint8_t *prop_kind, int32_t *prop_pos,
                   uint8_t *prop_base, int32_t *tally)
{
    const int nrec = (prop_kind != nullptr) + (prop_pos != nullptr) + (prop_base != nullptr);
    bool outs_ok = (!fixed || fixed_off) && (nrec == 0 || (nrec == 3 && prop_off));
    for (int64_t k = 0; outs_ok && nrec == 3 && k < npairs; ++k)
        outs_ok = prop_off[k] >= 0 && prop_off[k + 1] >= prop_off[k];
    if (int e = pair_check(ctx, "rf_pair_shifts", PairCall::Align, outs_ok, npairs, seq, tpl, bw, flags))
        return e;
    const PairFix fx{fixed, fixed_off, fixed_len, nprops, prop_off, prop_kind, prop_pos, prop_base, tally};
    PairIo io{npairs, nullptr, seq, tpl, bw, fill_flags(flags), out_score, nullptr, nullptr, nullptr, nullptr, nullptr};
    io.fx = &fx;
    return pair_run(ctx, io, true, fx.any(), nullptr);
}

int rf_last_pair_shifts_ms(const rf_ctx *ctx, double *fix_ms)
{
    if (!ctx || !fix_ms)
        return RF_ERR_ARG;
    *fix_ms = ctx->pa_fix_ms;
    return 0;
}

int rf_host_shift_fix(int64_t npairs, const int8_t *moves, const int64_t *moves_off, const int32_t *nmoves,
                      const uint8_t *sbases, const int64_t *s_off, const uint8_t *tbases, const int64_t *t_off,
                      uint8_t *fixed, const int64_t *fixed_off, int32_t *fixed_len, int32_t *nprops,
                      const int64_t *prop_off, uint8_t *prop_kind, int32_t *prop_pos, uint8_t *prop_base,
                      int32_t *tally)
{
    return host_shift_fix(npairs, moves, moves_off, nmoves, sbases, s_off, tbases, t_off, fixed, fixed_off,
                          fixed_len, nprops, prop_off, prop_kind, prop_pos, prop_base, tally);
}

// smart_forward_moves! (model.jl:643-672) of independent pairs: rounds of
// pair_run over the pairs still pending, each at its current bandwidth;
// the loop's decisions are taken here from the downloaded counts.
// `fn` names the entry point (rf_pair_align_smart, rf_pair_align_text); `tx`
// (may be NULL) is rf_pair_align_text's outputs, which also lets threshold be
// NULL when max_doublings is 0: no pair then gets past its first fill.
// `errors`: rf_pair_errors, whose rounds take their counts from the fills
// (pair_run with io.errors) and which has rf_pair_align_text's threshold rule.
static int pair_smart_run(rf_ctx *ctx, const std::string &fn, bool outs_ok, int64_t npairs, const int32_t *seq,
                          const int32_t *tpl, const int32_t *bw, const double *threshold, const uint8_t *fixed,
                          int32_t max_doublings, int32_t flags, double *out_score, int8_t *moves,
                          const int64_t *moves_off, int32_t *nmoves, int32_t *nerrors, int32_t *out_bw,
                          int32_t *out_rounds, const PairText *tx, bool errors = false)
{
    if (int e = pair_check(ctx, fn, errors ? PairCall::Errors : PairCall::Align, outs_ok, npairs, seq, tpl, bw, flags))
        return e;
    if (npairs > 0 && !threshold && !((tx || errors) && max_doublings == 0))
        return fail(ctx, RF_ERR_ARG, fn + ": threshold is NULL");
    if (max_doublings < 0 || max_doublings > 5)
        return fail(ctx, RF_ERR_ARG, fn + ": max_doublings must be 0..5");
    std::vector<int32_t> cur((size_t)npairs), maxbw((size_t)npairs);
    for (int64_t k = 0; k < npairs; ++k) {
        const int64_t n = ctx->seqs[seq[k]].n, m = ctx->tpls[tpl[k]].m;
        // model.jl:648-651
        const int64_t mb = (fixed && fixed[k]) ? bw[k] : std::min({(int64_t)bw[k] << max_doublings, m, n});
        const int64_t H = 2 * mb + std::abs(n - m) + 1;
        const std::string why = pair_band_fault(ctx, fn, errors ? PairCall::Errors : PairCall::Align, H, m, k, mb);
        if (!why.empty())
            return fail(ctx, RF_ERR_ARG, why);
        cur[(size_t)k] = bw[k];
        maxbw[(size_t)k] = (int32_t)mb;
    }
    const bool want = moves || nmoves || nerrors || (tx && tx->any());
    // the loop reads every pair's score and error count, whatever the caller asked for
    std::vector<double> sc_own;
    std::vector<int32_t> ne_own;
    if (!out_score) {
        sc_own.resize((size_t)npairs);
        out_score = sc_own.data();
    }
    if (!nerrors) {
        ne_own.resize((size_t)npairs);
        nerrors = ne_own.data();
    }
    std::vector<int32_t> n_err((size_t)npairs, INT32_MAX), old_err((size_t)npairs, INT32_MAX);
    std::vector<int64_t> pending((size_t)npairs), next;
    std::vector<uint8_t> more((size_t)npairs, 0);
    for (int64_t k = 0; k < npairs; ++k)
        pending[(size_t)k] = k;
    if (out_rounds)
        std::fill(out_rounds, out_rounds + npairs, 0);
    auto stops_at_fill = [&](int64_t k) { return (fixed && fixed[k]) || cur[(size_t)k] >= maxbw[(size_t)k]; };
    auto ended = [&](int64_t k, double score, int32_t, int32_t ne) {
        more[(size_t)k] = 0;
        if (score != score || stops_at_fill(k))   // the reference raised / model.jl:656-658
            return true;
        old_err[(size_t)k] = n_err[(size_t)k];
        n_err[(size_t)k] = ne;
        // a walk that failed (-1) ends the pair like the error it would be
        more[(size_t)k] = ne >= 0 && (double)ne > threshold[k] && ne < old_err[(size_t)k];
        return !more[(size_t)k];
    };
    while (!pending.empty()) {
        bool walk = want;
        for (int64_t k : pending)
            walk = walk || !stops_at_fill(k);
        const PairIo io{(int64_t)pending.size(), pending.data(), seq, tpl, cur.data(), fill_flags(flags), out_score,
                        moves, moves_off, nmoves, nerrors, tx, errors};
        if (int e = pair_run(ctx, io, true, walk, ended))
            return e;
        next.clear();
        for (int64_t k : pending) {
            if (out_rounds)
                ++out_rounds[k];
            if (!walk)
                continue;   // every pair of the round stopped at its fill
            if (more[(size_t)k]) {
                cur[(size_t)k] = (int32_t)std::min<int64_t>(2 * (int64_t)cur[(size_t)k], maxbw[(size_t)k]);
                next.push_back(k);
            }
        }
        pending.swap(next);
    }
    if (out_bw)
        std::copy(cur.begin(), cur.end(), out_bw);
    return 0;
}

int rf_pair_align_smart(rf_ctx *ctx, int64_t npairs, const int32_t *seq, const int32_t *tpl, const int32_t *bw,
                        const double *threshold, const uint8_t *fixed, int32_t max_doublings, int32_t flags,
                        double *out_score, int8_t *moves, const int64_t *moves_off, int32_t *nmoves,
                        int32_t *nerrors, int32_t *out_bw, int32_t *out_rounds)
{
    return pair_smart_run(ctx, "rf_pair_align_smart", !moves == !moves_off, npairs, seq, tpl, bw, threshold, fixed,
                          max_doublings, flags, out_score, moves, moves_off, nmoves, nerrors, out_bw, out_rounds,
                          nullptr);
}

// rf_pair_align_smart whose products are k_pa_emit's: align (align.jl:346-353,
// moves_to_aligned_seqs :286-311), moves_to_indices (:322-335) and
// band_tolerance (:262-284) of each pair's last fill.  The moves stay on the
// device.
int rf_pair_align_text(rf_ctx *ctx, int64_t npairs, const int32_t *seq, const int32_t *tpl, const int32_t *bw,
                       const double *threshold, const uint8_t *fixed, int32_t max_doublings, int32_t flags,
                       double *out_score, uint8_t *aln_t, uint8_t *aln_s, const int64_t *aln_off, int32_t *aln_len,
                       int32_t *t2s, const int64_t *t2s_off, int32_t *t2s_len, int32_t *tolerance,
                       int32_t *nerrors, int32_t *out_bw, int32_t *out_rounds)
{
    const bool outs_ok = (!aln_t == !aln_s) && (!aln_t || aln_off) && (!t2s || t2s_off);
    const PairText tx{aln_t, aln_s, aln_off, aln_len, t2s, t2s_off, t2s_len, tolerance};
    return pair_smart_run(ctx, "rf_pair_align_text", outs_ok, npairs, seq, tpl, bw, threshold, fixed, max_doublings,
                          flags, out_score, nullptr, nullptr, nullptr, nerrors, out_bw, out_rounds, &tx);
}

// rf_pair_align_smart without moves, the error count carried through the
// fill beside the score (k_pe / k_pe_gen): no trace, no walk.  Pairs whose
// band is wider than DP_COUNT_H take rf_pair_align_smart's path inside the
// same rounds.
int rf_pair_errors(rf_ctx *ctx, int64_t npairs, const int32_t *seq, const int32_t *tpl, const int32_t *bw,
                   const double *threshold, const uint8_t *fixed, int32_t max_doublings, int32_t flags,
                   double *out_score, int32_t *nerrors, int32_t *out_bw, int32_t *out_rounds)
{
    return pair_smart_run(ctx, "rf_pair_errors", true, npairs, seq, tpl, bw, threshold, fixed, max_doublings, flags,
                          out_score, nullptr, nullptr, nullptr, nerrors, out_bw, out_rounds, nullptr, true);
}

int rf_last_pair_errors_ms(const rf_ctx *ctx, double *fill_ms)
{
    if (!ctx || !fill_ms)
        return RF_ERR_ARG;
    *fill_ms = ctx->pe_ms;
    return 0;
}

int rf_last_pair_text_ms(const rf_ctx *ctx, double *emit_ms)
{
    if (!ctx || !emit_ms)
        return RF_ERR_ARG;
    *emit_ms = ctx->pa_emit_ms;
    return 0;
}

int rf_last_pair_align_ms(const rf_ctx *ctx, double *fill_ms, double *walk_ms)
{
    if (!ctx)
        return RF_ERR_ARG;
    if (fill_ms)
        *fill_ms = ctx->pa_fill_ms;
    if (walk_ms)
        *walk_ms = ctx->pa_walk_ms;
    return 0;
}

// Launch the backtraces of `tasks` (moves into BUF_MOVES_OR_CTASKS at t.out,
// counts in BUF_COUNTS_OR_PROPS) in k_bt_win (round 4: codon alignments and bands of any height
// too); with d_mask, the walks also mark alignment proposals.
static int launch_backtraces(rf_ctx *ctx, std::vector<BTTask> &tasks, uint8_t *d_mask, int do_indels)
{
    const int32_t nslots = (int32_t)tasks.size();
    std::vector<BTTask> &win = ctx->bt_win;   // alive until the caller's sync
    win = tasks;
    int32_t *d_cnt = dev<int32_t>(ctx, BUF_COUNTS_OR_PROPS);
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_WALKS_BEGIN], ctx->stream));
    if (!win.empty()) {
        if (int e = upload(ctx, ctx->scratch[BUF_BT_TASKS], win))
            return e;
        // a launch of few walks (the reference's, edit_distance's: one
        // latency-bound walk each) runs each walk on 4 waves (NW = 4)
        const bool few = win.size() <= (size_t)BTW_FEW && ctx->opt.bt_nw != 1;
        auto kern = few ? k_bt_win<4096, 4> : ctx->opt.bt_win_kb == 16 ? k_bt_win<2048> : k_bt_win<4096>;
        hipLaunchKernelGGL(kern, dim3((unsigned)win.size()), dim3(few ? 256 : 64), 0, ctx->stream,
                           dev<const BTTask>(ctx, BUF_BT_TASKS), (const uint8_t *)ctx->bytes_arena.d,
                           (const double *)ctx->tab_arena.d, (const double *)ctx->band_arena.d,
                           dev<int8_t>(ctx, BUF_MOVES_OR_CTASKS), d_cnt, d_cnt + nslots, ctx->d_err, d_mask, do_indels);
    }
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_WALKS_END], ctx->stream));
    return 0;
}

// kernel time of the last launch_backtraces (after the caller's sync)
static void note_bt_ms(rf_ctx *ctx)
{
    float ms = 0;
    if (hipEventElapsedTime(&ms, ctx->ev[EV_WALKS_BEGIN], ctx->ev[EV_WALKS_END]) == hipSuccess)
        ctx->bt_ms = ms;
}

// Backtrace descriptors of `nslots` slots (moves slot k at offs[k], n+m bytes)
// and the scratch buffers for moves and counts, for the call `fn`.
static int build_bt_tasks(rf_ctx *ctx, const char *fn, int32_t nslots, const int32_t *slot,
                          std::vector<BTTask> &tasks, std::vector<int64_t> &offs)
{
    tasks.assign(nslots, BTTask{});
    offs.assign(nslots, 0);
    int64_t total = 0;
    for (int32_t k = 0; k < nslots; ++k) {
        if (const char *why = a_band_fault(ctx, slot[k]))
            return fail(ctx, RF_ERR_STATE, std::string(fn) + ": " + why);
        const Band &b = ctx->slots[slot[k]].a;
        BTTask &t = tasks[k] = slot_desc<BTTask>(ctx, slot[k]);
        t.out = total;
        t.flags = fill_flags(b.flags);
        t.idx = k;
        offs[k] = total;
        total += b.n + b.m;
    }
    if (int e = ensure_buf(ctx, ctx->scratch[BUF_MOVES_OR_CTASKS], std::max<int64_t>(total, 16)))
        return e;
    if (int e = ensure_buf(ctx, ctx->scratch[BUF_COUNTS_OR_PROPS], sizeof(int32_t) * 2 * std::max(nslots, 1)))
        return e;
    return 0;
}

int rf_backtrace(rf_ctx *ctx, int32_t nslots, const int32_t *slot, int8_t *moves,
                 const int64_t *moves_off, int32_t *nmoves, int32_t *nerrors)
{
    if (!ctx || nslots < 0 || (nslots > 0 && !slot) || (moves && !moves_off))
        return fail(ctx, RF_ERR_ARG, "rf_backtrace: bad arguments");
    (void)hipSetDevice(ctx->device);
    std::vector<BTTask> tasks;
    std::vector<int64_t> offs;
    if (int e = build_bt_tasks(ctx, "rf_backtrace", nslots, slot, tasks, offs))
        return e;
    const int64_t total = nslots > 0 ? offs[nslots - 1] + tasks[nslots - 1].n + tasks[nslots - 1].m : 0;
    int32_t *d_cnt = dev<int32_t>(ctx, BUF_COUNTS_OR_PROPS);
    if (nslots > 0)
        if (int e = launch_backtraces(ctx, tasks, nullptr, 0))
            return e;
    // the counts at 0, then the moves at cb, land with the error flag: one wait
    const size_t cb = (sizeof(int32_t) * 2 * (size_t)nslots + 15) & ~(size_t)15;
    if (int e = ensure_landing(ctx, cb + (moves ? (size_t)total : 0)))
        return e;
    HIPCHK(ctx, pre_d2h(ctx));
    if (nslots > 0)
        HIPCHK(ctx, land(ctx, 0, d_cnt, sizeof(int32_t) * 2 * nslots));
    if (moves && total > 0)
        HIPCHK(ctx, land(ctx, cb, ctx->scratch[BUF_MOVES_OR_CTASKS].p, total));
    HIPCHK(ctx, land_wait(ctx));
    if (nslots > 0)
        note_bt_ms(ctx);
    if (int e = check_landed(ctx))
        return e;
    const int32_t *cnt = landed<int32_t>(ctx);
    const int8_t *all = landed<int8_t>(ctx, cb);
    for (int32_t k = 0; k < nslots; ++k) {
        if (nmoves)
            nmoves[k] = cnt[k];
        if (nerrors)
            nerrors[k] = cnt[nslots + k];
        if (moves)   // the walk leaves the moves at the end of the read's n+m slot
            std::memcpy(moves + moves_off[k], all + offs[k] + tasks[k].n + tasks[k].m - cnt[k], cnt[k]);
    }
    return 0;
}

int rf_alignment_proposals(rf_ctx *ctx, int32_t ngroups, const int32_t *slot_off, const int32_t *slots,
                           int32_t do_indels, uint8_t *out_mask)
{
    if (!ctx || ngroups < 0 || (ngroups > 0 && (!slot_off || !slots || !out_mask)))
        return fail(ctx, RF_ERR_ARG, "rf_alignment_proposals: bad arguments");
    const int32_t nslots = ngroups > 0 ? slot_off[ngroups] : 0;
    (void)hipSetDevice(ctx->device);
    // 1. descriptors: backtrace tasks of every batch slot + each cluster's mask
    std::vector<BTTask> tasks;
    std::vector<int64_t> offs;
    if (int e = build_bt_tasks(ctx, "rf_alignment_proposals", nslots, slots, tasks, offs))
        return e;
    int64_t mask_total = 0;
    for (int32_t g = 0; g < ngroups; ++g) {
        int32_t tpl = -1, m = 0;
        for (int32_t k = slot_off[g]; k < slot_off[g + 1]; ++k) {
            const Band &b = ctx->slots[slots[k]].a;
            if (tpl >= 0 && b.tpl != tpl)
                return fail(ctx, RF_ERR_ARG, "rf_alignment_proposals: batch slots use different templates");
            tpl = b.tpl;
            m = b.m;
            tasks[k].mask = mask_total;
        }
        if (slot_off[g + 1] > slot_off[g])
            mask_total += (int64_t)(m + 1) * 9;
    }
    if (nslots == 0)
        return 0;
    if (int e = ensure_buf(ctx, ctx->scratch[BUF_READS_OR_MASK], std::max<int64_t>(mask_total, 16)))
        return e;
    HIPCHK(ctx, hipMemsetAsync(ctx->scratch[BUF_READS_OR_MASK].p, 0, mask_total, ctx->stream));
    // 2. the walks mark the mask as they go
    if (int e = launch_backtraces(ctx, tasks, dev<uint8_t>(ctx, BUF_READS_OR_MASK), do_indels ? 1 : 0))
        return e;
    HIPCHK(ctx, hipGetLastError());
    if (int e = ensure_landing(ctx, mask_total))
        return e;
    HIPCHK(ctx, pre_d2h(ctx));
    HIPCHK(ctx, land(ctx, 0, ctx->scratch[BUF_READS_OR_MASK].p, mask_total));
    HIPCHK(ctx, land_wait(ctx));
    note_bt_ms(ctx);
    if (int e = check_landed(ctx))
        return e;
    std::memcpy(out_mask, landed<uint8_t>(ctx), mask_total);
    return 0;
}

int rf_score(rf_ctx *ctx, int32_t ngroups, const int32_t *slot_off, const int32_t *slots,
             const int32_t *ref_slot, const int64_t *prop_off, const uint8_t *kind,
             const int32_t *pos, const uint8_t *base, double *out_total, double *out_per_seq)
{
    if (!ctx || ngroups < 0 || (ngroups > 0 && (!slot_off || !prop_off)))
        return fail(ctx, RF_ERR_ARG, "rf_score: bad arguments");
    (void)hipSetDevice(ctx->device);
    const int64_t nprops = ngroups > 0 ? prop_off[ngroups] - prop_off[0] : 0;
    if (nprops > 0 && (!kind || !pos || !base || !out_total))
        return fail(ctx, RF_ERR_ARG, "rf_score: bad proposal arrays");

    // 1. the slots, group by group in slot order: batch slots, then the reference
    std::vector<ScoreReadIn> in;
    std::vector<ScoreGroupIn> gin(ngroups);
    std::vector<int32_t> has_reads(ngroups, 0), has_ref(ngroups, 0);
    in.reserve(ngroups > 0 ? std::max(slot_off[ngroups], 0) : 0);
    for (int32_t g = 0; g < ngroups; ++g) {
        int32_t tpl = -1;
        const int32_t r0 = (int32_t)in.size();
        if (int e = score_group_slots(ctx, "rf_score", RF_ERR_STATE, slots, slot_off[g], slot_off[g + 1], tpl, &in))
            return e;
        if (ref_slot && ref_slot[g] >= 0) {
            if (const char *why = score_band_fault(ctx, ref_slot[g]))
                return fail(ctx, RF_ERR_STATE, std::string("rf_score (reference): ") + why);
            const int32_t rt = ctx->slots[ref_slot[g]].a.tpl;
            if (tpl >= 0 && rt != tpl)
                return fail(ctx, RF_ERR_ARG, "rf_score: reference uses a different template");
            tpl = rt;
            has_ref[g] = 1;
        }
        has_reads[g] = (int32_t)in.size() > r0;
        gin[g] = {r0, (int32_t)in.size(), tpl < 0 ? 0 : ctx->tpls[tpl].m, tpl < 0 ? 0 : ctx->tpls[tpl].bases.off};
    }
    // 2. the layout and the scorer; its vectors source the uploads below
    ScorePlan P;
    score_plan(in, gin, ctx->opt, true, P);
    const std::vector<ScoreGroup> &groups = P.groups;
    const std::vector<WorkItem> &items = P.items;
    const int64_t dense_total = P.dense_total, split_total = P.split_total;
    // rf_score counts 64-column items whichever scorer runs
    const bool split = score_split(P.items64, P.max_reads, ctx->opt.score_mode, out_per_seq != nullptr);
    // 3. the proposals; codon tasks for those of a group with a reference
    std::vector<CodonTask> ctasks;
    std::vector<int32_t> pgroup(nprops);
    int64_t scratch_total = 0;
    for (int32_t g = 0; g < ngroups; ++g)
        for (int64_t k = prop_off[g]; k < prop_off[g + 1]; ++k) {
            const int kd = kind[k], ps = pos[k], b = base[k], m = groups[g].m;
            if (kd > 2 || b > 3 || (kd == 1 ? (ps < 0 || ps > m) : (ps < 1 || ps > m)))
                return fail(ctx, RF_ERR_ARG, "rf_score: proposal out of range");
            if (!has_reads[g] && !has_ref[g])
                return fail(ctx, RF_ERR_ARG, "rf_score: group has neither reads nor reference");
            pgroup[k - prop_off[0]] = g;
            if (has_ref[g]) {
                CodonTask t = slot_desc<CodonTask>(ctx, ref_slot[g]);
                t.scratch = scratch_total;
                scratch_total += 4 * (int64_t)(t.n + 1);
                t.kind = kd;
                t.pos = ps;
                t.base = b;
                t.out_idx = (int32_t)(k - prop_off[0]);
                ctasks.push_back(t);
            }
        }

    // uploads
    if (int e = upload(ctx, ctx->scratch[BUF_SCORE_ITEMS], items)) return e;
    if (int e = upload(ctx, ctx->scratch[BUF_SCORE_GROUPS], groups)) return e;
    if (int e = upload(ctx, ctx->scratch[BUF_READS_OR_MASK], P.reads)) return e;
    if (int e = upload(ctx, ctx->scratch[BUF_MOVES_OR_CTASKS], ctasks)) return e;
    // proposal arrays + per-group flags + gstart
    const size_t pbytes = align_up(nprops * 4, 256) * 2 + align_up(nprops, 256) * 2 +
                          align_up(ngroups * 4, 256) * 2 + align_up((ngroups + 1) * 8, 256);
    if (int e = ensure_buf(ctx, ctx->scratch[BUF_COUNTS_OR_PROPS], pbytes + 256)) return e;
    char *pb = dev<char>(ctx, BUF_COUNTS_OR_PROPS);
    int32_t *d_pgroup = (int32_t *)pb;  pb += align_up(nprops * 4, 256);
    int32_t *d_pos = (int32_t *)pb;     pb += align_up(nprops * 4, 256);
    uint8_t *d_kind = (uint8_t *)pb;    pb += align_up(nprops, 256);
    uint8_t *d_base = (uint8_t *)pb;    pb += align_up(nprops, 256);
    int32_t *d_hr = (int32_t *)pb;      pb += align_up(ngroups * 4, 256);
    int32_t *d_href = (int32_t *)pb;    pb += align_up(ngroups * 4, 256);
    int64_t *d_gstart = (int64_t *)pb;
    // the seven arrays in their device layout: one copy out of the ring
    const size_t pused = (size_t)((char *)(d_gstart + ngroups + 1) - dev<char>(ctx, BUF_COUNTS_OR_PROPS));
    char *h;
    if (int e = ring_take(ctx, pused, &h))
        return e;
    auto put = [&](void *d, const void *src, size_t n) -> hipError_t {
        if (!n)
            return hipSuccess;
        if (h) {
            std::memcpy(h + ((char *)d - dev<char>(ctx, BUF_COUNTS_OR_PROPS)), src, n);
            return hipSuccess;
        }
        return hipMemcpyAsync(d, src, n, hipMemcpyHostToDevice, ctx->stream);
    };
    if (nprops > 0) {
        HIPCHK(ctx, put(d_pgroup, pgroup.data(), nprops * 4));
        HIPCHK(ctx, put(d_pos, pos + prop_off[0], nprops * 4));
        HIPCHK(ctx, put(d_kind, kind + prop_off[0], nprops));
        HIPCHK(ctx, put(d_base, base + prop_off[0], nprops));
    }
    if (ngroups > 0) {
        HIPCHK(ctx, put(d_hr, has_reads.data(), ngroups * 4));
        HIPCHK(ctx, put(d_href, has_ref.data(), ngroups * 4));
        HIPCHK(ctx, put(d_gstart, P.gstart.data(), (ngroups + 1) * 8));
    }
    if (h && (nprops > 0 || ngroups > 0))
        HIPCHK(ctx, hipMemcpyAsync(ctx->scratch[BUF_COUNTS_OR_PROPS].p, h, pused, hipMemcpyHostToDevice, ctx->stream));
    // work buffers: dense totals, split partials, codon scratch + outputs, final totals
    const size_t wbytes = align_up(std::max<int64_t>(dense_total, 1) * 8, 256) +
                          (split ? align_up(std::max<int64_t>(split_total, 1) * 8, 256) : 0) +
                          align_up(std::max<int64_t>(scratch_total, 1) * 8, 256) +
                          2 * align_up(std::max<int64_t>(nprops, 1) * 8, 256);
    if (int e = ensure_buf(ctx, ctx->scratch[BUF_SEGS_OR_WORK], wbytes)) return e;
    char *wb = dev<char>(ctx, BUF_SEGS_OR_WORK);
    double *d_dense = (double *)wb;   wb += align_up(std::max<int64_t>(dense_total, 1) * 8, 256);
    double *d_split = nullptr;
    if (split) { d_split = (double *)wb; wb += align_up(std::max<int64_t>(split_total, 1) * 8, 256); }
    double *d_cscr = (double *)wb;    wb += align_up(std::max<int64_t>(scratch_total, 1) * 8, 256);
    double *d_ref = (double *)wb;     wb += align_up(std::max<int64_t>(nprops, 1) * 8, 256);
    double *d_out = (double *)wb;

    const uint8_t *d_bases = (const uint8_t *)ctx->bytes_arena.d;
    const double *d_tabs = (const double *)ctx->tab_arena.d;
    const double *d_bands = (const double *)ctx->band_arena.d;

    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_SCORER_BEGIN], ctx->stream));
    unsigned gy = 0;
    if (!items.empty()) {
        gy = launch_scorer(ctx, P.pick, (unsigned)items.size(), split ? (unsigned)P.max_reads : 1u,
                           dev<const WorkItem>(ctx, BUF_SCORE_ITEMS), dev<const ScoreGroup>(ctx, BUF_SCORE_GROUPS),
                           dev<const ScoreRead>(ctx, BUF_READS_OR_MASK), d_dense, d_split);
        if (split && dense_total > 0)
            hipLaunchKernelGGL(k_reduce<false>, dim3((unsigned)((dense_total + 255) / 256)), dim3(256), 0,
                               ctx->stream, dev<const ScoreGroup>(ctx, BUF_SCORE_GROUPS), ngroups, d_gstart,
                               dense_total, d_split, d_dense);
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_CODON_BEGIN], ctx->stream));
    if (!ctasks.empty())
        hipLaunchKernelGGL(k_codon, dim3((unsigned)((ctasks.size() + 63) / 64)), dim3(64), 0,
                           ctx->stream, dev<const CodonTask>(ctx, BUF_MOVES_OR_CTASKS), (int)ctasks.size(),
                           d_bases, d_tabs, d_bands, d_cscr, d_ref);
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_SCORER_END], ctx->stream));
    if (nprops > 0)
        hipLaunchKernelGGL(k_gather, dim3((unsigned)((nprops + 255) / 256)), dim3(256), 0, ctx->stream,
                           nprops, d_pgroup, d_kind, d_pos, d_base, dev<const ScoreGroup>(ctx, BUF_SCORE_GROUPS),
                           d_hr, d_dense, d_ref, d_href, d_out, ctx->d_err);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_GATHER_END], ctx->stream));
    // the totals land with the error flag (per-read columns, a test /
    // sharding path, stay pageable and follow the flag)
    if (int e = ensure_landing(ctx, (size_t)std::max<int64_t>(nprops, 0) * 8))
        return e;
    HIPCHK(ctx, pre_d2h(ctx));
    if (nprops > 0)
        HIPCHK(ctx, land(ctx, 0, d_out, nprops * 8));
    HIPCHK(ctx, land_flag(ctx));
    std::vector<double> split_host;
    if (out_per_seq && split_total > 0) {
        split_host.resize(split_total);
        HIPCHK(ctx, hipMemcpyAsync(split_host.data(), d_split, split_total * 8, hipMemcpyDeviceToHost,
                                   ctx->stream));
    }
    std::vector<double> ref_host;
    if (out_per_seq && !ctasks.empty()) {
        ref_host.resize(nprops);
        HIPCHK(ctx, hipMemcpyAsync(ref_host.data(), d_ref, nprops * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(ctx, stream_wait(ctx));
    ctx->score_ms = mark_ms(ctx, EV_SCORER_BEGIN, EV_SCORER_END);
    ctx->gather_ms = mark_ms(ctx, EV_SCORER_END, EV_GATHER_END);
    const double cms = mark_ms(ctx, EV_CODON_BEGIN, EV_SCORER_END);
    ctx->codon_ms = ctasks.empty() ? 0.0 : cms;
    if (out_per_seq) {
        // [k][r] rows, r = batch position (+1 column for the reference, if any)
        int64_t row = 0;
        for (int32_t g = 0; g < ngroups; ++g) {
            const ScoreGroup &G = groups[g];
            const int R = G.r1 - G.r0;
            const int width = R + (has_ref[g] ? 1 : 0);
            for (int64_t k = prop_off[g]; k < prop_off[g + 1]; ++k) {
                const int kd = kind[k];
                const int sl = kd == 0 ? base[k] : (kd == 2 ? 4 : 5 + base[k]);
                for (int r = 0; r < R; ++r)
                    out_per_seq[row + r] =
                        split_host[G.split_off + ((int64_t)r * (G.m + 1) + pos[k]) * 9 + sl];
                if (has_ref[g])
                    out_per_seq[row + R] = ref_host[k - prop_off[0]];
                row += width;
            }
        }
    }
    if (int e = check_landed(ctx))
        return e;
    if (nprops > 0)
        std::memcpy(out_total, landed<double>(ctx), nprops * 8);
    note_score_launch(ctx, P.pick, split, items.size(), gy);
    return 0;
}

// init (rf_score_dense_from; NULL: the fold starts at 0.0): the table the
// fold continues, in the call's row layout, host or device memory by
// init_kind.  It is copied into BUF_DENSE_TOTALS once every check has passed,
// and the scorers then read and write that one resident table in place.
static int score_dense_impl(rf_ctx *ctx, int32_t ngroups, const int32_t *slot_off, const int32_t *slots,
                            double *out, hipMemcpyKind out_kind, const double *init = nullptr,
                            hipMemcpyKind init_kind = hipMemcpyHostToDevice)
{
    if (!ctx || ngroups < 0 || (ngroups > 0 && (!slot_off || !slots)))
        return fail(ctx, RF_ERR_ARG, "rf_score_dense: bad arguments");
    (void)hipSetDevice(ctx->device);
    const int32_t nslots = ngroups > 0 ? slot_off[ngroups] : 0;
    auto &C = ctx->dplan;
    ScorePlan &P = C.plan;
    const bool same = C.valid && C.gen == ctx->layout_gen && C.ngroups == ngroups && C.opt_gen == ctx->opt_gen &&
                      C.slots.size() == (size_t)nslots &&
                      !std::memcmp(C.slot_off.data(), slot_off, sizeof(int32_t) * (ngroups + 1)) &&
                      (nslots == 0 || !std::memcmp(C.slots.data(), slots, sizeof(int32_t) * nslots));
    // per-call validation of the bands, unless this very slot list was
    // validated and nothing (sequences, templates, bands) changed since; a
    // new slot list is planned from the records of the same pass
    if (!(same && C.val_epoch == ctx->state_epoch)) {
        std::vector<ScoreReadIn> in;
        std::vector<ScoreGroupIn> gin;
        in.reserve(same ? 0 : std::max(nslots, 0));
        gin.reserve(ngroups);
        for (int32_t g = 0; g < ngroups; ++g) {
            int32_t tpl = -1;
            const int32_t r0 = (int32_t)in.size();
            if (int e = score_group_slots(ctx, "rf_score_dense", RF_ERR_ARG, slots, slot_off[g], slot_off[g + 1], tpl,
                                          same ? nullptr : &in))
                return e;
            gin.push_back({r0, (int32_t)in.size(), tpl < 0 ? 0 : ctx->tpls[tpl].m, tpl < 0 ? 0 : ctx->tpls[tpl].bases.off});
            if (tpl < 0)   // no slots: score_plan refuses the group, the later ones stay unread
                break;
        }
        if (!same) {
            C.valid = false;
            if (score_plan(in, gin, ctx->opt, false, P))
                return fail(ctx, RF_ERR_ARG, "rf_score_dense: empty group");
            if (int e = upload(ctx, ctx->scratch[BUF_DENSE_ITEMS], P.items)) return e;
            if (int e = upload(ctx, ctx->scratch[BUF_DENSE_GROUPS], P.groups)) return e;
            if (int e = upload(ctx, ctx->scratch[BUF_DENSE_READS], P.reads)) return e;
            if (int e = upload(ctx, ctx->scratch[BUF_DENSE_GSTART], P.gstart)) return e;
            C.valid = true;
            C.gen = ctx->layout_gen;
            C.ngroups = ngroups;
            C.slot_off.assign(slot_off, slot_off + ngroups + 1);
            C.slots.assign(slots, slots + nslots);
            C.opt_gen = ctx->opt_gen;
        }
        C.val_epoch = ctx->state_epoch;
    }
    const size_t nitems = P.items.size();
    const bool split = score_split((int64_t)nitems, P.max_reads, ctx->opt.score_mode, false);
    if (int e = ensure_buf(ctx, ctx->scratch[BUF_DENSE_TOTALS], sizeof(double) * std::max<int64_t>(P.dense_total, 1)))
        return e;
    if (split)
        if (int e = ensure_buf(ctx, ctx->scratch[BUF_RING_OR_SPLIT],
                               sizeof(double) * std::max<int64_t>(P.split_total, 1)))
            return e;
    double *d_dense = dev<double>(ctx, BUF_DENSE_TOTALS);
    const bool from = init != nullptr && P.dense_total > 0;
    if (from)
        HIPCHK(ctx, hipMemcpyAsync(d_dense, init, sizeof(double) * P.dense_total, init_kind, ctx->stream));
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_SCORER_BEGIN], ctx->stream));
    unsigned gy = 0;
    if (nitems) {
        gy = launch_scorer(ctx, P.pick, (unsigned)nitems, split ? (unsigned)P.max_reads : 1u,
                           dev<const WorkItem>(ctx, BUF_DENSE_ITEMS), dev<const ScoreGroup>(ctx, BUF_DENSE_GROUPS),
                           dev<const ScoreRead>(ctx, BUF_DENSE_READS), d_dense,
                           split ? dev<double>(ctx, BUF_RING_OR_SPLIT) : nullptr, from);
        if (split && from)
            hipLaunchKernelGGL(k_reduce<true>, dim3((unsigned)((P.dense_total + 255) / 256)), dim3(256), 0,
                               ctx->stream, dev<const ScoreGroup>(ctx, BUF_DENSE_GROUPS), ngroups,
                               dev<const int64_t>(ctx, BUF_DENSE_GSTART), P.dense_total,
                               dev<const double>(ctx, BUF_RING_OR_SPLIT), d_dense);
        else if (split)
            hipLaunchKernelGGL(k_reduce<false>, dim3((unsigned)((P.dense_total + 255) / 256)), dim3(256), 0,
                               ctx->stream, dev<const ScoreGroup>(ctx, BUF_DENSE_GROUPS), ngroups,
                               dev<const int64_t>(ctx, BUF_DENSE_GSTART), P.dense_total,
                               dev<const double>(ctx, BUF_RING_OR_SPLIT), d_dense);
    }
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_SCORER_END], ctx->stream));
    if (out && P.dense_total > 0) {
        HIPCHK(ctx, pre_d2h(ctx));
        HIPCHK(ctx, hipMemcpyAsync(out, d_dense, sizeof(double) * P.dense_total, out_kind, ctx->stream));
    }
    HIPCHK(ctx, stream_wait(ctx));
    ctx->score_ms = mark_ms(ctx, EV_SCORER_BEGIN, EV_SCORER_END);
    ctx->gather_ms = 0;
    note_score_launch(ctx, P.pick, split, nitems, gy);
    return 0;
}

int rf_score_dense(rf_ctx *ctx, int32_t ngroups, const int32_t *slot_off, const int32_t *slots,
                   double *out)
{
    return score_dense_impl(ctx, ngroups, slot_off, slots, out, hipMemcpyDeviceToHost);
}

int rf_score_dense_dev(rf_ctx *ctx, int32_t ngroups, const int32_t *slot_off, const int32_t *slots,
                       double *dev_out)
{
    if (!dev_out)
        return fail(ctx, RF_ERR_ARG, "rf_score_dense_dev: null device buffer");
    return score_dense_impl(ctx, ngroups, slot_off, slots, dev_out, hipMemcpyDeviceToDevice);
}

// rf_score_dense_ref and the rf_score_dense_from calls: the reads' fold (from
// init when given), then the reference term of the groups that have one.
// ref_slot may be NULL here (no reference term).
static int score_dense_ref_impl(rf_ctx *ctx, int32_t ngroups, const int32_t *slot_off, const int32_t *slots,
                                const int32_t *ref_slot, const double *init, hipMemcpyKind init_kind, double *out,
                                hipMemcpyKind out_kind)
{
    if (!ctx || ngroups < 0 || (ngroups > 0 && (!slot_off || !slots)))
        return fail(ctx, RF_ERR_ARG, "rf_score_dense: bad arguments");
    // the reference slots, before anything runs
    bool any_ref = false;
    for (int32_t g = 0; ref_slot && g < ngroups; ++g) {
        const int32_t rs = ref_slot[g];
        if (rs < 0)
            continue;
        any_ref = true;
        if (rs >= (int32_t)ctx->slots.size())
            return fail(ctx, RF_ERR_ARG, "rf_score_dense_ref: unknown reference slot");
        if (const char *why = score_band_fault(ctx, rs))
            return fail(ctx, RF_ERR_STATE, std::string("rf_score_dense_ref (reference): ") + why);
        // the group's template is its first batch slot's (a bad batch slot is
        // refused by the reads' fold below)
        if (slot_off[g + 1] > slot_off[g]) {
            const int32_t s0 = slots[slot_off[g]];
            if (s0 >= 0 && s0 < (int32_t)ctx->slots.size() && ctx->slots[s0].a.valid &&
                ctx->slots[s0].a.tpl != ctx->slots[rs].a.tpl)
                return fail(ctx, RF_ERR_ARG, "rf_score_dense_ref: reference uses a different template");
        }
    }
    // the reads' fold: totals in BUF_DENSE_TOTALS
    if (int e = score_dense_impl(ctx, ngroups, slot_off, slots, nullptr, hipMemcpyDeviceToHost, init, init_kind))
        return e;
    const ScorePlan &P = ctx->dplan.plan;
    ctx->codon_dense_ms = 0;
    double *d_dense = dev<double>(ctx, BUF_DENSE_TOTALS);
    if (any_ref) {
        std::vector<CodonDenseGroup> cg;
        int64_t nblk = 0;
        for (int32_t g = 0; g < ngroups; ++g) {
            if (ref_slot[g] < 0)
                continue;
            CodonDenseGroup G = slot_desc<CodonDenseGroup>(ctx, ref_slot[g]);
            G.dense_off = P.groups[g].dense_off;
            G.blk0 = (int32_t)nblk;
            nblk += (9 * ((int64_t)G.m + 1) + 63) / 64;
            cg.push_back(G);
        }
        if (nblk > INT32_MAX)
            return fail(ctx, RF_ERR_ARG, "rf_score_dense_ref: too many slots for one launch");
        if (int e = upload(ctx, ctx->scratch[BUF_CODON_GROUPS], cg)) return e;
        HIPCHK(ctx, hipEventRecord(ctx->ev[EV_CODON_DENSE_BEGIN], ctx->stream));
        hipLaunchKernelGGL(k_codon_dense, dim3((unsigned)nblk), dim3(64), 0, ctx->stream,
                           dev<const CodonDenseGroup>(ctx, BUF_CODON_GROUPS), (int)cg.size(),
                           (const uint8_t *)ctx->bytes_arena.d, (const double *)ctx->tab_arena.d,
                           (const double *)ctx->band_arena.d, d_dense);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipEventRecord(ctx->ev[EV_CODON_DENSE_END], ctx->stream));
        // cg sources the upload when it does not fit the pinned ring
        HIPCHK(ctx, stream_wait(ctx));
        ctx->codon_dense_ms = mark_ms(ctx, EV_CODON_DENSE_BEGIN, EV_CODON_DENSE_END);
        ctx->score_ms += ctx->codon_dense_ms;
    }
    if (out && P.dense_total > 0) {
        HIPCHK(ctx, hipMemcpyAsync(out, d_dense, sizeof(double) * P.dense_total, out_kind, ctx->stream));
        HIPCHK(ctx, stream_wait(ctx));
    }
    return 0;
}

int rf_score_dense_ref(rf_ctx *ctx, int32_t ngroups, const int32_t *slot_off, const int32_t *slots,
                       const int32_t *ref_slot, double *out)
{
    if (ctx && !ref_slot && !(ngroups < 0 || (ngroups > 0 && (!slot_off || !slots))))
        return fail(ctx, RF_ERR_ARG, "rf_score_dense_ref: null ref_slot");
    return score_dense_ref_impl(ctx, ngroups, slot_off, slots, ref_slot, nullptr, hipMemcpyHostToDevice, out,
                                hipMemcpyDeviceToHost);
}

int rf_score_dense_from(rf_ctx *ctx, int32_t ngroups, const int32_t *slot_off, const int32_t *slots,
                        const int32_t *ref_slot, const double *init, double *out)
{
    return score_dense_ref_impl(ctx, ngroups, slot_off, slots, ref_slot, init, hipMemcpyHostToDevice, out,
                                hipMemcpyDeviceToHost);
}

int rf_score_dense_from_dev(rf_ctx *ctx, int32_t ngroups, const int32_t *slot_off, const int32_t *slots,
                            const int32_t *ref_slot, const double *dev_init, double *dev_out)
{
    if (!dev_out)
        return fail(ctx, RF_ERR_ARG, "rf_score_dense_from_dev: null device buffer");
    return score_dense_ref_impl(ctx, ngroups, slot_off, slots, ref_slot, dev_init, hipMemcpyDeviceToDevice, dev_out,
                                hipMemcpyDeviceToDevice);
}

int64_t rf_host_reserve_fit(int64_t budget)
{
    if (budget < arena_capacity(0, 0))
        return -1;
    int64_t lo = 0, hi = budget;   // arena_capacity(lo, 0) <= budget < arena_capacity(hi + 1, 0)
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (arena_capacity(mid, 0) <= budget)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

int64_t rf_band_arena_bytes(const rf_ctx *ctx) { return ctx ? ctx->band_arena.cap : 0; }

int64_t rf_host_band_bytes(int32_t n, int32_t m, int32_t bw, int32_t pad)
{
    if (n < 1 || m < 0 || bw < 0)
        return -1;
    return 2 * band_region_bytes(n, m, bw, pad != 0);
}

int rf_last_score_launch(const rf_ctx *ctx, int32_t *launch)
{
    if (!ctx || !launch)
        return RF_ERR_ARG;
    std::copy(ctx->last_score, ctx->last_score + RF_SCL_FIELDS, launch);
    return 0;
}

int rf_host_score_plan(int32_t nreads, const int32_t *n, const int32_t *m, const int32_t *bw, const int32_t *stride,
                       const uint8_t *finite, int32_t ngroups, const int32_t *read_off, int32_t nopt,
                       const int32_t *opt_key, const int32_t *opt_val, int32_t per_seq, int32_t empty_ok,
                       int32_t *pick, int32_t *split, int32_t item_cap, int32_t *items, int32_t *nitems,
                       int64_t *dense_off, int64_t *split_off)
{
    if (nreads < 0 || ngroups < 0 || nopt < 0 || item_cap < 0 || !pick || !split || !nitems || !dense_off ||
        (nopt > 0 && (!opt_key || !opt_val)) || (nreads > 0 && (!n || !m || !bw || !finite)) ||
        (ngroups > 0 && (!read_off || !split_off || read_off[0] != 0 || read_off[ngroups] != nreads)) ||
        (ngroups == 0 && nreads > 0) || (item_cap > 0 && !items))
        return RF_ERR_ARG;
    ScoreOpts o;
    for (int32_t i = 0; i < nopt; ++i) {
        int *v = opt_key[i] == RF_OPT_SCORE_MODE ? &o.score_mode : opt_key[i] == RF_OPT_SCORE_KERNEL ? &o.score_kernel
                 : opt_key[i] == RF_OPT_LEAN_LDS_KB ? &o.lean_lds_kb : nullptr;
        if (!v)
            return RF_ERR_ARG;
        *v = opt_val[i];
    }
    std::vector<ScoreReadIn> in(nreads);
    std::vector<ScoreGroupIn> gin(ngroups);
    for (int32_t g = 0; g < ngroups; ++g) {
        if (read_off[g + 1] < read_off[g])
            return RF_ERR_ARG;
        gin[g] = {read_off[g], read_off[g + 1], read_off[g + 1] > read_off[g] ? m[read_off[g]] : 0, 0};
        for (int32_t r = read_off[g]; r < read_off[g + 1]; ++r) {
            // as rf_host_dp_plan: H and K = H + 2 m in range, a stride that holds the band's row pairs
            const int64_t H = 2 * (int64_t)bw[r] + std::abs((int64_t)n[r] - m[r]) + 1;
            if (n[r] < 0 || m[r] < 0 || bw[r] < 1 || m[r] != gin[g].m || H + 2 * (int64_t)m[r] > INT32_MAX / 2 ||
                (stride && (stride[r] < (H + 1) / 2 || stride[r] > (H + 1) / 2 + 16)))
                return RF_ERR_ARG;
            in[r] = {0, 0, 0, 0, n[r], m[r], bw[r], (int32_t)H, stride ? stride[r] : band_P((int)H), finite[r] != 0, false};
        }
    }
    ScorePlan P;
    if (int e = score_plan(in, gin, o, empty_ok != 0, P))
        return e;
    if (P.items.size() > (size_t)item_cap)
        return RF_ERR_ARG;
    pick[0] = P.pick.family();
    pick[1] = P.pick.lds;
    pick[2] = P.pick.cols();
    split[0] = score_split(P.items64, P.max_reads, o.score_mode, per_seq != 0);          // rf_score
    split[1] = score_split((int64_t)P.items.size(), P.max_reads, o.score_mode, false);   // the dense calls
    *nitems = (int32_t)P.items.size();
    for (size_t i = 0; i < P.items.size(); ++i) {
        items[2 * i] = P.items[i].group;
        items[2 * i + 1] = P.items[i].p0;
    }
    std::copy(P.gstart.begin(), P.gstart.end(), dense_off);
    for (int32_t g = 0; g < ngroups; ++g)
        split_off[g] = P.groups[g].split_off;
    return 0;
}

int rf_host_score_chunks(int32_t kernel, int32_t split, int32_t nitems, int32_t max_reads, int32_t score_wgs,
                         int32_t seg_wgs, int32_t *rchunk, int32_t *grid_y)
{
    if (kernel < RF_SCK_GENERAL || kernel > RF_SCK_WS || nitems < 1 || max_reads < 1 || !rchunk || !grid_y)
        return RF_ERR_ARG;
    const ScoreChunks ch = score_chunks(kernel, split != 0, nitems, max_reads, score_wgs, seg_wgs);
    *rchunk = ch.rchunk;
    *grid_y = (int32_t)ch.grid_y;
    return 0;
}

int rf_host_row_codes(int32_t nseq, const uint8_t *bases, const int64_t *off, const double *match,
                      const double *mismatch, const double *ins, const double *del, int32_t nup, const int32_t *up,
                      const uint8_t *flags, int32_t nthreads, uint8_t *coded, uint8_t *finite, uint64_t *records,
                      double *val3, double *val1, int64_t *sizes)
{
    return host_row_codes(nseq, bases, off, match, mismatch, ins, del, nup, up, flags, nthreads, coded, finite,
                          records, val3, val1, sizes);
}

int rf_host_upload_chunks(int32_t nseq, const int64_t *off, const int64_t *cins_off, const int64_t *cdel_off,
                          int32_t codes, int32_t stage_kb, int64_t budget, int32_t *end, int32_t *nchunks)
{
    return host_upload_chunks(nseq, off, cins_off, cdel_off, codes, stage_kb, budget, end, nchunks);
}

int rf_slot_geometry(rf_ctx *ctx, int32_t slot, int32_t which, int32_t *nrows, int32_t *ncols,
                     int32_t *bw, int32_t *H)
{
    if (!ctx || slot < 0 || slot >= (int32_t)ctx->slots.size())
        return fail(ctx, RF_ERR_ARG, "rf_slot_geometry: unknown slot");
    const Band &b = which == RF_BAND_A ? ctx->slots[slot].a : ctx->slots[slot].b;
    if (!b.valid)
        return fail(ctx, RF_ERR_STATE, "rf_slot_geometry: band not computed");
    if (nrows) *nrows = b.n + 1;
    if (ncols) *ncols = b.m + 1;
    if (bw) *bw = b.bw;
    if (H) *H = b.H;
    return 0;
}

int rf_download_band(rf_ctx *ctx, int32_t slot, int32_t which, double *out)
{
    if (!ctx || !out || slot < 0 || slot >= (int32_t)ctx->slots.size())
        return fail(ctx, RF_ERR_ARG, "rf_download_band: bad arguments");
    (void)hipSetDevice(ctx->device);
    const Band &b = which == RF_BAND_A ? ctx->slots[slot].a : ctx->slots[slot].b;
    if (!b.valid)
        return fail(ctx, RF_ERR_STATE, "rf_download_band: band not computed");
    // kappa-major device layout -> the reference's column-major data
    const int P = b.P;
    const int64_t K = band_K(b.H, b.m);
    std::vector<double> buf((size_t)K * P);
    HIPCHK(ctx, hipMemcpyAsync(buf.data(), ctx->band_arena.d + b.r.off, buf.size() * 8,
                               hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, stream_wait(ctx));
    for (int jj = 0; jj <= b.m; ++jj)
        for (int d = 0; d < b.H; ++d)
            out[(size_t)jj * b.H + d] = buf[(size_t)(d + 2 * jj) * P + (d >> 1)];
    return 0;
}

int rf_last_backtrace_ms(const rf_ctx *ctx, double *ms)
{
    if (!ctx || !ms)
        return RF_ERR_ARG;
    *ms = ctx->bt_ms;
    return 0;
}

int rf_last_codon_ms(const rf_ctx *ctx, double *ms)
{
    if (!ctx || !ms)
        return RF_ERR_ARG;
    *ms = ctx->codon_ms;
    return 0;
}

int rf_last_codon_dense_ms(const rf_ctx *ctx, double *ms)
{
    if (!ctx || !ms)
        return RF_ERR_ARG;
    *ms = ctx->codon_dense_ms;
    return 0;
}

int rf_last_timing(const rf_ctx *ctx, double *dp_ms, double *score_ms, double *gather_ms)
{
    if (!ctx)
        return RF_ERR_ARG;
    if (dp_ms) *dp_ms = ctx->dp_ms;
    if (score_ms) *score_ms = ctx->score_ms;
    if (gather_ms) *gather_ms = ctx->gather_ms;
    return 0;
}

}  // extern "C"

// alignment_error_probs's per-column sums on the device (k_aln_sums) for
// rf_aln_error_sums (rifraf_batch.cpp): returns 1 (nothing done) when a read
// has no row codes -- the caller then folds the moves on the host.  out NULL:
// the sums stay on the device (BUF_ALN_SUMS, rf_qv_probs).  A launch
// whose largest group has more than ALN_MARKS_MIN_READS reads uses
// k_aln_marks + k_aln_fold (RF_OPT_ALN_MARKS_MIN; tests set 0: always).
int rf_internal_aln_sums_dev(rf_ctx *ctx, int32_t ngroups, const int32_t *slot_off, const int32_t *slots,
                             const int32_t *tlen, double *out)
{
    if (ctx->opt.aln_sums_host)
        return 1;
    (void)hipSetDevice(ctx->device);
    const int32_t ns = ngroups > 0 ? slot_off[ngroups] : 0;
    std::vector<BTTask> tasks;
    std::vector<int64_t> offs;
    if (int e = build_bt_tasks(ctx, "rf_aln_error_sums", ns, slots, tasks, offs))
        return e;
    for (int32_t k = 0; k < ns; ++k)
        if (!ctx->seqs[ctx->slots[slots[k]].a.seq].coded)
            return 1;
    // errlut for the dictionary entries added since the last call
    DevCodeDict &D = ctx->codes;
    const size_t n3 = D.t3v.size() / 4;
    const double log3 = std::log10(3.0);
    for (size_t e = D.errv.size(); e < n3; ++e)
        D.errv.push_back(std::log10(1.0 - std::pow(10.0, D.t3v[4 * e])) - log3);
    if (int e = ensure_buf(ctx, D.errlut, (size_t)RF_CODES * 8))
        return e;
    if (n3 > D.uperr)
        HIPCHK(ctx, hipMemcpyAsync((double *)D.errlut.p + D.uperr, D.errv.data() + D.uperr, (n3 - D.uperr) * 8,
                                   hipMemcpyHostToDevice, ctx->stream));
    D.uperr = n3;
    std::vector<AlnSumRead> rd(ns);
    std::vector<AlnSumGroup> gr(ngroups);
    int64_t rows = 0;
    for (int32_t g = 0; g < ngroups; ++g) {
        gr[g] = {rows * 4, slot_off[g], slot_off[g + 1], tlen[g], 0};
        rows += tlen[g];
        for (int32_t k = slot_off[g]; k < slot_off[g + 1]; ++k) {
            const Band &b = ctx->slots[slots[k]].a;
            const SeqObj &S = ctx->seqs[b.seq];
            if (b.m != tlen[g])
                return fail(ctx, RF_ERR_ARG, "rf_aln_error_sums: consensus length differs from the A band's");
            rd[k] = {offs[k], S.tabs.off / 8 + row_code_off(S.n, S.ncins, S.ncdel), b.n, b.m, k, 0};
        }
    }
    if (ns > 0)
        if (int e = launch_backtraces(ctx, tasks, nullptr, 0))
            return e;
    if (int e = upload(ctx, ctx->scratch[BUF_ALN_READS], rd)) return e;
    if (int e = upload(ctx, ctx->scratch[BUF_ALN_GROUPS], gr)) return e;
    if (int e = ensure_buf(ctx, ctx->scratch[BUF_ALN_SUMS], (size_t)std::max<int64_t>(rows * 4 * 8, 16))) return e;
    int maxr = 0;
    for (int32_t g = 0; g < ngroups; ++g)
        maxr = std::max(maxr, slot_off[g + 1] - slot_off[g]);
    if (ngroups > 0 && maxr > ctx->opt.aln_marks_min && ns > 0) {
        // two launches: per-read marks, then a per-column ordered fold
        std::vector<int64_t> rbase(ns), gcol(ngroups + 1), gbase(ngroups);
        int64_t nm = 0, nc = 0;
        for (int32_t g = 0; g < ngroups; ++g) {
            gcol[g] = nc;
            gbase[g] = nm;
            nc += tlen[g];
            for (int32_t k = slot_off[g]; k < slot_off[g + 1]; ++k) {
                rbase[k] = nm;
                nm += tlen[g];
            }
        }
        gcol[ngroups] = nc;
        if (int e = upload(ctx, ctx->scratch[BUF_ALN_READ_BASE], rbase)) return e;
        if (int e = upload(ctx, ctx->scratch[BUF_ALN_GROUP_COL], gcol)) return e;
        if (int e = upload(ctx, ctx->scratch[BUF_ALN_GROUP_BASE], gbase)) return e;
        if (int e = ensure_buf(ctx, ctx->scratch[BUF_ALN_MARKS], (size_t)std::max<int64_t>(nm * 4, 16))) return e;
        HIPCHK(ctx, hipMemsetAsync(ctx->scratch[BUF_ALN_MARKS].p, 0, (size_t)nm * 4, ctx->stream));
        hipLaunchKernelGGL(k_aln_marks, dim3((unsigned)ns), dim3(64), 0, ctx->stream,
                           dev<const AlnSumGroup>(ctx, BUF_ALN_GROUPS), ngroups,
                           dev<const AlnSumRead>(ctx, BUF_ALN_READS),
                           dev<const int64_t>(ctx, BUF_ALN_READ_BASE), (const double *)ctx->tab_arena.d,
                           dev<const int8_t>(ctx, BUF_MOVES_OR_CTASKS), dev<const int32_t>(ctx, BUF_COUNTS_OR_PROPS),
                           dev<uint32_t>(ctx, BUF_ALN_MARKS));
        if (nc > 0)
            hipLaunchKernelGGL(k_aln_fold, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, ctx->stream,
                               dev<const AlnSumGroup>(ctx, BUF_ALN_GROUPS), ngroups,
                               dev<const int64_t>(ctx, BUF_ALN_GROUP_COL),
                               dev<const int64_t>(ctx, BUF_ALN_GROUP_BASE), dev<const uint32_t>(ctx, BUF_ALN_MARKS),
                               (const double *)D.lut.p, (const double *)D.errlut.p, dev<double>(ctx, BUF_ALN_SUMS), nc);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, pre_d2h(ctx));
        if (out)
            HIPCHK(ctx, hipMemcpyAsync(out, ctx->scratch[BUF_ALN_SUMS].p, (size_t)rows * 4 * 8, hipMemcpyDeviceToHost,
                                       ctx->stream));
    } else if (ngroups > 0) {
        hipLaunchKernelGGL(k_aln_sums, dim3((unsigned)ngroups), dim3(256), 0, ctx->stream,
                           dev<const AlnSumGroup>(ctx, BUF_ALN_GROUPS), dev<const AlnSumRead>(ctx, BUF_ALN_READS),
                           (const double *)ctx->tab_arena.d, dev<const int8_t>(ctx, BUF_MOVES_OR_CTASKS),
                           dev<const int32_t>(ctx, BUF_COUNTS_OR_PROPS), (const double *)D.lut.p,
                           (const double *)D.errlut.p, dev<double>(ctx, BUF_ALN_SUMS));
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, pre_d2h(ctx));
        if (out)
            HIPCHK(ctx, hipMemcpyAsync(out, ctx->scratch[BUF_ALN_SUMS].p, (size_t)rows * 4 * 8, hipMemcpyDeviceToHost,
                                       ctx->stream));
    }
    HIPCHK(ctx, stream_wait(ctx));
    if (ns > 0)
        note_bt_ms(ctx);
    return check_err(ctx);
}

// arena_grow count and seconds of a context (rf_rifraf_batch's RIFRAF_BATCH_TIMING line)
void rf_internal_arena_stats(const rf_ctx *ctx, int64_t *grows, double *secs)
{
    *grows = ctx ? ctx->arena_grows : 0;
    *secs = ctx ? ctx->arena_grow_s : 0.0;
}


// ---------------------------------------------------------------------
// k_qv: the quality pass's normalisations on the device (round 4)
//
// estimate_probs (model.jl:737-771, normalize_log_differences :722-735) and
// alignment_error_probs' final step (:835-839) for one cluster per
// workgroup, from its dense totals ((m+1) x 9, rf_score_dense's layout) and
// its per-column base-distribution sums (m x 4, k_aln_sums): the maxima,
// the checks and the row sums exactly as rf_host_qv_prep / rf_host_qv_finish
// (same order), with 10^x evaluated by the device's FP64 exp10 instead of the
// host's numpy power -- within 2 ulp of it, so the probabilities agree with
// the host path to ~1e-15 relative (tests/test_batch.py compares them at
// 1e-12), not bit for bit.  The consensus, scores and accepted proposals do
// not depend on this step.
// ---------------------------------------------------------------------
struct alignas(16) QvGroup {
    int64_t dense_off;   // doubles: (m + 1) x 9 dense totals
    int64_t sums_off;    // doubles: m x 4 alignment sums
    int64_t pos_off;     // rows of out_pos (m rows of 5)
    int64_t ins_off;     // rows of out_ins (m + 1 rows of 4)
    int64_t cons_off;    // bytes arena: the consensus bases
    double score;        // state.score
    int32_t m, pad;
};

__global__ void __launch_bounds__(256) k_qv(const QvGroup *__restrict__ groups, const double *__restrict__ dense,
                                            const double *__restrict__ sums, const uint8_t *__restrict__ bases,
                                            double *__restrict__ pos, double *__restrict__ ins,
                                            double *__restrict__ aln, int32_t *__restrict__ gerr)
{
    __shared__ double rS[4], rD[4], rI[4];
    __shared__ int rN[4];
    const QvGroup G = groups[blockIdx.x];
    const double *D = dense + G.dense_off;
    const uint8_t *cons = bases + G.cons_off;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, m = G.m;
    double mS = -RF_INF, mD = -RF_INF, mI = -RF_INF;
    int nan = 0;
    for (int p = tid; p <= m; p += 256) {
        const double *d = D + (size_t)p * 9;
        for (int q = 5; q < 9; ++q) {
            nan |= d[q] != d[q];
            mI = d[q] > mI ? d[q] : mI;
        }
        if (p >= 1) {
            const int cb = cons[p - 1];
            for (int q = 0; q < 5; ++q)
                nan |= (q != cb && d[q] != d[q]) ? 1 : 0;
            for (int q = 0; q < 4; ++q) {
                const double v = q == cb ? 0.0 + G.score : d[q];
                mS = v > mS ? v : mS;
            }
            mD = d[4] > mD ? d[4] : mD;
        }
    }
    // maxima are exact in any order
    for (int off = 32; off >= 1; off >>= 1) {
        mS = fmax(mS, __shfl_xor(mS, off));
        mD = fmax(mD, __shfl_xor(mD, off));
        mI = fmax(mI, __shfl_xor(mI, off));
        nan |= __shfl_xor(nan, off);
    }
    if (lane == 0) {
        rS[w] = mS;
        rD[w] = mD;
        rI[w] = mI;
        rN[w] = nan;
    }
    __syncthreads();
    mS = fmax(fmax(rS[0], rS[1]), fmax(rS[2], rS[3]));
    mD = fmax(fmax(rD[0], rD[1]), fmax(rD[2], rD[3]));
    mI = fmax(fmax(rI[0], rI[1]), fmax(rI[2], rI[3]));
    nan = rN[0] | rN[1] | rN[2] | rN[3];
    double mx = mS;   // Python max(mxS, mxD, mxI)
    if (mD > mx)
        mx = mD;
    if (mI > mx)
        mx = mI;
    const int e = nan ? 1 : mS - mx > 0.0 ? 2 : mD - mx > 0.0 ? 3 : mI - mx > 0.0 ? 4 : 0;
    if (tid == 0)
        gerr[blockIdx.x] = e;
    if (e)
        return;
    const double st_pow = exp10(G.score - mx);
    for (int p = tid; p <= m; p += 256) {
        const double *d = D + (size_t)p * 9;
        double ei[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            ei[q] = exp10(d[5 + q] - mx);
        const double si = st_pow + (((ei[0] + ei[1]) + ei[2]) + ei[3]);
        double *oi = ins + (size_t)(G.ins_off + p) * 4;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            oi[q] = ei[q] / si;
        if (p >= 1) {
            const int cb = cons[p - 1];
            double ep[5];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                ep[q] = exp10((q == cb ? 0.0 + G.score : d[q]) - mx);
            ep[4] = exp10(d[4] - mx);
            const double sp = (((ep[0] + ep[1]) + ep[2]) + ep[3]) + ep[4];
            double *op = pos + (size_t)(G.pos_off + p - 1) * 5;
#pragma unroll
            for (int q = 0; q < 5; ++q)
                op[q] = ep[q] / sp;
            const double *a = sums + G.sums_off + (size_t)(p - 1) * 4;
            double ea[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                ea[q] = exp10(a[q]);
            const double t = ((ea[0] + ea[1]) + ea[2]) + ea[3];
            double mxq = ea[0] / t;
#pragma unroll
            for (int q = 1; q < 4; ++q) {   // numpy max: NaN propagates
                const double v = ea[q] / t;
                mxq = (mxq != mxq || !(v <= mxq)) ? (mxq != mxq ? mxq : v) : mxq;
            }
            aln[G.pos_off + p - 1] = 1.0 - mxq;
        }
    }
}

extern "C" int rf_qv_probs(rf_ctx *ctx, int32_t ngroups, const int32_t *slot_off, const int32_t *slots,
                           const int32_t *tlen, const double *score, double *out_pos, double *out_ins,
                           double *out_aln, int32_t *err_out)
{
    if (!ctx || ngroups < 0 ||
        (ngroups > 0 && (!slot_off || !slots || !tlen || !score || !out_pos || !out_ins || !out_aln || !err_out)))
        return fail(ctx, RF_ERR_ARG, "rf_qv_probs: bad arguments");
    err_out[0] = err_out[1] = 0;
    if (ngroups == 0)
        return 0;
    (void)hipSetDevice(ctx->device);
    // 1. dense totals, kept on the device (BUF_DENSE_TOTALS, dplan's group offsets)
    if (int e = score_dense_impl(ctx, ngroups, slot_off, slots, nullptr, hipMemcpyDeviceToHost))
        return e;
    // 2. the alignment sums, kept on the device (BUF_ALN_SUMS); 1 = a read
    //    without row codes: the caller takes the host path
    if (int e = rf_internal_aln_sums_dev(ctx, ngroups, slot_off, slots, tlen, nullptr))
        return e;
    const ScorePlan &P = ctx->dplan.plan;
    std::vector<QvGroup> gq(ngroups);
    int64_t rows = 0;
    for (int32_t g = 0; g < ngroups; ++g) {
        if (P.groups[g].m != tlen[g])
            return fail(ctx, RF_ERR_ARG, "rf_qv_probs: consensus length differs from the bands'");
        QvGroup &q = gq[g];
        q.dense_off = P.groups[g].dense_off;
        q.sums_off = rows * 4;
        q.pos_off = rows;
        q.ins_off = rows + g;
        q.cons_off = P.groups[g].tb;   // the consensus the dense totals were scored against
        q.score = score[g];
        q.m = tlen[g];
        rows += tlen[g];
    }
    if (int e = upload(ctx, ctx->scratch[BUF_QV_GROUPS], gq)) return e;
    const size_t npos = (size_t)rows * 5, nins = (size_t)(rows + ngroups) * 4, naln = (size_t)rows;
    const size_t ob = align_up((npos + nins + naln) * 8, 256);
    if (int e = ensure_buf(ctx, ctx->scratch[BUF_QV_OUT], ob + (size_t)ngroups * 4)) return e;
    double *d_pos = dev<double>(ctx, BUF_QV_OUT), *d_ins = d_pos + npos, *d_aln = d_ins + nins;
    int32_t *d_gerr = (int32_t *)(dev<char>(ctx, BUF_QV_OUT) + ob);
    hipLaunchKernelGGL(k_qv, dim3((unsigned)ngroups), dim3(256), 0, ctx->stream, dev<const QvGroup>(ctx, BUF_QV_GROUPS),
                       dev<const double>(ctx, BUF_DENSE_TOTALS), dev<const double>(ctx, BUF_ALN_SUMS),
                       (const uint8_t *)ctx->bytes_arena.d, d_pos, d_ins, d_aln, d_gerr);
    HIPCHK(ctx, hipGetLastError());
    std::vector<int32_t> gerr(ngroups);
    HIPCHK(ctx, pre_d2h(ctx));
    HIPCHK(ctx, hipMemcpyAsync(out_pos, d_pos, npos * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(out_ins, d_ins, nins * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(out_aln, d_aln, naln * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(gerr.data(), d_gerr, (size_t)ngroups * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, stream_wait(ctx));
    for (int32_t g = 0; g < ngroups; ++g)
        if (gerr[g]) {
            err_out[0] = gerr[g];
            err_out[1] = g;
            break;
        }
    return 0;
}

// ---------------------------------------------------------------------
// Candidate selection on the device: get_candidates' filter
// (model.jl:499-526) and choose_candidates (proposals.jl:104-115) over a dense
// table in rf_score_dense's layout, one workgroup of 256 per group (one
// cluster).  Which slots are proposals, and their order, is stated once in
// rifraf_candidates.h (with the host restatement, rf_host_candidates) and in
// DESIGN.md §4 "Candidate selection".
//
// k_cand_select walks the group's 9 (m + 1) slots in proposal order, 256
// consecutive order indices at a time (one contiguous stretch of the table
// and of the mask, permuted only within a position's nine slots), and
// compacts the candidates in that order: a ballot per wave, the waves' counts
// through LDS, a running base.  Records past the capacity are counted only.
//
// k_cand_choose is the greedy choice without a sorted list: each round takes
// the first candidate in (descending score, proposal order) that comes after
// the last chosen one and whose position is not suppressed -- a block argmax
// over the table -- and then suppresses the positions nearer than min_dist in
// a bitmap of m + 1 bits in LDS.  Its memory does not depend on the number of
// candidates; it runs nchosen + 1 rounds.
// ---------------------------------------------------------------------
struct alignas(16) CandGroup {
    int64_t table_off;    // doubles: the group's (m + 1) x 9 totals
    int64_t mask_off;     // bytes: its (m + 1) x 9 mask (sources 1, 2, 4)
    int64_t cons_off;     // bytes: its consensus
    int64_t cand_off, chosen_off;   // records
    double score;         // state.score
    int32_t m, source;
    int32_t cand_cap, chosen_cap;
};

struct alignas(16) CandRec {
    double score;
    int32_t pos;
    uint8_t kind, base, pad[2];
};

// the candidate at order index t of the group, if it is one: slot index and total
__device__ __forceinline__ bool cand_at(const CandGroup &G, const double *__restrict__ T,
                                        const uint8_t *__restrict__ M, const uint8_t *__restrict__ cons, int64_t t,
                                        int &p, int &k, double &tot, int *__restrict__ err)
{
    p = (int)(t / 9);
    k = cand_slot_of_rank(G.source, (int)(t - (int64_t)p * 9));
    const int64_t at = (int64_t)p * 9 + k;
    const int mb = cand_source_reads_mask(G.source) ? M[at] : 0;
    // the cheap tests first: most slots of a mask are no proposals
    if (cand_source_reads_mask(G.source) && !mb)
        return false;
    if (!cand_is_proposal(G.source, p, k, p > 0 ? (int)cons[p - 1] : -1, mb))
        return false;
    tot = T[at];
    if (tot != tot) {
        if (err)
            set_err(err, 3);   // k_gather's: failed to compute a valid score
        return false;
    }
    return tot > G.score;
}

__device__ __forceinline__ CandRec cand_rec(int p, int k, double tot)
{
    CandRec r;
    r.score = tot;
    r.pos = p;
    r.kind = (uint8_t)cand_kind_of_slot(k);
    r.base = (uint8_t)cand_base_of_slot(k);
    r.pad[0] = r.pad[1] = 0;
    return r;
}

__global__ void __launch_bounds__(256) k_cand_select(const CandGroup *__restrict__ groups,
                                                     const double *__restrict__ table,
                                                     const uint8_t *__restrict__ mask,
                                                     const uint8_t *__restrict__ bases, CandRec *__restrict__ cand,
                                                     int32_t *__restrict__ ncand, int *__restrict__ err)
{
    __shared__ int wsum[4];
    const CandGroup G = groups[blockIdx.x];
    const double *T = table + G.table_off;
    const uint8_t *M = mask + G.mask_off;
    const uint8_t *cons = bases + G.cons_off;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t total = 9 * ((int64_t)G.m + 1);
    int base = 0;
    for (int64_t t0 = 0; t0 < total; t0 += 256) {
        const int64_t t = t0 + tid;
        int p = 0, k = 0;
        double tot = 0.0;
        const bool is = t < total && cand_at(G, T, M, cons, t, p, k, tot, err);
        const unsigned long long bal = __ballot(is);
        if (lane == 0)
            wsum[w] = __popcll(bal);
        __syncthreads();
        int wbase = 0, tile = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = wsum[i];
            wbase += i < w ? c : 0;
            tile += c;
        }
        const int idx = base + wbase + __popcll(bal & ((1ull << lane) - 1ull));
        if (is && idx < G.cand_cap)
            cand[G.cand_off + idx] = cand_rec(p, k, tot);
        base += tile;
        __syncthreads();   // wsum is written again
    }
    if (tid == 0)
        ncand[blockIdx.x] = base;
}

__global__ void __launch_bounds__(256) k_cand_choose(const CandGroup *__restrict__ groups,
                                                     const double *__restrict__ table,
                                                     const uint8_t *__restrict__ mask,
                                                     const uint8_t *__restrict__ bases, int min_dist,
                                                     const int32_t *__restrict__ ncand,
                                                     CandRec *__restrict__ chosen, int32_t *__restrict__ nchosen)
{
    extern __shared__ uint32_t supp[];   // min_dist >= 1: bit p set = position p is too near a chosen one
    __shared__ double rs[4];
    __shared__ int64_t ro[4];
    const CandGroup G = groups[blockIdx.x];
    const double *T = table + G.table_off;
    const uint8_t *M = mask + G.mask_off;
    const uint8_t *cons = bases + G.cons_off;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t total = 9 * ((int64_t)G.m + 1);
    const bool dist = min_dist >= 1;
    if (ncand[blockIdx.x] == 0) {   // the usual end of a stage: nothing to choose from
        if (tid == 0)
            nchosen[blockIdx.x] = 0;
        return;
    }
    if (dist)
        for (int i = tid; i < (G.m + 32) / 32; i += 256)
            supp[i] = 0;
    __syncthreads();
    int n = 0;
    double last_s = 0.0;
    int64_t last_o = -1;
    for (;;) {
        double bs = 0.0;
        int64_t bo = -1;   // none yet
        for (int64_t t = tid; t < total; t += 256) {
            int p, k;
            double tot;
            if (dist && ((supp[(int)(t / 9) >> 5] >> ((int)(t / 9) & 31)) & 1u))
                continue;
            if (!cand_at(G, T, M, cons, t, p, k, tot, nullptr))
                continue;
            if (n > 0 && !cand_before(last_s, last_o, tot, t))
                continue;   // chosen already, or skipped for good
            if (bo < 0 || cand_before(tot, t, bs, bo)) {
                bs = tot;
                bo = t;
            }
        }
        for (int off = 32; off >= 1; off >>= 1) {
            const double os = __shfl_xor(bs, off);
            const int64_t oo = __shfl_xor(bo, off);
            if (oo >= 0 && (bo < 0 || cand_before(os, oo, bs, bo))) {
                bs = os;
                bo = oo;
            }
        }
        if (lane == 0) {
            rs[w] = bs;
            ro[w] = bo;
        }
        __syncthreads();
        bs = rs[0];
        bo = ro[0];
#pragma unroll
        for (int i = 1; i < 4; ++i)
            if (ro[i] >= 0 && (bo < 0 || cand_before(rs[i], ro[i], bs, bo))) {
                bs = rs[i];
                bo = ro[i];
            }
        if (bo < 0)
            break;
        const int p = (int)(bo / 9);
        if (tid == 0 && n < G.chosen_cap)
            chosen[G.chosen_off + n] = cand_rec(p, cand_slot_of_rank(G.source, (int)(bo - (int64_t)p * 9)), bs);
        ++n;
        last_s = bs;
        last_o = bo;
        if (dist) {
            const int64_t lo = max((int64_t)0, (int64_t)p - (min_dist - 1));
            const int64_t hi = min((int64_t)G.m, (int64_t)p + (min_dist - 1));
            for (int64_t q = lo + tid; q <= hi; q += 256)
                atomicOr(&supp[q >> 5], 1u << (q & 31));
        }
        __syncthreads();   // the bitmap, and rs / ro before the next round writes them
    }
    if (tid == 0)
        nchosen[blockIdx.x] = n;
}

namespace {

// widest template whose suppression bitmap k_cand_choose holds in 48 KB of LDS
constexpr int64_t CAND_MAX_M = 48 * 1024 * 8 - 32;

// the outputs of the candidate calls, as the caller passed them
struct CandOut {
    int32_t *ncand;
    const int64_t *cand_off;
    uint8_t *cand_kind;
    int32_t *cand_pos;
    uint8_t *cand_base;
    double *cand_score;
    int32_t *nchosen;
    const int64_t *chosen_off;
    uint8_t *ch_kind;
    int32_t *ch_pos;
    uint8_t *ch_base;
    double *ch_score;
};

int cand_check(rf_ctx *ctx, const char *fn, int32_t ngroups, const CandOut &o)
{
    if (const char *why = cand_check_outputs(ngroups, o.cand_off, o.cand_kind, o.cand_pos, o.cand_base, o.cand_score))
        return fail(ctx, RF_ERR_ARG, std::string(fn) + ": candidate " + why);
    if (const char *why = cand_check_outputs(ngroups, o.chosen_off, o.ch_kind, o.ch_pos, o.ch_base, o.ch_score))
        return fail(ctx, RF_ERR_ARG, std::string(fn) + ": chosen " + why);
    return 0;
}

// The two kernels over groups whose table, mask and consensus offsets are
// set: record offsets and capacities from the caller's, one download of the
// counts and the records, one wait.
int cand_run(rf_ctx *ctx, const char *fn, std::vector<CandGroup> &gr, const double *d_table, const uint8_t *d_mask,
             const uint8_t *d_cons, int32_t min_dist, const CandOut &o)
{
    const int32_t ng = (int32_t)gr.size();
    ctx->cand_select_ms = ctx->cand_choose_ms = 0;
    if (ng == 0)
        return 0;
    int64_t max_m = 0;
    for (int32_t g = 0; g < ng; ++g) {
        CandGroup &G = gr[g];
        max_m = std::max<int64_t>(max_m, G.m);
        G.cand_off = o.cand_kind ? o.cand_off[g] - o.cand_off[0] : 0;
        G.chosen_off = o.ch_kind ? o.chosen_off[g] - o.chosen_off[0] : 0;
        G.cand_cap = o.cand_kind ? (int32_t)std::min<int64_t>(o.cand_off[g + 1] - o.cand_off[g], INT32_MAX) : 0;
        G.chosen_cap = o.ch_kind ? (int32_t)std::min<int64_t>(o.chosen_off[g + 1] - o.chosen_off[g], INT32_MAX) : 0;
    }
    if (max_m > CAND_MAX_M)
        return fail(ctx, RF_ERR_ARG, std::string(fn) + ": template too long for the suppression bitmap");
    const int64_t ncd = o.cand_kind ? o.cand_off[ng] - o.cand_off[0] : 0;
    const int64_t nch = o.ch_kind ? o.chosen_off[ng] - o.chosen_off[0] : 0;
    const size_t cb = (size_t)align_up((int64_t)ng * 2 * 4, 256);
    const size_t bytes = cb + (size_t)(nch + ncd) * sizeof(CandRec);
    if (int e = upload(ctx, ctx->scratch[BUF_CAND_GROUPS], gr)) return e;
    if (int e = ensure_buf(ctx, ctx->scratch[BUF_CAND_OUT], bytes)) return e;
    if (int e = ensure_landing(ctx, bytes)) return e;
    int32_t *d_cnt = dev<int32_t>(ctx, BUF_CAND_OUT);
    CandRec *d_ch = (CandRec *)(dev<char>(ctx, BUF_CAND_OUT) + cb), *d_cd = d_ch + nch;
    const CandGroup *d_gr = dev<const CandGroup>(ctx, BUF_CAND_GROUPS);
    const size_t lds = min_dist >= 1 ? (size_t)((max_m + 32) / 32) * 4 : 4;
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_CAND_SELECT_BEGIN], ctx->stream));
    hipLaunchKernelGGL(k_cand_select, dim3((unsigned)ng), dim3(256), 0, ctx->stream, d_gr, d_table, d_mask, d_cons,
                       d_cd, d_cnt, ctx->d_err);
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_CAND_CHOOSE_BEGIN], ctx->stream));
    hipLaunchKernelGGL(k_cand_choose, dim3((unsigned)ng), dim3(256), lds, ctx->stream, d_gr, d_table, d_mask, d_cons,
                       (int)min_dist, (const int32_t *)d_cnt, d_ch, d_cnt + ng);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(ctx->ev[EV_CAND_CHOOSE_END], ctx->stream));
    HIPCHK(ctx, pre_d2h(ctx));
    HIPCHK(ctx, land(ctx, 0, d_cnt, bytes));
    HIPCHK(ctx, land_wait(ctx));   // gr sources its upload until here
    ctx->cand_select_ms = mark_ms(ctx, EV_CAND_SELECT_BEGIN, EV_CAND_CHOOSE_BEGIN);
    ctx->cand_choose_ms = mark_ms(ctx, EV_CAND_CHOOSE_BEGIN, EV_CAND_CHOOSE_END);
    if (int e = check_landed(ctx))
        return e;
    const int32_t *cnt = landed<int32_t>(ctx);
    const CandRec *ch = landed<CandRec>(ctx, cb), *cd = ch + nch;
    auto unpack = [](const CandRec *r, int64_t n, uint8_t *kind, int32_t *pos, uint8_t *base, double *sc) {
        for (int64_t i = 0; i < n; ++i) {
            kind[i] = r[i].kind;
            pos[i] = r[i].pos;
            base[i] = r[i].base;
            sc[i] = r[i].score;
        }
    };
    for (int32_t g = 0; g < ng; ++g) {
        const CandGroup &G = gr[g];
        if (o.ncand)
            o.ncand[g] = cnt[g];
        if (o.nchosen)
            o.nchosen[g] = cnt[ng + g];
        if (o.cand_kind) {
            const int64_t at = o.cand_off[g];
            unpack(cd + G.cand_off, std::min<int64_t>(cnt[g], G.cand_cap), o.cand_kind + at, o.cand_pos + at,
                   o.cand_base + at, o.cand_score + at);
        }
        if (o.ch_kind) {
            const int64_t at = o.chosen_off[g];
            unpack(ch + G.chosen_off, std::min<int64_t>(cnt[ng + g], G.chosen_cap), o.ch_kind + at, o.ch_pos + at,
                   o.ch_base + at, o.ch_score + at);
        }
    }
    return 0;
}

}  // namespace

extern "C" int rf_candidates(rf_ctx *ctx, int32_t ngroups, const int32_t *slot_off, const int32_t *slots,
                             const int32_t *ref_slot, const double *score, const uint8_t *source,
                             const uint8_t *in_mask, int32_t min_dist, int32_t *ncand, const int64_t *cand_off,
                             uint8_t *cand_kind, int32_t *cand_pos, uint8_t *cand_base, double *cand_score,
                             int32_t *nchosen, const int64_t *chosen_off, uint8_t *ch_kind, int32_t *ch_pos,
                             uint8_t *ch_base, double *ch_score)
{
    if (!ctx || ngroups < 0 || (ngroups > 0 && (!slot_off || !slots || !score || !source)))
        return fail(ctx, RF_ERR_ARG, "rf_candidates: bad arguments");
    const CandOut o{ncand, cand_off, cand_kind, cand_pos, cand_base, cand_score,
                    nchosen, chosen_off, ch_kind, ch_pos, ch_base, ch_score};
    if (int e = cand_check(ctx, "rf_candidates", ngroups, o))
        return e;
    bool walks = false, given = false;
    for (int32_t g = 0; g < ngroups; ++g) {
        if (source[g] >= CAND_SRC_COUNT)
            return fail(ctx, RF_ERR_ARG, "rf_candidates: unknown source");
        walks = walks || source[g] == CAND_SRC_ALN || source[g] == CAND_SRC_ALN_SUBS;
        given = given || source[g] == CAND_SRC_MASK;
    }
    if (given && !in_mask)
        return fail(ctx, RF_ERR_ARG, "rf_candidates: source 4 needs a mask");
    // 1. the dense table, with the reference term where a group has one: its
    //    checks and refusals; the totals stay in BUF_DENSE_TOTALS
    if (int e = ref_slot ? rf_score_dense_ref(ctx, ngroups, slot_off, slots, ref_slot, nullptr)
                         : score_dense_impl(ctx, ngroups, slot_off, slots, nullptr, hipMemcpyDeviceToHost))
        return e;
    if (ngroups == 0)
        return 0;
    const ScorePlan &P = ctx->dplan.plan;
    std::vector<CandGroup> gr(ngroups);
    for (int32_t g = 0; g < ngroups; ++g) {
        CandGroup &G = gr[g];
        G.table_off = G.mask_off = P.groups[g].dense_off;
        G.cons_off = P.groups[g].tb;
        G.score = score[g];
        G.m = P.groups[g].m;
        G.source = source[g];
    }
    // 2. the mask: the caller's rows, then the walks' marks (with indels: a
    //    group of source 2 reads the substitution slots only)
    std::vector<uint8_t> hmask;   // sources its upload until cand_run's wait
    if (given) {
        hmask.assign((size_t)P.dense_total, 0);
        for (int32_t g = 0; g < ngroups; ++g)
            if (source[g] == CAND_SRC_MASK)
                std::memcpy(hmask.data() + gr[g].mask_off, in_mask + gr[g].mask_off, (size_t)(gr[g].m + 1) * 9);
        if (int e = upload(ctx, ctx->scratch[BUF_CAND_MASK], hmask)) return e;
    } else if (walks) {
        if (int e = ensure_buf(ctx, ctx->scratch[BUF_CAND_MASK], std::max<int64_t>(P.dense_total, 16))) return e;
        HIPCHK(ctx, hipMemsetAsync(ctx->scratch[BUF_CAND_MASK].p, 0, P.dense_total, ctx->stream));
    }
    if (walks) {
        std::vector<int32_t> ws;
        std::vector<int64_t> wmask;
        for (int32_t g = 0; g < ngroups; ++g)
            if (source[g] == CAND_SRC_ALN || source[g] == CAND_SRC_ALN_SUBS)
                for (int32_t k = slot_off[g]; k < slot_off[g + 1]; ++k) {
                    ws.push_back(slots[k]);
                    wmask.push_back(gr[g].mask_off);
                }
        std::vector<BTTask> tasks;
        std::vector<int64_t> offs;
        if (int e = build_bt_tasks(ctx, "rf_candidates", (int32_t)ws.size(), ws.data(), tasks, offs))
            return e;
        for (size_t k = 0; k < tasks.size(); ++k)
            tasks[k].mask = wmask[k];
        if (int e = launch_backtraces(ctx, tasks, dev<uint8_t>(ctx, BUF_CAND_MASK), 1))
            return e;
    }
    // 3. select and choose
    const int e = cand_run(ctx, "rf_candidates", gr, dev<const double>(ctx, BUF_DENSE_TOTALS),
                           dev<const uint8_t>(ctx, BUF_CAND_MASK), (const uint8_t *)ctx->bytes_arena.d, min_dist, o);
    if (walks && e != RF_ERR_HIP)
        note_bt_ms(ctx);
    return e;
}

extern "C" int rf_candidates_table(rf_ctx *ctx, int32_t ngroups, const int32_t *m, const uint8_t *cons,
                                   const int64_t *cons_off, const double *table, const uint8_t *mask,
                                   const double *score, const uint8_t *source, int32_t min_dist, int32_t *ncand,
                                   const int64_t *cand_off, uint8_t *cand_kind, int32_t *cand_pos, uint8_t *cand_base,
                                   double *cand_score, int32_t *nchosen, const int64_t *chosen_off, uint8_t *ch_kind,
                                   int32_t *ch_pos, uint8_t *ch_base, double *ch_score)
{
    if (!ctx)
        return RF_ERR_ARG;
    if (const char *why = cand_check_table(ngroups, m, cons, cons_off, table, mask, score, source))
        return fail(ctx, RF_ERR_ARG, std::string("rf_candidates_table: ") + why);
    const CandOut o{ncand, cand_off, cand_kind, cand_pos, cand_base, cand_score,
                    nchosen, chosen_off, ch_kind, ch_pos, ch_base, ch_score};
    if (int e = cand_check(ctx, "rf_candidates_table", ngroups, o))
        return e;
    (void)hipSetDevice(ctx->device);
    // the consensus bases packed group after group; table and mask as given
    std::vector<CandGroup> gr(ngroups);
    std::vector<uint8_t> hc;
    int64_t rows = 0;
    bool reads_mask = false;
    for (int32_t g = 0; g < ngroups; ++g) {
        CandGroup &G = gr[g];
        G.table_off = G.mask_off = rows * 9;
        G.cons_off = (int64_t)hc.size();
        if (m[g] > 0)
            hc.insert(hc.end(), cons + cons_off[g], cons + cons_off[g] + m[g]);
        G.score = score[g];
        G.m = m[g];
        G.source = source[g];
        reads_mask = reads_mask || cand_source_reads_mask(source[g]);
        rows += (int64_t)m[g] + 1;
    }
    if (int e = upload(ctx, ctx->scratch[BUF_CAND_TABLE], table, (size_t)rows * 9 * 8)) return e;
    if (int e = upload(ctx, ctx->scratch[BUF_CAND_CONS], hc)) return e;   // hc: alive until cand_run's wait
    if (int e = upload(ctx, ctx->scratch[BUF_CAND_MASK], mask, reads_mask ? (size_t)rows * 9 : 0)) return e;
    return cand_run(ctx, "rf_candidates_table", gr, dev<const double>(ctx, BUF_CAND_TABLE),
                    dev<const uint8_t>(ctx, BUF_CAND_MASK), dev<const uint8_t>(ctx, BUF_CAND_CONS), min_dist, o);
}

extern "C" int rf_host_candidates(int32_t ngroups, const int32_t *m, const uint8_t *cons, const int64_t *cons_off,
                                  const double *table, const uint8_t *mask, const double *score,
                                  const uint8_t *source, int32_t min_dist, int32_t *ncand, const int64_t *cand_off,
                                  uint8_t *cand_kind, int32_t *cand_pos, uint8_t *cand_base, double *cand_score,
                                  int32_t *nchosen, const int64_t *chosen_off, uint8_t *ch_kind, int32_t *ch_pos,
                                  uint8_t *ch_base, double *ch_score)
{
    if (cand_check_table(ngroups, m, cons, cons_off, table, mask, score, source) ||
        cand_check_outputs(ngroups, cand_off, cand_kind, cand_pos, cand_base, cand_score) ||
        cand_check_outputs(ngroups, chosen_off, ch_kind, ch_pos, ch_base, ch_score))
        return RF_ERR_ARG;
    return host_candidates(ngroups, m, cons, cons_off, table, mask, score, source, min_dist, ncand, cand_off,
                           cand_kind, cand_pos, cand_base, cand_score, nchosen, chosen_off, ch_kind, ch_pos, ch_base,
                           ch_score);
}

extern "C" int rf_last_candidates_ms(const rf_ctx *ctx, double *select_ms, double *choose_ms)
{
    if (!ctx)
        return RF_ERR_ARG;
    if (select_ms)
        *select_ms = ctx->cand_select_ms;
    if (choose_ms)
        *choose_ms = ctx->cand_choose_ms;
    return 0;
}
