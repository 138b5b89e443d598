// rifraf_candidates.h -- candidate selection over a dense proposal table
// (get_candidates, model.jl:499-526, and choose_candidates,
// proposals.jl:104-115): which slots of a group are proposals, their order,
// and the plain host restatement of k_cand_select / k_cand_choose
// (rf_host_candidates).  No HIP: a plain C++17 compiler takes it alone.  The
// rules are stated once in DESIGN.md §4 "Candidate selection".
#ifndef RIFRAF_CANDIDATES_H
#define RIFRAF_CANDIDATES_H

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "../../include/rifraf_hip.h"
#ifndef RF_HD
#ifdef __HIPCC__
#define RF_HD __host__ __device__
#else
#define RF_HD
#endif
#endif

// Where a group's proposals come from (the `source` byte of the calls)
constexpr int CAND_SRC_ALL = 0;        // all_proposals with subs and indels (INIT / SCORE, no seeds)
constexpr int CAND_SRC_ALN = 1;        // the alignments' proposals, with indels
constexpr int CAND_SRC_ALN_SUBS = 2;   // the alignments' substitutions
constexpr int CAND_SRC_SUBS = 3;       // every substitution (all_proposals in REFINE)
constexpr int CAND_SRC_MASK = 4;       // the caller's mask (FRAME)
constexpr int CAND_SRC_COUNT = 5;

RF_HD inline bool cand_source_reads_mask(int source)
{
    return source == CAND_SRC_ALN || source == CAND_SRC_ALN_SUBS || source == CAND_SRC_MASK;
}

// The dense slot (0..3 Sub, 4 Del, 5..8 Ins) that comes r-th (0..8) within a
// position: all_proposals emits Sub, Del, Ins (model.jl:401-456), the
// alignments' mask is read in (kind, base) order, Sub, Ins, Del.
RF_HD inline int cand_slot_of_rank(int source, int r)
{
    if (source == CAND_SRC_ALN || source == CAND_SRC_ALN_SUBS)
        return r < 4 ? r : r < 8 ? r + 1 : 4;
    return r;
}

// Is slot k of position p a proposal?  cons_base: the consensus base at p
// (any value at p = 0); mask_byte: the group's mask at (p, k), read only when
// cand_source_reads_mask.
RF_HD inline bool cand_is_proposal(int source, int p, int k, int cons_base, int mask_byte)
{
    if (k < 5 && p == 0)   // no Sub or Del before the first base
        return false;
    if (k < 4 && k == cons_base)
        return false;
    switch (source) {
    case CAND_SRC_ALL: return true;
    case CAND_SRC_ALN: return mask_byte != 0;
    case CAND_SRC_ALN_SUBS: return k < 4 && mask_byte != 0;
    case CAND_SRC_SUBS: return k < 4;
    case CAND_SRC_MASK: return mask_byte != 0;
    default: return false;
    }
}

// kind (0 Sub, 1 Ins, 2 Del) and base of a dense slot
RF_HD inline int cand_kind_of_slot(int k) { return k < 4 ? 0 : k == 4 ? 2 : 1; }
RF_HD inline int cand_base_of_slot(int k) { return k < 4 ? k : k == 4 ? 0 : k - 5; }

// does a candidate (score s, order index o) sort before (score t, order u)?
// Descending score, equal scores to the earlier proposal (a stable sort).
RF_HD inline bool cand_before(double s, int64_t o, double t, int64_t u) { return s > t || (s == t && o < u); }

// Both kernels on the host for ngroups groups over a table and mask in
// rf_score_dense's layout.  Returns 0, RF_ERR_ARG, or RF_ERR_NUMERIC when a
// proposal slot holds NaN (k_gather's refusal).
inline int host_candidates(int32_t ngroups, const int32_t *m, const uint8_t *cons, const int64_t *cons_off,
                           const double *table, const uint8_t *mask, const double *score, const uint8_t *source,
                           int32_t min_dist, int32_t *ncand, const int64_t *cand_off, uint8_t *cand_kind,
                           int32_t *cand_pos, uint8_t *cand_base, double *cand_score, int32_t *nchosen,
                           const int64_t *chosen_off, uint8_t *ch_kind, int32_t *ch_pos, uint8_t *ch_base,
                           double *ch_score)
{
    struct Rec {
        int32_t pos;
        int32_t slot;
        double score;
    };
    int64_t row = 0;
    std::vector<Rec> cands, chosen;
    for (int32_t g = 0; g < ngroups; ++g) {
        const int src = source[g];
        const uint8_t *t = cons + cons_off[g];
        cands.clear();
        for (int32_t p = 0; p <= m[g]; ++p)
            for (int r = 0; r < 9; ++r) {
                const int k = cand_slot_of_rank(src, r);
                const int64_t at = (row + p) * 9 + k;
                const int mb = cand_source_reads_mask(src) ? mask[at] : 0;
                if (!cand_is_proposal(src, p, k, p > 0 ? t[p - 1] : -1, mb))
                    continue;
                const double tot = table[at];
                if (tot != tot)
                    return RF_ERR_NUMERIC;
                if (tot > score[g])
                    cands.push_back({p, k, tot});
            }
        // choose_candidates: stable sort by descending score, then the greedy
        // distance filter over the positions already taken
        chosen = cands;
        std::stable_sort(chosen.begin(), chosen.end(), [](const Rec &x, const Rec &y) { return x.score > y.score; });
        size_t nc = 0;
        for (size_t i = 0; i < chosen.size(); ++i) {
            bool near = false;
            for (size_t j = 0; j < nc && !near; ++j)
                near = std::abs((int64_t)chosen[i].pos - chosen[j].pos) < min_dist;
            if (!near)
                chosen[nc++] = chosen[i];
        }
        chosen.resize(nc);
        auto put = [](const std::vector<Rec> &v, int64_t at, int64_t cap, uint8_t *kind, int32_t *pos, uint8_t *base,
                      double *sc) {
            for (int64_t i = 0; i < std::min<int64_t>((int64_t)v.size(), cap); ++i) {
                kind[at + i] = (uint8_t)cand_kind_of_slot(v[i].slot);
                pos[at + i] = v[i].pos;
                base[at + i] = (uint8_t)cand_base_of_slot(v[i].slot);
                sc[at + i] = v[i].score;
            }
        };
        if (ncand)
            ncand[g] = (int32_t)cands.size();
        if (nchosen)
            nchosen[g] = (int32_t)chosen.size();
        if (cand_kind)
            put(cands, cand_off[g], cand_off[g + 1] - cand_off[g], cand_kind, cand_pos, cand_base, cand_score);
        if (ch_kind)
            put(chosen, chosen_off[g], chosen_off[g + 1] - chosen_off[g], ch_kind, ch_pos, ch_base, ch_score);
        row += (int64_t)m[g] + 1;
    }
    return 0;
}

// The argument rules rf_candidates_table and rf_host_candidates share: NULL
// (everything fine) or what is wrong.  Record arrays come four at a time with
// their offsets, which must not decrease.
inline const char *cand_check_outputs(int32_t ngroups, const int64_t *off, const uint8_t *kind, const int32_t *pos,
                                      const uint8_t *base, const double *sc)
{
    const int n = (kind != nullptr) + (pos != nullptr) + (base != nullptr) + (sc != nullptr);
    if (n != 0 && n != 4)
        return "record arrays must be given together";
    if (n == 4 && ngroups > 0) {
        if (!off)
            return "record arrays need their offsets";
        for (int32_t g = 0; g < ngroups; ++g)
            if (off[g + 1] < off[g] || off[g] < 0)
                return "record offsets decrease";
    }
    return nullptr;
}

inline const char *cand_check_table(int32_t ngroups, const int32_t *m, const uint8_t *cons, const int64_t *cons_off,
                                    const double *table, const uint8_t *mask, const double *score,
                                    const uint8_t *source)
{
    if (ngroups < 0)
        return "bad arguments";
    if (ngroups == 0)
        return nullptr;
    if (!m || !cons_off || !table || !score || !source)
        return "bad arguments";
    for (int32_t g = 0; g < ngroups; ++g) {
        if (m[g] < 0)
            return "negative template length";
        if (m[g] > 0 && !cons)
            return "bad arguments";
        if (source[g] >= CAND_SRC_COUNT)
            return "unknown source";
        if (cand_source_reads_mask(source[g]) && !mask)
            return "source needs a mask";
    }
    return nullptr;
}

#endif
