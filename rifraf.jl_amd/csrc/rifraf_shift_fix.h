// rifraf_shift_fix.h -- frameshift correction from a pair's moves
// (single_indel_proposals, model.jl:538-562; apply_proposals,
// proposals.jl:80-102; are_ambiguous, proposals.jl:41-56): the per-move rules
// that k_pa_fix and the host share, and the plain host restatement of the
// kernel (rf_host_shift_fix).  No HIP: a plain C++17 compiler takes it alone.
// The rules are stated once at k_pa_fix in rifraf_hip.hip.
#ifndef RIFRAF_SHIFT_FIX_H
#define RIFRAF_SHIFT_FIX_H

#include <cstdint>

#include "../../include/rifraf_hip.h"
#ifndef RF_HD
#ifdef __HIPCC__
#define RF_HD __host__ __device__
#else
#define RF_HD
#endif
#endif

constexpr int SF_TALLIES = 5;   // int32 per pair: the moves of each code 1..5
constexpr int SF_INS = 1, SF_DEL = 2;   // the record kinds: Proposal's (rf_candidates' coding)

// offset_forward (align.jl:20-23) of a move code; 0 for anything else
RF_HD inline int sf_di(int mv) { return (mv == 1 || mv == 2) ? 1 : (mv == 4 ? 3 : 0); }
RF_HD inline int sf_dj(int mv) { return (mv == 1 || mv == 3) ? 1 : (mv == 5 ? 3 : 0); }
// bases a move adds to the corrected template: a match its template base, an
// insert the sequence's, a codon delete its three template bases
RF_HD inline int sf_width(int mv) { return (mv == 1 || mv == 2) ? 1 : (mv == 5 ? 3 : 0); }
// does the move give a proposal (an insert or a delete)?
RF_HD inline bool sf_proposes(int mv) { return mv == 2 || mv == 3; }

// k_pa_fix on the host for npairs pairs.  Pair k: moves[moves_off[k] ...],
// nmoves[k] of them (< 0: a failed pair, which gets the -1 outputs), the
// sequence sbases[s_off[k] .. s_off[k + 1]) and the template tbases[t_off[k] ..
// t_off[k + 1]).  The outputs are rf_pair_shifts'.  Returns 0, or RF_ERR_ARG
// (nothing written) for a missing array, a move code outside 1..5, moves that
// leave either string or record offsets that decrease.
inline int host_shift_fix(int64_t npairs, const int8_t *moves, const int64_t *moves_off, const int32_t *nmoves,
                          const uint8_t *sbases, const int64_t *s_off, const uint8_t *tbases, const int64_t *t_off,
                          uint8_t *fixed, const int64_t *fixed_off, int32_t *fixed_len, int32_t *nprops,
                          const int64_t *prop_off, uint8_t *prop_kind, int32_t *prop_pos, uint8_t *prop_base,
                          int32_t *tally)
{
    const int nrec = (prop_kind != nullptr) + (prop_pos != nullptr) + (prop_base != nullptr);
    if (npairs < 0 || (fixed && !fixed_off) || (nrec != 0 && nrec != 3) || (nrec == 3 && !prop_off))
        return RF_ERR_ARG;
    if (npairs > 0 && (!moves_off || !nmoves || !s_off || !t_off))
        return RF_ERR_ARG;
    for (int64_t k = 0; k < npairs; ++k) {
        const int64_t n = s_off[k + 1] - s_off[k], m = t_off[k + 1] - t_off[k];
        if (n < 0 || m < 0 || (nrec == 3 && (prop_off[k] < 0 || prop_off[k + 1] < prop_off[k])))
            return RF_ERR_ARG;
        if (nmoves[k] > 0 && (!moves || (n > 0 && !sbases) || (m > 0 && !tbases)))
            return RF_ERR_ARG;
        int64_t i = 0, j = 0;
        for (int32_t x = 0; x < nmoves[k]; ++x) {
            const int mv = moves[moves_off[k] + x];
            if (mv < 1 || mv > 5)
                return RF_ERR_ARG;
            i += sf_di(mv);
            j += sf_dj(mv);
            if (i > n || j > m)
                return RF_ERR_ARG;
        }
    }
    for (int64_t k = 0; k < npairs; ++k) {
        if (nmoves[k] < 0) {
            if (fixed_len)
                fixed_len[k] = -1;
            if (nprops)
                nprops[k] = -1;
            for (int c = 0; tally && c < SF_TALLIES; ++c)
                tally[k * SF_TALLIES + c] = -1;
            continue;
        }
        const uint8_t *s = sbases + s_off[k], *t = tbases + t_off[k];
        const int64_t cap = nrec == 3 ? prop_off[k + 1] - prop_off[k] : 0;
        int32_t cnt[SF_TALLIES] = {0, 0, 0, 0, 0};
        int64_t i = 0, j = 0, len = 0, np = 0, last_ins = -1;
        // two inserts at one j: no move between them advanced j
        bool ambiguous = false;
        for (int32_t x = 0; x < nmoves[k]; ++x) {
            const int mv = moves[moves_off[k] + x];
            j += sf_dj(mv);
            if (mv == 2) {
                ambiguous = ambiguous || j == last_ins;
                last_ins = j;
            }
        }
        j = 0;
        // apply_proposals fails on an ambiguous set: none of its bytes are written
        uint8_t *out = fixed && !ambiguous ? fixed + fixed_off[k] : nullptr;
        for (int32_t x = 0; x < nmoves[k]; ++x) {
            const int mv = moves[moves_off[k] + x];
            i += sf_di(mv);
            j += sf_dj(mv);
            ++cnt[mv - 1];
            if (sf_proposes(mv)) {
                if (np < cap) {
                    prop_kind[prop_off[k] + np] = (uint8_t)(mv == 2 ? SF_INS : SF_DEL);
                    prop_pos[prop_off[k] + np] = (int32_t)j;
                    prop_base[prop_off[k] + np] = mv == 2 ? s[i - 1] : 0;
                }
                ++np;
            }
            const int w = sf_width(mv);
            for (int u = 0; out && u < w; ++u)
                out[len + u] = mv == 2 ? s[i - 1] : t[j - w + u];
            len += w;
        }
        if (fixed_len)
            fixed_len[k] = ambiguous ? -2 : (int32_t)len;
        if (nprops)
            nprops[k] = (int32_t)np;
        for (int c = 0; tally && c < SF_TALLIES; ++c)
            tally[k * SF_TALLIES + c] = cnt[c];
    }
    return 0;
}

#endif
