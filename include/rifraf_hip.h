/*
 * rifraf_hip.h -- C-ABI of the MI355X-native RIFRAF hot-path engine
 * (librifraf_hip.so, built from rifraf.jl_amd/csrc/).
 *
 * The reference (Rifraf.jl) has no FFI layer: the hot path is a set of
 * internal Julia functions.  Each entry point below replaces one of them and
 * is what a Julia `ccall` or Python `ctypes` binds:
 *
 *   rf_set_sequences  <- RifrafSequence tables      src/rifrafsequences.jl:19-82
 *   rf_set_templates  <- state.consensus            src/model.jl:169
 *   rf_realign        <- forward_moves!/forward!/backward! over a batch
 *                        src/align.jl:114-141,155-179,196-202;
 *                        realign! src/model.jl:679-714
 *   rf_pair_scores    <- forward!(...)[end, end] over many pairs
 *                        src/align.jl:155-179
 *   rf_pair_align     <- backtrace(forward_moves(...)[2]) + count_errors over
 *                        many pairs (align_moves, align, edit_distance,
 *                        correct_shifts)  src/align.jl:114-153,229-260
 *   rf_pair_align_smart <- smart_forward_moves! (band doubling) over many
 *                        pairs  src/model.jl:643-672
 *   rf_pair_align_text <- align / moves_to_aligned_seqs, moves_to_indices and
 *                        band_tolerance over many pairs
 *                        src/align.jl:262-311,322-335,346-353
 *   rf_pair_errors    <- count_errors and smart_forward_moves!' band doubling
 *                        over many pairs, without moves
 *                        src/align.jl:240-250, src/model.jl:643-672
 *   rf_pair_shifts    <- single_indel_proposals, has_single_indels and
 *                        correct_shifts (apply_proposals, are_ambiguous) over
 *                        many pairs  src/model.jl:532-562,1303-1316,
 *                        src/proposals.jl:41-102, scripts/correct_shifts.jl:61-68
 *   rf_backtrace      <- backtrace + count_errors   src/align.jl:229-245
 *   rf_alignment_proposals <- alignment_proposals / moves_to_proposals
 *                        src/model.jl:458-497
 *   rf_score          <- score_proposal(m, state, newcols, use_ref) summed
 *                        over the batch, as called by get_candidates and
 *                        estimate_probs  src/model.jl:385-399,499-526,737-791
 *                        (per-sequence: score_nocodon :242-285 / codon
 *                        score_proposal :302-383 / seq_score_deletion :227-236)
 *   rf_score_dense_from <- the same left fold over the batch, continued from
 *                        a table of earlier reads' totals
 *                        src/model.jl:385-399
 *   rf_candidates     <- get_candidates' filter and choose_candidates over
 *                        the dense table, on the device
 *                        src/model.jl:499-526, src/proposals.jl:104-115
 *   rf_download_band  <- BandedArray data (tests)   src/bandedarrays.jl:5-42
 *
 * Conventions
 *  - Every call returns 0 on success and a negative code on failure; the
 *    message is rf_last_error(ctx), using the reference's error text
 *    ("new score is invalid", "failed to compute a valid score", ...).
 *  - Bases are 2-bit codes A=0, C=1, G=2, T=3 (BioSequences DNAAlphabet{2}).
 *  - Sequence tables are FP64 and uploaded bit-exact from the host (the
 *    host computes them exactly as RifrafSequence() does).
 *  - Proposal positions use the reference's 1-based Proposal.pos
 *    (Insertion(0, b) inserts before the first base). kind: 0 = Substitution,
 *    1 = Insertion, 2 = Deletion.
 *  - Bands stay device resident between calls.  A "slot" is one alignment
 *    (sequence x template) owning an A band and a B band: the H x (m+1) FP64
 *    cells of the reference's data[(i-j)+h_off+bw+1, j]
 *    (src/bandedarrays.jl:101-114), H = 2*bw + |n-m| + 1.  On the device a
 *    band is stored anti-diagonal ("kappa") major: cell (d, j) (0-based data
 *    row d, column j) at kappa = d + 2j, element d >> 1 of a kappa row of
 *    P = ((H+1) >> 1) | 1 doubles; the B band is stored
 *    already flipped.  rf_download_band converts to the reference's
 *    column-major data.
 *  - One context per host thread; calls are synchronous on the context's
 *    HIP stream.  No torch types cross this boundary.
 */
#ifndef RIFRAF_HIP_H
#define RIFRAF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RF_ABI_VERSION 1

/* rf_realign flags */
#define RF_FWD  1   /* A band: forward_moves!/forward!             align.jl:114,155 */
#define RF_BWD  2   /* B band: backward! (reverse forward + flip!) align.jl:196    */
#define RF_SKEW 4   /* skew_matches: mismatch score *= 0.99        align.jl:70-72  */
#define RF_TRIM 8   /* trim: free insertions in first/last column  align.jl:74-76  */

/* rf_download_band `which` */
#define RF_BAND_A 0
#define RF_BAND_B 1

/* error codes */
#define RF_ERR_ARG        (-1)
#define RF_ERR_HIP        (-2)
#define RF_ERR_NUMERIC    (-3)   /* a reference error() on the numeric path */
#define RF_ERR_STATE      (-4)   /* stale / mismatched bands */
#define RF_ERR_NEED_HOST  (-5)   /* rf_aln_error_sums: host bases / match scores needed (passed NULL) */

typedef struct rf_ctx rf_ctx;

int rf_abi_version(void);

/* Create a context on HIP device `device`. */
int rf_create(int device, rf_ctx **out);
int rf_destroy(rf_ctx *ctx);
const char *rf_last_error(const rf_ctx *ctx);

/* Tuning options of a context (rf_set_option / rf_get_option keys).  Every
 * value selects between code paths with bit-identical results; the defaults
 * are read once from the RIFRAF_* environment at rf_create.  No reference
 * counterpart (the reference has one code path). */
#define RF_OPT_SCORE_MODE   1   /* 0 auto, 1 fused in-kernel fold, 2 split + k_reduce  */
#define RF_OPT_SCORE_KERNEL 2   /* 0 auto, 1 general k_score, 2 k_score_segl, 3 k_score_ws whenever it fits */
#define RF_OPT_LEAN_LDS_KB  4   /* k_score_ws LDS budget in KB (0 = default 160)       */
/* key 9 (RF_OPT_BT_GLOBAL: every walk in the one-lane k_backtrace) removed in round 5 */
#define RF_OPT_DP_PSPLIT   10   /* lean DP stride-class split mask (-1 auto)           */
#define RF_OPT_DP_NP8      11   /* 0: H 128..255 bands in k_dp<64> instead of k_dpr<8> */
#define RF_OPT_DP_NP8_LEAN 12   /* 0: k_dpr<8> general steps only                      */
#define RF_OPT_DP_STREAMS  13   /* 0: DP classes serialised on the context stream      */
#define RF_OPT_BT_WIN_KB   15   /* k_bt_win A-window LDS: 16 (default) or 32 KB        */
#define RF_OPT_STAGE_KB    16   /* rf_set_sequences host staging chunk, KB of tables   */
#define RF_OPT_BAND_PAD    17   /* an rf_realign call whose widest band has H >= value
                                    lays out all its bands with kappa rows of whole
                                    128-B lines (default 64; 1 always, 0 never)       */
#define RF_OPT_DP_WIDE     18   /* lean DP task widths: bit 0 H 128..255 as 64-lane
                                    tasks (k_dpr<2,..,64>), bit 1 H 64..127 as 32-lane
                                    tasks (k_dpr<2,..,32>); 0 = 16-lane tasks only   */
#define RF_OPT_ALN_SUMS_HOST 19 /* 1: rf_aln_error_sums folds the moves on host
                                    threads instead of the device (k_aln_sums)     */
#define RF_OPT_ALN_MARKS_MIN 22 /* rf_aln_error_sums on the device: groups of more
                                   than this many reads (default 128) use the
                                   per-read marks + per-column fold launches      */
#define RF_OPT_SYNC_BLOCK  23   /* 1: host waits for the engine's stream yield
                                   the core, then sleep between event polls,
                                   instead of spinning (ranks held to a few
                                   host cores); 2: auto,
                                   sleep when the waiting thread may run on
                                   fewer than 4 CPUs (its affinity mask; the
                                   default)                                     */
#define RF_OPT_DP_NL64     24   /* at most this many non-lean DP tasks of H <= 127
                                   per call (codon / skew / trim) run as one
                                   latency-bound task per wave, k_dpx (default
                                   1024; 0: the 16-lane non-lean kernels)       */
#define RF_OPT_DP_LAT      26   /* latency mode: an rf_realign call with at most
                                   this many lean tasks of H <= 127 runs them all
                                   as one latency-bound task per wave (k_dpx, one
                                   launch; such a call cannot fill the GPU, so a
                                   task's step latency is the time).  Default
                                   2048; 0 never.  align.jl:114-212            */
#define RF_OPT_SCORE_WGS   27   /* split-mode k_score_ws: reads per workgroup chosen
                                   so that about this many workgroups remain
                                   (default 2048; small values: many reads per
                                   workgroup, partials written per read)        */
#define RF_OPT_SEG_WGS     28   /* split-mode k_score_segl: reads per workgroup
                                   chosen so that about this many workgroups
                                   remain (default 262144)                      */
#define RF_OPT_DP_PFIT     29   /* 1 (default): a lean NP >= 2 DP class in one
                                   launch takes the smallest stride class that
                                   holds its widest task (fewer repeated flush
                                   stores); 0: the class maximum                */
#define RF_OPT_DP_MC       30   /* 1 (default): bands of H > 2040 without codon
                                   moves (edit_distance's) filled across CUs in
                                   slices that hand off every 32 anti-diagonals
                                   (k_dpm); 0: one workgroup per band (k_dp)    */
#define RF_OPT_BT_NW       31   /* 4 (default): a backtrace launch of at most 64
                                   walks runs each on 4 waves (k_bt_win<4096, 4>,
                                   a 252-cell box); 1: one wave per walk        */
#define RF_OPT_PAIR_CHUNK  32   /* rf_pair_scores: pairs per launch set (default
                                   65536); descriptors and scores of one chunk are
                                   all the device memory the call needs         */
#define RF_OPT_PAIR_TRACE_MB 33 /* rf_pair_align: device bytes of move trace per
                                   launch set, MB (default 1024); a set also holds
                                   at most RF_OPT_PAIR_CHUNK pairs                */
#define RF_OPT_PAIR_WALK   34   /* the walk of rf_pair_align and of every round of
                                   rf_pair_align_smart (model.jl:643-672 walks the
                                   pending pairs once per round): 1: one lane per
                                   pair (k_pa_walk); 2: one wave per pair over a
                                   64-diagonal window of trace words held in the
                                   lanes (k_pa_walk_w); 0 (default): per launch
                                   set, the wave walk where the mean n + m of its
                                   pairs is at least 512, as measured for 16 to
                                   62,500 pairs.  Same moves and
                                   counts under every value                      */
#define RF_OPT_CAND_DEVICE  35   /* the native driver's get_candidates + choose_candidates
                                   (rf_rifraf_batch): 1: rf_candidates, on the device;
                                   0 (default): rf_alignment_proposals + rf_score and the
                                   host filter and sort.  Same candidates, chosen lists
                                   and runs under both values (DESIGN.md §4 "Candidate
                                   selection" has the measurement behind the default)  */
#define RF_OPT_PAIR_WIDE   36   /* the wide tier of the pair calls (rf_pair_scores,
                                   rf_pair_align, rf_pair_align_smart, rf_pair_align_text,
                                   rf_pair_errors, rf_pair_shifts): 0 (default): a band
                                   of more than 5,114 rows is RF_ERR_ARG, as ever.  1: such
                                   a pair runs in the wide tier (k_ps_wide / k_pa_wide /
                                   k_pe_wide: the same cell recurrence with its four
                                   anti-diagonals in device memory, one workgroup per
                                   pair at a time), every other pair as before.  v >= 2:
                                   also every pair whose band has at least v rows,
                                   whichever tier it would take (for tests of the
                                   tier at small shapes).  Same bits, moves and counts
                                   as the other tiers.  With the option on, rf_pair_errors
                                   counts its wide pairs in the fill (k_pe_wide); bands of
                                   3,408 to 5,114 rows keep the trace route.  The
                                   limits with the option on, checked before anything
                                   runs (RF_ERR_ARG): a band of at most
                                   RF_PAIR_WIDE_MAX_H rows, H + 2 m below 2^31 (the
                                   int32 fields of a task), and for the calls that
                                   keep a move trace fewer than 2^31 trace words per
                                   pair (ceil(ceil((H + 2 m) / 2) / 16) blocks of H
                                   rounded up to even: the lane walk's 32-bit index;
                                   16 GiB of trace).  A trace or ring the device cannot
                                   hold is RF_ERR_HIP from the allocation, as for
                                   every buffer, and changes nothing               */
#define RF_PAIR_WIDE_MAX_H (1 << 24)
#define RF_OPT_PAIR_RING_MB 37  /* device bytes of the wide tier's rings per launch
                                   set, MB (default 256).  A workgroup's ring is
                                   4 (H + 6) doubles for the widest wide pair of the
                                   set (12 instead of 8 bytes per entry in
                                   rf_pair_errors); as many workgroups run as the
                                   budget holds rings, at least one (0: exactly
                                   one) and at most one per pair, and loop over the
                                   pairs, longest first.  The ring memory is at most
                                   max(budget, one ring), whatever npairs is
                                   (rf_host_pair_wide_plan)                        */
/* Keys 3, 5-8, 14 and 20 selected scorer variants measured slower and removed
   in round 3 (k_score_lean, the 128-lane k_score_ws, k_score_seg /
   k_score_segc, 16-diagonal k_score_segl, the unspecialised k_score_w2);
   keys 9 (the one-lane k_backtrace walk), 21 (128-column k_score_segw) and 25
   (k_fuse, the fused forward fill + scoring step) in round 5.  rf_set_option rejects them. */
int rf_set_option(rf_ctx *ctx, int32_t key, int32_t value);
int rf_get_option(rf_ctx *ctx, int32_t key, int32_t *value);

/* Pre-size the device band arena (bytes); optional. */
int rf_reserve(rf_ctx *ctx, int64_t band_bytes);
/* Drop every slot's A and B band (each must be filled again before it is
 * read) and reuse the band arena from its start; the device memory is kept.
 * For a caller that starts a new batch of alignments (the batched driver's
 * waves), so an arena sized once serves every later batch. */
int rf_release_bands(rf_ctx *ctx);
/* Bytes currently allocated on the device by this context. */
int64_t rf_device_bytes(const rf_ctx *ctx);
/* Row-code dictionary of the context (the lean DP's 8-B per-row records):
   distinct (match, mismatch, ins) triples and del values held, reads left
   uncoded because the 65,536-entry dictionary was full (their DP reads the
   tables: slower, same values), and fresh starts (an upload that replaces
   every coded sequence resets it).  Engine-internal; no reference analog. */
int rf_code_stats(const rf_ctx *ctx, int64_t *entries3, int64_t *entries1, int64_t *uncoded_reads,
                  int64_t *resets);

/* Sequences (reads or a reference): ids [first, first+nseq).  Replaces any
 * previous content of those ids.  Every upload of an id (this call,
 * rf_set_sequences_codes, rf_set_sequences_codes_prep; identical content
 * included) makes the bands that were filled from it stale, like a template
 * upload does (rf_set_templates): rf_score, rf_score_dense(_dev),
 * rf_backtrace, rf_alignment_proposals, rf_aln_error_sums and rf_qv_probs
 * refuse such a slot, the reference slot included, with RF_ERR_STATE
 * ("sequence changed since the bands were computed") until rf_realign fills
 * it again; a fill of only one of its two bands leaves the other stale.
 * rf_download_band still returns the old cells.
 * A failed fill does the same: when rf_realign / rf_realign_jobs returns
 * RF_ERR_NUMERIC ("new score is invalid"), the reference's error() has left
 * no state behind, so the same calls refuse every band that call was asked to
 * fill -- the bands of its good jobs too -- with RF_ERR_STATE ("the last fill
 * of this band failed") until a later fill of the band succeeds.  Any other
 * failure of the call past its argument checks (RF_ERR_ARG changes nothing)
 * marks the bands it named in the same way.  The mark belongs to this
 * context: a caller that spreads one logical call over several contexts
 * applies it to the other contexts' bands itself.  The
 * partner band a forward-only or backward-only call did not name, and the
 * bands of slots it did not name, stay as they were; rf_download_band and
 * rf_slot_geometry still answer for a failed band.
 * Per sequence k (n_k = off[k+1]-off[k]):
 *   bases    off[k]..off[k+1]                    (n_k codes)
 *   match, mismatch, ins at off[k]..off[k+1]     (rifrafsequences.jl:45-47)
 *   del      at off[k]+k .. off[k+1]+k+1         (n_k+1, :49-53)
 *   cins     cins_off[k]..cins_off[k+1]           (n_k-2 or 0, :57-64)
 *   cdel     cdel_off[k]..cdel_off[k+1]           (n_k+1 or 0, :65-72)
 * cins/cdel/cins_off/cdel_off may be NULL (no codon moves).
 * Refusals change nothing.  All three upload calls check their pointers and
 * every sequence's lengths (n_k >= 1, cins 0 or n_k - 2 entries, cdel 0 or
 * n_k + 1) before their first state change: after RF_ERR_ARG the ids, their
 * tables and row codes, the code dictionary (rf_code_stats) and the bands
 * filled from the ids are as before the call, and still readable.  So are
 * they after rf_set_sequences_codes(_prep)'s RF_ERR_STATE ("row-code
 * dictionary full").  Any other failure (RF_ERR_HIP: an allocation, a HIP
 * error) comes after that point: the ids it named are then unknown to
 * rf_realign and their bands stale, until a later upload of them succeeds. */
int rf_set_sequences(rf_ctx *ctx, int32_t first, int32_t nseq,
                     const uint8_t *bases, const int64_t *off,
                     const double *match, const double *mismatch,
                     const double *ins, const double *del,
                     const double *cins, const int64_t *cins_off,
                     const double *cdel, const int64_t *cdel_off);
/* The same upload for Phred-coded reads without codon moves, with the
   tables built on the device from one byte per position: codes[off[k]..]
   index lp_t[256] (log10 error probability) and match_t[256]
   (log10(1 - 10^lp), both evaluated by the caller's libm, as the
   RifrafSequence constructor does, rifrafsequences.jl:19-53); mismatch /
   ins / del follow with the scores' mismatch / insertion / deletion by FP64
   addition and maximum -- bit-identical to rf_set_sequences of the host
   tables.  Moves 2 B per position over PCIe instead of ~41.  Returns
   RF_ERR_STATE when the row-code dictionary is full (upload host tables). */
int rf_set_sequences_codes(rf_ctx *ctx, int32_t first, int32_t nseq, const uint8_t *bases, const int64_t *off,
                           const uint8_t *codes, const double *lp_t, const double *match_t, double s_mis,
                           double s_ins, double s_del);
/* rf_set_sequences_codes plus the native driver's per-read setup values,
 * computed on the device from the same staged codes (k_code_prep, round 5;
 * bit-identical to rf_host_code_prep, which it replaces on the driver's
 * path): est[k] = est_n_errors (Julia-order sum of p10_t[code],
 * rifrafsequences.jl:74), ucode[k] = the code of the first maximal match
 * score, tsum[k] = the sequential sum of grid[ucode * 256 + code] --
 * logsumexp10 of the match scores is log10(tsum) + match_t[ucode]
 * (rf_host_lse_finish; util.jl:28-38, model.jl:575-579).  p10_t: 256 values
 * 10^lp; grid: 256 x 256, grid[u * 256 + x] = 10^(match_t[x] - match_t[u]). */
int rf_set_sequences_codes_prep(rf_ctx *ctx, int32_t first, int32_t nseq, const uint8_t *bases, const int64_t *off,
                                const uint8_t *codes, const double *lp_t, const double *match_t, double s_mis,
                                double s_ins, double s_del, const double *p10_t, const double *grid, double *est,
                                int32_t *ucode, double *tsum);

/* Templates (consensus sequences, one per cluster): ids [first, first+n).
 * Every upload of an id makes the bands filled against it stale: the calls
 * listed at rf_set_sequences refuse them with RF_ERR_STATE ("template changed
 * since the bands were computed") until rf_realign fills them again. */
int rf_set_templates(rf_ctx *ctx, int32_t first, int32_t ntpl,
                     const uint8_t *bases, const int64_t *off);

/* Templates with arbitrary ids: ids[k] receives bases off[k]..off[k+1]
 * (rf_set_templates for a sparse set, e.g. the clusters of a batched run
 * whose consensus changed this iteration). */
int rf_set_templates_ids(rf_ctx *ctx, int32_t ntpl, const int32_t *ids,
                         const uint8_t *bases, const int64_t *off);

/* Batched DP fill.  Job k aligns sequence seq[k] (rows) against template
 * tpl[k] (columns) with bandwidth bw[k] into slot slot[k].  flags: RF_FWD
 * and/or RF_BWD, optionally RF_SKEW / RF_TRIM (forward only).
 * out_score[k] (may be NULL) = A[end,end] if RF_FWD else B[1,1]. */
int rf_realign(rf_ctx *ctx, int32_t njobs, const int32_t *slot,
               const int32_t *seq, const int32_t *tpl, const int32_t *bw,
               int32_t flags, double *out_score);
/* rf_realign with flags per job (round 5): independent fills of one stage
 * machine step -- e.g. the reads' backward! and the reference's skewed
 * forward_moves! of single_indel_proposals (model.jl:538-562) -- share one
 * launch set, so a latency-bound task runs beside the others. */
int rf_realign_jobs(rf_ctx *ctx, int32_t njobs, const int32_t *slot,
                    const int32_t *seq, const int32_t *tpl, const int32_t *bw,
                    const int32_t *flags, double *out_score);

/* Score-only alignment: out[k] = A[end,end] of forward!(tpl[k], seq[k];
 * bandwidth bw[k]) (align.jl:155-179, cell rule :50-112) for npairs
 * independent pairs, without bands or slots -- exactly the value
 * rf_realign(..., RF_FWD | flags) writes to out_score[k], bit for bit, from a
 * fill that keeps only the last anti-diagonals on chip.  For R x T score
 * grids (which reference / cluster does a read belong to) whose bands would
 * not fit the device and that nobody reads.  flags: 0 or RF_SKEW / RF_TRIM;
 * RF_FWD is implied and accepted, RF_BWD is RF_ERR_ARG.  Unknown ids, bw < 1
 * and a band of more than 5,114 rows (2 bw + |n - m| + 1: what the widest
 * pass holds in LDS) are RF_ERR_ARG; RF_OPT_PAIR_WIDE lifts the band limit for
 * every pair call.  Sequences come from any of the three
 * upload calls, templates from rf_set_templates(_ids).  A pair the reference
 * raises on ("new score is invalid", align.jl:105-110) gets NaN and the call
 * still returns 0 (rf_score_dense's convention).  The call touches no slot,
 * makes no band stale or fresh and does not move the band arena; pairs are
 * sent RF_OPT_PAIR_CHUNK at a time, so device memory does not grow with
 * npairs. */
int rf_pair_scores(rf_ctx *ctx, int64_t npairs, const int32_t *seq, const int32_t *tpl,
                   const int32_t *bw, int32_t flags, double *out);
/* Kernel time of the last rf_pair_scores call (all its chunks), milliseconds. */
int rf_last_pair_ms(const rf_ctx *ctx, double *ms);

/* Alignments of npairs independent pairs without bands or slots: pair k is
 * backtrace(forward_moves(tpl[k], seq[k]; bandwidth bw[k], trim,
 * skew_matches)[2]) (align.jl:144-153, 229-238).  Its moves, in alignment
 * order and in rf_backtrace's int8 codes, go to moves[moves_off[k] ...]
 * (capacity n + m), their count to nmoves[k], count_errors (align.jl:240-245)
 * to nerrors[k] and A[end, end] -- the bits rf_pair_scores returns -- to
 * out_score[k].  Any output pointer may be NULL; moves and moves_off are NULL
 * together.  The fill keeps the scores on chip and writes a 4-bit move per
 * band cell (1/16 of an FP64 band); a walk follows the moves.
 * flags, id checks, bw < 1 and the band limit are rf_pair_scores' (RF_FWD
 * implied, RF_BWD is RF_ERR_ARG).  A pair the reference raises on ("new score
 * is invalid") gets score NaN, nmoves = nerrors = -1 and no moves; the call
 * still returns 0.  The call touches no slot, makes no band stale or fresh and
 * does not move the band arena.  Pairs go out in launch sets of at most
 * RF_OPT_PAIR_CHUNK pairs and RF_OPT_PAIR_TRACE_MB of trace (a single pair
 * above the budget runs alone), so device memory does not grow with npairs. */
int rf_pair_align(rf_ctx *ctx, int64_t npairs, const int32_t *seq, const int32_t *tpl,
                  const int32_t *bw, int32_t flags, double *out_score,
                  int8_t *moves, const int64_t *moves_off, int32_t *nmoves, int32_t *nerrors);
/* Kernel time of the last rf_pair_align call (all its sets), milliseconds:
 * the fills and the walks.  Either pointer may be NULL. */
int rf_last_pair_align_ms(const rf_ctx *ctx, double *fill_ms, double *walk_ms);

/* rf_pair_align with the band doubling of smart_forward_moves!
 * (model.jl:643-672), pair by pair: bw[k] is the starting bandwidth,
 * fixed[k] != 0 the sequence's bandwidth_fixed (fixed may be NULL: none),
 * threshold[k] the caller's cquantile(Poisson(est_n_errors), pvalue) as in
 * rf_rifraf_batch, and
 *   max_bw = fixed ? bw : min(bw << max_doublings, m, n)
 * with max_doublings in 0..5 (the reference's 2^5 is 5).  A round fills the
 * pair at its current bandwidth and stops if it is fixed or bw >= max_bw;
 * otherwise old = n_err, n_err = count_errors (both start at INT_MAX), and if
 * n_err > threshold && n_err < old the pair goes into another round at
 * bw = min(2 bw, max_bw).  A round submits only the pairs still pending.
 * out_score, moves, nmoves and nerrors are those of the pair's last fill
 * (nerrors is count_errors of the final moves, also when the loop stopped at
 * max_bw), out_bw[k] the final bandwidth and out_rounds[k] the number of
 * fills.  Any output pointer may be NULL; moves and moves_off are NULL
 * together.  A pair whose fill is invalid in some round stops there with
 * score NaN, nmoves = nerrors = -1 and out_bw the bandwidth that raised; the
 * call still returns 0.  Checked before anything runs, each RF_ERR_ARG with a
 * message naming the first such pair: rf_pair_align's checks, threshold
 * non-NULL, max_doublings in 0..5, and the band at max_bw within the 5,114
 * rows (2 max_bw + |n - m| + 1).  Like rf_pair_align the call touches no
 * slot, no band and not the band arena, and its device memory is bounded by
 * RF_OPT_PAIR_CHUNK / RF_OPT_PAIR_TRACE_MB, not by npairs or the number of
 * rounds.  max_doublings = 0 is rf_pair_align at bw, bit for bit.
 * rf_last_pair_align_ms then sums the fills and walks of all rounds. */
int rf_pair_align_smart(rf_ctx *ctx, int64_t npairs, const int32_t *seq, const int32_t *tpl,
                        const int32_t *bw, const double *threshold, const uint8_t *fixed,
                        int32_t max_doublings, int32_t flags, double *out_score, int8_t *moves,
                        const int64_t *moves_off, int32_t *nmoves, int32_t *nerrors,
                        int32_t *out_bw, int32_t *out_rounds);

/* rf_pair_align_smart that hands back what callers make of the moves instead
 * of the moves, computed on the device from the walk's output (k_pa_emit):
 *   aln_t, aln_s  align(t, s) (align.jl:346-353), i.e. moves_to_aligned_seqs
 *                 (align.jl:286-311): ASCII 'A' 'C' 'G' 'T' '-' at
 *                 aln_t / aln_s[aln_off[k] ...] (capacity n + m each, no
 *                 terminator), aln_len[k] bytes each.  A codon insertion is
 *                 "---" over s[i-2..i], a codon deletion t[j-2..j] over "---".
 *   t2s           moves_to_indices (align.jl:322-335) at t2s[t2s_off[k] ...]
 *                 (capacity m), t2s_len[k] entries: for every move that
 *                 advances j, the 1-based i reached (0 before the first
 *                 sequence base).  A codon deletion advances j by 3 and adds
 *                 one entry, as in the reference, so t2s_len < m then.
 *   tolerance     band_tolerance (align.jl:262-284) of the band
 *                 (n + 1, m + 1, out_bw[k]): the least |i - start| over the
 *                 path's cells with start > 1 and |i - stop| over those with
 *                 stop < n + 1, (start, stop) = row_range(band, j)
 *                 (bandedarrays.jl:133-137); n + 1 if no cell qualifies.
 * All describe the pair's last fill, like out_score, nerrors, out_bw and
 * out_rounds, which are rf_pair_align_smart's.  Every output pointer may be
 * NULL; aln_t and aln_s are NULL together and need aln_off, t2s needs
 * t2s_off (else RF_ERR_ARG).  If aln_t, aln_len, t2s, t2s_len and tolerance
 * are all NULL the kernel is not launched and the call is
 * rf_pair_align_smart without moves.  Checks, messages, flags (RF_FWD
 * implied, RF_BWD is RF_ERR_ARG), the 5,114-row limit at max_bw and the
 * return value are rf_pair_align_smart's, with one addition: with
 * max_doublings == 0 the call is rf_pair_align at bw and threshold may be
 * NULL.  A pair the reference raises on, or whose walk fails, gets
 * aln_len = t2s_len = tolerance = -1 and none of its bytes or entries are
 * written; the call still returns 0.  The moves are not downloaded.  The call
 * touches no slot, no band and not the band arena; its device memory is
 * bounded by RF_OPT_PAIR_CHUNK / RF_OPT_PAIR_TRACE_MB (per launch set: the
 * trace, n + m bytes of moves and of each text, and 4 m bytes of map). */
int rf_pair_align_text(rf_ctx *ctx, int64_t npairs, const int32_t *seq, const int32_t *tpl,
                       const int32_t *bw, const double *threshold, const uint8_t *fixed,
                       int32_t max_doublings, int32_t flags, double *out_score,
                       uint8_t *aln_t, uint8_t *aln_s, const int64_t *aln_off, int32_t *aln_len,
                       int32_t *t2s, const int64_t *t2s_off, int32_t *t2s_len,
                       int32_t *tolerance, int32_t *nerrors, int32_t *out_bw, int32_t *out_rounds);
/* Summed k_pa_emit time of the last rf_pair_align_text call, milliseconds
 * (0 if it launched none); rf_last_pair_align_ms reports its fills and walks. */
int rf_last_pair_text_ms(const rf_ctx *ctx, double *emit_ms);

/* Scores, error counts and the band doubling of smart_forward_moves!
 * (model.jl:643-672) of many pairs with nothing per cell leaving the chip.
 * count_errors (align.jl:240-250) is the number of alignment columns whose two
 * characters differ: along the path a match adds s[i] != t[j], an insertion or
 * a deletion 1, a codon move 3.  The path into a cell is the path into the
 * predecessor its move names, so the count rides through the fill beside the
 * score (k_pe / k_pe_gen) and comes out of the last cell with A[end, end]: no
 * move trace, no walk.  out_score, nerrors, out_bw and out_rounds equal what
 * rf_pair_align_smart returns with moves = moves_off = nmoves = NULL for the
 * same arguments: the scores bit for bit, the integers equal.  A pair the
 * reference raises on gets score NaN, nerrors = -1 and out_bw the bandwidth
 * that raised; the call still returns 0.  With max_doublings == 0 the call is
 * rf_pair_align's score and nerrors at bw and threshold may be NULL
 * (rf_pair_align_text's rule).  Checks, messages, flags (RF_FWD implied,
 * RF_BWD is RF_ERR_ARG), the 5,114-row limit at max_bw and the return value
 * are rf_pair_align_smart's.  Every output pointer may be NULL.  The call
 * touches no slot, no band and not the band arena.  Its device memory is
 * bounded by RF_OPT_PAIR_CHUNK: the descriptors plus 12 B per pair (score and
 * count), whatever npairs, the rounds or the cell counts are.  The exception
 * are pairs whose band is wider than 3,407 rows (two LDS rings, 48 (H + 6) B,
 * no longer fit 160 KiB): they run inside the same call through
 * rf_pair_align's trace fill and walk, with the same numbers, and add its
 * RF_OPT_PAIR_TRACE_MB budget. */
int rf_pair_errors(rf_ctx *ctx, int64_t npairs, const int32_t *seq, const int32_t *tpl,
                   const int32_t *bw, const double *threshold, const uint8_t *fixed,
                   int32_t max_doublings, int32_t flags, double *out_score, int32_t *nerrors,
                   int32_t *out_bw, int32_t *out_rounds);
/* Summed kernel time of the last rf_pair_errors call (all its sets and
 * rounds; the trace fills and walks of its widest pairs included),
 * milliseconds.  Leaves rf_last_pair_align_ms' values as they were. */
int rf_last_pair_errors_ms(const rf_ctx *ctx, double *fill_ms);

/* rf_pair_align that hands back frameshift correction instead of the moves,
 * computed on the device from the walk's output (k_pa_fix).  The sequence is
 * the reference, the template the consensus; i and j are the sequence and
 * template positions after a move.
 *   proposals   single_indel_proposals (model.jl:538-562) in move order: an
 *               insert gives Insertion(j, s[i-1]), a delete Deletion(j); kind
 *               1 / 2, 1-based pos (Insertion at 0 allowed) and base at
 *               prop_kind / prop_pos / prop_base[prop_off[k] ...].  The pair's
 *               capacity is prop_off[k+1] - prop_off[k] (npairs + 1 offsets):
 *               the first that many records are written, nprops[k] is the true
 *               count (rf_candidates' rule).
 *   fixed       correct_shifts (model.jl:1303-1316), i.e. apply_proposals
 *               (proposals.jl:80-102) of those proposals to the template:
 *               base codes 0..3 at fixed[fixed_off[k] ...] (capacity n + m),
 *               fixed_len[k] of them.  A set apply_proposals refuses
 *               (are_ambiguous, proposals.jl:41-56: two insertions at one
 *               position) gets fixed_len = -2 and no bytes; its proposals and
 *               tallies are reported.
 *   tally       5 int32 per pair: its moves of each code 1..5 (match, insert,
 *               delete, codon insert, codon delete).
 * The caller passes RF_SKEW for correct_shifts and single_indel_proposals and
 * 0 for has_single_indels (model.jl:532-536: tally[5k+1] + tally[5k+2] > 0).
 * Every output pointer may be NULL; fixed needs fixed_off, the three record
 * arrays are NULL together and need prop_off (else RF_ERR_ARG; a refused call
 * changes nothing).  If fixed, fixed_len, nprops, the records and tally are all
 * NULL the kernel is not launched and the call is rf_pair_align's score.
 * Checks, messages, flags (RF_FWD implied, RF_BWD is RF_ERR_ARG), the
 * 5,114-row limit and the return value are rf_pair_align's.  A pair the
 * reference raises on (score NaN), or whose walk fails, gets fixed_len =
 * nprops = -1, tallies of -1 and none of its bytes or records; the call still
 * returns 0.  The moves are not downloaded.  The call touches no slot, no band
 * and not the band arena; its device memory is bounded by RF_OPT_PAIR_CHUNK /
 * RF_OPT_PAIR_TRACE_MB (per launch set: rf_pair_align's, n + m bytes of
 * corrected template and at most 5 (n + m) bytes of records per pair). */
int rf_pair_shifts(rf_ctx *ctx, int64_t npairs, const int32_t *seq, const int32_t *tpl,
                   const int32_t *bw, int32_t flags, double *out_score,
                   uint8_t *fixed, const int64_t *fixed_off, int32_t *fixed_len,
                   int32_t *nprops, const int64_t *prop_off, uint8_t *prop_kind,
                   int32_t *prop_pos, uint8_t *prop_base, int32_t *tally);
/* Summed k_pa_fix time of the last rf_pair_shifts call, milliseconds (0 if it
 * launched none); rf_last_pair_align_ms reports its fills and walks. */
int rf_last_pair_shifts_ms(const rf_ctx *ctx, double *fix_ms);
/* rf_pair_shifts' products from given moves, on the host alone (no context,
 * no GPU; csrc/rifraf_shift_fix.h): pair k has nmoves[k] moves at
 * moves[moves_off[k] ...], the sequence sbases[s_off[k] .. s_off[k+1]) and the
 * template tbases[t_off[k] .. t_off[k+1]) (npairs + 1 offsets each).  A pair
 * with nmoves < 0 gets the -1 outputs.  Returns 0, or RF_ERR_ARG (nothing
 * written) for a missing array, a move code outside 1..5, moves that leave
 * either string, or record offsets that decrease. */
int rf_host_shift_fix(int64_t npairs, const int8_t *moves, const int64_t *moves_off,
                      const int32_t *nmoves, const uint8_t *sbases, const int64_t *s_off,
                      const uint8_t *tbases, const int64_t *t_off,
                      uint8_t *fixed, const int64_t *fixed_off, int32_t *fixed_len,
                      int32_t *nprops, const int64_t *prop_off, uint8_t *prop_kind,
                      int32_t *prop_pos, uint8_t *prop_base, int32_t *tally);

/* Backtrace of the A band of each slot (align.jl:229-238), moves in
 * alignment order written at moves[moves_off[k] ...] (capacity n+m each);
 * nmoves[k] = count; nerrors[k] = count_errors (align.jl:240-245).
 * Any of moves/moves_off/nmoves/nerrors may be NULL. */
int rf_backtrace(rf_ctx *ctx, int32_t nslots, const int32_t *slot,
                 int8_t *moves, const int64_t *moves_off,
                 int32_t *nmoves, int32_t *nerrors);

/* alignment_proposals (model.jl:483-497 over moves_to_proposals :458-480)
 * on the device: backtrace every batch slot of each group (one cluster) and
 * mark the proposals its alignment implies -- Substitution at mismatching
 * matches, and if do_indels, Insertion / Deletion -- in the group's dense
 * mask out_mask[(row_g + p) * 9 + k] (0/1 bytes, slots as rf_score_dense,
 * row_g = sum over h < g of (m_h + 1)).  The mask is the reference's Set
 * union over the batch; position-major order is (pos, kind, base) order. */
int rf_alignment_proposals(rf_ctx *ctx, int32_t ngroups, const int32_t *slot_off,
                           const int32_t *slots, int32_t do_indels, uint8_t *out_mask);

/* Proposal scoring.  Group g (one cluster) = batch slots
 * slots[slot_off[g] .. slot_off[g+1]) in batch order, an optional
 * reference slot ref_slot[g] (-1: none; scored with codon moves when its
 * sequence has codon tables), and proposals prop_off[g] .. prop_off[g+1].
 * out_total[k] = 0.0 + s_1 + ... + s_R (+ s_ref), the left fold of
 * model.jl:389-397.  out_per_seq (may be NULL) receives s_r for every
 * (proposal, batch slot) pair, row-major [k][r] with r in batch order,
 * followed by s_ref in an extra last column when the group has a
 * reference (row width R_g or R_g + 1). */
int rf_score(rf_ctx *ctx, int32_t ngroups,
             const int32_t *slot_off, const int32_t *slots,
             const int32_t *ref_slot, const int64_t *prop_off,
             const uint8_t *kind, const int32_t *pos, const uint8_t *base,
             double *out_total, double *out_per_seq);

/* Dense scoring of every proposal anchored at every consensus position --
 * the STAGE_SCORE all_proposals set (model.jl:401-456) that estimate_probs
 * scores (model.jl:737-791) -- for batch reads only (no reference):
 * out[(row_g + p) * 9 + k] = 0.0 + s_1 + ... + s_R for p = 0..m_g, with
 * k = 0..3 Substitution(p, A/C/G/T) (the consensus base's own slot is not a
 * proposal), k = 4 Deletion(p), k = 5..8 Insertion(p, A/C/G/T);
 * row_g = sum over h < g of (m_h + 1).  Sub/Del slots of p = 0 are NaN.
 * A failed update or a -Inf sum is reported as NaN in that slot (the
 * reference raises on such a proposal when it scores it).
 * out may be NULL: totals then stay on the device. */
int rf_score_dense(rf_ctx *ctx, int32_t ngroups, const int32_t *slot_off,
                   const int32_t *slots, double *out);

/* rf_score_dense with the totals written to DEVICE memory of the context's
 * device (dev_out: at least sum_g (m_g + 1) * 9 doubles, e.g. a torch tensor).
 * For the read-sharded exchange: each rank's partial fold
 * goes straight into the RCCL all-gather buffer without a host round trip. */
int rf_score_dense_dev(rf_ctx *ctx, int32_t ngroups, const int32_t *slot_off,
                       const int32_t *slots, double *dev_out);

/* rf_score_dense with the reference term of score_proposal(m, state, newcols,
 * use_ref = true) (model.jl:385-399 over :302-383): ref_slot[g] >= 0 adds
 * s_ref last, out = (0.0 + s_1 + ... + s_R) + s_ref; ref_slot[g] = -1 gives
 * rf_score_dense's bits for that group.  s_ref is rf_score's reference score
 * of the slot's proposal (codon moves when the reference's sequence has codon
 * tables), computed for the whole table by k_codon_dense without a
 * per-proposal descriptor or scratch column; a slot the reference would raise
 * on is NaN.  ref_slot must not be NULL; a reference slot must be known
 * (RF_ERR_ARG), hold current A and B bands (RF_ERR_STATE, as rf_score) of the
 * group's template (RF_ERR_ARG).  Everything else is rf_score_dense's,
 * out == NULL included. */
int rf_score_dense_ref(rf_ctx *ctx, int32_t ngroups, const int32_t *slot_off,
                       const int32_t *slots, const int32_t *ref_slot, double *out);

/* Dense scoring that continues a fold.  score_proposal's sum over the batch
 * (model.jl:385-399) is a plain left fold in read order, so it can be cut
 * anywhere and continued exactly: with init[e] the fold of reads 1..k-1,
 *   out[e] = ((init[e] + s_k) + s_{k+1}) + ... + s_R   (folded in batch order)
 * has the bits of the one-shot fold over reads 1..R.  A cluster of any depth
 * can so be scored chunk by chunk with only one chunk's bands on the device.
 * Layout, groups, slots, checks, stale-band refusals and messages are
 * rf_score_dense's; init and out both hold sum_g (m_g + 1) * 9 doubles in
 * that call's row layout.  out may be NULL: the totals stay on the device.
 * A group without reads stays RF_ERR_ARG (its template, and so its row count,
 * is not known without a slot).
 * init == NULL starts at 0.0: the call is then rf_score_dense (ref_slot NULL
 * or all -1) or rf_score_dense_ref, bit for bit.
 * ref_slot may be NULL (no reference term) or hold one entry per group (-1:
 * none); ref_slot[g] >= 0 adds s_ref last, after the reads of this call, as
 * rf_score_dense_ref does and with its checks.  A caller that chunks a
 * cluster passes the reference with the last chunk only.
 * NaN: a NaN in init stays NaN.  Each read's own term is made NaN where
 * rf_score_dense makes it NaN (Sub/Del of p = 0, a failed update, a -Inf
 * sum) before it is added -- the rule is applied per read, never to the
 * folded total -- so a chunked fold has NaN exactly where the one-shot fold
 * has.
 * A refused call changes nothing, out included.  rf_last_timing and
 * rf_last_score_launch report the call like any dense call (the upload of
 * init lies before the scorer's events); the launch plan is the one
 * rf_score_dense caches, so a chunk loop over one slot list plans once.
 * An added call: the ABI version stays 1. */
int rf_score_dense_from(rf_ctx *ctx, int32_t ngroups, const int32_t *slot_off, const int32_t *slots,
                        const int32_t *ref_slot, const double *init, double *out);

/* rf_score_dense_from with init and the totals in DEVICE memory of the
 * context's device.  dev_init may be NULL (start at 0.0); dev_out must not be
 * (RF_ERR_ARG).  The two may be the same buffer: the table then accumulates
 * in place. */
int rf_score_dense_from_dev(rf_ctx *ctx, int32_t ngroups, const int32_t *slot_off, const int32_t *slots,
                            const int32_t *ref_slot, const double *dev_init, double *dev_out);

/* Candidate selection on the device: the iteration loop's get_candidates ->
 * choose_candidates (model.jl:499-526, proposals.jl:104-115) for many groups
 * (clusters) at once, without the proposal list, the mask or the totals
 * crossing to the host.  The call is rf_score_dense -- rf_score_dense_ref when
 * ref_slot is not NULL, ref_slot[g] = -1 for a group without a reference --
 * followed by two kernels over the dense table, which stays on the device.
 *
 * Slot (p, k) of group g (k = 0..3 Substitution, 4 Deletion, 5..8 Insertion,
 * as rf_score_dense) is a proposal under source[g]:
 *   0  all_proposals with substitutions and indels (INIT / SCORE without
 *      seeds, model.jl:401-456); order within a position: Sub A..T, Del,
 *      Ins A..T
 *   1  alignment_proposals with indels (model.jl:483-497): the walks of
 *      rf_alignment_proposals run into a device mask that is not downloaded;
 *      order within a position Sub A..T, Ins A..T, Del -- the (pos, kind,
 *      base) order in which that call's mask is read
 *   2  alignment_proposals, substitutions only; order as 1
 *   3  every substitution (all_proposals in REFINE)
 *   4  in_mask's bytes for this group (FRAME: seeded all_proposals,
 *      indel_correction_only); order as 0.  in_mask has rf_score_dense's row
 *      layout for all groups; only the rows of source-4 groups are read, and it
 *      may be NULL when there are none
 * Under every source Sub and Del at p = 0 and the substitution to the
 * consensus base are no proposals, and Insertion(0, b) comes before position 1.
 * A proposal is a candidate iff total > score[g] on the FP64 total rf_score
 * returns for it (NaN compares false).  A proposal slot that holds NaN fails
 * the call as rf_score fails for a list with that proposal: RF_ERR_NUMERIC,
 * "failed to compute a valid score"; other slots may hold anything.
 *
 * Candidates are reported in proposal order; the chosen list is
 * choose_candidates': by descending score, equal scores to the earlier
 * proposal (a stable sort), skipping a candidate with |pos - q| < min_dist for
 * a position q chosen before it -- in rank order.  ncand[g] and nchosen[g] are
 * the true counts; the record arrays (kind 0 Sub / 1 Ins / 2 Del, 1-based pos,
 * base, score) receive the first off[g + 1] - off[g] entries of group g at
 * off[g].  Each set of four arrays is given together with its offsets or left
 * NULL (counts only); ncand and nchosen may be NULL too.
 *
 * Checks, stale-band refusals and messages are rf_score_dense(_ref)'s; a group
 * without reads is RF_ERR_ARG.  A template longer than 393,184 is RF_ERR_ARG
 * (the chooser's position bitmap lives in LDS).  The call fills no band, makes
 * none stale, and a refused call changes nothing. */
int rf_candidates(rf_ctx *ctx, int32_t ngroups, const int32_t *slot_off, const int32_t *slots,
                  const int32_t *ref_slot, const double *score, const uint8_t *source,
                  const uint8_t *in_mask, int32_t min_dist,
                  int32_t *ncand, const int64_t *cand_off, uint8_t *cand_kind, int32_t *cand_pos,
                  uint8_t *cand_base, double *cand_score,
                  int32_t *nchosen, const int64_t *chosen_off, uint8_t *ch_kind, int32_t *ch_pos,
                  uint8_t *ch_base, double *ch_score);
/* The same two kernels over a table the caller holds on the host (a table
 * summed elsewhere, e.g. across ranks): group g has a consensus of m[g] bases
 * at cons[cons_off[g] ...], its (m[g] + 1) x 9 totals in `table` and, for
 * sources 1, 2 and 4, its mask bytes in `mask` (both in rf_score_dense's row
 * layout; for sources 1 and 2 the mask is what rf_alignment_proposals
 * returned).  Needs no slots, sequences or bands.  Outputs as rf_candidates. */
int rf_candidates_table(rf_ctx *ctx, int32_t ngroups, const int32_t *m, const uint8_t *cons,
                        const int64_t *cons_off, const double *table, const uint8_t *mask,
                        const double *score, const uint8_t *source, int32_t min_dist,
                        int32_t *ncand, const int64_t *cand_off, uint8_t *cand_kind, int32_t *cand_pos,
                        uint8_t *cand_base, double *cand_score,
                        int32_t *nchosen, const int64_t *chosen_off, uint8_t *ch_kind, int32_t *ch_pos,
                        uint8_t *ch_base, double *ch_score);
/* rf_candidates_table on the host alone: no context, no GPU
 * (csrc/rifraf_candidates.h).  Returns 0, RF_ERR_ARG, or RF_ERR_NUMERIC for
 * NaN in a proposal slot.  No template length limit. */
int rf_host_candidates(int32_t ngroups, const int32_t *m, const uint8_t *cons, const int64_t *cons_off,
                       const double *table, const uint8_t *mask, const double *score,
                       const uint8_t *source, int32_t min_dist,
                       int32_t *ncand, const int64_t *cand_off, uint8_t *cand_kind, int32_t *cand_pos,
                       uint8_t *cand_base, double *cand_score,
                       int32_t *nchosen, const int64_t *chosen_off, uint8_t *ch_kind, int32_t *ch_pos,
                       uint8_t *ch_base, double *ch_score);
/* Kernel time of k_cand_select and k_cand_choose in the last rf_candidates /
 * rf_candidates_table call, milliseconds.  Either pointer may be NULL. */
int rf_last_candidates_ms(const rf_ctx *ctx, double *select_ms, double *choose_ms);

/* Native batched rifraf() (src/model.jl:1116-1275) for reference-free
 * clusters: the INIT stage of every cluster runs in lockstep on this context
 * with one batched engine call per step kind (rifraf_batch.cpp); each
 * cluster ends exactly as a separate rifraf() call would (consensus, score,
 * iteration count).  The caller (rifraf_amd.batch) uploads the reads and
 * initial consensus first and supplies the host values that need the Python
 * mirror's transcendental functions.
 *   read_off[c]..read_off[c+1]: cluster c's reads; read_seq / read_len per
 *     read: its sequence id and length; threshold per read:
 *     cquantile(Poisson(est_n_errors), bandwidth_pvalue) (model.jl:661)
 *   fixed_off / fixed: the fixed batch per cluster (local read indices in
 *     batch order, sortperm of est_n_errors; required if batch_fixed)
 *   random batches (resample!, model.jl:1038-1066: batch_size below the read
 *     count without batch_fixed, or in REFINE) are drawn here from
 *     params->est_n_errors (per read) and params->seed (per cluster), with
 *     rifraf_amd/resampling.py's RNG and draw; both NULL: such a cluster is
 *     rejected (RF_ERR_ARG)
 *   slot_base[c]: first of the cluster's batch slots; tpl_id[c]: its template
 *   cons / cons_off: the initial consensus per cluster (already uploaded)
 * Outputs per cluster: final score, INIT iterations, status (0 = reached
 * max_iters, 1 = converged, 2 = failed: rf_batch_fetch has the message; a
 * cluster whose accepted candidates remove every base of its consensus fails
 * with "empty consensus: ..." before a zero-length template is uploaded),
 * consensus length; out_bw per read = final bandwidth, negated once
 * bandwidth_fixed.  Results stay in the context until rf_batch_release. */
typedef struct rf_batch_params {
    int32_t max_iters;
    int32_t min_dist;
    int32_t bandwidth;               /* initial bandwidth of every read */
    int32_t do_alignment_proposals;
    int32_t batch_fixed;
    int32_t batch_size;              /* params.batch_size (<= 1: every read) */
    double batch_threshold;
    double batch_randomness;         /* initial state.batch_randomness (model.jl:592) */
    double batch_mult;               /* its decay per iteration (model.jl:1234-1238) */
    const double *est_n_errors;      /* per read, or NULL: resample!'s weights */
    const uint64_t *seed;            /* per cluster, or NULL: the random batches' RNG */
} rf_batch_params;
int rf_rifraf_batch(rf_ctx *ctx, int32_t nclusters, const rf_batch_params *params,
                    const int32_t *read_off, const int32_t *read_seq, const int32_t *read_len,
                    const double *threshold, const int32_t *fixed_off, const int32_t *fixed,
                    const int32_t *slot_base, const int32_t *tpl_id, const uint8_t *cons,
                    const int64_t *cons_off, double *out_score, int32_t *out_iters,
                    int32_t *out_status, int64_t *out_len, int32_t *out_bw);
/* Reference-guided clusters (FRAME and REFINE, model.jl:937-995, 499-562):
 * rf_rifraf_batch with, per cluster, a reference record (ref_seq < 0: none).
 * The stage machine then runs INIT -> FRAME -> REFINE like rifraf():
 * edit_distance at FRAME entry (align.jl:253-260, on edit_seq: the
 * reference's copy with log p = -1 and ErrorModel(1, 1, 1) scores, uploaded
 * by the caller), has_single_indels / single_indel_proposals (the reference
 * aligned to the consensus in scratch_slot), seeded all_proposals, scoring
 * with the reference's codon moves (ref_slot) and the reference term of
 * rescore!.  The two host steps that need the caller's transcendental
 * functions go through `cb`:
 *   event 0 (FRAME entry), value = ref_error_rate: build the reference with
 *     log p = log10(value) and the current reference scores, upload it at
 *     ref_seq, write *thr = cquantile(Poisson(est_n_errors), bandwidth_pvalue);
 *   event 1 (penalty increase), value = n_ref_indel_mults: rescale the
 *     reference's indel scores by ref_indel_mult^n (model.jl:978-985) and
 *     upload it again.
 * cb returns 0, or nonzero to fail the cluster.  Scope as rf_rifraf_batch. */
typedef struct rf_batch_ref_params {
    int32_t do_frame, do_refine, seed_indels, indel_correction_only;
    int32_t max_ref_indel_mults, pad;
    double ref_error_mult;
} rf_batch_ref_params;
typedef struct rf_batch_ref {
    int32_t ref_seq, edit_seq, ref_slot, scratch_slot;
    int64_t ref_off, ref_len;   /* the reference's bases in ref_bases */
} rf_batch_ref;
typedef int (*rf_ref_callback)(void *user, int32_t cluster, int32_t event, double value, double *thr);
int rf_rifraf_batch_ref(rf_ctx *ctx, int32_t nclusters, const rf_batch_params *params,
                        const rf_batch_ref_params *ref_params, const int32_t *read_off,
                        const int32_t *read_seq, const int32_t *read_len, const double *threshold,
                        const int32_t *fixed_off, const int32_t *fixed, const int32_t *slot_base,
                        const int32_t *tpl_id, const uint8_t *cons, const int64_t *cons_off,
                        const rf_batch_ref *refs, const uint8_t *ref_bases, rf_ref_callback cb,
                        void *cb_user, double *out_score, int32_t *out_iters, int32_t *out_status,
                        int64_t *out_len, int32_t *out_bw);
/* Stage record of cluster c of the last batch: iterations per stage (INIT,
 * FRAME, REFINE), the stage of each recorded consensus (1/2/3, as many as
 * rf_batch_fetch's stages), the reference's final bandwidth (negated once
 * fixed; 0 without one), A_ref[end,end], n_ref_indel_mults and the length
 * of the final batch (what rf_batch_fetch's `batch` receives: REFINE's
 * batch holds every read even when INIT / FRAME used the fixed batch). */
int rf_batch_fetch_ref(rf_ctx *ctx, int32_t cluster, int32_t *stage_iters, int8_t *stage_of,
                       int32_t *ref_bw, double *ref_score, int32_t *n_ref_indel_mults, int32_t *batch_len);
/* Cluster c of the last rf_rifraf_batch: consensus (out_len[c] bytes), the
 * consensus at each INIT iteration (stage_len[i] bytes each, concatenated
 * in `stages`), the final batch (local read indices; room for every read of
 * the cluster, or rf_batch_fetch_ref's batch_len) and the error message of a
 * failed cluster.  Any output may be NULL. */
int rf_batch_fetch(rf_ctx *ctx, int32_t cluster, uint8_t *cons, int64_t *stage_len, uint8_t *stages,
                   int32_t *batch, char *err, int64_t err_cap);
/* Free the context's stored batch results. */
void rf_batch_release(rf_ctx *ctx);
/* alignment_error_probs (model.jl:817-840) before its final normalisation,
 * for many groups at once: backtraces every slot of group g (slots
 * slot_off[g]..slot_off[g+1], batch order) and sums base_distribution(read
 * base, match score) (model.jl:804-809) at each match move, per consensus
 * column, in batch order: out[(row_g + j) * 4 + b], row_g = sum over h < g
 * of tlen[h].  bases[k] / match[k] point at slot k's read bases and match
 * scores (seq_len[k] each, host memory).  When every read is row-coded the
 * sums are folded on the device and bases / match may be NULL; if they are
 * NULL and the host fold is needed, RF_ERR_NEED_HOST. */
int rf_aln_error_sums(rf_ctx *ctx, int32_t ngroups, const int32_t *slot_off, const int32_t *slots,
                      const int32_t *tlen, const uint8_t *const *bases, const double *const *match,
                      const int32_t *seq_len, double *out);
/* The quality pass of many groups on the device (model.jl:737-771 estimate_probs
 * over the dense totals, normalize_log_differences :722-735, and
 * alignment_error_probs :817-840): out_pos[(row_g + p) * 5 + s] (p < m_g; s =
 * Sub A..T, Del at position p + 1), out_ins[(row_g + g + p) * 4 + b] (p <= m_g),
 * out_aln[row_g + p]; score[g] = state.score; err_out = {kind, group} (kind 1:
 * "failed to compute a valid score", 2 / 3 / 4: sub / deletion / insertion
 * scores cannot be positive).  10^x is the device's FP64 exp10 (~1e-15
 * relative of the host's).  Returns 1 (nothing done) when a read has no row
 * codes. */
int rf_qv_probs(rf_ctx *ctx, int32_t ngroups, const int32_t *slot_off, const int32_t *slots,
                const int32_t *tlen, const double *score, double *out_pos, double *out_ins, double *out_aln,
                int32_t *err_out);
/* Host sums of segments values[off[k]..off[k+1]): Julia 0.6 sum() order
 * (pairwise, blocks of 1024; rifrafsequences.jl:74 est_n_errors) and the
 * plain sequential order (cumsum(...)[end], util.jl:28-38 logsumexp10). */
int rf_host_julia_sums(int64_t nseg, const double *values, const int64_t *off, double *out);
int rf_host_seq_sums(int64_t nseg, const double *values, const int64_t *off, double *out);
/* RifrafSequence tables of many sequences from one byte code per position
 * (Phred scores): lp_t / p10_t / match_t per code, s_* the Scores terms;
 * concatenated outputs (del: n+1 per sequence at off[k]+k), est_n_errors. */
int rf_host_tables_from_codes(int64_t nseg, const uint8_t *codes, const int64_t *off, const double *lp_t,
                              const double *p10_t, const double *match_t, double s_mis, double s_ins,
                              double s_del, double *lp, double *match, double *mism, double *ins,
                              double *del, double *est);
/* Per segment, the sequential sum of grid[ucode[k] * 256 + codes[i]]. */
int rf_host_code_seq_sums(int64_t nseg, const uint8_t *codes, const int64_t *off, const int32_t *ucode,
                          const double *grid, double *out);
/* Native-driver setup from Phred codes without host tables: per sequence
 * est_n_errors (Julia-order sum of p10_t[code], rifrafsequences.jl:74), a
 * code of its maximum match score, and logsumexp10 of its match scores
 * (util.jl:28-38 with grid[u * 256 + x] = 10^(match_t[x] - match_t[u])). */
int rf_host_code_prep(int64_t nseg, const uint8_t *codes, const int64_t *off, const double *p10_t,
                      const double *match_t, const double *grid, double *est, int32_t *ucode, double *lse);
/* logsumexp10 from rf_set_sequences_codes_prep's outputs: lse[k] =
 * log10(tsum[k]) + match_t[ucode[k]] (libm log10), or match_t[ucode[k]] when
 * that is infinite -- the values rf_host_code_prep writes. */
int rf_host_lse_finish(int64_t nseg, const double *tsum, const int32_t *ucode, const double *match_t, double *lse);
/* estimate_probs (model.jl:742-800) and alignment_error_probs's
 * normalisation (model.jl:835-839) for K clusters, around the caller's 10^x:
 * prep checks the stacked dense totals D ((m_k+1) x 9 per cluster) and
 * writes the exponents xpos (M x 5: subs with the consensus slot = score,
 * deletion; minus the cluster maximum mx_k) and xins ((M+K) x 4); err[0] =
 * 1 NaN / 2 sub / 3 del / 4 ins positive, err[1] = cluster.  finish
 * normalises 10^xpos, 10^xins (with st_pow_k = 10^(score_k - mx_k)) and
 * 10^sums (M x 4, -> aln[M]) in place. */
int rf_host_qv_prep(int64_t K, const int64_t *moff, const double *D, const uint8_t *cons, const double *score,
                    double *xpos, double *xins, double *mx, int32_t *err);
int rf_host_qv_finish(int64_t K, const int64_t *moff, const double *st_pow, double *epos, double *eins,
                      const double *ealn, double *aln);

/* Geometry of a slot's band: nrows = n+1, ncols = m+1, bandwidth, H. */
int rf_slot_geometry(rf_ctx *ctx, int32_t slot, int32_t which,
                     int32_t *nrows, int32_t *ncols, int32_t *bw, int32_t *H);

/* Copy a slot's band (H x ncols doubles, column-major) to the host. */
int rf_download_band(rf_ctx *ctx, int32_t slot, int32_t which, double *out);

/* Kernel timing of the last rf_realign / rf_score call (HIP events on the
 * context stream), milliseconds; used by bench.py's roofline. */
int rf_last_timing(const rf_ctx *ctx, double *dp_ms, double *score_ms,
                   double *gather_ms);
/* Kernel time of the walks of the last rf_backtrace / rf_alignment_proposals
 * call (k_bt_win), milliseconds. */
int rf_last_backtrace_ms(const rf_ctx *ctx, double *ms);
/* Kernel time of the reference's codon score_proposal (k_codon,
 * model.jl:287-383) in the last rf_score call, milliseconds (0 when the call
 * scored no reference); it is part of that call's score_ms. */
int rf_last_codon_ms(const rf_ctx *ctx, double *ms);
/* k_codon_dense ms of the last rf_score_dense_ref (inside its score_ms). */
int rf_last_codon_dense_ms(const rf_ctx *ctx, double *ms);

/* The DP launch planner made observable (DESIGN.md §4 "DP launch planner").
 * Every kernel family computes the same bits, so only these two calls show
 * which one a task took.  A launch is a record of RF_DPL_FIELDS int32:
 * kernel (RF_DPK_*), npi (NP = 1 << npi per lane; the k_dpr families), pmi
 * (stride class, RF_DPK_DPR_LEAN_PM), first task, task count, stream (-1: the
 * context's stream, else side stream 0..2), grid x, block size, dynamic LDS
 * bytes (RF_DPK_DPM runs in chunks: the first chunk's grid).  No reference
 * counterpart. */
#define RF_DPK_DPR          0   /* k_dpr<NP, general>: four 16-lane tasks per wave     */
#define RF_DPK_DPR_LEAN     1   /* k_dpr<NP, lean>                                      */
#define RF_DPK_DPR_LEAN_PM  2   /* k_dpr<NP, lean, stride class pmi> (NP 1: exact P)    */
#define RF_DPK_DPR_WIDE64   3   /* lean H 128..255: one 64-lane task per wave           */
#define RF_DPK_DPR_WIDE32   4   /* lean H 64..127: two 32-lane tasks per wave           */
#define RF_DPK_DPX_CODON    5   /* k_dpx, few non-lean H <= 127 tasks, one per wave     */
#define RF_DPK_DPX_LEAN     6   /* k_dpx, latency mode: lean H <= 127, one per wave     */
#define RF_DPK_DP64         7   /* k_dp<64>: H <= 2040, one task per wave               */
#define RF_DPK_DPW_LDS      8   /* k_dp of 1,024 threads, ring in LDS                   */
#define RF_DPK_DPW_GLOBAL   9   /* k_dp of 1,024 threads, ring in global memory         */
#define RF_DPK_DPM         10   /* k_dpm: band slices across the CUs of an XCD          */
#define RF_DPL_FIELDS       9
/* rf_realign's planner on the host alone: no context, no GPU.  Job k is a read
 * of n[k] bases (ncins[k] / ncdel[k] codon table entries, finite[k]: no -Inf
 * table entry) against a template of m[k] at bandwidth bw[k] with flags[k]
 * (RF_FWD and / or RF_BWD, RF_SKEW, RF_TRIM).  stride_a / stride_b (each may be
 * NULL: the unpadded stride of the band's H) are the row strides of the A and
 * B bands.  Options: nopt pairs (opt_key[i] = RF_OPT_DP_*, opt_val[i]), the
 * rest at their defaults.  Outputs, each with room for 2 * njobs tasks / launch_cap
 * launches: per task in device order its job, direction (0 forward, 1
 * backward), launch (index into the launch records, which are in issue
 * order) and score slot (the job's own when the task's score is the one
 * rf_realign's out_score[job] reports, njobs + job for a backward fill beside
 * a forward one).  RF_ERR_ARG: bad arguments (a negative length or table
 * count, bw < 1, no direction, H + 2 m above 2^30, a stride below the band's
 * row pairs or more than 16 above them), an unknown key, or more launches
 * than launch_cap. */
int rf_host_dp_plan(int32_t njobs, const int32_t *n, const int32_t *m, const int32_t *bw, const int32_t *flags,
                    const int32_t *ncins, const int32_t *ncdel, const uint8_t *finite, const int32_t *stride_a,
                    const int32_t *stride_b, int32_t nopt, const int32_t *opt_key, const int32_t *opt_val,
                    int32_t *task_job, int32_t *task_dir, int32_t *task_launch, int32_t *task_out,
                    int32_t *ntasks, int32_t launch_cap, int32_t *launches, int32_t *nlaunches);
/* The launch records of the context's last successful rf_realign /
 * rf_realign_jobs, in issue order; RF_ERR_ARG when there are more than cap. */
int rf_last_dp_launches(const rf_ctx *ctx, int32_t cap, int32_t *launches, int32_t *nlaunches);
/* Where the context's regions lie in its bump-allocated arenas, for the tests
 * that place bands and tables at offsets beyond 32 bits and have to prove it
 * (DESIGN.md §4 "High arena offsets").  Reads only: no state changes.
 * slot >= 0: band[0] = byte offset and band[1] = capacity in bytes of band
 * `which` (RF_BAND_A / RF_BAND_B) of that slot in the band arena.  seq >= 0:
 * the same pair for the sequence's table region (tables and row codes, in the
 * table arena) in tabs[2] and for its bases (in the byte arena) in bases[2].
 * slot or seq = -1 asks for nothing of that kind, and its pointers may be
 * NULL; both -1 is RF_ERR_ARG.  A slot that is unknown or whose band holds no
 * region (never filled, or dropped by rf_release_bands), another `which`, and
 * an id without a completed upload are RF_ERR_ARG, with nothing written.
 * Offsets hold until the next call that allocates (an upload, a fill of a new
 * or larger band, rf_reserve, rf_release_bands).  An added call: the ABI
 * version stays 1, which changes only when a declared call or struct does.
 * Engine-internal; no reference counterpart. */
int rf_region_offsets(const rf_ctx *ctx, int32_t slot, int32_t which, int32_t seq, int64_t *band, int64_t *tabs,
                      int64_t *bases);

/* The bytes one slot's A band plus B band take in the band arena, on the host
 * alone: no context, no GPU.  For a read of n bases against a template of m
 * at bandwidth bw, filled by an rf_realign call that pads its bands to whole
 * 128-B lines (pad != 0: the call's widest band has H >= RF_OPT_BAND_PAD) or
 * does not (pad = 0).  H = 2 bw + |n - m| + 1 band rows, row stride
 * P = ((H + 1) >> 1) | 1 doubles (padded: (H + 1) >> 1 rounded up to 16),
 * H + 2 m kappa rows, each band's region rounded up to 256 bytes: computed by
 * the code the arena allocates with (csrc/rifraf_dp_plan.h), so it equals the
 * two capacities rf_region_offsets reports after a fill into fresh slots.  A
 * planner that cuts a deep cluster into chunks of a fixed band budget sums
 * it.  -1: n < 1, m < 0 or bw < 0.  An added call: the ABI version stays 1.
 * Engine-internal; no reference counterpart. */
int64_t rf_host_band_bytes(int32_t n, int32_t m, int32_t bw, int32_t pad);

/* The band arena against a budget.  rf_band_arena_bytes: the capacity in
 * bytes of the context's band arena now (0 before the first fill or
 * rf_reserve; it never shrinks).  rf_host_reserve_fit, on the host alone (no
 * context, no GPU): the largest band_bytes for which rf_reserve on a context
 * whose band arena is still empty allocates an arena of at most `budget`
 * bytes -- rf_reserve adds the arena's guards and a growth margin of an eighth
 * plus 1 MiB and rounds to whole MiB, and this inverts that arithmetic with
 * the code that does it -- or -1 when even rf_reserve(0) allocates more (a
 * budget below 2 MiB).  Bands of that many bytes (rf_host_band_bytes) then fit
 * the reserved arena without growing it.  Added calls: the ABI version stays
 * 1.  Engine-internal; no reference counterpart. */
int64_t rf_band_arena_bytes(const rf_ctx *ctx);
int64_t rf_host_reserve_fit(int64_t budget);

/* The scoring planner made observable (DESIGN.md §4 "Scoring planner"), for
 * the same reason: the three scorers, fused and split mode and both item
 * widths compute the same bits.  No reference counterpart. */
#define RF_SCK_GENERAL      1   /* k_score: any tables, 64 columns per item             */
#define RF_SCK_SEG          2   /* k_score_segl: finite tables, wide bands, 64 columns  */
#define RF_SCK_WS           3   /* k_score_ws: finite tables, 256 columns per item      */
#define RF_SCL_FIELDS       4
/* The scorer launch of the context's last successful rf_score, rf_score_dense,
 * rf_score_dense_dev, rf_score_dense_ref, rf_score_dense_from(_dev) or
 * rf_qv_probs, as RF_SCL_FIELDS
 * int32: kernel family (RF_SCK_*), split mode (0 / 1), work items, grid.y (0
 * items: nothing was launched, grid.y 0). */
int rf_last_score_launch(const rf_ctx *ctx, int32_t *launch);
/* The scoring planner on the host alone: no context, no GPU.  Read r has
 * n[r] bases against a template of m[r] at bandwidth bw[r] with band row
 * stride stride[r] (stride NULL: the unpadded stride of the band's H) and
 * finite[r] tables; group g holds reads [read_off[g], read_off[g + 1]), all
 * of one m.  Options: nopt pairs of RF_OPT_SCORE_MODE, RF_OPT_SCORE_KERNEL or
 * RF_OPT_LEAN_LDS_KB, the rest at their defaults.  per_seq: rf_score with
 * per-read output.  empty_ok: a group without reads is legal and gets no
 * items and no span (rf_score), else RF_ERR_ARG (the dense calls).  Outputs:
 * pick[3] = kernel family (RF_SCK_*), LDS doubles, columns per item;
 * split[2] = split mode as rf_score decides it (from the count of 64-column
 * items, with per_seq) and as the dense calls do (from the count of items);
 * the items as (group, first column) pairs, room for item_cap; per group
 * dense_off (ngroups + 1 values, the last the total) and split_off (doubles).
 * RF_ERR_ARG also for bad arguments as rf_host_dp_plan's, reads of several m
 * in a group, an unknown key and more items than item_cap. */
int rf_host_score_plan(int32_t nreads, const int32_t *n, const int32_t *m, const int32_t *bw, const int32_t *stride,
                       const uint8_t *finite, int32_t ngroups, const int32_t *read_off, int32_t nopt,
                       const int32_t *opt_key, const int32_t *opt_val, int32_t per_seq, int32_t empty_ok,
                       int32_t *pick, int32_t *split, int32_t item_cap, int32_t *items, int32_t *nitems,
                       int64_t *dense_off, int64_t *split_off);
/* The reads-per-workgroup rule of a scorer launch on the host alone: no
 * context, no GPU (csrc/rifraf_score_plan.h score_chunks).  A launch of
 * kernel family `kernel` (RF_SCK_*) in split mode (split != 0) or fused mode
 * over nitems work items of groups of at most max_reads reads, at
 * RF_OPT_SCORE_WGS = score_wgs and RF_OPT_SEG_WGS = seg_wgs (an option below
 * 1 counts as 1).  Outputs: *rchunk, the consecutive reads of a group one
 * workgroup takes, and *grid_y.  Fused: 1 and 1.  Split, RF_SCK_GENERAL: 1
 * and max_reads.  Split, RF_SCK_SEG: rchunk = ceil(nitems * max_reads /
 * seg_wgs), RF_SCK_WS: rchunk = max(1, floor(nitems * max_reads /
 * score_wgs)), and grid_y = ceil(max_reads / rchunk) in both; rchunk may
 * exceed max_reads (grid_y is then 1).  The product is taken in 64 bits.
 * RF_ERR_ARG: an unknown family, nitems or max_reads below 1, a NULL output. */
int rf_host_score_chunks(int32_t kernel, int32_t split, int32_t nitems, int32_t max_reads, int32_t score_wgs,
                         int32_t seg_wgs, int32_t *rchunk, int32_t *grid_y);

/* The launch of a set's wide pair class (RF_OPT_PAIR_WIDE) on the host alone:
 * no context, no GPU (csrc/rifraf_dp_plan.h pair_wide_plan).  H: the band rows
 * of the class's npairs pairs; mode: 0 the score alone (rf_pair_scores), 1 with
 * the move trace (rf_pair_align and its kin), 2 with the error count
 * (rf_pair_errors); budget: bytes of ring (RF_OPT_PAIR_RING_MB << 20).
 * Outputs, from 64-bit arithmetic: *ring_ld = max(H) + 6, the entries of one
 * anti-diagonal; *nwg = the workgroups, max(1, min(npairs, budget / one)) for
 * one = 4 ring_ld 8 bytes (mode 2: 4 ring_ld 12, the int32 counts behind the
 * doubles); *ring_bytes = nwg * one, what BUF_PAIR_RING holds.  RF_ERR_ARG:
 * npairs < 1, an H below 1 or above RF_PAIR_WIDE_MAX_H, an unknown mode, a
 * negative budget, a NULL pointer. */
int rf_host_pair_wide_plan(int64_t npairs, const int32_t *H, int32_t mode, int64_t budget, int64_t *nwg,
                           int64_t *ring_ld, int64_t *ring_bytes);

/* The row codes of rf_set_sequences on the host alone: no context, no GPU
 * (csrc/rifraf_seq_upload.h, DESIGN.md §4 "Sequence uploads").  nseq sequences
 * in rf_set_sequences' layout (bases, match, mismatch, ins at off[k], del at
 * off[k] + k; codon tables do not enter the records) are coded as nup uploads,
 * upload u the sequences [up[u], up[u + 1]) (up[0] = 0, up[nup] = nseq), on
 * nthreads host threads and a dictionary of the call's own.  flags[u] bit 0:
 * the upload starts a fresh dictionary (as one that replaces every coded
 * sequence of a context); bit 1: its dictionary entries are undone after it,
 * as rf_set_sequences_codes does when it refuses.  Outputs: per sequence
 * coded (a full dictionary leaves it 0) and finite (no non-finite value among
 * its 4 n + 1 table values); one 8-B record per position, at off[k] - off[0]
 * (bits 0-15 the code of (match, mismatch, ins)[i], 16-31 / 32-47 the codes of
 * del[i] / del[i + 1], 48-55 the base; zeros for an uncoded sequence); the
 * dictionary's values after the last upload, val3 (4 doubles per triple code:
 * match, mismatch, ins, 0) and val1 (a del value per code), each with room
 * for 65,536 codes; sizes[3] = triple codes, del codes, reads left uncoded.
 * The records and values do not depend on nthreads. */
int rf_host_row_codes(int32_t nseq, const uint8_t *bases, const int64_t *off, const double *match,
                      const double *mismatch, const double *ins, const double *del, int32_t nup, const int32_t *up,
                      const uint8_t *flags, int32_t nthreads, uint8_t *coded, uint8_t *finite, uint64_t *records,
                      double *val3, double *val1, int64_t *sizes);
/* The staging chunks of one upload of nseq sequences (off, cins_off, cdel_off
 * as rf_set_sequences'; codes != 0: rf_set_sequences_codes', no codon tables)
 * at RF_OPT_STAGE_KB = stage_kb, or within `budget` bytes when that is
 * positive: end[c] is one past the last sequence of chunk c (room for nseq),
 * *nchunks their number.  A chunk takes one sequence, then further ones while
 * its staged bytes fit the budget. */
int rf_host_upload_chunks(int32_t nseq, const int64_t *off, const int64_t *cins_off, const int64_t *cdel_off,
                          int32_t codes, int32_t stage_kb, int64_t budget, int32_t *end, int32_t *nchunks);

#ifdef __cplusplus
}
#endif
#endif
