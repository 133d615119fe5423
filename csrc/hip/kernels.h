// Host-visible launch interface of the oni_ml_amd HIP kernels (gfx950).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace oni {

// Padded topic counts (row stride of word-major beta, multiple of 4) that have
// compiled kernel instantiations.  Any K is served by the next larger entry;
// padding topics carry beta = 0 and are masked in the per-topic phase.
// Device parameter block (double[kParamCount]) read by the E-step kernels and
// written by the alpha Newton / EM control kernels; kParamDone != 0 gates every
// kernel of the EM iteration (device-side convergence, em_control.hip).
constexpr int kParamDone = 4;
constexpr int kParamCount = 8;
constexpr int kHistCols = 6;

#define ONI_FOR_EACH_KS(X) X(8) X(12) X(16) X(20) X(24) X(32) X(52) X(64) X(100) X(128)

// Huge documents (the long-context analogue): one document over
// several workgroups that exchange their per-chunk partials through global memory
// as tagged granules (launch_gs_split).  All workgroups of one launch must be
// co-resident: the host caps a launch below gs_split_capacity(KS).
struct SplitArgs {
  const int* seg_doc;     // [n_blocks] document of each workgroup
  const int* seg_index;   // [n_blocks] segment number within its document
  const int* seg_count;   // [n_blocks] segments of that document
  const int* seg_base;    // [n_blocks] block id of the document's segment 0
  const int* doc_slot;    // [n_blocks] counter slot of the document
  int n_blocks;
  int tab_rows;           // rows per workgroup of `tab` (>= nch of every document of the launch)
  unsigned long long* xchg;  // tagged granules (parity double-buffer), layout per kernel; gs_splitw:
                             // [2][n_blocks][2 (KS + 1)] partials, then [2][n_docs][2 (KS + 1)] totals
  int* counter;           // [2][n_docs] per document: launch epoch (tags of different launches never
                          // match), exit count (the last segment out bumps the epoch, resets the count)
  int n_docs;             // documents in this launch
  int* error;             // set to 1 if a wait times out (never hangs the GPU)
  double* tab = nullptr;  // U > the LDS table rows (KS > 32): per-segment chunk tables [n_blocks][tab_rows][2][KS]
  const double* csum = nullptr;  // [n_docs][csum_stride] chunk count sums of each document (nullptr: the
  int csum_stride = 0;           // kernel sums the counts itself)
};

// Sufficient-statistic launches: workgroups for [heavy | medium | light] word lists
// (a heavy word per workgroup, 4 medium or 16 light words per workgroup).
int suff_fused_blocks(int n_heavy, int n_medium, int n_light);

// alpha Newton on the device: reads scalars[1] (alpha_ss), writes params[0..1]
// (alpha, lgamma(K alpha) - K lgamma(alpha)) and alpha_out[0].
// Skipped once params[kParamDone] is set.
void launch_alpha_newton(const double* scalars, double num_docs, int K, bool estimate, double* params,
                         double* alpha_out, hipStream_t s);

// Device-side EM convergence test (em_control.hip), the lda-c driver loop
//   while ((conv < 0 || conv > EM_CONVERGED || i <= 2) && i <= EM_MAX_ITER)
// evaluated after each iteration without a host round trip.  ctl (double[8]):
//   [0] previous likelihood  [1] EM_CONVERGED  [2] history slot  [3] iteration i
//   [4] EM_MAX_ITER  [5] stop allowed (0: never set done)
// scalars = {likelihood, alpha_ss}.  It appends {likelihood, conv, alpha (params[0]),
// VAR_MAX_ITER, alpha_ss, -} (kHistCols
// doubles) to hist[slot], doubles
// VAR_MAX_ITER in params when the likelihood decreased (lda-c), and sets
// params[kParamDone] when the loop ends.
void launch_em_control(const double* scalars, double* params, double* ctl, double* hist, int hist_slots,
                       hipStream_t s);

// M-step fused with the EM control step (launch_gs_mstep_control): the last workgroup to finish
// (every other one has read the gate) runs em_control_step.  done_count: one int, zero before the
// first launch, left zero by the kernel.
struct EMControlArgs {
  const double* scalars;
  double* params;
  double* ctl;
  double* hist;
  int hist_slots;
  int* done_count;
};
// alpha Newton fused into the M-step: workgroup 0 runs it (lanes 0-1) beside the beta
// rows of the other workgroups; the control step (last workgroup) reads its alpha.
struct NewtonArgs {
  int enabled;            // 0: params[0..1] are left as they are
  int estimate;           // lda-c "alpha estimate" (else only the lgamma constant is refreshed)
  double num_docs;
  double* alpha_out;      // [1]
};
// ------------------------------------------------- fp64 block Gauss-Seidel ---
// lda-c-faithful E-step (lda_gs64.hip; kernels in gs_short.hip, gs_team.hip, gs_wteam.hip, gs_split.hip):
// everything in double, gamma / digamma refreshed
// after every chunk of W = ceil(n / U) words (U = gs_updates refreshes per sweep; a
// document of n <= U words is lda-c's literal per-word schedule).  The CPU oracle is
// csrc/native/lda_ref.cpp lda_inference(..., gs_updates).
constexpr int kGsUMax = 32;          // largest U with the chunk tables in LDS
constexpr int kGsUMaxWide = 4096;    // largest U at KS > 32 (chunk tables in the c*phi rows, gs_team GM)
enum GsVariant : int {
  kGsTiny = 0,     // TG lanes per document, literal schedule, n <= gs_tiny_max(KS)
  kGsTeam1 = 1,    // one wave per document
  kGsTeam4 = 2,    // one 4-wave workgroup per document
  kGsTeam8 = 3,    // one 8-wave workgroup per document (8 prefetched words per slot and chunk)
  kGsSmall = 4,    // 16 lanes per document: KS <= 32 tiny < n <= 64 words (register state); KS > 32 the
                   // one-wave range (gs_smallw, chunk tables in the c*phi rows)
  kGsChain = 5,    // KS > 32, U > 32: one wave per document, a topic per lane, rows of the next 8 words in
                   // flight (the planner routes chunks of W <= GSPlan.CHAIN_MAX_W = 2 words here:
                   // lda-c's per-word schedule, ops/hip.py wide_u_edges)
};
struct GSArgs {
  const int* doc_ptr;     // [D+1]
  const int* word_idx;    // [nnz]
  const float* counts;    // [nnz] (integer valued)
  const int* order;       // [n_items] documents of this launch
  int n_items;
  const double* beta;     // [V][KS] p(w|z) = exp(log_prob_w), word-major; 0 for padding topics
  int K;
  int gs_updates;         // U, 1 <= U <= gs_umax(KS)
  const double* params;   // {alpha, lgamma(K a) - K lgamma(a), VAR_MAX_ITER, VAR_CONVERGED, done, ...}
  double* gamma;          // [D][KS]
  double* cphi;           // [nnz][KS] c_n * phi_nk of the final sweep (sufficient-statistic input)
  double* lik;            // [D]
  double* alpha_ss;       // [D]
  int* iters;             // [D]
  // optional phase timer (scripts/bench_gs64.py --phases): workgroup 0, thread 0 of the team kernels
  // accumulates clock64() cycles into dbg[0..7]: word phase, slot reduction, barrier 1, topic phase,
  // barrier 2, sweep likelihood, final pass, chunks
  long long* dbg = nullptr;
  // optional staged rows (kGsTeam8 at KS <= 32, launch_gs_stage): item i's document has its beta rows
  // copied in document order to stage + stage_off[i] (double2 units), tiled [n/64][KS/2][64] so that a
  // wave's 64 consecutive words are 16-byte-contiguous per topic pair; stage_off[i] < 0: not staged
  const double* stage = nullptr;
  const long long* stage_off = nullptr;
  // optional chunk count sums (gs_wsteam): csum[i * kGsUMax + j] = sum of the counts of chunk j of item i's
  // document, built once per plan on the host (constants of the corpus); nullptr: the kernel sums the counts
  const double* csum = nullptr;
  // optional deferred final pass (gs_wsteam): when set, the workgroup of item i leaves the E of every chunk's
  // final sweep in et[(i * kGsUMax + j) * KS + k] and writes no c*phi rows; the suff-stats pass recomputes
  // them (launch_gs_suff64 with SuffRecompArgs)
  double* et = nullptr;
};
void launch_gs_estep(const GSArgs& a, int variant, int KS, hipStream_t s);
// stage[(t KS/2 + k) 64 + l] (double2) = beta row pair k of the word at corpus entry tile_ent[t] + l
// (l < tile_cnt[t], else 0): the staged rows of launch_gs_estep, filled after every M-step
void launch_gs_stage(const double* beta, const int* word_idx, const int* tile_ent, const int* tile_cnt, int n_tiles,
                     double* stage, int KS, const double* gate, hipStream_t s);   // gate: as gs_mstep
int gs_tiny_max(int KS);   // longest document of the kGsTiny kernel
int gs_umax(int KS);       // largest gs_updates the E-step accepts at row stride KS
int gs_split_umax(int KS); // largest gs_updates of the split kernel (KS > 32: kGsUMaxWide, else 32 / 64)
int gs_split_lds_umax(int KS);   // largest gs_updates with the chunk tables in LDS (64 at KS <= 52, else 32)
// One long document over s.seg_count[b] workgroups (8 waves each): every chunk is cut into
// that many word ranges whose partials are exchanged as tagged granules (2 per double,
// s.xchg = [2][n_blocks][2 (KS + 1)]); s.seg_words is unused.  Every segment of a launch
// must be co-resident: n_blocks <= gs_split_capacity(KS) (the host keeps a margin).
void launch_gs_split(const GSArgs& a, const SplitArgs& s, int KS, hipStream_t st);
int gs_split_capacity(int KS);

// class_word[w] = sum over w's CSC entries of cphi rows (fixed order, no atomics); part
// [nb][2 + KS] per-workgroup {lik slice, alpha_ss slice, column sums} for colsum_partials.
// Recompute mode (KS <= 32, et != nullptr): the row of CSC slot s is not loaded from cphi but computed as the
// longest-document kernel's final pass would have written it (gs_math.h cphi_row, bitwise the same): the beta
// row of the word, the chunk's final-sweep E at et[et_row[s] * KS] (GSArgs::et) and counts[csc_ent[s]].
struct SuffRecompArgs {
  const double* beta = nullptr;    // [V][KS]
  const double* et = nullptr;      // [n_items * kGsUMax][KS]
  const int* et_row = nullptr;     // [slots of csc_ent] item slot * kGsUMax + chunk of the entry
  const float* counts = nullptr;   // [nnz]
};
void launch_gs_suff64(const int* word_ptr, const int* csc_ent, const int* order, int n_heavy, int n_medium,
                      int n_light, const double* cphi, double* cw, double* part, const double* lik,
                      const double* ass, int lo, int hi, int KS, const double* gate, hipStream_t s,
                      const double* cw_base = nullptr,   // cw[w] = cw_base[w] + sum (nullable)
                      const SuffRecompArgs& rc = SuffRecompArgs());
// Staged rows refilled by the M-step launch itself (trailing workgroups): the next E-step's staged
// copies of the longest documents' beta rows (launch_gs_stage's layout) computed straight from cw and
// class_total, so no separate stage launch (and its inter-kernel gap) sits between the M-step and the
// longest-document kernel.  n_sets = 0: none.
struct StageFuseArgs {
  const int* word_idx = nullptr;
  const int* tile_ent[2] = {nullptr, nullptr};
  const int* tile_cnt[2] = {nullptr, nullptr};
  double* out[2] = {nullptr, nullptr};
  int n_tiles[2] = {0, 0};
  int n_sets = 0;
  int blocks = 0;     // set by the launcher
};
// fp64 M-step + alpha Newton (workgroup 0) + EM control (last workgroup) [+ staged rows]
void launch_gs_mstep_control(const double* cw, const double* class_total, double* beta, int V, int K, int KS,
                             const int* rows, int n_rows, const EMControlArgs& c, const NewtonArgs& nw,
                             hipStream_t s, StageFuseArgs sf = StageFuseArgs());
// lda-c random start on the device: cw[w][k] = 1/V + u(seed, k V + w) (k < K), 0 for padding;
// the same values as csrc/native random_ss (counter-based splitmix64).
void launch_init_random_ss(double* cw, int V, int K, int KS, unsigned long long seed, hipStream_t s);
void launch_gs_mstep(const double* cw, const double* class_total, double* beta, int V, int K, int KS,
                     const double* gate, hipStream_t s);

// ------------------------------------------------------------- reductions ---
// Deterministic reductions (reduce.hip).  gate (nullable): skip when *gate != 0.
// out[k] = sum_b part[b][k] (b in order), the second pass of the fused suff-stats.
void launch_colsum_partials(const double* part, int nb, int cols, double* out, const double* gate, hipStream_t s);
// out [K][V] = log(cw[v][k]) - log(ct[k]) (floor_v where cw == 0): the saved log beta in file order.
void launch_log_beta_t(const double* cw, int V, int K, int ld, const double* ct, double floor_v, double* out,
                       hipStream_t s);
// Sparse class_word exchange: out[rows[i]] = 0 + src_0 + src_1 + ... over row i's sources
// (CSR ptr/src; src >= 0: recv row, src < 0: the rank's own row own[rows[i]]), fp64, double2 granules.
void launch_rows_accumulate(const int* rows, const int* ptr, const int* src, const double* own, const double* recv,
                            double* out, int n_rows, int width, hipStream_t s);

// ---------------------------------------------------------------- scoring ---
struct ScoreArgs {
  const double* theta;    // [D][K] p(z|d)
  const double* phi;      // [V][K] p(w|z)
  int K;                  // topics summed (reference: 20)
  double dflt;            // value of the default vector used for misses
  const int* doc_a;       // [n] doc index or -1
  const int* word_a;      // [n] word index or -1
  const int* doc_b;       // [n] (flow: destination side) or nullptr
  const int* word_b;      // [n]
  int64_t n;
  double tol;
  double* score_a;        // [n]
  double* score_b;        // [n] or nullptr
  double* key;            // [n] min(score_a, score_b) (or score_a)
  uint8_t* flag;          // [n] key < tol
};
void launch_score_events(const ScoreArgs& a, hipStream_t s);

// Ensemble scoring (score_ensemble.hip): the mean over R members of score_events' member score, summed in
// member order and divided by (double)R; R = 1 is score_events bit for bit.
constexpr int kEnsembleMax = 64;   // largest R
struct EnsembleScoreArgs {
  const double* theta;    // [D][R][K] the members' p(z|d), interleaved per document
  const double* phi;      // [V][R][K] the members' p(w|z), interleaved per word
  int R;                  // members, 1 <= R <= kEnsembleMax
  int K;                  // topics summed
  double dflt;            // value of the default vector used for misses (every member)
  const int* doc_a;       // [n] doc index or -1
  const int* word_a;      // [n] word index or -1
  const int* doc_b;       // [n] (flow: destination side) or nullptr
  const int* word_b;      // [n] or nullptr, with doc_b
  int64_t n;              // 0 <= n < 2^31
  double tol;
  double* score_a;        // [n] ensemble score of side a
  double* score_b;        // [n] or nullptr, with doc_b
  double* key;            // [n] min(score_a, score_b) (or score_a)
  uint8_t* flag;          // [n] key < tol
  uint8_t* votes;         // [n] members whose own key (min of that member's side scores) is < tol
};
// max_blocks: cap on the workgroups (0: 8192); more events than the grid's lanes are grid-strided
void launch_score_ensemble(const EnsembleScoreArgs& a, int max_blocks, hipStream_t s);

// MAXRESULTS (select_lowest.hip): the rows that a stable ascending sort of the flagged keys puts first.
constexpr int kSelectTile = 2048;      // rows of one tile (256 threads x 8 rows); tiles are fixed and contiguous
constexpr int kSelectPasses = 6;       // radix digits of 11, 11, 11, 11, 11 and 9 bits, most significant first
constexpr int kSelectBins = 2048;      // histogram words per pass
constexpr int kSelectStateWords = 8;   // 32-bit words of a pass's state {prefix lo, hi, need, all, flagged, m, -, -}
struct SelectArgs {
  const double* key;      // [n]
  const uint8_t* flag;    // [n] non-zero: the row takes part
  int64_t n;              // 0 < n < 2^31
  unsigned limit;         // rows to select, >= 1
  unsigned ntiles;        // ceil(n / kSelectTile)
  unsigned* work;         // [select_work_words(n)]: kSelectPasses histograms, as many states, 2 counters per tile
  long long* out;         // [out_cap] the selected rows, ascending by row
  unsigned out_cap;       // >= min(limit, n)
};
size_t select_work_words(int64_t n);
// word of `work` that holds, once the launches are done, the number of flagged rows; the next word holds
// the number of selected rows m = min(limit, flagged)
int select_result_word();
// max_blocks: cap on the workgroups per launch (0: 2048); more tiles than that are grid-strided
void launch_select_lowest(const SelectArgs& a, int max_blocks, hipStream_t s);

// Host report (host_summary.hip): per document the number of scored sides, of sides under TOL, the lowest
// non-NaN score (as its order key) and the lowest side number 2 * event + side that attains it.
constexpr int kHostSummaryStats = 3;   // stats words: atomics issued for the counts, for min_key, for worst
struct HostSummaryArgs {
  const int* doc_a;            // [n] document row of side a, or -1
  const double* score_a;       // [n]
  const int* doc_b;            // [n] side b (flow: the destination) or nullptr
  const double* score_b;       // [n] or nullptr, with doc_b
  int64_t n;                   // events, 0 < n < 2^31 (a side number 2 n + 1 fits 32 bits)
  int64_t D;                   // documents, 0 < D < 2^31; a row outside [0, D) is a skipped side
  double tol;
  unsigned* events;            // [D] sides of the document
  unsigned* flagged;           // [D] of those, the sides with score < tol
  unsigned long long* min_key; // [D] lowest order key of the non-NaN scores; all-ones: none
  unsigned* worst;             // [D] lowest side number whose key is min_key; all-ones: none
  unsigned* skipped;           // [1] sides whose row is no document
  int fold;                    // non-zero: a wave folds the documents that repeat in it (0: one atomic per side)
  unsigned long long* stats;   // [kHostSummaryStats] or nullptr: atomics issued (measurement only)
};
// Starts the outputs at 0 / 0 / all-ones / all-ones / 0 (and stats at 0) itself, then two grid-stride passes.
// max_blocks: cap on the workgroups per launch (0: 2048)
void launch_host_summary(const HostSummaryArgs& a, int max_blocks, hipStream_t s);

// --explain (explain.hip).  group_rows_sum: row g of `out` is the sum of the table rows
// order[seg_start[g] .. seg_end[g]), column by column, in a fixed order: the segment is cut into blocks of
// `block` members, every block is summed from 0.0 in member order, the block sums are added from 0.0 in
// block order.  Plain rounded fp64 adds, no atomics.
struct GroupRowsArgs {
  const double* table;       // [V][W]
  const int* order;          // [V] table rows, every value in [0, V) (checked on the host)
  const int64_t* seg_start;  // [G] 0 <= seg_start <= seg_end <= V (checked on the host)
  const int64_t* seg_end;    // [G]
  const int64_t* blk_off;    // [G + 1] exclusive prefix sum of the segments' block counts ceil(len / block)
  int64_t G;                 // segments, 1 <= G < 2^31
  int64_t B;                 // blocks of all segments, blk_off[G], < 2^31
  int W;                     // doubles of a row
  int block;                 // members of a block, >= 1
  double* scratch;           // [B][W] block sums of the segments of more than one block
  double* out;               // [G][W]
};
// max_blocks: cap on the workgroups per launch (0: 4096)
void launch_group_rows_sum(const GroupRowsArgs& a, int max_blocks, hipStream_t s);

// explain_sides: per side the score s = theta[doc] . phi[word] as score_ensemble computes it, the same
// expression m_f with the row grow[i][f] of `gsum` in place of the phi row, cond[i][f] = s / m_f and why[i]
// the lowest f with the lowest non-NaN cond (255: none).  cond is NaN where word[i] < 0 or grow[i][f] < 0.
constexpr int kExplainMaxFields = 8;
struct ExplainArgs {
  const double* theta;   // [D][R][K]
  const double* phi;     // [V][R][K]
  const double* gsum;    // [Gtot][R][K] group sums of phi rows
  int R, K, F;           // 1 <= R <= kEnsembleMax, K >= 1, 1 <= F <= kExplainMaxFields
  double dflt;           // value of the default vector of a side without a document
  const int* doc;        // [n] theta row or -1
  const int* word;       // [n] phi row or -1
  const int* grow;       // [n][F] gsum row or -1
  int64_t n;             // 0 <= n < 2^31
  double* cond;          // [n][F]
  uint8_t* why;          // [n]
};
// max_blocks: cap on the workgroups (0: 8192)
void launch_explain_sides(const ExplainArgs& a, int max_blocks, hipStream_t s);

// --expect (expect.hip).  An item is a (document, word) pair and one explained field of the word: its group is the
// segment order[seg_start, seg_end) of phi rows.  p_v = the pair's score with member row v in place of its word, as
// score_ensemble computes it (doc < 0: the default vector for theta); s = p_word.  best = the member with the
// greatest p_v under IEEE > (a NaN never wins, ties to the lowest row, -0.0 and +0.0 tie), pbest its p_v, above =
// #{p_v > s}.  An item with seg_start < 0 (no word or no group) gets -1, NaN, -1; an empty segment -1, NaN, 0.
// Max, lowest-row tie-break and an integer count: the same bits for every grid and every block cut, no atomics.
struct ExpectArgs {
  const double* theta;       // [D][R][K]
  const double* phi;         // [V][R][K]
  int R, K;                  // 1 <= R <= kEnsembleMax, K >= 1
  double dflt;               // value of the default vector of an item without a document
  const int* order;          // [n_ord] phi rows, every value in [0, V) (checked on the host)
  const int* doc;            // [n] theta row or -1
  const int* word;           // [n] phi row, in [0, V) where seg_start >= 0
  const int64_t* seg_start;  // [n] -1: no value; else 0 <= seg_start <= seg_end <= n_ord (checked on the host)
  const int64_t* seg_end;    // [n]
  const int64_t* out_at;     // [n] where the item's results go in best / pbest / above
  const int64_t* blk_off;    // [n + 1] exclusive prefix sum of the items' block counts ceil(len / block)
  const int* blk_item;       // [B] the item of every block
  int64_t n;                 // items, 0 <= n < 2^31
  int64_t B;                 // blocks of all items, blk_off[n], < 2^31
  int block;                 // members of a block, >= 1
  double* part_p;            // [B] per-block pbest of the items of more than one block
  int* part_best;            // [B] per-block best
  int* part_above;           // [B] per-block above
  int* best;                 // [n]
  double* pbest;             // [n]
  int* above;                // [n]
};
enum ExpectPath : int {
  kExpectRegisters = 0,   // theta row in registers (the ladder of tail_common.h)
  kExpectGlobal = 1,      // theta row read from global memory at every member
};
int expect_theta_path(int R, int K);
// max_blocks: cap on the workgroups per launch (0: 65536)
void launch_expect_sides(const ExpectArgs& a, int max_blocks, hipStream_t s);

// --tail (tail_mass.hip).  For side i with doc[i] >= 0 and word[i] >= 0, over every row v of phi: p_v = the
// side's score with row v in place of its word, as score_ensemble computes it; s = p_word.  The rows are cut into
// nblk blocks of `block`; within a block, from 0.0 in row order, le_b += (p_v <= s ? p_v : 0.0) and tot_b += p_v;
// the block values are added from 0.0 in block order.  rarer = #{p_v < s}, ties = #{p_v == s}.  Any other side:
// NaN, NaN, -1, -1.  Plain rounded fp64 multiplies and adds, no atomics: the same bits for every grid.
enum TailPath : int {
  kTailRegisters = 0,   // theta row in registers (padded to a compiled width of at most 100 doubles)
  kTailLdsTheta = 1,    // theta rows in LDS (R K <= 256)
  kTailDirect = 2,      // rows read from global memory
};
struct TailArgs {
  const double* theta;   // [D][R][K]
  const double* phi;     // [V][R][K]
  int R, K;              // 1 <= R <= kEnsembleMax, K >= 1
  int64_t V;             // rows of phi, 0 <= V < 2^31
  const int* doc;        // [n] theta row or -1 (bounds checked on the host)
  const int* word;       // [n] phi row or -1
  int64_t n;             // 0 <= n < 2^31
  int64_t block;         // rows of a block, >= 1
  int64_t nblk;          // ceil(V / block)
  double* scratch;       // nblk * n * 24 bytes: [2][nblk][n] doubles (le_b, tot_b), then [2][nblk][n] ints
  double* le;            // [n]
  double* tot;           // [n]
  int* rarer;            // [n]
  int* ties;             // [n]
};
// max_blocks: cap on the workgroups per launch (0: 65536)
void launch_tail_mass(const TailArgs& a, int max_blocks, hipStream_t s);
int tail_theta_path(int R, int K);   // the TailPath the launch takes at this row shape
// --tail-tol (tail_docs.hip): the same four values, bit for bit, for pairs sorted by document -- doc non-decreasing,
// doc >= 0 and word >= 0 (checked on the host) -- with p_v evaluated once per (document of a tile of 256 pairs,
// row) instead of once per pair.  Only where tail_theta_path(R, K) == kTailRegisters; any other width throws.
void launch_tail_docs(const TailArgs& a, int max_blocks, hipStream_t s);

// --peers (peers.hip).  Rows of theta are W = R K doubles.  L(q, p) = the L1 distance of rows q and p: from 0.0, for
// j = 0 .. W - 1 in order, t = theta[q][j] - theta[p][j] (one rounded subtraction), acc = acc + |t| (one rounded add).
// For query i the N candidates p != query[i] lowest in the total order (L, p), a NaN L never among them, in that
// order: rows[i][0 .. count[i]) and dist[i][..]; the slots past count[i] hold -1 and +inf.  The top N of a set under
// a total order does not depend on how the set is cut: the same bits for every grid, block and batch, no atomics.
constexpr int kPeersMax = 16;   // largest N
enum PeerPath : int {
  kPeerRegisters = 0,   // the query's row in registers (padded to a compiled width of at most 100 doubles)
  kPeerDirect = 1,      // both rows read from global memory
};
struct PeerArgs {
  const double* theta;   // [D][W]
  int W;                 // doubles of a row, >= 1
  int64_t D;             // rows, 0 <= D < 2^31
  const int* query;      // [n] rows, 0 <= query[i] < D (bounds checked on the host)
  int64_t n;             // 0 <= n < 2^31
  int N;                 // 1 <= N <= kPeersMax
  int64_t block;         // candidate rows of a block, >= 1
  int64_t nblk;          // ceil(D / block)
  double* scratch;       // nblk * n * N * 12 bytes: [nblk][N][n] doubles (L), then [nblk][N][n] ints (row)
  int* rows;             // [n][N]
  double* dist;          // [n][N]
  int* count;            // [n]
};
// max_blocks: cap on the workgroups per launch (0: 65536)
void launch_peer_topn(const PeerArgs& a, int max_blocks, hipStream_t s);
int peer_theta_path(int R, int K);   // the PeerPath the launch takes at this row shape

// --topic-report (topic_report.hip).  column_topn: per column j of table [rows][W] the N rows first in the total
// order (value descending under IEEE >, row ascending) -- equal values, -0.0 and +0.0 among them, go to the lower
// row, a NaN never enters: out_rows[j][0 .. out_count[j]) and out_vals[j][..]; the slots past the count hold -1 and
// -inf.  The top N of a set under a total order does not depend on how the set is cut: the same bits for every
// grid, block and batch, no atomics.  One launch handles the columns c0 .. c0 + wb - 1.
constexpr int kTopicReportMax = 32;       // largest N
constexpr int64_t kTopicRowsMax = ((int64_t)1 << 31) - 65536;   // largest table of column_topn
constexpr int kTopicMergeGroup = 64;      // blocks whose lists one workgroup of pass 2 merges
constexpr int kTopicColumnsMax = 8192;    // largest R K of row_dominant (its LDS histogram: 32 KiB)
struct TopnArgs {
  const double* table;   // [rows][ld], the first W of a row its values
  int64_t rows;          // 1 <= rows <= kTopicRowsMax
  int W;                 // doubles of a row, >= 1
  int64_t ld;            // doubles from a row to the next, >= W (a strided sample of a table: a multiple of W)
  const double* tau;     // [W] or null: pass 1 skips a value below tau[column] -- a lower bound of the column's
                         // N-th value (that of a subset of the rows), so nothing listed is skipped
  int c0, wb;            // the launch's columns: 0 <= c0, 1 <= wb, c0 + wb <= W
  int N;                 // 1 <= N <= kTopicReportMax
  int64_t block;         // rows of a block, >= 1
  int64_t nblk;          // ceil(rows / block)
  double* scratch;       // nblk * N * wb * 12 bytes: [nblk][N][wb] doubles (value), then [nblk][N][wb] ints (row)
  double* scratch2;      // nblk > kTopicMergeGroup: the same layout for topic_merge_groups(nblk) blocks; else unused
  int* out_rows;         // [W][N]
  double* out_vals;      // [W][N]
  int* out_count;        // [W]
};
// max_blocks: cap on the workgroups per launch (0: 65536)
void launch_column_topn(const TopnArgs& a, int max_blocks, hipStream_t s);
int topic_merge_groups(int64_t nblk);   // lists of the second scratch (0: pass 2 has one level)
int topic_threads(int N);           // lanes of a workgroup at this N (the lists are N x lanes x 12 bytes of LDS)
int topic_groups(int N, int wb);    // row sub-groups of a workgroup at this N and column count (1: a lane per column)

// row_dominant: arg[row][r] = the first k attaining the maximum of table[row][r][0 .. K) (a NaN never wins; -1: all
// NaN); counts[r][k] += the rows whose arg is k (integer atomics; the caller zeroes counts).
struct DominantArgs {
  const double* table;          // [rows][R][K]
  int64_t rows;                 // rows R < 2^31
  int R, K;                     // R K <= kTopicColumnsMax
  int* arg;                     // [rows][R]
  unsigned long long* counts;   // [R][K]
};
void launch_row_dominant(const DominantArgs& a, int max_blocks, hipStream_t s);

// topic_sides: per side (doc, word), over j = 0 .. R K - 1 in order p_j = theta[doc][j] * phi[word][j] (one rounded
// product): col = the first j with the greatest p_j (a NaN never wins), resp = p* / (s * (double)R) with s the
// side's score as score_ensemble.hip computes it, host_share = theta[doc][col], host_topic = the first k attaining
// the maximum of theta[doc][col / K][.].  A side with doc < 0, word < 0 or NaN products only: -1, NaN, NaN, -1 --
// so the scorers' default vector of a miss never enters, and the launch takes no default value.
struct TopicSidesArgs {
  const double* theta;   // [D][R][K]
  const double* phi;     // [V][R][K]
  int R, K;
  const int* doc;        // [n] theta rows or -1 (bounds checked on the host)
  const int* word;       // [n] phi rows or -1
  int64_t n;             // 0 <= n < 2^31
  int* col;              // [n]
  double* resp;          // [n]
  double* host_share;    // [n]
  int* host_topic;       // [n]
};
void launch_topic_sides(const TopicSidesArgs& a, int max_blocks, hipStream_t s);

// --topic-match (column_l1.hip).  column_l1: C[a][b] = the sum over the M pairs of |A[ia[m]][a] - B[ib[m]][b]| (ia
// and ib null: the identity).  The pairs are cut into blocks of `block`; a block is summed from 0.0 in pair order
// (one rounded subtraction, its magnitude, one rounded add), the block sums are added from 0.0 in block order.  A
// NaN difference makes the sum NaN.  One launch handles the blocks b0 .. b0 + nb - 1 and continues C from the
// batch before it (first: from 0.0): the same sequence of adds for every batch size, no atomics.
constexpr int kColumnL1WidthMax = 1 << 15;   // largest Wa / Wb
struct ColumnL1Args {
  const double* A;       // [Va][Wa]
  const double* B;       // [Vb][Wb]
  int64_t Va, Vb;
  int Wa, Wb;            // 1 .. kColumnL1WidthMax
  const int64_t* ia;     // [M] rows of A, or null with ib: pair m is row m of both (bounds checked on the host)
  const int64_t* ib;     // [M] rows of B
  int64_t M;             // pairs, 0 <= M < 2^40
  int64_t block;         // pairs of a block, 1 .. 2^31 - 1
  int64_t b0, nb;        // the launch's blocks: 0 <= b0, b0 + nb <= ceil(M / block)
  double* scratch;       // [nb][Wa][Wb]
  double* C;             // [Wa][Wb]
  int first;             // 1: the sums start at 0.0; 0: they continue from C
};
// max_blocks: cap on the workgroups per launch (0: 65536)
void launch_column_l1(const ColumnL1Args& a, int max_blocks, hipStream_t s);
int column_l1_tile(int W);   // columns of a tile along a side of W columns (32 or 64)

// --holdout (holdout.hip).  holdout_draw: t[e] = the tokens j of CSR entry e, 0 <= j < counts[e], with
// splitmix64(key ^ (base[e] + j)) >> 11 < thr -- integers only, so t depends on nothing but (key, thr, corpus).
// An entry of at most lane_tokens tokens is drawn by one lane; a longer one is cut into chunks of
// 64 * lane_tokens tokens, a wave per chunk (lanes stride over the tokens, ballot popcount per step), and the
// chunk counts of an entry of several chunks are added with an integer atomic.
struct HoldoutDrawArgs {
  const int64_t* base;        // [nnz] exclusive prefix sum of counts
  const int64_t* counts;      // [nnz] >= 0 (checked on the host)
  const int64_t* chunk_off;   // [nnz + 1] exclusive prefix sum of the chunks of the entries over lane_tokens
  int64_t nnz;                // entries, 0 <= nnz < 2^31
  int64_t chunks;             // chunk_off[nnz], < 2^31
  unsigned long long key;     // splitmix64(seed ^ salt), from the host
  unsigned long long thr;     // 0 < thr <= 2^52
  int lane_tokens;            // >= 1
  int64_t* t;                 // [nnz]
};
// max_blocks: cap on the workgroups per launch (0: 8192)
void launch_holdout_draw(const HoldoutDrawArgs& a, int max_blocks, hipStream_t s);

// holdout_entries: ll[e] = (double)t[e] * log_rn(theta[doc[e]] . phi[word[e]]) where t[e] > 0 and
// seen[word[e]] != 0, else 0.0.  The dot is score_events' (score_dot.h); log_rn is a natural log of correctly
// rounded fp64 operations in a fixed order (ops/reference.py log_rn is its torch twin).
struct HoldoutEntriesArgs {
  const double* theta;   // [D][K]
  const double* phi;     // [V][K]
  int K;                 // >= 1
  const int* doc;        // [n] theta row of the entry, in [0, D) (checked on the host)
  const int* word;       // [n] phi row of the entry, in [0, V) (checked on the host)
  const int64_t* t;      // [n] held-out tokens of the entry
  const uint8_t* seen;   // [V] non-zero: the word has a training entry
  int64_t n;             // 0 <= n < 2^31
  double* ll;            // [n]
};
// max_blocks: cap on the workgroups (0: 8192)
void launch_holdout_entries(const HoldoutEntriesArgs& a, int max_blocks, hipStream_t s);

// Byte entropy of every string of a batch (string_entropy.hip): out[i] = (t[n] - sum_b t[c_b]) / n over the
// bytes [offsets[i], offsets[i + 1]) of `bytes`, t = table (c log2 c, host-built), 0 for n <= 1.
struct StringEntropyArgs {
  const uint8_t* bytes;     // [offsets[n]] at any alignment; nothing outside a string's range is loaded
  const int64_t* offsets;   // [n + 1] non-decreasing, inside the bytes buffer (checked on the host)
  int64_t n;                // strings
  const double* table;      // [table_len], table_len > the longest string's length
  int64_t table_len;
  double* out;              // [n]
};
// max_blocks: cap on the workgroups (0: 4096); more strings than the grid's waves are grid-strided
void launch_string_entropy(const StringEntropyArgs& a, int max_blocks, hipStream_t s);

// ------------------------------------------------------------ flow words ---
struct FlowWordArgs {
  const double* hour;      // [n] col 4
  const double* minute;    // [n] col 5
  const double* second;    // [n] col 6
  const double* port_a;    // [n] col 10 (reference variable name: dport)
  const double* port_b;    // [n] col 11 (reference variable name: sport)
  const double* ipkt;      // [n] col 16
  const double* ibyt;      // [n] col 17
  const double* time_cuts; // [n_time_cuts]
  const double* ibyt_cuts;
  const double* ipkt_cuts;
  int n_time_cuts, n_ibyt_cuts, n_ipkt_cuts;
  int64_t n;
  double* time_out;        // [n] col 27
  int8_t* time_bin;        // [n]
  int8_t* ibyt_bin;        // [n]
  int8_t* ipkt_bin;        // [n]
  double* word_port;       // [n]
  int8_t* p_case;          // [n]
  int8_t* src_prefix;      // [n] 1 if src word carries "-1_"
  int8_t* dst_prefix;      // [n]
};
void launch_flow_words(const FlowWordArgs& a, hipStream_t s);

// bins[i*ncols + c] = #{cut in cuts_c : value_c[i] > cut}   (generic binning)
void launch_bin_columns(const double* const* values, const double* const* cuts, const int* ncuts,
                        int ncols, int64_t n, int8_t* bins, hipStream_t s);

// ------------------------------------------------------- engine construction ---
// csc_ent[s] = perm[s] (the stable sort's int64 permutation, narrowed) and csc_doc[s] = the document whose
// [doc_ptr[d], doc_ptr[d + 1]) holds that entry (corpus_plan.hip).
void launch_csc_docs(const long long* perm, const int* doc_ptr, int D, int nnz, int* csc_ent, int* csc_doc,
                     hipStream_t s);

// Early / late partition of the CSC (corpus_plan.hip): slots whose document has late[d] != 0 go to ce_late, the
// others to ce_early, slot order kept; wp_late[w] = late slots ahead of word_ptr[w], wp_early[w] the others.
constexpr int kCscPartTile = 2048;   // slots per workgroup: tile_sum holds ceil(nnz / kCscPartTile) ints
struct CscPartArgs {
  const int* csc_ent;    // [nnz]
  const int* csc_doc;    // [nnz]
  const int* word_ptr;   // [V + 1]
  const uint8_t* late;   // [D]
  int nnz, V, D;
  int n_early, n_late;   // the two sides' slots (n_early + n_late = nnz), from the host plan: bounds of the lists
  int* ce_early;         // [n_early]
  int* ce_late;          // [n_late]
  int* wp_early;         // [V + 1]
  int* wp_late;          // [V + 1]
  int* tile_sum;         // scratch [max(1, ceil(nnz / kCscPartTile))]
  int* before;           // scratch [nnz + 1]: late slots ahead of each slot
  // deferred final pass (nullptr: none): et_row[i] of late slot i = et_base[d] + min((entry - et_s0[d]) /
  // et_w[d], umax - 1) with d the slot's document
  int* et_row;           // [n_late]
  const int* et_s0;      // [D]
  const int* et_w;       // [D]
  const int* et_base;    // [D]
  int umax;
};
void launch_csc_partition(const CscPartArgs& a, hipStream_t s);

}  // namespace oni
