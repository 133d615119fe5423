// --holdout: document-completion held-out perplexity (models/lda/holdout.py; twins: ops/reference.py
// holdout_draw, log_rn, holdout_entries).
//
// The split.  Token j of CSR entry e has the global index g = base[e] + j (base: the exclusive prefix sum of the
// counts) and is held out iff splitmix64(key ^ g) >> 11 < thr: a counter-based draw, compared as integers, so the
// split depends on nothing but (key, thr, corpus) -- not on the grid, and not on which of the two paths an entry
// took.  Counts are skewed (feedback rows carry DUPFACTOR weights), so the work is cut by tokens:
//   holdout_draw_lanes   one lane per entry, grid-stride: an entry of at most L = lane_tokens tokens is drawn by
//                        its lane; a longer one gets t = 0 here.
//   holdout_draw_waves   an entry over L tokens is cut into chunks of 64 L tokens, a wave per chunk, grid-stride:
//                        the lanes stride over the chunk's tokens, every step's hits are counted with one ballot
//                        popcount.  An entry of one chunk is stored, the chunks of a longer one are added with an
//                        integer atomic (any order, the same integer).  No lane loops over more than L tokens.
//
// The evaluation.  One lane per entry, grid-stride: ll = (double)t * log_rn(theta_d . phi_w) for an entry with
// held-out tokens whose word the training corpus has, else 0.0.  The dot is score_events' (score_dot.h).
// log_rn is a natural log built from correctly rounded fp64 operations only, in a fixed order, so that it has an
// exact torch twin: frexp, one division, a Horner polynomial in ((m - 1) / (m + 1))^2 of rounded products and
// sums, ln 2 in two parts.  (The engine's flog goes through v_rcp_f64, which has no host twin.)  The sums over a
// document's entries and over the documents are group_rows_sum's (explain.hip).
#include <stdexcept>
#include <string>

#include "../common/splitmix64.h"
#include "common.h"
#include "kernels.h"
#include "score_dot.h"

namespace oni {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

__device__ __forceinline__ bool drawn(const HoldoutDrawArgs& a, unsigned long long g) {
  return (splitmix64(a.key ^ g) >> 11) < a.thr;
}

__global__ __launch_bounds__(kThreads) void holdout_draw_lanes_kernel(HoldoutDrawArgs a) {
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < a.nnz; e += (int64_t)gridDim.x * kThreads) {
    const int64_t c = a.counts[e];
    int64_t t = 0;
    if (c <= a.lane_tokens) {
      const unsigned long long g0 = (unsigned long long)a.base[e];
      for (int j = 0; j < (int)c; ++j) t += drawn(a, g0 + (unsigned long long)j) ? 1 : 0;
    }
    a.t[e] = t;   // an entry over lane_tokens: 0, the chunks' counts follow (holdout_draw_waves_kernel)
  }
}

__global__ __launch_bounds__(kThreads) void holdout_draw_waves_kernel(HoldoutDrawArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t span = (int64_t)64 * a.lane_tokens;   // tokens of a chunk
  // b is the same in the 64 lanes of a wave: every branch on it is wave-uniform, __ballot sees all lanes
  for (int64_t b = (int64_t)blockIdx.x * kWaves + threadIdx.x / 64; b < a.chunks; b += (int64_t)gridDim.x * kWaves) {
    // the chunk's entry: the last e with chunk_off[e] <= b (entries without chunks share their successor's offset)
    int64_t lo = 0, hi = a.nnz;
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (a.chunk_off[mid] <= b) lo = mid; else hi = mid;
    }
    const int64_t e = lo, b0 = a.chunk_off[e];
    const int64_t j0 = (b - b0) * span;
    const int64_t rem = a.counts[e] - j0;             // > 0: tokens from j0 on
    const unsigned long long g0 = (unsigned long long)(a.base[e] + j0);
    unsigned cnt = 0;
    for (int i = 0; i < a.lane_tokens && (int64_t)i * 64 < rem; ++i) {
      const int64_t j = (int64_t)i * 64 + lane;
      const bool hit = j < rem && drawn(a, g0 + (unsigned long long)j);
      cnt += (unsigned)__popcll(__ballot(hit));
    }
    if (lane == 0) {
      if (a.chunk_off[e + 1] - b0 == 1)
        a.t[e] = (int64_t)cnt;
      else
        atomicAdd(reinterpret_cast<unsigned long long*>(a.t + e), (unsigned long long)cnt);
    }
  }
}

// ln y for a positive normal or subnormal double; every operation correctly rounded, none contracted.
__device__ __forceinline__ double log_rn(double y) {
#pragma clang fp contract(off)
  constexpr double c[11] = {2.0 / 3.0,  2.0 / 5.0,  2.0 / 7.0,  2.0 / 9.0,  2.0 / 11.0, 2.0 / 13.0,
                            2.0 / 15.0, 2.0 / 17.0, 2.0 / 19.0, 2.0 / 21.0, 2.0 / 23.0};
  int e;
  double m = frexp(y, &e);                  // m in [0.5, 1)
  if (m < 0.70710678118654752) {
    m = m + m;
    e = e - 1;
  }
  const double num = m - 1.0, den = m + 1.0;
  const double f = num / den;
  const double s = f * f;
  double P = c[10];
#pragma unroll
  for (int i = 9; i >= 0; --i) {
    const double q = P * s;                 // rounded product, then rounded sum
    P = q + c[i];
  }
  const double fs = f * s;
  const double a = fs * P;
  const double ff = f + f;
  double r = a + ff;
  const double ed = (double)e;
  const double lo = ed * 1.90821492927058770002e-10;
  r = lo + r;
  const double hi = ed * 6.93147180369123816490e-01;
  return hi + r;
}

__global__ __launch_bounds__(kThreads) void holdout_entries_kernel(HoldoutEntriesArgs a) {
#pragma clang fp contract(off)
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kThreads) {
    const int64_t t = a.t[i];
    const int w = a.word[i];
    double ll = 0.0;
    if (t > 0 && a.seen[w]) {
      const double s = score_one(a.theta, a.phi, a.K, 0.0, a.doc[i], w);
      const double lg = log_rn(s);
      ll = (double)t * lg;
    }
    a.ll[i] = ll;
  }
}

int64_t grid_of(int64_t items, int per_block, int max_blocks) {
  int64_t blocks = (items + per_block - 1) / per_block;
  const int64_t cap = max_blocks > 0 ? max_blocks : 8192;
  return blocks > cap ? cap : blocks;
}

}  // namespace

void launch_holdout_draw(const HoldoutDrawArgs& a, int max_blocks, hipStream_t s) {
  if (a.nnz < 0 || a.nnz >= ((int64_t)1 << 31) || a.chunks < 0 || a.chunks >= ((int64_t)1 << 31))
    throw std::runtime_error("holdout_draw: nnz or chunks outside 0 .. 2^31 - 1");
  if (a.lane_tokens < 1 || a.lane_tokens > (1 << 20)) throw std::runtime_error("holdout_draw: lane_tokens outside 1 .. 2^20");
  if (a.thr == 0 || a.thr > (1ull << 52)) throw std::runtime_error("holdout_draw: thr outside 1 .. 2^52");
  if (max_blocks < 0) throw std::runtime_error("holdout_draw: max_blocks < 0");
  if (a.nnz == 0) return;
  if (!a.base || !a.counts || !a.chunk_off || !a.t) throw std::runtime_error("holdout_draw: null buffer");
  hipLaunchKernelGGL(holdout_draw_lanes_kernel, dim3((unsigned)grid_of(a.nnz, kThreads, max_blocks)), dim3(kThreads),
                     0, s, a);
  ONI_HIP_CHECK(hipGetLastError());
  if (a.chunks > 0) {
    hipLaunchKernelGGL(holdout_draw_waves_kernel, dim3((unsigned)grid_of(a.chunks, kWaves, max_blocks)),
                       dim3(kThreads), 0, s, a);
    ONI_HIP_CHECK(hipGetLastError());
  }
}

void launch_holdout_entries(const HoldoutEntriesArgs& a, int max_blocks, hipStream_t s) {
  if (a.n < 0 || a.n >= ((int64_t)1 << 31)) throw std::runtime_error("holdout_entries: n outside 0 .. 2^31 - 1");
  if (a.K < 1) throw std::runtime_error("holdout_entries: K < 1");
  if (max_blocks < 0) throw std::runtime_error("holdout_entries: max_blocks < 0");
  if (a.n == 0) return;
  if (!a.theta || !a.phi || !a.doc || !a.word || !a.t || !a.seen || !a.ll)
    throw std::runtime_error("holdout_entries: null buffer");
  hipLaunchKernelGGL(holdout_entries_kernel, dim3((unsigned)grid_of(a.n, kThreads, max_blocks)), dim3(kThreads), 0,
                     s, a);
  ONI_HIP_CHECK(hipGetLastError());
}

}  // namespace oni
