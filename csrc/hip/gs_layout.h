// Lane layouts and word-phase helpers shared by two or more families of the fp64 block Gauss-Seidel E-step
// (gs_short.hip gs_smallw, gs_team.hip, gs_split.hip) and by the suff-stats gather (lda_gs64.hip gs_suff64).
// A helper that only one family uses lives in that family's file.
#pragma once
#include "common.h"
#include "gs_math.h"
#include "kernels.h"

namespace oni {
namespace gs {

constexpr int tg_of(int KS) { return KS <= 32 ? 4 : (KS <= 64 ? 8 : 16); }
constexpr int kpl_of(int KS) { return (KS + tg_of(KS) - 1) / tg_of(KS); }

// topic of a lane's i-th value in the team layouts (TeamShape::PAIR: consecutive pairs)
template <int TG, bool PAIR>
__device__ __forceinline__ int tk(int q, int i) { return PAIR ? 2 * q + (i & 1) + 2 * TG * (i >> 1) : q + TG * i; }

// a word's KPL values of this lane at constant offsets.  The row's last, partial topic group: lanes past KS
// re-read the group's last valid topic (the cache line a valid lane already fetches), so a row gather touches
// only the row's own lines -- reading on into the next row touched ~1.75 extra 128-B lines per 800-B row at
// KS = 100 (8.75 instead of 7).  Measured at 100 M events: team8 0.147 -> 0.141 ns per word-sweep (-4 %), team4
// -1 % (profiles/r6p_team4_rmax.md): these gathers are not bound by the lines they fetch.
// Those lanes' values only ever meet E = 0 or are never stored (every consumer guards tk < KS).
template <int KS, int KPL, int TG, bool PAIR>
__device__ __forceinline__ void load_row(const double* __restrict__ beta, int w, int q, double (&b)[KPL]) {
  const double* rb = beta + (size_t)w * KS;
  if constexpr (PAIR) {
    static_assert(KS % 2 == 0, "pair rows: even KS");
    const dvec2* r = reinterpret_cast<const dvec2*>(rb + 2 * q);
#pragma unroll
    for (int ii = 0; ii < KPL / 2; ++ii) {
      dvec2 v;
      if (2 * TG * (ii + 1) <= KS) {
        v = r[TG * ii];
      } else {
        const int last = (KS - 2 * TG * ii) / 2 - 1;     // the group's last valid pair (compile-time)
        v = *reinterpret_cast<const dvec2*>(rb + 2 * TG * ii + 2 * min(q, last));
      }
      b[2 * ii] = v.x;
      b[2 * ii + 1] = v.y;
    }
  } else {
    const double* brow = rb + q;
#pragma unroll
    for (int i = 0; i < KPL; ++i) {
      if (TG * (i + 1) <= KS)
        b[i] = brow[TG * i];
      else
        b[i] = rb[TG * i + min(q, KS - TG * i - 1)];
    }
  }
}

// Threads of a document team exchange data through LDS only (lds_barrier keeps the
// next chunk's prefetched global loads in flight across the barrier).
template <int NW>
__device__ __forceinline__ void team_sync() {
  if constexpr (NW == 1)
    wave_lds_sync();
  else
    lds_barrier();
}

template <int KS, int NW>
struct TeamShape {
  static constexpr int DPB = (NW == 1 && KS <= 32) ? 4 : 1;   // documents per workgroup
  static constexpr int NTD = NW * 64;                          // threads per document
  static constexpr int TG = tg_of(KS);
  // PAIR (TG >= 8, KS > 32): a lane holds topic PAIRS 2q, 2q + 1 (+ 2 TG per pair) and loads each pair with one
  // 16-byte load -- half the load instructions of one topic per 8-byte lane; the row gathers of the K = 100
  // team kernels are issue-bound (a chunk's prefetch issue 2.5-4.5 k cycles, profiles/r5_k100.md)
  static constexpr bool PAIR = TG >= 8;
  static constexpr int KPL = PAIR ? 2 * ((KS + 2 * TG - 1) / (2 * TG)) : kpl_of(KS);
  static constexpr int NSW = 64 / TG;                          // word slots per wave
  static constexpr int LSW = ilog2(NSW);
  static constexpr int NS = NW * NSW;                          // word slots per document
  static constexpr int TO = (KS + NTD - 1) / NTD;              // topics owned per thread
  // prefetched words per slot per chunk (even).  The 4-wave team keeps one round at KS > 32 too, although it runs
  // 2 waves per SIMD at any VGPR count up to 256 (171 with one round): 2 or 3 rounds (205 / 230 VGPRs) measured
  // slower on the K = 100 shard (team4 bucket 5.89 ms at 1, 6.01 at 2, 6.28 at 3; profiles/r6p_team4_rmax.md)
  static constexpr int RMAX = NW >= 8 ? (KPL <= 5 ? 8 : 4) : 1;
};

// N words of the word phase, interleaved (independent dependency chains): P = sum_k E_k b_k over
// the TG lanes of each slot, r = c / P, acc += r b, lw += c log P.  A word with c == 0 (no word in
// that round) contributes nothing (its P is replaced by 1 before the reciprocal).
template <int N, int KPL, int LSW, bool TAB = false>
__device__ __forceinline__ void word_steps(const double (&E)[KPL], const double (*b)[KPL], const double* c,
                                           double (&acc)[KPL], double& lw, const dvec2* tab = nullptr) {
  double P[N];
#pragma unroll
  for (int u = 0; u < N; ++u) {
    double p0 = 0.0, p1 = 0.0;
#pragma unroll
    for (int i = 0; i < KPL; i += 2) p0 = fma(E[i], b[u][i], p0);
#pragma unroll
    for (int i = 1; i < KPL; i += 2) p1 = fma(E[i], b[u][i], p1);
    P[u] = bits_sum<LSW, 6>(p0 + p1);
  }
#pragma unroll
  for (int u = 0; u < N; ++u) {
    const double Pu = c[u] > 0.0 ? P[u] : 1.0;
    const double r = c[u] * drcp(Pu);
    lw = fma(c[u], TAB ? flog_t(Pu, tab) : flog(Pu), lw);
#pragma unroll
    for (int i = 0; i < KPL; ++i) acc[i] = fma(r, b[u][i], acc[i]);
  }
}

// RMAX streamed words of one slot (p0, p0 + NS, ...; past `end` counts 0 and re-reads a valid row):
// ids, then rows, then the word steps, so a batch costs about one gather latency
template <int RMAX, int KS, int KPL, int TG, int LSW, bool PAIR, bool TAB = false>
__device__ __forceinline__ void stream_batch(const double* __restrict__ beta, const int* __restrict__ wrow,
                                             const float* __restrict__ crow, int p0, int end, int NS, int q,
                                             const double (&E)[KPL], double (&b)[RMAX][KPL], double (&acc)[KPL],
                                             double& lw, const dvec2* tab = nullptr) {
  int w[RMAX];
  double c[RMAX];
#pragma unroll
  for (int r = 0; r < RMAX; ++r) {
    const int p = p0 + r * NS;
    const int pc = min(p, end - 1);
    w[r] = wrow[pc];
    c[r] = p < end ? (double)crow[pc] : 0.0;
  }
#pragma unroll
  for (int r = 0; r < RMAX; ++r) load_row<KS, KPL, TG, PAIR>(beta, w[r], q, b[r]);
  word_steps<RMAX, KPL, LSW, TAB>(E, b, c, acc, lw, tab);
}

// the streamed tail of one slot: full batches while >= 2 rounds remain, the last round alone (a
// lone word in a full batch paid RMAX rows and word steps; measured on the split kernel)
template <int RMAX, int KS, int KPL, int TG, int LSW, bool PAIR, bool TAB = false>
__device__ __forceinline__ void stream_tail(const double* __restrict__ beta, const int* __restrict__ wrow,
                                            const float* __restrict__ crow, int p0, int end, int NS, int q,
                                            const double (&E)[KPL], double (&b)[RMAX][KPL], double (&acc)[KPL],
                                            double& lw, const dvec2* tab = nullptr) {
  int p = p0;
  if (p + NS < end) {
    // the ids of batch i + 1 load while batch i's rows are in flight: a batch then waits one memory latency
    // (its rows), not two (ids, then rows)
    int w[RMAX];
    double c[RMAX];
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
      const int pr = p + r * NS;
      const int pc = min(pr, end - 1);
      w[r] = wrow[pc];
      c[r] = pr < end ? (double)crow[pc] : 0.0;
    }
    for (; p + NS < end; p += RMAX * NS) {
#pragma unroll
      for (int r = 0; r < RMAX; ++r) load_row<KS, KPL, TG, PAIR>(beta, w[r], q, b[r]);
      double cb[RMAX];
      const int pn = p + RMAX * NS;
#pragma unroll
      for (int r = 0; r < RMAX; ++r) {
        cb[r] = c[r];
        const int pr = pn + r * NS;
        const int pc = max(0, min(pr, end - 1));
        w[r] = wrow[pc];
        c[r] = pr < end ? (double)crow[pc] : 0.0;
      }
      word_steps<RMAX, KPL, LSW, TAB>(E, b, cb, acc, lw, tab);
    }
  }
  if (p < end) {
    double b1[1][KPL];
    stream_batch<1, KS, KPL, TG, LSW, PAIR, TAB>(beta, wrow, crow, p, end, NS, q, E, b1, acc, lw, tab);
  }
}

}  // namespace gs
}  // namespace oni
