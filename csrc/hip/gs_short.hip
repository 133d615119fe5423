// fp64 block Gauss-Seidel E-step, the short-document kernels: a few lanes or one wave per document, no
// workgroup barrier (chunk algebra and schedule: header of lda_gs64.hip).
//   gs_tiny   TG lanes per document (KPL = KS / TG topics per lane), n <= NMAX words, literal per-word
//             schedule; the per-word contributions C[n][.] live in VGPRs.
//   gs_small  16 lanes per document, KS <= 32, register state.
//   gs_chain  one wave per document, a topic per lane: lda-c's per-word schedule (U > 32).
//   gs_smallw 16 lanes per document at KS > 32, chunk tables in the document's own c*phi rows.
#include <stdexcept>
#include <string>

#include "common.h"
#include "gs_families.h"
#include "gs_layout.h"
#include "gs_math.h"
#include "kernels.h"

namespace oni {
namespace gs {

// tiny kernel: wider topic groups than the team kernels (fewer topics, hence fewer
// digamma/exp chains and queue registers per lane)
constexpr int tiny_tg(int KS) { return KS <= 32 ? 8 : 16; }
constexpr int tiny_kpl(int KS) { return (KS + tiny_tg(KS) - 1) / tiny_tg(KS); }
constexpr int tiny_max(int KS) { return tiny_kpl(KS) <= 4 ? 8 : 4; }

// ------------------------------------------------------------------ tiny ----
// C[j][.] (the current contribution of word j) is a register queue: word j always
// uses C[0], then the queue rotates left by one with the new value at the back, so
// the word loop is a runtime loop (one copy of the digamma/exp code, ~160 VGPRs)
// instead of an unrolled one (>256 VGPRs + scratch).  After a sweep of n words the
// queue is rotated back by (-n) mod NMAX in log2(NMAX) conditional stages.
template <int N, int KPL>
__device__ __forceinline__ void rotl1(double (&C)[N][KPL]) {
#pragma unroll
  for (int i = 0; i < KPL; ++i) {
    const double t0 = C[0][i];
#pragma unroll
    for (int j = 0; j < N - 1; ++j) C[j][i] = C[j + 1][i];
    C[N - 1][i] = t0;
  }
}

template <int N, int KPL, int B>
__device__ __forceinline__ void rotl_if(double (&C)[N][KPL], bool on) {
#pragma unroll
  for (int i = 0; i < KPL; ++i) {
    double T[N];
#pragma unroll
    for (int j = 0; j < N; ++j) T[j] = C[(j + B) % N][i];
#pragma unroll
    for (int j = 0; j < N; ++j) C[j][i] = on ? T[j] : C[j][i];
  }
}

template <int KS>
__global__ __launch_bounds__(256) void gs_tiny(GSArgs a) {
  constexpr int TG = tiny_tg(KS), KPL = tiny_kpl(KS), NMAX = tiny_max(KS);
  constexpr int LTG = ilog2(TG);
  static_assert(NMAX == 4 || NMAX == 8, "tiny queue length");
  constexpr int DPB = 256 / TG;
  // the document's beta rows and counts, staged once per E-step (every sweep reads them)
  constexpr int BST = NMAX * KS + 1;   // odd stride in doubles: groups of a wave hit different banks
  __shared__ double sB[DPB][BST];
  __shared__ double sN[DPB][NMAX];
  __shared__ dvec2 sLog[kMathTabN];          // flog_t's table
  if (a.params[kParamDone] != 0.0) return;
  log_table_fill(sLog);
  __syncthreads();
  const int t = threadIdx.x, q = t & (TG - 1), g = t / TG;
  const int item = blockIdx.x * DPB + g;
  if (item >= a.n_items) return;   // whole TG groups leave together
  const double alpha = a.params[0], lik_const = a.params[1];
  const int vmi = (int)a.params[2];
  const double vconv = params_vconv(a.params);
  const int K = a.K;
  const int d = a.order[item];
  if (d < 0) return;   // XCD placement gap (GSPlan.xcd_gaps): this document slot only
  const int s0 = a.doc_ptr[d];
  const int n = min(a.doc_ptr[d + 1] - s0, NMAX);
  const int* __restrict__ wrow = a.word_idx + s0;
  const float* __restrict__ crow = a.counts + s0;
  for (int x = q; x < n * KS; x += TG) {
    const int j = x / KS, k = x - j * KS;
    sB[g][j * KS + k] = a.beta[(size_t)wrow[j] * KS + k];
  }
  if (q < n) sN[g][q] = (double)crow[q];
  wave_lds_sync();
  double total = 0.0;
  for (int j = 0; j < n; ++j) total += sN[g][j];
  const double g0 = alpha + total / K;
  const double m = psi_only(g0);
  double gam[KPL], psi[KPL], E[KPL], C[NMAX][KPL];
#pragma unroll
  for (int i = 0; i < KPL; ++i) {
    const bool real = q + TG * i < K;
    gam[i] = real ? g0 : 1.0;   // padding topics hold gamma = 1 (finite refresh, never summed or stored)
    psi[i] = m;
    E[i] = real ? 1.0 : 0.0;
  }
#pragma unroll
  for (int j = 0; j < NMAX; ++j) {
    const double cj = j < n ? sN[g][j] : 0.0;
#pragma unroll
    for (int i = 0; i < KPL; ++i) C[j][i] = (q + TG * i < K) ? cj / K : 0.0;
  }
  double L = 0.0, L_old = 0.0, conv = 1.0, GS = 0.0;
  int it = 0;
  while (var_continue(conv, vconv, it, vmi)) {
    ++it;
    double lw = 0.0, lp = 0.0;
#pragma unroll 1
    for (int j = 0; j < n; ++j) {
      const double* brow = &sB[g][j * KS];
      const double c = sN[g][j];
      double b[KPL];
#pragma unroll
      for (int i = 0; i < KPL; ++i) b[i] = (q + TG * i < KS) ? brow[q + TG * i] : 0.0;
      double pp = 0.0;
#pragma unroll
      for (int i = 0; i < KPL; ++i) pp = fma(E[i], b[i], pp);
      const double P = bits_sum<0, LTG, false>(pp);
      const double r = c * drcp(P);
      lw = fma(c, flog_t(P, sLog), lw);
      // branch-free refresh: the KPL digamma/exp chains interleave (a topic-guarded psi_exp is a basic block
      // of its own and the chains ran one after another); padding topics have E = 0, so nw = 0, and keep
      // gamma = 1, E = 0
#pragma unroll
      for (int i = 0; i < KPL; ++i) {
        const bool real = q + TG * i < K;
        const double nw = E[i] * b[i] * r;
        lp = fma(psi[i], nw, lp);
        gam[i] += nw - C[0][i];
        C[0][i] = nw;
        double pn, en;
        // padding topics: gamma stays 1 (nw = 0, C = 0), psi finite and only ever multiplied by nw = 0
        psi_exp<true, true, (KS > 32)>(gam[i], m, pn, en, sLog);   // table exp: K > 32 only (r5aq)
        psi[i] = pn;
        E[i] = real ? en : 0.0;
      }
      rotl1(C);
    }
    // n rotations so far: rotate by (-n) mod NMAX back to word order
    const int rb = (NMAX - n) & (NMAX - 1);
    rotl_if<NMAX, KPL, 1>(C, rb & 1);
    rotl_if<NMAX, KPL, 2>(C, rb & 2);
    if constexpr (NMAX == 8) rotl_if<NMAX, KPL, 4>(C, rb & 4);
    double gs = 0.0, lg = 0.0;
#pragma unroll
    for (int i = 0; i < KPL; ++i) {
      if (q + TG * i < K) {
        gs += gam[i];
        lg += lgamma_pos<true>(gam[i], sLog);
      }
    }
    GS = bits_sum<0, LTG, false>(gs);
    lg = bits_sum<0, LTG, false>(lg);
    lp = bits_sum<0, LTG, false>(lp);
    L = lik_const - lgamma_pos(GS) + lg + fma(m, total, lw) - lp;
    conv = (L_old - L) / L_old;
    L_old = L;
  }
  double ps = 0.0;
#pragma unroll
  for (int i = 0; i < KPL; ++i) {
    const int k = q + TG * i;
    if (k < K) ps += psi[i];
    if (k < KS) a.gamma[(size_t)d * KS + k] = k < K ? gam[i] : 0.0;
  }
  ps = bits_sum<0, LTG, false>(ps);
#pragma unroll
  for (int j = 0; j < NMAX; ++j) {
    if (j < n) {
      double* row = a.cphi + (size_t)(s0 + j) * KS;
#pragma unroll
      for (int i = 0; i < KPL; ++i)
        if (q + TG * i < KS) __builtin_nontemporal_store(C[j][i], &row[q + TG * i]);
    }
  }
  if (q == 0) {
    a.lik[d] = L;
    a.alpha_ss[d] = ps - K * psi_only(GS);
    a.iters[d] = it;
  }
}

// ----------------------------------------------------------------- small ----
// Short documents (the tiny kernel's limit < n <= kGsSmallMax words): 16 lanes per document, four
// documents per wave, everything in registers except the per-chunk tables.  A word's P is a 16-lane
// DPP sum (every lane holds the bitwise same value), the refresh runs in the same lanes right after
// the chunk's last word -- no LDS, no barrier between the word and the refresh, which is what a
// per-word schedule (n <= U: every word is a chunk) pays for in the one-wave team kernel.  The chunk
// contributions C[j] and the E each chunk used (final pass) are per-lane private arrays (scratch).
constexpr int kGsSmallMax = 64;
constexpr int small_kpl(int KS) { return (KS + 15) / 16; }

template <int KS>
__global__ __launch_bounds__(256) void gs_small(GSArgs a) {
  static_assert(KS <= 32, "small kernel: KS <= 32");
  constexpr int TG = 16, KPL = small_kpl(KS);
  if (a.params[kParamDone] != 0.0) return;
  const int t = threadIdx.x, q = t & (TG - 1);
  const int item = blockIdx.x * (256 / TG) + t / TG;
  if (item >= a.n_items) return;   // whole 16-lane groups leave together
  const double alpha = a.params[0], lik_const = a.params[1];
  const int vmi = (int)a.params[2];
  const double vconv = params_vconv(a.params);
  const int K = a.K;
  const int d = a.order[item];
  if (d < 0) return;   // XCD placement gap (GSPlan.xcd_gaps): this document slot only
  const int s0 = a.doc_ptr[d], n = a.doc_ptr[d + 1] - s0;
  const int U = a.gs_updates;
  const int W = n > 0 ? (n + U - 1) / U : 1;
  const int nch = (n + W - 1) / W;
  const int* __restrict__ wrow = a.word_idx + s0;
  const float* __restrict__ crow = a.counts + s0;
  double C[kGsUMax][KPL], Et[kGsUMax][KPL];
  // counts: each lane sums a stride of the document, a 16-lane sum gives the total; chunk sums serially
  double total = 0.0;
  for (int p = q; p < n; p += TG) total += (double)crow[p];
  total = bits_sum<0, 4, false>(total);
  const double g0 = alpha + total / K;
  const double m = psi_only(g0);
  double gam[KPL], psi[KPL], E[KPL], lps[KPL];
  bool real[KPL];
#pragma unroll
  for (int i = 0; i < KPL; ++i) {
    real[i] = q + TG * i < K;
    gam[i] = real[i] ? g0 : 0.0;
    psi[i] = m;
    E[i] = real[i] ? 1.0 : 0.0;
  }
  for (int j = 0; j < nch; ++j) {
    const int n0 = j * W, n1 = min(n, n0 + W);
    double cs = 0.0;
    for (int p = n0; p < n1; ++p) cs += (double)crow[p];   // integer counts: exact in any order
#pragma unroll
    for (int i = 0; i < KPL; ++i) C[j][i] = real[i] ? cs / K : 0.0;
  }
  // one-word-ahead prefetch of (row, count); the word order wraps into the next sweep
  auto load_row = [&](int p, double (&b)[KPL]) {
    const double* brow = a.beta + (size_t)wrow[p] * KS;
#pragma unroll
    for (int i = 0; i < KPL; ++i) b[i] = (q + TG * i < KS) ? brow[q + TG * i] : 0.0;
  };
  double bn[KPL];
  double cn = 0.0;
  if (n > 0) {
    load_row(0, bn);
    cn = (double)crow[0];
  }
  double L = 0.0, L_old = 0.0, conv = 1.0, GS = 0.0;
  int it = 0;
  while (var_continue(conv, vconv, it, vmi)) {
    ++it;
    double lw = 0.0;
#pragma unroll
    for (int i = 0; i < KPL; ++i) lps[i] = 0.0;
    for (int j = 0; j < nch; ++j) {
      const int n0 = j * W, n1 = min(n, n0 + W);
      double acc[KPL];
#pragma unroll
      for (int i = 0; i < KPL; ++i) acc[i] = 0.0;
      for (int p = n0; p < n1; ++p) {
        double b[KPL];
#pragma unroll
        for (int i = 0; i < KPL; ++i) b[i] = bn[i];
        const double c = cn;
        const int pn = p + 1 < n ? p + 1 : 0;
        load_row(pn, bn);
        cn = (double)crow[pn];
        double pp = 0.0;
#pragma unroll
        for (int i = 0; i < KPL; ++i) pp = fma(E[i], b[i], pp);
        const double P = bits_sum<0, 4, false>(pp);
        const double r = c * drcp(P);
        lw = fma(c, flog(P), lw);
#pragma unroll
        for (int i = 0; i < KPL; ++i) acc[i] = fma(r, b[i], acc[i]);
      }
      // branch-free refresh (interleaved chains; padding topics: E = 0, nw = 0, psi stays m)
#pragma unroll
      for (int i = 0; i < KPL; ++i) {
        const double nw = E[i] * acc[i];
        Et[j][i] = E[i];
        lps[i] = fma(psi[i], nw, lps[i]);
        gam[i] += nw - C[j][i];
        double pn, en;
        psi_exp(real[i] ? gam[i] : 1.0, m, pn, en);
        psi[i] = real[i] ? pn : psi[i];
        E[i] = real[i] ? en : 0.0;
        C[j][i] = nw;
      }
    }
    double gs = 0.0, lg = 0.0, lp = 0.0;
#pragma unroll
    for (int i = 0; i < KPL; ++i) {
      if (real[i]) {
        gs += gam[i];
        lg += lgamma_pos(gam[i]);
        lp += lps[i];
      }
    }
    GS = bits_sum<0, 4, false>(gs);
    lg = bits_sum<0, 4, false>(lg);
    lp = bits_sum<0, 4, false>(lp);
    L = lik_const - lgamma_pos(GS) + lg + fma(m, total, lw) - lp;
    conv = (L_old - L) / L_old;
    L_old = L;
  }
  double ps = 0.0;
#pragma unroll
  for (int i = 0; i < KPL; ++i) {
    const int k = q + TG * i;
    if (real[i]) ps += psi[i];
    if (k < KS) a.gamma[(size_t)d * KS + k] = gam[i];
  }
  ps = bits_sum<0, 4, false>(ps);
  if (q == 0) {
    a.lik[d] = L;
    a.alpha_ss[d] = ps - K * psi_only(GS);
    a.iters[d] = it;
  }
  // final pass: c_n phi_nk = E_jk b_nk r_n with the final sweep's chunk E
  for (int j = 0; j < nch; ++j) {
    const int n0 = j * W, n1 = min(n, n0 + W);
    for (int p = n0; p < n1; ++p) {
      double b[KPL];
      load_row(p, b);
      double pp = 0.0;
#pragma unroll
      for (int i = 0; i < KPL; ++i) pp = fma(Et[j][i], b[i], pp);
      const double r = (double)crow[p] * drcp(bits_sum<0, 4, false>(pp));
      double* row = a.cphi + (size_t)(s0 + p) * KS;
#pragma unroll
      for (int i = 0; i < KPL; ++i)
        if (q + TG * i < KS) __builtin_nontemporal_store(Et[j][i] * b[i] * r, &row[q + TG * i]);
    }
  }
}

// ----------------------------------------------------------------- chain ----
// lda-c's per-word schedule and chunks of a few words at K > 32 (U > 32): one wave per document, lane l
// holding topics l and l + 64 (TC = ceil(KS / 64)).  A chunk's P is a full-wave sum, the refresh TC
// digamma/exp chains per lane with E, gamma, psi in registers: no LDS, no barrier.  At U = 1024 a document of
// 257-4,096 words is a chain of up to 1,024 refreshes per sweep; the one-wave team paid an LDS round trip
// each way per chunk and waited on the row of the next word, gathered one chunk (= one word) ahead (r5h:
// 3.9 k cycles per chunk).  Here the rows of the next D words are in flight in a register ring (their ids D
// words further ahead), so a chunk costs its arithmetic.  Chunk tables in the document's own c*phi rows:
// C_j in row j W, the E chunk j used in row j W + 1 (chunks of >= 2 words); every row access is by the lane
// owning the topic.  Words wrap into the next sweep (a stopped run discards D prefetched rows).
template <int KS, int D>
__global__ __launch_bounds__(256) void gs_chain(GSArgs a) {
  static_assert(KS <= 128, "gs_chain: KS <= 128");
  constexpr int TC = (KS + 63) / 64;
  // TC = 2: lane l holds the topic pair 2l, 2l + 1 and loads it with one 16-byte load (KS even)
  constexpr bool PAIR = TC == 2;
  __shared__ dvec2 sLog[kMathTabN];      // flog_t's table
  if (a.params[kParamDone] != 0.0) return;
  log_table_fill(sLog);
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int item = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= a.n_items) return;   // whole waves leave together
  const double alpha = a.params[0], lik_const = a.params[1];
  const int vmi = (int)a.params[2];
  const double vconv = params_vconv(a.params);
  const int K = a.K;
  const int d = a.order[item];
  if (d < 0) return;
  const int s0 = a.doc_ptr[d], n = a.doc_ptr[d + 1] - s0;
  if (n <= 0) return;              // (the planner never sends an empty document)
  const int U = a.gs_updates;
  const int W = (n + U - 1) / U;
  const int nch = (n + W - 1) / W;
  const int* __restrict__ wrow = a.word_idx + s0;
  const float* __restrict__ crow = a.counts + s0;
  double* __restrict__ rows = a.cphi + (size_t)s0 * KS;
  auto topic = [&](int o) -> int { return PAIR ? 2 * lane + o : lane + 64 * o; };
  auto owned = [&](int o) { return topic(o) < KS; };
  // a word's TC values of this lane (lanes past KS read into the next row: beta's pad row)
  auto row_of = [&](int w, double (&v)[TC]) {
    if constexpr (PAIR) {
      const dvec2 x = *reinterpret_cast<const dvec2*>(a.beta + (size_t)w * KS + 2 * lane);
      v[0] = x.x;
      v[1] = x.y;
    } else if constexpr (KS >= 64) {
      v[0] = a.beta[(size_t)w * KS + lane];
    } else {
      // KS <= 32 (lda-c's per-word schedule at K <= 32): lanes past KS hold no topic and read nothing
      // (64 - KS of them would run past beta's one pad row)
      v[0] = lane < KS ? a.beta[(size_t)w * KS + lane] : 0.0;
    }
  };
  double total = 0.0;
  for (int j = 0; j < nch; ++j) {
    const int n0 = j * W, n1 = min(n, n0 + W);
    double cs = 0.0;
    for (int p = n0; p < n1; ++p) cs += (double)crow[p];   // integer counts: exact
    total += cs;
#pragma unroll
    for (int o = 0; o < TC; ++o)
      if (owned(o)) rows[(size_t)n0 * KS + topic(o)] = topic(o) < K ? cs / K : 0.0;
  }
  const double g0 = alpha + total / K;
  const double m = psi_only(g0);
  double gam[TC], psi[TC], E[TC], Cn[TC], acc[TC];
#pragma unroll
  for (int o = 0; o < TC; ++o) {
    const int k = topic(o);
    gam[o] = k < K ? g0 : 0.0;
    psi[o] = m;
    E[o] = k < K ? 1.0 : 0.0;
    Cn[o] = owned(o) ? rows[k] : 0.0;   // C_0 (this lane's own store)
    acc[o] = 0.0;
  }
  // rings: rb / rc the rows and counts of words g .. g + D - 1, wi / wc the ids and counts of words
  // g + D .. g + 2D - 1 (word g in slot g mod D); beta's pad row covers the lanes past KS
  double rb[D][TC], rc[D];
  int wi[D];
  float wc[D];
#pragma unroll
  for (int t = 0; t < D; ++t) {
    const int p = t % n;
    row_of(wrow[p], rb[t]);
    rc[t] = (double)crow[p];
    const int p2 = (t + D) % n;
    wi[t] = wrow[p2];
    wc[t] = crow[p2];
  }
  double L = 0.0, L_old = 0.0, conv = 1.0, GS = 0.0;
  double lw = 0.0, lp = 0.0;
  int pw = 0, j = 0;               // word of the sweep, its chunk
  int cend = min(n, W);            // end of chunk j
  int g2 = 2 * D;                  // the word whose id the slot being consumed loads next (mod n)
  bool run = var_continue(conv, vconv, 0, vmi);
  int it = run ? 1 : 0;            // sweeps begun
  while (run) {
#pragma unroll
    for (int t = 0; t < D; ++t) {
      if (run) {
        // word pw: P over the whole wave, then its contribution to the chunk
        double pp = 0.0;
#pragma unroll
        for (int o = 0; o < TC; ++o) pp = fma(E[o], rb[t][o], pp);
        const double P = group_sum<64>(pp);
        const double c = rc[t];
        const double r = c * drcp(P);
        lw = fma(c, flog_t(P, sLog), lw);
#pragma unroll
        for (int o = 0; o < TC; ++o) acc[o] = fma(r, rb[t][o], acc[o]);
        // the slot's next row (word pw + D) and the id D words beyond it
        {
          row_of(wi[t], rb[t]);
          rc[t] = (double)wc[t];
          const int p2 = g2 % n;
          wi[t] = wrow[p2];
          wc[t] = crow[p2];
          ++g2;
        }
        if (++pw == cend) {
          // chunk j ends: its tables, then the refresh (branch-free: padding topics keep E = 0)
          const int n0 = j * W;
          const bool two = cend - n0 >= 2;
#pragma unroll
          for (int o = 0; o < TC; ++o) {
            if (owned(o)) {
              rows[(size_t)n0 * KS + topic(o)] = E[o] * acc[o];
              if (two) rows[(size_t)(n0 + 1) * KS + topic(o)] = E[o];
            }
          }
#pragma unroll
          for (int o = 0; o < TC; ++o) {
            const bool real = topic(o) < K;
            const double nw = E[o] * acc[o];
            lp = fma(psi[o], nw, lp);
            gam[o] = real ? gam[o] + (nw - Cn[o]) : gam[o];
            double pn, en;
            psi_exp<true>(real ? gam[o] : 1.0, m, pn, en, sLog);
            psi[o] = real ? pn : psi[o];
            E[o] = real ? en : 0.0;
            acc[o] = 0.0;
          }
          j = j + 1 < nch ? j + 1 : 0;
          cend = min(n, (j + 1) * W);
#pragma unroll
          for (int o = 0; o < TC; ++o) Cn[o] = owned(o) ? rows[(size_t)j * W * KS + topic(o)] : 0.0;
          if (pw == n) {
            // sweep end: lda-c's likelihood and convergence test
            double gs = 0.0, lg = 0.0;
#pragma unroll
            for (int o = 0; o < TC; ++o) {
              const bool real = topic(o) < K;
              const double l = lgamma_pos<true>(real ? gam[o] : 1.0, sLog);
              gs += real ? gam[o] : 0.0;
              lg += real ? l : 0.0;
            }
            GS = group_sum<64>(gs);
            const double LG = group_sum<64>(lg), LP = group_sum<64>(lp);
            L = lik_const - lgamma_pos(GS) + LG + fma(m, total, lw) - LP;
            conv = (L_old - L) / L_old;
            L_old = L;
            run = var_continue(conv, vconv, it, vmi);
            it += run ? 1 : 0;
            pw = 0;
            lw = 0.0;
            lp = 0.0;
          }
        }
      }
    }
  }
  double ps = 0.0;
#pragma unroll
  for (int o = 0; o < TC; ++o) {
    const int k = topic(o);
    if (k < K) ps += psi[o];
    if (owned(o)) a.gamma[(size_t)d * KS + k] = gam[o];
  }
  ps = group_sum<64>(ps);
  if (lane == 0) {
    a.lik[d] = L;
    a.alpha_ss[d] = ps - K * psi_only(GS);
    a.iters[d] = it;
  }
  // final pass over chunks of >= 2 words: c_n phi_nk = E_jk b_nk r_n with the final sweep's chunk E
  if (W < 2) return;
  for (int jj = 0; jj < nch; ++jj) {
    const int n0 = jj * W, n1 = min(n, n0 + W);
    if (n1 - n0 < 2) continue;
    double Ej[TC];
#pragma unroll
    for (int o = 0; o < TC; ++o) Ej[o] = owned(o) ? rows[(size_t)(n0 + 1) * KS + topic(o)] : 0.0;
    for (int p = n0; p < n1; ++p) {
      double b[TC], pp = 0.0;
      row_of(wrow[p], b);
#pragma unroll
      for (int o = 0; o < TC; ++o) pp = fma(Ej[o], b[o], pp);
      const double rr = (double)crow[p] * drcp(group_sum<64>(pp));
#pragma unroll
      for (int o = 0; o < TC; ++o)
        if (owned(o)) __builtin_nontemporal_store(Ej[o] * b[o] * rr, &rows[(size_t)p * KS + topic(o)]);
    }
  }
}

// ---------------------------------------------------------- small, K > 32 ----
// The one-wave range at K > 32 (short documents; at lda-c's per-word schedule every document whose chunks
// hold <= 2 words): 16 lanes per document, KPL = ceil(KS / 16) topics per lane, four documents per wave,
// no LDS and no barrier.  The one-wave team (gs_team<KS, 1>) spreads a chunk's words over 4 word slots, then
// pays a cross-slot reduction and an LDS round trip per chunk and refreshes 2 topics per lane with 28 of
// 128 lane slots idle at K = 100; here the word loop runs in the document's 16 lanes and the refresh is
// KPL independent digamma/exp chains per lane (100 of 112 lane slots busy at K = 100).  Chunk tables live in
// the document's own c*phi rows (gs_team's GM layout): C_j in row j W, the E chunk j used in row j W + 1
// (chunks of >= 2 words); a one-word chunk's C_j IS that word's c*phi, so documents of <= U words need no
// final pass.  Every access to a row is by the lane that owns the topic (same-lane program order).
// RQ: words of the NEXT chunk whose rows are gathered during this chunk (ids one chunk earlier still); the
// rest of a chunk streams in batches of RQ.  Row loads are brow[q + 16 i] at constant offsets: lanes whose
// topic is >= KS read into the next row (beta carries one zero pad row, LDAEngine), values that only ever
// meet E = 0 / are never stored -- the clamped index held two address VGPRs per load.
template <int N, int KPL>
__device__ __forceinline__ void quad_word_steps(const double (&E)[KPL], const double (*b)[KPL], const double* c,
                                                double (&acc)[KPL], double& lw, const dvec2* __restrict__ tab) {
  double P[N];
#pragma unroll
  for (int u = 0; u < N; ++u) {
    double p0 = 0.0, p1 = 0.0;
#pragma unroll
    for (int i = 0; i < KPL; i += 2) p0 = fma(E[i], b[u][i], p0);
#pragma unroll
    for (int i = 1; i < KPL; i += 2) p1 = fma(E[i], b[u][i], p1);
    P[u] = bits_sum<0, 4, false>(p0 + p1);
  }
#pragma unroll
  for (int u = 0; u < N; ++u) {
    const double Pu = c[u] > 0.0 ? P[u] : 1.0;
    const double r = c[u] * drcp(Pu);
    lw = fma(c[u], flog_t(Pu, tab), lw);
#pragma unroll
    for (int i = 0; i < KPL; ++i) acc[i] = fma(r, b[u][i], acc[i]);
  }
}

template <int KS, int RQ, int MINW = 1>
__global__ __launch_bounds__(256, MINW) void gs_smallw(GSArgs a) {
  static_assert(KS > 32, "gs_smallw: KS > 32 (gs_small covers KS <= 32)");
  // one topic per 8-byte lane: the pair layout (TeamShape::PAIR) measured slower here (K = 100 bucket 9.48 vs
  // 8.99 ms, r5s: 8 topics per lane instead of 7 and 235 vs 196 VGPRs), the 16-lane kernel being refresh-bound
  constexpr bool PAIR = false;
  constexpr int TG = 16, KPL = PAIR ? 2 * ((KS + 2 * TG - 1) / (2 * TG)) : (KS + TG - 1) / TG;
  __shared__ dvec2 sLog[kMathTabN];          // flog_t's table
  if (a.params[kParamDone] != 0.0) return;
  log_table_fill(sLog);
  __syncthreads();
  const int t = threadIdx.x, q = t & (TG - 1);
  const int item = blockIdx.x * (256 / TG) + t / TG;
  if (item >= a.n_items) return;   // whole 16-lane groups leave together
  const double alpha = a.params[0], lik_const = a.params[1];
  const int vmi = (int)a.params[2];
  const double vconv = params_vconv(a.params);
  const int K = a.K;
  const int d = a.order[item];
  if (d < 0) return;
  const int s0 = a.doc_ptr[d], n = a.doc_ptr[d + 1] - s0;
  if (n <= 0) return;              // (the planner never sends an empty document)
  const int U = a.gs_updates;
  const int W = (n + U - 1) / U;
  const int nch = (n + W - 1) / W;
  const int* __restrict__ wrow = a.word_idx + s0;
  const float* __restrict__ crow = a.counts + s0;
  double* __restrict__ rows = a.cphi + (size_t)s0 * KS;
  // chunk count sums: C_j = cs_j / K into row j W (integer counts: the sums are exact in any order)
  double total = 0.0;
  for (int j = 0; j < nch; ++j) {
    const int n0 = j * W, n1 = min(n, n0 + W);
    double cs;
    if (W == 1) {
      cs = (double)crow[n0];
    } else {
      cs = 0.0;
      for (int p = n0 + q; p < n1; p += TG) cs += (double)crow[p];
      cs = bits_sum<0, 4, false>(cs);
    }
    total += cs;
#pragma unroll
    for (int i = 0; i < KPL; ++i) {
      const int k = tk<TG, PAIR>(q, i);
      if (k < KS) rows[(size_t)n0 * KS + k] = k < K ? cs / K : 0.0;
    }
  }
  const double g0 = alpha + total / K;
  const double m = psi_only(g0);
  double gam[KPL], psi[KPL], E[KPL], Cn[KPL];
#pragma unroll
  for (int i = 0; i < KPL; ++i) {
    const int k = tk<TG, PAIR>(q, i);
    gam[i] = k < K ? g0 : 1.0;   // padding topics hold gamma = 1 (finite refresh, never summed or stored)
    psi[i] = m;
    E[i] = k < K ? 1.0 : 0.0;
    Cn[i] = k < KS ? rows[k] : 0.0;   // C_0 (this lane's own stores above)
  }
  // head of a chunk: its first RQ words (past the chunk's end: count 0, the chunk's last row again)
  int wn[RQ];
  float cn[RQ];
  double bq[RQ][KPL], cq[RQ];
  auto head_ids = [&](int j) {
    const int n0 = j * W, n1 = min(n, n0 + W);
#pragma unroll
    for (int r = 0; r < RQ; ++r) {
      const int pc = min(n0 + r, n1 - 1);
      wn[r] = wrow[pc];
      cn[r] = n0 + r < n1 ? crow[pc] : 0.0f;
    }
  };
  auto head_rows = [&]() {
#pragma unroll
    for (int r = 0; r < RQ; ++r) {
      cq[r] = (double)cn[r];
      load_row<KS, KPL, TG, PAIR>(a.beta, wn[r], q, bq[r]);
    }
  };
  head_ids(0);
  head_rows();
  head_ids(nch > 1 ? 1 : 0);
  double L = 0.0, L_old = 0.0, conv = 1.0, GS = 0.0;
  int it = 0;
  while (var_continue(conv, vconv, it, vmi)) {
    ++it;
    double lw = 0.0, lp = 0.0;   // lp: sum of psi_k nw_jk over this lane's topics and the chunks
    for (int j = 0; j < nch; ++j) {
      const int n0 = j * W, n1 = min(n, n0 + W);
      double acc[KPL];
#pragma unroll
      for (int i = 0; i < KPL; ++i) acc[i] = 0.0;
      quad_word_steps<RQ, KPL>(E, bq, cq, acc, lw, sLog);
      // the rest of the chunk: batches of RQ rows, a batch's loads in flight together
      for (int p0 = n0 + RQ; p0 < n1; p0 += RQ) {
        double c[RQ];
#pragma unroll
        for (int r = 0; r < RQ; ++r) {
          const int pc = min(p0 + r, n1 - 1);
          c[r] = p0 + r < n1 ? (double)crow[pc] : 0.0;
          load_row<KS, KPL, TG, PAIR>(a.beta, wrow[pc], q, bq[r]);
        }
        quad_word_steps<RQ, KPL>(E, bq, c, acc, lw, sLog);
      }
      // next chunk's head rows in flight during the refresh; ids of the one after
      const int j1 = j + 1 < nch ? j + 1 : 0;
      head_rows();
      head_ids(j1 + 1 < nch ? j1 + 1 : 0);
      const bool two = n1 - n0 >= 2;
      // this chunk's C_j (and E_j) rows; lanes past KS exist only in the last topic group (static test)
#pragma unroll
      for (int i = 0; i < KPL; ++i) {
        const int k = tk<TG, PAIR>(q, i);
        if (k < KS) {
          rows[(size_t)n0 * KS + k] = E[i] * acc[i];
          if (two) rows[(size_t)(n0 + 1) * KS + k] = E[i];
        }
      }
      // the refresh without branches: a topic-guarded psi_exp is a basic block of its own, so the KPL
      // chains would run one after another instead of interleaved (padding topics keep gamma = 1
      // and E = 0: nw = 0 there)
#pragma unroll
      for (int i = 0; i < KPL; ++i) {
        const bool real = tk<TG, PAIR>(q, i) < K;
        const double nw = E[i] * acc[i];
        lp = fma(psi[i], nw, lp);
        gam[i] += nw - Cn[i];
        double p, e;
        // padding topics: gamma stays 1 (nw = 0, C = 0), psi finite and only ever multiplied by nw = 0
        psi_exp<true, true, false>(gam[i], m, p, e, sLog);
        psi[i] = p;
        E[i] = real ? e : 0.0;
      }
      // C of the next chunk, after this chunk's row stores (nch == 1: the same row)
#pragma unroll
      for (int i = 0; i < KPL; ++i) {
        const int k = tk<TG, PAIR>(q, i);
        Cn[i] = (k < KS) ? rows[(size_t)j1 * W * KS + k] : 0.0;
      }
    }
    double gs = 0.0, lg = 0.0;
#pragma unroll
    for (int i = 0; i < KPL; ++i) {
      const bool real = tk<TG, PAIR>(q, i) < K;
      const double l = lgamma_pos<true>(real ? gam[i] : 1.0, sLog);
      gs += real ? gam[i] : 0.0;
      lg += real ? l : 0.0;
    }
    GS = bits_sum<0, 4, false>(gs);
    lg = bits_sum<0, 4, false>(lg);
    lp = bits_sum<0, 4, false>(lp);
    L = lik_const - lgamma_pos(GS) + lg + fma(m, total, lw) - lp;
    conv = (L_old - L) / L_old;
    L_old = L;
  }
  double ps = 0.0;
#pragma unroll
  for (int i = 0; i < KPL; ++i) {
    const int k = tk<TG, PAIR>(q, i);
    if (k < K) ps += psi[i];
    if (k < KS) a.gamma[(size_t)d * KS + k] = k < K ? gam[i] : 0.0;
  }
  ps = bits_sum<0, 4, false>(ps);
  if (q == 0) {
    a.lik[d] = L;
    a.alpha_ss[d] = ps - K * psi_only(GS);
    a.iters[d] = it;
  }
  // final pass over chunks of >= 2 words: c_n phi_nk = E_jk b_nk r_n with the final sweep's chunk E
  // (read from row j W + 1 before the chunk's rows are overwritten; the same lane's addresses only)
  if (W < 2) return;
  for (int j = 0; j < nch; ++j) {
    const int n0 = j * W, n1 = min(n, n0 + W);
    if (n1 - n0 < 2) continue;
    double Ej[KPL];
#pragma unroll
    for (int i = 0; i < KPL; ++i) {
      const int k = tk<TG, PAIR>(q, i);
      Ej[i] = k < KS ? rows[(size_t)(n0 + 1) * KS + k] : 0.0;
    }
    for (int p0 = n0; p0 < n1; p0 += RQ) {
      double b[RQ][KPL], c[RQ];
#pragma unroll
      for (int r = 0; r < RQ; ++r) {
        const int pc = min(p0 + r, n1 - 1);
        c[r] = (double)crow[pc];
        load_row<KS, KPL, TG, PAIR>(a.beta, wrow[pc], q, b[r]);
      }
#pragma unroll
      for (int r = 0; r < RQ; ++r) {
        if (p0 + r >= n1) break;
        double pp0 = 0.0, pp1 = 0.0;
#pragma unroll
        for (int i = 0; i < KPL; i += 2) pp0 = fma(Ej[i], b[r][i], pp0);
#pragma unroll
        for (int i = 1; i < KPL; i += 2) pp1 = fma(Ej[i], b[r][i], pp1);
        const double rr = c[r] * drcp(bits_sum<0, 4, false>(pp0 + pp1));
        double* row = rows + (size_t)(p0 + r) * KS;
#pragma unroll
        for (int i = 0; i < KPL; ++i) {
          const int k = tk<TG, PAIR>(q, i);
          if (k < KS) __builtin_nontemporal_store(Ej[i] * b[r][i] * rr, &row[k]);
        }
      }
    }
  }
}

}  // namespace gs

// ------------------------------------------------------------------ launch ---
void launch_gs_tiny(const GSArgs& a, int KS, hipStream_t s) {
  switch (KS) {
#define ONI_KS(X)                                                                                       \
  case X: {                                                                                             \
    constexpr int per = 256 / gs::tiny_tg(X);                                                           \
    hipLaunchKernelGGL((gs::gs_tiny<X>), dim3((a.n_items + per - 1) / per), dim3(256), 0, s, a);        \
    break;                                                                                              \
  }
    ONI_FOR_EACH_KS(ONI_KS)
#undef ONI_KS
    default:
      throw std::runtime_error("gs_estep: unsupported KS " + std::to_string(KS));
  }
  ONI_HIP_CHECK(hipGetLastError());
}

template <int KS>
static void gs_small_ks(const GSArgs& a, hipStream_t s) {
  if (KS <= 32 && a.gs_updates > kGsUMax)
    throw std::runtime_error("gs_estep: gs_small keeps its chunk tables in LDS (U <= 32 at KS <= 32)");
  if constexpr (KS <= 32)
    hipLaunchKernelGGL((gs::gs_small<KS>), dim3((a.n_items + 15) / 16), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((gs::gs_smallw<KS, 2, (KS > 100 ? 1 : 2)>), dim3((a.n_items + 15) / 16), dim3(256), 0, s, a);
}

void launch_gs_small(const GSArgs& a, int KS, hipStream_t s) {
  switch (KS) {
#define ONI_KS(X)         \
  case X:                 \
    gs_small_ks<X>(a, s); \
    break;
    ONI_FOR_EACH_KS(ONI_KS)
#undef ONI_KS
    default:
      throw std::runtime_error("gs_estep: unsupported KS " + std::to_string(KS));
  }
  ONI_HIP_CHECK(hipGetLastError());
}

void launch_gs_chain(const GSArgs& a, int KS, hipStream_t s) {
  switch (KS) {
#define ONI_KS(X)                                                                                       \
  case X:                                                                                               \
    hipLaunchKernelGGL((gs::gs_chain<X, 8>), dim3((a.n_items + 3) / 4), dim3(256), 0, s, a);            \
    break;
    ONI_FOR_EACH_KS(ONI_KS)
#undef ONI_KS
    default:
      throw std::runtime_error("gs_estep: unsupported KS " + std::to_string(KS));
  }
  ONI_HIP_CHECK(hipGetLastError());
}

int gs_tiny_max(int KS) {
  switch (KS) {
#define ONI_KS(X) \
  case X:         \
    return gs::tiny_max(X);
    ONI_FOR_EACH_KS(ONI_KS)
#undef ONI_KS
    default:
      throw std::runtime_error("gs_tiny_max: unsupported KS " + std::to_string(KS));
  }
}

}  // namespace oni
