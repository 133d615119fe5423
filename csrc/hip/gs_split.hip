// fp64 block Gauss-Seidel E-step, the split-document kernel gs_splitw: one long document over several
// workgroups (chunk algebra and schedule: header of lda_gs64.hip; word-slot geometry and the word phase of
// the 8-wave team: gs_layout.h; tags and the launch epoch: estep_common.h).
#include <stdexcept>
#include <string>

#include "common.h"
#include "estep_common.h"
#include "gs_layout.h"
#include "gs_math.h"
#include "kernels.h"

namespace oni {
namespace gs {

// ----------------------------------------------------------------- split ----
// One long document over G workgroups (K > 32).  Chunk j of a sweep
// (W = ceil(n / U) words) is cut into G contiguous ranges of ceil(W / G) words; workgroup g gathers
// and reduces its range's S_k = sum_n r_n b_nk and sum_n c_n log P_n, publishes them, and reads all
// G partials back in segment order (the same bits in every workgroup), so the G replicas of
// (gamma, psi, E, C) run the identical refresh and the identical lda-c convergence test: one
// exchange per chunk.  A double travels as two tagged 8-byte granules {uint32 half, uint32 tag}
// (relaxed agent-scope 64-bit stores / loads are single-copy atomic); tag = (launch epoch, chunk
// sequence number) (estep_common.h) and a parity double buffer: a workgroup reuses buffer (seq & 1)
// at seq + 2 only after every segment has published seq + 1, i.e. after every segment has finished
// reading seq.  The host caps a launch below the co-resident capacity (gs_split_capacity), so the
// exchange cannot deadlock; a bounded wait sets `error`.
__device__ __forceinline__ void put_tagged_bits(unsigned long long* p, unsigned v, unsigned tag) {
  __hip_atomic_store(p, ((unsigned long long)tag << 32) | (unsigned long long)v, __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}

// Segment-order sums of the tagged doubles of TC columns (column c: granules x[u * stride + 2 c] and
// x[u * stride + 2 c + 1] = (lo, hi) bits of segment u's value, u < G <= GMX).  Every pass issues ALL
// TC x GMX x 2 loads back to back (unconditional, clamped indices) and then checks the tags; a pass that
// finds any stale granule is repeated whole.  Loads inside per-granule branches get a vmcnt(0) each -- one
// round trip per granule group; the round-3 form polled 4 segments per round trip, 2 x 4 serial round
// trips per chunk at G = 16, K = 100 (12.8 k cycles per chunk, profiles/r5f) -- and the microbenchmark
// (scripts/micro/xcd_exchange.hip) measured batched polls at half the per-granule form.  False on a timeout.
constexpr int kSplitMaxSeg = 16;   // GMX of the single-round gather (more: split_allreduce2)
template <int TC, int GMX, int NC>
__device__ __forceinline__ bool tagged_gather(const unsigned long long* x, int G, int stride, int lane, unsigned tag,
                                              double (&out)[TC]) {
  unsigned long long v[TC][GMX][2];
  long spins = 0;
  for (;;) {
#pragma unroll
    for (int o = 0; o < TC; ++o) {
      const int c = min(lane + 64 * o, NC - 1);
#pragma unroll
      for (int u = 0; u < GMX; ++u) {
        const unsigned long long* p = x + (size_t)min(u, G - 1) * stride + 2 * c;
        v[o][u][0] = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v[o][u][1] = __hip_atomic_load(p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    bool ok = true;
#pragma unroll
    for (int o = 0; o < TC; ++o)
#pragma unroll
      for (int u = 0; u < GMX; ++u)
        ok &= u >= G || ((unsigned)(v[o][u][0] >> 32) == tag && (unsigned)(v[o][u][1] >> 32) == tag);
    if (ok) break;
    if (++spins > kSplitSpinLimit) {
#pragma unroll
      for (int o = 0; o < TC; ++o) out[o] = __builtin_nan("");
      return false;
    }
    __builtin_amdgcn_s_sleep(1);
  }
#pragma unroll
  for (int o = 0; o < TC; ++o) {
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < GMX; ++u)
      if (u < G)
        s += __longlong_as_double((long long)(((v[o][u][1] & 0xffffffffull) << 32) | (v[o][u][0] & 0xffffffffull)));
    out[o] = s;
  }
  return true;
}

// Two-phase exchange for G > kSplitMaxSeg segments (up to kSplitMaxSeg2): a single-round gather reads
// G x NC x 2 granules per segment -- linear in G, and past 16 segments more than the topic wave's registers
// can keep in flight -- so the columns are owned instead: segment g reduces columns c = g + G x (x < nown)
// over the G published partials (reduce-scatter: ~NC x 2 granules per segment, <= 4 per lane, all in one
// batched poll), publishes each owned total once with the chunk's tag into the document's totals row, and
// every segment then gathers the NC totals (all-gather: NC x 2 granules).  Two round trips whatever G is;
// each total is computed by exactly one segment, so every replica reads the same bits.  Buffer reuse: the
// totals row (seq & 1) is rewritten at seq + 2 only after its owner has read every segment's seq + 2
// partial, which a segment publishes only after it has gathered the seq + 1 totals, i.e. after it has
// finished reading seq's.  sPair: LDS scratch of >= NC + kSplitMaxSeg2 doubles (the topic wave only).
constexpr int kSplitMaxSeg2 = 128;   // two-phase exchange: two segments per topic-wave lane
template <int TC, int NC, int GR>
__device__ __forceinline__ bool split_allreduce2(const unsigned long long* __restrict__ xs, unsigned long long* xt,
                                                 int G, int g, int lane, unsigned tag, double* sPair,
                                                 double (&out)[TC]) {
  // pairs (column, segment) per lane: nown x G < NC + G when G < NC, = G <= kSplitMaxSeg2 otherwise, and
  // < 2 NC when NC / 2 < G < NC (nown = 2)
  constexpr int PMAX = ((2 * NC > kSplitMaxSeg2 ? 2 * NC : kSplitMaxSeg2) + 63) / 64;
  const int nown = g < NC ? (NC - 1 - g) / G + 1 : 0;        // uniform across the wave
  const int npair = nown * G;
  if (npair > 0) {
    int off[PMAX];
#pragma unroll
    for (int o = 0; o < PMAX; ++o) {
      const int i = min(lane + 64 * o, npair - 1);
      const int x = i / G, u = i - x * G;
      off[o] = u * GR + 2 * (g + G * x);
    }
    unsigned long long v[PMAX][2];
    long spins = 0;
    for (;;) {
#pragma unroll
      for (int o = 0; o < PMAX; ++o) {
        v[o][0] = __hip_atomic_load(xs + off[o], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v[o][1] = __hip_atomic_load(xs + off[o] + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      bool ok = true;
#pragma unroll
      for (int o = 0; o < PMAX; ++o)
        ok &= lane + 64 * o >= npair || ((unsigned)(v[o][0] >> 32) == tag && (unsigned)(v[o][1] >> 32) == tag);
      if (ok) break;
      if (++spins > kSplitSpinLimit) {
#pragma unroll
        for (int o = 0; o < TC; ++o) out[o] = __builtin_nan("");
        return false;
      }
      __builtin_amdgcn_s_sleep(1);
    }
#pragma unroll
    for (int o = 0; o < PMAX; ++o)
      if (lane + 64 * o < npair)
        sPair[lane + 64 * o] =
            __longlong_as_double((long long)(((v[o][1] & 0xffffffffull) << 32) | (v[o][0] & 0xffffffffull)));
    wave_lds_sync();
    for (int x = 0; x < nown; ++x) {
      double s = (lane < G ? sPair[x * G + lane] : 0.0) + (lane + 64 < G ? sPair[x * G + lane + 64] : 0.0);
      s = group_sum<64>(s);   // fixed DPP tree: computed once, by this owner
      if (lane == 0) {
        const unsigned long long bits = (unsigned long long)__double_as_longlong(s);
        unsigned long long* row = xt + 2 * (g + G * x);
        put_tagged_bits(row, (unsigned)(bits & 0xffffffffull), tag);
        put_tagged_bits(row + 1, (unsigned)(bits >> 32), tag);
      }
    }
    wave_lds_sync();
  }
  return tagged_gather<TC, 1, NC>(xt, 1, GR, lane, tag, out);
}

// ------------------------------------------------------------ split kernel ----
// 7 word waves + 1 topic wave: the word waves leave their chunk partials in LDS, signal an LDS arrival
// counter and issue the NEXT chunk's row prefetch at once; the topic wave sums the waves, publishes the
// segment's tagged granules, sweeps the document's G segments and runs the refresh.  Its poll loads
// never queue behind row prefetches (vmcnt is in order per wave, and the hand-off price sits in the
// consumer's memory queue -- MI355X_MICROARCH handoff-1to1 / gather-pass), and a chunk costs one
// workgroup barrier.  (The round-2 form with all three roles in the same eight waves and three barriers
// per chunk was 3.82 vs 3.17 ms on the K = 50 split bucket and is gone; profiles/r3_tuning_log.md.)
// UM: chunk-table rows in LDS (U <= UM): 32, or 64 where 2 x 64 x KS doubles still fit the 64 KB of
// static LDS (KS <= 52: K = 50 at U = 64, the schedule that meets lda-c parity there,
// profiles/r3_precision_parity.md).  GM (U > UM at KS > 32, lda-c's per-word schedule): the chunk tables
// move to the launch's per-segment scratch sp.tab ([n_blocks][U][C_j | E_j][KS]; each replica reads only
// what it wrote itself) and C_j is loaded one chunk ahead, as gs_team's c*phi-row layout does.
template <int KS, int UM = kGsUMax, bool GM = false>
__global__ __launch_bounds__(512) void gs_splitw(GSArgs a, SplitArgs sp) {
  using T = TeamShape<KS, 8>;   // word-slot geometry and prefetch depth of the 8-wave team
  constexpr int NW = 7, NTD = (NW + 1) * 64, TG = T::TG, KPL = T::KPL, NSW = T::NSW, LSW = T::LSW, NS = NW * NSW,
                RMAX = T::RMAX;
  constexpr bool PAIR = T::PAIR;
  constexpr int NC = KS + 1;                 // exchanged columns: KS topic sums + the log-sum
  constexpr int GR = 2 * NC;                 // granules per segment row
  constexpr int TC = (NC + 63) / 64;         // columns per topic-wave lane
  constexpr int UT = GM ? 1 : UM;             // LDS chunk-table rows
  __shared__ double sC[UT][KS];
  __shared__ double sEt[UT][KS];
  __shared__ double sE[KS];
  __shared__ double sRed[NW][KS];
  __shared__ double sRedL[NW];
  __shared__ double sCs[GM ? kGsUMaxWide : UM];
  __shared__ double sScal[4];
  __shared__ int arrive[NW];   // per word wave: chunks whose partial sums it has left in sRed / sRedL
  __shared__ int sFail;
  __shared__ double sPair[KS > 32 ? 2 * NC + kSplitMaxSeg2 : 1];   // the two-phase exchange's values
  if (a.params[kParamDone] != 0.0) return;
  const int t = threadIdx.x, b = blockIdx.x;
  const int d = sp.seg_doc[b], g = sp.seg_index[b], G = sp.seg_count[b], base = sp.seg_base[b];
  const int dslot = sp.doc_slot[b];
  int* counter = sp.counter + dslot;
  const int epoch = __hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const double alpha = a.params[0], lik_const = a.params[1];
  const int vmi = (int)a.params[2];
  const double vconv = params_vconv(a.params);
  const int K = a.K;
  auto kc_ = [](int k) { return k < KS ? k : KS - 1; };   // an in-bounds LDS column for guarded reads
  const int lane = t & 63, wv = t >> 6;
  const bool topic_wave = wv == NW;
  const int q = lane >> LSW, sl = lane & (NSW - 1);
  const int slot = wv * NSW + sl;
  const int s0 = a.doc_ptr[d], n = a.doc_ptr[d + 1] - s0;   // n > 0 (host)
  const int U = a.gs_updates;
  const int W = (n + U - 1) / U;
  const int nch = (n + W - 1) / W;
  const int WG = (W + G - 1) / G;             // words of a chunk per segment
  const int nact = min(NW, (WG + NSW - 1) / NSW);
  const bool active = wv < nact;              // never the topic wave
  const int* __restrict__ wrow = a.word_idx + s0;
  const float* __restrict__ crow = a.counts + s0;
  // row j: C_j, then E_j; sp.tab_rows >= every batch document's nch (GSSplitPlan)
  double* __restrict__ tab = GM ? sp.tab + (size_t)b * sp.tab_rows * 2 * KS : nullptr;
  auto range = [&](int j, int& m0, int& m1) {
    const int n1 = min(n, (j + 1) * W);
    m0 = min(n1, j * W + g * WG);
    m1 = min(n1, m0 + WG);
  };
  if (GM && nch > sp.tab_rows) {   // a host plan error: every segment of d leaves (same nch), none waits
    if (t == 0) __hip_atomic_store(sp.error, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  if (sp.csum) {
    // the chunk count sums the plan computed once (GSSplitPlan.chunk_sums): no pass over the whole
    // document's counts in every segment (443 k words x 124 segments at config 5)
    const double* cs = sp.csum + (size_t)dslot * sp.csum_stride;
    for (int j = t; j < nch; j += NTD) sCs[j] = cs[j];
    if (t == 0) sFail = 0;
    if (t < NW) arrive[t] = 0;
  } else {
    for (int j = t; j < nch; j += NTD) sCs[j] = 0.0;
    if (t == 0) sFail = 0;
    if (t < NW) arrive[t] = 0;
    lds_barrier();
    for (int p = t; p < n; p += NTD) atomicAdd(&sCs[p / W], (double)crow[p]);   // integer counts: exact
  }
  lds_barrier();
  double total = 0.0;
  for (int j = 0; j < nch; ++j) total += sCs[j];
  const double g0 = alpha + total / K;
  const double m = psi_only(g0);
  const bool twt = a.dbg != nullptr && b == 0 && t == NW * 64;   // topic-wave timer lane
  const bool wwt = a.dbg != nullptr && b == 0 && t == 0;         // word-wave timer lane
  long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  long long tc = (twt || wwt) ? clock64() : 0;
  auto tick = [&](int i) {
    if (twt || wwt) {
      const long long x = clock64();
      ph[i] += x - tc;
      tc = x;
    }
  };
  double L = 0.0, L_old = 0.0, conv = 1.0, GS = 0.0;
  int it = 0;
  bool failed = false;
  auto sweep_end = [&]() {
    lds_barrier();
    GS = sScal[1];
    L = lik_const - lgamma_pos(GS) + sScal[2] + fma(m, total, sScal[0]) - sScal[3];
    conv = (L_old - L) / L_old;
    L_old = L;
    lds_barrier();
  };
  if (topic_wave) {
    // ------------------------------------------------------------ topic wave
    __builtin_amdgcn_s_setprio(3);   // its chain is the critical path; the word waves wait on it
    double gam[TC], psi[TC], lps[TC], Cn[TC];
#pragma unroll
    for (int o = 0; o < TC; ++o) {
      const int k = lane + 64 * o;
      gam[o] = k < K ? g0 : 0.0;
      psi[o] = m;
      lps[o] = 0.0;
      Cn[o] = 0.0;
      if (k < KS) {
        sE[k] = k < K ? 1.0 : 0.0;
        for (int j = 0; j < nch; ++j) {
          const double c0 = k < K ? sCs[j] / K : 0.0;
          if constexpr (GM)
            tab[(size_t)j * 2 * KS + k] = c0;
          else
            sC[j][k] = c0;
        }
        if constexpr (GM) Cn[o] = tab[k];   // C_0 (this lane's own store)
      }
    }
    double LWs = 0.0;
    int want = 0;
    lds_barrier();   // (1)
    while (!failed && var_continue(conv, vconv, it, vmi)) {
      ++it;
#pragma unroll
      for (int o = 0; o < TC; ++o) lps[o] = 0.0;
      for (int j = 0; j < nch; ++j) {
        ph[7] += twt ? 1 : 0;
        ++want;
        // this chunk's C_jk and E_k before the waits (the LDS reads are off the chain)
        double gC[TC], Eo[TC];
#pragma unroll
        for (int o = 0; o < TC; ++o) {
          const int k = lane + 64 * o;
          gC[o] = k < KS ? gam[o] - (GM ? Cn[o] : sC[j][kc_(k)]) : 0.0;
          Eo[o] = k < KS ? sE[k] : 0.0;
        }
        // the segment's column sums, in wave order as the waves arrive (one add after the last)
        double part[TC];
#pragma unroll
        for (int o = 0; o < TC; ++o) part[o] = 0.0;
#pragma unroll
        for (int v = 0; v < NW; ++v) {
          if (v < nact) {
            while (__hip_atomic_load(&arrive[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < want)
              __builtin_amdgcn_s_sleep(1);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
#pragma unroll
            for (int o = 0; o < TC; ++o) {
              const int c = lane + 64 * o;
              part[o] += c < KS ? sRed[v][c] : (c == KS ? sRedL[v] : 0.0);
            }
          }
        }
        tick(3);
        const int seq = (it - 1) * nch + j + 1;
        const unsigned tag = split_tag(epoch, seq);
        unsigned long long* xb = sp.xchg + (size_t)(seq & 1) * sp.n_blocks * GR;
        // publish this segment's column sums, then sweep the G segments
#pragma unroll
        for (int o = 0; o < TC; ++o) {
          const int c = lane + 64 * o;
          if (c < NC) {
            const unsigned long long bits = (unsigned long long)__double_as_longlong(part[o]);
            unsigned long long* row = xb + (size_t)b * GR + 2 * c;
            put_tagged_bits(row, (unsigned)(bits & 0xffffffffull), tag);
            put_tagged_bits(row + 1, (unsigned)(bits >> 32), tag);
          }
        }
        // one batched pass over every column and segment up to 8 segments; past that a pass per column
        // (TC x 16 x 2 granules in flight spilled at K = 100)
        double tot[TC];
        const unsigned long long* xs = xb + (size_t)base * GR;
        bool ok = true;
        if (G <= 4) {
          ok = tagged_gather<TC, 4, NC>(xs, G, GR, lane, tag, tot);
        } else if (G <= 8) {
          ok = tagged_gather<TC, 8, NC>(xs, G, GR, lane, tag, tot);
        } else if (G <= kSplitMaxSeg) {
#pragma unroll
          for (int o = 0; o < TC; ++o) {
            double t1[1];
            ok &= tagged_gather<1, kSplitMaxSeg, NC>(xs, G, GR, lane + 64 * o, tag, t1);
            tot[o] = t1[0];
          }
        } else if constexpr (KS > 32) {
          // the document's totals row, after the launch's 2 x n_blocks partial rows (KS <= 32 splits take at
          // most kSplitMaxSeg segments: GSSplitPlan; the narrow word layout has no registers to spare for it)
          unsigned long long* xt = sp.xchg + (size_t)2 * sp.n_blocks * GR +
                                   ((size_t)(seq & 1) * sp.n_docs + dslot) * GR;
          ok = split_allreduce2<TC, NC, GR>(xs, xt, G, g, lane, tag, sPair, tot);
        } else {
          ok = false;
        }
        tick(4);
        if (!ok) {
          sFail = 1;
          __hip_atomic_store(sp.error, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // branch-free refresh: the TC chains of a lane interleave (padding / log-sum columns have
        // Eo = 0: nw = 0, and keep gamma = 0, psi = m, E = 0)
        double En[TC];
#pragma unroll
        for (int o = 0; o < TC; ++o) {
          const bool real = lane + 64 * o < K;
          const double nw = Eo[o] * tot[o];
          lps[o] = fma(psi[o], nw, lps[o]);
          gam[o] = real ? fma(Eo[o], tot[o], gC[o]) : gam[o];   // gamma_k + (new_jk - C_jk) in one rounding
          double pn, en;
          psi_exp(real ? gam[o] : 1.0, m, pn, en);
          psi[o] = real ? pn : psi[o];
          En[o] = real ? en : 0.0;
        }
#pragma unroll
        for (int o = 0; o < TC; ++o) {
          const int k = lane + 64 * o;
          if (k < KS) {
            if constexpr (GM) {
              tab[(size_t)j * 2 * KS + k] = Eo[o] * tot[o];
              tab[(size_t)j * 2 * KS + KS + k] = Eo[o];
              Cn[o] = tab[(size_t)(j + 1 < nch ? j + 1 : 0) * 2 * KS + k];   // after the store (nch == 1)
            } else {
              sC[j][k] = Eo[o] * tot[o];
              sEt[j][k] = Eo[o];
            }
            sE[k] = En[o];
          } else if (k == KS) {
            LWs += tot[o];
          }
        }
        tick(5);
        lds_barrier();   // (B) E of chunk j + 1 published
        if (sFail) {
          failed = true;
          break;
        }
      }
      if (failed) break;
      double gs = 0.0, lg = 0.0, lp = 0.0, lw = 0.0;
#pragma unroll
      for (int o = 0; o < TC; ++o) {
        const int k = lane + 64 * o;
        if (k < K) {
          gs += gam[o];
          lg += lgamma_pos(gam[o]);
          lp += lps[o];
        }
        if (k == KS) lw = LWs;
      }
      LWs = 0.0;
      const double w1 = group_sum<64>(gs), w2 = group_sum<64>(lg), w3 = group_sum<64>(lp), w0 = group_sum<64>(lw);
      if (lane == 0) {
        sScal[0] = w0;
        sScal[1] = w1;
        sScal[2] = w2;
        sScal[3] = w3;
      }
      sweep_end();
      tick(6);
    }
    if constexpr (GM) __syncthreads();   // pairs with the word waves': the E_j table stores before their final pass
    if (twt)
      for (int i = 3; i < 8; ++i) a.dbg[i] = ph[i];
    split_exit(counter, sp.n_docs, G);   // thread 0 only: a no-op here (kept beside the word waves' call)
    double ps = 0.0;
#pragma unroll
    for (int o = 0; o < TC; ++o) {
      const int k = lane + 64 * o;
      if (k < K) ps += psi[o];
      if (g == 0 && k < KS) a.gamma[(size_t)d * KS + k] = gam[o];
    }
    ps = group_sum<64>(ps);
    if (g == 0 && lane == 0) {
      a.lik[d] = failed ? __builtin_nan("") : L;   // a timed-out exchange surfaces as a NaN likelihood
      a.alpha_ss[d] = ps - K * psi_only(GS);
      a.iters[d] = it;
    }
    return;
  }
  // -------------------------------------------------------------- word waves
  int wc[RMAX], wn[RMAX];
  float cc[RMAX], cn[RMAX];
  unsigned vc = 0, vn = 0;
  double bc[RMAX][KPL];
  auto load_ids = [&](int j, int (&w)[RMAX], float (&c)[RMAX], unsigned& v) {
    int m0, m1;
    range(j, m0, m1);
    v = 0;
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
      const int p = m0 + slot + r * NS;
      v |= (active && p < m1) ? (1u << r) : 0u;
      const int pc = max(0, min(p, m1 - 1));
      w[r] = wrow[pc];
      c[r] = crow[pc];
    }
  };
  auto load_rows = [&](const int (&w)[RMAX], unsigned v) {
    if (!active) return;
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
      // unconditional, constant offsets: a round past the range re-reads a valid row of the document
      // and carries count 0 (beta's pad row covers topic lanes past KS: gs_smallw)
      load_row<KS, KPL, TG, PAIR>(a.beta, w[r], q, bc[r]);
    }
  };
  load_ids(0, wc, cc, vc);
  load_rows(wc, vc);
  load_ids(nch > 1 ? 1 : 0, wn, cn, vn);
  lds_barrier();   // (1)
  while (!failed && var_continue(conv, vconv, it, vmi)) {
    ++it;
    for (int j = 0; j < nch; ++j) {
      if (active) {
        int m0, m1;
        range(j, m0, m1);
        double E[KPL], acc[KPL], lw = 0.0;
#pragma unroll
        for (int i = 0; i < KPL; ++i) {
          E[i] = (tk<TG, PAIR>(q, i) < KS) ? sE[tk<TG, PAIR>(q, i)] : 0.0;
          acc[i] = 0.0;
        }
        double cr[RMAX];
#pragma unroll
        for (int r = 0; r < RMAX; ++r) cr[r] = ((vc >> r) & 1u) ? (double)cc[r] : 0.0;
        const int R = (m1 - m0 + NS - 1) / NS;
        if (R <= 1) {
          word_steps<1, KPL, LSW>(E, bc, cr, acc, lw);
        } else if (R <= 2 || RMAX <= 2) {
          word_steps<(RMAX < 2 ? RMAX : 2), KPL, LSW>(E, bc, cr, acc, lw);
        } else if (R <= 4 || RMAX <= 4) {
          word_steps<(RMAX < 4 ? RMAX : 4), KPL, LSW>(E, bc, cr, acc, lw);
        } else {
          word_steps<RMAX, KPL, LSW>(E, bc, cr, acc, lw);
        }
        stream_tail<RMAX, KS, KPL, TG, LSW, PAIR>(a.beta, wrow, crow, m0 + slot + RMAX * NS, m1, NS, q, E, bc, acc, lw);
#pragma unroll
        for (int i = 0; i < KPL; ++i) acc[i] = bits_sum<0, LSW, false>(acc[i]);
        lw = group_sum<64>(q == 0 ? lw : 0.0);
        if (sl == 0) {
#pragma unroll
          for (int i = 0; i < KPL; ++i)
            if (tk<TG, PAIR>(q, i) < KS) sRed[wv][tk<TG, PAIR>(q, i)] = acc[i];
        }
        if (lane == 0) sRedL[wv] = lw;
        // arrival (LDS only: no vmcnt wait), then the next chunk's rows -- beside the exchange
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
        if (lane == 0) __hip_atomic_fetch_add(&arrive[wv], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        tick(0);
        const int j1 = j + 1 < nch ? j + 1 : 0;
        const int j2 = j1 + 1 < nch ? j1 + 1 : 0;
#pragma unroll
        for (int r = 0; r < RMAX; ++r) {
          wc[r] = wn[r];
          cc[r] = cn[r];
        }
        vc = vn;
        load_rows(wc, vc);
        load_ids(j2, wn, cn, vn);
        tick(1);
      }
      lds_barrier();   // (B)
      tick(2);
      if (sFail) {
        failed = true;
        break;
      }
    }
    if (failed) break;
    sweep_end();
  }
  if constexpr (GM) __syncthreads();     // the topic wave's E_j table stores are visible past this
  if (wwt)
    for (int i = 0; i < 3; ++i) a.dbg[i] = ph[i];
  // every thread of this workgroup is past its last exchange (the loops end on a barrier)
  split_exit(counter, sp.n_docs, G);
  // final pass over this segment's ranges: c_n phi_nk = E_jk b_nk r_n with the final sweep's chunk E
  if (!active) return;
  for (int j = 0; j < nch; ++j) {
    int m0, m1;
    range(j, m0, m1);
    double E[KPL];
#pragma unroll
    for (int i = 0; i < KPL; ++i) {
      const int k = tk<TG, PAIR>(q, i);
      E[i] = k < KS ? (GM ? tab[(size_t)j * 2 * KS + KS + k] : sEt[j][kc_(k)]) : 0.0;
    }
    for (int p = m0 + slot; p < m1; p += NS) {
      const double* brow = a.beta + (size_t)wrow[p] * KS;
      const double c = (double)crow[p];
      double bv[KPL];
#pragma unroll
      for (int i = 0; i < KPL; ++i) bv[i] = (tk<TG, PAIR>(q, i) < KS) ? brow[tk<TG, PAIR>(q, i)] : 0.0;
      double pp = 0.0;
#pragma unroll
      for (int i = 0; i < KPL; ++i) pp = fma(E[i], bv[i], pp);
      const double r = c * drcp(bits_sum<LSW, 6>(pp));
      double* row = a.cphi + (size_t)(s0 + p) * KS;
#pragma unroll
      for (int i = 0; i < KPL; ++i)
        if (tk<TG, PAIR>(q, i) < KS) __builtin_nontemporal_store(E[i] * bv[i] * r, &row[tk<TG, PAIR>(q, i)]);
    }
  }
}

}  // namespace gs

template <int KS>
constexpr int split_umax_ks() { return KS <= 52 ? 64 : kGsUMax; }   // chunk tables in LDS

int gs_split_lds_umax(int KS) {
  switch (KS) {
#define ONI_KS(X) \
  case X:         \
    return split_umax_ks<X>();
    ONI_FOR_EACH_KS(ONI_KS)
#undef ONI_KS
    default:
      return kGsUMax;
  }
}

// past the LDS tables, KS > 32 keeps its chunk tables in the launch's scratch (gs_splitw GM)
int gs_split_umax(int KS) { return KS > 32 ? kGsUMaxWide : gs_split_lds_umax(KS); }

template <int KS>
static int gs_split_capacity_ks() {
  int dev = 0, per_cu = 0;
  hipDeviceProp_t p;
  ONI_HIP_CHECK(hipGetDevice(&dev));
  ONI_HIP_CHECK(hipGetDeviceProperties(&p, dev));
  // the U <= 64 instantiation holds the larger LDS tables: where it exists its residency bounds both
  if constexpr (split_umax_ks<KS>() > kGsUMax)
    ONI_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &per_cu, reinterpret_cast<const void*>(&gs::gs_splitw<KS, split_umax_ks<KS>()>), 512, 0));
  else
    ONI_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &per_cu, reinterpret_cast<const void*>(&gs::gs_splitw<KS>), 512, 0));
  return per_cu * p.multiProcessorCount;
}

int gs_split_capacity(int KS) {
  switch (KS) {
#define ONI_KS(X) \
  case X:         \
    return gs_split_capacity_ks<X>();
    ONI_FOR_EACH_KS(ONI_KS)
#undef ONI_KS
    default:
      throw std::runtime_error("gs_split_capacity: unsupported KS " + std::to_string(KS));
  }
}

void launch_gs_split(const GSArgs& a, const SplitArgs& s, int KS, hipStream_t st) {
  if (s.n_blocks <= 0) return;
  const int um = gs_split_umax(KS);
  if (a.gs_updates < 1 || a.gs_updates > um)
    throw std::runtime_error("gs_split: gs_updates must be in [1, " + std::to_string(um) + "] at KS " +
                             std::to_string(KS));
  if (!a.params) throw std::runtime_error("gs_split: params block required");
  switch (KS) {
#define ONI_KS(X)                                                                                          \
  case X:                                                                                                  \
    if (a.gs_updates > split_umax_ks<X>()) {                                                               \
      if constexpr (X > 32) {                                                                              \
        if (!s.tab) throw std::runtime_error("gs_split: U past the LDS chunk tables needs the tab scratch");   \
        hipLaunchKernelGGL((gs::gs_splitw<X, kGsUMax, true>), dim3(s.n_blocks), dim3(512), 0, st, a, s);   \
      }                                                                                                    \
    } else if (a.gs_updates > kGsUMax) {                                                                   \
      if constexpr (split_umax_ks<X>() > kGsUMax)                                                          \
        hipLaunchKernelGGL((gs::gs_splitw<X, split_umax_ks<X>()>), dim3(s.n_blocks), dim3(512), 0, st, a, s); \
    } else                                                                                                 \
      hipLaunchKernelGGL((gs::gs_splitw<X>), dim3(s.n_blocks), dim3(512), 0, st, a, s);                    \
    break;
    ONI_FOR_EACH_KS(ONI_KS)
#undef ONI_KS
    default:
      throw std::runtime_error("gs_split: unsupported KS " + std::to_string(KS));
  }
  ONI_HIP_CHECK(hipGetLastError());
}

}  // namespace oni
