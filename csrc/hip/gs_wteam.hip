// fp64 block Gauss-Seidel E-step, the word-per-lane kernels of KS <= 32 at U <= 32: gs_wteam (one wave per
// document) and gs_wsteam (the longest documents: 7 word waves + a topic wave).  Chunk algebra and schedule:
// header of lda_gs64.hip.
#include <stdexcept>
#include <string>

#include "common.h"
#include "gs_families.h"
#include "gs_layout.h"
#include "gs_math.h"
#include "kernels.h"

namespace oni {
namespace gs {

// ------------------------------------------------------------- word team ----
// Word-per-lane team kernel for KS <= 32: every lane owns whole words (all KS topics in
// registers), so a word costs 2 KS FMAs, one reciprocal and one log per LANE instead of per
// topic group (the topic-group layout repeats the reciprocal, the log and the cross-lane P sum
// on TG lanes).  The per-chunk topic sums are a register reduce-scatter per wave
// (wave_topic_sums), then the topic owners add the waves in order.  Rows of the next chunk are
// prefetched as in gs_team.
constexpr int wteam_dpb(int NW) { return 1; }
constexpr int wteam_threads(int NW) { return wteam_dpb(NW) * NW * 64; }

template <int KS, int N>
__device__ __forceinline__ void wword_steps(const double (&E)[KS], const double (*b)[KS], const double* c,
                                            double (&acc)[KS], double& lw) {
  double P[N];
#pragma unroll
  for (int u = 0; u < N; ++u) {
    double p0 = 0.0, p1 = 0.0, p2 = 0.0, p3 = 0.0;
#pragma unroll
    for (int k = 0; k < KS; k += 4) {
      p0 = fma(E[k], b[u][k], p0);
      if (k + 1 < KS) p1 = fma(E[k + 1], b[u][k + 1], p1);
      if (k + 2 < KS) p2 = fma(E[k + 2], b[u][k + 2], p2);
      if (k + 3 < KS) p3 = fma(E[k + 3], b[u][k + 3], p3);
    }
    P[u] = (p0 + p1) + (p2 + p3);
  }
#pragma unroll
  for (int u = 0; u < N; ++u) {
    const double Pu = c[u] > 0.0 ? P[u] : 1.0;
    const double r = c[u] * drcp(Pu);
    lw = fma(c[u], flog(Pu), lw);
#pragma unroll
    for (int k = 0; k < KS; ++k) acc[k] = fma(r, b[u][k], acc[k]);
  }
}

// the row of word position p from a staged document copy ([n/64][KS/2][64] double2 tiles,
// launch_gs_stage): 64 consecutive positions are 16-byte-contiguous per topic pair, so a wave's
// gather of 64 words touches ~9 cache lines per instruction instead of 64 rows' worth
template <int KS>
__device__ __forceinline__ void load_row_staged(const dvec2* __restrict__ s, int p, double (&b)[KS]) {
  const dvec2* q = s + (size_t)(p >> 6) * (KS / 2) * 64 + (p & 63);
#pragma unroll
  for (int k = 0; k < KS / 2; ++k) {
    const dvec2 v = q[k * 64];
    b[2 * k] = v.x;
    b[2 * k + 1] = v.y;
  }
}

template <int KS>
__device__ __forceinline__ void load_row_full(const double* __restrict__ beta, int w, double (&b)[KS]) {
  const double2* p = reinterpret_cast<const double2*>(beta + (size_t)w * KS);
#pragma unroll
  for (int k = 0; k < KS / 2; ++k) {
    const double2 v = p[k];
    b[2 * k] = v.x;
    b[2 * k + 1] = v.y;
  }
}

template <int KS, int NW, int RMAX>
__global__ __launch_bounds__(wteam_threads(NW)) void gs_wteam(GSArgs a) {
  static_assert(KS <= 32 && KS % 2 == 0, "word team: KS <= 32");
  constexpr int DPB = wteam_dpb(NW), NTD = NW * 64, NS = NTD;
  __shared__ double sC[DPB][kGsUMax][KS];
  __shared__ double sEt[DPB][kGsUMax][KS];
  __shared__ double sE[DPB][KS];
  __shared__ double sRed[DPB][NW][KS];
  __shared__ double sCs[DPB][kGsUMax];
  __shared__ double sScal[DPB][NW][4];
  if (a.params[kParamDone] != 0.0) return;
  const int t = threadIdx.x % NTD, ds = threadIdx.x / NTD;
  const int item = blockIdx.x * DPB + ds;
  if (item >= a.n_items) return;
  const int d = a.order[item];
  if (d < 0) return;   // placement gap (GSPlan.isolate_longest)
  const double alpha = a.params[0], lik_const = a.params[1];
  const int vmi = (int)a.params[2];
  const double vconv = params_vconv(a.params);
  const int K = a.K;
  const int lane = t & 63, wv = t >> 6;
  const int s0 = a.doc_ptr[d], n = a.doc_ptr[d + 1] - s0;
  const int U = a.gs_updates;
  const int W = n > 0 ? (n + U - 1) / U : 1;
  const int nch = (n + W - 1) / W;
  const int nact = min(NW, (W + 63) / 64);
  const bool active = wv < nact;
  const int* __restrict__ wrow = a.word_idx + s0;
  const float* __restrict__ crow = a.counts + s0;
  double(*C)[KS] = sC[ds];
  double(*Et)[KS] = sEt[ds];
  double* E_ = sE[ds];
  double* Cs = sCs[ds];
  for (int j = t; j < nch; j += NTD) Cs[j] = 0.0;
  team_sync<NW>();
  for (int p = t; p < n; p += NTD) atomicAdd(&Cs[p / W], (double)crow[p]);
  team_sync<NW>();
  double total = 0.0;
  for (int j = 0; j < nch; ++j) total += Cs[j];
  const double g0 = alpha + total / K;
  const double m = psi_only(g0);
  // topic owner: thread t < KS (wave 0)
  const int k = t;
  double gam = k < K ? g0 : 0.0, psi = m, lps = 0.0;
  if (k < KS) {
    E_[k] = k < K ? 1.0 : 0.0;
    for (int j = 0; j < nch; ++j) C[j][k] = k < K ? Cs[j] / K : 0.0;
  }
  int wc[RMAX], wn[RMAX];
  float cc[RMAX], cn[RMAX];
  unsigned vc = 0, vn = 0;
  double bc[RMAX][KS];
  auto load_ids = [&](int j, int (&w)[RMAX], float (&c)[RMAX], unsigned& v) {
    const int n0 = j * W, n1 = min(n, n0 + W);
    v = 0;
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
      const int p = n0 + t + r * NS;
      v |= (active && p < n1) ? (1u << r) : 0u;
      // rounds past the chunk end re-read the chunk's last word: the same address as a valid
      // lane, so no extra row is gathered (clamping to the document end fetched the next chunk's rows)
      const int pc = min(p, n1 - 1);
      w[r] = wrow[pc];
      c[r] = crow[pc];
    }
  };
  // rounds without a word (past the chunk end) load nothing: exec-masked lanes return no data, and
  // the row return path (64 B/clk per CU) is what a chunk's word phase waits on
  auto load_rows = [&](const int (&w)[RMAX], unsigned v) {
    if (!active) return;   // wave-uniform
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
      if ((v >> r) & 1u) {
        load_row_full<KS>(a.beta, w[r], bc[r]);
      } else {
#pragma unroll
        for (int k = 0; k < KS; ++k) bc[r][k] = 0.0;
      }
    }
  };
  if (nch > 0) {
    load_ids(0, wc, cc, vc);
    load_rows(wc, vc);
    load_ids(nch > 1 ? 1 : 0, wn, cn, vn);
  }
  team_sync<NW>();
  double L = 0.0, L_old = 0.0, conv = 1.0, GS = 0.0;
  int it = 0;
  const bool timer = a.dbg != nullptr && blockIdx.x == 0 && threadIdx.x == 0;
  long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  long long tc = timer ? clock64() : 0;
  auto tick = [&](int i) {
    if (timer) {
      const long long x = clock64();
      ph[i] += x - tc;
      tc = x;
    }
  };
  while (var_continue(conv, vconv, it, vmi)) {
    ++it;
    double lw = 0.0;
    lps = 0.0;
    for (int j = 0; j < nch; ++j) {
      ph[7] += timer ? 1 : 0;
      if (active) {
        const int n0 = j * W, n1 = min(n, n0 + W);
        double E[KS], acc[KS];
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) {
          E[kk] = E_[kk];
          acc[kk] = 0.0;
        }
        double cr[RMAX];
#pragma unroll
        for (int r = 0; r < RMAX; ++r) cr[r] = ((vc >> r) & 1u) ? (double)cc[r] : 0.0;
        if (RMAX == 1 || n1 - n0 <= NS)
          wword_steps<KS, 1>(E, bc, cr, acc, lw);
        else
          wword_steps<KS, RMAX>(E, bc, cr, acc, lw);
        for (int p = n0 + t + RMAX * NS; p < n1; p += NS) {   // beyond the prefetched rounds
          double b[1][KS];
          load_row_full<KS>(a.beta, wrow[p], b[0]);
          const double cp = (double)crow[p];
          wword_steps<KS, 1>(E, b, &cp, acc, lw);
        }
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
        tick(0);
        wave_topic_sums<KS>(acc, lane, sRed[ds][wv]);
        tick(1);
      }
      team_sync<NW>();
      tick(2);
      if (k < KS) {
        double S = 0.0;
#pragma unroll
        for (int v = 0; v < NW; ++v) S += v < nact ? sRed[ds][v][k] : 0.0;
        const double Eo = E_[k];
        const double nw = Eo * S;
        double En = 0.0;
        if (k < K) {
          lps = fma(psi, nw, lps);
          gam += nw - C[j][k];
          psi_exp(gam, m, psi, En);
        }
        C[j][k] = nw;
        Et[j][k] = Eo;
        E_[k] = En;
      }
      tick(3);
      team_sync<NW>();
      tick(4);
    }
    const bool own = k < K;
    const double w0 = group_sum<64>(lw);
    const double w1 = group_sum<64>(own ? gam : 0.0), w2 = group_sum<64>(own ? lgamma_pos(gam) : 0.0);
    const double w3 = group_sum<64>(own ? lps : 0.0);
    if (lane == 0) {
      sScal[ds][wv][0] = w0;
      sScal[ds][wv][1] = w1;
      sScal[ds][wv][2] = w2;
      sScal[ds][wv][3] = w3;
    }
    team_sync<NW>();
    double LW = 0.0, LG = 0.0, LP = 0.0;
    GS = 0.0;
#pragma unroll
    for (int v = 0; v < NW; ++v) {
      LW += sScal[ds][v][0];
      GS += sScal[ds][v][1];
      LG += sScal[ds][v][2];
      LP += sScal[ds][v][3];
    }
    L = lik_const - lgamma_pos(GS) + LG + fma(m, total, LW) - LP;
    conv = (L_old - L) / L_old;
    L_old = L;
    team_sync<NW>();
    tick(5);
  }
  if (timer)
    for (int i = 0; i < 8; ++i) a.dbg[i] = ph[i];
  const double ps = group_sum<64>(k < K ? psi : 0.0);
  if (k < KS) a.gamma[(size_t)d * KS + k] = gam;
  if (lane == 0) sScal[ds][wv][0] = ps;
  team_sync<NW>();
  if (t == 0) {
    double PS = 0.0;
    for (int v = 0; v < NW; ++v) PS += sScal[ds][v][0];
    a.lik[d] = L;
    a.alpha_ss[d] = PS - K * psi_only(GS);
    a.iters[d] = it;
  }
  if (!active) return;
  for (int j = 0; j < nch; ++j) {
    const int n0 = j * W, n1 = min(n, n0 + W);
    double E[KS];
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) E[kk] = Et[j][kk];
    for (int p = n0 + t; p < n1; p += NS) {
      double b[KS];
      load_row_full<KS>(a.beta, wrow[p], b);
      double p0 = 0.0, p1 = 0.0, p2 = 0.0, p3 = 0.0;
#pragma unroll
      for (int kk = 0; kk < KS; kk += 4) {
        p0 = fma(E[kk], b[kk], p0);
        if (kk + 1 < KS) p1 = fma(E[kk + 1], b[kk + 1], p1);
        if (kk + 2 < KS) p2 = fma(E[kk + 2], b[kk + 2], p2);
        if (kk + 3 < KS) p3 = fma(E[kk + 3], b[kk + 3], p3);
      }
      const double r = (double)crow[p] * drcp((p0 + p1) + (p2 + p3));
      dvec2* row = reinterpret_cast<dvec2*>(a.cphi + (size_t)(s0 + p) * KS);
#pragma unroll
      for (int kk = 0; kk < KS / 2; ++kk) {
        const dvec2 v = {E[2 * kk] * b[2 * kk] * r, E[2 * kk + 1] * b[2 * kk + 1] * r};
        __builtin_nontemporal_store(v, &row[kk]);
      }
    }
  }
}

// ------------------------------------------------- word team, topic wave ----
// The longest documents (gs_wteam measured: ~8.7k cycles per chunk, the critical path of the
// E-step).  NW word waves own the words; one extra TOPIC WAVE owns the K topics and runs the
// refresh.  The two roles run separate loops with the same barrier sequence, so:
//  - the word waves' registers (E, accumulators, the next chunk's prefetched rows) are not live
//    in the refresh code, which therefore needs no spills; in gs_wteam the refresh ran in wave 0
//    beside 256 live VGPRs and its spill reloads waited (vmcnt is in order) behind the next
//    chunk's row prefetch;
//  - the topic wave issues no global loads, so nothing queues in front of its LDS traffic;
//  - the word waves take log P of their words (only the sweep likelihood needs it) while the
//    topic wave refreshes, off the chunk's critical path.
// Arithmetic per word and per topic is that of gs_wteam (the likelihood's lw partial sums are
// grouped by wave, so the two kernels agree to rounding, not bitwise).
// EP (early prefetch): rounds u < EP of the next chunk's rows are gathered
// into bc[u] as soon as the axpy of round u has consumed them -- before the topic sums and the
// arrival -- so the address unit works beside the reduction; the other rounds after the arrival.
// Outside the sweeps (profiles/defer_final.md), both optional and bitwise neutral: the chunk count sums
// come from the plan's table (GSArgs::csum) instead of a pass over the document's counts, and the final
// pass (every entry's c*phi row: re-reading all rows and writing as many on this one CU) is left to the
// suff-stats pass when GSArgs::et is set -- the topic wave then copies out Et, the E each chunk used.
// (Measured slower and removed in round 5, records in profiles/r4_tuning_log.md: the topic wave summing
// the word waves' lane partials, 5 or 3 word waves, two early rounds, the LDS-ring loader variant.)
template <int KS, int NW, int RMAX, int EP = 0, bool STG = false>
__global__ __launch_bounds__((NW + 1) * 64) void gs_wsteam(GSArgs a) {
  static_assert(KS <= 32 && KS % 2 == 0, "word team: KS <= 32");
  constexpr int NTD = (NW + 1) * 64, NS = NW * 64;
  __shared__ double C[kGsUMax][KS];     // chunk contributions (previous sweep)
  __shared__ double Et[kGsUMax][KS];    // E each chunk used (final pass)
  __shared__ double E_[KS];             // current E, broadcast
  __shared__ double sRed[NW][KS];       // per-wave topic sums of a chunk
  __shared__ double Cs[kGsUMax];        // chunk count sums
  __shared__ double sScal[NW + 1][4];   // sweep partials: lw per word wave; gamma sums (topic wave)
  __shared__ int arrive[NW];            // per word wave: chunks whose topic sums it has left in sRed
  __shared__ int sDefer;                // a.et != nullptr, for the word waves after their sweeps: read from LDS
                                        // so that no kernel argument more stays live in SGPRs across the chunk
                                        // loop (the kernel is at the SGPR limit; profiles/defer_final.md)
  if (a.params[kParamDone] != 0.0) return;
  const int t = threadIdx.x;
  const int d = a.order[blockIdx.x];
  if (d < 0) return;                    // placement gap (GSPlan.isolate_longest): whole workgroup
  const double alpha = a.params[0], lik_const = a.params[1];
  const int vmi = (int)a.params[2];
  const double vconv = params_vconv(a.params);
  const int K = a.K;
  auto kc_ = [](int k) { return k < KS ? k : KS - 1; };   // an in-bounds LDS column for guarded reads
  const int lane = t & 63, wv = t >> 6;
  const bool topic_wave = wv == NW;
  const int s0 = a.doc_ptr[d], n = a.doc_ptr[d + 1] - s0;
  const int U = a.gs_updates;
  const int W = n > 0 ? (n + U - 1) / U : 1;
  const int nch = (n + W - 1) / W;
  const int nact = min(NW, (W + 63) / 64);
  const bool active = wv < nact;        // word waves holding words of a chunk (never the topic wave)
  const int* __restrict__ wrow = a.word_idx + s0;
  const float* __restrict__ crow = a.counts + s0;
  // chunk count sums: constants of the corpus, taken from the plan's table (a.csum, nch plain loads) when
  // there is one; else summed here, one exposed global load and one LDS atomic per word and thread
  const double* __restrict__ cs = a.csum != nullptr ? a.csum + (size_t)blockIdx.x * kGsUMax : nullptr;
  for (int j = t; j < nch; j += NTD) Cs[j] = cs != nullptr ? cs[j] : 0.0;
  if (t < NW) arrive[t] = 0;
  if (t == NTD - 1) sDefer = a.et != nullptr;
  lds_barrier();
  if (cs == nullptr) {   // workgroup-uniform
    for (int p = t; p < n; p += NTD) atomicAdd(&Cs[p / W], (double)crow[p]);   // integer counts: exact
    lds_barrier();
  }
  double total = 0.0;
  for (int j = 0; j < nch; ++j) total += Cs[j];
  const double g0 = alpha + total / K;
  const double m = psi_only(g0);
  const bool timer = a.dbg != nullptr && blockIdx.x == 0 && t == 0;
  long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  long long tc = timer ? clock64() : 0;
  auto tick = [&](int i) {
    if (timer) {
      const long long x = clock64();
      ph[i] += x - tc;
      tc = x;
    }
  };
  double L = 0.0, L_old = 0.0, conv = 1.0, GS = 0.0;
  int it = 0;
  // sweep likelihood from the partials every wave left in sScal (same order in every thread)
  auto sweep_end = [&]() {
    lds_barrier();
    double LW = 0.0;
#pragma unroll
    for (int v = 0; v < NW; ++v) LW += sScal[v][0];
    GS = sScal[NW][1];
    L = lik_const - lgamma_pos(GS) + sScal[NW][2] + fma(m, total, LW) - sScal[NW][3];
    conv = (L_old - L) / L_old;
    L_old = L;
    lds_barrier();
  };
  if (topic_wave) {
    // ------------------------------------------------------------ topic wave
    __builtin_amdgcn_s_setprio(3);   // its chain is the critical path; the word waves wait on it
    const int k = lane;
    int want = 0;
    // dbg[8..11] (the int64[16] timer of gs_estep): this wave's cycles waiting for the arrivals,
    // summing + refreshing, and at barrier B, summed over chunks
    const bool ttimer = a.dbg != nullptr && blockIdx.x == 0 && lane == 0;
    long long tph[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // [4 + i]: chunk start -> wave v_i's arrival seen
    long long ttc = ttimer ? clock64() : 0;
    auto ttick = [&](int i) {
      if (ttimer) {
        const long long x = clock64();
        tph[i] += x - ttc;
        ttc = x;
      }
    };
    double gam = k < K ? g0 : 0.0, psi = m, lps = 0.0;
    // this lane's E_k stays in a register (the wave is E_'s only writer), and C_jk is read before
    // the arrival wait: after the last arrival only the sRed loads precede the refresh chain
    double Ecur = k < K ? 1.0 : 0.0;
    if (k < KS) {
      E_[k] = Ecur;
      for (int j = 0; j < nch; ++j) C[j][k] = k < K ? Cs[j] / K : 0.0;
    }
    lds_barrier();   // (1) E_ and C ready; word waves' first rows in flight
    while (var_continue(conv, vconv, it, vmi)) {
      ++it;
      lps = 0.0;
      for (int j = 0; j < nch; ++j) {
        // (A) the nact word waves' topic sums of chunk j are in sRed: summed in wave order as each
        // wave arrives, so after the last arrival one add remains (not nact dependent adds)
        ++want;
        ttick(3);
        const double gC = k < KS ? gam - C[j][k] : 0.0;
        double S = 0.0;
#pragma unroll
        for (int v = 0; v < NW; ++v) {
          if (v < nact) {
            while (__hip_atomic_load(&arrive[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < want)
              __builtin_amdgcn_s_sleep(1);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
            if (ttimer && (v == 0 || v == 3 || v == 4 || v == nact - 1))
              tph[v == 0 ? 4 : v == 3 ? 5 : v == 4 ? 6 : 7] += clock64() - ttc;
            S += k < KS ? sRed[v][k] : 0.0;
          }
        }
        ttick(0);
        if (k < KS) {
          const double Eo = Ecur;
          const double nw = Eo * S;
          double En = 0.0;
          if (k < K) {
            lps = fma(psi, nw, lps);
            gam = fma(Eo, S, gC);   // gamma_k + (new_jk - C_jk) in one rounding, off the nw product
            psi_exp(gam, m, psi, En);
          }
          E_[k] = En;
          C[j][k] = nw;
          Et[j][k] = Eo;
          Ecur = En;
        }
        ttick(1);
        lds_barrier();   // (B) E of chunk j + 1 published
        ttick(2);
      }
      const bool own = k < K;
      const double w1 = group_sum<64>(own ? gam : 0.0), w2 = group_sum<64>(own ? lgamma_pos(gam) : 0.0);
      const double w3 = group_sum<64>(own ? lps : 0.0);
      if (lane == 0) {
        sScal[NW][1] = w1;
        sScal[NW][2] = w2;
        sScal[NW][3] = w3;
      }
      sweep_end();
    }
    if (ttimer)
      for (int i = 0; i < 8; ++i) a.dbg[8 + i] = tph[i];
    const double ps = group_sum<64>(k < K ? psi : 0.0);
    if (k < KS) a.gamma[(size_t)d * KS + k] = gam;
    if (lane == 0) {
      a.lik[d] = L;
      a.alpha_ss[d] = ps - K * psi_only(GS);
      a.iters[d] = it;
    }
    // deferred final pass (a.et): the E each chunk used in the final sweep -- this wave's own Et -- leaves for
    // the suff-stats pass, which recomputes this document's c*phi rows on the whole GPU (gs_suff64 RECOMP)
    // instead of this one CU writing and that pass re-reading them
    if (a.et != nullptr && k < KS) {
      double* __restrict__ eo = a.et + (size_t)blockIdx.x * kGsUMax * KS;
      for (int j = 0; j < nch; ++j) eo[j * KS + k] = Et[j][k];
    }
    return;
  }
  // -------------------------------------------------------------- word waves
  // STG: rows come from the document's staged copy (launch_gs_stage) indexed by word position, so
  // the ids below are positions; otherwise they are vocabulary ids into beta
  const dvec2* stg = nullptr;
  if constexpr (STG) stg = reinterpret_cast<const dvec2*>(a.stage) + a.stage_off[blockIdx.x];
  auto row_of = [&](int p) { return STG ? p : wrow[p]; };
  auto load_row = [&](int id, double(&b)[KS]) {
    if constexpr (STG)
      load_row_staged<KS>(stg, id, b);
    else
      load_row_full<KS>(a.beta, id, b);
  };
  int wc[RMAX], wn[RMAX];
  float cc[RMAX], cn[RMAX];
  unsigned vc = 0, vn = 0;
  double bc[RMAX][KS];
  auto load_ids = [&](int j, int (&w)[RMAX], float (&c)[RMAX], unsigned& v) {
    const int n0 = j * W, n1 = min(n, n0 + W);
    v = 0;
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
      const int p = n0 + t + r * NS;
      v |= (active && p < n1) ? (1u << r) : 0u;
      const int pc = min(p, n1 - 1);
      w[r] = row_of(pc);
      c[r] = crow[pc];
    }
  };
  auto load_rows = [&](const int (&w)[RMAX], unsigned v) {
    if (!active) return;   // wave-uniform
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
      if ((v >> r) & 1u) {   // rounds past the chunk end gather nothing
        load_row(w[r], bc[r]);
      } else {
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) bc[r][kk] = 0.0;
      }
    }
  };
  if (nch > 0) {
    load_ids(0, wc, cc, vc);
    load_rows(wc, vc);
    load_ids(nch > 1 ? 1 : 0, wn, cn, vn);
  }
  lds_barrier();   // (1)
  while (var_continue(conv, vconv, it, vmi)) {
    ++it;
    double lw = 0.0;
    for (int j = 0; j < nch; ++j) {
      ph[7] += timer ? 1 : 0;
      double P[RMAX], cr[RMAX];
      if (active) {
        const int n0 = j * W, n1 = min(n, n0 + W);
        double E[KS], acc[KS];
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) {
          E[kk] = E_[kk];
          acc[kk] = 0.0;
        }
#pragma unroll
        for (int r = 0; r < RMAX; ++r) cr[r] = ((vc >> r) & 1u) ? (double)cc[r] : 0.0;
        // dot, reciprocal and axpy now; log P after barrier A (beside the refresh)
#pragma unroll
        for (int u = 0; u < RMAX; ++u) {
          double p0 = 0.0, p1 = 0.0, p2 = 0.0, p3 = 0.0;
#pragma unroll
          for (int kk = 0; kk < KS; kk += 4) {
            p0 = fma(E[kk], bc[u][kk], p0);
            if (kk + 1 < KS) p1 = fma(E[kk + 1], bc[u][kk + 1], p1);
            if (kk + 2 < KS) p2 = fma(E[kk + 2], bc[u][kk + 2], p2);
            if (kk + 3 < KS) p3 = fma(E[kk + 3], bc[u][kk + 3], p3);
          }
          P[u] = cr[u] > 0.0 ? (p0 + p1) + (p2 + p3) : 1.0;
        }
        if (timer) {   // split of the word phase: E read + dot | reciprocal + axpy + prefetch issue
          __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0) only... values consumed below anyway
          const long long x = clock64();
          ph[6] += x - tc;
          tc = x;
        }
#pragma unroll
        for (int u = 0; u < RMAX; ++u) {
          const double r = cr[u] * drcp(P[u]);
#pragma unroll
          for (int kk = 0; kk < KS; ++kk) acc[kk] = fma(r, bc[u][kk], acc[kk]);
          if (u < EP) {   // bc[u] is free: the next chunk's round u (ids already here)
            __builtin_amdgcn_sched_barrier(0);   // keep the gather below the axpy (no second row set)
            if ((vn >> u) & 1u) {
              load_row(wn[u], bc[u]);
            } else {
#pragma unroll
              for (int kk = 0; kk < KS; ++kk) bc[u][kk] = 0.0;
            }
          }
        }
        for (int p = n0 + t + RMAX * NS; p < n1; p += NS) {   // beyond the prefetched rounds
          double b[1][KS];
          load_row(row_of(p), b[0]);
          const double cp = (double)crow[p];
          wword_steps<KS, 1>(E, b, &cp, acc, lw);
        }
        tick(0);
        wave_topic_sums<KS>(acc, lane, sRed[wv]);
        // (A) arrival: this wave's topic sums are in sRed.  A counter instead of a workgroup barrier,
        // so the refresh starts while the word waves are still issuing the next chunk's row loads
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");   // LDS only: no vmcnt wait
        if (lane == 0) __hip_atomic_fetch_add(&arrive[wv], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        tick(1);
        // prefetch of the next chunk's rows: a chunk's ~700 row gathers keep the CU's address unit busy
        // for ~2k cycles (64 B/clk) and the issuing wave blocks until they are queued -- now beside the
        // refresh instead of before it
        const int j1 = j + 1 < nch ? j + 1 : 0;
        const int j2 = j1 + 1 < nch ? j1 + 1 : 0;
#pragma unroll
        for (int r = 0; r < RMAX; ++r) {
          wc[r] = wn[r];
          cc[r] = cn[r];
        }
        vc = vn;
        if constexpr (EP == 0) {
          load_rows(wc, vc);
        } else if (active) {
#pragma unroll
          for (int r = EP; r < RMAX; ++r) {
            if ((vc >> r) & 1u) {
              load_row(wc[r], bc[r]);
            } else {
#pragma unroll
              for (int kk = 0; kk < KS; ++kk) bc[r][kk] = 0.0;
            }
          }
        }
        load_ids(j2, wn, cn, vn);
        tick(2);
#pragma unroll
        for (int u = 0; u < RMAX; ++u) lw = fma(cr[u], flog(P[u]), lw);
      }
      tick(3);
      lds_barrier();   // (B)
      tick(4);
    }
    const double w0 = group_sum<64>(lw);
    if (lane == 0) sScal[wv][0] = w0;
    sweep_end();
    tick(5);
  }
  if (timer)
    for (int i = 0; i < 8; ++i) a.dbg[i] = ph[i];
  if (sDefer) return;   // deferred final pass (workgroup-uniform): the topic wave has left Et in a.et
  // final pass: c_n phi_nk = E_jk b_nk r_n with the final sweep's chunk E (same P as the sweep)
  if (!active) return;
  for (int j = 0; j < nch; ++j) {
    const int n0 = j * W, n1 = min(n, n0 + W);
    double E[KS];
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) E[kk] = Et[j][kk];
    for (int p = n0 + t; p < n1; p += NS) {
      double b[KS], v[KS];
      load_row(row_of(p), b);
      cphi_row<KS, 1>(E, b, (double)crow[p], v);
      dvec2* row = reinterpret_cast<dvec2*>(a.cphi + (size_t)(s0 + p) * KS);
#pragma unroll
      for (int kk = 0; kk < KS / 2; ++kk) __builtin_nontemporal_store(dvec2{v[2 * kk], v[2 * kk + 1]}, &row[kk]);
    }
  }
}

}  // namespace gs

// ------------------------------------------------------------------ launch ---
void launch_gs_wteam(const GSArgs& a, int KS, hipStream_t s) {
  switch (KS) {
    // one wave per document, a word per lane, in-wave refresh: 2.128 / 2.129 / 2.143 vs 2.136 / 2.141 /
    // 2.144 ms per EM iteration for 3 word waves + a topic wave (3 A/B rounds, profiles/r3_tuning_log.md):
    // a quarter of the waves for the same chains leaves the CUs to the other buckets
#define ONI_KS(X)                                                                             \
  case X:                                                                                     \
    if constexpr (X <= 32)                                                                    \
      hipLaunchKernelGGL((gs::gs_wteam<X, 1, 1>), dim3(a.n_items), dim3(64), 0, s, a);        \
    else                                                                                      \
      throw std::runtime_error("gs_wteam: one word per lane needs KS <= 32");                 \
    break;
    ONI_FOR_EACH_KS(ONI_KS)
#undef ONI_KS
    default:
      throw std::runtime_error("gs_estep: unsupported KS " + std::to_string(KS));
  }
  ONI_HIP_CHECK(hipGetLastError());
}

template <int KS>
static void gs_wsteam_ks(const GSArgs& a, hipStream_t s) {
  // longest documents: 7 word waves x 2 prefetched words per lane + a topic wave (5 x 3: 2.64 ms, 3 x 4:
  // 2.06 ms vs 1.74 per headline EM iteration; profiles/r4_tuning_log.md).  Staged rows (GSStage): every
  // next-chunk round gathered after the arrival (1.726-1.740 vs 1.824-1.833 ms for an early round-0
  // gather); rows gathered from beta (a plan past the staging budget): round 0 early (2.13-2.14 vs
  // 2.17-2.18 ms).  The LDS-ring and topic-wave-reduction variants were slower and are gone.
  if constexpr (KS <= 32) {
    if (a.stage != nullptr)
      hipLaunchKernelGGL((gs::gs_wsteam<KS, 7, 2, 0, true>), dim3(a.n_items), dim3(512), 0, s, a);
    else
      hipLaunchKernelGGL((gs::gs_wsteam<KS, 7, 2, 1>), dim3(a.n_items), dim3(512), 0, s, a);
  } else {
    throw std::runtime_error("gs_wsteam: one word per lane needs KS <= 32");
  }
}

void launch_gs_wsteam(const GSArgs& a, int KS, hipStream_t s) {
  switch (KS) {
#define ONI_KS(X)          \
  case X:                  \
    gs_wsteam_ks<X>(a, s); \
    break;
    ONI_FOR_EACH_KS(ONI_KS)
#undef ONI_KS
    default:
      throw std::runtime_error("gs_estep: unsupported KS " + std::to_string(KS));
  }
  ONI_HIP_CHECK(hipGetLastError());
}

}  // namespace oni
