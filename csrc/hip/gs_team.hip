// fp64 block Gauss-Seidel E-step, the team kernel (chunk algebra and schedule: header of lda_gs64.hip).
//   gs_team   one wave / 4-wave / 8-wave workgroup per document.  Lanes are
//             (topic group q) x (word slot sl) with the slot in the low lane bits:
//             a word's P is an xor-16/32 (permlane swap) reduction over q, the slot
//             reduction of S is a row DPP reduction; cross-wave sums go through LDS in
//             wave order (bitwise reproducible).  Topic owners (one thread per topic)
//             run the refresh and broadcast E through LDS.
// Lane layout, row loads and the word phase (shared with gs_split.hip): gs_layout.h.
#include <stdexcept>
#include <string>

#include "common.h"
#include "gs_families.h"
#include "gs_layout.h"
#include "gs_math.h"
#include "kernels.h"

namespace oni {
namespace gs {

// ------------------------------------------------------------------ team ----
constexpr int team_threads(int KS, int NW) { return ((NW == 1 && KS <= 32) ? 4 : 1) * NW * 64; }

// MINW: minimum waves per SIMD requested from the register allocator (the LDS-free one-wave team
// at K > 32 is latency-bound on its per-word refresh chains: 3 waves per SIMD, 13.2 -> 11.7 ms on the
// K = 100 shard; 4 spilled, 19.5 ms -- profiles/r2_k100_split.md)
template <int KS, int NW, int MINW = 1, bool GMT = false>
__global__ __launch_bounds__(team_threads(KS, NW), MINW) void gs_team(GSArgs a) {
  using T = TeamShape<KS, NW>;
  // (KS <= 32 GMT, the parity mode: 4 / 2 prefetched rounds -- 8 spilled 284 bytes at KS = 20, 4 at KS 24-32)
  constexpr int DPB = T::DPB, NTD = T::NTD, TG = T::TG, KPL = T::KPL, NSW = T::NSW, LSW = T::LSW, NS = T::NS,
                TO = T::TO, RMAX = (GMT && KS <= 32) ? (T::RMAX < (KS <= 20 ? 4 : 2) ? T::RMAX : (KS <= 20 ? 4 : 2))
                                                         : T::RMAX;
  constexpr bool PAIR = T::PAIR;
  // GM (one-wave documents at KS > 32, and every team size when GMT: U > kGsUMax refreshes per
  // sweep): the chunk tables live in the document's own c*phi rows instead of LDS (2 x 32 x KS
  // doubles of LDS held one wave per CU to ~3 waves; U chunks of them do not fit at all): C_j in
  // row j W, the E chunk j used in row j W + 1 (chunks of >= 2 words).  A one-word chunk's C_j IS
  // that word's c*phi (E_j r b), so documents of <= U words need no final pass at all.
  constexpr bool GM = GMT || (NW == 1 && KS > 32);
  // KS <= 32 with U > kGsUMax (lda-c's per-word schedule at K <= 32): the 4- and 8-wave teams only (DPB == 1,
  // so the early returns stay workgroup-uniform); the one-wave range goes to gs_chain there
  static_assert(!GMT || KS > 32 || NW > 1, "U > kGsUMax at KS <= 32: 4- and 8-wave team kernels only");
  constexpr int UT = GM ? 1 : kGsUMax;
  __shared__ double sC[DPB][UT][KS];         // chunk contributions (previous sweep)
  __shared__ double sEt[DPB][UT][KS];        // E each chunk used (final pass)
  __shared__ double sE[DPB][KS];             // current E, broadcast
  __shared__ double sRed[DPB][NW][KS];       // per-wave slot sums
  __shared__ double sCs[DPB][UT];            // chunk count sums (GM: straight into the C_j rows)
  __shared__ double sScal[DPB][NW][4];       // per-wave sweep partials
  // KS > 32: flog_t's table for the per-word log and the refresh (DPB == 1 there: the workgroup is one
  // document, so every early return below is workgroup-uniform)
  constexpr bool TAB = KS > 32;
  __shared__ dvec2 sLog[TAB ? kMathTabN : 1];
  if (a.params[kParamDone] != 0.0) return;
  if constexpr (TAB) {
    log_table_fill(sLog);
    __syncthreads();
  }
  const int t = threadIdx.x % NTD, ds = threadIdx.x / NTD;
  const int item = blockIdx.x * DPB + ds;
  if (item >= a.n_items) return;             // NW == 1: one wave per document (no block barriers)
  const double alpha = a.params[0], lik_const = a.params[1];
  const int vmi = (int)a.params[2];
  const double vconv = params_vconv(a.params);
  const int K = a.K;
  const int lane = t & 63, wv = t >> 6;
  const int q = lane >> LSW, sl = lane & (NSW - 1);
  const int slot = wv * NSW + sl;
  const int d = a.order[item];
  if (d < 0) return;   // XCD placement gap (GSPlan.xcd_gaps): this document slot only
  const int s0 = a.doc_ptr[d], n = a.doc_ptr[d + 1] - s0;
  const int U = a.gs_updates;
  const int W = n > 0 ? (n + U - 1) / U : 1;
  const int nch = (n + W - 1) / W;           // <= U (host-checked: <= kGsUMax unless GM)
  const int nact = min(NW, (W + NSW - 1) / NSW);   // waves holding words of a chunk
  const bool active = wv < nact;
  const int* __restrict__ wrow = a.word_idx + s0;
  const float* __restrict__ crow = a.counts + s0;
  double(*C)[KS] = sC[ds];
  double(*Et)[KS] = sEt[ds];
  double* E_ = sE[ds];
  double total = 0.0;
  if constexpr (GM) {
    // a thread per chunk: its count sum Cs_j, and C_j = Cs_j / K straight into row j W (any number
    // of chunks); the document total from the per-thread sums (integer counts: exact in any order)
    double part = 0.0;
    for (int j = t; j < nch; j += NTD) {
      const int n0 = j * W, n1 = min(n, n0 + W);
      double cs = 0.0;
      for (int p = n0; p < n1; ++p) cs += (double)crow[p];
      part += cs;
      double* row = a.cphi + (size_t)(s0 + n0) * KS;
      for (int k = 0; k < KS; ++k) row[k] = k < K ? cs / K : 0.0;
    }
    part = group_sum<64>(part);
    if constexpr (NW == 1) {
      total = part;
    } else {
      if (lane == 0) sScal[ds][wv][0] = part;
      __syncthreads();   // also orders the C_j row stores before the topic owners read them
#pragma unroll
      for (int v = 0; v < NW; ++v) total += sScal[ds][v][0];
      __syncthreads();
    }
  } else {
    double* Cs = sCs[ds];
    for (int j = t; j < nch; j += NTD) Cs[j] = 0.0;
    team_sync<NW>();
    // integer counts: the LDS double atomics are exact in any order
    for (int p = t; p < n; p += NTD) atomicAdd(&Cs[p / W], (double)crow[p]);
    team_sync<NW>();
    for (int j = 0; j < nch; ++j) total += Cs[j];
  }
  const double g0 = alpha + total / K;
  const double m = psi_only(g0);
  double gam[TO], psi[TO], lps[TO];
#pragma unroll
  for (int o = 0; o < TO; ++o) {
    const int k = t + NTD * o;
    gam[o] = k < K ? g0 : 0.0;
    psi[o] = m;
    lps[o] = 0.0;
    if (k < KS) {
      E_[k] = k < K ? 1.0 : 0.0;
      if constexpr (!GM) {
        for (int j = 0; j < nch; ++j) C[j][k] = k < K ? sCs[ds][j] / K : 0.0;
      }
    }
  }
  // GM: C of the next chunk, loaded one chunk ahead (NW == 1: this wave wrote it, same-address
  // order; NW > 1: behind the __syncthreads above)
  double Cn[TO];
  if constexpr (GM) {
#pragma unroll
    for (int o = 0; o < TO; ++o) {
      const int k = t + NTD * o;
      Cn[o] = (k < KS && nch > 0) ? a.cphi[(size_t)s0 * KS + k] : 0.0;
    }
  }
  // chunk-ahead prefetch: the beta rows of chunk j + 1 are in flight while chunk j reduces and
  // refreshes (chunks wrap into the next sweep); chunk j + 1's word ids are loaded at the START of
  // chunk j (after its counts left the registers) and land during its word phase.  (Ids loaded two
  // chunks ahead just before the barrier had to be rotated into the loop-carried registers at the
  // loop latch, and that copy made the compiler wait for every outstanding load -- the row prefetch
  // included -- before barrier 1, putting the row latency in front of the refresh.)  Loads are
  // unconditional (clamped indices); a round without a word has count 0 (its row is real but unused).
  int wc[RMAX];
  float cc[RMAX];
  unsigned vc = 0;                            // valid-round mask
  double bc[RMAX][KPL];
  auto load_ids = [&](int j, int (&w)[RMAX], float (&c)[RMAX], unsigned& v) {
    const int n0 = j * W, n1 = min(n, n0 + W);
    v = 0;
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
      const int p = n0 + slot + r * NS;
      v |= (active && p < n1) ? (1u << r) : 0u;
      // rounds past the chunk end re-read the chunk's last word: the same address as a valid
      // lane, so no extra row is gathered (clamping to the document end fetched the next chunk's rows)
      const int pc = min(p, n1 - 1);
      w[r] = wrow[pc];
      c[r] = crow[pc];
    }
  };
  auto load_rows = [&](const int (&w)[RMAX]) {
    if (!active) return;   // wave-uniform: waves without words of a chunk gather no rows
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
      load_row<KS, KPL, TG, PAIR>(a.beta, w[r], q, bc[r]);   // constant offsets (beta's pad row: gs_smallw)
    }
  };
  if (nch > 0) {
    load_ids(0, wc, cc, vc);
    load_rows(wc);
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
#pragma unroll
    for (int o = 0; o < TO; ++o) lps[o] = 0.0;
    for (int j = 0; j < nch; ++j) {
      ph[7] += timer ? 1 : 0;
      if (active) {
        const int n0 = j * W, n1 = min(n, n0 + W);
        // this chunk's counts out of the id registers, then the next chunk's ids into them
        double cr[RMAX];
#pragma unroll
        for (int r = 0; r < RMAX; ++r) cr[r] = ((vc >> r) & 1u) ? (double)cc[r] : 0.0;
        load_ids(j + 1 < nch ? j + 1 : 0, wc, cc, vc);
        double E[KPL], acc[KPL];
#pragma unroll
        for (int i = 0; i < KPL; ++i) {
          E[i] = (tk<TG, PAIR>(q, i) < KS) ? E_[tk<TG, PAIR>(q, i)] : 0.0;
          acc[i] = 0.0;
        }
        // rounds of this chunk (team-uniform): pairs of words in flight per slot
        const int R = (n1 - n0 + NS - 1) / NS;
        if constexpr (RMAX == 1) {
          word_steps<1, KPL, LSW, TAB>(E, bc, cr, acc, lw, sLog);
        } else if (R > 2) {
          word_steps<RMAX, KPL, LSW, TAB>(E, bc, cr, acc, lw, sLog);    // every round in flight at once
        } else {
          word_steps<2, KPL, LSW, TAB>(E, bc, cr, acc, lw, sLog);
        }
        // words beyond the prefetched rounds (documents longer than RMAX * NS * U): streamed in
        // batches of RMAX rows per slot with a batch's loads in flight together (bc is free until
        // the next chunk's prefetch below); one row at a time left the word phase latency-bound
        stream_tail<RMAX, KS, KPL, TG, LSW, PAIR, TAB>(a.beta, wrow, crow, n0 + slot + RMAX * NS, n1, NS, q, E, bc, acc,
                                                        lw, sLog);
        // next chunk's rows (its ids landed during the word phase)
        load_rows(wc);
        tick(0);
        // whole active waves; a one-word chunk (lda-c's per-word schedule: every chunk of a document of
        // <= U words) has its word in slot 0 and exact zeros in the other slots, so the sum is slot 0's
        if (n1 - n0 > 1) {
#pragma unroll
          for (int i = 0; i < KPL; ++i) acc[i] = bits_sum<0, LSW, false>(acc[i]);
        }
        if (sl == 0) {
#pragma unroll
          for (int i = 0; i < KPL; ++i)
            if (tk<TG, PAIR>(q, i) < KS) sRed[ds][wv][tk<TG, PAIR>(q, i)] = acc[i];
        }
        tick(1);
      }
      team_sync<NW>();
      tick(2);
      // gather, then a branch-free refresh (TO > 1: the chains of a thread interleave; a topic-guarded
      // psi_exp is a basic block of its own), then the table stores.  Padding topics: Eo = 0, nw = 0,
      // gamma = 0, psi = m, E = 0.
      double nwv[TO], Eov[TO], Env[TO];
#pragma unroll
      for (int o = 0; o < TO; ++o) {
        const int k = t + NTD * o;
        const int kc = k < KS ? k : KS - 1;
        // all NW loads issued together (a dynamic loop serialises LDS round trips)
        double S = 0.0;
#pragma unroll
        for (int v = 0; v < NW; ++v) S += v < nact ? sRed[ds][v][kc] : 0.0;
        Eov[o] = k < KS ? E_[kc] : 0.0;
        nwv[o] = Eov[o] * S;
        const double Cj = GM ? Cn[o] : C[j][kc];
        const bool real = k < K;
        lps[o] = fma(psi[o], nwv[o], lps[o]);
        gam[o] = real ? gam[o] + (nwv[o] - Cj) : gam[o];
        double pn, en;
        psi_exp<TAB>(real ? gam[o] : 1.0, m, pn, en, sLog);
        psi[o] = real ? pn : psi[o];
        Env[o] = real ? en : 0.0;
      }
#pragma unroll
      for (int o = 0; o < TO; ++o) {
        const int k = t + NTD * o;
        if (k < KS) {
          if constexpr (GM) {
            double* crw = a.cphi + (size_t)(s0 + j * W) * KS;
            crw[k] = nwv[o];
            if (min(n, (j + 1) * W) - j * W >= 2) crw[KS + k] = Eov[o];
            const int j1 = j + 1 < nch ? j + 1 : 0;
            Cn[o] = a.cphi[(size_t)(s0 + j1 * W) * KS + k];
          } else {
            C[j][k] = nwv[o];
            Et[j][k] = Eov[o];
          }
          E_[k] = Env[o];
        }
      }
      tick(3);
      team_sync<NW>();
      tick(4);
    }
    // sweep likelihood: wave partials -> LDS -> every thread sums in wave order
    double gs = 0.0, lg = 0.0, lp = 0.0;
#pragma unroll
    for (int o = 0; o < TO; ++o) {
      if (t + NTD * o < K) {
        gs += gam[o];
        lg += lgamma_pos<TAB>(gam[o], sLog);
        lp += lps[o];
      }
    }
    const double w0 = group_sum<64>(q == 0 ? lw : 0.0);
    const double w1 = group_sum<64>(gs), w2 = group_sum<64>(lg), w3 = group_sum<64>(lp);
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
  // outputs
  double ps = 0.0;
#pragma unroll
  for (int o = 0; o < TO; ++o) {
    const int k = t + NTD * o;
    if (k < K) ps += psi[o];
    if (k < KS) a.gamma[(size_t)d * KS + k] = gam[o];
  }
  ps = group_sum<64>(ps);
  if (lane == 0) sScal[ds][wv][0] = ps;
  team_sync<NW>();
  if (t == 0) {
    double PS = 0.0;
    for (int v = 0; v < NW; ++v) PS += sScal[ds][v][0];
    a.lik[d] = L;
    a.alpha_ss[d] = PS - K * psi_only(GS);
    a.iters[d] = it;
  }
  // final pass: c_n phi_nk = E_jk b_nk r_n with the final sweep's chunk E (same P as the sweep)
  if constexpr (GM && NW > 1) {
    // every wave reads E_j from row n0 + 1 before any wave overwrites the chunk's rows: one
    // workgroup barrier per chunk, so the waves without words stay in the loop
    __syncthreads();   // the last sweep's C_j / E_j row stores (topic owners) before the reads
    for (int j = 0; j < nch; ++j) {
      const int n0 = j * W, n1 = min(n, n0 + W);
      if (n1 - n0 < 2) continue;           // team-uniform: a one-word chunk's row is its c*phi
      const double* er = a.cphi + (size_t)(s0 + n0 + 1) * KS;
      double E[KPL];
#pragma unroll
      for (int i = 0; i < KPL; ++i) E[i] = (tk<TG, PAIR>(q, i) < KS) ? er[tk<TG, PAIR>(q, i)] : 0.0;
      __syncthreads();
      if (active) {
        for (int p = n0 + slot; p < n1; p += NS) {
          const double* brow = a.beta + (size_t)wrow[p] * KS;
          const double c = (double)crow[p];
          double b[KPL];
#pragma unroll
          for (int i = 0; i < KPL; ++i) b[i] = (tk<TG, PAIR>(q, i) < KS) ? brow[tk<TG, PAIR>(q, i)] : 0.0;
          double pp = 0.0;
#pragma unroll
          for (int i = 0; i < KPL; ++i) pp = fma(E[i], b[i], pp);
          const double r = c * drcp(bits_sum<LSW, 6>(pp));
          double* row = a.cphi + (size_t)(s0 + p) * KS;
#pragma unroll
          for (int i = 0; i < KPL; ++i)
            if (tk<TG, PAIR>(q, i) < KS) __builtin_nontemporal_store(E[i] * b[i] * r, &row[tk<TG, PAIR>(q, i)]);
        }
      }
    }
    return;
  }
  if (!active) return;
  for (int j = 0; j < nch; ++j) {
    const int n0 = j * W, n1 = min(n, n0 + W);
    double E[KPL];
    if constexpr (GM) {
      // one-word chunk: its c*phi row already holds C_j; else E_j from row n0 + 1, read by the
      // whole wave before any lane overwrites the chunk's rows (the stores depend on the loads)
      if (n1 - n0 < 2) continue;
      const double* er = a.cphi + (size_t)(s0 + n0 + 1) * KS;
#pragma unroll
      for (int i = 0; i < KPL; ++i) E[i] = (tk<TG, PAIR>(q, i) < KS) ? er[tk<TG, PAIR>(q, i)] : 0.0;
    } else {
#pragma unroll
      for (int i = 0; i < KPL; ++i) E[i] = (tk<TG, PAIR>(q, i) < KS) ? Et[j][tk<TG, PAIR>(q, i)] : 0.0;
    }
    for (int p = n0 + slot; p < n1; p += NS) {
      const double* brow = a.beta + (size_t)wrow[p] * KS;
      const double c = (double)crow[p];
      double b[KPL];
#pragma unroll
      for (int i = 0; i < KPL; ++i) b[i] = (tk<TG, PAIR>(q, i) < KS) ? brow[tk<TG, PAIR>(q, i)] : 0.0;
      double pp = 0.0;
#pragma unroll
      for (int i = 0; i < KPL; ++i) pp = fma(E[i], b[i], pp);
      const double r = c * drcp(bits_sum<LSW, 6>(pp));
      double* row = a.cphi + (size_t)(s0 + p) * KS;
#pragma unroll
      for (int i = 0; i < KPL; ++i)
        if (tk<TG, PAIR>(q, i) < KS) __builtin_nontemporal_store(E[i] * b[i] * r, &row[tk<TG, PAIR>(q, i)]);
    }
  }
}

}  // namespace gs

// ------------------------------------------------------------------ launch ---
template <int KS>
static void gs_team_ks(const GSArgs& a, int NW, hipStream_t s) {
  switch (NW) {
    case 1: {
      if (KS <= 32 && a.gs_updates > kGsUMax)
        throw std::runtime_error("gs_estep: the one-wave team keeps its chunk tables in LDS (U <= 32 at KS <= 32)");
      // one wave per document (<= 256 words, chunks of <= 8 words): the topic-group layout keeps
      // more lanes busy than one word per lane (measured 0.90 vs 1.13 ms on the headline corpus)
      constexpr int dpb = gs::TeamShape<KS, 1>::DPB;
      const dim3 grid((a.n_items + dpb - 1) / dpb), blk(dpb * 64);
      if constexpr (KS > 32) {
        // 3 waves per SIMD (168 VGPRs, 12 B spilled): K = 100 shard team1 13.2 -> 11.7 ms; 4 (128 VGPRs,
        // 100 B spilled) 19.5 ms (profiles/r2_k100_split.md)
        hipLaunchKernelGGL((gs::gs_team<KS, 1, 3>), grid, blk, 0, s, a);
      } else {
        hipLaunchKernelGGL((gs::gs_team<KS, 1>), grid, blk, 0, s, a);
      }
      break;
    }
    case 4:
      if (KS <= 32 && a.gs_updates > kGsUMax) {
        // lda-c's per-word schedule at K <= 32: the topic-group team with its chunk tables in the c*phi rows
        hipLaunchKernelGGL((gs::gs_team<KS, 4, 1, true>), dim3(a.n_items), dim3(256), 0, s, a);
      } else if constexpr (KS <= 32) {
        throw std::runtime_error("gs_team: KS <= 32 at U <= 32 runs one word per lane (launch_gs_wteam)");
      }
      else
        // KS > 32, any U: the chunk tables in the c*phi rows (GM) and 3 waves per SIMD.  The LDS-table form
        // (2 x 32 x KS doubles: 58 KB at K = 100) fits two workgroups per CU; this one (6.7 KB, 166 VGPRs, 12 B
        // spilled) three: team4 bucket 5.88 -> 4.78 ms on the 12.5 M-event shard, 38.1 -> 30.7 ms at 100 M
        // events (E-step graph 170.0 -> 167.1 ms); 4 waves per SIMD spill 160 B and gain less
        // (profiles/r6z_team4_gm.md)
        hipLaunchKernelGGL((gs::gs_team<KS, 4, 3, true>), dim3(a.n_items), dim3(256), 0, s, a);
      break;
    case 8:
      if (KS <= 32 && a.gs_updates > kGsUMax) {
        if (a.stage != nullptr) throw std::runtime_error("gs_estep: no staged rows past U = 32 at KS <= 32");
        hipLaunchKernelGGL((gs::gs_team<KS, 8, 1, true>), dim3(a.n_items), dim3(512), 0, s, a);
      } else if constexpr (KS <= 32) {
        throw std::runtime_error("gs_team: KS <= 32 at U <= 32 runs one word per lane (launch_gs_wsteam)");
      }
      else if (a.gs_updates > kGsUMax)
        hipLaunchKernelGGL((gs::gs_team<KS, 8, 1, true>), dim3(a.n_items), dim3(512), 0, s, a);
      else
        hipLaunchKernelGGL((gs::gs_team<KS, 8>), dim3(a.n_items), dim3(512), 0, s, a);
      break;
    default:
      throw std::runtime_error("gs_team: 1, 4 or 8 waves per document");
  }
}

void launch_gs_team(const GSArgs& a, int KS, int NW, hipStream_t s) {
  switch (KS) {
#define ONI_KS(X)            \
  case X:                    \
    gs_team_ks<X>(a, NW, s); \
    break;
    ONI_FOR_EACH_KS(ONI_KS)
#undef ONI_KS
    default:
      throw std::runtime_error("gs_estep: unsupported KS " + std::to_string(KS));
  }
  ONI_HIP_CHECK(hipGetLastError());
}

}  // namespace oni
