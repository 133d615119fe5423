// fp64 block Gauss-Seidel E-step, sufficient statistics and M-step (gfx950).
//
// Reference: oni-lda-c's lda_inference (call site /root/reference/ml_ops.sh:80;
// SURVEY.md C9c-C9h) computes in double and refreshes gamma and digamma(gamma)
// after EVERY word.  This engine keeps lda-c's arithmetic (double, lda-c's series
// digamma, lgamma, the -100 floor) and its schedule up to the block size: a
// document of n words is walked in chunks of W = ceil(n / U) words (U = gs_updates
// refreshes per sweep); a chunk's words take phi from one digamma vector, then
// gamma and digamma are refreshed.  n <= U is exactly lda-c's per-word schedule.
// The CPU oracle is csrc/native/lda_ref.cpp lda_inference(..., gs_updates).
//
// Chunk algebra (why no per-word phi state is needed): with E_k = exp(psi_k - m)
// (m = psi of the initial gamma, a per-document constant), P_n = sum_k E_k b_nk,
// r_n = c_n / P_n, the chunk's contribution to gamma is
//     new_jk = sum_{n in j} c_n phi_nk = E_k * S_k,   S_k = sum_{n in j} r_n b_nk,
// so a chunk update is gamma_k += new_jk - C_jk; C_jk = new_jk (C = the chunk's
// previous contribution, c_total/K before the first sweep), one table of U x KS
// doubles per document in LDS.  The per-sweep likelihood (lda-c compute_likelihood)
// collapses to
//     L = lgG(K a) - K lgG(a) - lgG(sum g) + sum_k lgG(g_k)
//         + sum_n c_n (m + log P_n) - sum_j sum_k psi_jk new_jk
// (the (a - 1), (g - 1) and (g - a) psi terms cancel exactly; psi_jk is the digamma
// the chunk's words saw).  The final sweep's c_n phi_nk = E_jk b_nk r_n rows are
// written per corpus entry; the suff-stats kernel gathers them in CSC order.
//
// The E-step kernels, one translation unit per family (launchers: gs_families.h; shared lane layouts: gs_layout.h):
//   gs_short.hip   gs_tiny, gs_small, gs_chain, gs_smallw: a few lanes or one wave per document
//   gs_team.hip    gs_team: one wave / 4-wave / 8-wave workgroup per document
//   gs_wteam.hip   gs_wteam, gs_wsteam: one word per lane (KS <= 32)
//   gs_split.hip   gs_splitw: one long document over several workgroups
// This file: the E-step dispatch by bucket variant, the sufficient statistics, the M-step with the alpha
// Newton and the EM control step, the staged rows and the random start.
#include <algorithm>
#include <cstdlib>
#include <stdexcept>
#include <string>

#include "../common/splitmix64.h"
#include "alpha_newton.h"
#include "common.h"
#include "em_control.h"
#include "gs_families.h"
#include "gs_layout.h"
#include "gs_math.h"
#include "kernels.h"

namespace oni {
namespace gs {

constexpr double kExpM100 = 3.720075976020836e-44;   // exp(-100), lda-c's log-probability floor

// ------------------------------------------------------------ suff stats ----
// One word per workgroup (heavy) / wave (medium) / 16 lanes (light); a CSC entry's
// row is read by TG lanes (KPL topics each), S = G / TG entries in flight per group.
// RECOMP (KS <= 32, the late pass of a deferred longest-document bucket, em.py): slot s's row is not loaded from
// cphi but computed -- the word's beta row (once per word: all of its entries share it), the chunk's final-sweep
// E at rc.et[rc.et_row[s]] (left by gs_wsteam, L2-resident: U x KS doubles per document) and the entry's
// count, through the final pass's own cphi_row: the TG = 4 lanes of an entry hold topics q + 4 i, lane q the
// chain p_q.  The rows, their order of summation and hence class_word are bitwise the materialised path's.
template <int KS, bool RECOMP = false>
__global__ __launch_bounds__(256) void gs_suff64(const int* __restrict__ word_ptr, const int* __restrict__ csc_ent,
                                                 const int* __restrict__ order, int n_heavy, int n_medium,
                                                 int n_light, const double* __restrict__ cphi,
                                                 double* cw, double* __restrict__ part,
                                                 const double* __restrict__ lik, const double* __restrict__ ass,
                                                 int lo, int hi, const double* gate,
                                                 const double* cw_base, SuffRecompArgs rc) {
  // one topic per lane: the paired 16-byte loads of the team kernels measured slower here (K = 100 early
  // pass 2.06 -> 2.62 ms, r5v); the c.phi pad row (em.py) is kept so PAIR stays a one-line switch
  constexpr int TG = tg_of(KS), NSLOT = 256 / TG;
  constexpr bool PAIR = false;
  constexpr int KPL = PAIR ? 2 * ((KS + 2 * TG - 1) / (2 * TG)) : kpl_of(KS);
  __shared__ double sAcc[NSLOT][KS];
  __shared__ double sRow[16][KS];
  if (gated(gate)) return;
  const int t = threadIdx.x, b = blockIdx.x;
  double* prow = part + (size_t)b * (KS + 2);
  // likelihood / alpha_ss slice of this workgroup (wave 0, fixed order)
  if (t < 64) {
    const int nd = hi - lo, nb = (int)gridDim.x;
    const int per = (nd + nb - 1) / nb;
    const int i0 = lo + b * per, i1 = min(hi, i0 + per);
    double x = 0.0, y = 0.0;
    if (lik)
      for (int i = i0 + t; i < i1; i += 64) {
        x += lik[i];
        y += ass[i];
      }
    x = group_sum<64>(x);
    y = group_sum<64>(y);
    if (t == 0) {
      prow[0] = x;
      prow[1] = y;
    }
  }
  const int nbM = (n_medium + 3) / 4;
  int G, item, nitems, base;
  if (b < n_heavy) {
    G = 256, item = b, nitems = n_heavy, base = 0;
  } else if (b < n_heavy + nbM) {
    G = 64, item = (b - n_heavy) * 4 + t / 64, nitems = n_medium, base = n_heavy;
  } else {
    G = 16, item = (b - n_heavy - nbM) * 16 + t / 16, nitems = n_light, base = n_heavy + n_medium;
  }
  const int S = G / TG, gi = t / G;
  const int sidx = (t % G) / TG, q = t % TG;
  const bool valid = item < nitems;
  double acc[KPL];
#pragma unroll
  for (int i = 0; i < KPL; ++i) acc[i] = 0.0;
  if (valid) {
    const int w = order[base + item];
    int e = word_ptr[w] + sidx;
    const int end = word_ptr[w + 1];
    double bw[KPL];
    if constexpr (RECOMP) {
      static_assert(!RECOMP || (TG == 4 && !PAIR && KS % 4 == 0), "recomputed rows: a quad of lanes per entry");
      load_row<KS, KPL, TG, PAIR>(rc.beta, w, q, bw);
    }
    // the row of CSC slot x (the 4 lanes of an entry share x, so the quad is active as a whole)
    auto entry = [&](int x, double (&v)[KPL]) {
      if constexpr (RECOMP) {
        double Ev[KPL];
        load_row<KS, KPL, TG, PAIR>(rc.et, rc.et_row[x], q, Ev);
        cphi_row<KPL, 4>(Ev, bw, (double)rc.counts[csc_ent[x]], v);
      } else {
        load_row<KS, KPL, TG, PAIR>(cphi, csc_ent[x], q, v);
      }
    };
    for (; e + 3 * S < end; e += 4 * S) {
      double v[4][KPL];
#pragma unroll
      for (int u = 0; u < 4; ++u) entry(e + u * S, v[u]);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int i = 0; i < KPL; ++i) acc[i] += v[u][i];
    }
    for (; e < end; e += S) {
      double v[KPL];
      entry(e, v);
#pragma unroll
      for (int i = 0; i < KPL; ++i) acc[i] += v[i];
    }
  }
#pragma unroll
  for (int i = 0; i < KPL; ++i)
    if (tk<TG, PAIR>(q, i) < KS) sAcc[t / TG][tk<TG, PAIR>(q, i)] = acc[i];
  __syncthreads();
  const int ngroups = 256 / G;
  for (int idx = t; idx < ngroups * KS; idx += 256) {
    const int g = idx / KS, k = idx % KS;
    const int it = (G == 256 ? item : item - gi + g);
    // cw_base (nullable): rows summed earlier from the other entries of each word (the early /
    // late split of the suff-stats and the c.phi windows, em.py), added first so the order is
    // fixed; cw_base == cw (in place) is allowed: each element is read, then written, by one thread
    const size_t row = it < nitems ? (size_t)order[base + it] * KS : 0;
    double v = (cw_base != nullptr && it < nitems) ? cw_base[row + k] : 0.0;
    for (int u = 0; u < S; ++u) v += sAcc[g * S + u][k];
    if (it < nitems) cw[row + k] = v;
    else v = 0.0;
    sRow[g][k] = v;
  }
  __syncthreads();
  if (t < KS) {
    double s = 0.0;
    for (int g = 0; g < ngroups; ++g) s += sRow[g][t];
    prow[2 + t] = s;
  }
}

// ------------------------------------------------------------ random init ---
// lda-c "random" start (random_initialize_ss): class_word[k][w] = 1/V + u, u ~ U[0, 1) from a
// counter-based generator, so the host (csrc/native, CPU backends) and the device produce the same
// bits without a host-side stream: u = splitmix64(splitmix64(seed) ^ (k V + w)) >> 11, x 2^-53.
// (splitmix64: csrc/common/splitmix64.h, shared with the host twin and the holdout draw)
__global__ __launch_bounds__(256) void init_random_ss_kernel(double* __restrict__ cw, int V, int K, int KS,
                                                             unsigned long long seed) {
  const unsigned long long s = splitmix64(seed);
  const double inv = 1.0 / (double)V;
  const long long total = (long long)V * KS;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int w = (int)(i / KS), k = (int)(i % KS);
    double v = 0.0;
    if (k < K) {
      const unsigned long long h = splitmix64(s ^ ((unsigned long long)k * (unsigned long long)V + (unsigned long long)w));
      v = inv + (double)(h >> 11) * 0x1.0p-53;
    }
    cw[i] = v;
  }
}

// ----------------------------------------------------------------- M-step ---
__device__ __forceinline__ double mle(double c, double ct) { return c > 0.0 ? c / ct : kExpM100; }

// SKS > 0: the trailing sf.blocks workgroups refill staged rows at KS = SKS (one thread per staged
// position: its word's row in SKS / 2 independent 16-byte loads, as gs_stage_kernel)
template <int SKS>
__global__ __launch_bounds__(256) void gs_mstep_control_kernel(const double* __restrict__ cw,
                                                               const double* __restrict__ ct,
                                                               double* __restrict__ beta, int V, int K, int KS,
                                                               const int* __restrict__ rows, int n_rows,
                                                               EMControlArgs c, NewtonArgs nw, StageFuseArgs sf) {
  if (c.params[kParamDone] != 0.0) return;
  // with the alpha Newton (a serial chain of ~10-20 digamma / trigamma / exp / log steps on two lanes),
  // block 0 runs only the Newton and the other blocks compute beta beside it
  const bool newton = nw.enabled && gridDim.x > 1;
  if (nw.enabled && blockIdx.x == 0 && threadIdx.x < 64) {
    if (threadIdx.x < 2)
      alpha_newton_lanes(c.scalars, nw.num_docs, K, nw.estimate, c.params, nw.alpha_out, threadIdx.x);
    __builtin_amdgcn_s_waitcnt(0);
  }
  const int hq = KS / 2;
  const int total2 = (rows ? n_rows : V) * hq;
  const double2* cw2 = reinterpret_cast<const double2*>(cw);
  double2* beta2 = reinterpret_cast<double2*>(beta);
  const int sb0 = (int)gridDim.x - sf.blocks;   // the trailing sf.blocks workgroups refill staged rows
  if constexpr (SKS > 0) {
    if ((int)blockIdx.x >= sb0) {
      // one thread per (tile, lane): the row's SKS / 2 pairs loaded together, mle(cw, ct) -- bit for bit
      // the beta entries -- stored one 16-byte element per pair in [tile][pair][64 lanes]
      constexpr int HQ = SKS / 2;
      const int n0 = sf.n_tiles[0] * 64, n1 = sf.n_sets > 1 ? sf.n_tiles[1] * 64 : 0;
      for (int e = ((int)blockIdx.x - sb0) * (int)blockDim.x + (int)threadIdx.x; e < n0 + n1;
           e += sf.blocks * (int)blockDim.x) {
        const int set = e < n0 ? 0 : 1;
        const int el = set ? e - n0 : e;
        const int t = el >> 6, l = el & 63;
        double2 v[HQ];
        if (l < sf.tile_cnt[set][t]) {
          const double2* row = cw2 + (size_t)sf.word_idx[sf.tile_ent[set][t] + l] * HQ;
#pragma unroll
          for (int k = 0; k < HQ; ++k) v[k] = row[k];
#pragma unroll
          for (int k = 0; k < HQ; ++k) {
            v[k].x = 2 * k < K ? mle(v[k].x, ct[2 * k]) : 0.0;
            v[k].y = 2 * k + 1 < K ? mle(v[k].y, ct[2 * k + 1]) : 0.0;
          }
        } else {
#pragma unroll
          for (int k = 0; k < HQ; ++k) v[k] = double2{0.0, 0.0};
        }
        double2* o = reinterpret_cast<double2*>(sf.out[set]) + (size_t)t * HQ * 64 + l;
#pragma unroll
        for (int k = 0; k < HQ; ++k) o[k * 64] = v[k];
      }
    }
  }
  if ((int)blockIdx.x < sb0) {
    const int bx = newton ? (int)blockIdx.x - 1 : (int)blockIdx.x, nbx = newton ? sb0 - 1 : sb0;
    for (int g = bx * blockDim.x + threadIdx.x; bx >= 0 && g < total2; g += nbx * blockDim.x) {
      const int k0 = (g % hq) * 2;
      const int i = rows ? rows[g / hq] * hq + g % hq : g;
      const double2 v = cw2[i];
      double2 o;
      o.x = k0 < K ? mle(v.x, ct[k0]) : 0.0;
      o.y = k0 + 1 < K ? mle(v.y, ct[k0 + 1]) : 0.0;
      beta2[i] = o;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (__hip_atomic_fetch_add(c.done_count, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1) {
      __hip_atomic_store(c.done_count, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const double alpha_now = __hip_atomic_load(c.params, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      em_control_step(c.scalars, c.params, c.ctl, c.hist, c.hist_slots, alpha_now);
    }
  }
}

__global__ __launch_bounds__(256) void gs_mstep_kernel(const double* __restrict__ cw, const double* __restrict__ ct,
                                                       double* __restrict__ beta, int V, int K, int KS,
                                                       const double* gate) {
  if (gated(gate)) return;
  const int64_t total = (int64_t)V * KS;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int k = (int)(i % KS);
    beta[i] = k < K ? mle(cw[i], ct[k]) : 0.0;
  }
}

// Staged rows of the longest documents (GSArgs::stage): one thread per double2 of the tiled copy,
// coalesced stores and 16-byte gathers from beta (the gathers are spread over the whole GPU here,
// instead of through the one CU that walks the document 20 times per E-step)
template <int KS>
__global__ __launch_bounds__(256) void gs_stage_kernel(const double* __restrict__ beta,
                                                       const int* __restrict__ word_idx,
                                                       const int* __restrict__ tile_ent,
                                                       const int* __restrict__ tile_cnt, int n_tiles,
                                                       dvec2* __restrict__ out, const double* gate) {
  if (gate != nullptr && *gate != 0.0) return;   // converged EM loop: the queued iterations are no-ops
  // one thread per (tile, lane): its word's whole row in KS / 2 independent 16-byte loads, stored
  // as one 16-byte element per topic pair (a wave's stores are 1 KB-contiguous per pair)
  const long long total = (long long)n_tiles * 64;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int t = (int)(i >> 6), l = (int)(i & 63);
    dvec2 v[KS / 2];
    if (l < tile_cnt[t]) {
      const dvec2* row = reinterpret_cast<const dvec2*>(beta + (size_t)word_idx[tile_ent[t] + l] * KS);
#pragma unroll
      for (int k = 0; k < KS / 2; ++k) v[k] = row[k];
    } else {
#pragma unroll
      for (int k = 0; k < KS / 2; ++k) v[k] = dvec2{0.0, 0.0};
    }
    dvec2* o = out + (size_t)t * (KS / 2) * 64 + l;
#pragma unroll
    for (int k = 0; k < KS / 2; ++k) o[k * 64] = v[k];
  }
}

}  // namespace gs

// every KS: U > kGsUMax keeps the chunk tables in the c*phi rows (gs_team GMT, gs_chain, gs_smallw at KS > 32)
int gs_umax(int KS) { (void)KS; return kGsUMaxWide; }

void launch_gs_stage(const double* beta, const int* word_idx, const int* tile_ent, const int* tile_cnt, int n_tiles,
                     double* stage, int KS, const double* gate, hipStream_t s) {
  if (n_tiles <= 0) return;
  if (KS > 32 || KS % 2) throw std::runtime_error("gs_stage: staged rows need an even KS <= 32");
  const long long total = (long long)n_tiles * 64;
  const unsigned blocks = (unsigned)std::min<long long>((total + 255) / 256, 16384);
  switch (KS) {
#define ONI_KS(X)                                                                                           \
  case X:                                                                                                   \
    if constexpr (X <= 32 && X % 2 == 0)                                                                    \
      hipLaunchKernelGGL((gs::gs_stage_kernel<X>), dim3(blocks), dim3(256), 0, s, beta, word_idx, tile_ent, \
                         tile_cnt, n_tiles, reinterpret_cast<gs::dvec2*>(stage), gate);                     \
    break;
    ONI_FOR_EACH_KS(ONI_KS)
#undef ONI_KS
    default:
      throw std::runtime_error("gs_stage: unsupported KS " + std::to_string(KS));
  }
  ONI_HIP_CHECK(hipGetLastError());
}

static bool gs_ks_compiled(int KS) {
  switch (KS) {
#define ONI_KS(X) \
  case X:         \
    return true;
    ONI_FOR_EACH_KS(ONI_KS)
#undef ONI_KS
    default:
      return false;
  }
}

// the family of a bucket variant (gs_families.h); each family launcher picks its instantiation
void launch_gs_estep(const GSArgs& a, int variant, int KS, hipStream_t s) {
  if (a.gs_updates < 1 || a.gs_updates > gs_umax(KS))
    throw std::runtime_error("gs_estep: gs_updates must be in [1, " + std::to_string(gs_umax(KS)) + "] at KS " +
                             std::to_string(KS));
  if (!a.params) throw std::runtime_error("gs_estep: params block required");
  if (!gs_ks_compiled(KS)) throw std::runtime_error("gs_estep: unsupported KS " + std::to_string(KS));
  if (a.n_items <= 0) return;
  // KS <= 32 at U <= kGsUMax: the 4- and 8-wave buckets run one word per lane (gs_wteam.hip)
  const bool wordlane = KS <= 32 && a.gs_updates <= kGsUMax;
  switch (variant) {
    case kGsTiny:
      launch_gs_tiny(a, KS, s);
      break;
    case kGsSmall:
      launch_gs_small(a, KS, s);
      break;
    case kGsChain:
      launch_gs_chain(a, KS, s);
      break;
    case kGsTeam1:
      launch_gs_team(a, KS, 1, s);
      break;
    case kGsTeam4:
      if (wordlane)
        launch_gs_wteam(a, KS, s);
      else
        launch_gs_team(a, KS, 4, s);
      break;
    case kGsTeam8:
      if (wordlane)
        launch_gs_wsteam(a, KS, s);
      else
        launch_gs_team(a, KS, 8, s);
      break;
    default:
      throw std::runtime_error("gs_estep: unknown variant");
  }
}

int suff_fused_blocks(int n_heavy, int n_medium, int n_light) {
  return n_heavy + (n_medium + 3) / 4 + (n_light + 15) / 16;
}

void launch_gs_suff64(const int* word_ptr, const int* csc_ent, const int* order, int n_heavy, int n_medium,
                      int n_light, const double* cphi, double* cw, double* part, const double* lik,
                      const double* ass, int lo, int hi, int KS, const double* gate, hipStream_t s,
                      const double* cw_base, const SuffRecompArgs& rc) {
  const int nb = suff_fused_blocks(n_heavy, n_medium, n_light);
  if (nb <= 0) return;
  const bool recomp = rc.et != nullptr;
  if (recomp && (KS > 32 || !rc.beta || !rc.et_row || !rc.counts))
    throw std::runtime_error("gs_suff64: recomputed rows need KS <= 32 and beta, et, et_row, counts");
  switch (KS) {
#define ONI_KS(X)                                                                                             \
  case X:                                                                                                     \
    if constexpr (X <= 32) {                                                                                  \
      if (recomp) {                                                                                           \
        hipLaunchKernelGGL((gs::gs_suff64<X, true>), dim3(nb), dim3(256), 0, s, word_ptr, csc_ent, order,     \
                           n_heavy, n_medium, n_light, cphi, cw, part, lik, ass, lo, hi, gate, cw_base, rc);  \
        break;                                                                                                \
      }                                                                                                       \
    }                                                                                                         \
    hipLaunchKernelGGL((gs::gs_suff64<X>), dim3(nb), dim3(256), 0, s, word_ptr, csc_ent, order, n_heavy,      \
                       n_medium, n_light, cphi, cw, part, lik, ass, lo, hi, gate, cw_base, rc);               \
    break;
    ONI_FOR_EACH_KS(ONI_KS)
#undef ONI_KS
    default:
      throw std::runtime_error("gs_suff64: unsupported KS " + std::to_string(KS));
  }
  ONI_HIP_CHECK(hipGetLastError());
}

void launch_gs_mstep_control(const double* cw, const double* class_total, double* beta, int V, int K, int KS,
                             const int* rows, int n_rows, const EMControlArgs& c, const NewtonArgs& nw,
                             hipStream_t s, StageFuseArgs sf) {
  const int64_t total = (int64_t)(rows ? n_rows : V) * KS;
  int64_t blocks = (total / 2 + 255) / 256;
  if (blocks > 512) blocks = 512;
  if (blocks < 1) blocks = 1;
  if (nw.enabled) blocks += 1;   // block 0: the alpha Newton alone
  sf.blocks = 0;
  if (sf.n_sets > 0) {
    if (sf.n_sets > 2 || KS > 32 || KS % 2 || !sf.word_idx)
      throw std::runtime_error("gs_mstep_control: staged rows need 1-2 sets, an even KS <= 32 and word_idx");
    long long pos = 0;
    for (int i = 0; i < sf.n_sets; ++i) {
      if (sf.n_tiles[i] > 0 && (!sf.tile_ent[i] || !sf.tile_cnt[i] || !sf.out[i]))
        throw std::runtime_error("gs_mstep_control: staged set without its tables");
      pos += (long long)std::max(sf.n_tiles[i], 0) * 64;
    }
    if (pos > INT32_MAX) throw std::runtime_error("gs_mstep_control: too many staged positions");
    sf.blocks = (int)std::min<long long>((pos + 255) / 256, 1024);   // one thread per staged position
    blocks += sf.blocks;
  }
  if (sf.blocks == 0) {
    hipLaunchKernelGGL(gs::gs_mstep_control_kernel<0>, dim3((unsigned)blocks), dim3(256), 0, s, cw, class_total,
                       beta, V, K, KS, rows, n_rows, c, nw, sf);
  } else {
    switch (KS) {
#define ONI_KS(X)                                                                                          \
  case X:                                                                                                  \
    if constexpr (X <= 32 && X % 2 == 0)                                                                   \
      hipLaunchKernelGGL((gs::gs_mstep_control_kernel<X>), dim3((unsigned)blocks), dim3(256), 0, s, cw,    \
                         class_total, beta, V, K, KS, rows, n_rows, c, nw, sf);                            \
    break;
      ONI_FOR_EACH_KS(ONI_KS)
#undef ONI_KS
      default:
        throw std::runtime_error("gs_mstep_control: staged rows at unsupported KS " + std::to_string(KS));
    }
  }
  ONI_HIP_CHECK(hipGetLastError());
}

void launch_init_random_ss(double* cw, int V, int K, int KS, unsigned long long seed, hipStream_t s) {
  const long long total = (long long)V * KS;
  if (total <= 0) return;
  long long blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(gs::init_random_ss_kernel, dim3((unsigned)blocks), dim3(256), 0, s, cw, V, K, KS, seed);
  ONI_HIP_CHECK(hipGetLastError());
}

void launch_gs_mstep(const double* cw, const double* class_total, double* beta, int V, int K, int KS,
                     const double* gate, hipStream_t s) {
  const int64_t total = (int64_t)V * KS;
  if (total == 0) return;
  int64_t blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(gs::gs_mstep_kernel, dim3((unsigned)blocks), dim3(256), 0, s, cw, class_total, beta, V, K, KS,
                     gate);
  ONI_HIP_CHECK(hipGetLastError());
}

}  // namespace oni
