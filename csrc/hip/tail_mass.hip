// --tail: the probability mass a host's model puts at or below an event's word (pipeline/common.py write_tail;
// twin: ops/reference.py tail_mass).
//
// For a side (document d, word w) and every row v of the phi table, p_v is the side's score with row v in place
// of w, evaluated as the scorers evaluate it: per member a rounded product and a rounded sum per topic, in topic
// order from 0.0 (score_dot.h), the members added in order from 0.0 and divided by (double)R
// (score_ensemble.hip).  s = p_w.  The vocabulary is cut into blocks of `block` consecutive rows; within a block,
// from 0.0 in row order, le_b += (p_v <= s ? p_v : 0.0) and tot_b += p_v; rarer_b and ties_b count p_v < s and
// p_v == s; the block values are added from 0.0 in block order.  One set of bits whatever the grid, no atomics.
//
// The arithmetic is fp64 VALU with a separate multiply and add (contraction off).  The bit contract rules out
// FMA -- it rounds once where the definition rounds twice -- and with it MFMA, whose fp64 form is a chain of FMAs
// in an order of its own.  What the kernel saves is phi traffic: a block's rows are staged in LDS once per
// workgroup and every lane reads the same LDS address (a broadcast read), so a row comes from HBM or L2 once per
// tile of sides instead of once per side, and nothing of size sides x V is stored.
//
// Pass 1, item = (tile of sides, vocabulary block), grid-stride; a lane owns one side and walks the block's rows
// in order.  Three forms by row width:
//   registers  the side's theta row in registers, padded to TM members of TK topics; the staged phi rows carry
//              the same padding, 0.0 on both sides.  A padding step adds 0.0 * 0.0 = +0.0 to a sum that started
//              at +0.0 and so is never -0.0: no bit changes, and the inner loops have compile-time bounds and no
//              branch.  TK is the next of {4, 8, 20, 32, 50, 100} >= K; TM is 1 for one model, else 100 / TK
//              members (a row of more members takes the next form).  The bound of 100 doubles is from the
//              compiler's VGPR report: th[100] is 200 VGPRs and the kernel 240, two waves per SIMD; th[104] with
//              two rows in flight came to 263, a wave alone on its SIMD.  One model: 54 VGPRs at TK = 4, 89 at
//              20 (5 waves per SIMD, which is also what 32 KiB of LDS per workgroup allows), 108 at 32, 145 at 50.
//   LDS theta  R K <= 256 that the ladder does not hold: a tile of 64 sides, theta rows in LDS as [j][lane]
//              (conflict-free 8-byte reads, 128 KiB); the workgroup's four waves walk four consecutive blocks
//              over them, phi rows in LDS unpadded, a sub-tile per wave.  One workgroup per CU.
//   direct     anything wider: theta and phi rows from global memory (the phi address is the same in every lane).
// A side's four partials of a block go to scratch[b][side].  Pass 2, one lane per side, folds them in block
// order.  A side with doc < 0 or word < 0 gets NaN, NaN, -1, -1.
#include <stdexcept>
#include <string>

#include "common.h"
#include "kernels.h"
#include "tail_common.h"

namespace oni {

namespace {

using namespace tail;   // Part, take, dot_any, dot_pad, stage_rows, put, reg_topics: shared with tail_docs.hip

constexpr int kPhiLds = 4096;        // doubles of staged phi rows, register form (32 KiB)
constexpr int kGenMax = 256;         // widest row (R K) of the LDS-theta form
constexpr int kGenSides = 64;        // sides of its tile, one per lane of a wave
constexpr int kGenWaves = kThreads / kGenSides;   // vocabulary blocks a workgroup walks at a time
constexpr int kGenTheta = kGenSides * kGenMax;    // doubles of theta rows in LDS (128 KiB)
constexpr int kGenPhi = 512;         // doubles of staged phi rows per wave (4 x 4 KiB)

// registers: theta row padded in registers, phi sub-tiles padded in LDS
template <int TK, int TM>
__global__ __launch_bounds__(kThreads) void tail_blocks_reg_kernel(TailArgs a, int64_t ntiles, int vec) {
  __shared__ double2 ph_l[kPhiLds / 2];
  constexpr int W = TK * TM;   // doubles of a padded row as the lanes walk it
  const int K = a.K, R = a.R, RK = a.R * a.K;
  const int rowl = R * TK;     // doubles of a staged row (members past R are not staged: dot_pad skips them)
  const int sub = kPhiLds / rowl;
  const double rd = (double)R;
  const int64_t items = ntiles * a.nblk;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t b = item / ntiles, i = (item % ntiles) * kThreads + threadIdx.x;
    const int d = i < a.n ? a.doc[i] : -1, w = i < a.n ? a.word[i] : -1;
    const bool ok = d >= 0 && w >= 0;
    double th[W];
#pragma unroll
    for (int m = 0; m < TM; ++m)
#pragma unroll
      for (int k = 0; k < TK; ++k) th[m * TK + k] = ok && m < R && k < K ? a.theta[(size_t)d * RK + m * K + k] : 0.0;
    const double s = ok ? dot_any(a.theta + (size_t)d * RK, 1, a.phi + (size_t)w * RK, R, K, rd) : 0.0;
    Part pt{0.0, 0.0, 0, 0};
    const int64_t v0 = b * a.block, v1 = v0 + a.block < a.V ? v0 + a.block : a.V;
    for (int64_t r0 = v0; r0 < v1; r0 += sub) {
      const int nr = (int)(v1 - r0 < sub ? v1 - r0 : sub);
      __syncthreads();   // the lanes are done with the previous sub-tile
      stage_rows(reinterpret_cast<double*>(ph_l), rowl, a.phi, r0, nr, R, K, TK, vec);
      __syncthreads();
      if (ok) {
        if (W <= 50) {   // two rows in flight where the registers allow it
#pragma unroll 2
          for (int row = 0; row < nr; ++row) take(pt, dot_pad<TK, TM>(th, ph_l + row * (rowl / 2), R, rd), s);
        } else {
#pragma unroll 1
          for (int row = 0; row < nr; ++row) take(pt, dot_pad<TK, TM>(th, ph_l + row * (rowl / 2), R, rd), s);
        }
      }
    }
    if (ok) put(a, b, i, pt);
  }
}

// LDS theta: a tile of 64 sides, their theta rows in LDS [j][lane]; the workgroup's four waves walk four
// consecutive vocabulary blocks, one each, over the same theta rows, each wave staging its own phi sub-tiles
__global__ __launch_bounds__(kThreads) void tail_blocks_lds_kernel(TailArgs a, int64_t ntiles, int vec) {
  __shared__ double th_l[kGenTheta];
  __shared__ double2 ph_l[kGenWaves][kGenPhi / 2];
  const int lane = threadIdx.x % kGenSides, wv = threadIdx.x / kGenSides;
  const int K = a.K, R = a.R, RK = a.R * a.K;
  const int sub = kGenPhi / RK;   // >= 2 rows
  const double rd = (double)R;
  const int64_t span = a.block < a.V ? a.block : a.V;   // rows of the longest block
  const int64_t items = ntiles * ((a.nblk + kGenWaves - 1) / kGenWaves);
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t b = (item / ntiles) * kGenWaves + wv, i = (item % ntiles) * kGenSides + lane;
    const int d = i < a.n ? a.doc[i] : -1, w = i < a.n ? a.word[i] : -1;
    const bool ok = d >= 0 && w >= 0, live = ok && b < a.nblk;
    __syncthreads();   // every wave is done with the previous item's theta rows
    if (ok)   // the side's four lanes, one per wave, share the copy
      for (int j = wv; j < RK; j += kGenWaves) th_l[j * kGenSides + lane] = a.theta[(size_t)d * RK + j];
    const double s = ok ? dot_any(a.theta + (size_t)d * RK, 1, a.phi + (size_t)w * RK, R, K, rd) : 0.0;
    Part pt{0.0, 0.0, 0, 0};
    const int64_t v0 = b * a.block, v1 = b >= a.nblk ? v0 : (v0 + a.block < a.V ? v0 + a.block : a.V);
    for (int64_t off = 0; off < span; off += sub) {   // the same trips in every wave: the barriers are the workgroup's
      const int64_t r0 = v0 + off;
      const int nr = r0 < v1 ? (int)(v1 - r0 < sub ? v1 - r0 : sub) : 0;
      __syncthreads();   // the lanes are done with the previous sub-tile
      const double* src = a.phi + (size_t)r0 * RK;   // nr whole rows, contiguous
      if (vec) {   // R K even, phi 16-byte aligned
        for (int t = lane; t < nr * RK / 2; t += kGenSides) ph_l[wv][t] = reinterpret_cast<const double2*>(src)[t];
      } else {
        double* dst = reinterpret_cast<double*>(ph_l[wv]);
        for (int t = lane; t < nr * RK; t += kGenSides) dst[t] = src[t];
      }
      __syncthreads();   // the sub-tile, and at the first trip the theta rows, are complete
      if (live) {
        const double* rows = reinterpret_cast<const double*>(ph_l[wv]);
        for (int row = 0; row < nr; ++row) take(pt, dot_any(th_l + lane, kGenSides, rows + row * RK, R, K, rd), s);
      }
    }
    if (live) put(a, b, i, pt);
  }
}

// direct: any row width, both rows from global memory
__global__ __launch_bounds__(kThreads) void tail_blocks_direct_kernel(TailArgs a, int64_t ntiles) {
  const int K = a.K, R = a.R;
  const size_t RK = (size_t)a.R * a.K;
  const double rd = (double)R;
  const int64_t items = ntiles * a.nblk;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t b = item / ntiles, i = (item % ntiles) * kThreads + threadIdx.x;
    const int d = i < a.n ? a.doc[i] : -1, w = i < a.n ? a.word[i] : -1;
    if (d < 0 || w < 0) continue;
    const double* tr = a.theta + (size_t)d * RK;
    const double s = dot_any(tr, 1, a.phi + (size_t)w * RK, R, K, rd);
    Part pt{0.0, 0.0, 0, 0};
    const int64_t v0 = b * a.block, v1 = v0 + a.block < a.V ? v0 + a.block : a.V;
    for (int64_t v = v0; v < v1; ++v) take(pt, dot_any(tr, 1, a.phi + (size_t)v * RK, R, K, rd), s);
    put(a, b, i, pt);
  }
}

// pass 2: one lane per side adds its blocks' partials from 0.0 in block order
__global__ __launch_bounds__(kThreads) void tail_fold_kernel(TailArgs a) {
  const size_t cells = (size_t)a.nblk * (size_t)a.n;
  const double* sd = a.scratch;
  const int* si = reinterpret_cast<const int*>(sd + 2 * cells);
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kThreads) {
    if (a.doc[i] < 0 || a.word[i] < 0) {   // no host model or no word to place
      a.le[i] = nan;
      a.tot[i] = nan;
      a.rarer[i] = -1;
      a.ties[i] = -1;
      continue;
    }
    double le = 0.0, tot = 0.0;
    int rarer = 0, ties = 0;
    for (int64_t b = 0; b < a.nblk; ++b) {
      const size_t at = (size_t)b * (size_t)a.n + (size_t)i;
      le = le + sd[at];
      tot = tot + sd[cells + at];
      rarer += si[at];
      ties += si[cells + at];
    }
    a.le[i] = le;
    a.tot[i] = tot;
    a.rarer[i] = rarer;
    a.ties[i] = ties;
  }
}

template <int TK>
void launch_reg(const TailArgs& a, int64_t ntiles, int vec, unsigned blocks, hipStream_t s) {
  constexpr int TM = kRegMax / TK;
  if (a.R == 1)
    hipLaunchKernelGGL((tail_blocks_reg_kernel<TK, 1>), dim3(blocks), dim3(kThreads), 0, s, a, ntiles, vec);
  else
    hipLaunchKernelGGL((tail_blocks_reg_kernel<TK, TM>), dim3(blocks), dim3(kThreads), 0, s, a, ntiles, vec);
}

}  // namespace

int tail_theta_path(int R, int K) {
  if (R < 1 || K < 1 || R > kEnsembleMax) throw std::runtime_error("tail_theta_path: R or K out of range");
  if (reg_topics(R, K)) return kTailRegisters;
  return (int64_t)R * K <= kGenMax ? kTailLdsTheta : kTailDirect;
}

bool tail_args_check(const TailArgs& a, int max_blocks, const char* who) {
  const std::string w(who);
  if (a.n < 0 || a.n >= ((int64_t)1 << 31) || a.V < 0 || a.V >= ((int64_t)1 << 31))
    throw std::runtime_error(w + ": n or V outside 0 .. 2^31 - 1");
  if (a.R < 1 || a.R > kEnsembleMax) throw std::runtime_error(w + ": R outside 1 .. " + std::to_string(kEnsembleMax));
  if (a.K < 1 || (int64_t)a.R * a.K >= ((int64_t)1 << 31)) throw std::runtime_error(w + ": K < 1 or R K >= 2^31");
  if (a.block < 1 || a.block >= ((int64_t)1 << 31)) throw std::runtime_error(w + ": block outside 1 .. 2^31 - 1");
  if (a.nblk != (a.V + a.block - 1) / a.block) throw std::runtime_error(w + ": nblk is not ceil(V / block)");
  if (max_blocks < 0) throw std::runtime_error(w + ": max_blocks < 0");
  if (a.n == 0) return false;
  if (!a.theta || !a.doc || !a.word || !a.le || !a.tot || !a.rarer || !a.ties)
    throw std::runtime_error(w + ": null buffer");
  if (a.V > 0 && (!a.phi || !a.scratch)) throw std::runtime_error(w + ": null buffer");
  if ((uintptr_t)a.scratch % 8 != 0) throw std::runtime_error(w + ": scratch is not 8-byte aligned");
  return true;
}

void launch_tail_fold(const TailArgs& a, int64_t cap, hipStream_t s) {
  int64_t blocks = (a.n + kThreads - 1) / kThreads;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(tail_fold_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, a);
  ONI_HIP_CHECK(hipGetLastError());
}

void launch_tail_mass(const TailArgs& a, int max_blocks, hipStream_t s) {
  if (!tail_args_check(a, max_blocks, "tail_mass")) return;
  const int64_t cap = max_blocks > 0 ? max_blocks : 65536;
  if (a.nblk > 0) {
    const int path = tail_theta_path(a.R, a.K);
    const int RK = a.R * a.K;
    const int tile = path == kTailLdsTheta ? kGenSides : kThreads;
    const int64_t ntiles = (a.n + tile - 1) / tile;
    int64_t blocks = ntiles * (path == kTailLdsTheta ? (a.nblk + kGenWaves - 1) / kGenWaves : a.nblk);
    if (blocks > cap) blocks = cap;
    const bool al = (uintptr_t)a.phi % 16 == 0;
    if (path == kTailRegisters) {
      const int vec = a.K % 2 == 0 && al;
      switch (reg_topics(a.R, a.K)) {
        case 4: launch_reg<4>(a, ntiles, vec, (unsigned)blocks, s); break;
        case 8: launch_reg<8>(a, ntiles, vec, (unsigned)blocks, s); break;
        case 20: launch_reg<20>(a, ntiles, vec, (unsigned)blocks, s); break;
        case 32: launch_reg<32>(a, ntiles, vec, (unsigned)blocks, s); break;
        case 50: launch_reg<50>(a, ntiles, vec, (unsigned)blocks, s); break;
        default: launch_reg<100>(a, ntiles, vec, (unsigned)blocks, s); break;
      }
    } else if (path == kTailLdsTheta) {
      const int vec = RK % 2 == 0 && al;
      hipLaunchKernelGGL(tail_blocks_lds_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, a, ntiles, vec);
    } else {
      hipLaunchKernelGGL(tail_blocks_direct_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, a, ntiles);
    }
    ONI_HIP_CHECK(hipGetLastError());
  }
  launch_tail_fold(a, cap, s);
}

}  // namespace oni
