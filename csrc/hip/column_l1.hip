// --topic-match: the L1 distances between the columns of two tables (pipeline/common.py write_topic_match; twin:
// ops/reference.py column_l1).
//
// A is [Va][Wa], B is [Vb][Wb], row-major fp64; ia / ib are M row indices each (both null: the identity, row m of
// both).  C[a][b] = sum over the M pairs of |A[ia[m]][a] - B[ib[m]][b]|, and this fixes the bits: the pairs are cut
// into blocks of `block` consecutive pairs; within a block, from 0.0 in pair order, t = x - y (one rounded
// subtraction) and acc = acc + |t| (one rounded add); the block sums are added from 0.0 in block order (the scheme
// of group_rows_sum in explain.hip, so the block size is part of the result as it is there).  No multiply, so
// nothing can contract (contraction is off all the same).  A NaN difference, inf - inf among them, makes the sum
// NaN: no select.  M = 0 launches nothing (the wrapper returns zeros).
//
// Pass 1, item = (block of pairs, tile of A columns, tile of B columns), grid-stride.  The workgroup is 16 x 16
// lanes; a lane owns RA x RB outputs in registers (2 or 4 each way, so a tile is 32 or 64 columns each way), whose
// add chains interleave.  The block's gathered rows are staged in LDS sub-tiles, the tile's columns of A beside the
// tile's columns of B: 16-byte loads where the width is even and the table 16-byte aligned, 8-byte loads otherwise,
// one staging path.  A lane's columns are the pairs 2 t, 2 t + 1 of every stretch of 32, so the 16 lanes of a
// ds_read_b128 group read 256 contiguous bytes; every LDS value is used RB or RA times.  Columns past the table
// are staged as 0.0 on both sides and never written; pairs past the block's end are not visited.
// The block's partials go to scratch[block - b0][Wa][Wb].
// Pass 2, one lane per output, adds the blocks' partials in block order to the running sum: 0.0 at the first batch,
// C as the previous batch left it after that -- the same sequence of adds, so batching moves no bit.
//
// Plain launches on one stream; no workgroup waits on another; no atomics; every loop is bounded by its arguments.
#include <stdexcept>
#include <string>

#include "common.h"
#include "kernels.h"

namespace oni {

namespace {

constexpr int kSide = 16;              // lanes along each side of a tile
constexpr int kL1Threads = kSide * kSide;
constexpr int kL1Stage = 4096;         // doubles of staged rows (32 KiB)
constexpr int kFoldFlight = 8;         // partials a lane of pass 2 loads before it adds them

// Pairs m0 .. m0 + np of the table's columns c0 .. c0 + T into dst[np][ld] at column `at`; a column past W: 0.0.
// One lane per (pair, two columns).  vec: W even and the table 16-byte aligned (c0 is a multiple of 32).
template <int T>
__device__ __forceinline__ void stage_cols(double* __restrict__ dst, int ld, int at, const double* __restrict__ tab,
                                           int W, int c0, const int64_t* __restrict__ idx, int64_t m0, int np,
                                           int vec) {
  constexpr int H = T / 2;
  for (int t = threadIdx.x; t < np * H; t += kL1Threads) {
    const int p = t / H, c = (t % H) * 2;
    const int64_t row = idx ? idx[m0 + p] : m0 + p;
    const double* src = tab + (size_t)row * (size_t)W + (size_t)(c0 + c);
    double2 v;
    v.x = 0.0;
    v.y = 0.0;
    if (c0 + c + 1 < W) {
      if (vec) {
        v = *reinterpret_cast<const double2*>(src);
      } else {
        v.x = src[0];
        v.y = src[1];
      }
    } else if (c0 + c < W) {
      v.x = src[0];
    }
    *reinterpret_cast<double2*>(dst + p * ld + at + c) = v;
  }
}

template <int RA, int RB>
__global__ __launch_bounds__(kL1Threads) void column_l1_blocks_kernel(ColumnL1Args a, int nta, int ntb, int va,
                                                                      int vb) {
#pragma clang fp contract(off)
  constexpr int TA = kSide * RA, TB = kSide * RB, LD = TA + TB, SUB = kL1Stage / LD;
  __shared__ double2 l1_lds[kL1Stage / 2];
  double* st = reinterpret_cast<double*>(l1_lds);   // [SUB][TA + TB]
  const int ty = threadIdx.x / kSide, tx = threadIdx.x % kSide;
  const int64_t tiles = (int64_t)nta * ntb, items = a.nb * tiles;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t b = item / tiles;
    const int ca = (int)((item % tiles) / ntb) * TA, cb = (int)(item % ntb) * TB;
    // the lane works when its first column exists on both sides (its columns ascend)
    const bool live = ca + 2 * ty < a.Wa && cb + 2 * tx < a.Wb;
    double acc[RA][RB];
#pragma unroll
    for (int i = 0; i < RA; ++i)
#pragma unroll
      for (int j = 0; j < RB; ++j) acc[i][j] = 0.0;
    const int64_t m_lo = (a.b0 + b) * a.block, m_hi = m_lo + a.block < a.M ? m_lo + a.block : a.M;
    for (int64_t m0 = m_lo; m0 < m_hi; m0 += SUB) {
      const int np = (int)(m_hi - m0 < SUB ? m_hi - m0 : SUB);
      __syncthreads();   // the lanes are done with the previous sub-tile
      stage_cols<TA>(st, LD, 0, a.A, a.Wa, ca, a.ia, m0, np, va);
      stage_cols<TB>(st, LD, TA, a.B, a.Wb, cb, a.ib, m0, np, vb);
      __syncthreads();
      if (live) {
        const double2* pa = reinterpret_cast<const double2*>(st) + ty;
        const double2* pb = reinterpret_cast<const double2*>(st + TA) + tx;
#pragma unroll 2
        for (int p = 0; p < np; ++p) {
          double x[RA], y[RB];
#pragma unroll
          for (int h = 0; h < RA / 2; ++h) {
            const double2 q = pa[p * (LD / 2) + h * kSide];
            x[2 * h] = q.x;
            x[2 * h + 1] = q.y;
          }
#pragma unroll
          for (int h = 0; h < RB / 2; ++h) {
            const double2 q = pb[p * (LD / 2) + h * kSide];
            y[2 * h] = q.x;
            y[2 * h + 1] = q.y;
          }
#pragma unroll
          for (int i = 0; i < RA; ++i)
#pragma unroll
            for (int j = 0; j < RB; ++j) {
              const double t = x[i] - y[j];   // rounded difference, then rounded sum
              acc[i][j] = acc[i][j] + __builtin_fabs(t);
            }
        }
      }
    }
    if (live) {
      double* out = a.scratch + (size_t)b * (size_t)a.Wa * (size_t)a.Wb;
#pragma unroll
      for (int i = 0; i < RA; ++i) {
        const int ra = ca + (i / 2) * 2 * kSide + 2 * ty + i % 2;
#pragma unroll
        for (int j = 0; j < RB; ++j) {
          const int rb = cb + (j / 2) * 2 * kSide + 2 * tx + j % 2;
          if (ra < a.Wa && rb < a.Wb) out[(size_t)ra * a.Wb + rb] = acc[i][j];
        }
      }
    }
  }
}

// pass 2: one lane per output continues its running sum over the batch's blocks in block order
__global__ __launch_bounds__(kL1Threads) void column_l1_fold_kernel(ColumnL1Args a) {
  const int64_t cells = (int64_t)a.Wa * a.Wb;
  for (int64_t i = (int64_t)blockIdx.x * kL1Threads + threadIdx.x; i < cells; i += (int64_t)gridDim.x * kL1Threads) {
    double sum = a.first ? 0.0 : a.C[i];
    const double* p = a.scratch + i;
    int64_t b = 0;
    for (; b + kFoldFlight <= a.nb; b += kFoldFlight) {   // the loads together, the adds in block order
      double v[kFoldFlight];
#pragma unroll
      for (int u = 0; u < kFoldFlight; ++u) v[u] = p[(size_t)(b + u) * (size_t)cells];
#pragma unroll
      for (int u = 0; u < kFoldFlight; ++u) sum = sum + v[u];
    }
    for (; b < a.nb; ++b) sum = sum + p[(size_t)b * (size_t)cells];
    a.C[i] = sum;
  }
}

template <int RA, int RB>
void launch_blocks(const ColumnL1Args& a, int64_t cap, hipStream_t s) {
  constexpr int TA = kSide * RA, TB = kSide * RB;
  const int nta = (a.Wa + TA - 1) / TA, ntb = (a.Wb + TB - 1) / TB;
  int64_t blocks = a.nb * nta * ntb;
  if (blocks > cap) blocks = cap;
  const int va = a.Wa % 2 == 0 && (uintptr_t)a.A % 16 == 0, vb = a.Wb % 2 == 0 && (uintptr_t)a.B % 16 == 0;
  hipLaunchKernelGGL((column_l1_blocks_kernel<RA, RB>), dim3((unsigned)blocks), dim3(kL1Threads), 0, s, a, nta, ntb,
                     va, vb);
}

}  // namespace

int column_l1_tile(int W) { return W <= 2 * kSide ? 2 * kSide : 4 * kSide; }

void launch_column_l1(const ColumnL1Args& a, int max_blocks, hipStream_t s) {
  const std::string w("column_l1");
  if (a.Wa < 1 || a.Wb < 1 || a.Wa > kColumnL1WidthMax || a.Wb > kColumnL1WidthMax)
    throw std::runtime_error(w + ": Wa or Wb outside 1 .. " + std::to_string(kColumnL1WidthMax));
  if (a.M < 0 || a.M >= ((int64_t)1 << 40)) throw std::runtime_error(w + ": M outside 0 .. 2^40 - 1");
  if (a.Va < 0 || a.Vb < 0) throw std::runtime_error(w + ": Va or Vb < 0");
  if (a.block < 1 || a.block >= ((int64_t)1 << 31)) throw std::runtime_error(w + ": block outside 1 .. 2^31 - 1");
  if ((a.ia == nullptr) != (a.ib == nullptr)) throw std::runtime_error(w + ": ia and ib go together");
  if (!a.ia && (a.M > a.Va || a.M > a.Vb)) throw std::runtime_error(w + ": the identity form needs M <= Va, Vb");
  const int64_t nblk = (a.M + a.block - 1) / a.block;
  if (a.b0 < 0 || a.nb < 0 || a.b0 + a.nb > nblk) throw std::runtime_error(w + ": the batch's blocks outside the pairs");
  if (a.nb >= ((int64_t)1 << 31)) throw std::runtime_error(w + ": more than 2^31 - 1 blocks in a batch");
  if (max_blocks < 0) throw std::runtime_error(w + ": max_blocks < 0");
  if (a.nb == 0) return;
  if (!a.A || !a.B || !a.scratch || !a.C) throw std::runtime_error(w + ": null buffer");
  if ((uintptr_t)a.A % 8 != 0 || (uintptr_t)a.B % 8 != 0 || (uintptr_t)a.scratch % 8 != 0 || (uintptr_t)a.C % 8 != 0)
    throw std::runtime_error(w + ": a buffer is not 8-byte aligned");
  const int64_t cap = max_blocks > 0 ? max_blocks : 65536;
  const bool wa = a.Wa > 2 * kSide, wb = a.Wb > 2 * kSide;
  if (wa && wb) launch_blocks<4, 4>(a, cap, s);
  else if (wa) launch_blocks<4, 2>(a, cap, s);
  else if (wb) launch_blocks<2, 4>(a, cap, s);
  else launch_blocks<2, 2>(a, cap, s);
  ONI_HIP_CHECK(hipGetLastError());
  const int64_t cells = (int64_t)a.Wa * a.Wb;
  int64_t blocks = (cells + kL1Threads - 1) / kL1Threads;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(column_l1_fold_kernel, dim3((unsigned)blocks), dim3(kL1Threads), 0, s, a);
  ONI_HIP_CHECK(hipGetLastError());
}

}  // namespace oni
