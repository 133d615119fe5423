// --expect: the value a host would normally show in a field of a flagged event's word (pipeline/common.py
// write_expect; twin: ops/reference.py expect_sides).
//
// An item is a distinct (document d, word w) pair of the written sides and one explained field f of the word.  Its
// group N_f(w) -- the vocabulary's words that agree with w on every field but f, w among them -- is a segment of a
// row order (score/scorer.py field_segments).  For every member v of the group, p_v is the pair's score with phi
// row v in place of w, evaluated as the scorers evaluate it (tail_common.h dot_any / dot_reg: per member of the
// ensemble a rounded product and a rounded sum per topic, in topic order from 0.0, the members added in order from
// 0.0 and divided by (double)R; contraction off); d = -1 takes the default vector for theta.  s = p_w.
//
//   best   the member with the greatest p_v under IEEE >: a NaN never wins, ties go to the lowest phi row
//          (-0.0 and +0.0 tie); -1 when no member has a p_v that is a number
//   pbest  that member's p_v (NaN without one)
//   above  the number of members with p_v > s
//
// Where explain.hip's group sums had to fix a block order for their bits, nothing here does: a maximum, a
// lowest-row tie-break and an integer count give the same result in whatever order the members are visited, and
// every p_v has one fixed evaluation order of its own.  So the results are identical for every grid and every
// block cut; there are no floating-point sums across members and hence no floating-point atomics.
//
// Pass 1, one lane per (item, block of `block` members), grid-stride.  The host sorts the items by group, so the
// lanes of a wave mostly walk the same member rows in step and their phi loads are one address.  The lane holds
// its theta row in registers on the ladder of tail_common.h where the width fits and reads it from global memory
// otherwise; phi rows are 16-byte loads at an even K and an aligned table.  s is evaluated by every lane, once per
// (item, block) and not once per item: one more dot per block of members, the same bits in each.  An item of one
// block is written
// straight to the outputs, the others' blocks to a scratch.  Pass 2, one lane per item, folds the blocks of a
// longer item -- the greater p wins, the lower row on a tie, the counts are added -- and writes the items without
// a value.  A group of half a million members is thus walked by two thousand lanes, not by one.
#include <stdexcept>
#include <string>

#include "common.h"
#include "kernels.h"
#include "tail_common.h"

namespace oni {

namespace {

using tail::dot_any;
using tail::dot_reg;
using tail::kRegMax;
using tail::kThreads;
using tail::reg_topics;

struct Best {
  double p;
  int row;     // -1: none yet
  int above;
};

// one member into a running result; s fixed
__device__ __forceinline__ void take(Best& b, double p, int v, double s) {
  b.above += p > s ? 1 : 0;   // a NaN on either side counts nothing
  if (p == p && (b.row < 0 || p > b.p || (p == b.p && v < b.row))) {
    b.p = p;
    b.row = v;
  }
}

__device__ __forceinline__ void store(const ExpectArgs& a, const Best& b, bool single, int64_t blk, int64_t at) {
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  if (single) {
    a.best[at] = b.row;
    a.pbest[at] = b.row < 0 ? nan : b.p;
    a.above[at] = b.above;
  } else {
    a.part_best[blk] = b.row;
    a.part_p[blk] = b.p;
    a.part_above[blk] = b.above;
  }
}

// the block's item and its member range
struct Cut {
  int64_t it, m0, m1;
  bool single;
};
__device__ __forceinline__ Cut cut_of(const ExpectArgs& a, int64_t blk) {
  Cut c;
  c.it = a.blk_item[blk];
  const int64_t b0 = a.blk_off[c.it];
  c.single = a.blk_off[c.it + 1] - b0 == 1;
  c.m0 = a.seg_start[c.it] + (blk - b0) * a.block;
  const int64_t e = a.seg_end[c.it];
  c.m1 = c.m0 + a.block < e ? c.m0 + a.block : e;
  return c;
}

// pass 1, theta row padded in registers
template <int TK, int TM, bool VEC>
__global__ __launch_bounds__(kThreads) void expect_blocks_reg_kernel(ExpectArgs a) {
  constexpr int W = TK * TM;
  const int K = a.K, R = a.R, RK = a.R * a.K;
  const double rd = (double)R;
  for (int64_t blk = (int64_t)blockIdx.x * kThreads + threadIdx.x; blk < a.B; blk += (int64_t)gridDim.x * kThreads) {
    const Cut c = cut_of(a, blk);
    const int d = a.doc[c.it];
    double th[W];
#pragma unroll
    for (int m = 0; m < TM; ++m)
#pragma unroll
      for (int k = 0; k < TK; ++k)
        th[m * TK + k] = m < R && k < K ? (d >= 0 ? a.theta[(size_t)d * RK + m * K + k] : a.dflt) : 0.0;
    const double s = dot_reg<TK, TM, VEC>(th, a.phi + (size_t)a.word[c.it] * RK, R, K, rd);
    Best b{0.0, -1, 0};
    if (W <= 50) {   // two rows in flight where the registers allow it
#pragma unroll 2
      for (int64_t m = c.m0; m < c.m1; ++m) {
        const int v = a.order[m];
        take(b, dot_reg<TK, TM, VEC>(th, a.phi + (size_t)v * RK, R, K, rd), v, s);
      }
    } else {
#pragma unroll 1
      for (int64_t m = c.m0; m < c.m1; ++m) {
        const int v = a.order[m];
        take(b, dot_reg<TK, TM, VEC>(th, a.phi + (size_t)v * RK, R, K, rd), v, s);
      }
    }
    store(a, b, c.single, blk, a.out_at[c.it]);
  }
}

// pass 1, any row width: both rows from global memory
__global__ __launch_bounds__(kThreads) void expect_blocks_global_kernel(ExpectArgs a) {
  const int K = a.K, R = a.R;
  const size_t RK = (size_t)a.R * a.K;
  const double rd = (double)R;
  for (int64_t blk = (int64_t)blockIdx.x * kThreads + threadIdx.x; blk < a.B; blk += (int64_t)gridDim.x * kThreads) {
    const Cut c = cut_of(a, blk);
    const int d = a.doc[c.it];
    // without a document every topic of every member is the default value: a stride of 0 over one double
    const double* tr = d >= 0 ? a.theta + (size_t)d * RK : &a.dflt;
    const int ts = d >= 0 ? 1 : 0;
    const double s = dot_any(tr, ts, a.phi + (size_t)a.word[c.it] * RK, R, K, rd);
    Best b{0.0, -1, 0};
    for (int64_t m = c.m0; m < c.m1; ++m) {
      const int v = a.order[m];
      take(b, dot_any(tr, ts, a.phi + (size_t)v * RK, R, K, rd), v, s);
    }
    store(a, b, c.single, blk, a.out_at[c.it]);
  }
}

// pass 2: one lane per item of no block or of more than one
__global__ __launch_bounds__(kThreads) void expect_fold_kernel(ExpectArgs a) {
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  for (int64_t it = (int64_t)blockIdx.x * kThreads + threadIdx.x; it < a.n; it += (int64_t)gridDim.x * kThreads) {
    const int64_t b0 = a.blk_off[it], nb = a.blk_off[it + 1] - b0;
    if (nb == 1) continue;   // written by pass 1
    const int64_t at = a.out_at[it];
    if (nb == 0) {   // no word or no group: -1, NaN, -1; a group without members: -1, NaN, 0
      a.best[at] = -1;
      a.pbest[at] = nan;
      a.above[at] = a.seg_start[it] < 0 ? -1 : 0;
      continue;
    }
    Best b{0.0, -1, 0};
    for (int64_t j = 0; j < nb; ++j) {
      const int row = a.part_best[b0 + j];
      const double p = a.part_p[b0 + j];
      b.above += a.part_above[b0 + j];
      if (row >= 0 && (b.row < 0 || p > b.p || (p == b.p && row < b.row))) {
        b.p = p;
        b.row = row;
      }
    }
    a.best[at] = b.row;
    a.pbest[at] = b.row < 0 ? nan : b.p;
    a.above[at] = b.above;
  }
}

template <int TK, bool VEC>
void launch_reg(const ExpectArgs& a, unsigned blocks, hipStream_t s) {
  constexpr int TM = kRegMax / TK;
  if (a.R == 1)
    hipLaunchKernelGGL((expect_blocks_reg_kernel<TK, 1, VEC>), dim3(blocks), dim3(kThreads), 0, s, a);
  else
    hipLaunchKernelGGL((expect_blocks_reg_kernel<TK, TM, VEC>), dim3(blocks), dim3(kThreads), 0, s, a);
}

template <bool VEC>
void launch_ladder(const ExpectArgs& a, unsigned blocks, hipStream_t s) {
  switch (reg_topics(a.R, a.K)) {
    case 4: launch_reg<4, VEC>(a, blocks, s); break;
    case 8: launch_reg<8, VEC>(a, blocks, s); break;
    case 20: launch_reg<20, VEC>(a, blocks, s); break;
    case 32: launch_reg<32, VEC>(a, blocks, s); break;
    case 50: launch_reg<50, VEC>(a, blocks, s); break;
    default: launch_reg<100, VEC>(a, blocks, s); break;
  }
}

}  // namespace

int expect_theta_path(int R, int K) {
  if (R < 1 || K < 1 || R > kEnsembleMax) throw std::runtime_error("expect_theta_path: R or K out of range");
  return reg_topics(R, K) ? kExpectRegisters : kExpectGlobal;
}

void launch_expect_sides(const ExpectArgs& a, int max_blocks, hipStream_t s) {
  if (a.n < 0 || a.n >= ((int64_t)1 << 31) || a.B < 0 || a.B >= ((int64_t)1 << 31))
    throw std::runtime_error("expect_sides: n or B outside 0 .. 2^31 - 1");
  if (a.R < 1 || a.R > kEnsembleMax)
    throw std::runtime_error("expect_sides: R outside 1 .. " + std::to_string(kEnsembleMax));
  if (a.K < 1 || (int64_t)a.R * a.K >= ((int64_t)1 << 31)) throw std::runtime_error("expect_sides: K < 1 or R K >= 2^31");
  if (a.block < 1) throw std::runtime_error("expect_sides: block < 1");
  if (max_blocks < 0) throw std::runtime_error("expect_sides: max_blocks < 0");
  if (a.n == 0) return;
  if (!a.seg_start || !a.seg_end || !a.out_at || !a.blk_off || !a.best || !a.pbest || !a.above)
    throw std::runtime_error("expect_sides: null buffer");
  // (theta may have no row at all: every item then takes the default vector)
  if (a.B > 0 && (!a.phi || !a.order || !a.doc || !a.word || !a.blk_item || !a.part_p || !a.part_best ||
                  !a.part_above))
    throw std::runtime_error("expect_sides: null buffer");
  const int64_t cap = max_blocks > 0 ? max_blocks : 65536;
  if (a.B > 0) {
    int64_t blocks = (a.B + kThreads - 1) / kThreads;
    if (blocks > cap) blocks = cap;
    if (expect_theta_path(a.R, a.K) == kExpectRegisters) {
      if (a.K % 2 == 0 && (uintptr_t)a.phi % 16 == 0)
        launch_ladder<true>(a, (unsigned)blocks, s);
      else
        launch_ladder<false>(a, (unsigned)blocks, s);
    } else {
      hipLaunchKernelGGL(expect_blocks_global_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, a);
    }
    ONI_HIP_CHECK(hipGetLastError());
  }
  int64_t blocks = (a.n + kThreads - 1) / kThreads;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(expect_fold_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, a);
  ONI_HIP_CHECK(hipGetLastError());
}

}  // namespace oni
