// What the tail kernels share (tail_mass.hip: a side at a time; tail_docs.hip: a document's pairs share p): the
// partial sums of a side and a vocabulary block, the select-add, the scorers' member dots over plain and over padded
// rows, the staging of padded phi rows in LDS, the scratch cell of a (block, side) and the register ladder.  One
// definition, so the two kernels cannot drift apart in a bit.  expect.hip takes its member dots (dot_any, dot_reg)
// and the ladder from here too.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kernels.h"

namespace oni {
namespace tail {

constexpr int kThreads = 256;
constexpr int kRegMax = 100;   // doubles of a padded theta row in registers

struct Part {
  double le, tot;
  int rarer, ties;
};

__device__ __forceinline__ void take(Part& a, double p, double s) {
  // a select, then a plain rounded add: no branch in the sum.  A NaN p compares false everywhere.
  const double sel = p <= s ? p : 0.0;
  a.le = a.le + sel;
  a.tot = a.tot + p;
  a.rarer += p < s ? 1 : 0;
  a.ties += p == s ? 1 : 0;
}

// the scorers' member dots over rows of any width; th advances by `ts` doubles per element
__device__ __forceinline__ double dot_any(const double* __restrict__ th, int ts, const double* __restrict__ p, int R,
                                          int K, double rd) {
#pragma clang fp contract(off)
  double sum = 0.0;
  for (int r = 0; r < R; ++r) {
    double acc = 0.0;
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
      const double prod = th[(size_t)(r * K + k) * ts] * p[r * K + k];   // rounded product, then rounded sum
      acc = acc + prod;
    }
    sum = sum + acc;
  }
  return R == 1 ? sum : sum / rd;   // x / 1.0 is x
}

// the same over padded rows: th in registers [TM][TK], p in LDS [TM][TK], 0.0 in the padding of both
template <int TK, int TM>
__device__ __forceinline__ double dot_pad(const double (&th)[TK * TM], const double2* __restrict__ p, int R,
                                          double rd) {
#pragma clang fp contract(off)
  double sum = 0.0;
#pragma unroll
  for (int m = 0; m < TM; ++m) {
    if (m < R) {   // uniform; a member past R would add +0.0
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < TK; k += 2) {
        const double2 q = p[(m * TK + k) / 2];
        const double p0 = th[m * TK + k] * q.x;
        acc = acc + p0;
        const double p1 = th[m * TK + k + 1] * q.y;
        acc = acc + p1;
      }
      sum = sum + acc;
    }
  }
  return R == 1 ? sum : sum / rd;
}

// the same with th padded in registers [TM][TK] and p one plain row [R][K] in global memory (expect.hip: the rows
// of a group are gathered through an order, so nothing stages them).  A member's loads are issued together, ahead
// of the sums: a topic past K loads the row's last topic again and is left out of the sum (it would add 0.0 * x to
// a sum that started at +0.0).  VEC: K even and p 16-byte aligned, two topics per load.
template <int TK, int TM, bool VEC>
__device__ __forceinline__ double dot_reg(const double (&th)[TK * TM], const double* __restrict__ p, int R, int K,
                                          double rd) {
#pragma clang fp contract(off)
  double sum = 0.0;
#pragma unroll
  for (int m = 0; m < TM; ++m) {
    if (m < R) {   // uniform
      const double* pm = p + m * K;
      double2 q[TK / 2];
#pragma unroll
      for (int k = 0; k < TK; k += 2) {
        if (VEC) {
          q[k / 2] = reinterpret_cast<const double2*>(pm)[(k < K ? k : K - 2) / 2];
        } else {
          q[k / 2].x = pm[k < K ? k : K - 1];
          q[k / 2].y = pm[k + 1 < K ? k + 1 : K - 1];
        }
      }
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < TK; k += 2) {
        if (k < K) {   // uniform
          const double p0 = th[m * TK + k] * q[k / 2].x;
          acc = acc + p0;
        }
        if (k + 1 < K) {
          const double p1 = th[m * TK + k + 1] * q[k / 2].y;
          acc = acc + p1;
        }
      }
      sum = sum + acc;
    }
  }
  return R == 1 ? sum : sum / rd;
}

// nr phi rows from r0 on into LDS, each member run padded from K to TK topics with 0.0, rows `stride` doubles apart
// (stride >= R TK, even); one (row, member) run per lane.  vec: K even and phi 16-byte aligned, so is every run.
__device__ __forceinline__ void stage_rows(double* __restrict__ dst, int stride, const double* __restrict__ phi,
                                           int64_t r0, int nr, int R, int K, int TK, int vec) {
  const int RK = R * K;
  for (int t = threadIdx.x; t < nr * R; t += kThreads) {
    const int row = t / R, m = t % R;
    const double* src = phi + (size_t)(r0 + row) * RK + (size_t)m * K;
    double* to = dst + row * stride + m * TK;
    if (vec) {
      for (int k = 0; k < K / 2; ++k) reinterpret_cast<double2*>(to)[k] = reinterpret_cast<const double2*>(src)[k];
    } else {
      for (int k = 0; k < K; ++k) to[k] = src[k];
    }
    for (int k = K; k < TK; ++k) to[k] = 0.0;
  }
}

// a side's four partials of block b into its scratch cell
__device__ __forceinline__ void put(const TailArgs& a, int64_t b, int64_t i, const Part& pt) {
  const size_t cells = (size_t)a.nblk * (size_t)a.n, at = (size_t)b * (size_t)a.n + (size_t)i;
  double* sd = a.scratch;
  int* si = reinterpret_cast<int*>(sd + 2 * cells);
  sd[at] = pt.le;
  sd[cells + at] = pt.tot;
  si[at] = pt.rarer;
  si[cells + at] = pt.ties;
}

constexpr int kLadder[] = {4, 8, 20, 32, 50, 100};

// padded topics of the register form, 0 when the row does not fit it
inline int reg_topics(int R, int K) {
  for (int tk : kLadder)
    if (K <= tk) return R == 1 || R <= kRegMax / tk ? tk : 0;
  return 0;
}

}  // namespace tail

// the checks both launches make of their arguments; false: n == 0, nothing to launch
bool tail_args_check(const TailArgs& a, int max_blocks, const char* who);
// pass 2 of both (tail_mass.hip): one lane per side adds its blocks' partials from 0.0 in block order
void launch_tail_fold(const TailArgs& a, int64_t cap, hipStream_t s);

}  // namespace oni
