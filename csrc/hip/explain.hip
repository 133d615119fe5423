// --explain: which field of its word makes a flagged event side rare (pipeline/common.py write_explain; twins:
// ops/reference.py group_rows_sum, explain_sides).
//
// A word is a mixed-radix key over named fields.  For a side (document d, word w) and a field f, N_f(w) is the
// group of the vocabulary's words that agree with w on every field but f.  With
//
//   s   = theta_d . phi_w                         (the side's score, score_ensemble.hip bit for bit)
//   m_f = theta_d . (sum of phi over N_f(w))      (the same event with field f left open)
//
// cond_f = s / m_f is the model's probability of the value w has in field f given the document and the other
// fields.  Two kernels:
//
// group_rows_sum  the group sums.  A group is a segment of a row order; it is cut into blocks of `block` members,
//   a block is summed from 0.0 in member order, a group's block sums are added from 0.0 in block order: one set of
//   bits whatever the launch shape, no atomics.  Pass 1 runs over (block, column): a team of lanes along the
//   columns, so a member row is one contiguous read, eight members' loads issued ahead of their dependent adds;
//   a group of one block is written straight to the output, the others' block sums to a scratch.  Pass 2 runs
//   over (group, column) and adds a group's block sums in order.  A long group is thus summed by many teams.
// explain_sides   one lane per side, grid-stride.  The theta row is read once: the member dot of the phi row and
//   of the F group rows advance together, each in topic order with rounded products and sums (contraction off),
//   members added from 0.0 in member order and divided by (double)R, as score_ensemble does.
#include <stdexcept>
#include <string>

#include "common.h"
#include "kernels.h"

namespace oni {

namespace {

constexpr int kThreads = 256;
constexpr int kAhead = 8;   // member rows loaded ahead of the adds that consume them

// a column element: one double, or with an even row width and 16-byte aligned tables two
template <bool VEC>
struct Col;
template <>
struct Col<false> {
  using T = double;
  static __device__ __forceinline__ T zero() { return 0.0; }
  static __device__ __forceinline__ void add(T& a, const T& b) { a = a + b; }
};
template <>
struct Col<true> {
  using T = double2;
  static __device__ __forceinline__ T zero() { return make_double2(0.0, 0.0); }
  static __device__ __forceinline__ void add(T& a, const T& b) {
    a.x = a.x + b.x;
    a.y = a.y + b.y;
  }
};

// pass 1: item = one block of one segment; `team` lanes (a power of two <= kThreads) share an item
template <bool VEC>
__global__ __launch_bounds__(kThreads) void group_block_sums_kernel(GroupRowsArgs a, int team) {
  using C = Col<VEC>;
  using T = typename C::T;
  const int CL = VEC ? a.W / 2 : a.W;   // column elements of a row
  const int teams = kThreads / team;
  const int lane = threadIdx.x % team;
  const T* tab = reinterpret_cast<const T*>(a.table);
  for (int64_t b = (int64_t)blockIdx.x * teams + threadIdx.x / team; b < a.B; b += (int64_t)gridDim.x * teams) {
    // the block's segment: the last g with blk_off[g] <= b (empty segments share their successor's offset)
    int64_t lo = 0, hi = a.G;
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (a.blk_off[mid] <= b) lo = mid; else hi = mid;
    }
    const int64_t g = lo, b0 = a.blk_off[g];
    const bool single = a.blk_off[g + 1] - b0 == 1;
    const int64_t s = a.seg_start[g] + (b - b0) * a.block;
    const int64_t e = s + a.block < a.seg_end[g] ? s + a.block : a.seg_end[g];
    T* dst = reinterpret_cast<T*>(single ? a.out + (size_t)g * a.W : a.scratch + (size_t)b * a.W);
    for (int c = lane; c < CL; c += team) {
      T acc = C::zero();
      int64_t m = s;
      for (; m + kAhead <= e; m += kAhead) {
        T v[kAhead];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) v[u] = tab[(size_t)a.order[m + u] * CL + c];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) C::add(acc, v[u]);
      }
      for (; m < e; ++m) C::add(acc, tab[(size_t)a.order[m] * CL + c]);
      dst[c] = acc;
    }
  }
}

// pass 2: item = one segment of no block (a row of zeros) or of more than one
template <bool VEC>
__global__ __launch_bounds__(kThreads) void group_fold_blocks_kernel(GroupRowsArgs a, int team) {
  using C = Col<VEC>;
  using T = typename C::T;
  const int CL = VEC ? a.W / 2 : a.W;
  const int teams = kThreads / team;
  const int lane = threadIdx.x % team;
  const T* part = reinterpret_cast<const T*>(a.scratch);
  for (int64_t g = (int64_t)blockIdx.x * teams + threadIdx.x / team; g < a.G; g += (int64_t)gridDim.x * teams) {
    const int64_t b0 = a.blk_off[g], nb = a.blk_off[g + 1] - b0;
    if (nb == 1) continue;   // written by pass 1
    T* dst = reinterpret_cast<T*>(a.out + (size_t)g * a.W);
    for (int c = lane; c < CL; c += team) {
      T acc = C::zero();
      int64_t j = 0;
      for (; j + kAhead <= nb; j += kAhead) {
        T v[kAhead];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) v[u] = part[(size_t)(b0 + j + u) * CL + c];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) C::add(acc, v[u]);
      }
      for (; j < nb; ++j) C::add(acc, part[(size_t)(b0 + j) * CL + c]);
      dst[c] = acc;
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void explain_sides_kernel(ExplainArgs a) {
  // HIP compiles with -ffp-contract=fast; the JVM rounds the product and the sum separately.
#pragma clang fp contract(off)
  constexpr int NF = kExplainMaxFields;
  const int K = a.K, F = a.F;
  const size_t run = (size_t)a.R * K;   // doubles of one row's members
  const double rd = (double)a.R;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kThreads) {
    const int d = a.doc[i], w = a.word[i];
    double* co = a.cond + (size_t)i * F;
    if (w < 0) {   // no phi row: nothing to explain
      for (int f = 0; f < F; ++f) co[f] = nan;
      a.why[i] = 255;
      continue;
    }
    const double* tr = d >= 0 ? a.theta + (size_t)d * run : nullptr;
    // row 0: the phi row; row 1 + f: the group row of field f, nullptr without one
    const double* rows[NF + 1];
    rows[0] = a.phi + (size_t)w * run;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const int g = f < F ? a.grow[(size_t)i * F + f] : -1;
      rows[f + 1] = g >= 0 ? a.gsum + (size_t)g * run : nullptr;
    }
    double sum[NF + 1];
#pragma unroll
    for (int j = 0; j <= NF; ++j) sum[j] = 0.0;
    for (int r = 0; r < a.R; ++r) {
      const size_t o = (size_t)r * K;
      double acc[NF + 1];
#pragma unroll
      for (int j = 0; j <= NF; ++j) acc[j] = 0.0;
      if (VEC) {
        for (int k = 0; k < K / 2; ++k) {
          const double2 t = tr ? reinterpret_cast<const double2*>(tr + o)[k] : make_double2(a.dflt, a.dflt);
#pragma unroll
          for (int j = 0; j <= NF; ++j) {
            if (rows[j]) {
              const double2 p = reinterpret_cast<const double2*>(rows[j] + o)[k];
              const double p0 = t.x * p.x;   // contract(off): rounded product, then rounded sum
              acc[j] = acc[j] + p0;
              const double p1 = t.y * p.y;
              acc[j] = acc[j] + p1;
            }
          }
        }
      } else {
        for (int k = 0; k < K; ++k) {
          const double t = tr ? tr[o + k] : a.dflt;
#pragma unroll
          for (int j = 0; j <= NF; ++j) {
            if (rows[j]) {
              const double prod = t * rows[j][o + k];
              acc[j] = acc[j] + prod;
            }
          }
        }
      }
#pragma unroll
      for (int j = 0; j <= NF; ++j) sum[j] = sum[j] + acc[j];
    }
    const double s = sum[0] / rd;
    double best = 0.0;
    unsigned why = 255;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      if (f < F) {
        const double m = sum[f + 1] / rd;
        const double c = rows[f + 1] ? s / m : nan;
        co[f] = c;
        if (c == c && (why == 255 || c < best)) {   // '<': ties go to the lowest field
          best = c;
          why = (unsigned)f;
        }
      }
    }
    a.why[i] = (uint8_t)why;
  }
}

int team_of(int cl) {
  int t = 1;
  while (t < cl && t < kThreads) t <<= 1;
  return t;
}

}  // namespace

void launch_group_rows_sum(const GroupRowsArgs& a, int max_blocks, hipStream_t s) {
  if (a.G < 0 || a.G >= ((int64_t)1 << 31) || a.B < 0 || a.B >= ((int64_t)1 << 31))
    throw std::runtime_error("group_rows_sum: G or B outside 0 .. 2^31 - 1");
  if (a.W < 1) throw std::runtime_error("group_rows_sum: W < 1");
  if (a.block < 1) throw std::runtime_error("group_rows_sum: block < 1");
  if (max_blocks < 0) throw std::runtime_error("group_rows_sum: max_blocks < 0");
  if (a.G == 0) return;
  if (!a.seg_start || !a.seg_end || !a.blk_off || !a.out) throw std::runtime_error("group_rows_sum: null buffer");
  if (a.B > 0 && (!a.table || !a.order || !a.scratch)) throw std::runtime_error("group_rows_sum: null buffer");
  const bool vec = a.W % 2 == 0 && ((uintptr_t)a.table % 16 == 0) && ((uintptr_t)a.scratch % 16 == 0) &&
                   ((uintptr_t)a.out % 16 == 0);
  const int team = team_of(vec ? a.W / 2 : a.W);
  const int teams = kThreads / team;
  const int64_t cap = max_blocks > 0 ? max_blocks : 4096;
  if (a.B > 0) {
    int64_t blocks = (a.B + teams - 1) / teams;
    if (blocks > cap) blocks = cap;
    if (vec)
      hipLaunchKernelGGL((group_block_sums_kernel<true>), dim3((unsigned)blocks), dim3(kThreads), 0, s, a, team);
    else
      hipLaunchKernelGGL((group_block_sums_kernel<false>), dim3((unsigned)blocks), dim3(kThreads), 0, s, a, team);
    ONI_HIP_CHECK(hipGetLastError());
  }
  int64_t blocks = (a.G + teams - 1) / teams;
  if (blocks > cap) blocks = cap;
  if (vec)
    hipLaunchKernelGGL((group_fold_blocks_kernel<true>), dim3((unsigned)blocks), dim3(kThreads), 0, s, a, team);
  else
    hipLaunchKernelGGL((group_fold_blocks_kernel<false>), dim3((unsigned)blocks), dim3(kThreads), 0, s, a, team);
  ONI_HIP_CHECK(hipGetLastError());
}

void launch_explain_sides(const ExplainArgs& a, int max_blocks, hipStream_t s) {
  if (a.n < 0 || a.n >= ((int64_t)1 << 31)) throw std::runtime_error("explain_sides: n outside 0 .. 2^31 - 1");
  if (a.R < 1 || a.R > kEnsembleMax)
    throw std::runtime_error("explain_sides: R outside 1 .. " + std::to_string(kEnsembleMax));
  if (a.K < 1) throw std::runtime_error("explain_sides: K < 1");
  if (a.F < 1 || a.F > kExplainMaxFields)
    throw std::runtime_error("explain_sides: F outside 1 .. " + std::to_string(kExplainMaxFields));
  if (max_blocks < 0) throw std::runtime_error("explain_sides: max_blocks < 0");
  if (a.n == 0) return;
  if (!a.theta || !a.phi || !a.gsum || !a.doc || !a.word || !a.grow || !a.cond || !a.why)
    throw std::runtime_error("explain_sides: null buffer");
  int64_t blocks = (a.n + kThreads - 1) / kThreads;
  const int64_t cap = max_blocks > 0 ? max_blocks : 8192;
  if (blocks > cap) blocks = cap;
  const bool vec = a.K % 2 == 0 && ((uintptr_t)a.theta % 16 == 0) && ((uintptr_t)a.phi % 16 == 0) &&
                   ((uintptr_t)a.gsum % 16 == 0);
  if (vec)
    hipLaunchKernelGGL((explain_sides_kernel<true>), dim3((unsigned)blocks), dim3(kThreads), 0, s, a);
  else
    hipLaunchKernelGGL((explain_sides_kernel<false>), dim3((unsigned)blocks), dim3(kThreads), 0, s, a);
  ONI_HIP_CHECK(hipGetLastError());
}

}  // namespace oni
