// --topic-report: what the topics are (pipeline/common.py write_topic_report; twins: ops/reference.py column_topn,
// row_dominant, topic_sides).
//
// column_topn: per column of a table [rows][W] the N rows first in the total order (value descending under IEEE >,
// row ascending): equal values, -0.0 and +0.0 among them, go to the lower row, a NaN never enters.  The top N of a
// set under a total order does not depend on how the set is cut or in which order the pieces are merged, so no
// block order is part of the result: the same bits for every grid, block size and batch, and no atomics.
//
// Pass 1, item = (tile of columns, block of rows), grid-stride over the blocks.  Lanes run along the columns, so a wave reads a
// stretch of one row: consecutive lanes, consecutive doubles.  A table narrower than the workgroup (W <= T / 2)
// would leave lanes idle, so the lanes form G = T / W sub-groups of W lanes; sub-group g walks the block's rows
// g, g + G, ...  A lane keeps its list -- N (value, row) pairs in the total order -- in an LDS slice of its own,
// [slot][lane], so a slot is one conflict-free access per lane; the LDS is sized at the launch, N x T x 12 bytes,
// with T = 256 lanes up to N = 16 and 128 past it (at most 48 KiB).  The sub-groups' lists of a column are merged
// in LDS by a tree over g; the lists hold rows in no common order then, so an offer compares rows on ties.  The
// block's list goes to scratch[block][slot][column].
// A lower bound of a column's N-th value lets pass 1 skip whatever lies below it: the rows of any subset that are
// listed all precede such a value in the total order, so it cannot be among the N and the result is the same.  The
// wrapper takes the bound (tau) from this kernel pair run over a strided sample of the rows (ld: the doubles
// between two rows of the launch); after it almost no value reaches a list and pass 1 is a compare per load.
// Pass 2, item = tile of columns: sub-group g offers the lists of the blocks g, g + G, ... to its list, the same
// tree merges them, sub-group 0 writes the result.  A block's list descends: past its end, or past the first entry
// that does not enter, nothing enters.  A lane reads its blocks' lists one after the other, so past
// kTopicMergeGroup blocks there are two levels: groups of that many blocks are merged side by side, one workgroup
// each, into a second scratch, then the groups' lists into the result (4.5 M rows in blocks of 4096: 1,099 lists
// become 18, and no lane reads more than 64).
//
// row_dominant: one lane per (row, member), grid-stride: the first k attaining the maximum of the member's K
// values (a NaN never wins; -1: all NaN) and the rows per (member, k) -- integers, counted in an LDS histogram per
// workgroup that is flushed once with integer atomics.
//
// topic_sides: one lane per side, grid-stride.  Over j = 0 .. W - 1 in order p_j = theta[d][j] * phi[w][j], one
// rounded product (contraction off); the side's score s exactly as score_ensemble.hip adds it (member sums in
// topic order, the members in member order, one division by (double)R); the first j with the greatest p_j (a NaN
// never wins); resp = p* / (s * (double)R), one rounded multiply and one rounded division.
//
// Plain launches on one stream; no workgroup waits on another; every loop is bounded by its arguments.
#include <stdexcept>
#include <string>

#include "common.h"
#include "kernels.h"

namespace oni {

namespace {

constexpr int kDomThreads = 256;
constexpr int kFlight = 8;   // rows a lane of pass 1 loads before it offers them

__device__ __forceinline__ double neg_inf() { return __longlong_as_double(0xfff0000000000000LL); }
__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// a lane's list in LDS: slot s at ld[s * T] / lr[s * T]
struct TopList {
  double* ld;
  int* lr;
  int T, N, cnt;
  double worst;   // the last entry of a full list (-inf until then: any non-NaN value enters a short list)
  int worst_row;
};

// the candidate (v, p) to the list, in the total order (v descending, p ascending).  false: it did not enter.
__device__ __forceinline__ bool offer(TopList& l, double v, int p) {
  if (l.cnt < l.N) {
    if (!(v == v)) return false;   // a NaN never enters
  } else if (!(v > l.worst || (v == l.worst && p < l.worst_row))) {
    return false;
  }
  int s = l.cnt < l.N ? l.cnt : l.N - 1;   // the slot that opens: the end of a short list, else the last drops out
  while (s > 0) {
    const double u = l.ld[(s - 1) * l.T];
    if (!(u < v || (u == v && l.lr[(s - 1) * l.T] > p))) break;
    l.ld[s * l.T] = u;
    l.lr[s * l.T] = l.lr[(s - 1) * l.T];
    --s;
  }
  l.ld[s * l.T] = v;
  l.lr[s * l.T] = p;
  if (l.cnt < l.N) ++l.cnt;
  if (l.cnt == l.N) {
    l.worst = l.ld[(l.N - 1) * l.T];
    l.worst_row = l.lr[(l.N - 1) * l.T];
  }
  return true;
}

__device__ __forceinline__ TopList list_of(double2* lds, int N) {
  const int T = blockDim.x;
  double* base = reinterpret_cast<double*>(lds);
  TopList l;
  l.ld = base + threadIdx.x;
  l.lr = reinterpret_cast<int*>(base + (size_t)N * T) + threadIdx.x;
  l.T = T;
  l.N = N;
  l.cnt = 0;
  l.worst = neg_inf();
  l.worst_row = -1;
  return l;
}

// The G sub-groups' lists of a column (lanes g * cw + c) merged into sub-group 0's by a tree over g.  cnt_lds[T]:
// the lanes' counts.  Every lane of the workgroup calls it (the barriers); a lane outside every sub-group has
// g >= G.  Ends with a barrier: the lists may be reused after it.
__device__ __forceinline__ void tree_merge(TopList& l, int* cnt_lds, int g, int G, int cw) {
  cnt_lds[threadIdx.x] = l.cnt;
  for (int step = 1; step < G; step *= 2) {
    __syncthreads();   // the lists and counts of the previous round are written
    if (g < G && g % (2 * step) == 0 && g + step < G) {
      const int other = step * cw;   // the partner lane, relative to this one
      const int oc = cnt_lds[threadIdx.x + other];
      for (int s = 0; s < oc; ++s)
        if (!offer(l, l.ld[s * l.T + other], l.lr[s * l.T + other])) break;   // its list descends: nothing after
      cnt_lds[threadIdx.x] = l.cnt;
    }
  }
  __syncthreads();
}

// this lane's sub-group g and column c of the tile; false: the lane has none
__device__ __forceinline__ bool lane_place(const TopnArgs& a, int G, int tile, int& g, int& c) {
  const int T = blockDim.x;
  if (G > 1) {
    g = threadIdx.x / a.wb;
    c = threadIdx.x % a.wb;
    return g < G;
  }
  g = 0;
  c = tile * T + threadIdx.x;
  return c < a.wb;
}

// grid: x strides over the blocks of rows, y is the tile of columns
__global__ __launch_bounds__(256) void topn_blocks_kernel(TopnArgs a, int G) {
  extern __shared__ double2 topic_lds[];
  const int T = blockDim.x, N = a.N;
  int* cnt_lds = reinterpret_cast<int*>(reinterpret_cast<double*>(topic_lds) + (size_t)N * T) + (size_t)N * T;
  const int nblk = (int)a.nblk, tile = blockIdx.y;   // nblk <= 2^30: checked at the launch
  for (int b = blockIdx.x; b < nblk; b += gridDim.x) {
    int g, c;
    const bool ok = lane_place(a, G, tile, g, c);
    TopList l = list_of(topic_lds, N);
    if (ok) {
      const int64_t v0 = (int64_t)b * a.block, v1 = v0 + a.block < a.rows ? v0 + a.block : a.rows;
      const double low = a.tau ? a.tau[a.c0 + c] : neg_inf();   // nothing below it can be among the N
      const size_t step = (size_t)G * (size_t)a.ld;             // doubles from a row of this lane to its next
      const int n = (int)((v1 - v0 - g + G - 1) / G);            // rows of this lane (block < 2^31)
      const double* p = a.table + (size_t)(v0 + g) * (size_t)a.ld + (size_t)a.c0 + (size_t)c;
      int row = (int)(v0 + g);
      for (int i = 0; i < n; i += kFlight, row += kFlight * G) {   // kFlight rows in flight
        double x[kFlight];
        unsigned live = 0;   // bit u: row u of the flight exists and is not below the bound
#pragma unroll
        for (int u = 0; u < kFlight; ++u) x[u] = i + u < n ? p[(size_t)(i + u) * step] : low;
#pragma unroll
        for (int u = 0; u < kFlight; ++u) live |= (i + u < n && !(x[u] < low) ? 1u : 0u) << u;
        while (live) {   // the one place that offers: after the sampled bound few values get here
          const int u = __ffs(live) - 1;
          live &= live - 1;
          double xv = x[0];
#pragma unroll
          for (int k = 1; k < kFlight; ++k) xv = u == k ? x[k] : xv;
          offer(l, xv, row + u * G);
        }
      }
    }
    if (G > 1) tree_merge(l, cnt_lds, ok ? g : G, G, a.wb);
    if (ok && g == 0) {
      double* sd = a.scratch;
      int* si = reinterpret_cast<int*>(sd + (size_t)a.nblk * (size_t)N * (size_t)a.wb);
      for (int s = 0; s < N; ++s) {
        const size_t at = ((size_t)b * N + s) * (size_t)a.wb + (size_t)c;
        sd[at] = s < l.cnt ? l.ld[s * T] : neg_inf();
        si[at] = s < l.cnt ? l.lr[s * T] : -1;
      }
    }
  }
}

// Pass 2.  LAST: the lists of all `nin` blocks of `src` into the result.  Otherwise one level of a two-level
// merge: workgroup (tile, y) merges the blocks y * kTopicMergeGroup .. of `src` into list y of a.scratch2, which has
// the layout of the scratch with ceil(nin / kTopicMergeGroup) blocks.  grid: x strides over the tiles of columns.
template <bool LAST>
__global__ __launch_bounds__(256) void topn_merge_kernel(TopnArgs a, int G, int ntiles, const double* src, int nin) {
  extern __shared__ double2 topic_lds[];
  const int T = blockDim.x, N = a.N;
  int* cnt_lds = reinterpret_cast<int*>(reinterpret_cast<double*>(topic_lds) + (size_t)N * T) + (size_t)N * T;
  const size_t per = (size_t)N * (size_t)a.wb;   // cells of one block's lists
  const int* si = reinterpret_cast<const int*>(src + (size_t)nin * per);
  const int b0 = LAST ? 0 : (int)blockIdx.y * kTopicMergeGroup;
  const int b1 = LAST || b0 + kTopicMergeGroup > nin ? nin : b0 + kTopicMergeGroup;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    int g, c;
    const bool ok = lane_place(a, G, tile, g, c);
    TopList l = list_of(topic_lds, N);
    if (ok) {
      for (int b = b0 + g; b < b1; b += G) {
        for (int s = 0; s < N; ++s) {
          const size_t at = (size_t)b * per + (size_t)s * a.wb + (size_t)c;
          const int p = si[at];
          if (p < 0 || !offer(l, src[at], p)) break;
        }
      }
    }
    if (G > 1) tree_merge(l, cnt_lds, ok ? g : G, G, a.wb);
    if (ok && g == 0) {
      if (LAST) {
        const size_t o = ((size_t)a.c0 + (size_t)c) * N;
        for (int s = 0; s < N; ++s) {
          a.out_rows[o + s] = s < l.cnt ? l.lr[s * T] : -1;
          a.out_vals[o + s] = s < l.cnt ? l.ld[s * T] : neg_inf();
        }
        a.out_count[(size_t)a.c0 + c] = l.cnt;
      } else {
        double* dd = a.scratch2;
        int* di = reinterpret_cast<int*>(dd + (size_t)gridDim.y * per);
        for (int s = 0; s < N; ++s) {
          const size_t at = (size_t)blockIdx.y * per + (size_t)s * a.wb + (size_t)c;
          dd[at] = s < l.cnt ? l.ld[s * T] : neg_inf();
          di[at] = s < l.cnt ? l.lr[s * T] : -1;
        }
      }
    }
  }
}

// the first k attaining the maximum of row[0 .. K); a NaN never wins; -1: all NaN
__device__ __forceinline__ int first_max(const double* __restrict__ row, int K) {
  int best = -1;
  double bv = 0.0;
  for (int k = 0; k < K; ++k) {
    const double v = row[k];
    if (v == v && (best < 0 || v > bv)) {
      best = k;
      bv = v;
    }
  }
  return best;
}

__global__ __launch_bounds__(kDomThreads) void row_dominant_kernel(DominantArgs a) {
  extern __shared__ double2 topic_lds[];
  unsigned* hist = reinterpret_cast<unsigned*>(topic_lds);   // [R K]
  const int W = a.R * a.K;
  for (int j = threadIdx.x; j < W; j += kDomThreads) hist[j] = 0u;
  __syncthreads();
  const int64_t n = a.rows * a.R;
  for (int64_t i = (int64_t)blockIdx.x * kDomThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kDomThreads) {
    const int k = first_max(a.table + (size_t)i * a.K, a.K);
    a.arg[i] = k;
    if (k >= 0) atomicAdd(&hist[(int)(i % a.R) * a.K + k], 1u);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < W; j += kDomThreads)
    if (hist[j]) atomicAdd(a.counts + j, (unsigned long long)hist[j]);
}

__global__ __launch_bounds__(kDomThreads) void topic_sides_kernel(TopicSidesArgs a) {
#pragma clang fp contract(off)
  const int R = a.R, K = a.K;
  const size_t run = (size_t)R * K;
  const double rd = (double)R;
  for (int64_t i = (int64_t)blockIdx.x * kDomThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kDomThreads) {
    const int d = a.doc[i], w = a.word[i];
    int best = -1, ht = -1;
    double resp = quiet_nan(), share = quiet_nan();
    if (d >= 0 && w >= 0) {
      const double* tr = a.theta + (size_t)d * run;
      const double* pr = a.phi + (size_t)w * run;
      double bp = 0.0, sum = 0.0;
      for (int r = 0; r < R; ++r) {
        double s = 0.0;
        for (int k = 0; k < K; ++k) {
          const int j = r * K + k;
          const double p = tr[j] * pr[j];   // contract(off): rounded product, then rounded sum
          s = s + p;
          if (p == p && (best < 0 || p > bp)) {
            best = j;
            bp = p;
          }
        }
        sum = sum + s;
      }
      if (best >= 0) {
        const double sc = sum / rd;    // the side's score, score_ensemble.hip's operations
        const double den = sc * rd;    // exact at R = 1
        resp = bp / den;
        share = tr[best];
        ht = first_max(tr + (size_t)(best / K) * K, K);
      }
    }
    a.col[i] = best;
    a.resp[i] = resp;
    a.host_share[i] = share;
    a.host_topic[i] = ht;
  }
}

}  // namespace

int topic_threads(int N) { return N <= 16 ? 256 : 128; }

int topic_merge_groups(int64_t nblk) {
  return nblk > kTopicMergeGroup ? (int)((nblk + kTopicMergeGroup - 1) / kTopicMergeGroup) : 0;
}

int topic_groups(int N, int wb) {
  const int T = topic_threads(N);
  return wb >= 1 && wb <= T / 2 ? T / wb : 1;
}

void launch_column_topn(const TopnArgs& a, int max_blocks, hipStream_t s) {
  const std::string w("column_topn");
  // (a lane's row counter may step up to kFlight sub-groups past the last row before its loop ends)
  if (a.rows < 1 || a.rows > kTopicRowsMax) throw std::runtime_error(w + ": rows outside 1 .. 2^31 - 65536");
  if (a.W < 1 || a.ld < a.W) throw std::runtime_error(w + ": W < 1 or ld < W");
  if (a.c0 < 0 || a.wb < 1 || (int64_t)a.c0 + a.wb > a.W) throw std::runtime_error(w + ": columns outside the table");
  if (a.N < 1 || a.N > kTopicReportMax)
    throw std::runtime_error(w + ": N outside 1 .. " + std::to_string(kTopicReportMax));
  if (a.block < 1 || a.block >= ((int64_t)1 << 31)) throw std::runtime_error(w + ": block outside 1 .. 2^31 - 1");
  if (a.nblk != (a.rows + a.block - 1) / a.block) throw std::runtime_error(w + ": nblk is not ceil(rows / block)");
  if (max_blocks < 0) throw std::runtime_error(w + ": max_blocks < 0");
  if (!a.table || !a.scratch || !a.out_rows || !a.out_vals || !a.out_count)
    throw std::runtime_error(w + ": null buffer");
  if ((uintptr_t)a.scratch % 8 != 0) throw std::runtime_error(w + ": scratch is not 8-byte aligned");
  const int T = topic_threads(a.N);
  const int G = topic_groups(a.N, a.wb);
  const int64_t cap = max_blocks > 0 ? max_blocks : 65536;
  const int64_t ntiles = G > 1 ? 1 : ((int64_t)a.wb + T - 1) / T;
  // the lists, then the lanes' counts for the tree (16-byte multiple: N T 12 is one)
  const size_t lds = (size_t)a.N * T * (sizeof(double) + sizeof(int)) + (size_t)T * sizeof(int);
  if (a.nblk > ((int64_t)1 << 30) || ntiles > 65535)
    throw std::runtime_error(w + ": more than 2^30 blocks of rows or 65535 tiles of columns");
  int64_t blocks = cap / ntiles > 0 ? cap / ntiles : 1;   // per tile of columns: at least one workgroup
  if (blocks > a.nblk) blocks = a.nblk;
  hipLaunchKernelGGL(topn_blocks_kernel, dim3((unsigned)blocks, (unsigned)ntiles), dim3(T), lds, s, a, G);
  ONI_HIP_CHECK(hipGetLastError());
  blocks = ntiles < cap ? ntiles : cap;
  const double* src = a.scratch;
  int nin = (int)a.nblk;
  if (nin > kTopicMergeGroup) {   // two levels: groups of blocks side by side, then the groups' lists
    if (!a.scratch2 || (uintptr_t)a.scratch2 % 8 != 0) throw std::runtime_error(w + ": scratch2 missing or unaligned");
    const int groups = topic_merge_groups(a.nblk);
    if (groups > 65535) throw std::runtime_error(w + ": more than 65535 groups of blocks");
    const int64_t bx = cap / groups > 0 ? (cap / groups < ntiles ? cap / groups : ntiles) : 1;
    hipLaunchKernelGGL((topn_merge_kernel<false>), dim3((unsigned)bx, (unsigned)groups), dim3(T), lds, s, a, G,
                       (int)ntiles, src, nin);
    ONI_HIP_CHECK(hipGetLastError());
    src = a.scratch2;
    nin = groups;
  }
  hipLaunchKernelGGL((topn_merge_kernel<true>), dim3((unsigned)blocks), dim3(T), lds, s, a, G, (int)ntiles, src, nin);
  ONI_HIP_CHECK(hipGetLastError());
}

void launch_row_dominant(const DominantArgs& a, int max_blocks, hipStream_t s) {
  const std::string w("row_dominant");
  if (a.rows < 0 || a.R < 1 || a.K < 1) throw std::runtime_error(w + ": rows < 0, R < 1 or K < 1");
  if ((int64_t)a.R * a.K > kTopicColumnsMax)
    throw std::runtime_error(w + ": R K above " + std::to_string(kTopicColumnsMax));
  if (a.rows * a.R >= ((int64_t)1 << 31)) throw std::runtime_error(w + ": rows R outside 0 .. 2^31 - 1");
  if (max_blocks < 0) throw std::runtime_error(w + ": max_blocks < 0");
  if (a.rows == 0) return;
  if (!a.table || !a.arg || !a.counts) throw std::runtime_error(w + ": null buffer");
  const int64_t n = a.rows * a.R;
  const int64_t cap = max_blocks > 0 ? max_blocks : 2048;
  int64_t blocks = (n + kDomThreads - 1) / kDomThreads;
  if (blocks > cap) blocks = cap;
  const size_t lds = (((size_t)a.R * a.K * sizeof(unsigned)) + 15) / 16 * 16;
  hipLaunchKernelGGL(row_dominant_kernel, dim3((unsigned)blocks), dim3(kDomThreads), lds, s, a);
  ONI_HIP_CHECK(hipGetLastError());
}

void launch_topic_sides(const TopicSidesArgs& a, int max_blocks, hipStream_t s) {
  const std::string w("topic_sides");
  if (a.n < 0 || a.n >= ((int64_t)1 << 31)) throw std::runtime_error(w + ": n outside 0 .. 2^31 - 1");
  if (a.R < 1 || a.K < 1 || (int64_t)a.R * a.K >= ((int64_t)1 << 31))
    throw std::runtime_error(w + ": R < 1, K < 1 or R K >= 2^31");
  if (max_blocks < 0) throw std::runtime_error(w + ": max_blocks < 0");
  if (a.n == 0) return;
  if (!a.theta || !a.phi || !a.doc || !a.word || !a.col || !a.resp || !a.host_share || !a.host_topic)
    throw std::runtime_error(w + ": null buffer");
  const int64_t cap = max_blocks > 0 ? max_blocks : 8192;
  int64_t blocks = (a.n + kDomThreads - 1) / kDomThreads;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(topic_sides_kernel, dim3((unsigned)blocks), dim3(kDomThreads), 0, s, a);
  ONI_HIP_CHECK(hipGetLastError());
}

}  // namespace oni
