// Device side of the fp64 engine's construction (models/lda/em.py, the native plan path):
//   * csc_docs: the int32 CSC entry list from the sort's permutation and every slot's document (a binary
//     search of the entry in doc_ptr);
//   * csc_partition: the early / late split of the CSC in one pass -- flag (the slot's document is in the late
//     bucket) -> exclusive scan -> scatter, slot order kept: the two entry lists, their word pointers (the scan
//     value at word_ptr[w]) and, for the deferred final pass, et_row of every late slot from three
//     per-document tables (first entry, chunk width, first row), no search.
// The scan is three launches (per-tile counts, one workgroup over the tile counts, scatter): integer sums,
// no atomics, no waits between workgroups, any grid size.  Every index is checked against its array.
#include <stdexcept>

#include "common.h"
#include "kernels.h"

namespace oni {

namespace {
constexpr int kPT = 256;              // threads per workgroup
constexpr int kPI = 8;                // consecutive slots per thread
constexpr int kTile = kPT * kPI;      // slots per workgroup (kCscPartTile)
static_assert(kTile == kCscPartTile, "tile size of csc_partition");

__device__ __forceinline__ int late_flag(const CscPartArgs& a, long long s) {
  if (s >= a.nnz) return 0;
  const int d = a.csc_doc[s];
  return ((unsigned)d < (unsigned)a.D && a.late[d]) ? 1 : 0;
}

// exclusive prefix of v over the workgroup's threads (sh: kPT ints); total: the workgroup's sum
__device__ __forceinline__ int block_excl_scan(int v, int* sh, int& total) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int off = 1; off < kPT; off <<= 1) {
    const int x = t >= off ? sh[t - off] : 0;
    __syncthreads();
    sh[t] += x;
    __syncthreads();
  }
  total = sh[kPT - 1];
  const int incl = sh[t];
  __syncthreads();
  return incl - v;
}
}  // namespace

__global__ __launch_bounds__(kPT) void csc_docs_kernel(const long long* __restrict__ perm,
                                                       const int* __restrict__ doc_ptr, int D, int nnz,
                                                       int* __restrict__ csc_ent, int* __restrict__ csc_doc) {
  const long long s = (long long)blockIdx.x * kPT + threadIdx.x;
  if (s >= nnz) return;
  long long e = perm[s];
  if (e < 0 || e >= nnz) e = 0;           // (a permutation of 0 .. nnz - 1 never takes this)
  // the document d with doc_ptr[d] <= e < doc_ptr[d + 1]: first index in [1, D] whose doc_ptr exceeds e
  int lo = 1, hi = D;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (doc_ptr[mid] > (int)e)
      hi = mid;
    else
      lo = mid + 1;
  }
  csc_ent[s] = (int)e;
  csc_doc[s] = lo - 1;
}

__global__ __launch_bounds__(kPT) void csc_part_count_kernel(CscPartArgs a) {
  __shared__ int sh[kPT];
  const long long s0 = (long long)blockIdx.x * kTile + (long long)threadIdx.x * kPI;
  int c = 0;
#pragma unroll
  for (int j = 0; j < kPI; ++j) c += late_flag(a, s0 + j);
  int total;
  block_excl_scan(c, sh, total);
  if (threadIdx.x == 0) a.tile_sum[blockIdx.x] = total;
}

// one workgroup: tile_sum[b] <- late slots ahead of tile b; before[nnz] <- all late slots
__global__ __launch_bounds__(kPT) void csc_part_scan_kernel(CscPartArgs a, int n_tiles) {
  __shared__ int sh[kPT];
  int carry = 0;
  for (int base = 0; base < n_tiles; base += kPT) {
    const int i = base + threadIdx.x;
    const int v = i < n_tiles ? a.tile_sum[i] : 0;
    int total;
    const int ex = block_excl_scan(v, sh, total);
    if (i < n_tiles) a.tile_sum[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) a.before[a.nnz] = carry;
}

__global__ __launch_bounds__(kPT) void csc_part_scatter_kernel(CscPartArgs a) {
  __shared__ int sh[kPT];
  const long long s0 = (long long)blockIdx.x * kTile + (long long)threadIdx.x * kPI;
  int f[kPI], c = 0;
#pragma unroll
  for (int j = 0; j < kPI; ++j) {
    f[j] = late_flag(a, s0 + j);
    c += f[j];
  }
  int total;
  int lb = a.tile_sum[blockIdx.x] + block_excl_scan(c, sh, total);   // late slots ahead of slot s0
#pragma unroll
  for (int j = 0; j < kPI; ++j) {
    const long long s = s0 + j;
    if (s >= a.nnz) break;
    a.before[s] = lb;
    const int e = a.csc_ent[s];
    if (f[j]) {
      if (lb < a.n_late) {
        a.ce_late[lb] = e;
        if (a.et_row != nullptr) {
          const int d = a.csc_doc[s];          // in range: late_flag checked it
          const int w = max(a.et_w[d], 1), base = a.et_base[d];
          const int chunk = min(max((e - a.et_s0[d]) / w, 0), a.umax - 1);
          a.et_row[lb] = base < 0 ? 0 : base + chunk;
        }
      }
      ++lb;
    } else {
      const long long eb = s - lb;             // early slots ahead of slot s
      if (eb < a.n_early) a.ce_early[eb] = e;
    }
  }
}

__global__ __launch_bounds__(kPT) void csc_part_wptr_kernel(CscPartArgs a) {
  const int w = blockIdx.x * kPT + threadIdx.x;
  if (w > a.V) return;
  const int p = min(max(a.word_ptr[w], 0), a.nnz);
  const int l = a.before[p];
  a.wp_late[w] = l;
  a.wp_early[w] = p - l;
}

void launch_csc_docs(const long long* perm, const int* doc_ptr, int D, int nnz, int* csc_ent, int* csc_doc,
                     hipStream_t s) {
  if (nnz <= 0) return;
  if (D < 1) throw std::runtime_error("csc_docs: entries but no document");
  hipLaunchKernelGGL(csc_docs_kernel, dim3((unsigned)((nnz + kPT - 1) / kPT)), dim3(kPT), 0, s, perm, doc_ptr, D, nnz,
                     csc_ent, csc_doc);
  ONI_HIP_CHECK(hipGetLastError());
}

void launch_csc_partition(const CscPartArgs& a, hipStream_t s) {
  if (a.nnz < 0 || a.V < 0 || a.D < 0 || a.n_early < 0 || a.n_late < 0 || (long long)a.n_early + a.n_late != a.nnz)
    throw std::runtime_error("csc_partition: n_early + n_late must equal nnz");
  if ((a.et_row != nullptr) && (a.umax < 1 || !a.et_s0 || !a.et_w || !a.et_base))
    throw std::runtime_error("csc_partition: et_row needs the three per-document tables");
  const int n_tiles = (int)(((long long)a.nnz + kTile - 1) / kTile);
  if (n_tiles > 0) {
    hipLaunchKernelGGL(csc_part_count_kernel, dim3(n_tiles), dim3(kPT), 0, s, a);
    ONI_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(csc_part_scan_kernel, dim3(1), dim3(kPT), 0, s, a, n_tiles);
  ONI_HIP_CHECK(hipGetLastError());
  if (n_tiles > 0) {
    hipLaunchKernelGGL(csc_part_scatter_kernel, dim3(n_tiles), dim3(kPT), 0, s, a);
    ONI_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(csc_part_wptr_kernel, dim3((unsigned)(a.V / kPT + 1)), dim3(kPT), 0, s, a);
  ONI_HIP_CHECK(hipGetLastError());
}

}  // namespace oni
