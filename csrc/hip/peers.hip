// --peers: for each query host the N nearest of all D hosts in topic space (pipeline/common.py write_peers; twin:
// ops/reference.py peer_topn).
//
// A row of theta is W = R K doubles (an ensemble's members interleaved as the scorers hold them).  L(q, p) is the
// L1 distance of rows q and p: from 0.0, for j = 0 .. W - 1 in order, t = theta[q][j] - theta[p][j] (one rounded
// subtraction) and acc = acc + |t| (one rounded add).  The peers of q are the N candidates p != q lowest in the
// total order (L, p) ascending, in that order; a NaN L never enters.  The top N of a set under a total order does
// not depend on how the set is cut or in which order the pieces are merged, so no block order is part of the
// result: the same bits for every grid, block size and batch, and no atomics.
//
// The arithmetic is fp64 VALU, a subtraction and an add of a magnitude per element: no multiply, so nothing can
// contract (contraction is off all the same).  What the kernel saves is theta traffic and the Q x D matrix: a
// block's candidate rows are staged in LDS once per workgroup and every lane reads the same LDS address (a
// broadcast read), so a row comes from HBM or L2 once per tile of 256 queries instead of once per query.
//
// Pass 1, item = (tile of 256 queries, block of candidate rows), grid-stride; a lane owns one query and walks the
// block's rows in order.  Two forms by row width:
//   registers  W <= 100: the query's row in registers, padded to TK, the next of tail::kLadder >= W; the staged
//              rows carry the same padding, 0.0 on both sides (tail::stage_rows with the row as one member of W
//              topics).  A padding step adds |0 - 0| = +0.0 to a sum that is never -0.0: no bit changes, and the
//              inner loop has a compile-time bound and no branch.  Two rows in flight up to TK = 50.
//   direct     anything wider: both rows from global memory (the candidate's address is the same in every lane).
// A lane keeps its list -- N (L, row) pairs ascending -- in an LDS slice of its own, [slot][lane], so a slot is one
// conflict-free 8-byte access per lane; at N = 16 the slices are 48 KiB beside 15 KiB of staged rows.  Candidates
// arrive in ascending row order, so one that ties with the list's last entry loses and an equal L stays behind the
// entries already there: the order (L, p) without comparing rows.  The block's list goes to scratch[b][slot][query].
// Pass 2, one lane per query, offers its blocks' lists in block order -- ascending rows again -- to the same list.
#include <stdexcept>
#include <string>

#include "common.h"
#include "kernels.h"
#include "tail_common.h"

namespace oni {

namespace {

using namespace tail;   // kThreads, stage_rows, kLadder, reg_topics: shared with tail_mass.hip

constexpr int kStage = 1920;   // doubles of staged candidate rows (15 KiB; 63 KiB with the lists at N = 16)

__device__ __forceinline__ double inf() { return __longlong_as_double(0x7ff0000000000000LL); }

// the candidate (L, p) to a lane's list (ld, lr: its slot 0; slots kThreads apart), p above every row offered to
// it before.  false: it did not enter.  At most N - 1 shifts.
__device__ __forceinline__ bool offer(double* ld, int* lr, int N, int& cnt, double& worst, double L, int p) {
  if (!(L < worst || (cnt < N && L == L))) return false;   // worst: +inf until the list is full; NaN never enters
  int s = cnt < N ? cnt : N - 1;   // the slot that opens: the end of a short list, else the last entry drops out
  while (s > 0 && ld[(s - 1) * kThreads] > L) {   // an equal L stays ahead: it has the lower row
    ld[s * kThreads] = ld[(s - 1) * kThreads];
    lr[s * kThreads] = lr[(s - 1) * kThreads];
    --s;
  }
  ld[s * kThreads] = L;
  lr[s * kThreads] = p;
  if (cnt < N) ++cnt;
  if (cnt == N) worst = ld[(N - 1) * kThreads];
  return true;
}

// L of the lane's padded row th and the padded candidate row p in LDS
template <int TK>
__device__ __forceinline__ double dist_pad(const double (&th)[TK], const double2* __restrict__ p) {
#pragma clang fp contract(off)
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < TK; k += 2) {
    const double2 c = p[k / 2];
    const double t0 = th[k] - c.x;   // rounded difference, then rounded sum
    acc = acc + __builtin_fabs(t0);
    const double t1 = th[k + 1] - c.y;
    acc = acc + __builtin_fabs(t1);
  }
  return acc;
}

// a lane's list of block b into its scratch cell
__device__ __forceinline__ void put(const PeerArgs& a, int64_t b, int64_t i, const double* ld, const int* lr,
                                    int cnt) {
  const size_t cells = (size_t)a.nblk * (size_t)a.N * (size_t)a.n;
  double* sd = a.scratch;
  int* si = reinterpret_cast<int*>(sd + cells);
  for (int s = 0; s < a.N; ++s) {
    const size_t at = ((size_t)b * a.N + s) * (size_t)a.n + (size_t)i;
    sd[at] = s < cnt ? ld[s * kThreads] : inf();
    si[at] = s < cnt ? lr[s * kThreads] : -1;
  }
}

// registers: the query's row padded in registers, candidate sub-tiles padded in LDS
template <int TK>
__global__ __launch_bounds__(kThreads) void peer_blocks_reg_kernel(PeerArgs a, int64_t ntiles, int vec) {
  extern __shared__ double2 peer_lds[];
  double* st = reinterpret_cast<double*>(peer_lds);   // [kStage]
  double* ld = st + kStage + threadIdx.x;             // [N][kThreads]
  int* lr = reinterpret_cast<int*>(st + kStage + a.N * kThreads) + threadIdx.x;
  const int W = a.W, N = a.N;
  constexpr int sub = kStage / TK;
  const int64_t items = ntiles * a.nblk;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t b = item / ntiles, i = (item % ntiles) * kThreads + threadIdx.x;
    const bool ok = i < a.n;
    const int q = ok ? a.query[i] : -1;
    double th[TK];
#pragma unroll
    for (int k = 0; k < TK; ++k) th[k] = ok && k < W ? a.theta[(size_t)q * W + k] : 0.0;
    int cnt = 0;
    double worst = inf();
    const int64_t v0 = b * a.block, v1 = v0 + a.block < a.D ? v0 + a.block : a.D;
    for (int64_t r0 = v0; r0 < v1; r0 += sub) {
      const int nr = (int)(v1 - r0 < sub ? v1 - r0 : sub);
      __syncthreads();   // the lanes are done with the previous sub-tile
      stage_rows(st, TK, a.theta, r0, nr, 1, W, TK, vec);
      __syncthreads();
      if (ok) {
        const double2* rows = reinterpret_cast<const double2*>(st);
        int row = 0;
        if (TK <= 50) {   // two rows in flight where the registers allow it
          for (; row + 1 < nr; row += 2) {
            const double L0 = dist_pad<TK>(th, rows + row * (TK / 2));
            const double L1 = dist_pad<TK>(th, rows + (row + 1) * (TK / 2));
            const int p = (int)(r0 + row);
            if (p != q) offer(ld, lr, N, cnt, worst, L0, p);
            if (p + 1 != q) offer(ld, lr, N, cnt, worst, L1, p + 1);
          }
        }
#pragma unroll 1
        for (; row < nr; ++row) {
          const double L = dist_pad<TK>(th, rows + row * (TK / 2));
          const int p = (int)(r0 + row);
          if (p != q) offer(ld, lr, N, cnt, worst, L, p);
        }
      }
    }
    if (ok) put(a, b, i, ld, lr, cnt);
  }
}

// direct: any row width, both rows from global memory
__global__ __launch_bounds__(kThreads) void peer_blocks_direct_kernel(PeerArgs a, int64_t ntiles) {
#pragma clang fp contract(off)
  extern __shared__ double2 peer_lds[];
  double* ld = reinterpret_cast<double*>(peer_lds) + threadIdx.x;
  int* lr = reinterpret_cast<int*>(reinterpret_cast<double*>(peer_lds) + a.N * kThreads) + threadIdx.x;
  const int W = a.W, N = a.N;
  const int64_t items = ntiles * a.nblk;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t b = item / ntiles, i = (item % ntiles) * kThreads + threadIdx.x;
    if (i >= a.n) continue;
    const int q = a.query[i];
    const double* tq = a.theta + (size_t)q * W;
    int cnt = 0;
    double worst = inf();
    const int64_t v0 = b * a.block, v1 = v0 + a.block < a.D ? v0 + a.block : a.D;
    for (int64_t v = v0; v < v1; ++v) {
      if (v == q) continue;
      const double* tp = a.theta + (size_t)v * W;
      double acc = 0.0;
#pragma unroll 4
      for (int j = 0; j < W; ++j) {
        const double t = tq[j] - tp[j];
        acc = acc + __builtin_fabs(t);
      }
      offer(ld, lr, N, cnt, worst, acc, (int)v);
    }
    put(a, b, i, ld, lr, cnt);
  }
}

// pass 2: one lane per query offers its blocks' lists in block order
__global__ __launch_bounds__(kThreads) void peer_merge_kernel(PeerArgs a) {
  extern __shared__ double2 peer_lds[];
  double* ld = reinterpret_cast<double*>(peer_lds) + threadIdx.x;
  int* lr = reinterpret_cast<int*>(reinterpret_cast<double*>(peer_lds) + a.N * kThreads) + threadIdx.x;
  const int N = a.N;
  const size_t cells = (size_t)a.nblk * (size_t)N * (size_t)a.n;
  const double* sd = a.scratch;
  const int* si = reinterpret_cast<const int*>(sd + cells);
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kThreads) {
    int cnt = 0;
    double worst = inf();
    for (int64_t b = 0; b < a.nblk; ++b) {
      for (int s = 0; s < N; ++s) {
        const size_t at = ((size_t)b * N + s) * (size_t)a.n + (size_t)i;
        const int p = si[at];
        // a block's list ascends: past its end, or past the first entry that does not enter, nothing enters
        if (p < 0 || !offer(ld, lr, N, cnt, worst, sd[at], p)) break;
      }
    }
    for (int s = 0; s < N; ++s) {
      a.rows[(size_t)i * N + s] = s < cnt ? lr[s * kThreads] : -1;
      a.dist[(size_t)i * N + s] = s < cnt ? ld[s * kThreads] : inf();
    }
    a.count[i] = cnt;
  }
}

template <int TK>
void launch_reg(const PeerArgs& a, int64_t ntiles, int vec, unsigned blocks, size_t lists, hipStream_t s) {
  hipLaunchKernelGGL((peer_blocks_reg_kernel<TK>), dim3(blocks), dim3(kThreads), kStage * sizeof(double) + lists, s,
                     a, ntiles, vec);
}

}  // namespace

int peer_theta_path(int R, int K) {
  if (R < 1 || K < 1 || R > kEnsembleMax) throw std::runtime_error("peer_theta_path: R or K out of range");
  // the distance runs over the row as one stretch of R K doubles: the ladder takes it as one member of R K topics
  return (int64_t)R * K <= kRegMax && reg_topics(1, R * K) ? kPeerRegisters : kPeerDirect;
}

void launch_peer_topn(const PeerArgs& a, int max_blocks, hipStream_t s) {
  const std::string w("peer_topn");
  if (a.n < 0 || a.n >= ((int64_t)1 << 31) || a.D < 0 || a.D >= ((int64_t)1 << 31))
    throw std::runtime_error(w + ": n or D outside 0 .. 2^31 - 1");
  if (a.W < 1) throw std::runtime_error(w + ": W < 1");
  if (a.N < 1 || a.N > kPeersMax) throw std::runtime_error(w + ": N outside 1 .. " + std::to_string(kPeersMax));
  if (a.block < 1 || a.block >= ((int64_t)1 << 31)) throw std::runtime_error(w + ": block outside 1 .. 2^31 - 1");
  if (a.nblk != (a.D + a.block - 1) / a.block) throw std::runtime_error(w + ": nblk is not ceil(D / block)");
  if (max_blocks < 0) throw std::runtime_error(w + ": max_blocks < 0");
  if (a.n == 0) return;
  if (a.D == 0) throw std::runtime_error(w + ": queries of an empty table");
  if (!a.theta || !a.query || !a.scratch || !a.rows || !a.dist || !a.count)
    throw std::runtime_error(w + ": null buffer");
  if ((uintptr_t)a.scratch % 8 != 0) throw std::runtime_error(w + ": scratch is not 8-byte aligned");
  const int64_t cap = max_blocks > 0 ? max_blocks : 65536;
  const size_t lists = (size_t)a.N * kThreads * (sizeof(double) + sizeof(int));
  const int64_t ntiles = (a.n + kThreads - 1) / kThreads;
  int64_t blocks = ntiles * a.nblk;
  if (blocks > cap) blocks = cap;
  const int tk = a.W <= kRegMax ? reg_topics(1, a.W) : 0;
  if (tk) {
    const int vec = a.W % 2 == 0 && (uintptr_t)a.theta % 16 == 0;
    switch (tk) {
      case 4: launch_reg<4>(a, ntiles, vec, (unsigned)blocks, lists, s); break;
      case 8: launch_reg<8>(a, ntiles, vec, (unsigned)blocks, lists, s); break;
      case 20: launch_reg<20>(a, ntiles, vec, (unsigned)blocks, lists, s); break;
      case 32: launch_reg<32>(a, ntiles, vec, (unsigned)blocks, lists, s); break;
      case 50: launch_reg<50>(a, ntiles, vec, (unsigned)blocks, lists, s); break;
      default: launch_reg<100>(a, ntiles, vec, (unsigned)blocks, lists, s); break;
    }
  } else {
    hipLaunchKernelGGL(peer_blocks_direct_kernel, dim3((unsigned)blocks), dim3(kThreads), lists, s, a, ntiles);
  }
  ONI_HIP_CHECK(hipGetLastError());
  blocks = ntiles < cap ? ntiles : cap;
  hipLaunchKernelGGL(peer_merge_kernel, dim3((unsigned)blocks), dim3(kThreads), lists, s, a);
  ONI_HIP_CHECK(hipGetLastError());
}

}  // namespace oni
