// --tail-tol: the tail sums of every distinct (document, word) pair of a day, the pairs sorted by document
// (pipeline/common.py tail_keys through score/scorer.py tail_pairs; the bits are tail_mass.hip's, twin:
// ops/reference.py tail_mass).
//
// tail_mass.hip evaluates p(.|d) once per side: right for the written sides, which almost never share a document.
// The pairs of a whole day lie many to a document -- 10 on the 1 M-event flow day, 15,622 in the longest -- so here
// p_v is evaluated once per (document of a tile, row) and the tile's pairs select-add it from LDS.  The definition
// is unchanged -- p_v by dot_pad over the same padded rows, take() in row order from 0.0 within a vocabulary block,
// the block partials to the same scratch cells, tail_mass.hip's fold pass over them -- so the bits are the same.
//
// Pass 1, item = (tile of 256 consecutive pairs, vocabulary block), grid-stride.  Per item:
//   slots    head flag doc[i] != doc[i - 1] (the tile's first lane is a head), a prefix count over the tile (ballot
//            and popcount per wave, the waves' counts through LDS): a lane's slot is the number of heads before it,
//            slot_doc[slot] its document.  S slots, padded to SP, a power of two in 1 .. 256.
//   s        p_w of the lane's pair, by dot_any from global memory exactly as tail_mass.hip computes it.
//   per sub-tile of `sub` rows, two phases, a barrier between them and one after:
//   phase A  thread t works for slot t % SP on the rows t / SP, t / SP + G, ... (G = 256 / SP row groups): the
//            slot's theta row padded in registers (the ladder of tail_mass.hip), the phi rows from the staged
//            sub-tile, p to LDS as P[row][slot].  Lanes of one row group read one phi address (a broadcast);
//            the rows lie an odd number of 16-byte slots apart, so the 16 lanes of a b128 read that walk 16 rows
//            (SP = 1, inside a long document) fall in 16 different slots.  Consecutive threads store consecutive
//            doubles of P.
//   phase B  a lane owns its pair and walks P[.][slot] in row order with take(): lanes of one document read one
//            address, different documents consecutive doubles.  While the lanes are in phase B the next sub-tile's
//            phi rows are staged (phase A is behind a barrier, nobody reads the old rows).
// LDS: one pool of 8,192 doubles (64 KiB) for the phi sub-tile and the P sub-tile, sub = pool / (row stride + SP)
// rows, rounded down to whole row groups; with slot_doc and the wave counts 65.0 KiB, two workgroups per CU of
// 160 KiB.  At K = 20, one model: 356 -> 256 rows at SP = 1, 151 -> 144 at SP = 32, 29 at SP = 256.
//
// Registers (compiler's report for gfx950, 256 threads; no scratch and no VGPR spill at any width; every form two
// waves per SIMD, which is what 65 KiB of LDS per workgroup allows): one model, TK = 4: 63 VGPRs, 8: 79, 20: 101,
// 32: 126, 50: 162, 100: 256; TM = 25 x 4, 12 x 8, 5 x 20, 3 x 32, 2 x 50 members: 248, 243, 253, 244, 250.  The
// pair's partial sums and s stay in registers through phase A: 9 to 18 more than tail_mass.hip's forms, and the
// TK = 100 form sits at the 256 that two waves per SIMD leave.
//
// The kernel covers the widths of the register ladder; launch_tail_docs refuses any other.
#include <stdexcept>
#include <string>

#include "common.h"
#include "kernels.h"
#include "tail_common.h"

namespace oni {

namespace {

using namespace tail;

constexpr int kPool = 8192;   // doubles of the phi sub-tile and the P sub-tile together (64 KiB)

template <int TK, int TM>
__global__ __launch_bounds__(kThreads) void tail_docs_kernel(TailArgs a, int64_t ntiles, int vec) {
  __shared__ double2 pool[kPool / 2];
  __shared__ int slot_doc[kThreads];
  __shared__ int wave_heads[kThreads / 64];
  constexpr int W = TK * TM;   // doubles of a padded theta row
  const int K = a.K, R = a.R, RK = a.R * a.K;
  const int stride2 = (R * TK / 2) | 1;   // double2 of a staged row: an odd number of 16-byte slots
  const int stride = 2 * stride2;
  const double rd = (double)R;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t items = ntiles * a.nblk;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t b = item / ntiles, i = (item % ntiles) * kThreads + threadIdx.x;
    const bool ok = i < a.n;
    const int d = ok ? a.doc[i] : -1, w = ok ? a.word[i] : -1;
    const bool head = ok && (threadIdx.x == 0 || a.doc[i - 1] != d);   // (i - 1 is in the tile: threadIdx.x > 0)
    const unsigned long long heads = __ballot(head);
    __syncthreads();   // the lanes are done with the previous item's slots and sub-tiles
    if (lane == 0) wave_heads[wv] = __popcll(heads);
    __syncthreads();
    int before = 0, S = 0;
#pragma unroll
    for (int k = 0; k < kThreads / 64; ++k) {
      before += k < wv ? wave_heads[k] : 0;
      S += wave_heads[k];
    }
    // heads at or below this lane, this lane's wave; at lane 63 the mask is every bit
    const int slot = before + __popcll(heads & (lane == 63 ? ~0ull : (2ull << lane) - 1)) - 1;
    if (head) slot_doc[slot] = d;
    int lg = 0;   // SP = 2^lg >= S
    while ((1 << lg) < S) ++lg;
    const int SP = 1 << lg, G = kThreads >> lg;
    int sub = kPool / (stride + SP);   // >= 22: stride <= 102, SP <= 256
    if (sub >= G) sub -= sub % G;      // whole row groups: every thread of phase A the same trips
    double* ph_l = reinterpret_cast<double*>(pool);
    double* P = ph_l + sub * stride;
    __syncthreads();   // slot_doc is complete
    const int slot_a = threadIdx.x & (SP - 1), rg = threadIdx.x >> lg;
    const bool act = slot_a < S;
    const int d_a = act ? slot_doc[slot_a] : 0;
    double th[W];
#pragma unroll
    for (int m = 0; m < TM; ++m)
#pragma unroll
      for (int k = 0; k < TK; ++k) th[m * TK + k] = act && m < R && k < K ? a.theta[(size_t)d_a * RK + m * K + k] : 0.0;
    const double s = ok ? dot_any(a.theta + (size_t)d * RK, 1, a.phi + (size_t)w * RK, R, K, rd) : 0.0;
    Part pt{0.0, 0.0, 0, 0};
    const int64_t v0 = b * a.block, v1 = v0 + a.block < a.V ? v0 + a.block : a.V;
    stage_rows(ph_l, stride, a.phi, v0, (int)(v1 - v0 < sub ? v1 - v0 : sub), R, K, TK, vec);
    for (int64_t r0 = v0; r0 < v1; r0 += sub) {
      const int nr = (int)(v1 - r0 < sub ? v1 - r0 : sub);
      __syncthreads();   // the phi rows are staged, and the lanes are done with the previous sub-tile's P
      if (act) {         // phase A: p once per (slot, row)
        if (W <= 50) {   // two rows in flight where the registers allow it
#pragma unroll 2
          for (int row = rg; row < nr; row += G)
            P[(row << lg) + slot_a] = dot_pad<TK, TM>(th, pool + row * stride2, R, rd);
        } else {
#pragma unroll 1
          for (int row = rg; row < nr; row += G)
            P[(row << lg) + slot_a] = dot_pad<TK, TM>(th, pool + row * stride2, R, rd);
        }
      }
      __syncthreads();   // P is complete, and nobody reads these phi rows again
      if (ok) {          // phase B: the pair's select-adds in row order
#pragma unroll 4
        for (int row = 0; row < nr; ++row) take(pt, P[(row << lg) + slot], s);
      }
      const int64_t n0 = r0 + sub;
      if (n0 < v1) stage_rows(ph_l, stride, a.phi, n0, (int)(v1 - n0 < sub ? v1 - n0 : sub), R, K, TK, vec);
    }
    if (ok) put(a, b, i, pt);
  }
}

template <int TK>
void launch_docs(const TailArgs& a, int64_t ntiles, int vec, unsigned blocks, hipStream_t s) {
  constexpr int TM = kRegMax / TK;
  if (a.R == 1)
    hipLaunchKernelGGL((tail_docs_kernel<TK, 1>), dim3(blocks), dim3(kThreads), 0, s, a, ntiles, vec);
  else
    hipLaunchKernelGGL((tail_docs_kernel<TK, TM>), dim3(blocks), dim3(kThreads), 0, s, a, ntiles, vec);
}

}  // namespace

void launch_tail_docs(const TailArgs& a, int max_blocks, hipStream_t s) {
  const bool any = tail_args_check(a, max_blocks, "tail_mass_docs");
  if (a.R >= 1 && a.K >= 1 && !reg_topics(a.R, a.K))
    throw std::runtime_error("tail_mass_docs: a row of " + std::to_string(a.R) + " x " + std::to_string(a.K) +
                             " is wider than the register ladder (tail_mass takes it)");
  if (!any) return;
  const int64_t cap = max_blocks > 0 ? max_blocks : 65536;
  if (a.nblk > 0) {
    const int64_t ntiles = (a.n + kThreads - 1) / kThreads;
    int64_t blocks = ntiles * a.nblk;
    if (blocks > cap) blocks = cap;
    const int vec = a.K % 2 == 0 && (uintptr_t)a.phi % 16 == 0;
    switch (reg_topics(a.R, a.K)) {
      case 4: launch_docs<4>(a, ntiles, vec, (unsigned)blocks, s); break;
      case 8: launch_docs<8>(a, ntiles, vec, (unsigned)blocks, s); break;
      case 20: launch_docs<20>(a, ntiles, vec, (unsigned)blocks, s); break;
      case 32: launch_docs<32>(a, ntiles, vec, (unsigned)blocks, s); break;
      case 50: launch_docs<50>(a, ntiles, vec, (unsigned)blocks, s); break;
      default: launch_docs<100>(a, ntiles, vec, (unsigned)blocks, s); break;
    }
    ONI_HIP_CHECK(hipGetLastError());
  }
  launch_tail_fold(a, cap, s);
}

}  // namespace oni
