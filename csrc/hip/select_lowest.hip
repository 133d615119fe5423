// MAXRESULTS: the `limit` flagged rows a stable ascending sort of the keys would put first, found without
// sorting or compacting the flagged rows (oni_ml_amd/score/scorer.py rank_flagged(key, flag, limit)).
//
// Order of the keys: ops/sortgroup.py f64_order_keys as an unsigned 64-bit integer (IEEE bits, negatives
// with every bit flipped, the others with the sign bit set: -0.0 sits just below +0.0).  Ties at the cut go
// to the lowest row index.  Unflagged rows (every NaN of the scorer among them) are never looked at.
//
// A most-significant-digit radix select: six histogram passes over the rows (digits of 11, 11, 11, 11, 11
// and 9 bits), each a per-workgroup LDS histogram of the flagged rows whose higher digits equal the prefix
// chosen so far, flushed with integer atomics into that pass's global histogram.  The state {prefix, rows
// still to take} never leaves the device: every workgroup of pass p + 1 scans pass p's histogram itself
// (sel_derive) and arrives at the same digit; workgroup 0 also stores the state for the pass after it.
// After the last pass the prefix is the cut key T and `need` the number of rows equal to T to take.  Then
//   count:  per tile of kSelTile rows, the flagged rows below T and equal to T;
//   scan:   one workgroup turns those into exclusive prefixes over the tiles;
//   write:  every tile ranks its rows (ballot + popcount, per-wave offsets in LDS) and stores row i at
//           lt_before(i) + min(eq_before(i), need) when key < T, or key == T and eq_before(i) < need,
// so the output holds the selected rows in ascending row order.  Fewer flagged rows than `limit`: the
// first derive marks the state `all` (T = the largest key, need = no bound), the other histogram passes
// return at once and every flagged row is written.
//
// Plain launches on one stream; no workgroup waits on another; counters are 32-bit (n < 2^31, checked by
// the launcher); counts are integers, so nothing depends on the order the atomics arrive in.
#include <stdexcept>
#include <string>

#include "common.h"
#include "kernels.h"

namespace oni {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRowsPerThread = kSelectTile / kThreads;
constexpr unsigned kNoBound = 0xFFFFFFFFu;

__host__ __device__ constexpr int sel_bits(int p) { return p < kSelectPasses - 1 ? 11 : 9; }
__host__ __device__ constexpr int sel_shift(int p) { return p < kSelectPasses - 1 ? 53 - 11 * p : 0; }
static_assert(sel_shift(kSelectPasses - 2) == sel_bits(kSelectPasses - 1), "digits must tile the 64 bits");
static_assert((1 << sel_bits(0)) == kSelectBins && kSelectBins == 8 * kThreads, "derive: 8 bins per thread");

// state after pass p, kSelectStateWords 32-bit words at work[kSelectPasses * kSelectBins + p * kSelectStateWords]
struct SelState {
  unsigned long long prefix;   // the chosen digits of passes 0..p (after the last pass: the cut key T)
  unsigned need;               // rows still to take among the flagged rows with that prefix (>= 1)
  unsigned all;                // fewer flagged rows than the limit: every one is taken
  unsigned flagged;            // flagged rows (pass 0's total)
  unsigned m;                  // rows selected = min(limit, flagged)
};

__device__ __forceinline__ SelState load_state(const unsigned* w) {
  SelState s;
  s.prefix = ((unsigned long long)w[1] << 32) | w[0];
  s.need = w[2];
  s.all = w[3];
  s.flagged = w[4];
  s.m = w[5];
  return s;
}

__device__ __forceinline__ void store_state(unsigned* w, const SelState& s) {
  w[0] = (unsigned)(s.prefix & 0xFFFFFFFFull);
  w[1] = (unsigned)(s.prefix >> 32);
  w[2] = s.need;
  w[3] = s.all;
  w[4] = s.flagged;
  w[5] = s.m;
}

__device__ __forceinline__ unsigned* state_words(const SelectArgs& a, int p) {
  return a.work + kSelectPasses * kSelectBins + p * kSelectStateWords;
}

__device__ __forceinline__ unsigned long long order_key(double x) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ unsigned wave_incl_scan(unsigned x, int lane) {
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  return x;
}

// Exclusive prefix of x over the workgroup's threads and the workgroup total; sh: kWaves words of LDS that
// no thread reads again before the next __syncthreads() of the caller.
__device__ __forceinline__ unsigned block_excl_scan(unsigned x, unsigned* sh, unsigned& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned inc = wave_incl_scan(x, lane);
  if (lane == 63) sh[wave] = inc;
  __syncthreads();
  unsigned off = 0;
  total = 0;
  for (int w = 0; w < kWaves; ++w) {
    const unsigned c = sh[w];
    if (w < wave) off += c;
    total += c;
  }
  return off + inc - x;
}

// The state after pass p from that pass's finished histogram and the state before it; the same in every
// thread of every workgroup.  sh: kWaves + 2 words of LDS.
__device__ SelState sel_derive(const SelectArgs& a, int p, unsigned* sh) {
  SelState prev;
  if (p == 0) {
    prev.prefix = 0;
    prev.need = a.limit;
    prev.all = 0;
    prev.flagged = 0;
    prev.m = 0;
  } else {
    prev = load_state(state_words(a, p - 1));
  }
  if (prev.all) return prev;
  const unsigned* hist = a.work + p * kSelectBins;
  const int nb = 1 << sel_bits(p);
  unsigned c[8], s = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int b = (int)threadIdx.x * 8 + j;
    c[j] = b < nb ? hist[b] : 0u;
    s += c[j];
  }
  unsigned total;
  const unsigned exc = block_excl_scan(s, sh, total);
  SelState st;
  st.flagged = p == 0 ? total : prev.flagged;
  if (total < prev.need) {     // pass 0 only: fewer flagged rows than the limit
    st.prefix = ~0ull;
    st.need = kNoBound;
    st.all = 1;
    st.m = total;
    return st;
  }
  if (exc < prev.need && prev.need <= exc + s) {     // exactly one thread: need >= 1 and total >= need
    unsigned cum = exc;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (cum < prev.need && prev.need <= cum + c[j]) {
        sh[kWaves] = threadIdx.x * 8 + j;
        sh[kWaves + 1] = cum;
      }
      cum += c[j];
    }
  }
  __syncthreads();
  st.prefix = (prev.prefix << sel_bits(p)) | sh[kWaves];
  st.need = prev.need - sh[kWaves + 1];
  st.all = 0;
  st.m = a.limit;
  return st;
}

__global__ __launch_bounds__(kThreads) void select_hist_kernel(SelectArgs a, int p) {
  __shared__ unsigned h[kSelectBins];
  __shared__ unsigned sh[kWaves + 2];
  unsigned long long prefix = 0;
  if (p > 0) {
    const SelState st = sel_derive(a, p - 1, sh);
    if (blockIdx.x == 0 && threadIdx.x == 0) store_state(state_words(a, p - 1), st);
    if (st.all) return;
    prefix = st.prefix;
  }
  for (int b = threadIdx.x; b < kSelectBins; b += kThreads) h[b] = 0;
  __syncthreads();
  const int shift = sel_shift(p), hi = shift + sel_bits(p);
  const unsigned mask = (1u << sel_bits(p)) - 1u;
  for (unsigned t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    const unsigned base = t * (unsigned)kSelectTile + threadIdx.x;
#pragma unroll
    for (int j = 0; j < kRowsPerThread; ++j) {
      const unsigned i = base + j * kThreads;
      if (i < a.n && a.flag[i]) {
        const unsigned long long ok = order_key(a.key[i]);
        if (p == 0 || (ok >> hi) == prefix) atomicAdd(&h[(unsigned)(ok >> shift) & mask], 1u);
      }
    }
  }
  __syncthreads();
  unsigned* hist = a.work + p * kSelectBins;
  for (int b = threadIdx.x; b <= (int)mask; b += kThreads) {
    const unsigned c = h[b];
    if (c) atomicAdd(&hist[b], c);
  }
}

__device__ __forceinline__ unsigned* tile_counts(const SelectArgs& a) {
  return a.work + kSelectPasses * (kSelectBins + kSelectStateWords);
}

__global__ __launch_bounds__(kThreads) void select_count_kernel(SelectArgs a) {
  __shared__ unsigned sh[kWaves + 2];
  __shared__ unsigned cnt[2][kWaves];
  const SelState st = sel_derive(a, kSelectPasses - 1, sh);
  if (blockIdx.x == 0 && threadIdx.x == 0) store_state(state_words(a, kSelectPasses - 1), st);
  const unsigned long long T = st.prefix;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned* tc = tile_counts(a);
  for (unsigned t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    const unsigned base = t * (unsigned)kSelectTile + threadIdx.x;
    unsigned lt = 0, eq = 0;
#pragma unroll
    for (int j = 0; j < kRowsPerThread; ++j) {
      const unsigned i = base + j * kThreads;
      if (i < a.n && a.flag[i]) {
        const unsigned long long ok = order_key(a.key[i]);
        lt += ok < T;
        eq += ok == T;
      }
    }
    lt = wave_incl_scan(lt, lane);
    eq = wave_incl_scan(eq, lane);
    if (lane == 63) {
      cnt[0][wave] = lt;
      cnt[1][wave] = eq;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
      unsigned s = 0;
      for (int w = 0; w < kWaves; ++w) s += cnt[threadIdx.x][w];
      tc[2 * (size_t)t + threadIdx.x] = s;
    }
    __syncthreads();
  }
}

// one workgroup: tile counts {below T, equal to T} -> their exclusive prefixes over the tiles, in place
__global__ __launch_bounds__(kThreads) void select_scan_kernel(SelectArgs a) {
  __shared__ unsigned sh[2][kWaves];
  unsigned* tc = tile_counts(a);
  const unsigned chunk = (a.ntiles + kThreads - 1) / kThreads;
  const unsigned lo = threadIdx.x * chunk < a.ntiles ? threadIdx.x * chunk : a.ntiles;
  const unsigned hi = lo + chunk < a.ntiles ? lo + chunk : a.ntiles;
  unsigned lt = 0, eq = 0;
  for (unsigned t = lo; t < hi; ++t) {
    lt += tc[2 * (size_t)t];
    eq += tc[2 * (size_t)t + 1];
  }
  unsigned total;
  unsigned run_lt = block_excl_scan(lt, sh[0], total);
  unsigned run_eq = block_excl_scan(eq, sh[1], total);
  for (unsigned t = lo; t < hi; ++t) {
    const unsigned cl = tc[2 * (size_t)t], ce = tc[2 * (size_t)t + 1];
    tc[2 * (size_t)t] = run_lt;
    tc[2 * (size_t)t + 1] = run_eq;
    run_lt += cl;
    run_eq += ce;
  }
}

__global__ __launch_bounds__(kThreads) void select_write_kernel(SelectArgs a) {
  __shared__ unsigned cnt[2][kWaves];
  const SelState st = load_state(state_words(a, kSelectPasses - 1));
  const unsigned long long T = st.prefix;
  const unsigned need = st.need;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  const unsigned* tc = tile_counts(a);
  for (unsigned t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    unsigned run_lt = tc[2 * (size_t)t], run_eq = tc[2 * (size_t)t + 1];
    const unsigned base = t * (unsigned)kSelectTile + threadIdx.x;
    for (int j = 0; j < kRowsPerThread; ++j) {
      const unsigned i = base + j * kThreads;
      bool lt = false, eq = false;
      if (i < a.n && a.flag[i]) {
        const unsigned long long ok = order_key(a.key[i]);
        lt = ok < T;
        eq = ok == T;
      }
      const unsigned long long ml = __ballot(lt), me = __ballot(eq);
      if (lane == 0) {
        cnt[0][wave] = (unsigned)__popcll(ml);
        cnt[1][wave] = (unsigned)__popcll(me);
      }
      __syncthreads();
      unsigned my_lt = run_lt + (unsigned)__popcll(ml & below), my_eq = run_eq + (unsigned)__popcll(me & below);
      for (int w = 0; w < kWaves; ++w) {
        const unsigned cl = cnt[0][w], ce = cnt[1][w];
        if (w < wave) {
          my_lt += cl;
          my_eq += ce;
        }
        run_lt += cl;
        run_eq += ce;
      }
      if (lt || (eq && my_eq < need)) {
        const unsigned pos = my_lt + (my_eq < need ? my_eq : need);
        if (pos < a.out_cap) a.out[pos] = (long long)i;   // pos < m <= out_cap by construction
      }
      __syncthreads();
    }
  }
}

}  // namespace

size_t select_work_words(int64_t n) {
  const int64_t ntiles = (n + kSelectTile - 1) / kSelectTile;
  return (size_t)kSelectPasses * (kSelectBins + kSelectStateWords) + 2 * (size_t)ntiles;
}

int select_result_word() { return kSelectPasses * kSelectBins + (kSelectPasses - 1) * kSelectStateWords + 4; }

void launch_select_lowest(const SelectArgs& a, int max_blocks, hipStream_t s) {
  if (a.n <= 0) throw std::runtime_error("select_lowest: no rows");
  if (a.n >= ((int64_t)1 << 31)) throw std::runtime_error("select_lowest: n >= 2^31 rows (32-bit counters)");
  if (a.limit < 1) throw std::runtime_error("select_lowest: limit must be >= 1");
  if ((int64_t)a.ntiles != (a.n + kSelectTile - 1) / kSelectTile) throw std::runtime_error("select_lowest: tile count");
  if (!a.key || !a.flag || !a.work || !a.out) throw std::runtime_error("select_lowest: null buffer");
  if ((int64_t)a.out_cap < ((int64_t)a.limit < a.n ? (int64_t)a.limit : a.n))
    throw std::runtime_error("select_lowest: output too small");
  // every pass's histogram and state, cleared at once
  ONI_HIP_CHECK(hipMemsetAsync(a.work, 0, sizeof(unsigned) * kSelectPasses * (kSelectBins + kSelectStateWords), s));
  unsigned blocks = a.ntiles;
  const unsigned cap = max_blocks > 0 ? (unsigned)max_blocks : 2048u;
  if (blocks > cap) blocks = cap;
  for (int p = 0; p < kSelectPasses; ++p)
    hipLaunchKernelGGL(select_hist_kernel, dim3(blocks), dim3(kThreads), 0, s, a, p);
  hipLaunchKernelGGL(select_count_kernel, dim3(blocks), dim3(kThreads), 0, s, a);
  hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(kThreads), 0, s, a);
  hipLaunchKernelGGL(select_write_kernel, dim3(blocks), dim3(kThreads), 0, s, a);
  ONI_HIP_CHECK(hipGetLastError());
}

}  // namespace oni
