// Shannon entropy of the bytes of every string of a batch (proxy front end: H(fulluri) of every request).
//
//   H(s) = (t[n] - sum_b t[c_b]) / n,   t[c] = c log2(c),  t[0] = t[1] = 0,   H = 0 for n <= 1
//
// n: the string's byte length, c_b: the count of byte value b (unsigned).  t is a host-built fp64 table
// (ops/reference.py entropy_table) sized to the longest string of the call: the device evaluates no log,
// and with the summation order below the result is one fixed bit pattern, which the numpy twin
// (ops/reference.py string_entropy) reproduces:
//
//   lane l of the wave sums its four byte values in ascending order,
//       p_l = ((t[c_4l] + t[c_4l+1]) + t[c_4l+2]) + t[c_4l+3]
//   then a balanced tree over the 64 lanes, neighbours first: (p_0 + p_1), (p_2 + p_3), ... , then pairs of
//   those, six levels.  Every step adds a lane and its partner, and a + b == b + a bit for bit, so the xor
//   butterfly leaves that tree's value in every lane.
//
// One wave per string, grid-strided; four waves per workgroup, each with its own 256 x u32 LDS histogram
// filled by LDS integer atomics.  A wave's LDS operations execute in program order; the wavefront fences
// below keep the compiler from moving a string's clear, its atomics and its reads across each other (the
// waves of a workgroup take different numbers of strings, so there is no workgroup barrier in the loop).
//
// No load touches a byte outside [begin, end) of its string: the bytes up to the first 16-byte-aligned
// address and those after the last one are loaded one by one, the aligned middle as uint4.
#include "common.h"
#include "kernels.h"

namespace oni {

namespace {

constexpr int kEntropyWaves = 4;   // waves (strings in flight) per workgroup

__device__ __forceinline__ void wave_order() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ void count4(unsigned* hist, unsigned w) {
  atomicAdd(&hist[w & 0xffu], 1u);
  atomicAdd(&hist[(w >> 8) & 0xffu], 1u);
  atomicAdd(&hist[(w >> 16) & 0xffu], 1u);
  atomicAdd(&hist[w >> 24], 1u);
}

__device__ __forceinline__ double shfl_xor_f64(double x, int mask) {
  const long long b = __double_as_longlong(x);
  const int lo = __shfl_xor((int)(b & 0xffffffffLL), mask, 64), hi = __shfl_xor((int)(b >> 32), mask, 64);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

}  // namespace

__global__ __launch_bounds__(64 * kEntropyWaves) void string_entropy_kernel(StringEntropyArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned lds[kEntropyWaves][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned* hist = lds[wave];
  const int64_t stride = (int64_t)gridDim.x * kEntropyWaves;
  for (int64_t s = (int64_t)blockIdx.x * kEntropyWaves + wave; s < a.n; s += stride) {
    const int64_t o0 = a.offsets[s], o1 = a.offsets[s + 1];
    const int64_t len = o1 - o0;
    if (len <= 1) {                      // wave-uniform
      if (lane == 0) a.out[s] = 0.0;
      continue;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) hist[4 * lane + k] = 0u;
    wave_order();
    const uint8_t* p = a.bytes + o0;
    const uint8_t* end = a.bytes + o1;
    // [p, v0): bytes before the first 16-byte boundary; [v0, v1): whole aligned uint4; [v1, end): the rest
    const uintptr_t ap = reinterpret_cast<uintptr_t>(p), ae = reinterpret_cast<uintptr_t>(end);
    uintptr_t a0 = (ap + 15) & ~(uintptr_t)15;
    if (a0 > ae) a0 = ae;
    const uintptr_t a1 = a0 + ((ae - a0) & ~(uintptr_t)15);
    const uint8_t* v0 = p + (a0 - ap);
    const uint8_t* v1 = p + (a1 - ap);
    if (p + lane < v0) atomicAdd(&hist[p[lane]], 1u);            // < 16 bytes
    if (v1 + lane < end) atomicAdd(&hist[v1[lane]], 1u);         // < 16 bytes
    const uint4* vec = reinterpret_cast<const uint4*>(v0);
    const int64_t nvec = (int64_t)(a1 - a0) >> 4;
    for (int64_t i = lane; i < nvec; i += 64) {
      const uint4 w = vec[i];
      count4(hist, w.x);
      count4(hist, w.y);
      count4(hist, w.z);
      count4(hist, w.w);
    }
    wave_order();
    const uint4 c = make_uint4(hist[4 * lane], hist[4 * lane + 1], hist[4 * lane + 2], hist[4 * lane + 3]);
    wave_order();                        // the next string's clear stays behind these reads
    // counts <= len <= a.table_len - 1 (checked on the host); t[0] = t[1] = 0 need no load
    const double t0 = c.x > 1u ? a.table[c.x] : 0.0, t1 = c.y > 1u ? a.table[c.y] : 0.0;
    const double t2 = c.z > 1u ? a.table[c.z] : 0.0, t3 = c.w > 1u ? a.table[c.w] : 0.0;
    double sum = ((t0 + t1) + t2) + t3;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) sum = sum + shfl_xor_f64(sum, m);
    if (lane == 0) a.out[s] = (a.table[len] - sum) / (double)len;
  }
}

void launch_string_entropy(const StringEntropyArgs& a, int max_blocks, hipStream_t s) {
  if (a.n <= 0) return;
  const int64_t cap = max_blocks > 0 ? max_blocks : 4096;
  int64_t blocks = (a.n + kEntropyWaves - 1) / kEntropyWaves;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(string_entropy_kernel, dim3((unsigned)blocks), dim3(64 * kEntropyWaves), 0, s, a);
  ONI_HIP_CHECK(hipGetLastError());
}

}  // namespace oni
