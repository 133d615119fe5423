// splitmix64: the counter-based generator shared by the device and the host (plain C++, no other include).
//   * lda-c "random" start: u = splitmix64(splitmix64(seed) ^ (k V + w)) >> 11, x 2^-53
//     (csrc/hip/lda_gs64.hip init_random_ss_kernel, csrc/native/bind_native.cpp random_ss)
//   * --holdout: token g is held out iff splitmix64(key ^ g) >> 11 < thr (csrc/hip/holdout.hip;
//     oni_ml_amd/ops/reference.py splitmix64 is the torch twin)
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SPLITMIX_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define SPLITMIX_HD inline
#endif

namespace oni {

SPLITMIX_HD unsigned long long splitmix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

}  // namespace oni
