// The scorers' theta_d . phi_w (score_events.hip, holdout.hip): one rounded multiply and one rounded add per
// topic, in topic order, from 0.0 -- what the reference evaluates on the JVM in strict IEEE double.
#pragma once
#include <hip/hip_runtime.h>

namespace oni {

__device__ __forceinline__ double score_one(const double* __restrict__ theta, const double* __restrict__ phi,
                                            int K, double dflt, int d, int w) {
  // HIP compiles with -ffp-contract=fast; the JVM rounds the product and the sum separately.
#pragma clang fp contract(off)
  const double* tr = d >= 0 ? theta + (size_t)d * K : nullptr;
  const double* pr = w >= 0 ? phi + (size_t)w * K : nullptr;
  double s = 0.0;
  for (int k = 0; k < K; ++k) {
    const double tk = tr ? tr[k] : dflt;
    const double pk = pr ? pr[k] : dflt;
    const double prod = tk * pk;  // contract(off): rounded product, then rounded sum
    s = s + prod;
  }
  return s;
}

}  // namespace oni
