// Ensemble event scoring (oni_ml_amd/score/scorer.py EnsembleModel; twin: ops/reference.py score_ensemble).
//
// R models fitted on the same corpus from different seeds share their document and word rows.  The score of
// an event side is the uniform mixture of the members:
//
//   s_r   = sum_{k<K} theta_r[doc][k] * phi_r[word][k]      (score_events.hip score_one, bit for bit)
//   score = (((0.0 + s_0) + s_1) + ... + s_{R-1}) / (double)R
//
// Every operation is a rounded fp64 one in the order written (contraction off), so the torch twin matches bit
// for bit and R = 1 is score_events.  A miss (row -1) takes the constant default vector in every member.
//   key   = min of the two ensemble side scores (a < b ? a : b), or the one side
//   flag  = key < tol
//   votes = number of members whose own key (the min of that member's two side scores) is < tol
//
// Tables are interleaved per row, theta [D][R][K] and phi [V][R][K]: the R member rows of a side are one
// contiguous run of R K doubles.  One event per lane, grid-stride; no LDS, no atomics.  With K even every
// member row starts on a 16-byte boundary and is read as double2; K = 20 (the reference's topic count) has an
// instantiation with the topic loop unrolled, so a member row's loads are all issued before the first add.
#include <stdexcept>
#include <string>

#include "common.h"
#include "kernels.h"

namespace oni {

namespace {

constexpr int kThreads = 256;

// one member's score; tr / pr: the member's row or nullptr (miss).  VEC: K is even, rows are 16-byte aligned.
// KC: K when it is known at compile time (the loop unrolls), else 0.
template <bool VEC, int KC>
__device__ __forceinline__ double member_score(const double* __restrict__ tr, const double* __restrict__ pr, int Kr,
                                               double dflt) {
  // HIP compiles with -ffp-contract=fast; the JVM rounds the product and the sum separately.
#pragma clang fp contract(off)
  const int K = KC ? KC : Kr;
  double s = 0.0;
  if (VEC) {
    const double2* t2 = reinterpret_cast<const double2*>(tr);
    const double2* p2 = reinterpret_cast<const double2*>(pr);
    const double2 d2 = make_double2(dflt, dflt);
#pragma unroll
    for (int k = 0; k < K / 2; ++k) {
      const double2 t = tr ? t2[k] : d2;
      const double2 p = pr ? p2[k] : d2;
      const double p0 = t.x * p.x;
      s = s + p0;
      const double p1 = t.y * p.y;
      s = s + p1;
    }
  } else {
    for (int k = 0; k < K; ++k) {
      const double tk = tr ? tr[k] : dflt;
      const double pk = pr ? pr[k] : dflt;
      const double prod = tk * pk;  // contract(off): rounded product, then rounded sum
      s = s + prod;
    }
  }
  return s;
}

template <bool VEC, int KC>
__global__ __launch_bounds__(kThreads) void score_ensemble_kernel(EnsembleScoreArgs a) {
#pragma clang fp contract(off)
  const int K = KC ? KC : a.K;
  const size_t run = (size_t)a.R * K;        // doubles of one row's members
  const double rd = (double)a.R;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kThreads) {
    const int da = a.doc_a[i], wa = a.word_a[i];
    const double* ta = da >= 0 ? a.theta + (size_t)da * run : nullptr;
    const double* pa = wa >= 0 ? a.phi + (size_t)wa * run : nullptr;
    const double* tb = nullptr;
    const double* pb = nullptr;
    if (a.doc_b) {
      const int db = a.doc_b[i], wb = a.word_b[i];
      tb = db >= 0 ? a.theta + (size_t)db * run : nullptr;
      pb = wb >= 0 ? a.phi + (size_t)wb * run : nullptr;
    }
    double sum_a = 0.0, sum_b = 0.0;
    unsigned votes = 0;
    for (int r = 0; r < a.R; ++r) {
      const size_t o = (size_t)r * K;
      const double sa = member_score<VEC, KC>(ta ? ta + o : nullptr, pa ? pa + o : nullptr, K, a.dflt);
      sum_a = sum_a + sa;
      double mk = sa;
      if (a.doc_b) {
        const double sb = member_score<VEC, KC>(tb ? tb + o : nullptr, pb ? pb + o : nullptr, K, a.dflt);
        sum_b = sum_b + sb;
        mk = sa < sb ? sa : sb;
      }
      votes += mk < a.tol ? 1u : 0u;
    }
    const double ea = sum_a / rd;
    double key = ea;
    a.score_a[i] = ea;
    if (a.doc_b) {
      const double eb = sum_b / rd;
      a.score_b[i] = eb;
      key = ea < eb ? ea : eb;  // breeze/scala min on two doubles
    }
    a.key[i] = key;
    a.flag[i] = key < a.tol ? 1 : 0;
    a.votes[i] = (uint8_t)votes;
  }
}

}  // namespace

void launch_score_ensemble(const EnsembleScoreArgs& a, int max_blocks, hipStream_t s) {
  if (a.n < 0 || a.n >= ((int64_t)1 << 31)) throw std::runtime_error("score_ensemble: n outside 0 .. 2^31 - 1");
  if (a.R < 1 || a.R > kEnsembleMax)
    throw std::runtime_error("score_ensemble: R outside 1 .. " + std::to_string(kEnsembleMax));
  if (a.K < 1) throw std::runtime_error("score_ensemble: K < 1");
  if (max_blocks < 0) throw std::runtime_error("score_ensemble: max_blocks < 0");
  if (a.n == 0) return;
  if (!a.theta || !a.phi || !a.doc_a || !a.word_a || !a.score_a || !a.key || !a.flag || !a.votes)
    throw std::runtime_error("score_ensemble: null buffer");
  if ((a.doc_b == nullptr) != (a.word_b == nullptr) || (a.doc_b == nullptr) != (a.score_b == nullptr))
    throw std::runtime_error("score_ensemble: doc_b, word_b and score_b go together");
  int64_t blocks = (a.n + kThreads - 1) / kThreads;
  const int64_t cap = max_blocks > 0 ? max_blocks : 8192;
  if (blocks > cap) blocks = cap;
  const bool vec = a.K % 2 == 0 && ((uintptr_t)a.theta % 16 == 0) && ((uintptr_t)a.phi % 16 == 0);
  if (vec && a.K == 20)
    hipLaunchKernelGGL((score_ensemble_kernel<true, 20>), dim3((unsigned)blocks), dim3(kThreads), 0, s, a);
  else if (vec)
    hipLaunchKernelGGL((score_ensemble_kernel<true, 0>), dim3((unsigned)blocks), dim3(kThreads), 0, s, a);
  else
    hipLaunchKernelGGL((score_ensemble_kernel<false, 0>), dim3((unsigned)blocks), dim3(kThreads), 0, s, a);
  ONI_HIP_CHECK(hipGetLastError());
}

}  // namespace oni
