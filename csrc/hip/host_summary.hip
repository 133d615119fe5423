// Host report: the day's scored sides folded per document (oni_ml_amd/score/scorer.py host_summary).
//
// Event i has a side a (doc_a[i], score_a[i]) and, for flow, a side b (doc_b[i], score_b[i]); side number
// 2 * i + side.  A side whose row is outside [0, D) (-1: the IP is not a document) takes no part and is
// counted in `skipped`.  For every document d:
//   events[d]   sides with doc == d (a flow from an IP to itself counts twice);
//   flagged[d]  of those, the sides with score < tol (a NaN score is never under tol);
//   min_key[d]  the lowest order key of their non-NaN scores -- ops/sortgroup.py f64_order_keys as an unsigned
//               64-bit integer, the order select_lowest.hip uses: -0.0 sits just below +0.0 -- all-ones: none;
//   worst[d]    the lowest side number among the sides whose key is min_key[d]; all-ones: none.
//
// Two grid-stride passes over the events:
//   pass 1:  the counts by 32-bit atomicAdd and min_key by 64-bit atomicMin;
//   pass 2:  every side whose key equals the finished min_key[doc] does a 32-bit atomicMin of its side
//            number into worst[doc].
// One document can own a large share of the sides (the day's busiest resolver), so one address can receive a
// large share of the atomics, and atomics on one address execute one after the other (measured on an MI355X,
// profiles/host_report.md: about 90 M a second on one address against 15 G a second on spread addresses).
// Two measures, both on purpose:
//   * the minima are filtered: the current value is read first with a relaxed agent-scope load (it is served
//     by L2, where the atomics execute; a plain load could keep returning a stale line of the CU's L1) and
//     the atomic is skipped when the side cannot lower it.  The value only ever decreases, so whatever the
//     load returns is an upper bound of the current value and the filter never drops a side that would win;
//   * the counts cannot be filtered, every side must add.  With `fold` each wave folds them first.  A lane
//     whose neighbour has the same document marks a document that repeats in the wave; while there is such a
//     lane, the first one broadcasts its document, a ballot counts the lanes that have it, and the count goes
//     into the wave's one pending entry {document, sides, flagged}.  The entry is carried over the grid-stride
//     loop and added with one atomic pair only when another document takes its place and after the loop, so a
//     document with half of the sides costs a wave a handful of atomics in all.  The lanes left add 1 each.
//     (A document with share p of the sides has two neighbouring lanes in a wave with probability
//     1 - (1 - p^2)^63: 0.98 at p = 0.25, 0.47 at p = 0.1.  Below that its address is not hot.)
// Plain launches on one stream; no workgroup waits on another; counters are 32-bit (n < 2^31, checked by the
// launcher).  Every quantity is an integer count or a minimum, so nothing depends on the order the atomics
// arrive in: the outputs are the same bits on every run, for every grid size, with and without the fold.
#include <stdexcept>
#include <string>

#include "common.h"
#include "kernels.h"

namespace oni {

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ unsigned long long order_key(double x) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

template <typename T>
__device__ __forceinline__ T load_l2(const T* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// per-thread tallies of the atomics issued (stats != nullptr only)
struct Tally {
  unsigned counts, mins, worsts;
};

// the counts of one document a wave has folded and not yet added; the same in every lane
struct Pending {
  int doc;      // -1: none
  unsigned events, flagged;
};

__device__ __forceinline__ void flush(const HostSummaryArgs& a, Pending& p, Tally& t) {
  if (p.doc >= 0 && (threadIdx.x & 63) == 0) {
    atomicAdd(&a.events[p.doc], p.events);
    ++t.counts;
    if (p.flagged) {
      atomicAdd(&a.flagged[p.doc], p.flagged);
      ++t.counts;
    }
  }
  p.doc = -1;
  p.events = p.flagged = 0;
}

// events[d] += 1 and flagged[d] += fl for every lane with `valid`; with a.fold the documents that repeat in
// neighbouring lanes go through the wave's pending entry.  Called by every lane of the wave (the ballots
// need them all).
__device__ __forceinline__ void add_counts(const HostSummaryArgs& a, bool valid, int d, bool fl, Pending& p, Tally& t) {
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(valid);
  if (a.fold) {
    const int next = __shfl_down(d, 1);
    const bool pair = valid && lane < 63 && ((todo >> (lane + 1)) & 1ull) && d == next;
    unsigned long long cand = __ballot(pair);
    while (cand) {
      const int dl = __shfl(d, __ffsll((long long)cand) - 1);
      const bool mine = valid && d == dl;
      const unsigned long long same = __ballot(mine);
      if (p.doc != dl) {
        flush(a, p, t);
        p.doc = dl;
      }
      p.events += (unsigned)__popcll(same);
      p.flagged += (unsigned)__popcll(__ballot(mine && fl));
      todo &= ~same;
      cand &= ~same;
    }
  }
  if ((todo >> lane) & 1ull) {
    atomicAdd(&a.events[d], 1u);
    ++t.counts;
    if (fl) {
      atomicAdd(&a.flagged[d], 1u);
      ++t.counts;
    }
  }
}

__device__ __forceinline__ unsigned wave_sum(unsigned x) {
  for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d);
  return x;
}

__device__ __forceinline__ void flush_stats(const HostSummaryArgs& a, const Tally& t) {
  if (!a.stats) return;
  const unsigned c = wave_sum(t.counts), m = wave_sum(t.mins), w = wave_sum(t.worsts);
  if ((threadIdx.x & 63) == 0) {
    if (c) atomicAdd(&a.stats[0], (unsigned long long)c);
    if (m) atomicAdd(&a.stats[1], (unsigned long long)m);
    if (w) atomicAdd(&a.stats[2], (unsigned long long)w);
  }
}

__global__ __launch_bounds__(kThreads) void host_summary_pass1(HostSummaryArgs a) {
  const long long stride = (long long)gridDim.x * kThreads;
  const int sides = a.doc_b ? 2 : 1;
  unsigned skipped = 0;
  Tally t{0, 0, 0};
  Pending p{-1, 0, 0};
  // the bound is the same for the whole workgroup: every lane of a wave reaches the ballots of add_counts
  for (long long base = (long long)blockIdx.x * kThreads; base < a.n; base += stride) {
    const long long i = base + threadIdx.x;
    const bool in = i < a.n;
    for (int side = 0; side < sides; ++side) {
      const int* doc = side ? a.doc_b : a.doc_a;
      const double* score = side ? a.score_b : a.score_a;
      const int d = in ? doc[i] : -1;
      const double s = in ? score[i] : 0.0;
      const bool valid = in && d >= 0 && (long long)d < a.D;
      skipped += in && !valid;
      add_counts(a, valid, d, s < a.tol, p, t);
      if (valid && s == s) {
        const unsigned long long k = order_key(s);
        if (k < load_l2(&a.min_key[d])) {
          atomicMin(&a.min_key[d], k);
          ++t.mins;
        }
      }
    }
  }
  flush(a, p, t);
  skipped = wave_sum(skipped);
  if ((threadIdx.x & 63) == 0 && skipped) atomicAdd(a.skipped, skipped);
  flush_stats(a, t);
}

__global__ __launch_bounds__(kThreads) void host_summary_pass2(HostSummaryArgs a) {
  const long long stride = (long long)gridDim.x * kThreads;
  const int sides = a.doc_b ? 2 : 1;
  Tally t{0, 0, 0};
  for (long long base = (long long)blockIdx.x * kThreads; base < a.n; base += stride) {
    const long long i = base + threadIdx.x;
    if (i < a.n) {
      for (int side = 0; side < sides; ++side) {
        const int d = (side ? a.doc_b : a.doc_a)[i];
        const double s = (side ? a.score_b : a.score_a)[i];
        if (d >= 0 && (long long)d < a.D && s == s && order_key(s) == a.min_key[d]) {
          const unsigned num = 2u * (unsigned)i + (unsigned)side;
          if (num < load_l2(&a.worst[d])) {
            atomicMin(&a.worst[d], num);
            ++t.worsts;
          }
        }
      }
    }
  }
  flush_stats(a, t);
}

}  // namespace

void launch_host_summary(const HostSummaryArgs& a, int max_blocks, hipStream_t s) {
  if (a.n <= 0 || a.n >= ((int64_t)1 << 31)) throw std::runtime_error("host_summary: n outside 1 .. 2^31 - 1");
  if (a.D <= 0 || a.D >= ((int64_t)1 << 31)) throw std::runtime_error("host_summary: D outside 1 .. 2^31 - 1");
  if (!a.doc_a || !a.score_a || !a.events || !a.flagged || !a.min_key || !a.worst || !a.skipped)
    throw std::runtime_error("host_summary: null buffer");
  if ((a.doc_b == nullptr) != (a.score_b == nullptr)) throw std::runtime_error("host_summary: doc_b without score_b");
  if (max_blocks < 0) throw std::runtime_error("host_summary: max_blocks < 0");
  ONI_HIP_CHECK(hipMemsetAsync(a.events, 0, sizeof(unsigned) * (size_t)a.D, s));
  ONI_HIP_CHECK(hipMemsetAsync(a.flagged, 0, sizeof(unsigned) * (size_t)a.D, s));
  ONI_HIP_CHECK(hipMemsetAsync(a.min_key, 0xFF, sizeof(unsigned long long) * (size_t)a.D, s));
  ONI_HIP_CHECK(hipMemsetAsync(a.worst, 0xFF, sizeof(unsigned) * (size_t)a.D, s));
  ONI_HIP_CHECK(hipMemsetAsync(a.skipped, 0, sizeof(unsigned), s));
  if (a.stats) ONI_HIP_CHECK(hipMemsetAsync(a.stats, 0, sizeof(unsigned long long) * kHostSummaryStats, s));
  int64_t blocks = (a.n + kThreads - 1) / kThreads;
  const int64_t cap = max_blocks > 0 ? max_blocks : 2048;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(host_summary_pass1, dim3((unsigned)blocks), dim3(kThreads), 0, s, a);
  hipLaunchKernelGGL(host_summary_pass2, dim3((unsigned)blocks), dim3(kThreads), 0, s, a);
  ONI_HIP_CHECK(hipGetLastError());
}

}  // namespace oni
