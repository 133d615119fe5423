// Host planner of the fp64 engine's headline path (KS <= 32, U <= the LDS chunk tables, no split documents,
// no c.phi windows): everything LDAEngine's Python planners (ops/hip.py GSPlan, SuffPlan, GSStage,
// gs_chunk_sums, the tables behind gs_et_rows; models/lda/em.py _build_suff_split) derive from the host CSR,
// array for array, in one pass into one caller-provided buffer that is uploaded once.
#pragma once
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

namespace onin {

struct PlanEdge {
  int variant;   // the kernel variant of the bucket (ops/hip.py GS_*)
  int64_t lo;    // lengths > lo ( < 0: > the tiny bound)
  int64_t hi;    // lengths <= hi ( < 0: no upper edge)
};

struct EnginePlanIn {
  const int64_t* doc_ptr = nullptr;   // [D + 1]
  const int32_t* word_idx = nullptr;  // [nnz]
  const int64_t* counts = nullptr;    // [nnz]
  int64_t D = 0, V = 0, nnz = 0;
  int KS = 0, U = 0;
  std::vector<PlanEdge> edges;        // GSPlan.EDGES_NARROW, in launch order
  int tiny_variant = 0;               // GS_TINY
  int team8_variant = 3;              // GS_TEAM8: the bucket that is staged, isolated, gets chunk sums
  int64_t tiny = 0;                   // min(gs_tiny_max(KS), U)
  int64_t heavy = 1024, light = 64;   // SuffPlan.HEAVY / LIGHT
  double late_share = 0.6;            // no early / late split when the late bucket holds more of the entries
  int suff_split = 1;                 // 0 off, 1 auto, 2 force
  double stage_cap = 0;               // staged-rows budget in bytes (0: no staged rows)
  int umax = 32;                      // GS_LDS_UMAX: rows of a document's chunk tables
  int iso_m = 1, xcds = 8;            // isolate_longest(o, m, xcds) on the team8 bucket (m = 0: off)
  bool defer_final = true;
  int threads = 1;
};

struct PlanSection {
  std::string name;
  int64_t offset = 0;   // bytes from the buffer's start, a multiple of 256
  int64_t count = 0;    // elements
  int elem = 4;         // bytes per element
};

struct PlanBucket {
  int variant;
  int64_t offset, count;   // elements into the "orders" section
};

struct EnginePlanOut {
  std::vector<PlanSection> sections;
  std::vector<PlanBucket> buckets;
  int64_t bytes = 0;                       // bytes of the buffer in use
  std::vector<int64_t> doc_len, word_len;  // host copies (DeviceCorpus.doc_len / word_len)
  // suff-stats plans: full, early, late -- {n_heavy, n_medium, n_light}
  int64_t suff_counts[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  bool split = false;      // early / late suff-stats (else the early / late sections are absent)
  bool defer = false;      // the late bucket defers its final pass (et tables present)
  int64_t late_docs = 0, n_early = 0, n_late = 0;   // documents of the late bucket; CSC slots of either side
  bool staged = false;     // staged rows of the team8 bucket (stage_* sections present)
  int64_t n_tiles = 0;
  bool csum = false;       // chunk sums of the team8 bucket
  std::vector<std::pair<std::string, double>> phase_us;   // the planner's phases, microseconds each
  const PlanSection* find(const std::string& name) const {
    for (const auto& s : sections)
      if (s.name == name) return &s;
    return nullptr;
  }
};

// Upper bound of the buffer's bytes for a corpus of these sizes (team8_lo: the team8 bucket's lower edge,
// which bounds its documents by nnz / (team8_lo + 1); < 1: any document may be one).
int64_t engine_plan_bound(int64_t D, int64_t V, int64_t nnz, int64_t team8_lo, int xcds);

// Plans into buf[0, cap); throws std::invalid_argument on inconsistent input, std::length_error when cap is
// too small.
EnginePlanOut engine_plan(const EnginePlanIn& in, void* buf, int64_t cap);

}  // namespace onin
