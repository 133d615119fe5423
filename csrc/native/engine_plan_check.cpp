// Stand-alone check of the engine planner (engine_plan.cpp) for a host sanitizer build
// (scripts/engine_plan_check.sh: -fsanitize=address,undefined; a CPU program, never loaded into Python).
// Corpora from a fixed LCG -- the bucket edges from both sides, equal lengths, empty documents at both ends,
// 0 / 1 / 8 / 9 team8 documents, a dominant late bucket, large counts -- planned at (KS, U) = (20, 32), (8, 8),
// (32, 32) and compared with a reference written from std::stable_sort inside this program.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "engine_plan.h"

using namespace onin;

static uint64_t g_lcg = 0x2545F4914F6CDD1Dull;
static uint32_t rnd() {
  g_lcg = g_lcg * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_lcg >> 33);
}

struct Case {
  std::vector<int64_t> ptr, cnt;
  std::vector<int32_t> w;
  int64_t V;
};

static Case make(const std::vector<int64_t>& lens, int64_t V, int64_t big = 0) {
  Case c;
  c.V = V;
  c.ptr.push_back(0);
  for (int64_t n : lens) {
    const int64_t start = rnd() % V;   // n distinct words: a run of consecutive ids from a random start
    for (int64_t i = 0; i < n; ++i) {
      c.w.push_back((int32_t)((start + i) % V));
      c.cnt.push_back(big && i < 129 && n > 4000 ? big : 1 + rnd() % 5);
    }
    c.ptr.push_back((int64_t)c.w.size());
  }
  return c;
}

static int g_fail = 0;
#define CHECK(x)                                                        \
  do {                                                                  \
    if (!(x)) {                                                         \
      std::printf("FAILED %s (line %d, case %d)\n", #x, __LINE__, g_case); \
      ++g_fail;                                                         \
    }                                                                   \
  } while (0)
static int g_case = 0;

template <class T>
static const T* sec(const EnginePlanOut& o, const char* buf, const char* name, int64_t* n = nullptr) {
  const PlanSection* s = o.find(name);
  if (!s) return nullptr;
  if (n) *n = s->count;
  if (s->offset % 256 || s->elem != (int)sizeof(T)) {
    std::printf("FAILED section %s layout\n", name);
    ++g_fail;
  }
  return reinterpret_cast<const T*>(buf + s->offset);
}

static std::vector<int32_t> desc_stable(const std::vector<int64_t>& key) {
  std::vector<int32_t> o(key.size());
  std::iota(o.begin(), o.end(), 0);
  std::stable_sort(o.begin(), o.end(), [&](int32_t a, int32_t b) { return key[a] > key[b]; });
  return o;
}

static void run(const Case& c, int KS, int U, int suff_split, double stage_cap) {
  ++g_case;
  EnginePlanIn in;
  in.doc_ptr = c.ptr.data();
  in.word_idx = c.w.data();
  in.counts = c.cnt.data();
  in.D = (int64_t)c.ptr.size() - 1;
  in.V = c.V;
  in.nnz = (int64_t)c.w.size();
  in.KS = KS;
  in.U = U;
  in.edges = {{3, 2048, -1}, {2, 256, 2048}, {1, 64, 256}, {4, -1, 64}};
  in.tiny = std::min(KS <= 20 ? 16 : 8, U);
  in.suff_split = suff_split;
  in.stage_cap = stage_cap;
  in.threads = 1 + g_case % 3;
  const int64_t cap = engine_plan_bound(in.D, in.V, in.nnz, 2048, in.xcds);
  std::vector<char> raw((size_t)cap + 256);
  char* buf = raw.data() + (256 - reinterpret_cast<uintptr_t>(raw.data()) % 256) % 256;
  const EnginePlanOut o = engine_plan(in, buf, cap);
  CHECK(o.bytes <= cap);
  const int64_t D = in.D, V = in.V, nnz = in.nnz;

  // corpus arrays
  std::vector<int64_t> len((size_t)D), wl((size_t)V, 0);
  for (int64_t d = 0; d < D; ++d) len[d] = c.ptr[d + 1] - c.ptr[d];
  for (int32_t w : c.w) ++wl[w];
  CHECK(o.doc_len == len && o.word_len == wl);
  const int32_t* dp = sec<int32_t>(o, buf, "doc_ptr");
  const float* cf = sec<float>(o, buf, "counts");
  const int32_t* wi = sec<int32_t>(o, buf, "word_idx");
  const int32_t* wp = sec<int32_t>(o, buf, "word_ptr");
  for (int64_t d = 0; d <= D; ++d) CHECK(dp[d] == c.ptr[d]);
  for (int64_t i = 0; i < nnz; ++i) CHECK(wi[i] == c.w[i] && cf[i] == (float)c.cnt[i]);
  int64_t run_ = 0;
  for (int64_t w = 0; w <= V; ++w) {
    CHECK(wp[w] == run_);
    if (w < V) run_ += wl[w];
  }

  // buckets: the stable descending order filtered per edge, the team8 one with its gaps
  const std::vector<int32_t> ord = desc_stable(len);
  std::vector<std::pair<int, std::vector<int32_t>>> want;
  auto add = [&](int var, int64_t lo, int64_t hi) {
    std::vector<int32_t> b;
    for (int32_t d : ord)
      if (len[d] > lo && (hi < 0 || len[d] <= hi)) b.push_back(d);
    if (var == 3 && !b.empty()) {   // isolate_longest(o, 1, 8): slot 0 the longest, slots 8, 16, ... empty
      std::vector<int32_t> g;
      size_t r = 1;
      for (int64_t s = 0; r < b.size() || s == 0; ++s) g.push_back(s == 0 ? b[0] : (s % 8 == 0 ? -1 : b[r++]));
      while (g.back() == -1) g.pop_back();
      b = g;
    }
    if (!b.empty()) want.push_back({var, b});
  };
  for (const auto& e : in.edges) add(e.variant, e.lo < 0 ? in.tiny : e.lo, e.hi);
  add(0, -1, in.tiny);
  CHECK(o.buckets.size() == want.size());
  for (size_t i = 0; i < want.size() && i < o.buckets.size(); ++i) {
    const auto& b = o.buckets[i];
    CHECK(b.variant == want[i].first && b.count == (int64_t)want[i].second.size() && b.offset % 256 == 0);
    const int32_t* p = reinterpret_cast<const int32_t*>(buf + b.offset);
    if (b.count == (int64_t)want[i].second.size()) CHECK(std::equal(p, p + b.count, want[i].second.begin()));
  }

  // suff-stats plans
  auto suff = [&](const char* name, const std::vector<int64_t>& l, const int64_t got[3]) {
    const std::vector<int32_t> so = desc_stable(l);
    const int32_t* p = sec<int32_t>(o, buf, name);
    CHECK(p && std::equal(so.begin(), so.end(), p));
    int64_t h = 0, m = 0, s = 0;
    for (int64_t x : l) (x > 1024 ? h : (x > 64 ? m : s))++;
    CHECK(got[0] == h && got[1] == m && got[2] == s);
  };
  suff("suff_order", wl, o.suff_counts[0]);
  std::vector<int64_t> lenL((size_t)V, 0), lenE((size_t)V);
  std::vector<uint8_t> mask((size_t)D, 0);
  int64_t late_n = 0, late_sum = 0;
  if (want.size() >= 2)
    for (int32_t d : want[0].second)
      if (d >= 0) {
        ++late_n;
        late_sum += len[d];
        mask[d] = 1;
        for (int64_t i = c.ptr[d]; i < c.ptr[d + 1]; ++i) ++lenL[c.w[i]];
      }
  const bool split = suff_split != 0 && want.size() >= 2 && late_n > 0 &&
                     (suff_split == 2 || !((double)late_sum > 0.6 * (double)std::max<int64_t>(1, nnz)));
  CHECK(o.split == split);
  if (split) {
    for (int64_t w = 0; w < V; ++w) lenE[w] = wl[w] - lenL[w];
    suff("suff_order_early", lenE, o.suff_counts[1]);
    suff("suff_order_late", lenL, o.suff_counts[2]);
    const uint8_t* m = sec<uint8_t>(o, buf, "late_mask");
    CHECK(m && std::equal(mask.begin(), mask.end(), m));
    CHECK(o.n_late == late_sum && o.n_early == nnz - late_sum && o.late_docs == late_n);
  }

  // team8 tables
  const bool has8 = !want.empty() && want[0].first == 3;
  CHECK(o.csum == has8);
  if (has8) {
    const auto& b = want[0].second;
    int64_t tiles = 0;
    for (int32_t d : b)
      if (d >= 0) tiles += (len[d] + 63) / 64;
    const bool staged = stage_cap > 0 && !((double)(tiles * 64 * KS * 8) > stage_cap);
    CHECK(o.staged == staged);
    const double* cs = sec<double>(o, buf, "csum");
    const int32_t* te = staged ? sec<int32_t>(o, buf, "stage_tile_ent") : nullptr;
    const int32_t* tc = staged ? sec<int32_t>(o, buf, "stage_tile_cnt") : nullptr;
    const int64_t* so = staged ? sec<int64_t>(o, buf, "stage_off") : nullptr;
    if (staged) CHECK(o.n_tiles == tiles);
    int64_t nt = 0;
    for (size_t i = 0; i < b.size(); ++i) {
      const int32_t d = b[i];
      std::vector<double> row(32, 0.0);
      if (d >= 0) {
        const int64_t n = len[d], W = (n + U - 1) / U;
        for (int64_t e = 0; e < n; ++e) row[e / W] += (double)c.cnt[c.ptr[d] + e];   // (small integers: exact)
        if (staged) {
          CHECK(so[i] == nt * (KS / 2) * 64);
          for (int64_t j = 0; j * 64 < n; ++j, ++nt)
            CHECK(te[nt] == c.ptr[d] + 64 * j && tc[nt] == std::min<int64_t>(64, n - 64 * j));
        }
      } else if (staged) {
        CHECK(so[i] == 0);
      }
      for (int j = 0; j < 32; ++j) CHECK(cs[i * 32 + j] == row[j]);
    }
    CHECK(o.defer == split);
    if (o.defer) {
      const int32_t* s0 = sec<int32_t>(o, buf, "et_s0");
      const int32_t* ew = sec<int32_t>(o, buf, "et_w");
      const int32_t* eb = sec<int32_t>(o, buf, "et_base");
      std::vector<int32_t> base((size_t)D, -1);
      for (size_t i = 0; i < b.size(); ++i)
        if (b[i] >= 0 && len[b[i]] > 0) base[b[i]] = (int32_t)(i * 32);
      for (int64_t d = 0; d < D; ++d) {
        CHECK(eb[d] == base[d]);
        if (base[d] >= 0) CHECK(s0[d] == c.ptr[d] && ew[d] == (len[d] + U - 1) / U);
      }
    }
  } else {
    CHECK(!o.staged && !o.defer);
  }
}

int main() {
  std::vector<Case> cases;
  {
    std::vector<int64_t> l = {0, 0, 0, 0, 1, 8, 9, 64, 65, 256, 257, 2048, 2049, 2112, 4097, 9, 2049, 65};
    for (int i = 0; i < 1100; ++i) l.push_back(3 + rnd() % 6);
    l.push_back(0);
    l.push_back(0);
    cases.push_back(make(l, 5000, (int64_t)1 << 31));
  }
  for (int n8 : {0, 1, 8, 9}) {
    std::vector<int64_t> l;
    for (int i = 0; i < 40; ++i) l.push_back(rnd() % 300);
    for (int i = 0; i < n8; ++i) l.insert(l.begin() + rnd() % l.size(), 2049 + i / 2);
    cases.push_back(make(l, 2400));
  }
  {
    std::vector<int64_t> l = {2100};
    for (int i = 0; i < 100; ++i) l.push_back(1 + rnd() % 11);
    cases.push_back(make(l, 2300));
  }
  cases.push_back(make({70, 80, 90, 100, 70}, 300));
  cases.push_back(make({0, 0, 0}, 5));
  cases.push_back(make({}, 3));
  const int ksu[3][2] = {{20, 32}, {8, 8}, {32, 32}};
  for (const Case& c : cases)
    for (const auto& s : ksu)
      for (int mode : {0, 1, 2}) {
        run(c, s[0], s[1], mode, 4.0 * (1 << 30));
        run(c, s[0], s[1], mode, 2049.0 / 64 * 64 * s[0] * 8);   // below every team8 plan's bytes but a tiny one's
      }
  std::printf("engine_plan_check: %d plans, %d failures\n", g_case, g_fail);
  return g_fail ? 1 : 0;
}
