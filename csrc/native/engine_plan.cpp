#include "engine_plan.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <numeric>
#include <stdexcept>
#include <thread>

namespace onin {

namespace {

constexpr int64_t kAlign = 256;
inline int64_t align_up(int64_t x) { return (x + kAlign - 1) / kAlign * kAlign; }
inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

struct Arena {
  char* base;
  int64_t cap;
  EnginePlanOut* out;
  template <class T>
  T* take(const std::string& name, int64_t count) {
    const int64_t off = align_up(out->bytes), bytes = count * (int64_t)sizeof(T);
    if (count < 0 || off + bytes > cap) throw std::length_error("engine_plan: buffer too small at section " + name);
    out->bytes = off + bytes;
    out->sections.push_back({name, off, count, (int)sizeof(T)});
    return reinterpret_cast<T*>(base + off);
  }
};

// np.argsort(-key, kind="stable") of non-negative keys: a counting sort (a comparison sort when the largest
// key would make the count table much larger than the input)
void order_desc_stable(const int64_t* key, int64_t n, int32_t* out) {
  if (n <= 0) return;
  const int64_t mx = *std::max_element(key, key + n);
  if (mx <= 16 * n + (1 << 20)) {
    std::vector<int32_t> pos((size_t)mx + 1, 0);
    for (int64_t i = 0; i < n; ++i) ++pos[(size_t)key[i]];
    int32_t run = 0;
    for (int64_t l = mx; l >= 0; --l) {
      const int32_t c = pos[(size_t)l];
      pos[(size_t)l] = run;
      run += c;
    }
    for (int64_t i = 0; i < n; ++i) out[pos[(size_t)key[i]]++] = (int32_t)i;
  } else {
    std::iota(out, out + n, 0);
    std::stable_sort(out, out + n, [key](int32_t a, int32_t b) { return key[a] > key[b]; });
  }
}

// GSPlan.isolate_longest(o, m, xcds)
std::vector<int32_t> isolate_longest(const std::vector<int32_t>& o, int m, int xcds) {
  const size_t nh = std::min<size_t>((size_t)std::max(m, 0), o.size());
  size_t h = 0, r = nh;
  std::vector<int32_t> out;
  out.reserve(o.size() + o.size() / 4 + 8);
  for (int64_t b = 0; h < nh || r < o.size(); ++b) {
    if (b % xcds < m)
      out.push_back(h < nh ? o[h++] : -1);
    else
      out.push_back(r < o.size() ? o[r++] : -1);
  }
  while (!out.empty() && out.back() == -1) out.pop_back();
  return out;
}

// SuffPlan: the stable descending order of the word lengths and its heavy / medium / light counts
void suff_plan(const std::vector<int64_t>& wl, int64_t heavy, int64_t light, int32_t* order, int64_t counts[3]) {
  order_desc_stable(wl.data(), (int64_t)wl.size(), order);
  counts[0] = counts[1] = counts[2] = 0;
  for (int64_t l : wl) ++counts[l > heavy ? 0 : (l > light ? 1 : 2)];
}

// a worker thread that is joined when its scope ends, an exception's unwinding included
struct Joiner {
  std::thread t;
  void join() {
    if (t.joinable()) t.join();
  }
  ~Joiner() { join(); }
};

}  // namespace

int64_t engine_plan_bound(int64_t D, int64_t V, int64_t nnz, int64_t team8_lo, int xcds) {
  const int64_t n8 = team8_lo >= 1 ? std::min(D, nnz / (team8_lo + 1) + 1) : D;
  const int64_t items8 = (n8 + 1) * std::max(xcds, 1);
  int64_t b = 4 * (D + 1) + 8 * nnz + 4 * (V + 1);   // doc_ptr, word_idx, counts, word_ptr
  b += 4 * (D + items8) + D + 12 * V;                // bucket orders, late mask, three suff orders
  b += 8 * (nnz / 64 + n8 + 1) + 8 * items8;         // staged tiles, stage offsets
  b += 8 * 64 * items8 + 12 * D;                     // chunk sums (<= 64 rows per item), et tables
  return b + 40 * kAlign;
}

EnginePlanOut engine_plan(const EnginePlanIn& in, void* buf, int64_t cap) {
  const int64_t D = in.D, V = in.V, nnz = in.nnz;
  const int U = in.U, umax = in.umax;
  if (D < 0 || V < 0 || nnz < 0 || nnz >= INT32_MAX - 1 || D >= INT32_MAX - 1 || V >= INT32_MAX - 1)
    throw std::invalid_argument("engine_plan: sizes outside int32");
  if (in.KS < 2 || in.KS > 32 || in.KS % 2 || U < 1 || U > umax || umax > 64 || in.xcds < 1 || in.iso_m >= in.xcds)
    throw std::invalid_argument("engine_plan: KS / U / umax / xcds outside the planned path");
  if (!in.doc_ptr || in.doc_ptr[0] != 0 || in.doc_ptr[D] != nnz)
    throw std::invalid_argument("engine_plan: inconsistent doc_ptr");
  for (int64_t d = 0; d < D; ++d)
    if (in.doc_ptr[d + 1] < in.doc_ptr[d]) throw std::invalid_argument("engine_plan: doc_ptr not monotone");
  if (!buf || (reinterpret_cast<uintptr_t>(buf) % kAlign) != 0)
    throw std::invalid_argument("engine_plan: the buffer must be 256-byte aligned");

  EnginePlanOut out;
  Arena ar{static_cast<char*>(buf), cap, &out};
  auto t_prev = std::chrono::steady_clock::now();
  auto phase = [&](const char* name) {   // microseconds since the previous mark (scripts/setup_profile.py)
    const auto t = std::chrono::steady_clock::now();
    out.phase_us.emplace_back(name, std::chrono::duration<double, std::micro>(t - t_prev).count());
    t_prev = t;
  };

  // ---- corpus arrays: narrowed copies + the word histogram, one threaded pass over the entries
  int32_t* dp32 = ar.take<int32_t>("doc_ptr", D + 1);
  int32_t* widx = ar.take<int32_t>("word_idx", nnz);
  float* cnt32 = ar.take<float>("counts", nnz);
  int32_t* wptr = ar.take<int32_t>("word_ptr", V + 1);
  for (int64_t d = 0; d <= D; ++d) dp32[d] = (int32_t)in.doc_ptr[d];
  out.doc_len.resize((size_t)D);
  for (int64_t d = 0; d < D; ++d) out.doc_len[(size_t)d] = in.doc_ptr[d + 1] - in.doc_ptr[d];
  const int T = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)in.threads, 16, nnz / 400000 + 1}));
  std::vector<std::vector<int32_t>> hist((size_t)T);
  std::atomic<bool> bad{false};
  auto pass = [&](int t) {
    hist[(size_t)t].assign((size_t)V, 0);
    int32_t* h = hist[(size_t)t].data();
    const int64_t a = nnz * t / T, b = nnz * (t + 1) / T;
    if (b > a) std::memcpy(widx + a, in.word_idx + a, (size_t)(b - a) * sizeof(int32_t));
    for (int64_t i = a; i < b; ++i) cnt32[i] = (float)in.counts[i];
    bool oob = false;
    for (int64_t i = a; i < b; ++i) {
      const uint32_t w = (uint32_t)in.word_idx[i];
      if (w >= (uint32_t)V) {
        oob = true;
        continue;
      }
      ++h[w];
    }
    if (oob) bad.store(true);
  };
  {
    std::vector<std::thread> th;
    for (int t = 1; t < T; ++t) th.emplace_back(pass, t);
    pass(0);
    for (auto& x : th) x.join();
  }
  phase("entries");
  if (bad.load()) throw std::invalid_argument("engine_plan: word index out of range");
  out.word_len.assign((size_t)V, 0);
  for (int t = 0; t < T; ++t) {
    const int32_t* h = hist[(size_t)t].data();
    for (int64_t w = 0; w < V; ++w) out.word_len[(size_t)w] += h[w];
  }
  {
    int64_t run = 0;
    for (int64_t w = 0; w < V; ++w) {
      wptr[w] = (int32_t)run;
      run += out.word_len[(size_t)w];
    }
    wptr[V] = (int32_t)run;
  }

  phase("word_ptr");
  // the whole-vocabulary suff-stats plan on a second thread while this one plans the length buckets
  const bool par = in.threads > 1 && V >= 4096;
  int32_t* so_full = ar.take<int32_t>("suff_order", V);
  Joiner j_full;
  auto full_plan = [&] { suff_plan(out.word_len, in.heavy, in.light, so_full, out.suff_counts[0]); };
  if (par) j_full.t = std::thread(full_plan);

  // ---- length buckets (GSPlan): the stable descending order filtered per edge, then the tiny bucket
  std::vector<int32_t> order((size_t)D);
  order_desc_stable(out.doc_len.data(), D, order.data());
  // (the lengths along the order fall monotonically: every edge's documents are one contiguous run of it)
  std::vector<int64_t> Ls((size_t)D);
  for (int64_t i = 0; i < D; ++i) Ls[(size_t)i] = out.doc_len[(size_t)order[(size_t)i]];
  auto first_le = [&](int64_t x) {   // first position whose length is <= x
    return (int64_t)(std::partition_point(Ls.begin(), Ls.end(), [x](int64_t l) { return l > x; }) - Ls.begin());
  };
  std::vector<std::vector<int32_t>> bo;
  std::vector<int> bvar;
  auto bucket = [&](int var, int64_t i0, int64_t i1) {   // positions [i0, i1) of the order
    if (i1 <= i0) return;
    std::vector<int32_t> o(order.begin() + i0, order.begin() + i1);
    if (var == in.team8_variant && in.iso_m > 0) o = isolate_longest(o, std::min(in.iso_m, 8), in.xcds);
    bo.push_back(std::move(o));
    bvar.push_back(var);
  };
  for (const auto& e : in.edges)   // lo < L (<= hi when hi >= 0)
    bucket(e.variant, e.hi < 0 ? 0 : first_le(e.hi), first_le(e.lo < 0 ? in.tiny : e.lo));
  bucket(in.tiny_variant, first_le(in.tiny), D);
  for (size_t i = 0; i < bo.size(); ++i) {
    int32_t* p = ar.take<int32_t>("order_" + std::to_string(i), (int64_t)bo[i].size());
    std::memcpy(p, bo[i].data(), bo[i].size() * sizeof(int32_t));
    out.buckets.push_back({bvar[i], out.sections.back().offset, (int64_t)bo[i].size()});
  }

  phase("buckets");
  // ---- suff-stats plans: the full one; early / late when the first (longest-document) bucket can overlap
  if (par)
    j_full.join();
  else
    full_plan();
  if (in.suff_split != 0 && bo.size() >= 2) {
    int64_t late_n = 0, late_sum = 0;
    for (int32_t d : bo[0])
      if (d >= 0) {
        ++late_n;
        late_sum += out.doc_len[(size_t)d];
      }
    const bool force = in.suff_split == 2;
    if (late_n > 0 && (force || !((double)late_sum > in.late_share * (double)std::max<int64_t>(1, nnz)))) {
      out.split = true;
      out.late_docs = late_n;
      uint8_t* mask = ar.take<uint8_t>("late_mask", D);
      std::memset(mask, 0, (size_t)D);
      std::vector<int64_t> lenL((size_t)V, 0), lenE((size_t)V);
      for (int32_t d : bo[0]) {
        if (d < 0) continue;
        mask[d] = 1;
        for (int64_t i = in.doc_ptr[d]; i < in.doc_ptr[d + 1]; ++i) ++lenL[(size_t)in.word_idx[i]];
      }
      for (int64_t w = 0; w < V; ++w) lenE[(size_t)w] = out.word_len[(size_t)w] - lenL[(size_t)w];
      out.n_late = late_sum;
      out.n_early = nnz - late_sum;
      int32_t* so_e = ar.take<int32_t>("suff_order_early", V);
      int32_t* so_l = ar.take<int32_t>("suff_order_late", V);
      Joiner j_early;
      auto early_plan = [&] { suff_plan(lenE, in.heavy, in.light, so_e, out.suff_counts[1]); };
      if (par) j_early.t = std::thread(early_plan);
      suff_plan(lenL, in.heavy, in.light, so_l, out.suff_counts[2]);
      if (par)
        j_early.join();
      else
        early_plan();
    }
  }

  phase("suff_plans");
  // ---- per-document tables of the team8 bucket: staged-row tiles (GSStage), chunk sums (gs_chunk_sums)
  int b8 = -1;
  for (size_t i = 0; i < bo.size() && b8 < 0; ++i)
    if (bvar[i] == in.team8_variant) b8 = (int)i;
  if (b8 >= 0) {
    const auto& o = bo[(size_t)b8];
    const int64_t n_items = (int64_t)o.size();
    int64_t tiles = 0;
    for (int32_t d : o)
      if (d >= 0) tiles += ceil_div(out.doc_len[(size_t)d], 64);
    const int64_t need = tiles * 64 * in.KS * 8;
    if (in.stage_cap > 0 && !((double)need > in.stage_cap)) {
      out.staged = true;
      out.n_tiles = tiles;
      int32_t* te = ar.take<int32_t>("stage_tile_ent", tiles);
      int32_t* tc = ar.take<int32_t>("stage_tile_cnt", tiles);
      int64_t* so = ar.take<int64_t>("stage_off", n_items);
      const int64_t per = (in.KS / 2) * 64;
      int64_t nt = 0;
      for (int64_t i = 0; i < n_items; ++i) {
        so[i] = 0;
        const int32_t d = o[(size_t)i];
        if (d < 0) continue;
        const int64_t s0 = in.doc_ptr[d], n = out.doc_len[(size_t)d], Tn = ceil_div(n, 64);
        so[i] = nt * per;
        for (int64_t j = 0; j < Tn; ++j) {
          te[nt + j] = (int32_t)(s0 + 64 * j);
          tc[nt + j] = (int32_t)std::min<int64_t>(64, n - 64 * j);
        }
        nt += Tn;
      }
    }
    out.csum = true;
    double* cs = ar.take<double>("csum", n_items * umax);
    std::fill(cs, cs + n_items * umax, 0.0);
    for (int64_t i = 0; i < n_items; ++i) {
      const int32_t d = o[(size_t)i];
      if (d < 0) continue;
      const int64_t s0 = in.doc_ptr[d], n = out.doc_len[(size_t)d];
      if (n <= 0) continue;
      const int64_t W = ceil_div(n, U), nch = ceil_div(n, W);
      for (int64_t j = 0; j < nch; ++j) {
        int64_t s = 0;   // integer sums: exact, as the int64 reduceat of the Python planner
        for (int64_t e = s0 + j * W, e1 = std::min(s0 + (j + 1) * W, s0 + n); e < e1; ++e) s += in.counts[e];
        cs[i * umax + j] = (double)s;
      }
    }
  }

  phase("team8_tables");
  // ---- deferred final pass: per-document tables of the late (team8) bucket behind et_row
  if (out.split && in.defer_final && bvar[0] == in.team8_variant && U <= umax) {
    const auto& o = bo[0];
    if ((int64_t)o.size() * umax >= INT32_MAX) throw std::invalid_argument("engine_plan: et rows exceed int32");
    out.defer = true;
    int32_t* es0 = ar.take<int32_t>("et_s0", D);
    int32_t* ew = ar.take<int32_t>("et_w", D);
    int32_t* eb = ar.take<int32_t>("et_base", D);
    for (int64_t d = 0; d < D; ++d) {
      es0[d] = 0;
      ew[d] = 1;
      eb[d] = -1;
    }
    for (size_t i = 0; i < o.size(); ++i) {
      const int32_t d = o[i];
      if (d < 0 || out.doc_len[(size_t)d] <= 0) continue;
      es0[d] = (int32_t)in.doc_ptr[d];
      ew[d] = (int32_t)ceil_div(out.doc_len[(size_t)d], U);
      eb[d] = (int32_t)((int64_t)i * umax);
    }
  }
  phase("et_tables");
  return out;
}

}  // namespace onin
