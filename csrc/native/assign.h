// --topic-match: the minimum-cost assignment of a square cost matrix (pipeline/common.py write_topic_match).
//
// The shortest-augmenting-path form of the Hungarian method (Jonker-Volgenant style, row and column potentials),
// O(n^3): the rows enter one at a time; a Dijkstra step over the reduced costs finds the free column that is
// cheapest to reach, the potentials move by the step's distance and the path is flipped.  Every scan runs over the
// columns in ascending order with strict comparisons, so equal costs go to the lower column and the same input bits
// give the same output.  A NaN cost counts as `nan_cost` (the callers pass a value above every real cost).
#pragma once
#include <cstdint>
#include <limits>
#include <vector>

namespace oni {

// cost: [n][n] row-major, every entry finite or NaN (the caller checks).  match[i] = the column of row i; the sum of cost[i][match[i]] is the least over all
// permutations.
inline void assign_min(const double* cost, int64_t n, double nan_cost, int64_t* match) {
  const double inf = std::numeric_limits<double>::infinity();
  auto at = [&](int64_t i, int64_t j) {
    const double c = cost[i * n + j];
    return c == c ? c : nan_cost;
  };
  // 1-based with the sentinel column 0, as the method is usually written
  std::vector<double> u(n + 1, 0.0), v(n + 1, 0.0), minv(n + 1);
  std::vector<int64_t> p(n + 1, 0), way(n + 1, 0);   // p[j]: the row matched to column j (0: free)
  std::vector<char> used(n + 1);
  for (int64_t i = 1; i <= n; ++i) {
    p[0] = i;
    int64_t j0 = 0;
    for (int64_t j = 0; j <= n; ++j) {
      minv[j] = inf;
      used[j] = 0;
    }
    do {
      used[j0] = 1;
      const int64_t i0 = p[j0];
      double delta = inf;
      int64_t j1 = 0;
      for (int64_t j = 1; j <= n; ++j) {
        if (used[j]) continue;
        const double cur = at(i0 - 1, j - 1) - u[i0] - v[j];
        if (cur < minv[j]) {
          minv[j] = cur;
          way[j] = j0;
        }
        if (minv[j] < delta) {
          delta = minv[j];
          j1 = j;
        }
      }
      for (int64_t j = 0; j <= n; ++j) {
        if (used[j]) {
          u[p[j]] += delta;
          v[j] -= delta;
        } else {
          minv[j] -= delta;
        }
      }
      j0 = j1;
    } while (p[j0] != 0);
    do {
      const int64_t j1 = way[j0];
      p[j0] = p[j1];
      j0 = j1;
    } while (j0);
  }
  for (int64_t j = 1; j <= n; ++j) match[p[j] - 1] = j - 1;
}

}  // namespace oni
