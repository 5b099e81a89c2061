// rtla_plan.h -- the level-end plans of the multi-shard driver (rehome,
// rebalance in rtla_host.cpp) as pure functions: no device, no context.
// Every rank computes them from the same reduced counts, so every rank gets
// the same plan.  Host only; tests/hostmodel.cpp compiles it with g++.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace rtla {

// Re-homing: a's export region b (cnt rows) -> dst's next level at [base, +cnt).
struct RehomeMove {
  int a, b, dst;
  uint64_t base, cnt;
};

// expm[a * G + b] = rows a exported for b (at most rows_cap move), room[k] =
// k's next-level room, n[k] = k's next-level states (updated).  A transfer b
// has no room for stays with a; false: one fits neither (the level is full).
inline bool plan_rehome(int G, uint64_t rows_cap, const uint64_t* expm, const uint64_t* room, std::vector<uint64_t>& n,
                        std::vector<RehomeMove>& mv) {
  bool full = false;
  for (int a = 0; a < G; a++)
    for (int b = 0; b < G; b++) {
      const uint64_t c = std::min(expm[a * G + b], rows_cap);
      if (!c) continue;
      if (n[b] + c <= room[b]) {
        mv.push_back({a, b, b, n[b], c});
        n[b] += c;
      } else if (n[a] + c <= room[a]) {
        mv.push_back({a, b, a, n[a], c});
        n[a] += c;
      } else {
        full = true;
      }
    }
  return !full;
}

// Re-balancing: a's states [first, +cnt) -> b's slots [base, +cnt).
struct RebalanceMove {
  int a, b;
  uint64_t first, base, cnt;
};

// The even split of n[k] next-level states is total / G each (the first
// total % G shards one more); shards above it send their LAST rows, in shard
// order, to those below it.  m = the counts after the moves.  No moves while
// the largest excess is within 1 % + 64 rows of the split.
inline std::vector<RebalanceMove> plan_rebalance(int G, const std::vector<uint64_t>& n, std::vector<uint64_t>& m) {
  uint64_t total = 0;
  for (int k = 0; k < G; k++) total += n[k];
  std::vector<uint64_t> tgt(G);
  uint64_t worst = 0;
  for (int k = 0; k < G; k++) {
    tgt[k] = total / G + ((uint64_t)k < total % G ? 1 : 0);
    if (n[k] > tgt[k]) worst = std::max(worst, n[k] - tgt[k]);
  }
  std::vector<RebalanceMove> mv;
  m = n;
  if (worst <= 64 + total / (100ull * G)) return mv;
  for (int a = 0, b = 0;;) {  // greedy, in shard order
    while (a < G && m[a] <= tgt[a]) a++;
    while (b < G && m[b] >= tgt[b]) b++;
    if (a >= G || b >= G) break;
    const uint64_t c = std::min(m[a] - tgt[a], tgt[b] - m[b]);
    mv.push_back({a, b, m[a] - c, m[b], c});
    m[a] -= c;
    m[b] += c;
  }
  return mv;
}

}  // namespace rtla
