// rtla_audit.h -- the passes over rows outside the search: what their kernels
// (rtla_kaudit.hip, rtla_kpred.hip) and their host replays (rtla_audit.cpp,
// rtla_predhost.cpp) share, so both give the same masks, counts and reported
// violation: the violation key, the counters, the host's enumeration of a
// row's successors, and the invariant audit of one row.
//
// A pass evaluates each row itself (one evaluated state per row) or every
// enabled successor of each row, in- and out-of-model; a successor with a
// spec / row-capacity error raises the level kernels' flag and the call fails.
// Per row the result is a mask (successors: the OR over them); per mask bit the
// evaluated states that set it are counted.  The reported violation is the
// least key over all evaluated states.
//
// The invariant audit (rtla_check_batch / rtla_check_replay /
// rtla_check_frontier) takes a copy of the layout with inv_mask replaced by the
// set it was asked for and evaluates check_invariants_v: on the row, or on
// parent + delta -- the evaluation the level kernels and the random walks run.
#pragma once
#include "rtla_device.h"

namespace rtla {

constexpr int AUDIT_COUNTS = 8;  // rtla_audit_stats.counts: mask bits counted
constexpr uint64_t AUDIT_NO_VIOLATION = ~0ull;

// Violation key, least first: row index << 25 | instance << 9 | in_model << 8 |
// mask (a pass over the rows themselves: instance 0, in_model 1).  The low nine
// bits are a function of (row, instance), so the order is theirs.  (A layout
// has a few hundred instances: no key is AUDIT_NO_VIOLATION.)
RTLA_HD uint64_t audit_key(uint64_t index, int inst, int in_model, int mask) {
  return index << 25 | (uint64_t)inst << 9 | (uint64_t)(in_model ? 256 : 0) | (uint64_t)(mask & 255);
}
RTLA_HD uint64_t audit_key_index(uint64_t key) { return key >> 25; }
RTLA_HD int audit_key_inst(uint64_t key) { return (int)(key >> 9 & 0xffff); }
RTLA_HD int audit_key_in_model(uint64_t key) { return (int)(key >> 8 & 1); }
RTLA_HD int audit_key_mask(uint64_t key) { return (int)(key & 255); }
static_assert(INV_ALL <= 255 && AUDIT_COUNTS == 8, "the key's mask field holds every counted bit");

// Device counters of one pass (the host's tally has the same shape).
struct AuditCounters {
  unsigned long long evaluated;
  unsigned long long viol_key;  // AUDIT_NO_VIOLATION, or the least audit_key (atomicMin)
  int flags, pad;
  unsigned long long counts[AUDIT_COUNTS];
};

// One evaluated state / step on the host: its bits counted, its key kept if it is the least.
static inline void audit_tally(AuditCounters& t, uint64_t index, int inst, int in_model, int bad) {
  if (!bad) return;
  for (int k = 0; k < AUDIT_COUNTS; k++) t.counts[k] += bad >> k & 1;
  const uint64_t key = audit_key(index, inst, in_model, bad);
  if (key < t.viol_key) t.viol_key = key;
}

// The enabled successors of `row` on the host, as the kernels' candidates
// (candidate_inst: instances ascend): f(inst, d) for each one without an error;
// an error sets its flag bit in `flags`.
template <int NS, class F>
static inline void for_each_successor(const Layout& L, const uint32_t* row, int& flags, F f) {
  const int nmsg = row_nmsg(L, row), ncand = L.fam[F_RECEIVE] + 3 * nmsg;
  DeltaT<NS ? NS : NMAX> d;
  for (int q = 0; q < ncand; q++) {
    const int inst = candidate_inst(L, q, nmsg);
    compute_delta<NS>(L, row, inst, d);
    if (!d.enabled) continue;
    if (d.err) {
      flags |= d.err == 1 ? FLAG_SPEC_ERROR : FLAG_ROW_OVERFLOW;
      continue;
    }
    f(inst, d);
  }
}

// The invariant audit of one row on the host, serially: its mask; tally into t (index: the row's number).
template <int NS>
static inline int audit_row_serial(const Layout& L, const uint32_t* row, uint64_t index, int succ, AuditCounters& t) {
  if (!succ) {
    const int bad = check_invariants_v<NS>(L, row, -1, 0u, 0u, 0, 0u);
    t.evaluated++;
    audit_tally(t, index, 0, 1, bad);
    return bad;
  }
  int all = 0;
  for_each_successor<NS>(L, row, t.flags, [&](int inst, const auto& d) {
    const int bad = check_invariants_v<NS>(L, row, d.srv, d.rec[0], d.rec[1], d.elec, d.erec[0]);
    t.evaluated++;
    audit_tally(t, index, inst, d.in_model, bad);
    all |= bad;
  });
  return all;
}

}  // namespace rtla
