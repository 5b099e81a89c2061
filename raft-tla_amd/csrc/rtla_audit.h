// rtla_audit.h -- invariants evaluated outside the search (rtla_check_batch /
// rtla_check_replay / rtla_check_frontier): the definitions the kernels
// (rtla_kaudit.hip) and the host replay (rtla_audit.cpp) share, so both give
// the same masks, counts and reported violation.
//
// The audit takes a copy of the layout with inv_mask replaced by the set it
// was asked for, and evaluates check_invariants_v
//   * succ == 0: on each row itself (one evaluated state per row);
//   * succ == 1: on every enabled successor of each row, in- and out-of-model,
//     as parent + delta -- the evaluation the level kernels and the random
//     walks run; a successor with a spec / row-capacity error raises the level
//     kernels' flag and the call fails.
// Per row the result is the violated mask (succ: the OR over its successors);
// per invariant bit, the evaluated states that violate it are counted.  The
// reported violation is the least key over all evaluated states.
#pragma once
#include "rtla_device.h"

namespace rtla {

constexpr int AUDIT_COUNTS = 8;  // rtla_audit_stats.counts (INV_COUNT used)
constexpr uint64_t AUDIT_NO_VIOLATION = ~0ull;

// Violation key, least first: row index << 24 | instance << 8 | in_model << 5
// | violated mask (succ == 0: instance 0, in_model 1).  The low eight bits are
// a function of (row, instance), so the order is theirs.
RTLA_HD uint64_t audit_key(uint64_t index, int inst, int in_model, int mask) {
  return index << 24 | (uint64_t)inst << 8 | (uint64_t)(in_model ? 32 : 0) | (uint64_t)(mask & INV_ALL);
}
RTLA_HD uint64_t audit_key_index(uint64_t key) { return key >> 24; }
RTLA_HD int audit_key_inst(uint64_t key) { return (int)(key >> 8 & 0xffff); }
RTLA_HD int audit_key_in_model(uint64_t key) { return (int)(key >> 5 & 1); }
RTLA_HD int audit_key_mask(uint64_t key) { return (int)(key & INV_ALL); }
// The key of a predicate audit (rtla_kpred.hip; rows only, no instance): the low
// eight bits are the row's false definitions (rtla_audit_stats.counts has eight).
RTLA_HD uint64_t pred_key(uint64_t index, int mask) { return index << 24 | (uint64_t)(mask & 255); }
RTLA_HD int pred_key_mask(uint64_t key) { return (int)(key & 255); }
// The key of a step audit (k_pred_step): row index << 25 | instance << 9 | in_model << 8 |
// the step's false action definitions.  The low nine bits are a function of (row, instance).
RTLA_HD uint64_t step_key(uint64_t index, int inst, int in_model, int mask) {
  return index << 25 | (uint64_t)inst << 9 | (uint64_t)(in_model ? 256 : 0) | (uint64_t)(mask & 255);
}
RTLA_HD uint64_t step_key_index(uint64_t key) { return key >> 25; }
RTLA_HD int step_key_inst(uint64_t key) { return (int)(key >> 9 & 0xffff); }
RTLA_HD int step_key_in_model(uint64_t key) { return (int)(key >> 8 & 1); }
enum AuditKind { AUDIT_INVARIANTS = 0, AUDIT_PRED_STATE, AUDIT_PRED_STEP };  // which key an audit launch reports

// Device counters of one audit launch (the host's tally has the same shape).
struct AuditCounters {
  unsigned long long evaluated;
  unsigned long long viol_key;  // AUDIT_NO_VIOLATION, or the least audit_key (atomicMin)
  int flags, pad;
  unsigned long long counts[AUDIT_COUNTS];
};

// One row on the host, serially: its mask; tally into t (index: the row's number).
template <int NS>
static inline int audit_row_serial(const Layout& L, const uint32_t* row, uint64_t index, int succ, AuditCounters& t) {
  constexpr int NR = NS ? NS : NMAX;
  auto tally = [&](int bad, int inst, int in_model) {
    t.evaluated++;
    if (!bad) return;
    for (int k = 0; k < INV_COUNT; k++) t.counts[k] += bad >> k & 1;
    const uint64_t key = audit_key(index, inst, in_model, bad);
    if (key < t.viol_key) t.viol_key = key;
  };
  if (!succ) {
    const int bad = check_invariants_v<NS>(L, row, -1, 0u, 0u, 0, 0u);
    tally(bad, 0, 1);
    return bad;
  }
  const int fixed = L.fam[F_RECEIVE], nmsg = row_nmsg(L, row), ncand = fixed + 3 * nmsg;
  int all = 0;
  DeltaT<NR> d;
  for (int q = 0; q < ncand; q++) {  // the level kernels' candidates: instances ascend with q
    int inst = q;
    if (q >= fixed) {
      const int r = q - fixed, fam = r / nmsg;
      inst = fam_base(L, F_RECEIVE + fam) + (r - fam * nmsg);
    }
    compute_delta<NS>(L, row, inst, d);
    if (!d.enabled) continue;
    if (d.err) {
      t.flags |= d.err == 1 ? FLAG_SPEC_ERROR : FLAG_ROW_OVERFLOW;
      continue;
    }
    const int bad = check_invariants_v<NS>(L, row, d.srv, d.rec[0], d.rec[1], d.elec, d.erec[0]);
    tally(bad, inst, d.in_model);
    all |= bad;
  }
  return all;
}

}  // namespace rtla
