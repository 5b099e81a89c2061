// rtla_step.h -- action properties on the host: each enabled successor of a row
// (for_each_successor, rtla_audit.h) materialised and the action program run on
// (row, successor).  The kernel k_pred_step (rtla_kpred.hip) computes the same
// masks, counts and key.  Semantics: DESIGN.md section 14.
#pragma once
#include "rtla_audit.h"
#include "rtla_pred.h"

namespace rtla {

// t is s when their 128-bit fingerprints (row words 0..3) are equal: the seen set's identity.
template <class P, class Q>
RTLA_HD bool step_stutters(P s, Q t) {
  return s[0] == t[0] && s[1] == t[1] && s[2] == t[2] && s[3] == t[3];
}

// One row on the host, serially: the OR of its steps' false-definition masks; tally into t.
template <int NS>
static inline int step_row_serial(const Layout& L, const uint32_t* row, uint64_t index, const uint32_t* prog,
                                  AuditCounters& t) {
  uint32_t pall[33], child[WMAX];
  int file[PRED_FILE];
  const FP pfp = fp_add(row_fp(row), alllogs_delta<NS>(L, row, pall));
  int all = 0;
  for_each_successor<NS>(L, row, t.flags, [&](int inst, const auto& d) {
    materialize<NS>(L, row, d, pall, fp_add(pfp, delta_fp<NS>(L, row, d)), child);
    t.evaluated++;
    int err = 0;
    int bad = pred_eval_rows<NS, true>(L, row, (const uint32_t*)child, prog, file, &err);  // evaluated first, as [A]_vars
    if (err) {
      t.flags |= FLAG_SPEC_ERROR;
      return;
    }
    if (step_stutters(row, child)) bad = 0;
    audit_tally(t, index, inst, d.in_model, bad);
    all |= bad;
  });
  return all;
}

}  // namespace rtla
