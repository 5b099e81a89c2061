// rtla_step.h -- action properties on the host: one row's enabled successors
// enumerated as the audit's successor mode does (audit_row_serial, rtla_audit.h),
// each materialised and the action program run on (row, successor).  The kernel
// k_pred_step (rtla_kpred.hip) computes the same masks, counts and key.
// Semantics: DESIGN.md section 14.
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
  constexpr int NR = NS ? NS : NMAX;
  uint32_t pall[33], child[WMAX];
  int file[PRED_FILE];
  const FP pfp = fp_add(row_fp(row), alllogs_delta<NS>(L, row, pall));
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
    materialize<NS>(L, row, d, pall, fp_add(pfp, delta_fp<NS>(L, row, d)), child);
    t.evaluated++;
    int err = 0;
    int bad = pred_eval_rows<NS, true>(L, row, (const uint32_t*)child, prog, file, &err);  // evaluated first, as [A]_vars
    if (err) {
      t.flags |= FLAG_SPEC_ERROR;
      continue;
    }
    if (step_stutters(row, child)) bad = 0;
    if (!bad) continue;
    for (int k = 0; k < AUDIT_COUNTS; k++) t.counts[k] += bad >> k & 1;
    const uint64_t key = step_key(index, inst, d.in_model, bad);
    if (key < t.viol_key) t.viol_key = key;
    all |= bad;
  }
  return all;
}

}  // namespace rtla
