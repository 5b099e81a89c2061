// rtla_audit.cpp -- passes over rows outside the search (semantics:
// rtla_audit.h): audit_batch runs a pass's kernel over host rows staged into a
// device buffer, audit_frontier over the frontier where it lies.  The
// invariant audit is here too: rtla_check_batch and rtla_check_frontier are
// those two with the audit kernels (rtla_kaudit.hip); rtla_check_replay
// computes the same on the host (audit_row_serial), with no GPU.
#include "rtla_audit.h"
#include "rtla_ctx.h"

static bool audit_args_ok(int32_t inv_mask, int32_t succ) {
  return inv_mask >= 0 && inv_mask <= INV_ALL && (succ == 0 || succ == 1);
}

AuditCounters audit_zero() {
  AuditCounters h;
  memset(&h, 0, sizeof h);
  h.viol_key = AUDIT_NO_VIOLATION;
  return h;
}

static void audit_counts_out(const AuditCounters& h, uint64_t* counts) {
  if (!counts) return;
  for (int k = 0; k < AUDIT_COUNTS; k++) counts[k] = h.counts[k];
}

extern "C" int rtla_check_replay(const rtla_cfg* c, const uint32_t* rows, size_t n, int32_t inv_mask, int32_t succ,
                                 int threads, int32_t* masks, uint64_t* counts) {
  CFG_LAYOUT(L, c);
  if (!audit_args_ok(inv_mask, succ) || threads < 0 || !masks || (n && !rows)) return RTLA_E_ARG;
  L.inv_mask = inv_mask;
  return replay_rows(n, threads, masks, counts, nullptr, [&](size_t k, AuditCounters& tl) {
    return dispatch_n(L, [&](auto ns) {
      return audit_row_serial<decltype(ns)::value>(L, rows + k * (size_t)L.W, k, succ, tl);
    });
  });
}

// Stateless, like rtla_expand_batch: the rows are staged into a device buffer
// of their own (test-sized inputs).
int audit_batch(const Layout& L, const uint32_t* rows, size_t n, const AuditLaunch& launch, int32_t* masks,
                uint64_t* counts, uint64_t* evaluated) {
  const uint64_t cap = round64(std::max<size_t>(n, 1));
  uint32_t* d_rows = nullptr;
  int* d_masks = nullptr;
  AuditCounters* d_ctr = nullptr;
  AuditCounters h = audit_zero();
  auto run = [&]() -> int {
    HIPCHK(hipMalloc(&d_rows, cap * L.W * 4));
    HIPCHK(hipMalloc(&d_masks, cap * sizeof(int)));
    HIPCHK(hipMalloc(&d_ctr, sizeof h));
    HIPCHK(hipMemcpy(d_rows, rows, n * (size_t)L.W * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_ctr, &h, sizeof h, hipMemcpyHostToDevice));
    HIPCHK(launch(Ring{d_rows, 0, cap}, n, d_masks, d_ctr, nullptr));
    HIPCHK(hipMemcpy(&h, d_ctr, sizeof h, hipMemcpyDeviceToHost));
    if (n) HIPCHK(hipMemcpy(masks, d_masks, n * sizeof(int), hipMemcpyDeviceToHost));
    return RTLA_OK;
  };
  const int rc = run();
  for (void* p : {(void*)d_rows, (void*)d_masks, (void*)d_ctr})
    if (p) (void)hipFree(p);
  if (rc) return rc;
  if (h.flags) {
    report_flags(h.flags);
    return flags_to_status(h.flags);
  }
  audit_counts_out(h, counts);
  if (evaluated) *evaluated = h.evaluated;
  return RTLA_OK;
}

extern "C" int rtla_check_batch(const rtla_cfg* c, const uint32_t* rows, size_t n, int32_t inv_mask, int32_t succ,
                                int32_t* masks, uint64_t* counts) {
  CFG_LAYOUT(L, c);
  if (!audit_args_ok(inv_mask, succ) || !masks || (n && !rows)) return RTLA_E_ARG;
  L.inv_mask = inv_mask;
  return audit_batch(L, rows, n, [&](const Ring& cur, uint64_t nr, int* m, AuditCounters* ctr, hipStream_t st) {
    return launch_audit(L, cur, nr, succ, m, ctr, st);
  }, masks, counts);
}

int audit_frontier(rtla_ctx* x, int succ, const AuditLaunch& launch, rtla_audit_stats* out) {
  if (!frontier_pass_ok(x)) return RTLA_E_STATE;
  HIPCHK(hipSetDevice(x->device));
  Shard& s = x->sh[0];
  AuditState& a = x->audit;
  a.viol = false;
  x->sim.viol = false;
  if (!a.ctr) HIPCHK(hipMalloc((void**)&a.ctr, sizeof(AuditCounters)));
  if (!a.ev0) HIPCHK(hipEventCreate(&a.ev0));
  if (!a.ev1) HIPCHK(hipEventCreate(&a.ev1));
  AuditCounters h = audit_zero();
  HIPCHK(hipMemcpyAsync(a.ctr, &h, sizeof h, hipMemcpyHostToDevice, x->stream));
  HIPCHK(hipEventRecord(a.ev0, x->stream));
  HIPCHK(launch(cur_ring(x, s), s.n_cur, nullptr, a.ctr, x->stream));
  HIPCHK(hipEventRecord(a.ev1, x->stream));
  HIPCHK(hipMemcpyAsync(&h, a.ctr, sizeof h, hipMemcpyDeviceToHost, x->stream));
  HIPCHK(hipStreamSynchronize(x->stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, a.ev0, a.ev1));
  int status = RTLA_OK;
  if (h.flags) {
    report_flags(h.flags);
    status = flags_to_status(h.flags);
  } else if (h.viol_key != AUDIT_NO_VIOLATION) {
    status = RTLA_VIOLATION;
    a.viol = true;
    a.start = s.cur_base + audit_key_index(h.viol_key);
    a.inst = succ ? audit_key_inst(h.viol_key) : -1;
    a.mask = audit_key_mask(h.viol_key);
    a.in_model = audit_key_in_model(h.viol_key);
  }
  if (out) {
    memset(out, 0, sizeof *out);
    out->audited = s.n_cur;
    out->evaluated = h.evaluated;
    static_assert(sizeof out->counts / sizeof out->counts[0] == AUDIT_COUNTS, "rtla_audit_stats.counts");
    audit_counts_out(h, out->counts);
    out->kernel_ms = ms;
    out->row_bytes = (uint64_t)x->L.W * 4;
    out->viol_index = ~0ull;
    out->viol_inst = -1;
    if (a.viol) {
      out->viol_index = a.start - s.cur_base;
      out->viol_inst = a.inst;
      out->viol_mask = a.mask;
      out->viol_in_model = a.in_model;
    }
    out->status = status;
    out->flags = h.flags;
  }
  return status;
}

extern "C" int rtla_check_frontier(rtla_ctx* x, int32_t inv_mask, int32_t succ, rtla_audit_stats* out) {
  if (!x) return RTLA_E_ARG;
  if (!frontier_pass_ok(x)) return RTLA_E_STATE;
  if (!audit_args_ok(inv_mask, succ)) return RTLA_E_ARG;
  Layout L = x->L;
  L.inv_mask = inv_mask;
  return audit_frontier(x, succ, [&](const Ring& cur, uint64_t n, int* m, AuditCounters* ctr, hipStream_t st) {
    return launch_audit(L, cur, n, succ, m, ctr, st);
  }, out);
}
