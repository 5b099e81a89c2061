// rtla_predhost.cpp -- user-defined predicates: the rtla_pred_* ABI.  The
// compiler is rtla_pred.cpp (host only), the interpreter rtla_pred.h -- run
// here per row by rtla_pred_replay, and by the kernel of rtla_kpred.hip for
// rtla_pred_batch and rtla_pred_frontier, which are the batch and frontier
// passes of rtla_audit.cpp with that kernel.
#include "rtla_ctx.h"
#include "rtla_predc.h"
#include "rtla_step.h"

static int compile_abi(const rtla_cfg* c, const char* text, bool step, rtla_pred** out, char* err, size_t errcap) {
  if (err && errcap) err[0] = 0;
  if (!text || !out) return RTLA_E_ARG;
  *out = nullptr;
  CFG_LAYOUT(L, c);
  rtla_pred* p = new rtla_pred;
  std::string msg;
  if (!(step ? pred_compile_step : pred_compile)(L, text, strlen(text), p, &msg)) {
    delete p;
    if (err && errcap) snprintf(err, errcap, "%s", msg.c_str());
    return RTLA_E_ARG;
  }
  *out = p;
  return RTLA_OK;
}

extern "C" int rtla_pred_compile(const rtla_cfg* c, const char* text, rtla_pred** out, char* err, size_t errcap) {
  return compile_abi(c, text, false, out, err, errcap);
}

extern "C" int rtla_pred_compile_step(const rtla_cfg* c, const char* text, rtla_pred** out, char* err,
                                      size_t errcap) {
  return compile_abi(c, text, true, out, err, errcap);
}

extern "C" int rtla_pred_is_step(const rtla_pred* p) { return p ? (int)p->step : RTLA_E_ARG; }

extern "C" void rtla_pred_free(rtla_pred* p) { delete p; }

extern "C" int rtla_pred_count(const rtla_pred* p) { return p ? (int)p->names.size() : RTLA_E_ARG; }

extern "C" int rtla_pred_name(const rtla_pred* p, int k, char* buf, size_t cap) {
  if (!p || !buf || k < 0 || k >= (int)p->names.size() || p->names[(size_t)k].size() + 1 > cap) return RTLA_E_ARG;
  memcpy(buf, p->names[(size_t)k].c_str(), p->names[(size_t)k].size() + 1);
  return (int)p->names[(size_t)k].size();
}

// The layout of *c, if `p` was compiled for it and is of the kind the call takes (step: an action set).
static int pred_layout(const rtla_cfg* c, const rtla_pred* p, bool step, Layout* L) {
  if (int r = layout_from_cfg(c, L)) return r;
  return p && p->step == step && pred_bound_to(p, *L) ? RTLA_OK : RTLA_E_ARG;
}

extern "C" int rtla_pred_replay(const rtla_cfg* c, const rtla_pred* p, const uint32_t* rows, size_t n, int threads,
                                int32_t* masks, uint64_t* counts) {
  Layout L;
  if (int r = pred_layout(c, p, false, &L)) return r;
  if (threads < 0 || !masks || (n && !rows)) return RTLA_E_ARG;
  return replay_rows(n, threads, masks, counts, nullptr, [&](size_t k, AuditCounters& tl) {
    int file[PRED_FILE];
    int err = 0;
    const int bad = pred_eval<0>(L, rows + k * (size_t)L.W, p->code.data(), file, &err);
    if (err) {
      tl.flags |= FLAG_SPEC_ERROR;
      return 0;
    }
    audit_tally(tl, k, 0, 1, bad);
    return bad;
  });
}

extern "C" int rtla_pred_step_replay(const rtla_cfg* c, const rtla_pred* p, const uint32_t* rows, size_t n,
                                     int threads, int32_t* masks, uint64_t* counts, uint64_t* evaluated) {
  Layout L;
  if (int r = pred_layout(c, p, true, &L)) return r;
  if (threads < 0 || !masks || (n && !rows)) return RTLA_E_ARG;
  return replay_rows(n, threads, masks, counts, evaluated, [&](size_t k, AuditCounters& tl) {
    return dispatch_n(L, [&](auto ns) {
      return step_row_serial<decltype(ns)::value>(L, rows + k * (size_t)L.W, k, p->code.data(), tl);
    });
  });
}

// The kernel of a set's kind (rtla_kpred.hip).
static auto pred_launcher(const rtla_pred* p) { return p->step ? launch_pred_step : launch_pred; }

static int pred_batch(const rtla_cfg* c, const rtla_pred* p, bool step, const uint32_t* rows, size_t n,
                      int32_t* masks, uint64_t* counts, uint64_t* evaluated) {
  Layout L;
  if (int r = pred_layout(c, p, step, &L)) return r;
  if (!masks || (n && !rows)) return RTLA_E_ARG;
  uint32_t* d_prog = nullptr;
  const size_t bytes = p->code.size() * sizeof(uint32_t);
  HIPCHK(hipMalloc(&d_prog, bytes));
  int rc = RTLA_E_HIP;
  if (hipMemcpy(d_prog, p->code.data(), bytes, hipMemcpyHostToDevice) == hipSuccess)
    rc = audit_batch(L, rows, n, [&](const Ring& cur, uint64_t nr, int* m, AuditCounters* ctr, hipStream_t st) {
      return pred_launcher(p)(L, cur, nr, d_prog, (int)p->code.size(), m, ctr, st);
    }, masks, counts, evaluated);
  (void)hipFree(d_prog);
  return rc;
}

extern "C" int rtla_pred_batch(const rtla_cfg* c, const rtla_pred* p, const uint32_t* rows, size_t n, int32_t* masks,
                               uint64_t* counts) {
  return pred_batch(c, p, false, rows, n, masks, counts, nullptr);
}

extern "C" int rtla_pred_step_batch(const rtla_cfg* c, const rtla_pred* p, const uint32_t* rows, size_t n,
                                    int32_t* masks, uint64_t* counts, uint64_t* evaluated) {
  return pred_batch(c, p, true, rows, n, masks, counts, evaluated);
}

static int pred_frontier(rtla_ctx* x, const rtla_pred* p, bool step, rtla_audit_stats* out) {
  if (!x || !p) return RTLA_E_ARG;
  if (!frontier_pass_ok(x)) return RTLA_E_STATE;
  const Layout L = x->L;
  if (p->step != step || !pred_bound_to(p, L)) return RTLA_E_ARG;
  HIPCHK(hipSetDevice(x->device));
  AuditState& a = x->audit;
  if (!a.prog) HIPCHK(hipMalloc((void**)&a.prog, PRED_MAX_WORDS * sizeof(uint32_t)));
  HIPCHK(hipMemcpyAsync(a.prog, p->code.data(), p->code.size() * sizeof(uint32_t), hipMemcpyHostToDevice, x->stream));
  return audit_frontier(x, step, [&](const Ring& cur, uint64_t n, int* m, AuditCounters* ctr, hipStream_t st) {
    return pred_launcher(p)(L, cur, n, a.prog, (int)p->code.size(), m, ctr, st);
  }, out);
}

extern "C" int rtla_pred_frontier(rtla_ctx* x, const rtla_pred* p, rtla_audit_stats* out) {
  return pred_frontier(x, p, false, out);
}

extern "C" int rtla_pred_step_frontier(rtla_ctx* x, const rtla_pred* p, rtla_audit_stats* out) {
  return pred_frontier(x, p, true, out);
}
