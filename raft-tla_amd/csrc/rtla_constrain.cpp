// rtla_constrain.cpp -- user-defined CONSTRAINTs: rtla_pred_constrain prunes the
// level just produced by a compiled state set, on the GPU (kernels:
// rtla_kconstrain.hip); rtla_constrain_batch is the same pass on host rows laid
// into a ring of their own.
//
// Semantics.  TLC keeps a successor t only if t satisfies
// every CONSTRAINT.  A kept state is fingerprinted, counted as distinct and
// queued.  A state that fails is still checked against the invariants the first
// time it is met.  It is never counted as distinct and never expanded.  Initial
// states are filtered the same way.
//
// The built-in bounds already behave like this, through in_model in the level
// kernel.  The user constraint is applied as a pass over the level just produced,
// before anything reads that level as a frontier:
//
// 1. rtla_step / rtla_init / rtla_init_rows run unchanged.  The new level holds
//    every new in-model state.  The level kernel has already checked the built-in
//    invariants on all of them.  If user predicates are given, audit_predicates
//    runs next, over the unfiltered level.  TLC also checks invariants on states
//    it then discards.
// 2. rtla_pred_constrain(ctx, set, out) evaluates the state set on every row of
//    the current frontier.  Row g is kept if and only if every definition of the
//    set is TRUE on it.  Kept rows keep their relative order and become rows
//    0..kept-1 of the same level.  cur_start and cur_base do not change.  Their
//    parent records move with them, to parents[cur_base + 0..kept-1].  After the
//    call:
//      - n_cur = kept;
//      - distinct -= dropped.
//    The next level's parent records therefore start at cur_base + kept, as
//    level_setup already computes.  If kept == 0 the search is finished and the
//    call returns RTLA_DONE.
// 3. Action properties (audit_steps) then run over the kept rows only, and the
//    next rtla_step expands the kept rows only.
//
// The fingerprint set keeps the dropped states' keys.  That is deliberate and
// harmless.  A constraint is a function of the state.  A dropped state met again
// is "seen", generates nothing and counts nothing.  Its invariants were checked
// the first time.  Counts therefore equal TLC's.
//
// These totals are all taken after the drop: generated, per-level new,
// distinct_total, the depth, the level digests.
//
// Two things are not corrected.  The set's load is the pre-drop one.
// rtla_coverage's per-action distinct counts also still include dropped states,
// because a parent record does not carry the Receive sub-action.
//
// An evaluation error on any row fails the call with RTLA_E_SPEC.  The frontier,
// parent records and totals are then exactly as before the call: everything is
// evaluated first, rows move afterwards.  A HIP failure while rows are moving
// ends the search (finished), as HIP failures do elsewhere.
//
// The preconditions are frontier_pass_ok's: one shard, one process, rows kept,
// no pending violation, a non-empty frontier.  A step set, or a set compiled for
// another layout, gives RTLA_E_ARG.  SYMMETRY is allowed.  The constraint must be
// symmetric under server permutation, as TLC also requires.
//
// A checkpoint taken after the call holds the compacted level.  A recovered
// search continued with the same set gives the same counts.
#include "rtla_constrain.h"
#include "rtla_ctx.h"
#include "rtla_predc.h"

void constrain_free(ConstrainBufs& b) {
  for (void* p : {(void*)b.stage, (void*)b.stage_par, (void*)b.masks, (void*)b.keep, (void*)b.offs, (void*)b.tot,
                  (void*)b.ctr, (void*)b.prog})
    if (p) (void)hipFree(p);
  for (hipEvent_t e : b.ev)
    if (e) (void)hipEventDestroy(e);
  b = ConstrainBufs();
}

// Buffers for chunks of R rows of W words and a level of at most `level_rows` rows (kept from call to call while
// they are large enough).
static int constrain_alloc(ConstrainBufs& b, int W, uint64_t R, uint64_t level_rows) {
  const uint64_t words = round64(std::max<uint64_t>(level_rows, 1)) / 64;
  if (b.stage && b.rows == R && b.W == W && b.keep_words >= words) return RTLA_OK;
  constrain_free(b);
  HIPCHK(hipMalloc((void**)&b.stage, (R * (uint64_t)W + 4) * sizeof(uint32_t)));  // (+ 4: the destination's shift)
  HIPCHK(hipMalloc((void**)&b.stage_par, R * sizeof(uint64_t)));
  HIPCHK(hipMalloc((void**)&b.masks, R * sizeof(int)));
  HIPCHK(hipMalloc((void**)&b.keep, words * sizeof(uint64_t)));
  HIPCHK(hipMalloc((void**)&b.offs, R / 64 * sizeof(uint32_t)));
  HIPCHK(hipMalloc((void**)&b.tot, sizeof(ConstrainTotals)));
  HIPCHK(hipMalloc((void**)&b.ctr, sizeof(AuditCounters)));
  HIPCHK(hipMalloc((void**)&b.prog, PRED_MAX_WORDS * sizeof(uint32_t)));
  for (hipEvent_t& e : b.ev) HIPCHK(hipEventCreate(&e));
  b.rows = R;
  b.W = W;
  b.keep_words = words;
  return RTLA_OK;
}

namespace {
struct Outcome {
  uint64_t kept = 0, dropped = 0;
  uint64_t counts[AUDIT_COUNTS] = {};
  int flags = 0;
  float eval_ms = 0, move_ms = 0;
  bool moving = false;  // the call failed after the first row may have moved
};
}  // namespace

// The pass over rows [0, n) of `cur`, whose parent records are parents[0, n): the keep bitmap of the whole level
// first (k_pred_state's masks, chunk by chunk, packed by ballot), one synchronisation to learn of evaluation
// errors and of how many rows go, then the compaction, chunk by chunk in stream order.
static int constrain_run(const Layout& L, const Ring& cur, uint64_t n, uint64_t* parents, const rtla_pred* p,
                         ConstrainBufs& b, hipStream_t st, Outcome* o) {
  const uint64_t R = b.rows, nchunk = constrain_chunks(n, R);
  AuditCounters h = audit_zero();
  ConstrainTotals t{};
  HIPCHK(hipMemcpyAsync(b.prog, p->code.data(), p->code.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(b.ctr, &h, sizeof h, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(b.tot, &t, sizeof t, hipMemcpyHostToDevice, st));
  HIPCHK(hipEventRecord(b.ev[0], st));
  for (uint64_t c = 0; c < nchunk; c++) {
    const ConstrainChunk ch = constrain_chunk(n, R, c);
    const Ring sub{cur.base, ring_idx(cur, ch.first), cur.cap};
    HIPCHK(launch_pred(L, sub, ch.rows, b.prog, (int)p->code.size(), b.masks, b.ctr, st));
    HIPCHK(launch_constrain_pack(b.masks, ch.rows, b.keep + ch.first / 64, b.tot, st));
  }
  HIPCHK(hipEventRecord(b.ev[1], st));
  HIPCHK(hipMemcpyAsync(&h, b.ctr, sizeof h, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&t, b.tot, sizeof t, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipEventElapsedTime(&o->eval_ms, b.ev[0], b.ev[1]));
  o->flags = h.flags;
  if (h.flags) {
    report_flags(h.flags);
    return flags_to_status(h.flags);
  }
  for (int k = 0; k < AUDIT_COUNTS; k++) o->counts[k] = h.counts[k];
  o->dropped = t.dropped;
  o->kept = n - t.dropped;
  if (!t.dropped) return RTLA_OK;  // nothing goes: nothing is written
  o->moving = true;
  for (uint64_t c = 0; c < nchunk; c++) {
    const ConstrainChunk ch = constrain_chunk(n, R, c);
    HIPCHK(launch_constrain_move(cur, L.W, ch.first, ch.rows, b.keep + ch.first / 64, b.offs, parents, b.stage,
                                 b.stage_par, b.tot, st));
  }
  HIPCHK(hipEventRecord(b.ev[2], st));
  HIPCHK(hipMemcpyAsync(&t, b.tot, sizeof t, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipEventElapsedTime(&o->move_ms, b.ev[1], b.ev[2]));
  if (t.base + t.kept != o->kept) {  // (the scans and the bitmap's tally count the same bits)
    fprintf(stderr, "rtla: constraint pass kept %llu rows, its bitmap holds %llu\n",
            (unsigned long long)(t.base + t.kept), (unsigned long long)o->kept);
    return RTLA_E_HIP;
  }
  o->moving = false;
  return RTLA_OK;
}

extern "C" int rtla_pred_constrain(rtla_ctx* x, const rtla_pred* p, rtla_constrain_stats* out) {
  if (!x || !p) return RTLA_E_ARG;
  if (!frontier_pass_ok(x)) return RTLA_E_STATE;
  const Layout L = x->L;
  if (p->step || !pred_bound_to(p, L)) return RTLA_E_ARG;
  HIPCHK(hipSetDevice(x->device));
  Shard& s = x->sh[0];
  const uint64_t n = s.n_cur;
  const uint64_t R = std::min(constrain_chunk_rows(getenv("RTLA_CONSTRAIN_CHUNK")), x->front_cap);
  if (int rc = constrain_alloc(x->constrain, L.W, R, x->front_cap)) return rc;
  Outcome o;
  int status = constrain_run(L, cur_ring(x, s), n, s.parents + s.cur_base, p, x->constrain, x->stream, &o);
  if (status == RTLA_OK) {
    x->sim.viol = false;  // (their violations name rows of the level as it was)
    x->audit.viol = false;
    s.n_cur = o.kept;
    x->distinct -= o.dropped;
    x->max_front = o.kept;
    if (o.kept == 0) {
      x->finished = true;
      status = RTLA_DONE;
    }
  } else if (o.moving) {
    x->finished = true;
  }
  if (out) {
    memset(out, 0, sizeof *out);
    out->level = x->level;
    out->status = status;
    out->examined = n;
    out->kept = status < 0 ? 0 : o.kept;
    out->dropped = status < 0 ? 0 : o.dropped;
    static_assert(sizeof out->counts / sizeof out->counts[0] == AUDIT_COUNTS, "rtla_constrain_stats.counts");
    for (int k = 0; k < AUDIT_COUNTS; k++) out->counts[k] = o.counts[k];
    out->start = s.cur_start;
    out->eval_ms = o.eval_ms;
    out->move_ms = o.move_ms;
    out->distinct_total = x->distinct;
    out->flags = o.flags;
  }
  return status;
}

extern "C" int rtla_constrain_batch(const rtla_cfg* c, const rtla_pred* p, const uint32_t* rows, size_t n,
                                    uint64_t ring_cap, uint64_t ring_start, uint64_t chunk, uint32_t* out_rows,
                                    uint64_t* parents, size_t* kept, uint64_t* counts) {
  Layout L;
  if (int r = layout_from_cfg(c, &L)) return r;
  if (!p || p->step || !pred_bound_to(p, L)) return RTLA_E_ARG;
  if (!kept || (n && (!rows || !out_rows || !parents)) || !constrain_ring_ok(n, ring_cap, ring_start))
    return RTLA_E_ARG;
  if (!n) {
    *kept = 0;
    if (counts) memset(counts, 0, AUDIT_COUNTS * sizeof *counts);
    return RTLA_OK;
  }
  const size_t W = (size_t)L.W;
  ConstrainBufs b;
  uint32_t* d_ring = nullptr;
  uint64_t* d_par = nullptr;
  Outcome o;
  // rows [g, g + m) of the ring <-> host, in the pieces the wrap cuts them into
  auto ring_move = [&](uint32_t* host, uint64_t m, bool to_host) -> int {
    const Ring r{d_ring, ring_start, ring_cap};
    for (uint64_t g = 0; g < m;) {
      const uint64_t at = ring_idx(r, g), piece = std::min<uint64_t>(m - g, ring_cap - at);
      HIPCHK(to_host ? hipMemcpy(host + g * W, d_ring + at * W, piece * W * 4, hipMemcpyDeviceToHost)
                     : hipMemcpy(d_ring + at * W, host + g * W, piece * W * 4, hipMemcpyHostToDevice));
      g += piece;
    }
    return RTLA_OK;
  };
  auto run = [&]() -> int {
    if (int rc = constrain_alloc(b, L.W, std::min(constrain_chunk_rows(chunk), ring_cap), ring_cap)) return rc;
    HIPCHK(hipMalloc((void**)&d_ring, ring_cap * W * 4));
    HIPCHK(hipMalloc((void**)&d_par, n * sizeof(uint64_t)));
    HIPCHK(hipMemset(d_ring, 0, ring_cap * W * 4));
    if (int rc = ring_move(const_cast<uint32_t*>(rows), n, false)) return rc;
    HIPCHK(hipMemcpy(d_par, parents, n * sizeof(uint64_t), hipMemcpyHostToDevice));
    if (int rc = constrain_run(L, Ring{d_ring, ring_start, ring_cap}, n, d_par, p, b, nullptr, &o)) return rc;
    if (int rc = ring_move(out_rows, o.kept, true)) return rc;
    if (o.kept) HIPCHK(hipMemcpy(parents, d_par, o.kept * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return RTLA_OK;
  };
  const int rc = run();
  constrain_free(b);
  for (void* q : {(void*)d_ring, (void*)d_par})
    if (q) (void)hipFree(q);
  if (rc) return rc;
  *kept = o.kept;
  if (counts)
    for (int k = 0; k < AUDIT_COUNTS; k++) counts[k] = o.counts[k];
  return RTLA_OK;
}
