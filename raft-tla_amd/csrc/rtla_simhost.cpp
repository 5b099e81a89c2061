// rtla_simhost.cpp -- random-walk simulation (TLC -simulate; semantics:
// rtla_sim.h).  The walks run on the device (k_simulate); the same walks are
// computed on the host by sim_walk_serial: rtla_sim_replay / rtla_sim_walk
// (stateless, no GPU), and the counterexample of a simulated violation
// (rtla_trace).  The *_pred calls are the same walks carrying a compiled state
// set and / or action set: one driver each, the plain
// calls being the ones without a set.
#include "rtla_ctx.h"
#include "rtla_predc.h"
#include "rtla_sim.h"

static bool sim_layout_ok(const Layout& L) { return L.fam[F_RECEIVE] + 3 * L.K <= SIM_MAX_CAND; }

static void sim_fill_stats(rtla_sim_stats* st, uint64_t walks, const SimTally& t, uint64_t batch_first, double ms,
                           int status) {
  if (!st) return;
  memset(st, 0, sizeof *st);
  st->walks = walks; st->steps = t.steps; st->generated = t.generated; st->stuck = t.stuck;
  st->kernel_ms = ms; st->status = status; st->flags = t.flags;
  st->viol_walk = ~0ull; st->viol_inst = -1;
  if (t.viol_key != SIM_NO_VIOLATION) {
    st->viol_walk = batch_first + sim_key_walk(t.viol_key);
    st->viol_step = sim_key_step(t.viol_key);
    st->viol_inst = sim_key_inst(t.viol_key);
    st->viol_in_model = sim_key_in_model(t.viol_key);
    st->viol_mask = sim_key_mask(t.viol_key);
  }
  static_assert(sizeof st->taken / sizeof st->taken[0] == COVER_CODES, "rtla_sim_stats.taken holds every coverage code");
  for (int k = 0; k < COVER_CODES; k++) st->taken[k] = t.taken[k];
}

static void sim_fill_pred_stats(rtla_sim_pred_stats* po, const SimTally& t) {
  if (!po) return;
  memset(po, 0, sizeof *po);
  po->state_evaluated = t.state_evaluated;
  po->step_evaluated = t.step_evaluated;
  if (t.viol_key != SIM_NO_VIOLATION) {
    po->viol_inv_mask = sim_word_inv_mask(t.viol_word);
    po->viol_state_mask = sim_word_state_mask(t.viol_word);
    po->viol_step_mask = sim_word_step_mask(t.viol_word);
  }
}
// The reported violation of walks with user properties: the key names (walk, step, instance), the walk's fifth
// end word the rest.
static void sim_fill_from_word(rtla_sim_stats* st, const SimTally& t) {
  if (!st || t.viol_key == SIM_NO_VIOLATION) return;
  st->viol_in_model = sim_word_in_model(t.viol_word);
  st->viol_mask = sim_word_inv_mask(t.viol_word);
}

// The sets a *_pred call was given: either may be null, not both; each of its kind and compiled for L.
static bool sim_sets_ok(const Layout& L, const rtla_pred* states, const rtla_pred* steps) {
  if (!states && !steps) return false;
  if (states && (states->step || !pred_bound_to(states, L))) return false;
  if (steps && (!steps->step || !pred_bound_to(steps, L))) return false;
  return true;
}

int sim_walk_rows(const Layout& L, const uint32_t* start, uint64_t seed, uint64_t walk, int depth, uint32_t* rows,
                  int32_t* labels, size_t cap, size_t* n_rows, const uint32_t* sprog, const uint32_t* aprog) {
  if (!sim_layout_ok(L)) return RTLA_E_CONFIG;
  std::vector<uint32_t> buf(3 * (size_t)L.W);
  SimTally tl;
  size_t n = 0;
  const SimEnd e = dispatch_n(L, [&](auto ns) {
    return sim_walk_serial<decltype(ns)::value>(L, start, seed, walk, 0, depth, buf.data(), tl,
                                                [&](int, const uint32_t* row, int32_t label, bool) {
                                                  if (n < cap) {
                                                    if (rows) memcpy(rows + n * L.W, row, (size_t)L.W * 4);
                                                    if (labels) labels[n] = label;
                                                  }
                                                  n++;
                                                }, sprog, aprog);
  });
  if (n_rows) *n_rows = n;
  if (tl.flags) return flags_to_status(tl.flags);
  if ((rows || labels) && n > cap) return RTLA_E_ARG;
  return e.stop == SIM_STOP_VIOLATION ? RTLA_VIOLATION : RTLA_OK;
}

extern "C" int rtla_sim_walk(const rtla_cfg* c, const uint32_t* start_row, uint64_t seed, uint64_t walk, int32_t depth,
                             uint32_t* rows, int32_t* labels, size_t cap, size_t* n_rows) {
  CFG_LAYOUT(L, c);
  if (!start_row || depth < 0 || depth > SIM_MAX_DEPTH) return RTLA_E_ARG;
  return sim_walk_rows(L, start_row, seed, walk, depth, rows, labels, cap, n_rows, nullptr, nullptr);
}

extern "C" int rtla_sim_walk_pred(const rtla_cfg* c, const uint32_t* start_row, uint64_t seed, uint64_t walk,
                                  int32_t depth, const rtla_pred* states, const rtla_pred* steps, uint32_t* rows,
                                  int32_t* labels, size_t cap, size_t* n_rows) {
  CFG_LAYOUT(L, c);
  if (!start_row || depth < 0 || depth > SIM_MAX_DEPTH || !sim_sets_ok(L, states, steps)) return RTLA_E_ARG;
  return sim_walk_rows(L, start_row, seed, walk, depth, rows, labels, cap, n_rows,
                       states ? states->code.data() : nullptr, steps ? steps->code.data() : nullptr);
}

// The host walks of rtla_sim_replay (sprog == aprog == null: 4-word records) and rtla_sim_replay_pred (5-word).
static int sim_replay(const Layout& L, const uint32_t* start_rows, size_t n_start, uint64_t seed, uint64_t first_walk,
                      uint64_t n_walks, int depth, int threads, const uint32_t* sprog, const uint32_t* aprog,
                      uint64_t* ends, rtla_sim_stats* out, rtla_sim_pred_stats* pout) {
  if (!start_rows || !n_start || depth < 0 || depth > SIM_MAX_DEPTH || first_walk + n_walks < first_walk)
    return RTLA_E_ARG;
  if (!sim_layout_ok(L)) return RTLA_E_CONFIG;
  const bool pred = sprog || aprog;
  const int ew = pred ? 5 : 4;
  const double t0 = now_s();
  const int nt = std::min(text_threads(threads), 16);
  SimTally sum;
  uint64_t done = 0, viol_first = 0;
  // the same batches as rtla_simulate: no further batch after one that found a violation
  for (uint64_t b0 = 0; b0 < n_walks && sum.viol_key == SIM_NO_VIOLATION; b0 += SIM_BATCH) {
    const uint64_t nb = std::min<uint64_t>(SIM_BATCH, n_walks - b0);
    std::vector<SimTally> part((size_t)nt);
    parallel_chunks(nb, 64, nt, [&](int t, size_t i0, size_t i1) {
      std::vector<uint32_t> buf(3 * (size_t)L.W);
      for (uint64_t i = i0; i < i1; i++) {
        const uint64_t w = first_walk + b0 + i;
        const SimEnd e = dispatch_n(L, [&](auto ns) {
          return sim_walk_serial<decltype(ns)::value>(L, start_rows + (w % n_start) * (size_t)L.W, seed, w, i, depth,
                                                      buf.data(), part[(size_t)t],
                                                      [](int, const uint32_t*, int32_t, bool) {}, sprog, aprog);
        });
        if (ends) {
          uint64_t* o = ends + ew * (b0 + i);
          o[0] = e.last.a; o[1] = e.last.b; o[2] = e.digest; o[3] = sim_end_word(e.length, e.stop);
          if (pred)
            o[4] = e.stop != SIM_STOP_VIOLATION ? 0
                       : sim_viol_word(e.viol_inst, e.viol_in_model, e.viol_mask, e.viol_state_mask, e.viol_step_mask);
        }
      }
    });
    for (const SimTally& p : part) {
      sum.steps += p.steps; sum.generated += p.generated; sum.stuck += p.stuck; sum.flags |= p.flags;
      sum.state_evaluated += p.state_evaluated; sum.step_evaluated += p.step_evaluated;
      if (p.viol_key < sum.viol_key) {
        sum.viol_key = p.viol_key;
        sum.viol_word = p.viol_word;
      }
      for (int k = 0; k < COVER_CODES; k++) sum.taken[k] += p.taken[k];
    }
    viol_first = first_walk + b0;
    done = b0 + nb;
  }
  const int status = sum.flags ? flags_to_status(sum.flags) : sum.viol_key != SIM_NO_VIOLATION ? RTLA_VIOLATION : RTLA_OK;
  sim_fill_stats(out, done, sum, viol_first, (now_s() - t0) * 1e3, status);
  if (pred) {
    sim_fill_from_word(out, sum);
    sim_fill_pred_stats(pout, sum);
  }
  return status;
}

extern "C" int rtla_sim_replay(const rtla_cfg* c, const uint32_t* start_rows, size_t n_start, uint64_t seed,
                               uint64_t first_walk, uint64_t n_walks, int32_t depth, int threads, uint64_t* ends,
                               rtla_sim_stats* out) {
  CFG_LAYOUT(L, c);
  return sim_replay(L, start_rows, n_start, seed, first_walk, n_walks, depth, threads, nullptr, nullptr, ends, out,
                    nullptr);
}

extern "C" int rtla_sim_replay_pred(const rtla_cfg* c, const uint32_t* start_rows, size_t n_start, uint64_t seed,
                                    uint64_t first_walk, uint64_t n_walks, int32_t depth, int threads,
                                    const rtla_pred* states, const rtla_pred* steps, uint64_t* ends5,
                                    rtla_sim_stats* out, rtla_sim_pred_stats* pout) {
  CFG_LAYOUT(L, c);
  if (!sim_sets_ok(L, states, steps)) return RTLA_E_ARG;
  return sim_replay(L, start_rows, n_start, seed, first_walk, n_walks, depth, threads,
                    states ? states->code.data() : nullptr, steps ? steps->code.data() : nullptr, ends5, out, pout);
}

// The device walks of rtla_simulate (states == steps == null: k_simulate, 4-word records) and rtla_simulate_pred
// (k_simulate_pred, 5-word records).
static int sim_device(rtla_ctx* x, uint64_t seed, uint64_t first_walk, uint64_t n_walks, int depth,
                      const rtla_pred* states, const rtla_pred* steps, uint64_t* ends, rtla_sim_stats* out,
                      rtla_sim_pred_stats* pout) {
  const bool pred = states || steps;
  const uint64_t ew = pred ? 5 : 4;
  const Layout& L = x->L;
  if (!sim_layout_ok(L)) return RTLA_E_CONFIG;
  HIPCHK(hipSetDevice(x->device));
  Shard& s = x->sh[0];
  SimState& m = x->sim;
  m.viol = false;
  x->audit.viol = false;
  if (!m.ctr) HIPCHK(hipMalloc((void**)&m.ctr, sizeof(SimCounters)));
  if (!m.ev0) HIPCHK(hipEventCreate(&m.ev0));
  if (!m.ev1) HIPCHK(hipEventCreate(&m.ev1));
  const uint64_t batch = std::min<uint64_t>(SIM_BATCH, std::max<uint64_t>(1, n_walks));
  if (m.ends_cap < batch * ew) {
    if (m.ends) (void)hipFree(m.ends);
    m.ends = nullptr; m.ends_cap = 0;
    HIPCHK(hipMalloc((void**)&m.ends, batch * ew * 8));
    m.ends_cap = batch * ew;
  }
  int nsw = 0, naw = 0;
  if (pred) {  // both programs' device copy: P's words, then A's
    if (!m.prog) HIPCHK(hipMalloc((void**)&m.prog, 2 * PRED_MAX_WORDS * sizeof(uint32_t)));
    nsw = states ? (int)states->code.size() : 0;
    naw = steps ? (int)steps->code.size() : 0;
    if (nsw > PRED_MAX_WORDS || naw > PRED_MAX_WORDS) return RTLA_E_ARG;
    if (nsw) HIPCHK(hipMemcpyAsync(m.prog, states->code.data(), (size_t)nsw * 4, hipMemcpyHostToDevice, x->stream));
    if (naw)
      HIPCHK(hipMemcpyAsync(m.prog + PRED_MAX_WORDS, steps->code.data(), (size_t)naw * 4, hipMemcpyHostToDevice,
                            x->stream));
  }
  SimTally sum;
  double ms = 0;
  uint64_t done = 0, viol_first = 0;
  for (uint64_t b0 = 0; b0 < n_walks && sum.viol_key == SIM_NO_VIOLATION; b0 += SIM_BATCH) {
    const uint64_t nb = std::min<uint64_t>(SIM_BATCH, n_walks - b0);
    const int seg = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(depth, 1), SIM_LAUNCH_STEPS / nb));
    if (seg < depth && m.carry_cap < nb) {
      if (m.carry) (void)hipFree(m.carry);
      m.carry = nullptr; m.carry_cap = 0;
      HIPCHK(hipMalloc((void**)&m.carry, batch * (uint64_t)L.W * 4));
      m.carry_cap = batch;
    }
    SimCounters h;
    memset(&h, 0, sizeof h);
    h.viol_key = SIM_NO_VIOLATION;
    HIPCHK(hipMemcpyAsync(m.ctr, &h, sizeof h, hipMemcpyHostToDevice, x->stream));
    HIPCHK(hipEventRecord(m.ev0, x->stream));
    int t0 = 0;
    do {  // (depth 0: one launch that writes the end records of the start rows)
      const int t1 = std::min(depth, t0 + seg);
      uint32_t* const carry = seg < depth ? m.carry : nullptr;
      if (pred)
        HIPCHK(launch_simulate_pred(L, cur_ring(x, s), s.n_cur, seed, first_walk + b0, (uint32_t)nb, t0, t1, depth,
                                    carry, m.ends, m.ctr, m.prog, nsw, naw, x->stream));
      else
        HIPCHK(launch_simulate(L, cur_ring(x, s), s.n_cur, seed, first_walk + b0, (uint32_t)nb, t0, t1, depth, carry,
                               m.ends, m.ctr, x->stream));
      t0 = t1;
    } while (t0 < depth);
    HIPCHK(hipEventRecord(m.ev1, x->stream));
    HIPCHK(hipMemcpyAsync(&h, m.ctr, sizeof h, hipMemcpyDeviceToHost, x->stream));
    if (ends) HIPCHK(hipMemcpyAsync(ends + ew * b0, m.ends, nb * ew * 8, hipMemcpyDeviceToHost, x->stream));
    HIPCHK(hipStreamSynchronize(x->stream));
    float bms = 0;
    HIPCHK(hipEventElapsedTime(&bms, m.ev0, m.ev1));
    ms += bms;
    sum.steps += h.steps; sum.generated += h.generated; sum.stuck += h.stuck; sum.flags |= h.flags;
    sum.state_evaluated += h.state_evaluated; sum.step_evaluated += h.step_evaluated;
    sum.viol_key = h.viol_key;
    for (int k = 0; k < COVER_CODES; k++) sum.taken[k] += h.taken[k];
    viol_first = first_walk + b0;
    done = b0 + nb;
    if (sum.flags) break;
    if (pred && sum.viol_key != SIM_NO_VIOLATION)  // the masks: that walk's fifth word
      HIPCHK(hipMemcpy(&sum.viol_word, m.ends + 5 * sim_key_walk(sum.viol_key) + 4, 8, hipMemcpyDeviceToHost));
  }
  int status = RTLA_OK;
  if (sum.flags) {
    report_flags(sum.flags);
    status = flags_to_status(sum.flags);
  } else if (sum.viol_key != SIM_NO_VIOLATION) {
    status = RTLA_VIOLATION;
  }
  sim_fill_stats(out, done, sum, viol_first, ms, status);
  if (pred) {
    sim_fill_from_word(out, sum);
    sim_fill_pred_stats(pout, sum);
  }
  if (status == RTLA_VIOLATION) {
    m.viol = true;
    m.seed = seed;
    m.walk = viol_first + sim_key_walk(sum.viol_key);
    m.start = s.cur_base + m.walk % s.n_cur;
    m.step = sim_key_step(sum.viol_key);
    m.inst = sim_key_inst(sum.viol_key);
    m.in_model = pred ? sim_word_in_model(sum.viol_word) : sim_key_in_model(sum.viol_key);
    m.mask = sim_key_mask(sum.viol_key);
    m.scode.clear();
    m.acode.clear();
    if (pred) {  // rtla_violation: the built-in mask if nonzero, else the state mask, else the step mask
      const int im = sim_word_inv_mask(sum.viol_word), sm = sim_word_state_mask(sum.viol_word);
      m.mask = im ? im : sm ? sm : sim_word_step_mask(sum.viol_word);
      if (states) m.scode = states->code;  // rtla_trace replays the walk with the sets
      if (steps) m.acode = steps->code;
    }
  }
  return status;
}

extern "C" int rtla_simulate(rtla_ctx* x, uint64_t seed, uint64_t first_walk, uint64_t n_walks, int32_t depth,
                             uint64_t* ends, rtla_sim_stats* out) {
  if (!x) return RTLA_E_ARG;
  if (!frontier_pass_ok(x)) return RTLA_E_STATE;
  if (depth < 0 || depth > SIM_MAX_DEPTH || first_walk + n_walks < first_walk) return RTLA_E_ARG;
  return sim_device(x, seed, first_walk, n_walks, depth, nullptr, nullptr, ends, out, nullptr);
}

extern "C" int rtla_simulate_pred(rtla_ctx* x, uint64_t seed, uint64_t first_walk, uint64_t n_walks, int32_t depth,
                                  const rtla_pred* states, const rtla_pred* steps, uint64_t* ends5,
                                  rtla_sim_stats* out, rtla_sim_pred_stats* pout) {
  if (!x) return RTLA_E_ARG;
  if (!frontier_pass_ok(x)) return RTLA_E_STATE;
  if (depth < 0 || depth > SIM_MAX_DEPTH || first_walk + n_walks < first_walk || !sim_sets_ok(x->L, states, steps))
    return RTLA_E_ARG;
  return sim_device(x, seed, first_walk, n_walks, depth, states, steps, ends5, out, pout);
}
