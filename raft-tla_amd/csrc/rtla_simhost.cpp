// rtla_simhost.cpp -- random-walk simulation (TLC -simulate; semantics:
// rtla_sim.h).  The walks run on the device (k_simulate); the same walks are
// computed on the host by sim_walk_serial: rtla_sim_replay / rtla_sim_walk
// (stateless, no GPU), and the counterexample of a simulated violation
// (rtla_trace).
#include "rtla_ctx.h"
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

int sim_walk_rows(const Layout& L, const uint32_t* start, uint64_t seed, uint64_t walk, int depth, uint32_t* rows,
                  int32_t* labels, size_t cap, size_t* n_rows) {
  if (!sim_layout_ok(L)) return RTLA_E_CONFIG;
  std::vector<uint32_t> buf(2 * (size_t)L.W);
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
                                                });
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
  return sim_walk_rows(L, start_row, seed, walk, depth, rows, labels, cap, n_rows);
}

extern "C" int rtla_sim_replay(const rtla_cfg* c, const uint32_t* start_rows, size_t n_start, uint64_t seed,
                               uint64_t first_walk, uint64_t n_walks, int32_t depth, int threads, uint64_t* ends,
                               rtla_sim_stats* out) {
  CFG_LAYOUT(L, c);
  if (!start_rows || !n_start || depth < 0 || depth > SIM_MAX_DEPTH || first_walk + n_walks < first_walk)
    return RTLA_E_ARG;
  if (!sim_layout_ok(L)) return RTLA_E_CONFIG;
  const double t0 = now_s();
  const int nt = std::min(text_threads(threads), 16);
  SimTally sum;
  uint64_t done = 0, viol_first = 0;
  // the same batches as rtla_simulate: no further batch after one that found a violation
  for (uint64_t b0 = 0; b0 < n_walks && sum.viol_key == SIM_NO_VIOLATION; b0 += SIM_BATCH) {
    const uint64_t nb = std::min<uint64_t>(SIM_BATCH, n_walks - b0);
    std::vector<SimTally> part((size_t)nt);
    parallel_chunks(nb, 64, nt, [&](int t, size_t i0, size_t i1) {
      std::vector<uint32_t> buf(2 * (size_t)L.W);
      for (uint64_t i = i0; i < i1; i++) {
        const uint64_t w = first_walk + b0 + i;
        const SimEnd e = dispatch_n(L, [&](auto ns) {
          return sim_walk_serial<decltype(ns)::value>(L, start_rows + (w % n_start) * (size_t)L.W, seed, w, i, depth,
                                                      buf.data(), part[(size_t)t], [](int, const uint32_t*, int32_t, bool) {});
        });
        if (ends) {
          uint64_t* o = ends + 4 * (b0 + i);
          o[0] = e.last.a; o[1] = e.last.b; o[2] = e.digest; o[3] = sim_end_word(e.length, e.stop);
        }
      }
    });
    for (const SimTally& p : part) {
      sum.steps += p.steps; sum.generated += p.generated; sum.stuck += p.stuck; sum.flags |= p.flags;
      sum.viol_key = std::min(sum.viol_key, p.viol_key);
      for (int k = 0; k < COVER_CODES; k++) sum.taken[k] += p.taken[k];
    }
    viol_first = first_walk + b0;
    done = b0 + nb;
  }
  const int status = sum.flags ? flags_to_status(sum.flags) : sum.viol_key != SIM_NO_VIOLATION ? RTLA_VIOLATION : RTLA_OK;
  sim_fill_stats(out, done, sum, viol_first, (now_s() - t0) * 1e3, status);
  return status;
}

extern "C" int rtla_simulate(rtla_ctx* x, uint64_t seed, uint64_t first_walk, uint64_t n_walks, int32_t depth,
                             uint64_t* ends, rtla_sim_stats* out) {
  if (!x) return RTLA_E_ARG;
  if (!frontier_pass_ok(x)) return RTLA_E_STATE;
  if (depth < 0 || depth > SIM_MAX_DEPTH || first_walk + n_walks < first_walk) return RTLA_E_ARG;
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
  if (m.ends_cap < batch) {
    if (m.ends) (void)hipFree(m.ends);
    m.ends = nullptr; m.ends_cap = 0;
    HIPCHK(hipMalloc((void**)&m.ends, batch * 32));
    m.ends_cap = batch;
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
      HIPCHK(launch_simulate(L, cur_ring(x, s), s.n_cur, seed, first_walk + b0, (uint32_t)nb, t0, t1, depth,
                             seg < depth ? m.carry : nullptr, m.ends, m.ctr, x->stream));
      t0 = t1;
    } while (t0 < depth);
    HIPCHK(hipEventRecord(m.ev1, x->stream));
    HIPCHK(hipMemcpyAsync(&h, m.ctr, sizeof h, hipMemcpyDeviceToHost, x->stream));
    if (ends) HIPCHK(hipMemcpyAsync(ends + 4 * b0, m.ends, nb * 32, hipMemcpyDeviceToHost, x->stream));
    HIPCHK(hipStreamSynchronize(x->stream));
    float bms = 0;
    HIPCHK(hipEventElapsedTime(&bms, m.ev0, m.ev1));
    ms += bms;
    sum.steps += h.steps; sum.generated += h.generated; sum.stuck += h.stuck; sum.flags |= h.flags;
    sum.viol_key = h.viol_key;
    for (int k = 0; k < COVER_CODES; k++) sum.taken[k] += h.taken[k];
    viol_first = first_walk + b0;
    done = b0 + nb;
    if (sum.flags) break;
  }
  int status = RTLA_OK;
  if (sum.flags) {
    report_flags(sum.flags);
    status = flags_to_status(sum.flags);
  } else if (sum.viol_key != SIM_NO_VIOLATION) {
    status = RTLA_VIOLATION;
  }
  sim_fill_stats(out, done, sum, viol_first, ms, status);
  if (status == RTLA_VIOLATION) {
    m.viol = true;
    m.seed = seed;
    m.walk = viol_first + sim_key_walk(sum.viol_key);
    m.start = s.cur_base + m.walk % s.n_cur;
    m.step = sim_key_step(sum.viol_key);
    m.inst = sim_key_inst(sum.viol_key);
    m.in_model = sim_key_in_model(sum.viol_key);
    m.mask = sim_key_mask(sum.viol_key);
  }
  return status;
}
