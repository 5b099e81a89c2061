// rtla_rows.cpp -- the context-free part of the C ABI (rows, fingerprints,
// texts, digests, batch expansion: the parity seams of the tests) and the
// synthetic and probe micro-benchmarks.
#include <sched.h>

#include <atomic>
#include <string>
#include <thread>

#include "rtla_ctx.h"
#include "rtla_synth.h"
#include "rtla_text.h"

extern "C" int rtla_row_words(const rtla_cfg* c) {
  CFG_LAYOUT(L, c);
  return L.W;
}

extern "C" int rtla_row_layout(const rtla_cfg* c, int32_t* out, int n) {
  CFG_LAYOUT(L, c);
  if (!out) return RTLA_E_ARG;
  const int32_t v[10] = {L.W, L.off_hdr, L.off_srv, L.srv_w, L.off_all, L.all_words, L.off_elec, L.elec_w, L.off_bag,
                         L.slot_w};
  const int m = std::min(n, 10);
  for (int k = 0; k < m; k++) out[k] = v[k];
  return m;
}

extern "C" int rtla_init_row(const rtla_cfg* c, uint32_t* row) {
  CFG_LAYOUT(L, c);
  row_init(L, row);
  return RTLA_OK;
}

extern "C" int rtla_invariants(const rtla_cfg* c, const uint32_t* row) {
  CFG_LAYOUT(L, c);
  return check_invariants<0>(L, row, (const Delta*)nullptr);
}

extern "C" int rtla_row_fingerprint(const rtla_cfg* c, const uint32_t* row, uint64_t out[2]) {
  CFG_LAYOUT(L, c);
  FP f = row_fingerprint(L, row);
  out[0] = f.a;
  out[1] = f.b;
  return RTLA_OK;
}

extern "C" int rtla_orbit_key(const rtla_cfg* c, const uint32_t* row, uint64_t out[2], int* perms) {
  CFG_LAYOUT(L, c);
  const FP f = dispatch_n(L, [&](auto ns) { return orbit_key_row<decltype(ns)::value>(L, row, perms); });
  out[0] = f.a;
  out[1] = f.b;
  return RTLA_OK;
}

extern "C" int rtla_permute_row(const rtla_cfg* c, const uint32_t* row, const int* pi, uint32_t* out) {
  CFG_LAYOUT(L, c);
  int seen = 0;
  for (int i = 0; i < L.N; i++) {
    if (pi[i] < 0 || pi[i] >= L.N || (seen >> pi[i] & 1)) return RTLA_E_ARG;
    seen |= 1 << pi[i];
  }
  dispatch_n(L, [&](auto ns) { permute_row<decltype(ns)::value>(L, row, pi, out); });
  return RTLA_OK;
}

extern "C" int rtla_state_text(const rtla_cfg* c, const uint32_t* row, char* buf, size_t cap) {
  CFG_LAYOUT(L, c);
  std::string s = state_text(L, row);
  if (s.size() + 1 > cap) return RTLA_E_ARG;
  memcpy(buf, s.c_str(), s.size() + 1);
  return (int)s.size();
}

extern "C" int rtla_action_name(const rtla_cfg* c, int32_t inst, int32_t sub, char* buf, size_t cap) {
  CFG_LAYOUT(L, c);
  std::string s = action_name(L, inst, sub);
  if (s.size() + 1 > cap) return RTLA_E_ARG;
  memcpy(buf, s.c_str(), s.size() + 1);
  return (int)s.size();
}

// ---- level digests (rtla_rows_text_hash / rtla_level_text_hash): the sum of
// FNV-1a-64 of each state's canonical text, computed by a pool of host threads.
int text_threads(int want) {
  if (want > 0) return std::min(want, 256);
  int n = 0;
  if (const char* e = getenv("OMP_NUM_THREADS")) n = atoi(e);  // the GPU box's per-job CPU allowance
  if (n <= 0) {
    cpu_set_t cs;
    n = sched_getaffinity(0, sizeof cs, &cs) == 0 ? CPU_COUNT(&cs) : 8;
  }
  return std::max(1, std::min(n, 16));
}

// FNV-1a is one serial multiply chain per text: 8 texts are hashed together
// so the chains overlap (multiplier throughput, not latency, bounds a core).
constexpr int TEXT_ILP = 8;
static uint64_t fnv1a64_sum(char* const* txt, const size_t* len, int m) {
  uint64_t h[TEXT_ILP];
  size_t common = ~(size_t)0;
  for (int i = 0; i < m; i++) {
    h[i] = 0xcbf29ce484222325ull;
    common = std::min(common, len[i]);
  }
  for (size_t k = 0; k < common; k++)
    for (int i = 0; i < TEXT_ILP; i++)
      if (i < m) h[i] = (h[i] ^ (unsigned char)txt[i][k]) * 0x100000001b3ull;
  uint64_t sum = 0;
  for (int i = 0; i < m; i++) {
    for (size_t k = common; k < len[i]; k++) h[i] = (h[i] ^ (unsigned char)txt[i][k]) * 0x100000001b3ull;
    sum += h[i];
  }
  return sum;
}

uint64_t rows_digest(const Layout& L, const uint32_t* rows, size_t n, int threads, bool orbit) {
  threads = (int)std::min<size_t>((size_t)threads, std::max<size_t>(1, n / 4096));
  std::vector<uint64_t> part((size_t)threads, 0);
  const size_t cap = state_text_cap(L);
  parallel_chunks(n, 8192, threads, [&](int t, size_t b, size_t e) {
    std::vector<char> buf((TEXT_ILP + 1) * cap);  // TEXT_ILP texts + one scratch area
    char* txt[TEXT_ILP];
    size_t len[TEXT_ILP];
    for (int i = 0; i < TEXT_ILP; i++) txt[i] = buf.data() + i * cap;
    char* scratch = buf.data() + TEXT_ILP * cap;
    uint64_t acc = 0;
    for (size_t k = b; k < e; k += TEXT_ILP) {
      const int m = (int)std::min<size_t>(TEXT_ILP, e - k);
      for (int i = 0; i < m; i++)
        len[i] = orbit ? state_orbit_text_into(L, rows + (k + i) * (size_t)L.W, txt[i], scratch)
                       : state_text_into(L, rows + (k + i) * (size_t)L.W, txt[i], scratch);
      acc += fnv1a64_sum(txt, len, m);
    }
    part[(size_t)t] += acc;
  });
  uint64_t sum = 0;
  for (uint64_t v : part) sum += v;
  return sum;
}

static int rows_hash(const rtla_cfg* c, const uint32_t* rows, size_t n, int threads, uint64_t* out, bool orbit) {
  CFG_LAYOUT(L, c);
  if (!out || (n && !rows)) return RTLA_E_ARG;
  *out = rows_digest(L, rows, n, text_threads(threads), orbit);
  return RTLA_OK;
}
extern "C" int rtla_rows_text_hash(const rtla_cfg* c, const uint32_t* rows, size_t n, int threads, uint64_t* out) {
  return rows_hash(c, rows, n, threads, out, false);
}
extern "C" int rtla_rows_orbit_hash(const rtla_cfg* c, const uint32_t* rows, size_t n, int threads, uint64_t* out) {
  return rows_hash(c, rows, n, threads, out, true);
}

extern "C" int rtla_orbit_text(const rtla_cfg* c, const uint32_t* row, char* buf, size_t cap) {
  CFG_LAYOUT(L, c);
  const size_t tc = state_text_cap(L);
  std::vector<char> b(2 * tc);
  const size_t n = state_orbit_text_into(L, row, b.data(), b.data() + tc);
  if (n + 1 > cap) return RTLA_E_ARG;
  memcpy(buf, b.data(), n);
  buf[n] = 0;
  return (int)n;
}

// Every enabled successor of n device rows (d_rows holds round64(n) rows),
// copied to the host sorted by (input, instance).  The level kernel itself
// runs it -- k_expand_compact with XF_ALL_SUCCESSORS: the same evaluation,
// fingerprint derivation and row building as the BFS, minus the seen set --
// so this parity seam checks the hot kernel; layouts too wide for its LDS
// tile (and RTLA_XFLAGS=2048) use the wave-per-state k_expand_batch.
int expand_batch_dev(const Layout& L, const uint32_t* d_rows, size_t n, std::vector<uint32_t>& out,
                     std::vector<uint64_t>& info, hipStream_t st) {
  size_t cap = round64(std::max<size_t>(n, 1) * (size_t)L.fam[F_COUNT]);
  uint32_t* d_out = nullptr;
  uint64_t* d_info = nullptr;
  DevCounters* d_ctr = nullptr;
  HIPCHK(hipMalloc(&d_out, cap * L.W * 4));
  HIPCHK(hipMalloc(&d_info, cap * 8));
  HIPCHK(hipMalloc(&d_ctr, sizeof(DevCounters)));
  HIPCHK(hipMemsetAsync(d_ctr, 0, sizeof(DevCounters), st));
  const bool hot = expand_compact_wpb(L) > 0 && !(env_xflags() & XF_WAVE_KERNEL);
  if (hot) {
    const uint64_t caps[3] = {round64(n), cap, cap};  // DevCounters cap_cur / cap_next / cap_parents
    HIPCHK(hipMemcpyAsync(&d_ctr->cap_cur, caps, sizeof caps, hipMemcpyHostToDevice, st));
    const Ring cur{const_cast<uint32_t*>(d_rows), 0, round64(n)}, next{d_out, 0, cap};
    HIPCHK(launch_expand({.L = L,
                          .cur = cur,
                          .s_end = n,
                          .out = {next, d_info, 0, cap},
                          .ctr = d_ctr,
                          .st = st,
                          .xflags = XF_ALL_SUCCESSORS | XF_NO_COVER}));
  } else {
    HIPCHK(launch_expand_batch(L, d_rows, n, d_out, d_info, cap, d_ctr, st));
  }
  DevCounters h;
  HIPCHK(hipMemcpyAsync(&h, d_ctr, sizeof h, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  int rc = RTLA_OK;
  if (h.flags) { report_flags(h.flags); rc = flags_to_status(h.flags); }
  size_t m = (size_t)h.next_count;
  out.resize(m * L.W);
  info.resize(m);
  if (m) {
    HIPCHK(hipMemcpy(out.data(), d_out, m * L.W * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(info.data(), d_info, m * 8, hipMemcpyDeviceToHost));
  }
  (void)hipFree(d_out);
  (void)hipFree(d_info);
  (void)hipFree(d_ctr);
  std::vector<size_t> ord(m);
  for (size_t k = 0; k < m; k++) ord[k] = k;
  std::sort(ord.begin(), ord.end(), [&](size_t a, size_t b) {
    const uint64_t ia = successor_input(info[a]), ib = successor_input(info[b]);
    return ia != ib ? ia < ib : successor_inst(info[a]) < successor_inst(info[b]);
  });
  std::vector<uint32_t> o2(m * L.W);
  std::vector<uint64_t> i2(m);
  for (size_t k = 0; k < m; k++) {
    memcpy(&o2[k * L.W], &out[ord[k] * L.W], L.W * 4);
    i2[k] = info[ord[k]];
  }
  out.swap(o2);
  info.swap(i2);
  return rc;
}

extern "C" int rtla_expand_batch(const rtla_cfg* c, const uint32_t* rows, size_t n, uint32_t* succ, uint64_t* info,
                                 size_t cap, size_t* n_out) {
  CFG_LAYOUT(L, c);
  if (!rows || !n_out) return RTLA_E_ARG;
  uint32_t* d_rows = nullptr;
  HIPCHK(hipMalloc(&d_rows, round64(std::max<size_t>(n, 1)) * L.W * 4));
  HIPCHK(hipMemcpy(d_rows, rows, n * L.W * 4, hipMemcpyHostToDevice));
  std::vector<uint32_t> out;
  std::vector<uint64_t> inf;
  const int r = expand_batch_dev(L, d_rows, n, out, inf, nullptr);
  (void)hipFree(d_rows);
  if (r < 0) return r;
  *n_out = inf.size();
  if (inf.size() > cap) return RTLA_E_ARG;
  if (succ) memcpy(succ, out.data(), out.size() * 4);
  if (info) memcpy(info, inf.data(), inf.size() * 8);
  return RTLA_OK;
}

extern "C" int rtla_random_rows(const rtla_cfg* c, uint64_t seed, uint64_t first, uint64_t n, uint64_t pool,
                                uint32_t* rows) {
  CFG_LAYOUT(L, c);
  if (!rows && n) return RTLA_E_ARG;
  for (uint64_t k = 0; k < n; k++) random_state(L, seed, synth_state_id(seed, first + k, pool), rows + k * L.W);
  return RTLA_OK;
}

extern "C" int rtla_random_texts(const rtla_cfg* c, uint64_t seed, uint64_t first, uint64_t n, uint64_t pool,
                                 char* buf, size_t cap, size_t* len) {
  CFG_LAYOUT(L, c);
  if (!len || (!buf && cap)) return RTLA_E_ARG;
  // host threads, each rendering a contiguous slice of the inputs
  const int nt = (int)std::min<uint64_t>(std::max<uint64_t>(n / 256, 1), (uint64_t)text_threads(0));
  std::vector<std::string> part((size_t)nt);
  auto work = [&](int t) {
    const size_t tc = state_text_cap(L);
    std::vector<uint32_t> row(L.W);
    std::vector<char> tmp(2 * tc);
    const uint64_t b = n * t / nt, e = n * (t + 1) / nt;
    std::string& out = part[(size_t)t];
    for (uint64_t k = b; k < e; k++) {
      random_state(L, seed, synth_state_id(seed, first + k, pool), row.data());
      const size_t m = state_text_into(L, row.data(), tmp.data(), tmp.data() + tc);
      out.append(tmp.data(), m);
      out.push_back('\x1e');
    }
  };
  std::vector<std::thread> pool_th;
  for (int t = 1; t < nt; t++) pool_th.emplace_back(work, t);
  work(0);
  for (auto& th : pool_th) th.join();
  size_t at = 0;
  for (auto& p : part) {
    if (at + p.size() <= cap) memcpy(buf + at, p.data(), p.size());
    at += p.size();
  }
  *len = at;
  return at <= cap ? RTLA_OK : RTLA_E_ARG;
}

// Synthetic microbench step (BASELINE configs[4]): generate input states
// [first, first + n) into the row arena on the device (k_random_rows), then
// one launch of the level kernel over them in dedup-only mode: Next,
// fingerprint, probe/insert into this context's fingerprint set, no rows kept.
// The set accumulates across calls (rtla_reset clears it).
extern "C" int rtla_synthetic_generate(rtla_ctx* x, uint64_t seed, uint64_t first, uint64_t n, uint64_t pool,
                                       uint64_t at) {
  if (!x) return RTLA_E_ARG;
  if (x->sh.size() != 1 || x->nshard != 1 || x->inited) return RTLA_E_STATE;
  if (at > x->front_cap || n > x->front_cap - at) return RTLA_E_OVERFLOW;
  HIPCHK(hipSetDevice(x->device));
  Shard& s = x->sh[0];
  HIPCHK(launch_random_rows(x->L, seed, first, n, pool, s.arena + at * (uint64_t)x->L.W, x->stream));
  HIPCHK(hipStreamSynchronize(x->stream));
  return RTLA_OK;
}

// One dedup-only level-kernel launch over arena rows [begin, end).
extern "C" int rtla_synthetic_dedup(rtla_ctx* x, uint64_t begin, uint64_t end, rtla_level_stats* st) {
  if (!x || !st || begin > end || begin % 64) return RTLA_E_ARG;  // level-kernel groups start at multiples of 64
  if (x->sh.size() != 1 || x->nshard != 1 || x->inited) return RTLA_E_STATE;
  if (end > x->front_cap) return RTLA_E_OVERFLOW;
  const double t0 = now_s();
  HIPCHK(hipSetDevice(x->device));
  Shard& s = x->sh[0];
  HIPCHK(hipMemsetAsync(s.ctr, 0, offsetof(DevCounters, cover), x->stream));
  s.h_caps[0] = end; s.h_caps[1] = 0; s.h_caps[2] = s.parents_cap;
  HIPCHK(hipMemcpyAsync(&s.ctr->cap_cur, s.h_caps, sizeof s.h_caps, hipMemcpyHostToDevice, x->stream));
  const Ring ring{s.arena, 0, x->front_cap};
  HIPCHK(hipEventRecord(s.ev0, x->stream));
  HIPCHK(launch_expand({.L = x->L,
                        .cur = ring,
                        .s_begin = begin,
                        .s_end = end,
                        .out = {ring, s.parents, 0, 0},
                        .table = s.table,
                        .tlog2 = x->tlog2,
                        .ctr = s.ctr,
                        .st = x->stream,
                        .xflags = env_xflags() | XF_DEDUP_ONLY,
                        .grid = x->grid}));
  HIPCHK(hipEventRecord(s.ev1, x->stream));
  DevCounters h;
  HIPCHK(hipMemcpyAsync(&h, s.ctr, sizeof h, hipMemcpyDeviceToHost, x->stream));
  HIPCHK(hipStreamSynchronize(x->stream));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, s.ev0, s.ev1));
  print_stamps(h, 0);
  memset(st, 0, sizeof *st);
  st->frontier = end - begin; st->new_states = h.next_count; st->generated = h.generated; st->probes = h.probes;
  st->kernel_ms = ms; st->expand_ms = ms; st->row_bytes = (uint64_t)x->L.W * 4; st->flags = h.flags;
  st->seconds = now_s() - t0;
  if (h.flags) {
    report_flags(h.flags);
    return flags_to_status(h.flags);
  }
  return RTLA_OK;
}

extern "C" int rtla_synthetic_step(rtla_ctx* x, uint64_t seed, uint64_t first, uint64_t n, uint64_t pool,
                                   rtla_level_stats* st) {
  if (!st) return RTLA_E_ARG;
  const int rc = rtla_synthetic_generate(x, seed, first, n, pool, 0);
  return rc < 0 ? rc : rtla_synthetic_dedup(x, 0, n, st);
}

// Diagnostic: re-expand the current frontier `reps` times with the given
// k_expand_lane switches (XF_*) and report the mean device time per launch.
// Successors are inserted into the fingerprint set (so later reps find them
// seen) and written to the idle frontier buffer: call it only at the end of
// a search, never between rtla_step calls whose results matter.
extern "C" int rtla_time_expand(rtla_ctx* x, int xflags, int reps, double* ms) {
  if (!x || reps < 1 || !ms) return RTLA_E_ARG;
  if (x->sh.size() != 1 || x->nshard != 1) return RTLA_E_STATE;
  HIPCHK(hipSetDevice(x->device));
  Shard& s = x->sh[0];
  const uint64_t next_base = s.cur_base + s.n_cur;
  if (next_base >= s.parents_cap) return RTLA_E_OVERFLOW;
  const uint64_t next_cap = std::min<uint64_t>(next_room(x, s), s.parents_cap - next_base);
  float total = 0.f;
  for (int r = 0; r < reps; r++) {
    HIPCHK(hipMemsetAsync(s.ctr, 0, offsetof(DevCounters, cover), x->stream));
    HIPCHK(hipEventRecord(s.ev0, x->stream));
    HIPCHK(launch_expand({.L = x->L,
                          .cur = cur_ring(x, s),
                          .s_end = s.n_cur,
                          .cur_base = s.cur_base,
                          .out = {next_ring(x, s), s.parents, next_base, next_cap},
                          .table = s.table,
                          .tlog2 = x->tlog2,
                          .ctr = s.ctr,
                          .st = x->stream,
                          .xflags = xflags,
                          .grid = x->grid}));
    HIPCHK(hipEventRecord(s.ev1, x->stream));
    HIPCHK(hipEventSynchronize(s.ev1));
    float m = 0.f;
    HIPCHK(hipEventElapsedTime(&m, s.ev0, s.ev1));
    total += m;
  }
  *ms = total / reps;
  return RTLA_OK;
}

// ---- calibration of the fingerprint-set probe (no context).  The table, the
// counters and the events of a run: released on every way out.
namespace {
struct ProbeRig {
  int log2;
  uint64_t* table = nullptr;
  DevCounters* ctr = nullptr;
  hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
  explicit ProbeRig(int log2_) : log2(log2_) {}
  ~ProbeRig() {
    for (auto& v : e)
      if (v) (void)hipEventDestroy(v);
    if (table) (void)hipFree(table);
    if (ctr) (void)hipFree(ctr);
  }
  int clear(bool table_too) {
    if (table_too) HIPCHK(hipMemset(table, 0, 8ull << log2));
    HIPCHK(hipMemset(ctr, 0, sizeof(DevCounters)));
    return RTLA_OK;
  }
  int open(int events) {
    HIPCHK(hipMalloc(&table, 8ull << log2));
    HIPCHK(hipMalloc(&ctr, sizeof(DevCounters)));
    if (int rc = clear(true)) return rc;
    for (int k = 0; k < events; k++) HIPCHK(hipEventCreate(&e[k]));
    return RTLA_OK;
  }
  // seconds between events k and k + 1 (once the last event was reached), and the counters
  int result(int k, double* seconds, DevCounters* h) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e[k], e[k + 1]));
    if (seconds) *seconds = ms / 1e3;
    if (h) HIPCHK(hipMemcpy(h, ctr, sizeof *h, hipMemcpyDeviceToHost));
    return RTLA_OK;
  }
};
}  // namespace

// n random keys inserted (all new, CAS): device seconds.
extern "C" int rtla_probe_bench(int log2, uint64_t n, double* seconds, uint64_t* inserted) {
  ProbeRig g(log2);
  if (int rc = g.open(2)) return rc;
  HIPCHK(launch_probe_bench(g.table, log2, n / 8, 12345, g.ctr, nullptr));  // warm
  if (int rc = g.clear(true)) return rc;
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipEventRecord(g.e[0], nullptr));
  HIPCHK(launch_probe_bench(g.table, log2, n, 777, g.ctr, nullptr));
  HIPCHK(hipEventRecord(g.e[1], nullptr));
  HIPCHK(hipEventSynchronize(g.e[1]));
  DevCounters h;
  if (int rc = g.result(0, seconds, &h)) return rc;
  if (inserted) *inserted = h.next_count;
  return h.flags & FLAG_FPSET_FULL ? RTLA_E_OVERFLOW : RTLA_OK;
}

// n random keys inserted (all new, CAS), then the same n keys probed again
// (all present) with a CAS and with the load-first protocol the BFS kernel
// uses.  Device seconds of each pass.
extern "C" int rtla_probe_bench2(int log2, uint64_t n, double* s_insert, double* s_seen_cas, double* s_seen_load,
                                 uint64_t* inserted) {
  ProbeRig g(log2);
  if (int rc = g.open(4)) return rc;
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipEventRecord(g.e[0], nullptr));
  HIPCHK(launch_probe_bench(g.table, log2, n, 777, g.ctr, nullptr, 0));
  HIPCHK(hipEventRecord(g.e[1], nullptr));
  HIPCHK(launch_probe_bench(g.table, log2, n, 777, g.ctr, nullptr, 0));
  HIPCHK(hipEventRecord(g.e[2], nullptr));
  HIPCHK(launch_probe_bench(g.table, log2, n, 777, g.ctr, nullptr, 1));
  HIPCHK(hipEventRecord(g.e[3], nullptr));
  HIPCHK(hipEventSynchronize(g.e[3]));
  DevCounters h;
  double* out[3] = {s_insert, s_seen_cas, s_seen_load};
  for (int k = 0; k < 3; k++)
    if (int rc = g.result(k, out[k], k == 2 ? &h : nullptr)) return rc;
  if (inserted) *inserted = h.next_count;  // the two re-probe passes insert nothing
  return h.flags & FLAG_FPSET_FULL ? RTLA_E_OVERFLOW : RTLA_OK;
}

// n keys, a fraction new_frac of them new, probed into a table holding n_present keys: device seconds.
extern "C" int rtla_probe_bench3(int log2, uint64_t n_present, uint64_t n, double new_frac, double* seconds,
                                 uint64_t* inserted) {
  if (log2 < 16 || log2 > 36 || !n || n_present >= (1ull << log2)) return RTLA_E_ARG;
  if (seconds) *seconds = 0;
  if (inserted) *inserted = 0;
  ProbeRig g(log2);
  if (int rc = g.open(2)) return rc;
  HIPCHK(launch_probe_bench(g.table, log2, n_present, 777, g.ctr, nullptr, 0));  // the present keys (untimed)
  if (int rc = g.clear(false)) return rc;
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipEventRecord(g.e[0], nullptr));
  HIPCHK(launch_probe_mixed(g.table, log2, n, n_present, new_frac, 777, g.ctr, nullptr));
  HIPCHK(hipEventRecord(g.e[1], nullptr));
  HIPCHK(hipEventSynchronize(g.e[1]));
  DevCounters h;
  if (int rc = g.result(0, seconds, &h)) return rc;
  if (inserted) *inserted = h.next_count;
  return h.flags & FLAG_FPSET_FULL ? RTLA_E_OVERFLOW : RTLA_OK;
}

// The device insert functions on caller-chosen fingerprints (the tests' seam
// to the fingerprint set): the table goes up, input i is inserted by global
// thread i of k_fpset_probe -- or (protocol 3) the inputs by k_insert_remote
// as the exchange launches it --, the table comes back.
namespace {
struct DevBuf {  // a device allocation released on every way out
  void* p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};
}  // namespace

extern "C" int rtla_fpset_probe(int log2, const uint64_t* fps, size_t n, int protocol, uint64_t* table,
                                uint8_t* is_new, int32_t* flags) {
  if (log2 < 10 || log2 > 30 || protocol < 0 || protocol > 3 || !table || !flags || n > (1ull << 31) ||
      (n && (!fps || !is_new)))
    return RTLA_E_ARG;
  *flags = 0;
  ProbeRig g(log2);
  if (int rc = g.open(0)) return rc;
  DevBuf d_fps, d_new;
  HIPCHK(hipMalloc(&d_fps.p, std::max<size_t>(n, 1) * 16));
  HIPCHK(hipMalloc(&d_new.p, std::max<size_t>(n, 1)));
  HIPCHK(hipMemcpy(g.table, table, 8ull << log2, hipMemcpyHostToDevice));
  if (n) HIPCHK(hipMemcpy(d_fps.p, fps, n * 16, hipMemcpyHostToDevice));
  HIPCHK(hipMemset(d_new.p, 0, std::max<size_t>(n, 1)));
  if (protocol == 3) {  // the exchange's owner side itself: the inputs as one sender's region of n records
    DevBuf d_count, d_ans;
    const uint64_t count = n;
    HIPCHK(hipMalloc(&d_count.p, 8));
    HIPCHK(hipMalloc(&d_ans.p, std::max<size_t>(n, 1) * 4));
    HIPCHK(hipMemcpy(d_count.p, &count, 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_ans.p, 0, std::max<size_t>(n, 1) * 4));
    HIPCHK(launch_insert_remote((const uint64_t*)d_fps.p, (const uint64_t*)d_count.p, 1, n, g.table, log2,
                                (uint32_t*)d_ans.p, g.ctr, n, nullptr));
    HIPCHK(hipDeviceSynchronize());
    std::vector<uint32_t> ans(n);
    if (n) HIPCHK(hipMemcpy(ans.data(), d_ans.p, n * 4, hipMemcpyDeviceToHost));
    for (size_t k = 0; k < n; k++) is_new[k] = ans[k] ? 1 : 0;
  } else {
    HIPCHK(launch_fpset_probe(g.table, log2, (const uint64_t*)d_fps.p, n, protocol, (unsigned char*)d_new.p, g.ctr,
                              nullptr));
    HIPCHK(hipDeviceSynchronize());
    if (n) HIPCHK(hipMemcpy(is_new, d_new.p, n, hipMemcpyDeviceToHost));
  }
  DevCounters h;
  HIPCHK(hipMemcpy(&h, g.ctr, sizeof h, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(table, g.table, 8ull << log2, hipMemcpyDeviceToHost));
  *flags = h.flags;
  return h.flags & FLAG_FPSET_FULL ? RTLA_E_OVERFLOW : RTLA_OK;
}
