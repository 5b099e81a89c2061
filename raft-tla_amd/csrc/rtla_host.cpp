// rtla_host.cpp -- the C-ABI driver (include/rtla.h) around the HIP kernels:
// contexts, the BFS level step, the multi-shard exchange protocol, frontier
// access and traces.  (The other host units: rtla_ctx.h.)
//
// A context owns one or more SHARDS.  A shard is the unit of fingerprint
// ownership: it holds the part of the fingerprint set whose fingerprints it
// owns (fp_owner, rtla_device.h), the states it materialised (frontier double
// buffer) and their parent pointers.  Device memory per shard:
//   fingerprint set   2^fpset_log2 x 8 B   (open addressing, CAS insert)
//   parents           one u64 per state: its parent record (parent_record, rtla_device.h: the parent's shard in
//                     bits 56-63, its index in bits 16-55, the action instance in bits 0-15)
//   row arena         frontier_cap rows (a multiple of 64), used as a ring: the
//                     current level's rows, then the next level's after them
//   outbox / inbox    (multi-shard only) per destination: fingerprints, refs, answers
//
// Deployments:
//   world == 1, shards <= 1 : the whole search in one shard; one fused k_expand
//                             launch per BFS level (expand + probe + insert +
//                             materialise + invariants).
//   world == N (one process per GPU, RCCL over xGMI): one shard per rank.
//   world == 1, shards == S : S shards on one GPU, exchanging by device copies
//                             -- the multi-GPU protocol exercised on one device;
//                             with RTLA_TRANSPORT=rccl the same exchange runs
//                             through a one-rank RCCL communicator instead
//                             (every ncclSend/ncclRecv to self, the count
//                             all-gathers, the level all-reduces, the trace
//                             broadcasts): the RCCL call sites of the
//                             multi-GPU path execute on a one-GPU box.
//
// Multi-shard level: exchange rounds, all shards in lock-step (rtla_step):
//   1. k_expand_compact: successors owned locally are probed, inserted and
//      built at once; the others are queued as (fingerprint, parent ref) per
//      owner.  The kernel expands the rest of the frontier until an owner's
//      outbox region fills (its group guard), so a round is as large as the
//      outbox allows;
//   2. all-gather of the per-owner counts (+ what each shard has left) --
//      the round's only host synchronisation -- then all-to-all-v of the
//      16-byte fingerprints (ncclSend/ncclRecv pairs in one group: all 7 xGMI
//      links of an MI355X node carry traffic at once);
//   3. k_insert_remote at the owner answers each record new / seen;
//   4. all-to-all-v of the answers back;
//   5. k_build_winners: each sender builds the rows of its winners into its
//      own next level (rows never cross shards; parent records name the
//      parent's shard, so traces walk across shards).
// Then one all-reduce of {new, generated, probes, violation, flags} decides
// termination (TLC's "0 states left on queue"), and the next levels are
// re-balanced where they drifted from an even split.
#include <string>

#include "rtla_ctx.h"
#include "rtla_plan.h"

int layout_from_cfg(const rtla_cfg* c, Layout* L) {
  if (!c) return RTLA_E_ARG;
  int K = c->bag_cap ? c->bag_cap : (c->max_msgs > 0 ? c->max_msgs + 1 : 32);
  int E = c->elec_cap ? c->elec_cap : (c->max_term - 1) * c->n_server;
  if (E < 1) E = 1;
  if (make_layout(L, c->n_server, c->n_value, c->max_term, c->max_log, c->max_copies, c->max_msgs, K, E,
                  c->inv_mask) != 0)
    return RTLA_E_CONFIG;
  L->sym = c->symmetry ? 1 : 0;
  return RTLA_OK;
}

extern "C" int rtla_abi_version(void) { return RTLA_ABI_VERSION; }

extern "C" const char* rtla_strerror(int s) {
  switch (s) {
    case RTLA_OK: return "ok";
    case RTLA_DONE: return "search complete";
    case RTLA_VIOLATION: return "invariant violated";
    case RTLA_E_CONFIG: return "configuration outside the supported row format";
    case RTLA_E_HIP: return "HIP runtime error";
    case RTLA_E_OVERFLOW: return "capacity overflow (bag/elections/frontier/fingerprint set/outbox)";
    case RTLA_E_SPEC: return "TLC evaluation error in Next (index outside DOMAIN)";
    case RTLA_E_STATE: return "call out of order";
    case RTLA_E_ARG: return "bad argument";
    case RTLA_E_COMM: return "RCCL error";
    default: return "unknown status";
  }
}

void report_flags(int flags) {
  if (flags & FLAG_SPEC_ERROR) fprintf(stderr, "rtla: TLC evaluation error in Next (sequence index outside DOMAIN)\n");
  if (flags & FLAG_ROW_OVERFLOW) fprintf(stderr, "rtla: row capacity exceeded (raise bag_cap / elec_cap)\n");
  if (flags & FLAG_FRONTIER_FULL) fprintf(stderr, "rtla: next-frontier buffer full (raise frontier_cap / mem_budget)\n");
  if (flags & FLAG_FPSET_FULL) fprintf(stderr, "rtla: fingerprint set too full (raise fpset_log2)\n");
  if (flags & FLAG_OUTBOX_FULL) fprintf(stderr, "rtla: exchange outbox overflow list full\n");
  if (flags & FLAG_BAD_INDEX) fprintf(stderr, "rtla: checked build: a kernel index left its buffer\n");
  if (flags & FLAG_LOCAL_FAILURE) fprintf(stderr, "rtla: a rank's local work failed\n");
}

// RTLA_XFLAGS: kernel-variant switches (XF_* in rtla_device.h) for performance
// experiments; results are identical for the variants that do not skip work.
int env_xflags() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("RTLA_XFLAGS");
    v = e ? (atoi(e) & (XF_GENERIC_DELTA | XF_BLOCK4 | XF_NO_PERSIST | XF_CAS_ONLY | XF_WAVE_KERNEL | XF_NO_SPECIAL)) : 0;
  }
  return v;
}

// RTLA_FAULT=<where>:<rank> (tests): this rank's local work at <where> fails,
// so the tests can check that the failure reaches every rank promptly.
bool fault_here(const rtla_ctx* x, const char* where) {
  const char* e = getenv("RTLA_FAULT");
  if (!e) return false;
  const char* colon = strchr(e, ':');
  if (!colon || (size_t)(colon - e) != strlen(where) || strncmp(e, where, colon - e) != 0) return false;
  return atoi(colon + 1) == x->rank;
}

// Copy states [g, g + n) of a level to / from the host (two pieces if they wrap).
static hipError_t ring_copy(const Ring& r, int W, uint64_t g, uint64_t n, uint32_t* host, bool to_host) {
  while (n) {
    const uint64_t p = ring_idx(r, g), m = std::min<uint64_t>(n, r.cap - p);
    uint32_t* dev = r.base + p * (uint64_t)W;
    hipError_t e = to_host ? hipMemcpy(host, dev, m * W * 4, hipMemcpyDeviceToHost)
                           : hipMemcpy(dev, host, m * W * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) return e;
    host += m * (uint64_t)W;
    g += m;
    n -= m;
  }
  return hipSuccess;
}

static void free_shard(Shard& s) {
  void* ptrs[] = {s.table,    s.sent,     s.parents,  s.arena,    s.ctr,       s.dflags,    s.out_count,
                  s.in_count, s.all_count, s.send_fp, s.send_ref, s.send_ans,  s.recv_fp,   s.recv_ans,
                  s.rows_in,  s.rows_base, s.send_rows, s.recv_rows, s.over_fp[0], s.over_fp[1],
                  s.over_ref[0], s.over_ref[1], s.over_cnt};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  if (s.ev0) (void)hipEventDestroy(s.ev0);
  if (s.ev1) (void)hipEventDestroy(s.ev1);
  if (s.evm) (void)hipEventDestroy(s.evm);
  s = Shard();
}

extern "C" void rtla_close(rtla_ctx* x) {
  if (!x) return;
  (void)hipSetDevice(x->device);
  for (auto& s : x->sh) free_shard(s);
  if (x->red) (void)hipFree(x->red);
  for (void* p : {(void*)x->sim.ctr, (void*)x->sim.ends, (void*)x->sim.carry, (void*)x->sim.prog})
    if (p) (void)hipFree(p);
  if (x->sim.ev0) (void)hipEventDestroy(x->sim.ev0);
  if (x->sim.ev1) (void)hipEventDestroy(x->sim.ev1);
  if (x->audit.ctr) (void)hipFree(x->audit.ctr);
  if (x->audit.prog) (void)hipFree(x->audit.prog);
  if (x->audit.ev0) (void)hipEventDestroy(x->audit.ev0);
  if (x->audit.ev1) (void)hipEventDestroy(x->audit.ev1);
  constrain_free(x->constrain);
  comm_close(x);
  if (x->stream) (void)hipStreamDestroy(x->stream);
  delete x;
}

static int alloc_shard(rtla_ctx* x, Shard& s, uint64_t budget) {
  const Layout& L = x->L;
  const int G = x->nshard;
  uint64_t tbytes = 8ull << x->tlog2;
  // One parent record per slot of the set (RTLA_MODE_DEDUP: no BFS, no parent records): a search that
  // outgrows its set ends at the set's probe limit (RTLA_CAP_FPSET), whatever the load it reaches first.
  s.parents_cap = x->cfg.mode == RTLA_MODE_DEDUP ? 64 : 1ull << x->tlog2;
  uint64_t pbytes = s.parents_cap * 8;
  uint64_t rowb = (uint64_t)L.W * 4;
  uint64_t boxb = G > 1 ? (uint64_t)G * x->box_cap * (16 + 8 + 4 + 16 + 4) +
                              2ull * G * x->rows_cap * (L.W + 2) * 4 + 2ull * x->over_cap * 24
                        : 0;
  const uint64_t sbytes = G > 1 && x->slog2 ? 8ull << x->slog2 : 0;
  if (!x->front_cap) {
    uint64_t used = tbytes + sbytes + pbytes + boxb;
    uint64_t rest = budget > used ? budget - used : 0;
    x->front_cap = std::max<uint64_t>(rest / rowb, 2048);
  }
  x->front_cap = std::max<uint64_t>(x->front_cap & ~63ull, 128);  // whole 64-row groups (Ring)
  HIPCHK(hipMalloc(&s.table, tbytes));
  HIPCHK(hipMalloc(&s.parents, pbytes));
  HIPCHK(hipMalloc(&s.arena, x->front_cap * rowb));
  HIPCHK(hipMalloc(&s.ctr, sizeof(DevCounters)));
  HIPCHK(hipMalloc(&s.dflags, sizeof(int) * 64));
  if (G > 1) {
    HIPCHK(hipMalloc(&s.out_count, 8 * (G + 2)));
    HIPCHK(hipMalloc(&s.in_count, 8 * G));
    HIPCHK(hipMalloc(&s.all_count, 8 * G * (G + 2)));
    HIPCHK(hipMalloc(&s.send_fp, 16 * G * x->box_cap));
    HIPCHK(hipMalloc(&s.send_ref, 8 * G * x->box_cap));
    HIPCHK(hipMalloc(&s.send_ans, 4 * G * x->box_cap));
    HIPCHK(hipMalloc(&s.recv_fp, 16 * G * x->box_cap));
    HIPCHK(hipMalloc(&s.recv_ans, 4 * G * x->box_cap));
    HIPCHK(hipMalloc(&s.rows_in, 8 * G));
    HIPCHK(hipMalloc(&s.rows_base, 8 * G));
    HIPCHK(hipMalloc(&s.send_rows, 4ull * G * x->rows_cap * (L.W + 2)));
    HIPCHK(hipMalloc(&s.recv_rows, 4ull * G * x->rows_cap * (L.W + 2)));
    for (int k = 0; k < 2; k++) {
      HIPCHK(hipMalloc(&s.over_fp[k], 16 * std::max<uint64_t>(x->over_cap, 1)));
      HIPCHK(hipMalloc(&s.over_ref[k], 8 * std::max<uint64_t>(x->over_cap, 1)));
    }
    HIPCHK(hipMalloc(&s.over_cnt, 16));
    HIPCHK(hipMemsetAsync(s.over_cnt, 0, 16, x->stream));
    s.h_out.assign(G + 2, 0);
    s.h_in.assign(G, 0);
    if (sbytes) {
      HIPCHK(hipMalloc(&s.sent, sbytes));
      HIPCHK(hipMemsetAsync(s.sent, 0, sbytes, x->stream));
    }
  }
  HIPCHK(hipMemsetAsync(s.table, 0, tbytes, x->stream));
  HIPCHK(hipMemsetAsync(s.ctr, 0, sizeof(DevCounters), x->stream));
  HIPCHK(hipEventCreate(&s.ev0));
  HIPCHK(hipEventCreate(&s.ev1));
  HIPCHK(hipEventCreate(&s.evm));
  return RTLA_OK;
}

// Multi-shard exchange sizing.  Per owner, an outbox region
// of box_cap records (48 B each with the answers and the receiving side):
// ~1/10 of the budget over the G regions.  The level kernel takes frontier
// groups while every region is below stop_at; the groups in flight when one
// fills -- at most two per resident wave (the current group's tail and the
// group taken just before the guard tripped, k_expand_compact take_group),
// each of whose GROUP states may queue every action instance -- spill onto
// the overflow list (over_cap).  (A record lands past a region's end only
// from a chunk reserved after the guard tripped: chunks reserved before it
// start below stop_at, which is at least OBOX_CHUNK below the end.)
// Without the group queue (the wave-per-state kernel) a round is bounded
// instead, so that no region can overflow (chunk).  Every rank must agree on
// these (round counts and message sizes follow from them): world > 1 takes
// the smallest of each over the ranks.
static int size_exchange(rtla_ctx* x, uint64_t per) {
  const Layout& L = x->L;
  const int G = x->nshard;
  const uint64_t ninst = (uint64_t)L.fam[F_COUNT];  // records one frontier state queues at most
  int waves = 0, group = 0;
  x->guarded = level_kernel_shape(L, true, env_xflags(), &waves, &group);
  // (1/10: configs[1]'s level 17 at 2 virtual shards then fits one round -- 250.7 -> 239.7 ms; at 1/8
  // the arena of 8 virtual shards no longer holds its levels 16 + 17; profiles/r06_v5/outbox_*)
  x->box_cap = std::max<uint64_t>(per / 10 / ((uint64_t)G * 48), 16 * OBOX_CHUNK);
  if (const char* e = getenv("RTLA_OUTBOX_CAP"))  // tests: tiny regions, many rounds, the overflow list in use
    if (atoll(e) > 0) x->box_cap = std::max<uint64_t>((uint64_t)atoll(e), 16 * OBOX_CHUNK);
  if (x->cfg.chunk) x->chunk = round64(x->cfg.chunk);  // explicit bound on the states a round expands
  else x->chunk = x->guarded ? 0 : std::max<uint64_t>(64, (x->box_cap / ninst) & ~63ull);
  x->over_cap = x->guarded ? 2ull * (uint64_t)waves * (uint64_t)group * ninst : 0;
  // the two overflow lists (24 B a record) take at most 1/16 of the budget: a
  // small budget bounds the states a round expands instead, so that even
  // then every record of a launch would fit the list
  const uint64_t over_room = std::max<uint64_t>(per / 16 / 48, 64 * ninst);
  if (x->over_cap > over_room) {
    x->over_cap = over_room;
    const uint64_t c = std::max<uint64_t>(64, (over_room / ninst) & ~63ull);
    x->chunk = x->chunk ? std::min(x->chunk, c) : c;
  }
  // re-balancing staging: ~1/20 of the budget; more rows move in sub-rounds
  x->rows_cap = (per / 20) / (2ull * G * (L.W + 2) * 4);
  x->rows_cap = std::min<uint64_t>(std::max<uint64_t>(x->rows_cap, 256), x->box_cap);
  if (const char* e = getenv("RTLA_ROWS_CAP"))  // tests: tiny staging, every re-balancing move in sub-rounds
    if (atoll(e) > 0) x->rows_cap = std::min<uint64_t>((uint64_t)atoll(e), x->box_cap);
  if (x->world > 1) {  // min over the ranks (max of the complements); the overflow bound: max
    uint64_t v[5] = {~x->box_cap, ~(x->chunk ? x->chunk : ~0ull), ~x->rows_cap, x->over_cap, x->guarded ? 0ull : 1ull};
    if (int rc = allreduce_u64(x, v, 5, 1)) return rc;
    x->box_cap = ~v[0];
    x->chunk = ~v[1] == ~0ull ? 0 : ~v[1];
    x->rows_cap = ~v[2];
    x->over_cap = v[3];
    if (v[4] && x->guarded) {  // some rank runs the wave-per-state kernel: all bound their rounds alike
      x->guarded = false;
      if (!x->chunk) x->chunk = std::max<uint64_t>(64, (x->box_cap / ninst) & ~63ull);
    }
    // an agreed state bound per round also bounds every rank's overflow: no rank
    // allocates past its own budget share for a larger peer's list
    if (x->chunk && x->over_cap) x->over_cap = std::min(x->over_cap, x->chunk * ninst);
  }
  x->stop_at = x->box_cap - std::max<uint64_t>(x->box_cap / 8, OBOX_CHUNK);
  // owners by projection (rtla_model.h proj32) keep most successors on their
  // parent's owner only if states live at their owner: winners are re-homed
  // (RTLA_REHOME=0: kept by their sender, the round-5 protocol; A/B runs).
  // SYMMETRY owns by orbit key, which no action preserves: nothing to gain.
  const char* rh = getenv("RTLA_REHOME");
  x->rehome = G > 1 && !L.sym && x->rows_cap > 0 && !(rh && !strcmp(rh, "0"));
  return RTLA_OK;
}

extern "C" int rtla_open(const rtla_cfg* cfg, int rank, int world, const void* comm_id, rtla_ctx** out) {
  if (!cfg || !out || world < 1 || rank < 0 || rank >= world) return RTLA_E_ARG;
  *out = nullptr;
  if (world > 1 && !comm_id) return RTLA_E_ARG;
  if (world > 1 && cfg->shards > 1) return RTLA_E_CONFIG;
  if (world > SHARD_MAX || cfg->shards > SHARD_MAX) return RTLA_E_CONFIG;  // per-owner outbox state is sized by it
  if (cfg->mode != RTLA_MODE_BFS && (cfg->mode != RTLA_MODE_DEDUP || world > 1 || cfg->shards > 1))
    return RTLA_E_CONFIG;
  rtla_ctx* x = new rtla_ctx();
  x->cfg = *cfg;
  int r = layout_from_cfg(cfg, &x->L);
  if (r) { delete x; return r; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { delete x; return RTLA_E_HIP; }
  x->rank = rank;
  x->world = world;
  x->device = rank % ndev;
  x->nshard = world > 1 ? world : std::max(1, cfg->shards);
  x->shard0 = world > 1 ? rank : 0;
  int nlocal = world > 1 ? 1 : x->nshard;
  if (hipSetDevice(x->device) != hipSuccess) { delete x; return RTLA_E_HIP; }
  if (hipStreamCreateWithFlags(&x->stream, hipStreamNonBlocking) != hipSuccess) { delete x; return RTLA_E_HIP; }
  if (hipMalloc(&x->red, RED_WORDS * 8) != hipSuccess) { rtla_close(x); return RTLA_E_HIP; }
  if (comm_open(x, comm_id) != RTLA_OK) { rtla_close(x); return RTLA_E_COMM; }
  // From here on (world > 1) every rank reaches the same collectives: a local
  // failure is carried to the last one, which fails every rank together.
  int err = RTLA_OK;
  size_t free_b = 0, total_b = 0;
  (void)hipMemGetInfo(&free_b, &total_b);
  uint64_t budget = cfg->mem_budget ? cfg->mem_budget : (uint64_t)(free_b * 0.85);
  uint64_t per = budget / nlocal;
  const Layout& L = x->L;
  const int G = x->nshard;
  if (G > 1)
    if (int rc = size_exchange(x, per)) { rtla_close(x); return rc; }
  int tl = cfg->fpset_log2;
  if (!tl) {
    tl = 20;
    // the fingerprint set (multi-shard: + the sent cache, half its size): ~40% of the budget
    const uint64_t tshare = G > 1 ? per * 4 / 15 : per * 2 / 5;
    while (tl < 34 && (8ull << (tl + 1)) <= tshare) tl++;
  }
  if (tl < 10 || tl > 40) err = RTLA_E_CONFIG;
  x->tlog2 = tl;
  // the sent cache is a dedup hint (one slot per fingerprint, overwritten on
  // a miss): half the set's slots (configs[1], 8 shards: a quarter sends 8 %
  // more records and takes 5 % longer, profiles/r05_v2); RTLA_SENT_CACHE=0
  // turns it off (every remote successor is queued for its owner: 1.34x slower)
  const char* sc = getenv("RTLA_SENT_CACHE");
  x->slog2 = sc && atoi(sc) == 0 ? 0 : std::max(12, tl - 1);
  if (const char* sl = getenv("RTLA_SENT_LOG2"))  // experiments: the sent cache's size (log2 slots)
    if (x->slog2 && atoi(sl) >= 12 && atoi(sl) <= 36) x->slog2 = atoi(sl);
  x->front_cap = cfg->frontier_cap;
  x->sh.resize(nlocal);
  for (int k = 0; k < nlocal && !err; k++) {
    x->sh[k].id = x->shard0 + k;
    if (alloc_shard(x, x->sh[k], per) != RTLA_OK) {
      fprintf(stderr, "rtla: device allocation failed (fpset 2^%d slots, frontier 2x%llu rows of %d B)\n", tl,
              (unsigned long long)x->front_cap, L.W * 4);
      err = RTLA_E_HIP;
    }
  }
  if (!err && (hipStreamSynchronize(x->stream) != hipSuccess || fault_here(x, "open"))) err = RTLA_E_HIP;
  if (world > 1) {  // every rank opened, or none
    uint64_t bad = err ? 1 : 0;
    if (int rc = allreduce_u64(x, &bad, 1, 1)) err = err ? err : rc;
    else if (bad && !err) err = RTLA_E_COMM;
  }
  if (err) {
    rtla_close(x);
    return err;
  }
  hipDeviceProp_t prop;
  (void)hipGetDeviceProperties(&prop, x->device);
  x->grid = prop.multiProcessorCount * expand_blocks_per_cu(L) * 2;
  *out = x;
  return RTLA_OK;
}

extern "C" int rtla_device_info(rtla_ctx* x, char* buf, size_t cap) {
  if (!x || !buf) return RTLA_E_ARG;
  std::string fr;  // this process's shards' current levels
  for (auto& s : x->sh) fr += (fr.empty() ? "" : ", ") + std::to_string(s.n_cur);
  hipDeviceProp_t p;
  HIPCHK(hipGetDeviceProperties(&p, x->device));
  snprintf(buf, cap,
           "{\"device\": \"%s\", \"arch\": \"%s\", \"cus\": %d, \"rank\": %d, \"world\": %d, \"shards\": %d, "
           "\"fpset_slots_log2\": %d, \"frontier_cap\": %llu, \"row_words\": %d, \"grid\": %d, \"chunk\": %llu, "
           "\"transport\": \"%s\", \"sent_cache_slots_log2\": %d, \"rebalanced_rows\": %llu, "
           "\"outbox_records_per_owner\": %llu, \"overflow_records\": %llu, \"exchange_rounds\": %llu, "
           "\"overflowed_records\": %llu, \"records_sent\": %llu, \"rehomed_rows\": %llu, \"shard_frontier\": [%s]}",
           p.name, p.gcnArchName, p.multiProcessorCount, x->rank, x->world, x->nshard, x->tlog2,
           (unsigned long long)x->front_cap, x->L.W, x->grid, (unsigned long long)x->chunk, comm_name(x),
           x->nshard > 1 ? x->slog2 : 0, (unsigned long long)x->rebalanced, (unsigned long long)x->box_cap,
           (unsigned long long)x->over_cap, (unsigned long long)x->rounds, (unsigned long long)x->overflowed,
           (unsigned long long)x->records, (unsigned long long)x->rehomed, fr.c_str());
  return RTLA_OK;
}

extern "C" int rtla_reset(rtla_ctx* x) {
  if (!x) return RTLA_E_ARG;
  HIPCHK(hipSetDevice(x->device));
  for (auto& s : x->sh) {
    HIPCHK(hipMemsetAsync(s.table, 0, 8ull << x->tlog2, x->stream));
    if (s.sent) HIPCHK(hipMemsetAsync(s.sent, 0, 8ull << x->slog2, x->stream));
    HIPCHK(hipMemsetAsync(s.ctr, 0, sizeof(DevCounters), x->stream));
    s.n_cur = 0; s.cur_base = 0; s.cur_start = 0;
    s.viol_mask = 0; s.viol_in_model = 0; s.viol_inst = -1; s.viol_parent = 0; s.viol_child = ~0ull;
  }
  HIPCHK(hipStreamSynchronize(x->stream));
  x->inited = false; x->finished = false; x->level = 0; x->distinct = 0; x->generated = 0; x->max_front = 0;
  x->sim.viol = false;
  x->audit.viol = false;
  x->roots.clear();
  x->seeded = false;
  return RTLA_OK;
}

// Level 1 of a search: the n rows of `rows` (Init alone, or rtla_init_rows's) become its roots.  Each gets the
// fingerprint a generated state carries (its own, from scratch) and a seen-set key: that fingerprint -- or, for
// the rows of a seeded SYMMETRY search, the orbit key the level kernel probes with.  (Init keeps its fingerprint
// there too: it is its orbit's only member, and no action leads back to it.)  Roots equal by key count once.
// Root k lives on the shard that owns its key, after the roots before it, with the parent record root_record(k).
static int seed_level(rtla_ctx* x, const uint32_t* rows, size_t n, bool seeded, rtla_level_stats* st) {
  const double t0 = now_s();
  HIPCHK(hipSetDevice(x->device));
  const Layout& L = x->L;
  const size_t W = (size_t)L.W;
  std::vector<uint32_t> roots;
  std::vector<FP> keys;
  std::set<std::pair<uint64_t, uint64_t>> seen;
  for (size_t k = 0; k < n; k++) {
    std::vector<uint32_t> row(rows + k * W, rows + (k + 1) * W);
    if (row_nmsg(L, row.data()) > L.K || row_nelec(L, row.data()) > L.E) return RTLA_E_ARG;  // no row of this layout
    row_set_fp(row.data(), row_fingerprint(L, row.data()));
    const FP key = seeded && L.sym
                       ? dispatch_n(L, [&](auto ns) { return orbit_key_row<decltype(ns)::value>(L, row.data()); })
                       : row_fp(row.data());
    if (!seen.insert({key.a, key.b}).second) continue;
    roots.insert(roots.end(), row.begin(), row.end());
    keys.push_back(key);
  }
  const size_t nroot = keys.size();
  // per local shard: its roots in the given order, and the same rows carrying their keys (what k_insert_rows reads)
  struct Part {
    std::vector<uint32_t> rows, keyed;
    std::vector<uint64_t> recs;
  };
  std::vector<Part> part(x->sh.size());
  std::vector<std::pair<int, uint64_t>> home(nroot, {-1, 0});  // root -> (local shard, its index there)
  for (size_t k = 0; k < nroot; k++) {
    const int owner = fp_owner(keys[k], x->nshard);
    for (size_t q = 0; q < x->sh.size(); q++) {
      if (x->sh[q].id != owner) continue;
      Part& p = part[q];
      home[k] = {(int)q, p.recs.size()};
      p.rows.insert(p.rows.end(), roots.begin() + k * W, roots.begin() + (k + 1) * W);
      p.keyed.insert(p.keyed.end(), roots.begin() + k * W, roots.begin() + (k + 1) * W);
      row_set_fp(p.keyed.data() + p.keyed.size() - W, keys[k]);
      p.recs.push_back(root_record(k));
    }
  }
  uint64_t largest = 0;
  for (size_t q = 0; q < x->sh.size(); q++) {
    largest = std::max<uint64_t>(largest, part[q].recs.size());
    if (part[q].recs.size() > std::min(x->front_cap, x->sh[q].parents_cap)) return RTLA_E_OVERFLOW;
  }
  for (size_t q = 0; q < x->sh.size(); q++) {
    Shard& s = x->sh[q];
    const Part& p = part[q];
    const uint64_t m = p.recs.size();
    s.cur_start = 0; s.cur_base = 0; s.n_cur = 0;
    if (!m) continue;
    HIPCHK(hipMemcpyAsync(s.arena, p.keyed.data(), m * W * 4, hipMemcpyHostToDevice, x->stream));
    for (uint64_t b = 0; b < m; b += 64)  // (s.dflags holds 64 answers)
      HIPCHK(launch_insert_rows(L, s.arena + b * W, std::min<uint64_t>(64, m - b), s.table, x->tlog2, s.dflags, s.ctr,
                                x->stream));
    if (seeded && L.sym) HIPCHK(hipMemcpyAsync(s.arena, p.rows.data(), m * W * 4, hipMemcpyHostToDevice, x->stream));
    HIPCHK(hipMemcpyAsync(s.parents, p.recs.data(), m * 8, hipMemcpyHostToDevice, x->stream));
    s.n_cur = m;
  }
  HIPCHK(hipStreamSynchronize(x->stream));
  for (auto& s : x->sh) {  // (the next level's set-up clears the counters: a full set is reported here)
    int flags = 0;
    HIPCHK(hipMemcpy(&flags, &s.ctr->flags, sizeof flags, hipMemcpyDeviceToHost));
    if (flags) {
      report_flags(flags);
      return flags_to_status(flags);
    }
  }
  x->roots = std::move(roots);
  x->seeded = seeded;
  x->level = 1; x->distinct = nroot; x->generated = n; x->inited = true; x->max_front = largest;
  int status = RTLA_OK;
  for (size_t k = 0; k < nroot && status == RTLA_OK; k++) {
    const int bad = check_invariants<0>(L, x->roots.data() + k * W, (const Delta*)nullptr);
    if (!bad) continue;
    if (home[k].first >= 0) {
      Shard& s = x->sh[(size_t)home[k].first];
      s.viol_mask = bad; s.viol_in_model = 1; s.viol_child = home[k].second; s.viol_inst = -1;
    }
    x->finished = true;
    status = RTLA_VIOLATION;
  }
  if (st) {
    memset(st, 0, sizeof *st);
    st->level = 1; st->status = status; st->new_states = nroot; st->generated = n;
    st->distinct_total = nroot; st->generated_total = n; st->seconds = now_s() - t0;
    st->row_bytes = (uint64_t)L.W * 4;
  }
  return status;
}

extern "C" int rtla_init(rtla_ctx* x, rtla_level_stats* st) {
  if (!x) return RTLA_E_ARG;
  if (x->inited || x->cfg.mode == RTLA_MODE_DEDUP) return RTLA_E_STATE;
  std::vector<uint32_t> init((size_t)x->L.W, 0);
  row_init(x->L, init.data());  // (raft.tla:155-160: one state)
  return seed_level(x, init.data(), 1, false, st);
}

extern "C" int rtla_init_rows(rtla_ctx* x, const uint32_t* rows, size_t n, rtla_level_stats* st) {
  if (!x) return RTLA_E_ARG;
  if (x->inited || x->cfg.mode == RTLA_MODE_DEDUP || x->world > 1) return RTLA_E_STATE;
  if (!rows || n == 0) return RTLA_E_ARG;
  return seed_level(x, rows, n, true, st);
}

// ---- multi-shard exchange (the transport -- device copies for local shards,
// RCCL or shared memory across ranks -- is Exchange's business, rtla_comm.cpp)
//
// Two-phase: only fingerprints and answers cross shards.
// One exchange round: the level kernel queues (fingerprint, parent) records
// of successors other shards own; ONE host synchronisation learns every
// (sender, owner) record count, which sizes the fingerprint transfer and the
// answers coming back; the owners insert and answer new / seen; each sender
// builds its winners into its own next level (k_build_winners).  At the
// level's end the shards' next levels are re-balanced (rebalance) -- the only
// rows that ever move, and only what drifted from an even split.

// One rtla_step's state: per local shard, where its next level goes.
struct Level {
  std::vector<uint64_t> next_base, next_cap;
  // capacity shortfalls and local failures travel in the level's reduction like the kernels' flags
  // (a rank returning before the collectives would leave the others waiting in them)
  int lflags = 0;
  std::vector<DevCounters> hc;  // the shards' counters, read back at the level's end
  double emax = 0.0;            // probe-kernel (k_expand_*) time of this level, ms
};

// Where local shard k's new states of the level go.
static FrontierOut frontier_out(const rtla_ctx* x, const Level& lv, size_t k) {
  const Shard& s = x->sh[k];
  return FrontierOut{next_ring(x, s), s.parents, lv.next_base[k], lv.next_cap[k]};
}

// The row staging regions ([G][rows_cap][W + 2]): what s exports to peer p, what it received from p.
static uint32_t* export_region(const rtla_ctx* x, const Shard& s, int p) {
  return s.send_rows + (uint64_t)p * x->rows_cap * ((uint64_t)x->L.W + 2);
}
static uint32_t* staging_region(const rtla_ctx* x, const Shard& s, int p) {
  return s.recv_rows + (uint64_t)p * x->rows_cap * ((uint64_t)x->L.W + 2);
}
// Records shard a sends owner b this round (gather_counts; reservations past
// a region's end are on the overflow list: counted up to box_cap).
static uint64_t round_records(const rtla_ctx* x, int a, int b) {
  return a == b ? 0 : std::min(x->h_rows[(size_t)a * (x->nshard + 2) + b], x->box_cap);
}

// (1) The round's one synchronisation: every shard's out_count row (records
// reserved per owner, frontier states left, overflow records) -> x->h_rows
// on every rank; h_out[p] = records this shard sends owner p, h_in[p] =
// records it receives from p; in_count on the device.
static int gather_counts(rtla_ctx* x) {
  const int G = x->nshard, RW = G + 2;
  if (int rc = comm_gather_rows(x)) return rc;
  for (auto& s : x->sh)
    for (int p = 0; p < G; p++) {
      s.h_out[p] = std::min(x->h_rows[(size_t)s.id * RW + p], x->box_cap);
      s.h_in[p] = std::min(x->h_rows[(size_t)p * RW + s.id], x->box_cap);
    }
  // h_in stays untouched until the next round's synchronisation
  for (auto& s : x->sh) HIPCHK(hipMemcpyAsync(s.in_count, s.h_in.data(), 8 * G, hipMemcpyHostToDevice, x->stream));
  return RTLA_OK;
}

// (2) The round's two all-to-all-v (sizes known since gather_counts: no
// synchronisation).  Out: the queued 16-byte fingerprint records, send_fp ->
// their owners' recv_fp.  Back (`answers`): what the owners answered in
// recv_ans (4 bytes; 0 = seen, nonzero = new) -> the senders' send_ans.
// Transfers are listed by receiving shard, then by sending shard.
static int move_records(rtla_ctx* x, bool answers) {
  const uint64_t cap = x->box_cap;
  Exchange ex(x);
  for (int to = 0; to < x->nshard; to++)
    for (int from = 0; from < x->nshard; from++) {
      const uint64_t n = answers ? round_records(x, to, from) : round_records(x, from, to);
      if (!n) continue;
      Shard* s = x->local(from);
      Shard* d = x->local(to);
      const uint64_t at_s = (uint64_t)to * cap, at_d = (uint64_t)from * cap;  // the peer's region of each buffer
      const void* src = !s ? nullptr : answers ? (void*)(s->recv_ans + at_s) : s->send_fp + 2 * at_s;
      void* dst = !d ? nullptr : answers ? (void*)(d->send_ans + at_d) : d->recv_fp + 2 * at_d;
      if (int rc = ex.move(from, src, to, dst, (answers ? 4 : 16) * n)) return rc;
    }
  return ex.flush();
}

// Unpack the rows staged in `rows` (per region p: h_reb[p] rows for slots
// from h_reb[SHARD_MAX + p]) into local shard k's next level.
static int unpack_staged(rtla_ctx* x, const Level& lv, size_t k, const uint32_t* rows, uint64_t most) {
  Shard& s = x->sh[k];
  const int G = x->nshard;
  HIPCHK(hipMemcpyAsync(s.rows_in, s.h_reb, 8 * G, hipMemcpyHostToDevice, x->stream));
  HIPCHK(hipMemcpyAsync(s.rows_base, s.h_reb + SHARD_MAX, 8 * G, hipMemcpyHostToDevice, x->stream));
  HIPCHK(launch_unpack_rows(x->L.W, rows, s.rows_in, s.rows_base, G, x->rows_cap, frontier_out(x, lv, k), s.ctr, most,
                            x->stream));
  return RTLA_OK;
}

// Level end, re-homing (owners by projection, x->rehome): the winners each
// shard built for owner b during the level's rounds sit in its export region
// b (k_build_winners, rows in the k_unpack_rows format with their parent
// records); they move to b and join b's next level there, so that the state
// is expanded by the shard that owns most of its successors.  The plan
// (plan_rehome) is computed alike on every rank from the level reduction
// (expm[a][b] = rows a exported for b, room[b] = b's next-level room): a
// transfer b has no room for is unpacked into a's own next level instead; if
// neither has room the level is reported incomplete (RTLA_CAP_FRONTIER), on
// every rank.
static int rehome(rtla_ctx* x, const Level& lv, std::vector<uint64_t>& n, const uint64_t* expm, const uint64_t* room) {
  std::vector<RehomeMove> mv;
  if (!plan_rehome(x->nshard, x->rows_cap, expm, room, n, mv)) {
    report_flags(FLAG_FRONTIER_FULL);
    x->finished = true;
    return flags_to_status(FLAG_FRONTIER_FULL);
  }
  if (mv.empty()) return RTLA_OK;
  // (1) transfers between shards
  Exchange ex(x);
  for (auto& t : mv) {
    if (t.dst == t.a) continue;
    Shard* sa = x->local(t.a);
    Shard* sb = x->local(t.b);
    if (int r = ex.move(t.a, sa ? export_region(x, *sa, t.b) : nullptr, t.b, sb ? staging_region(x, *sb, t.a) : nullptr,
                        4 * t.cnt * ((uint64_t)x->L.W + 2)))
      return r;
  }
  if (int r = ex.flush()) return r;
  // (2) unpack: received rows (from recv_rows, by source), then rows kept by
  // their sender (from its own send_rows, by export region)
  for (int pass = 0; pass < 2; pass++) {
    for (size_t k = 0; k < x->sh.size(); k++) {
      Shard& s = x->sh[k];
      std::fill(s.h_reb, s.h_reb + 2 * SHARD_MAX, 0ull);
      uint64_t mx = 0;
      for (auto& t : mv) {
        if (t.dst != s.id || (pass == 0) != (t.a != t.dst)) continue;
        const int p = pass == 0 ? t.a : t.b;
        s.h_reb[p] = t.cnt;
        s.h_reb[SHARD_MAX + p] = t.base;
        mx = std::max(mx, t.cnt);
      }
      if (!mx) continue;
      if (int r = unpack_staged(x, lv, k, pass == 0 ? s.recv_rows : s.send_rows, mx)) return r;
      HIPCHK(hipStreamSynchronize(x->stream));  // (h_reb is rewritten next)
    }
  }
  for (auto& t : mv)
    if (t.dst != t.a && x->local(t.a)) x->rehomed += t.cnt;
  return RTLA_OK;
}

// Level end: even out the shards' next levels.  n[k] = next-level states of
// shard k (global ids, the same on every rank); the plan every rank computes
// alike (plan_rebalance) sends the LAST rows of the shards above the even
// split, in shard order, to those below it (rows and parent records, staged
// k_stage_rows -> exchange -> k_unpack_rows, in sub-rounds of rows_cap).  A
// new state is stored by the shard that generated it, so an even level stays
// about even, and after the first levels (Init's successors all come from
// Init's shard) little moves.
static int rebalance(rtla_ctx* x, const Level& lv, std::vector<uint64_t>& n) {
  std::vector<uint64_t> m;
  const std::vector<RebalanceMove> mv = plan_rebalance(x->nshard, n, m);
  if (mv.empty()) return RTLA_OK;
  // a receiver's room (its arena / parent records, as the level kernel's
  // next_cap) is known only where it lives: if any lacks it, nobody moves
  uint64_t short_of_room = 0;
  for (size_t k = 0; k < x->sh.size(); k++)
    if (m[x->sh[k].id] > lv.next_cap[k]) short_of_room = 1;
  if (x->world > 1)
    if (int rc = allreduce_u64(x, &short_of_room, 1, 1)) return rc;
  if (short_of_room) return RTLA_OK;
  const uint64_t rc = x->rows_cap;
  uint64_t most = 0;
  for (auto& t : mv) most = std::max(most, t.cnt);
  for (uint64_t lo = 0; lo < most; lo += rc) {
    for (auto& s : x->sh) std::fill(s.h_reb, s.h_reb + 2 * SHARD_MAX, 0ull);
    Exchange ex(x);
    uint64_t mx = 0;
    for (auto& t : mv) {
      if (t.cnt <= lo) continue;
      const uint64_t c = std::min(rc, t.cnt - lo);
      mx = std::max(mx, c);
      Shard* sa = x->local(t.a);
      Shard* sb = x->local(t.b);
      if (sa)
        HIPCHK(launch_stage_rows(x->L.W, next_ring(x, *sa), sa->parents, lv.next_base[sa - x->sh.data()], t.first + lo,
                                 c, export_region(x, *sa, t.b), x->stream));
      if (sb) {
        sb->h_reb[t.a] = c;
        sb->h_reb[SHARD_MAX + t.a] = t.base + lo;
      }
      if (int r = ex.move(t.a, sa ? export_region(x, *sa, t.b) : nullptr, t.b,
                          sb ? staging_region(x, *sb, t.a) : nullptr, 4 * c * ((uint64_t)x->L.W + 2)))
        return r;
    }
    if (int r = ex.flush()) return r;
    for (size_t k = 0; k < x->sh.size(); k++) {
      Shard& s = x->sh[k];
      if (std::all_of(s.h_reb, s.h_reb + x->nshard, [](uint64_t v) { return v == 0; })) continue;
      if (int r = unpack_staged(x, lv, k, s.recv_rows, mx)) return r;
    }
    HIPCHK(hipStreamSynchronize(x->stream));  // (h_reb is rewritten by the next sub-round)
  }
  for (auto& t : mv)
    if (x->local(t.a)) x->rebalanced += t.cnt;
  n = m;
  return RTLA_OK;
}

// RTLA_STAMPS builds with RTLA_STAMPS_PRINT set: where the level kernel's
// wave-cycles went (diagnostic).
void print_stamps(const DevCounters& c, int level) {
  if (!getenv("RTLA_STAMPS_PRINT")) return;
  if (c.cas) fprintf(stderr, "cas level %d: %llu pipelined CAS, %llu probes, %llu new\n", level,
                     (unsigned long long)c.cas, (unsigned long long)c.probes, (unsigned long long)c.next_count);
  static const char* ph[9] = {"setup", "ring", "compute", "resolve", "issue", "rows", "drain", "keys+end", "tile"};
  // (the group start is "tile", the row tile load, then "setup", the per-state setup; non-symmetric kernels:
  // "drain" = the group-end row build, "keys+end" = the group-end probe drain)
  unsigned long long tot = 0;
  for (int k = 0; k < RTLA_NSTAMP; k++) tot += c.stamp[k];
  if (!tot) return;
  fprintf(stderr, "stamps level %d:", level);
  for (int k = 0; k < RTLA_NSTAMP; k++) fprintf(stderr, " %s %.3f", ph[k], (double)c.stamp[k] / tot);
  fprintf(stderr, " (%.3g wave-cycles)\n", (double)tot);
}

// ---- rtla_step, in parts

// Level set-up: counters cleared, where each shard's next level goes, the caps on the device.
static int level_setup(rtla_ctx* x, Level& lv) {
  lv.next_base.resize(x->sh.size());
  lv.next_cap.resize(x->sh.size());
  for (size_t k = 0; k < x->sh.size(); k++) {
    Shard& s = x->sh[k];
    HIPCHK(hipMemsetAsync(s.ctr, 0, offsetof(DevCounters, cover), x->stream));
    lv.next_base[k] = s.cur_base + s.n_cur;
    const bool no_room = lv.next_base[k] >= s.parents_cap;
    if (no_room) {  // nothing fits: every new state is flagged, none stored
      lv.lflags |= FLAG_FRONTIER_FULL;
      lv.next_base[k] = s.parents_cap;
    }
    lv.next_cap[k] = no_room ? 0 : std::min<uint64_t>(next_room(x, s), s.parents_cap - lv.next_base[k]);
    s.h_caps[0] = s.n_cur; s.h_caps[1] = lv.next_cap[k]; s.h_caps[2] = s.parents_cap;
    HIPCHK(hipMemcpyAsync(&s.ctr->cap_cur, s.h_caps, sizeof s.h_caps, hipMemcpyHostToDevice, x->stream));
  }
  for (auto& s : x->sh) HIPCHK(hipEventRecord(s.ev0, x->stream));
  return RTLA_OK;
}

// One shard: the whole level in one fused launch.
static int launch_single(rtla_ctx* x, const Level& lv) {
  Shard& s = x->sh[0];
  HIPCHK(hipEventRecord(s.evm, x->stream));  // (re-recorded after the level kernel)
  HIPCHK(launch_expand({.L = x->L,
                        .cur = cur_ring(x, s),
                        .s_end = s.n_cur,
                        .cur_base = s.cur_base,
                        .out = frontier_out(x, lv, 0),
                        .table = s.table,
                        .tlog2 = x->tlog2,
                        .ctr = s.ctr,
                        .st = x->stream,
                        .xflags = env_xflags(),
                        .grid = (int)std::min<uint64_t>((s.n_cur + 3) / 4, (uint64_t)x->grid)},
                       s.evm));
  return RTLA_OK;
}

// Exchange rounds.  Each round every shard requeues its overflow list,
// expands the rest of its frontier until an owner region of its outbox
// fills (or, without the group guard, x->chunk states), and the records
// travel (gather_counts .. k_build_winners).  Every rank learns from the
// round's count gather what every shard has left, so all issue the same
// collectives, and the rounds end together once nothing is left.
//
// A local HIP failure (a launch, a memset) must not return from inside the
// rounds: the peers would wait in the next collective.  It stops this
// rank's local work instead (`local` runs nothing more once one call
// failed); its shards report FAIL_LEFT as their frontier left in the
// round's count gather, so every rank ends the rounds at the same point,
// and FLAG_LOCAL_FAILURE travels in the level reduction.
static int exchange_rounds(rtla_ctx* x, Level& lv) {
  const Layout& L = x->L;
  const int G = x->nshard, RW = G + 2;
  constexpr uint64_t FAIL_LEFT = ~0ull;
  bool lfail = false;
  auto local = [&lfail](auto&& call) {
    if (!lfail && call() != hipSuccess) {
      (void)hipGetLastError();
      lfail = true;
    }
  };
  for (auto& s : x->sh) {
    s.pos = 0;
    s.over_n = 0;
  }
  uint64_t last_left = ~0ull;
  for (uint64_t round = 0;; round++) {
    for (size_t k = 0; k < x->sh.size() && !lfail; k++) {
      Shard& s = x->sh[k];
      const int nv = s.ov ^ 1;  // the overflow list this round appends to
      local([&] { return hipMemsetAsync(s.out_count, 0, 8 * G, x->stream); });
      local([&] { return hipMemsetAsync(s.over_cnt + nv, 0, 8, x->stream); });
      ShardBox box{G, s.id, (unsigned long long)x->box_cap, x->slog2, (unsigned long long*)s.out_count,
                   (unsigned long long*)s.send_fp, (unsigned long long*)s.send_ref,
                   (unsigned long long)x->stop_at, (unsigned long long*)s.over_fp[nv],
                   (unsigned long long*)s.over_ref[nv], (unsigned long long*)(s.over_cnt + nv),
                   (unsigned long long)x->over_cap};
      local([&] {
        return launch_requeue(s.over_fp[s.ov], s.over_ref[s.ov], s.over_cnt + s.ov, s.over_n, box, s.ctr, x->stream);
      });
      const uint64_t b = s.pos, e = x->chunk ? std::min<uint64_t>(s.n_cur, b + x->chunk) : s.n_cur;
      if (e > b) {
        // RTLA_FAULT=launch:<rank> (tests): an actual launch fails
        if (round == 0 && fault_here(x, "launch")) local([&] { return launch_refused(x->stream); });
        local([&] {
          return launch_expand({.L = L,
                                .cur = cur_ring(x, s),
                                .s_begin = b,
                                .s_end = e,
                                .cur_base = s.cur_base,
                                .out = frontier_out(x, lv, k),
                                .table = s.table,
                                .tlog2 = x->tlog2,
                                .ctr = s.ctr,
                                .box = box,
                                .st = x->stream,
                                .xflags = env_xflags(),
                                .sent = s.sent,
                                .grid = (int)std::min<uint64_t>((e - b + 3) / 4, (uint64_t)x->grid)});
        });
      }
      local([&] {
        return launch_round_tail(s.ctr, s.out_count, G, e - b, s.n_cur - e, x->guarded && e > b, s.over_cnt + nv,
                                 x->stream);
      });
      s.ov = nv;
    }
    if (round == 0 && fault_here(x, "exchange")) lv.lflags |= FLAG_LOCAL_FAILURE;
    if (lfail)  // (best effort: a device that takes no copy fails the gather itself)
      for (auto& s : x->sh) (void)hipMemcpy(s.out_count + G, &FAIL_LEFT, 8, hipMemcpyHostToDevice);
    if (int rc = gather_counts(x)) return rc;
    uint64_t left = 0, sent_recs = 0;  // frontier states and overflow records left anywhere, records this round
    bool failed = false;
    for (int r = 0; r < G; r++) {
      if (x->h_rows[(size_t)r * RW + G] == FAIL_LEFT) failed = true;
      left += x->h_rows[(size_t)r * RW + G] + x->h_rows[(size_t)r * RW + G + 1];
      for (int p = 0; p < G; p++) sent_recs += x->h_rows[(size_t)r * RW + p];
    }
    if (failed) {  // some rank's local work failed: all end the rounds here
      lv.lflags |= FLAG_LOCAL_FAILURE;
      break;
    }
    for (auto& s : x->sh) {
      s.pos = s.n_cur - x->h_rows[(size_t)s.id * RW + G];
      s.over_n = x->h_rows[(size_t)s.id * RW + G + 1];
      x->overflowed += s.over_n;
      for (int p = 0; p < G; p++) x->records += s.h_out[p];
    }
    x->rounds++;
    if (left && !sent_recs && left >= last_left) {  // (cannot happen: a round with room takes a group)
      fprintf(stderr, "rtla: exchange round %llu made no progress\n", (unsigned long long)round);
      report_flags(FLAG_OUTBOX_FULL);
      x->finished = true;
      return RTLA_E_OVERFLOW;
    }
    last_left = left;
    if (int rc = move_records(x, false)) return rc;
    for (auto& s : x->sh) {
      const uint64_t mx_in = *std::max_element(s.h_in.begin(), s.h_in.end());
      local([&] {
        return launch_insert_remote(s.recv_fp, s.in_count, G, x->box_cap, s.table, x->tlog2, s.recv_ans, s.ctr, mx_in,
                                    x->stream);
      });
    }
    if (int rc = move_records(x, true)) return rc;
    for (size_t k = 0; k < x->sh.size() && !lfail; k++) {  // each sender builds its winners into its own next level
      Shard& s = x->sh[k];
      const uint64_t mx_out = *std::max_element(s.h_out.begin(), s.h_out.begin() + G);
      local([&] {
        return launch_build_winners({.L = L,
                                     .cur = cur_ring(x, s),
                                     .cur_base = s.cur_base,
                                     .me = s.id,
                                     .send_ref = s.send_ref,
                                     .ans = s.send_ans,
                                     .counts = s.out_count,
                                     .nshard = G,
                                     .cap = x->box_cap,
                                     .out = frontier_out(x, lv, k),
                                     .ctr = s.ctr,
                                     .max_count = mx_out,
                                     .exp_rows = s.send_rows,
                                     .exp_cap = x->rehome ? x->rows_cap : 0,
                                     .st = x->stream});
      });
    }
    if (!left) break;
  }
  if (lfail) lv.lflags |= FLAG_LOCAL_FAILURE;
  return RTLA_OK;
}

// The level reduction's wire layout, from (G, rehome).  Sums: new, generated,
// probes, frontier; (G > 1) next-level states per shard (global id); one count
// per flag bit (bits are summed, not max-reduced: every rank then reports the
// union of the flags); with re-homing, every shard's export counts per owner
// [G][G] and its next-level room [G].  Maxima: below.  Ranks and the shm
// slot size depend on the order and on total().
struct RedLayout {
  static constexpr int NFLAG = 8;
  enum { new_states = 0, generated = 1, probes = 2, frontier = 3 };                // sums
  enum { flags = 0, violation = 1, device_us = 2, largest_next = 3, NMAX = 4 };    // maxima
  int G, nnext;
  bool rehome;
  constexpr RedLayout(int G_, bool rehome_) : G(G_), nnext(G_ > 1 ? G_ : 0), rehome(rehome_) {}
  constexpr int next(int id) const { return 4 + id; }
  constexpr int flag(int bit) const { return 4 + nnext + bit; }
  constexpr int exported(int a, int b) const { return flag(NFLAG) + a * G + b; }
  constexpr int room(int id) const { return flag(NFLAG) + G * G + id; }
  constexpr int total() const { return flag(NFLAG) + (rehome ? G * G + G : 0); }
};
constexpr int RED_SUMS = RedLayout(SHARD_MAX, true).total();
static_assert(RED_SUMS <= RED_MAX_AT, "the level reduction fits the all-reduce scratch");

// Read the shards' counters back and reduce the level over all ranks.
static int reduce_level(rtla_ctx* x, Level& lv, const RedLayout& R, uint64_t* sums, uint64_t* maxs) {
  const int G = x->nshard;
  lv.hc.resize(x->sh.size());
  bool got = !(lv.lflags & FLAG_LOCAL_FAILURE);
  for (size_t k = 0; k < x->sh.size() && got; k++)
    got = hipMemcpyAsync(&lv.hc[k], x->sh[k].ctr, sizeof(DevCounters), hipMemcpyDeviceToHost, x->stream) == hipSuccess;
  got = got && hipStreamSynchronize(x->stream) == hipSuccess;
  if (!got) {  // (the counters are not read: only the failure is reported, by every rank)
    (void)hipGetLastError();
    lv.lflags |= FLAG_LOCAL_FAILURE;
    for (auto& c : lv.hc) memset(&c, 0, sizeof c);
  }
  for (size_t k = 0; k < x->sh.size(); k++) {
    Shard& s = x->sh[k];
    const DevCounters& c = lv.hc[k];
    float kms = 0.f, ems = 0.f;
    (void)hipEventElapsedTime(&kms, s.ev0, s.ev1);
    if (G == 1) (void)hipEventElapsedTime(&ems, s.ev0, s.evm);
    else ems = kms;  // multi-shard: rows are built inside the exchange rounds
    lv.emax = std::max(lv.emax, (double)ems);
    uint64_t exported = 0;  // new states built for other owners (in the export regions: re-homed afterwards)
    for (int p = 0; p < G && x->rehome; p++) {
      sums[R.exported(s.id, p)] = exported_rows(c, p, x->rows_cap);
      exported += sums[R.exported(s.id, p)];
    }
    if (x->rehome) sums[R.room(s.id)] = lv.next_cap[k];
    sums[R.new_states] += c.next_count + exported;
    sums[R.generated] += c.generated;
    sums[R.probes] += c.probes;
    sums[R.frontier] += s.n_cur;
    if (G > 1) sums[R.next(s.id)] = c.next_count;
    lv.lflags |= c.flags;
    maxs[R.violation] = std::max<uint64_t>(maxs[R.violation], c.viol_mask ? 1 : 0);
    maxs[R.device_us] = std::max<uint64_t>(maxs[R.device_us], (uint64_t)(kms * 1000.0));
    maxs[R.largest_next] = std::max<uint64_t>(maxs[R.largest_next], c.next_count);
    if (c.viol_mask && !s.viol_mask) {
      s.viol_mask = c.viol_mask; s.viol_in_model = c.viol_in_model; s.viol_inst = c.viol_inst;
      s.viol_parent = c.viol_parent; s.viol_child = c.viol_child;
    }
  }
  print_stamps(lv.hc[0], x->level + 1);
  for (int b = 0; b < R.NFLAG; b++) sums[R.flag(b)] = (uint64_t)(lv.lflags >> b & 1);
  if (int rc = allreduce2_u64(x, sums, R.total(), maxs, R.NMAX)) return rc;
  for (int b = 0; b < R.NFLAG; b++)
    if (sums[R.flag(b)]) maxs[R.flags] |= 1ull << b;
  return RTLA_OK;
}

// Commit the reduced level: totals and status, the level-end row moves, the
// shards' next levels become current, *st.
static int commit_level(rtla_ctx* x, const Level& lv, const RedLayout& R, const uint64_t* sums, const uint64_t* maxs,
                        rtla_level_stats* st, double t0) {
  const int G = x->nshard;
  const int flags = (int)maxs[R.flags];
  x->max_front = maxs[R.largest_next];
  if (flags) {
    report_flags(flags);
    x->finished = true;
    if (st) {  // the level is incomplete: only which capacity ran out is reported
      memset(st, 0, sizeof *st);
      st->level = x->level + 1; st->status = flags_to_status(flags); st->flags = flags;
      st->frontier = sums[R.frontier]; st->distinct_total = x->distinct; st->generated_total = x->generated;
      st->row_bytes = (uint64_t)x->L.W * 4; st->seconds = now_s() - t0;
    }
    return flags_to_status(flags);
  }
  const uint64_t nnew = sums[R.new_states];
  x->generated += sums[R.generated];
  x->distinct += nnew;
  x->level++;
  int status = RTLA_OK;
  if (maxs[R.violation]) {
    x->finished = true;
    status = RTLA_VIOLATION;
  } else if (nnew == 0) {
    x->finished = true;
    status = RTLA_DONE;
  }
  std::vector<uint64_t> nnext;
  if (G > 1) nnext.assign(sums + R.next(0), sums + R.next(G));
  if (G > 1 && status == RTLA_OK && x->rehome) {  // winners to their owners
    if (int r = rehome(x, lv, nnext, sums + R.exported(0, 0), sums + R.room(0))) return r;
  }
  if (G > 1 && status == RTLA_OK) {  // even out the shards' next levels
    if (int r = rebalance(x, lv, nnext)) return r;
    x->max_front = *std::max_element(nnext.begin(), nnext.end());
  }
  for (size_t k = 0; k < x->sh.size(); k++) {
    Shard& s = x->sh[k];
    s.cur_base = lv.next_base[k];
    s.cur_start = next_ring(x, s).start;
    s.n_cur = G > 1 ? nnext[s.id] : lv.hc[k].next_count;
  }
  if (st) {
    memset(st, 0, sizeof *st);
    st->level = x->level; st->status = status; st->frontier = sums[R.frontier]; st->new_states = nnew;
    st->generated = sums[R.generated]; st->distinct_total = x->distinct; st->generated_total = x->generated;
    st->kernel_ms = maxs[R.device_us] / 1000.0; st->probes = sums[R.probes]; st->row_bytes = (uint64_t)x->L.W * 4;
    st->expand_ms = x->world > 1 ? st->kernel_ms : lv.emax;
    st->seconds = now_s() - t0;
  }
  return status;
}

extern "C" int rtla_step(rtla_ctx* x, rtla_level_stats* st) {
  if (!x) return RTLA_E_ARG;
  if (!x->inited || x->finished) return RTLA_E_STATE;
  x->sim.viol = false;  // (a simulated violation is the last rtla_simulate's: the BFS goes on as if it had not run)
  x->audit.viol = false;  // (and an audit's the last rtla_check_frontier's)
  const double t0 = now_s();
  HIPCHK(hipSetDevice(x->device));
  Level lv;
  if (int rc = level_setup(x, lv)) return rc;
  if (int rc = x->nshard == 1 ? launch_single(x, lv) : exchange_rounds(x, lv)) return rc;
  for (auto& s : x->sh) (void)hipEventRecord(s.ev1, x->stream);  // (a failure here shows in the read-back below)
  const RedLayout R(x->nshard, x->rehome);
  uint64_t sums[RED_SUMS] = {}, maxs[RedLayout::NMAX] = {};
  if (int rc = reduce_level(x, lv, R, sums, maxs)) return rc;
  return commit_level(x, lv, R, sums, maxs, st, t0);
}

extern "C" int rtla_violation(rtla_ctx* x, int32_t* inv_mask, int32_t* in_model) {
  if (!x) return RTLA_E_ARG;
  if (x->sim.viol || x->audit.viol) {
    if (inv_mask) *inv_mask = x->sim.viol ? x->sim.mask : x->audit.mask;
    if (in_model) *in_model = x->sim.viol ? x->sim.in_model : x->audit.in_model;
    return RTLA_VIOLATION;
  }
  Shard* s = x->viol_shard();
  if (inv_mask) *inv_mask = s ? s->viol_mask : 0;
  if (in_model) *in_model = s ? s->viol_in_model : 0;
  return s ? RTLA_VIOLATION : RTLA_OK;
}

extern "C" int rtla_frontier(rtla_ctx* x, uint32_t* rows, size_t cap, size_t* n) {
  if (!x || !n) return RTLA_E_ARG;
  if (!x->inited) return RTLA_E_STATE;
  size_t tot = 0;
  for (auto& s : x->sh) tot += s.n_cur;
  *n = tot;
  if (!rows) return RTLA_OK;
  if (tot > cap) return RTLA_E_ARG;
  HIPCHK(hipSetDevice(x->device));
  size_t off = 0;
  for (auto& s : x->sh) {
    if (s.n_cur)
      HIPCHK(ring_copy(cur_ring(x, s), x->L.W, 0, s.n_cur, rows + off * x->L.W, true));
    off += s.n_cur;
  }
  return RTLA_OK;
}

extern "C" int rtla_frontier_rows(rtla_ctx* x, const uint64_t* index, size_t n, uint32_t* rows) {
  if (!x || (n && (!index || !rows))) return RTLA_E_ARG;
  if (!x->inited) return RTLA_E_STATE;
  uint64_t tot = 0;
  for (auto& s : x->sh) tot += s.n_cur;
  for (size_t i = 0; i < n; i++)
    if (index[i] >= tot) return RTLA_E_ARG;
  HIPCHK(hipSetDevice(x->device));
  for (size_t i = 0; i < n; i++) {  // (local shards in the order rtla_frontier lists them)
    uint64_t g = index[i];
    for (auto& s : x->sh) {
      if (g < s.n_cur) {
        HIPCHK(ring_copy(cur_ring(x, s), x->L.W, g, 1, rows + i * (uint64_t)x->L.W, true));
        break;
      }
      g -= s.n_cur;
    }
  }
  return RTLA_OK;
}

// Digest of the current frontier: rows stream to the host in chunks (the
// next chunk's copy overlaps the current chunk's hashing).
static int level_digest(rtla_ctx* x, int threads, uint64_t* out, bool orbit) {
  if (!x || !out) return RTLA_E_ARG;
  if (!x->inited) return RTLA_E_STATE;
  // A local failure (device, pinned buffers, a copy) skips the hashing but
  // still reaches the reduction below, so no other rank waits in it.
  int rc = hipSetDevice(x->device) == hipSuccess ? RTLA_OK : RTLA_E_HIP;
  const int W = x->L.W;
  const int nt = text_threads(threads);
  const uint64_t CH = std::max<uint64_t>(1, (256ull << 20) / (4ull * W));  // ~256 MB of rows per chunk
  uint32_t* hbuf[2] = {nullptr, nullptr};
  for (auto& b : hbuf)
    if (!rc && hipHostMalloc((void**)&b, CH * W * 4, hipHostMallocDefault) != hipSuccess) {
      b = nullptr;
      rc = RTLA_E_HIP;
    }
  uint64_t sum = 0;
  for (auto& s : x->sh) {
    if (rc) break;
    const Ring r = cur_ring(x, s);
    // chunk j covers states [j * CH, ...); copies go in pieces that do not wrap the ring
    auto issue = [&](uint64_t g0, uint32_t* dst) -> hipError_t {
      uint64_t n = std::min<uint64_t>(CH, s.n_cur - g0), g = g0;
      while (n) {
        const uint64_t p = ring_idx(r, g), m = std::min<uint64_t>(n, r.cap - p);
        hipError_t e = hipMemcpyAsync(dst, r.base + p * (uint64_t)W, m * W * 4, hipMemcpyDeviceToHost, x->stream);
        if (e != hipSuccess) return e;
        dst += m * (uint64_t)W;
        g += m;
        n -= m;
      }
      return hipSuccess;
    };
    if (!s.n_cur) continue;
    if (issue(0, hbuf[0]) != hipSuccess) { rc = RTLA_E_HIP; break; }
    for (uint64_t g = 0, j = 0; g < s.n_cur; g += CH, j++) {
      if (hipStreamSynchronize(x->stream) != hipSuccess) { rc = RTLA_E_HIP; break; }
      if (g + CH < s.n_cur && issue(g + CH, hbuf[(j + 1) & 1]) != hipSuccess) { rc = RTLA_E_HIP; break; }
      sum += rows_digest(x->L, hbuf[j & 1], std::min<uint64_t>(CH, s.n_cur - g), nt, orbit);
    }
    if (rc) break;
  }
  (void)hipStreamSynchronize(x->stream);
  for (auto& b : hbuf)
    if (b) (void)hipHostFree(b);
  // every rank joins the reduction, also after a local failure (the flag travels with it)
  uint64_t v[2] = {sum, rc ? 1ull : 0ull};
  if (int e = allreduce_u64(x, v, 2, 0)) return e;
  if (rc) return rc;
  if (v[1]) return RTLA_E_HIP;
  *out = v[0];
  return RTLA_OK;
}

extern "C" int rtla_level_text_hash(rtla_ctx* x, int threads, uint64_t* out) {
  return level_digest(x, threads, out, false);
}
extern "C" int rtla_level_orbit_hash(rtla_ctx* x, int threads, uint64_t* out) {
  return level_digest(x, threads, out, true);
}

// Collective when world > 1: a local failure (device, read-back) travels in
// the reduction (its last word), so every rank fails together.
extern "C" int rtla_coverage(rtla_ctx* x, uint64_t* gen, uint64_t* distinct, int n) {
  if (!x) return RTLA_E_ARG;
  std::vector<uint64_t> acc(2 * COVER_CODES + 1, 0);
  bool bad = hipSetDevice(x->device) != hipSuccess || fault_here(x, "coverage");
  for (auto& s : x->sh) {
    DevCounters h;
    if (bad || hipMemcpy(&h, s.ctr, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) {
      bad = true;
      break;
    }
    for (int k = 0; k < 2 * COVER_CODES; k++) acc[k] += h.cover[k];
  }
  acc[2 * COVER_CODES] = bad ? 1 : 0;
  int rc = allreduce_u64(x, acc.data(), 2 * COVER_CODES + 1, 0);
  if (rc) return rc;
  if (acc[2 * COVER_CODES]) return bad ? RTLA_E_HIP : RTLA_E_COMM;
  for (int k = 0; k < n && k < COVER_CODES; k++) {
    if (gen) gen[k] = acc[k];
    if (distinct) distinct[k] = acc[COVER_CODES + k];
  }
  return COVER_CODES;
}

// Where a counterexample starts: {has, holder shard, shard-local index,
// pending instance + 1} -- the violating state, or its parent + action when
// the violation was seen before the state had a home; the same on every rank.
static int trace_start(rtla_ctx* x, bool bad, uint64_t start[4]) {
  Shard* vs = x->viol_shard();
  if (x->sim.viol) {  // (single shard, world 1: rtla_simulate's precondition)
    start[0] = 1; start[1] = 0; start[2] = x->sim.start; start[3] = 0;
  } else if (x->audit.viol) {  // (the same precondition: the audited row, or its violating successor)
    start[0] = 1; start[1] = 0; start[2] = x->audit.start; start[3] = (uint64_t)(x->audit.inst + 1);
  } else if (vs) {
    start[0] = 1;
    start[1] = (uint64_t)vs->id;
    if (vs->viol_inst < 0) { start[2] = vs->viol_child; start[3] = 0; }  // a violating root (Init: index 0)
    else if (vs->viol_in_model && vs->viol_child != ~0ull) { start[2] = vs->viol_child; start[3] = 0; }
    else { start[2] = vs->viol_parent; start[3] = (uint64_t)vs->viol_inst + 1; }
  }
  if (x->world == 1) return start[0] ? RTLA_OK : RTLA_E_STATE;
  // the lowest shard holding a violation publishes its start record
  uint64_t v[2] = {(uint64_t)x->nshard - (start[0] ? start[1] : (uint64_t)x->nshard), bad ? 1ull : 0ull};
  int rc = allreduce_u64(x, v, 2, 1);  // max of (G - holder) == min holder; any failure
  if (rc) return rc;
  if (v[1]) return bad ? RTLA_E_HIP : RTLA_E_COMM;
  if (v[0] == 0) return RTLA_E_STATE;
  const int root = (int)((uint64_t)x->nshard - v[0]);
  uint64_t w[5] = {0, 0, 0, 0, 0};  // root's start record, then the failure count
  if (x->rank == root) memcpy(w, start, 32);
  rc = allreduce_u64(x, w, 5, 0);
  if (rc) return rc;
  memcpy(start, w, 32);
  return RTLA_OK;
}

// Counterexample: find where it starts (trace_start), walk the parent records
// back to a root (Init, or the row of a seeded search the record names: root_record, rtla_ctx.h) -- across
// shards: a record names its parent's shard (parent_record, rtla_device.h) -- then replay the action
// instances forward from that root's row with the kernel that built them.  Collective when world > 1
// (every rank calls it; each step's record comes from the rank that holds it).
extern "C" int rtla_trace(rtla_ctx* x, uint32_t* rows, int32_t* labels, size_t cap, size_t* n_rows) {
  if (!x || !n_rows) return RTLA_E_ARG;
  // world > 1: every rank reaches every reduction below; a local failure
  // travels in them (a failure count), so all ranks stop at the same step
  bool bad = hipSetDevice(x->device) != hipSuccess || fault_here(x, "trace");
  if (bad && x->world == 1) return RTLA_E_HIP;
  const Layout& L = x->L;
  const bool simv = x->sim.viol;
  uint64_t start[4] = {0, 0, 0, 0};
  if (int rc = trace_start(x, bad, start)) return rc;
  std::vector<int32_t> insts;
  if (start[3]) insts.push_back((int32_t)(start[3] - 1));
  uint64_t shard = start[1], g = start[2], root = ~0ull;
  for (int guard = 0; guard < (1 << 20); guard++) {
    uint64_t p = 0;
    if (int rc = comm_parent_record(x, shard, g, bad, &p)) return rc;
    if (is_root_record(p)) {  // Init, or root k of a seeded search
      root = root_of(p);
      break;
    }
    insts.push_back(parent_inst(p));
    shard = parent_shard(p);
    g = parent_index(p);
  }
  if (root >= x->roots.size() / (size_t)L.W) return RTLA_E_STATE;  // (the walk met no root record of this search)
  std::reverse(insts.begin(), insts.end());
  // a simulated violation: the walk's states after the BFS chain, the violating successor last
  size_t n = insts.size() + 1 + (simv ? (size_t)x->sim.step : 0);
  *n_rows = n;
  if (!rows && !labels) return RTLA_OK;
  if (n > cap) return RTLA_E_ARG;
  std::vector<uint32_t> row(x->roots.begin() + root * L.W, x->roots.begin() + (root + 1) * L.W);
  uint32_t* d_row = nullptr;
  HIPCHK(hipMalloc(&d_row, 64 * L.W * 4));  // a whole 64-row group (the level kernel's tile)
  if (rows) memcpy(rows, row.data(), L.W * 4);
  if (labels) labels[0] = -1;
  int rc = RTLA_OK;
  for (size_t k = 0; k < insts.size() && rc == RTLA_OK; k++) {
    if (hipMemcpy(d_row, row.data(), L.W * 4, hipMemcpyHostToDevice) != hipSuccess) { rc = RTLA_E_HIP; break; }
    std::vector<uint32_t> out;
    std::vector<uint64_t> info;
    int r = expand_batch_dev(L, d_row, 1, out, info, x->stream);
    if (r < 0) { rc = r; break; }
    size_t hit = info.size();
    for (size_t q = 0; q < info.size(); q++)
      if (successor_inst(info[q]) == insts[k]) hit = q;
    if (hit == info.size()) { rc = RTLA_E_STATE; break; }
    memcpy(row.data(), &out[hit * L.W], L.W * 4);
    if (rows) memcpy(rows + (k + 1) * L.W, row.data(), L.W * 4);
    if (labels) labels[k + 1] = successor_label(info[hit]);
  }
  (void)hipFree(d_row);
  if (rc == RTLA_OK && simv) {  // replayed on the host from (seed, walk): no path is stored on the device
    const size_t at = insts.size() + 1;
    size_t got = 0;
    rc = sim_walk_rows(L, row.data(), x->sim.seed, x->sim.walk, x->sim.step, rows ? rows + at * L.W : nullptr,
                       labels ? labels + at : nullptr, n - at, &got,
                       x->sim.scode.empty() ? nullptr : x->sim.scode.data(),
                       x->sim.acode.empty() ? nullptr : x->sim.acode.data());
    if (rc == RTLA_VIOLATION && got == (size_t)x->sim.step) rc = RTLA_OK;
    else if (rc >= 0) rc = RTLA_E_STATE;
  }
  return rc;
}
