// rtla_ctx.h -- private to the host driver's units: the context and what they share.
//   rtla_host.cpp     open / close / reset / init / step, the exchange protocol, frontier access, digests, trace
//   rtla_comm.cpp     collectives and transfers between shards (RCCL, shared memory, device copies)
//   rtla_ckpt.cpp     checkpoint / recover
//   rtla_simhost.cpp  random-walk simulation
//   rtla_audit.cpp    passes over rows outside the search (batch, host replay, frontier), and the invariant audit
//   rtla_predhost.cpp user-defined predicates: the rtla_pred_* ABI over the compiler (rtla_pred.cpp) and those passes
//   rtla_constrain.cpp user-defined CONSTRAINTs: the level just produced pruned by a state set (rtla_kconstrain.hip)
//   rtla_rows.cpp     the context-free row API, synthetic and probe micro-benchmarks
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <functional>
#include <set>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/rtla.h"
#include "rtla_device.h"
#include "rtla_audit.h"
#include "rtla_launch.h"
#include "rtla_model.h"

using namespace rtla;

#pragma GCC visibility push(hidden)  // nothing below is part of librtla.so's surface (include/rtla.h)

struct Shard {
  int id = 0;
  uint64_t* table = nullptr;
  uint64_t* parents = nullptr;
  uint64_t parents_cap = 0;
  uint32_t* arena = nullptr;        // frontier rows: the current and the next level, as a ring (Ring)
  uint64_t cur_start = 0;           // arena row of the current level's first state (a multiple of 64)
  uint64_t n_cur = 0, cur_base = 0;
  DevCounters* ctr = nullptr;
  int* dflags = nullptr;
  // exchange buffers (nshard > 1)
  uint64_t* out_count = nullptr;   // [G + 2] device: records queued per destination (reserved slots; those past
                                   // box_cap are on the overflow list), frontier states left, overflow records
  uint64_t* in_count = nullptr;    // [G] device: records received per source
  uint64_t* all_count = nullptr;   // [G][G + 2] device (RCCL all-gather target)
  uint64_t* send_fp = nullptr;     // [G][cap][2]
  uint64_t* send_ref = nullptr;    // [G][cap]
  uint32_t* send_ans = nullptr;    // [G][cap]  owners' answers to our records
  uint64_t* recv_fp = nullptr;     // [G][cap][2]
  uint32_t* recv_ans = nullptr;    // [G][cap]  our answers to the senders
  uint64_t* rows_in = nullptr;     // [G] device: rows received per source (re-balancing sub-round)
  uint64_t* rows_base = nullptr;   // [G] device: next-frontier slot of each source's first row
  uint32_t* send_rows = nullptr;   // [G][rows_cap][W + 2]  re-balancing staging
  uint32_t* recv_rows = nullptr;   // [G][rows_cap][W + 2]
  uint64_t* sent = nullptr;        // [2^slog2] sent cache: fingerprints this shard already sent to their owners
  uint64_t* over_fp[2] = {nullptr, nullptr};   // overflow lists [over_cap][2]: records past their region's end,
  uint64_t* over_ref[2] = {nullptr, nullptr};  // sent in the next round (k_requeue)
  uint64_t* over_cnt = nullptr;    // [2] their lengths
  int ov = 0;                      // the list the next round requeues
  uint64_t pos = 0, over_n = 0;    // this level: next frontier state to expand, records on list ov
  std::vector<uint64_t> h_out, h_in;
  uint64_t h_reb[2 * SHARD_MAX] = {};  // re-balancing: rows_in / rows_base of this sub-round (host staging)
  uint64_t h_caps[3] = {0, 0, 0};  // -> DevCounters cap_cur / cap_next / cap_parents
  hipEvent_t ev0 = nullptr, ev1 = nullptr, evm = nullptr;
  // violation found on this shard
  int viol_mask = 0, viol_in_model = 0, viol_inst = -1;
  uint64_t viol_parent = 0, viol_child = ~0ull;
};

// rtla_simulate's device buffers (allocated at first use, sized by the batch)
// and the violation its last call found (rtla_violation / rtla_trace).
struct SimState {
  SimCounters* ctr = nullptr;
  uint64_t* ends = nullptr;    // [ends_cap] u64: the batch's end records (4 words each; 5 with user properties)
  uint32_t* prog = nullptr;    // rtla_simulate_pred: the device copy of both programs (2 * PRED_MAX_WORDS words)
  uint32_t* carry = nullptr;   // [carry_cap][W] current rows of a batch whose depth is split across launches
  uint64_t ends_cap = 0, carry_cap = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool viol = false;
  uint64_t seed = 0, walk = 0, start = 0;  // start: parent-record index of the walk's start row
  int step = 0, inst = -1, mask = 0, in_model = 0;
  std::vector<uint32_t> scode, acode;  // rtla_simulate_pred: the programs the violating walk is replayed with
};

// rtla_check_frontier's device counters and events (allocated at first use)
// and the violation its last call found (rtla_violation / rtla_trace).
struct AuditState {
  AuditCounters* ctr = nullptr;
  uint32_t* prog = nullptr;  // rtla_pred_frontier: the program's device copy (PRED_MAX_WORDS words)
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool viol = false;
  uint64_t start = 0;  // parent-record index of the violating row (succ: of the violating successor's parent)
  int inst = -1, mask = 0, in_model = 0;  // inst >= 0: the violating successor's action instance
};

// rtla_pred_constrain's device buffers and events (allocated at first use, freed at close; rtla_constrain.cpp)
namespace rtla {
struct ConstrainTotals;
}
struct ConstrainBufs {
  uint32_t* stage = nullptr;      // [rows * W + 4] a chunk's kept rows on their way back into the ring
  uint64_t* stage_par = nullptr;  // [rows] and their parent records
  int* masks = nullptr;           // [rows] k_pred_state's per-row masks of one chunk
  uint64_t* keep = nullptr;       // [keep_words] the level's keep bitmap: one u64 per group of 64 rows
  uint32_t* offs = nullptr;       // [rows / 64] a chunk's kept rows before each of its groups
  ConstrainTotals* tot = nullptr;
  AuditCounters* ctr = nullptr;
  uint32_t* prog = nullptr;       // the program's device copy (PRED_MAX_WORDS words)
  uint64_t rows = 0, keep_words = 0;  // rows: the chunk size R the buffers were made for
  int W = 0;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
};

// device scratch of the all-reduces: sums at [0, RED_MAX_AT), maxima after
constexpr int RED_WORDS = 256, RED_MAX_AT = 192;

struct Comm;  // the transport between ranks / shards: rtla_comm.cpp alone looks inside

struct rtla_ctx {
  rtla_cfg cfg;
  Layout L;
  int rank = 0, world = 1, device = 0;
  int nshard = 1;          // shards in the whole job
  int shard0 = 0;          // global id of sh[0]
  std::vector<Shard> sh;   // shards held by this process
  hipStream_t stream = nullptr;
  Comm* comm = nullptr;
  int tlog2 = 0;
  int slog2 = 0;           // sent cache: 2^slog2 slots per shard (multi-shard)
  uint64_t front_cap = 0, box_cap = 0, chunk = 0, rows_cap = 0;
  uint64_t stop_at = 0, over_cap = 0;  // multi-shard outbox: the level kernel's group guard, overflow list capacity
  bool guarded = false;    // multi-shard rounds run the grouped level kernel (rounds sized by the outbox)
  std::vector<uint64_t> h_rows;  // [G][G + 2] the round's gathered counts, every shard's row
  uint64_t rebalanced = 0; // rows moved by level-end re-balancing (all levels, this process's shards)
  bool rehome = false;     // multi-shard, no SYMMETRY: winners are moved to their owner at level end (rehome)
  uint64_t rehomed = 0;    // rows this process's shards moved to their owners (all levels)
  uint64_t rounds = 0;     // exchange rounds run (all levels)
  uint64_t overflowed = 0; // records that went through the overflow list (all levels, this process's shards)
  uint64_t records = 0;    // fingerprint records this process's shards sent to other shards (all levels)
  uint64_t* red = nullptr;  // device scratch for all-reduces
  int level = 0;
  bool inited = false, finished = false;
  uint64_t distinct = 0, generated = 0;
  uint64_t max_front = 0;  // largest frontier of any shard in the job (multi-shard round count)
  int grid = 0;
  std::vector<uint32_t> roots;  // [n][W] the search's roots, each named by its parent record (root_record): Init
                                // alone, or the distinct rows rtla_init_rows was given
  bool seeded = false;          // the roots are rtla_init_rows's (no checkpoint holds them)
  SimState sim;
  AuditState audit;
  ConstrainBufs constrain;

  Shard* local(int id) {  // the shard with this global id, if this process holds it
    for (auto& s : sh)
      if (s.id == id) return &s;
    return nullptr;
  }
  Shard* viol_shard() {  // violation found on a local shard
    for (auto& s : sh)
      if (s.viol_mask) return &s;
    return nullptr;
  }
};

// What a pass over the frontier where it lies (audits, predicates, steps, random walks) needs, else RTLA_E_STATE:
// a search of one shard in one process that keeps rows, initialised, with no violation of its own and rows to read.
inline bool frontier_pass_ok(rtla_ctx* x) {
  return x->cfg.mode != RTLA_MODE_DEDUP && x->world == 1 && x->nshard == 1 && x->inited && !x->viol_shard() &&
         x->sh[0].n_cur != 0;
}

// Parent record of root k of a search: the root mark -- shard byte 0xFF and instance 0xFFFF, which no stored
// successor carries -- around an index field that counts down from 2^40 - 1, so root 0 (Init) keeps ~0ull.
inline uint64_t root_record(uint64_t k) { return ~0ull - (k << 16); }
inline bool is_root_record(uint64_t p) { return parent_shard(p) == 0xFF && parent_inst(p) == 0xFFFF; }
inline uint64_t root_of(uint64_t p) { return (1ull << 40) - 1 - parent_index(p); }

// A failing HIP call is reported and ends the function with `ret`.
#define HIPCHK_RET(x, ret)                                                                          \
  do {                                                                                              \
    hipError_t e_ = (x);                                                                            \
    if (e_ != hipSuccess) {                                                                         \
      fprintf(stderr, "rtla: HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
      return ret;                                                                                   \
    }                                                                                               \
  } while (0)
#define HIPCHK(x) HIPCHK_RET(x, RTLA_E_HIP)
// `Layout L` of the configuration *c, or the function ends with why it has none.
#define CFG_LAYOUT(L, c) \
  Layout L;              \
  if (int r_ = layout_from_cfg(c, &L)) return r_

// f(std::integral_constant<int, N>) for the model's server count (the templates over N)
template <class F>
auto dispatch_n(const Layout& L, F f) {
  switch (L.N) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 3: return f(std::integral_constant<int, 3>());
    case 4: return f(std::integral_constant<int, 4>());
    default: return f(std::integral_constant<int, 5>());
  }
}

// ---- the row arena as a ring (Ring, rtla_device.h)
inline uint64_t round64(uint64_t n) { return (n + 63) & ~63ull; }
inline Ring cur_ring(const rtla_ctx* x, const Shard& s) { return Ring{s.arena, s.cur_start, x->front_cap}; }
// The next level starts at the first 64-row boundary past the current one
// and may use every arena row the current level does not.
inline Ring next_ring(const rtla_ctx* x, const Shard& s) {
  return Ring{s.arena, (s.cur_start + round64(s.n_cur)) % x->front_cap, x->front_cap};
}
inline uint64_t next_room(const rtla_ctx* x, const Shard& s) {
  const uint64_t used = round64(s.n_cur);
  return x->front_cap > used ? x->front_cap - used : 0;
}

inline double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
inline int flags_to_status(int flags) {
  if (flags & FLAG_LOCAL_FAILURE) return RTLA_E_HIP;
  if (flags & FLAG_SPEC_ERROR) return RTLA_E_SPEC;
  if (flags) return RTLA_E_OVERFLOW;
  return RTLA_OK;
}

// rtla_host.cpp
void report_flags(int flags);
int env_xflags();
int layout_from_cfg(const rtla_cfg* c, Layout* L);
bool fault_here(const rtla_ctx* x, const char* where);
void print_stamps(const DevCounters& c, int level);
// rtla_audit.cpp: one pass (`launch`: the kernel, over the ring, row count, device counters and stream it is
// given) over host rows staged into a device buffer / over the context's frontier where it lies.  The masks'
// bits are what the kernel evaluates (RTLA_INV_* bits, a predicate or action set's definitions); the key is
// audit_key.  succ: the pass evaluates successors (a violation has an instance).  evaluated (may be null): the
// evaluated states / steps.
using AuditLaunch = std::function<hipError_t(const Ring&, uint64_t, int*, AuditCounters*, hipStream_t)>;
AuditCounters audit_zero();
int audit_batch(const Layout& L, const uint32_t* rows, size_t n, const AuditLaunch& launch, int32_t* masks,
                uint64_t* counts, uint64_t* evaluated = nullptr);
int audit_frontier(rtla_ctx* x, int succ, const AuditLaunch& launch, rtla_audit_stats* out);
// rtla_constrain.cpp
void constrain_free(ConstrainBufs& b);
// rtla_rows.cpp
int text_threads(int want);

// work(t, begin, end) for every chunk of `chunk` items of [0, n), handed out in ascending order to `threads`
// threads as each comes free (t: the thread, 0 the caller's own); returns when all are done.
template <class F>
void parallel_chunks(size_t n, size_t chunk, int threads, F work) {
  std::atomic<size_t> next{0};
  auto run = [&](int t) {
    for (;;) {
      const size_t b = next.fetch_add(chunk);
      if (b >= n) break;
      work(t, b, std::min(n, b + chunk));
    }
  };
  std::vector<std::thread> pool;
  for (int t = 1; t < threads; t++) pool.emplace_back(run, t);
  run(0);
  for (auto& th : pool) th.join();
}

// The host replay of a pass over n rows: masks[k] = row(k, tally), the tally being that of the thread that took
// the row's 256-row chunk; the threads' flags, counts and evaluated states are merged.
template <class F>
int replay_rows(size_t n, int threads, int32_t* masks, uint64_t* counts, uint64_t* evaluated, F row) {
  const int nt = (int)std::min<size_t>((size_t)std::min(text_threads(threads), 16), std::max<size_t>(1, n / 256));
  std::vector<AuditCounters> part((size_t)nt, audit_zero());
  auto merge = [](AuditCounters& into, const AuditCounters& p) {
    into.flags |= p.flags;
    into.evaluated += p.evaluated;
    for (int k = 0; k < AUDIT_COUNTS; k++) into.counts[k] += p.counts[k];
  };
  parallel_chunks(n, 256, nt, [&](int t, size_t b, size_t e) {
    AuditCounters tl = audit_zero();  // the chunk's own: the threads' tallies lie side by side in memory
    for (size_t k = b; k < e; k++) masks[k] = row(k, tl);
    merge(part[(size_t)t], tl);
  });
  AuditCounters sum = audit_zero();
  for (const AuditCounters& p : part) merge(sum, p);
  if (sum.flags) return flags_to_status(sum.flags);
  if (counts)
    for (int k = 0; k < AUDIT_COUNTS; k++) counts[k] = sum.counts[k];
  if (evaluated) *evaluated = sum.evaluated;
  return RTLA_OK;
}
uint64_t rows_digest(const Layout& L, const uint32_t* rows, size_t n, int threads, bool orbit = false);
int expand_batch_dev(const Layout& L, const uint32_t* d_rows, size_t n, std::vector<uint32_t>& out,
                     std::vector<uint64_t>& info, hipStream_t st);
// rtla_simhost.cpp: one walk's states (and, last, its violating successor) from the host; sprog / aprog: the
// programs of the state set and the action set the walk carries, or null
int sim_walk_rows(const Layout& L, const uint32_t* start, uint64_t seed, uint64_t walk, int depth, uint32_t* rows,
                  int32_t* labels, size_t cap, size_t* n_rows, const uint32_t* sprog, const uint32_t* aprog);

// ---- rtla_comm.cpp: collectives between ranks.  Every function is called
// by every rank in the same order; device buffers, in stream order.
int comm_open(rtla_ctx* x, const void* comm_id);  // the transport RTLA_TRANSPORT names for this deployment
void comm_close(rtla_ctx* x);
const char* comm_name(const rtla_ctx* x);         // rtla_device_info's "transport"
// Sum (op 0) or max (op 1) of n u64 over all ranks; host in/out.
int allreduce_u64(rtla_ctx* x, uint64_t* v, int n, int op);
// Sum of n1 (<= RED_MAX_AT) u64 and max of n2 u64 over all ranks (one synchronisation); host in/out.
int allreduce2_u64(rtla_ctx* x, uint64_t* sum, int n1, uint64_t* mx, int n2);
// Every shard's out_count row ([G + 2]) -> x->h_rows on every rank; synchronises the stream.
int comm_gather_rows(rtla_ctx* x);
// Parent record g of shard `shard` -> *p on every rank; `bad`: this rank's failure flag, which travels along.
int comm_parent_record(rtla_ctx* x, uint64_t shard, uint64_t g, bool& bad, uint64_t* p);

// One all-to-all-v round between shards (global ids): `move` queues or issues
// each transfer, `flush` runs what was queued in one exchange.  Every rank
// calls both with the same plan; a pointer is null where that shard is not local.
struct Msg {
  void* ptr;
  size_t bytes;
  int peer;
};
struct Exchange {
  rtla_ctx* x;
  std::vector<Msg> sends, recvs;
  explicit Exchange(rtla_ctx* x_) : x(x_) {}
  int move(int src_shard, const void* src, int dst_shard, void* dst, size_t bytes);
  int flush();
};

#pragma GCC visibility pop
