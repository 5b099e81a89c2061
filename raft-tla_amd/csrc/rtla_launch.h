// rtla_launch.h -- host-side launch wrappers for the kernels (csrc/*.hip) and their argument structs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rtla_device.h"

namespace rtla {

// LDS bytes a k_expand / k_expand_batch block of `wpb` waves needs.
size_t expand_lds_bytes(const Layout& L, int wpb);
// Waves per block of the lane-per-state row builders (k_build_winners).
int expand_lane_wpb(const Layout& L);
// Waves per block of the compacting level kernel (0: not usable).
int expand_compact_wpb(const Layout& L);
// Blocks of 4 waves that fit on one CU given the LDS footprint.
int expand_blocks_per_cu(const Layout& L);

// Where a shard's new states of a level go: its next level's rows, the parent
// records (record next_base + g for state g) and how many states fit.
struct FrontierOut {
  Ring next;
  uint64_t* parents;
  uint64_t next_base, next_cap;
};

// Arguments of one level launch (launch_expand): frontier states [s_begin,
// s_end) of `cur`, whose parent records start at cur_base.
struct LevelArgs {
  Layout L{};
  Ring cur{};
  uint64_t s_begin = 0, s_end = 0, cur_base = 0;
  FrontierOut out{};
  uint64_t* table = nullptr;
  int tlog2 = 1;
  DevCounters* ctr = nullptr;
  ShardBox box{1, 0, 0, 0, nullptr, nullptr, nullptr};  // (one shard: no outbox)
  hipStream_t st = nullptr;
  int xflags = 0;
  uint64_t* sent = nullptr;  // multi-shard: the sent cache
  int grid = 1;              // blocks of the wave-per-state kernel
  int* query = nullptr;      // non-null: store {waves launched at most, GROUP} of this launch, launch nothing
};
// The level kernel's shape for layout L (multi-shard or not): the most waves
// one launch keeps resident and its frontier states per group.  false: the
// layout runs the wave-per-state kernel (no group queue).
bool level_kernel_shape(const Layout& L, bool multi, int xflags, int* waves, int* group);
// Multi-shard exchange round: move the overflow list of the previous round
// (in_fp / in_ref, *in_count records) into the outbox regions of `box` (slots
// reserved on box.out_count); records whose region is full go to box's
// overflow list.
hipError_t launch_requeue(const uint64_t* in_fp, const uint64_t* in_ref, const uint64_t* in_count, uint64_t max_count,
                          const ShardBox& box, DevCounters* ctr, hipStream_t st);
// Multi-shard exchange round: out[G] = frontier states left for the next
// round -- `rest` past the launch's range, plus those of its `span` states the
// level kernel did not take (all taken unless `grouped`: then group_next *
// group_size were) -- and out[G + 1] = records on the overflow list.
hipError_t launch_refused(hipStream_t st);  // fault injection: a launch the runtime refuses
hipError_t launch_round_tail(const DevCounters* ctr, uint64_t* out, int G, uint64_t span, uint64_t rest, bool grouped,
                             const uint64_t* over_count, hipStream_t st);
// The level kernel's instantiations, one translation unit each (compiled in
// parallel): *done = false if the unit has no kernel for a.L.
hipError_t launch_compact_spec_a(const LevelArgs& a, bool* done);     // configs[1], configs[0], exhaust
hipError_t launch_compact_spec_b(const LevelArgs& a, bool* done);     // configs[2], configs[4], configs[3] (SYMMETRY)
hipError_t launch_compact_sym_a(const LevelArgs& a, bool* done);      // SYMMETRY, N = 1..3, run-time layout
hipError_t launch_compact_sym_b(const LevelArgs& a, bool* done);      // SYMMETRY, N = 4, 5, run-time layout
hipError_t launch_compact_generic_a(const LevelArgs& a, bool* done);  // N = 1..3, run-time layout
hipError_t launch_compact_generic_b(const LevelArgs& a, bool* done);  // N = 4, 5, run-time layout

// One level (or exchange round) of one shard: k_expand_compact, or the wave-per-state k_expand for rows too wide
// for its LDS tile (and XF_WAVE_KERNEL).  mid: recorded after the level kernel.
hipError_t launch_expand(const LevelArgs& a, hipEvent_t mid = nullptr);
// The wave-per-state level kernel (rtla_kwave.hip).
hipError_t launch_wave_expand(const LevelArgs& a);
// Random walks from the frontier (rtla_ksim.hip, rtla_sim.h): walks [0, n_walks) of the batch starting at global
// walk id `first`, steps t0 + 1 .. t1 of depth; carry (n_walks rows) only when the depth is split across launches.
struct SimCounters;
size_t simulate_lds_bytes(const Layout& L, int wpb);
hipError_t launch_simulate(const Layout& L, const Ring& cur, uint64_t n_front, uint64_t seed, uint64_t first,
                           uint32_t n_walks, int t0, int t1, int depth, uint32_t* carry, uint64_t* ends,
                           SimCounters* ctr, hipStream_t st);
// The same walks carrying user properties (k_simulate_pred): prog holds the state set's
// program (n_state words, 0: none) and, at word PRED_MAX_WORDS, the action set's (n_step words); ends: 5 words a walk.
hipError_t launch_simulate_pred(const Layout& L, const Ring& cur, uint64_t n_front, uint64_t seed, uint64_t first,
                                uint32_t n_walks, int t0, int t1, int depth, uint32_t* carry, uint64_t* ends,
                                SimCounters* ctr, const uint32_t* prog, int n_state, int n_step, hipStream_t st);
// The audit (rtla_kaudit.hip, rtla_audit.h): L.inv_mask evaluated on rows [0, n) of `cur` (succ 0) or on their
// enabled successors (succ 1); masks (n ints) may be null; ctr: counts added, least violation key kept.
struct AuditCounters;
hipError_t launch_audit(const Layout& L, const Ring& cur, uint64_t n, int succ, int* masks, AuditCounters* ctr,
                        hipStream_t st);
// A compiled predicate set (rtla_kpred.hip, rtla_pred.h) on rows [0, n) of `cur`: prog, nwords program words in
// device memory; masks and ctr as launch_audit's (bit k = definition k).
hipError_t launch_pred(const Layout& L, const Ring& cur, uint64_t n, const uint32_t* prog, int nwords, int* masks,
                       AuditCounters* ctr, hipStream_t st);
// A compiled action set on every step (row, enabled successor) out of rows [0, n) of `cur` (k_pred_step): masks
// the OR over each row's steps; the key carries the step's instance.
hipError_t launch_pred_step(const Layout& L, const Ring& cur, uint64_t n, const uint32_t* prog, int nwords,
                            int* masks, AuditCounters* ctr, hipStream_t st);
// The constraint pass (rtla_kconstrain.hip, rtla_constrain.h).  launch_constrain_pack:
// masks[0, n) of launch_pred -> keep[g], the ballot of "mask == 0" over group g of 64 rows; the rows with a mask
// are added to tot->dropped.  launch_constrain_move: one chunk -- rows [first, first + rows) of `cur`, first a
// multiple of 64, keep and offs (rows / 64 words, scratch) the chunk's own -- compacted in place behind the
// chunks before it: scan, gather into stage / stage_par (rows * W + 4 words, rows records), copy-back; parents:
// the level's records (row g's at parents[g]).  Chunks are enqueued in ascending order on one stream.
struct ConstrainTotals;
hipError_t launch_constrain_pack(const int* masks, uint64_t n, uint64_t* keep, ConstrainTotals* tot, hipStream_t st);
hipError_t launch_constrain_move(const Ring& cur, int W, uint64_t first, uint64_t rows, const uint64_t* keep,
                                 uint32_t* offs, uint64_t* parents, uint32_t* stage, uint64_t* stage_par,
                                 ConstrainTotals* tot, hipStream_t st);
hipError_t launch_insert_remote(const uint64_t* recv_fp, const uint64_t* counts, int nshard, uint64_t cap,
                                uint64_t* table, int tlog2, uint32_t* ans, DevCounters* ctr, uint64_t max_count,
                                hipStream_t st);
// Sender side of an exchange round (k_build_winners): the owners' answers `ans` to the records `send_ref` of the
// nshard outbox regions (`cap` slots each, counts[p] used, at most max_count in any).  exp_cap > 0: re-homing, the
// winners go to export region p of exp_rows while it has room.
struct WinnerArgs {
  Layout L;
  Ring cur;
  uint64_t cur_base;
  int me;
  const uint64_t* send_ref;
  const uint32_t* ans;
  const uint64_t* counts;
  int nshard;
  uint64_t cap;
  FrontierOut out;
  DevCounters* ctr;
  uint64_t max_count;
  uint32_t* exp_rows;
  uint64_t exp_cap;
  hipStream_t st;
};
hipError_t launch_build_winners(const WinnerArgs& a);
hipError_t launch_unpack_rows(int W, const uint32_t* rows, const uint64_t* counts, const uint64_t* bases, int nshard,
                              uint64_t rows_cap, const FrontierOut& out, DevCounters* ctr, uint64_t max_count,
                              hipStream_t st);
hipError_t launch_stage_rows(int W, const Ring& next, const uint64_t* parents, uint64_t next_base, uint64_t first,
                             uint64_t n, uint32_t* rows, hipStream_t st);
hipError_t launch_insert_rows(const Layout& L, const uint32_t* rows, uint64_t n, uint64_t* table,
                              int tlog2, int* new_flags, DevCounters* ctr, hipStream_t st);
hipError_t launch_expand_batch(const Layout& L, const uint32_t* rows, uint64_t n, uint32_t* out,
                               uint64_t* info, uint64_t cap, DevCounters* ctr, hipStream_t st);
hipError_t launch_random_rows(const Layout& L, uint64_t seed, uint64_t first, uint64_t n, uint64_t pool, uint32_t* out,
                              hipStream_t st);
hipError_t launch_probe_bench(uint64_t* table, int tlog2, uint64_t n, uint64_t seed,
                              DevCounters* ctr, hipStream_t st, int load_first = 0);
hipError_t launch_probe_mixed(uint64_t* table, int tlog2, uint64_t n, uint64_t n_present, double new_frac,
                              uint64_t seed, DevCounters* ctr, hipStream_t st);
hipError_t launch_fpset_probe(uint64_t* table, int tlog2, const uint64_t* fps, uint64_t n, int proto,
                              unsigned char* is_new, DevCounters* ctr, hipStream_t st);

}  // namespace rtla
