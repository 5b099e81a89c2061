// rtla_device.h -- structures shared by the kernels and the host driver.
#pragma once
#include <stdint.h>

#include "../../include/rtla.h"
#include "rtla_model.h"

namespace rtla {

// Coverage codes: the 10 Next families, with Receive split into its 6
// sub-actions (UpdateTerm, HandleRequestVoteRequest, HandleRequestVoteResponse,
// HandleAppendEntriesRequest, HandleAppendEntriesResponse, DropStaleResponse).
constexpr int COVER_CODES = (int)F_COUNT + (int)R_NONE;

enum {
  FLAG_SPEC_ERROR = 1,      // TLC evaluation error (sequence index outside its domain)
  FLAG_ROW_OVERFLOW = 2,    // bag / elections capacity of the row format exceeded
  FLAG_FRONTIER_FULL = 4,   // next-frontier buffer too small
  FLAG_FPSET_FULL = 8,      // fingerprint set probe limit hit
  FLAG_OUTBOX_FULL = 16,    // exchange outbox region too small
  FLAG_BAD_INDEX = 32,      // RTLA_CHECKED builds: a global index outside its buffer
  FLAG_LOCAL_FAILURE = 64,  // (host) a rank's local work failed: carried to every rank in the level reduction
};
static_assert(FLAG_SPEC_ERROR == RTLA_CAP_SPEC_ERROR && FLAG_ROW_OVERFLOW == RTLA_CAP_ROW &&
                  FLAG_FRONTIER_FULL == RTLA_CAP_FRONTIER && FLAG_FPSET_FULL == RTLA_CAP_FPSET &&
                  FLAG_OUTBOX_FULL == RTLA_CAP_OUTBOX,
              "rtla.h RTLA_CAP_* mirror the device flags");

// Most shards in one job (one per GPU of an 8-GPU node, or virtual shards on
// one device): the expand kernels keep per-owner outbox state in registers /
// LDS sized by it, and rtla_open refuses more (RTLA_E_CONFIG).
constexpr int SHARD_MAX = 8;
// Outbox slots a wave of the level kernel reserves per owner at a time.
constexpr int OBOX_CHUNK = 256;

// Fingerprint ownership across shards (ranks): low 32 bits of fp.a scaled to
// [0, nshard).  The fingerprint-set home slot uses the TOP bits of fp.a, so
// ownership and placement are independent.
RTLA_HD int fp_owner(FP f, int nshard) {
  return (int)(((f.a & 0xffffffffull) * (unsigned long long)nshard) >> 32);
}

// ---- the three 64-bit records, each defined here alone.
// Parent record of a stored state: shard << 56 | index << 16 | instance -- the
// shard that holds its parent, the parent's index among that shard's parent
// records (40 bits), the action instance that produced it.
RTLA_HD uint64_t parent_record(uint64_t shard, uint64_t index, uint64_t inst) { return shard << 56 | index << 16 | inst; }
RTLA_HD uint64_t parent_shard(uint64_t r) { return r >> 56; }
RTLA_HD uint64_t parent_index(uint64_t r) { return (r >> 16) & ((1ull << 40) - 1); }
RTLA_HD int parent_inst(uint64_t r) { return (int)(r & 0xffff); }
// Successor record (rtla_expand_batch, ABI: include/rtla.h): input index << 32
// | in_model << 31 | receive-sub << 16 | instance.  The low 31 bits are the
// label rtla_trace returns.
RTLA_HD uint64_t successor_info(uint64_t input, bool in_model, uint64_t sub, uint64_t inst) {
  return input << 32 | (uint64_t)(in_model ? 1u : 0u) << 31 | sub << 16 | inst;
}
RTLA_HD uint64_t successor_input(uint64_t r) { return r >> 32; }
RTLA_HD int successor_inst(uint64_t r) { return (int)(r & 0xffff); }
RTLA_HD int32_t successor_label(uint64_t r) { return (int32_t)(r & 0x7fffffffu); }
// Outbox ref of a queued successor (ShardBox::send_ref): parent's index in the
// sender's current level << 16 | instance.
RTLA_HD uint64_t outbox_ref(uint64_t parent, uint64_t inst) { return parent << 16 | inst; }
RTLA_HD uint64_t outbox_parent(uint64_t r) { return r >> 16; }
RTLA_HD int outbox_inst(uint64_t r) { return (int)(r & 0xffff); }

// A BFS level's rows inside the shard's row arena.  The arena (`cap` rows, a
// multiple of 64) is used as a ring: state g of the level is row
// (start + g) mod cap.  The next level starts at the first multiple of 64 past
// the current one, so one level's rows never overlap the next level's, both
// together may fill the whole arena (TLC's disk queue needs no second buffer
// either), and a group of 64 states starting at a multiple of 64 never wraps.
struct Ring {
  uint32_t* base;
  unsigned long long start, cap;
};
RTLA_HD unsigned long long ring_idx(const Ring& r, unsigned long long g) {
  const unsigned long long i = r.start + g;  // start < cap and g < cap
  return i >= r.cap ? i - r.cap : i;
}

// Outbox of one shard for one exchange round: region p (capacity `cap`
// records) holds the successors owned by shard p.  The level kernel stops
// taking frontier groups once any region holds `stop_at` records; what the
// groups already in flight still queue past a region's end goes to the
// overflow list (owner mixed, sent in the next round).  The overflow's
// capacity covers every in-flight group queueing all its candidates.
struct ShardBox {
  int nshard, me;
  unsigned long long cap;
  int slog2;                      // log2 slots of the sent cache (MULTI; 0 = no sent cache)
  unsigned long long* out_count;  // [nshard]
  unsigned long long* send_fp;    // [nshard][cap][2]
  unsigned long long* send_ref;   // [nshard][cap]: local parent index << 16 | instance
  unsigned long long stop_at;     // k_expand_compact: no new group once a region holds this many
  unsigned long long* over_fp;    // [over_cap][2]: records past their region's end
  unsigned long long* over_ref;   // [over_cap]
  unsigned long long* over_count; // its fill counter
  unsigned long long over_cap;
};

// Diagnostic switches of the expand kernels (rtla_time_expand, RTLA_XFLAGS; 0 in the BFS).
enum {
  XF_NO_PROBE = 1,        // skip the fingerprint-set CAS (every successor "seen")
  XF_NO_COVER = 2,        // skip the coverage counters
  XF_NO_HASH = 4,         // replace the fingerprint delta by a trivial sum
  XF_NO_MATERIALIZE = 8,  // compact kernel: write parent records but not the rows of new states
  XF_NO_CHUNKS = 32,      // compact kernel: load rows + per-state setup only
  XF_NO_DELTA = 64,       // compact kernel: compaction without evaluating actions
  XF_GENERIC_DELTA = 128, // compact kernel: never use the per-family specialised evaluation
  XF_BLOCK4 = 256,        // compact kernel: 4-wave workgroups instead of 1
  XF_NO_PERSIST = 512,    // compact kernel: one group per wave instead of persistent waves
  XF_CAS_ONLY = 1024,     // compact kernel: probe with CAS only (no load-first)
  XF_WAVE_KERNEL = 2048,  // use the wave-per-state k_expand (the fallback for rows too wide for the compact tile)
  XF_NO_SPECIAL = 4096,   // compact kernel: run-time layout even for a compiled-in configuration
  XF_DEDUP_ONLY = 8192,   // compact kernel: count new fingerprints, build no rows (synthetic microbench)
  XF_ALL_SUCCESSORS = 16384,  // compact kernel: no seen set -- every enabled successor (in-model or not) gets a
                              // row, its record = successor_info(input index, in_model, sub, instance)
                              // (rtla_expand_batch: the parity seam runs the hot kernel)
};

// Phase slots of the level kernel's cycle stamps: the diagnostic build (RTLA_STAMPS, every unit compiled
// with it) splits the group start into tile load and per-state setup and so has one more.
#ifdef RTLA_STAMPS
#define RTLA_NSTAMP 9
#else
#define RTLA_NSTAMP 8
#endif
// Per-level device counters (zeroed before each level except `cover`).
struct DevCounters {
  unsigned long long generated;
  unsigned long long next_count;
  unsigned long long probes;
  int flags;
  int viol_mask;
  int viol_inst;
  int viol_in_model;
  unsigned long long viol_parent;
  unsigned long long viol_child;
  unsigned long long group_next;  // k_expand_compact's work queue (zeroed before each launch)
  unsigned long long group_size;  // frontier states per group of the last k_expand_compact launch
  unsigned long long stamp[RTLA_NSTAMP];  // RTLA_STAMPS builds: cycles per level-kernel phase, summed over waves
  unsigned long long cas;         // RTLA_COUNT_CAS builds: pipelined fingerprint-set CAS issued by the level kernel
  unsigned long long exp[SHARD_MAX];  // multi-shard: export slots reserved for owner p (re-homed at level end) ...
  unsigned long long exp_cut[SHARD_MAX];  // ... and 1 + the first slot of the batch that did not fit (0: none)
  // buffer capacities (rows of the current / next frontier, parent records), for RTLA_CHECKED builds
  unsigned long long cap_cur, cap_next, cap_parents;
  unsigned long long cover[2 * COVER_CODES];  // [0,C): generated, [C,2C): distinct
};

// Rows in export region p after a level: the slots reserved, up to the batch
// that did not fit (k_build_winners: that batch and every later one went to
// the shard's own next level).
RTLA_HD unsigned long long exported_rows(const DevCounters& c, int p, unsigned long long cap) {
  return c.exp[p] <= cap ? c.exp[p] : c.exp_cut[p] ? c.exp_cut[p] - 1 : cap;
}

}  // namespace rtla
