// rtla_kaudit.h -- what the audit kernels (rtla_kaudit.hip) and the predicate
// kernels (rtla_kpred.hip) share on the device: the staging tile's size, the
// per-bit ballot counts, the end-of-kernel tally, and the two streams --
// audit_row_stream over the rows themselves (k_audit_state, k_pred_state) and
// audit_succ_stream over their enabled successors (k_pred_step; k_audit_succ
// keeps the same loop written out, see rtla_kaudit.hip).
// A kernel lays out its LDS, passes what it evaluates as a lambda and ends with
// audit_finish.  Both streams count per mask bit with ballots into wave-uniform
// registers and keep the wave's least violation key (audit_key, rtla_audit.h).
#pragma once
#include "rtla_kdev.h"
#include "rtla_audit.h"

namespace {

constexpr int AUDIT_HEAD = 8;  // the block's tally: u32 words at the start of the dynamic LDS (32 bytes)

// Rows of a state-audit staging tile: the most (a power of two <= 64) that fit in `bytes` per wave
// (k_audit_state: 12 KB, four waves: 48 KB of the 64 KB a block may ask for; configs[1]'s 43-word
// rows take 10.75 KB).
__host__ __device__ constexpr int audit_tile_rows(int W, int bytes = 12288) {
  int tr = 64;
  while (tr > 4 && tr * W * 4 > bytes) tr >>= 1;
  return tr;
}

// Per-bit ballots of `bad` added to the wave-uniform counts; returns the OR over the wave.
template <int NC>
__device__ __forceinline__ int audit_count(int bad, unsigned int (&cnt)[NC]) {
  int any = 0;
#pragma unroll
  for (int k = 0; k < NC; k++) {
    const int c = __popcll(__ballot(bad >> k & 1));
    cnt[k] += (unsigned int)c;
    any |= c ? 1 << k : 0;
  }
  return any;
}

// End of kernel: the wave's counts -> the block's LDS tally -> the device counters; the wave's least key.
template <int NC>
__device__ __forceinline__ void audit_finish(unsigned int* tally, const unsigned int (&cnt)[NC],
                                             unsigned long long evaluated, unsigned long long vkey, AuditCounters* ctr,
                                             int lane) {
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < NC; k++)
      if (cnt[k]) atomicAdd(&tally[k], cnt[k]);
    if (evaluated) atomicAdd(&ctr->evaluated, evaluated);
    if (vkey != AUDIT_NO_VIOLATION) atomicMin(&ctr->viol_key, vkey);
  }
  cover_flush(tally, NC, ctr->counts);
}

// The stream over rows [0, n) of `cur` themselves.  A wave takes 64 consecutive
// rows (a group never wraps the ring), in tiles of `tr` rows: it copies a tile
// into `tile` (the wave's LDS) with 16-byte loads, coalesced, and lane l < the
// tile's rows calls eval(row l in LDS) -> its mask -- the row stride W is odd,
// so the lanes' reads of word k fall on different banks.  masks (may be null):
// each row's mask.  (A wave's counts are u32: it sees far fewer than 2^32 rows.)
template <int NC, class E>
__device__ __forceinline__ void audit_row_stream(const Ring& cur, unsigned long long n, int W, int tr, uint32_t* tile,
                                                 int* __restrict__ masks, unsigned int (&cnt)[NC],
                                                 unsigned long long& evaluated, unsigned long long& vkey, int wave,
                                                 int wpb, int lane, E eval) {
  const unsigned long long ngroup = (n + 63) >> 6;
  for (unsigned long long g = (unsigned long long)blockIdx.x * wpb + wave; g < ngroup;
       g += (unsigned long long)gridDim.x * wpb) {
    const int nv = (int)min<unsigned long long>(64ull, n - (g << 6));
    for (int r0 = 0; r0 < nv; r0 += tr) {
      const int nt = min(tr, nv - r0);
      const unsigned long long first = (g << 6) + r0;
      copy_words_lds16(tile, ring_row(cur, first, W), nt * W, lane);
      wave_sync();
      int bad = 0;
      if (lane < nt) {
        bad = eval((const uint32_t*)(tile + lane * W));
        if (masks) masks[first + lane] = bad;
      }
      const unsigned long long mb = __ballot(bad != 0);
      if (mb) {
        audit_count(bad, cnt);
        if (vkey == AUDIT_NO_VIOLATION) {  // groups and tiles ascend: the wave's first is its least
          const int fl = __builtin_ctzll(mb);
          vkey = audit_key(first + fl, 0, 1, __shfl(bad, fl));
        }
      }
      evaluated += nt;
      wave_sync();
    }
  }
}

// The stream over every enabled successor of rows [0, n): one wave per state.
// load(s) brings state s into `prow` (the wave's LDS), visible to every lane;
// each lane then takes one candidate instance of the state, 64 at a time
// (candidate_delta), and the whole wave calls eval(en, m, inst, d) -> this
// lane's mask (0 where !en) for each chunk with an enabled successor, m being
// the ballot of en.  masks (may be null): the OR over each row's successors.
template <int NS, int NC, class LD, class E>
__device__ __forceinline__ void audit_succ_stream(const Layout& L, unsigned long long n, uint32_t* prow,
                                                  int* __restrict__ masks, unsigned int (&cnt)[NC],
                                                  unsigned long long& evaluated, unsigned long long& vkey,
                                                  AuditCounters* ctr, int wave, int wpb, int lane, LD load, E eval) {
  const int fixed = L.fam[F_RECEIVE];
  for (unsigned long long s = (unsigned long long)blockIdx.x * wpb + wave; s < n;
       s += (unsigned long long)gridDim.x * wpb) {
    load(s);
    const int nmsg = row_nmsg(L, prow);
    const int ncand = fixed + 3 * nmsg;
    int all = 0;
    bool found = false;
    for (int base = 0; base < ncand; base += 64) {
      DeltaT<NS> d;
      int inst;
      const bool en = candidate_delta<NS>(L, prow, base + lane, ncand, nmsg, &ctr->flags, inst, d);
      const unsigned long long m = __ballot(en);
      if (!m) continue;
      evaluated += __popcll(m);
      const int bad = eval(en, m, inst, d);
      const unsigned long long mb = __ballot(bad != 0);
      if (mb) {
        all |= audit_count(bad, cnt);
        if (!found) {  // the row's least instance with a mask: instances ascend with the candidates
          found = true;
          const int fl = __builtin_ctzll(mb);
          const unsigned long long key = audit_key(s, __shfl(inst, fl), __shfl((int)d.in_model, fl), __shfl(bad, fl));
          if (key < vkey) vkey = key;
        }
      }
    }
    if (masks && lane == 0) masks[s] = all;
    wave_sync();
  }
}

}  // namespace
