// rtla_kaudit.h -- what the audit kernels (rtla_kaudit.hip) and the predicate
// kernel (rtla_kpred.hip) share on the device: the staging tile's size, the
// per-bit ballot counts, the end-of-kernel tally.
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

}  // namespace
