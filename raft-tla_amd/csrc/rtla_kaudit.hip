// rtla_kaudit.hip -- the audit kernels: invariants evaluated outside the
// search, over a batch of rows or over the frontier in HBM (semantics in
// rtla_audit.h; the host replay computes the same masks, counts and key).
//   * k_audit_state: the rows themselves, by audit_row_stream (rtla_kaudit.h):
//     64 rows per wave staged into LDS in tiles of `tr` rows, each lane
//     evaluates its own row there.
//   * k_audit_succ: every enabled successor: one wave per state, the row in
//     LDS, each lane evaluates one action instance as a Delta and checks
//     parent + delta.  No set, no row building, no outbox.  The loop is its
//     own: it is audit_succ_stream's (rtla_kaudit.h), which k_pred_step runs,
//     but inlined into that stream this kernel measured 3 % slower (DESIGN.md
//     section 12).
// Both count per invariant bit with ballots into wave-uniform registers, add
// them to the block's LDS tally once per wave and to the device counters once
// per block, and report the least violation key with one atomicMin per wave
// (audit_finish).
#include "rtla_kaudit.h"

// Rows [0, n) of `cur`; masks (may be null): the violated mask of each row.
template <int NS>
__global__ void __launch_bounds__(256)
k_audit_state(Layout L, Ring cur, unsigned long long n, int tr, int* __restrict__ masks, AuditCounters* ctr) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  const int W = L.W;
  uint32_t* const tile = lds + AUDIT_HEAD + wave * tr * W;
  cover_zero(lds, AUDIT_HEAD);

  unsigned int cnt[INV_COUNT] = {};
  unsigned long long evaluated = 0, vkey = AUDIT_NO_VIOLATION;
  audit_row_stream(cur, n, W, tr, tile, masks, cnt, evaluated, vkey, wave, wpb, lane, [&](const uint32_t* row) {
    return check_invariants_v<NS>(L, row, -1, 0u, 0u, 0, 0u);
  });
  audit_finish(lds, cnt, evaluated, vkey, ctr, lane);
}

// Every enabled successor of rows [0, n) of `cur`; masks (may be null): the OR over each row's successors.
template <int NS>
__global__ void __launch_bounds__(256)
k_audit_succ(Layout L, Ring cur, unsigned long long n, int* __restrict__ masks, AuditCounters* ctr) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  const int W = L.W;
  uint32_t* const prow = lds + AUDIT_HEAD + wave * even_words(W);
  cover_zero(lds, AUDIT_HEAD);

  unsigned int cnt[INV_COUNT] = {};
  unsigned long long evaluated = 0, vkey = AUDIT_NO_VIOLATION;
  const int fixed = L.fam[F_RECEIVE];
  for (unsigned long long s = (unsigned long long)blockIdx.x * wpb + wave; s < n;
       s += (unsigned long long)gridDim.x * wpb) {
    const uint32_t* __restrict__ src = ring_row(cur, s, W);
    for (int w = lane; w < W; w += 64) prow[w] = src[w];
    wave_sync();
    const int nmsg = row_nmsg(L, prow);
    const int ncand = fixed + 3 * nmsg;
    int all = 0;
    bool found = false;
    for (int base = 0; base < ncand; base += 64) {
      const int q = base + lane;
      DeltaT<NS> d;
      d.enabled = 0;
      d.in_model = 0;
      int inst = 0;
      if (q < ncand) {
        inst = candidate_inst(L, q, nmsg);
        compute_delta<NS>(L, prow, inst, d);
      }
      const bool en = enabled_ok(&ctr->flags, d.enabled != 0, d.err);
      evaluated += __popcll(__ballot(en));
      const int bad = en ? check_invariants_v<NS>(L, prow, d.srv, d.rec[0], d.rec[1], d.elec, d.erec[0]) : 0;
      const unsigned long long mb = __ballot(bad != 0);
      if (mb) {
        all |= audit_count(bad, cnt);
        if (!found) {  // the row's least violating instance: instances ascend with the candidates
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
  audit_finish(lds, cnt, evaluated, vkey, ctr, lane);
}

namespace rtla {

hipError_t launch_audit(const Layout& L, const Ring& cur, uint64_t n, int succ, int* masks, AuditCounters* ctr,
                        hipStream_t st) {
  if (!n) return hipSuccess;
  const int wpb = 4;
  if (succ) {
    const unsigned grid = (unsigned)std::min<uint64_t>((n + wpb - 1) / wpb, (uint64_t)device_cus() * 16);
    const size_t lds = (size_t)(AUDIT_HEAD + wpb * even_words(L.W)) * sizeof(uint32_t);
    RTLA_DISPATCH_N(L, k_audit_succ, dim3(grid), dim3(64 * wpb), lds, st, L, cur, (unsigned long long)n, masks, ctr);
  } else {
    const int tr = audit_tile_rows(L.W);
    const uint64_t ngroup = (n + 63) / 64;
    const unsigned grid = (unsigned)std::min<uint64_t>((ngroup + wpb - 1) / wpb, (uint64_t)device_cus() * 8);
    const size_t lds = (size_t)(AUDIT_HEAD + wpb * tr * L.W) * sizeof(uint32_t);
    RTLA_DISPATCH_N(L, k_audit_state, dim3(grid), dim3(64 * wpb), lds, st, L, cur, (unsigned long long)n, tr, masks,
                    ctr);
  }
  return hipGetLastError();
}

}  // namespace rtla
