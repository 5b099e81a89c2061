// rtla_kpack.hip -- lane-per-state row builders: the multi-shard sender's
// k_build_winners and the wave-per-state k_expand_batch (the parity seam's
// fallback for rows too wide for the level kernel).  Shared device helpers,
// pick_layout and the compiled-in layouts: rtla_kdev.h.
#include "rtla_kdev.h"

// Sender side of the two-phase exchange: the owners
// answered every queued (fingerprint, parent) record with "new" (nonzero) or
// "seen"; the sender builds each winner ITSELF -- gathers its parent row
// (this shard's current level) into LDS, recomputes the successor's Delta,
// patches the row in place -- with a local parent record.  Invariants and
// distinct coverage are evaluated here, where parent and action are known.
// Where the row goes: with re-homing (exp_cap > 0: the owner is a hash of the
// state's projection, rtla_model.h proj32, so a state's successors are
// mostly its owner's) into EXPORT REGION p of the staging area (the owner's:
// rtla_step moves it there at level end, so the state is expanded where most
// of its successors are owned); when that region is full -- or without
// re-homing (SYMMETRY: the owner is a hash of the orbit key) -- appended to
// this shard's own next level.
// LC: compiled-in layout (Layout{} = run-time Lrt), as for the level kernel.
constexpr int BW_QUEUE = 128;  // per-wave LDS queue of winner refs (u64): batches of 64 winners
__host__ __device__ constexpr int build_winners_lds_words(int W, int AW) {
  return lane_lds_words(W, AW) + 2 * BW_QUEUE;
}
template <int NS, Layout LC>
__global__ void __launch_bounds__(256)
k_build_winners(Layout Lrt, Ring cur, unsigned long long cur_base, int me,
                const unsigned long long* __restrict__ send_ref, const uint32_t* __restrict__ ans,
                const unsigned long long* __restrict__ counts, int nshard, unsigned long long cap, Ring next,
                unsigned long long* __restrict__ parents, unsigned long long next_base, unsigned long long next_cap,
                DevCounters* ctr, uint32_t* __restrict__ exp_rows, unsigned long long exp_cap) {
  // A wave scans 64 records of owner p (grid.y) at a time and queues the
  // winners' refs in LDS; every 64 queued winners -- one full wave -- it
  // gathers their parent rows into LDS (one coalesced read per row), builds
  // each successor in place, reserves next-level slots with one atomic and
  // stores the rows (one coalesced write per row) and parent records.  (A
  // batch per 64 records instead would run compute_delta on the ~quarter of
  // the lanes whose record won.)
  const Layout& L = pick_layout<LC>(Lrt);
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  __shared__ unsigned int cov[COVER_CODES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  const int W = L.W, AW = L.all_words;
  uint32_t* lrows = lds + wave * build_winners_lds_words(W, AW);
  const LaneWords pall{lrows + 64 * W + lane};
  unsigned long long* q = reinterpret_cast<unsigned long long*>(lrows + lane_lds_words(W, AW));
  cover_zero(cov, COVER_CODES);
  const unsigned long long p = blockIdx.y;  // owner shard
  const unsigned long long n = min(counts[p], cap);  // (reservations may run past the region: the overflow list)
  // build the first nw queued winners (q[0, nw): their outbox refs)
  auto build = [&](int nw) {
    // export slots for all nw (owner p's region), or none: the batch then goes
    // to this shard's next level.  One atomicAdd (a CAS loop that reserves only
    // what fits serialises the waves on the counter: 10x slower); the batch
    // that crosses the region's end records where it started, so the region's
    // rows are exactly [0, that slot) (exported_rows).
    unsigned long long ebase = ~0ull;
    if (exp_cap && lane == 0) {
      ebase = atomicAdd(&ctr->exp[p], (unsigned long long)nw);
      if (ebase + (unsigned long long)nw > exp_cap) {
        if (ebase < exp_cap) ctr->exp_cut[p] = ebase + 1;
        ebase = ~0ull;
      }
    }
    ebase = shfl0_u64(ebase);
    const bool exported = ebase != ~0ull;
    unsigned long long obase = 0;
    if (!exported) obase = reserve_rows(&ctr->next_count, nw, next_cap, ctr, lane);
    const bool act = lane < nw;
    const unsigned long long ref = act ? q[lane] : 0ull;
    const unsigned long long s = outbox_parent(ref);  // parent: state s of the current level
    const int inst = outbox_inst(ref);
    gather_rows_lds(lrows, W, nw, [&](int r) { return ring_row(cur, readlane_u64(s, r), W); }, lane);
    wave_sync();
    uint32_t* prow = lrows + lane * W;
    if (act) {
      const FP pfp = fp_add(row_fp(prow), alllogs_delta<NS>(L, prow, pall));
      DeltaT<NS> d;
      compute_delta<NS>(L, prow, inst, d);
      const FP cfp = fp_add(pfp, delta_fp<NS>(L, prow, d));
      const int bad = check_invariants_v<NS>(L, prow, d.srv, d.rec[0], d.rec[1], d.elec, d.erec[0]);
      if (claim_violation_lane(ctr, bad))  // (an exported row has no home yet: the trace replays the instance from the parent)
        record_violation(ctr, cur_base + s, inst, 1,
                         !exported && obase + lane < next_cap ? next_base + obase + lane : ~0ull);
      atomicAdd(&cov[cover_code(L, inst, d.sub)], 1u);
      materialize<NS>(L, prow, d, pall, cfp, prow);  // in place
    }
    wave_sync();
    const unsigned long long prec = parent_record(me, cur_base + s, inst);
    if (exported) {  // the k_unpack_rows format: W row words, then the parent record's two halves
      const int RW = W + 2;
      uint32_t* dst = exp_rows + ((unsigned long long)p * exp_cap + ebase) * (unsigned long long)RW;
      int r = 0, w = lane;
      while (w >= W) { w -= W; r++; }
      for (int i0 = 0; i0 < nw * W; i0 += 64) {
        if (i0 + lane < nw * W) dst[r * RW + w] = lrows[i0 + lane];
        w += 64;
        while (w >= W) { w -= W; r++; }
      }
      if (act) {
        dst[lane * RW + W] = (uint32_t)prec;
        dst[lane * RW + W + 1] = (uint32_t)(prec >> 32);
      }
    } else {
      const int nrows = obase >= next_cap ? 0 : (int)min<unsigned long long>((unsigned long long)nw, next_cap - obase);
      store_rows_ring(next, obase, nrows, W, lrows, lane);
      if (lane < nrows) parents[next_base + obase + lane] = prec;
    }
    wave_sync();
  };
  int qn = 0;  // winners queued (wave-uniform)
  const unsigned long long lanes_below = (1ull << lane) - 1ull;
  for (unsigned long long k0 = ((unsigned long long)blockIdx.x * wpb + wave) * 64ull; k0 < n;
       k0 += (unsigned long long)gridDim.x * wpb * 64ull) {
    const unsigned long long k = k0 + lane;
    const bool win = k < n && ans[p * cap + k] != 0u;
    const unsigned long long m = __ballot(win);
    if (win) q[qn + __popcll(m & lanes_below)] = send_ref[p * cap + k];
    qn += __popcll(m);
    wave_sync();
    if (qn >= 64) {
      build(64);
      qn -= 64;
      if (lane < qn) q[lane] = q[64 + lane];  // (the rest moves to the front: fewer than 64)
      wave_sync();
    }
  }
  if (qn) build(qn);
  cover_flush(cov, COVER_CODES, ctr->cover + COVER_CODES);  // distinct coverage
}

// Parity seam: every enabled successor of every input row (in-model or not),
// materialised.  out_info[k] = the successor record (successor_info, rtla_device.h).
template <int NS>
__global__ void __launch_bounds__(256)
k_expand_batch(Layout L, const uint32_t* __restrict__ rows, unsigned long long n, uint32_t* __restrict__ out,
               unsigned long long* __restrict__ out_info, unsigned long long cap, DevCounters* ctr) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  const int W = L.W;
  const auto [prow, pall, hsrv, stage] = wave_lds(lds, wave, W);
  const int fixed = L.fam[F_RECEIVE];
  for (unsigned long long s = (unsigned long long)blockIdx.x * wpb + wave; s < n;
       s += (unsigned long long)gridDim.x * wpb) {
    const FP pfp = load_parent<NS>(L, rows + s * (unsigned long long)W, prow, pall, hsrv, lane);
    const int nmsg = row_nmsg(L, prow);
    const int ncand = fixed + 3 * nmsg;
    for (int base = 0; base < ncand; base += 64) {
      DeltaT<NS> d;
      int inst;
      const bool en = candidate_delta<NS>(L, prow, base + lane, ncand, nmsg, &ctr->flags, inst, d);
      const unsigned long long m = __ballot(en);
      const int cnt = __popcll(m);
      if (!cnt) continue;
      const int rank = __popcll(m & ((1ull << lane) - 1ull));
      const unsigned long long obase = reserve_rows(&ctr->next_count, cnt, cap, ctr, lane);
      if (obase + cnt > cap) continue;  // (a batch that does not fit whole is dropped)
      const FP cfp = en ? fp_add(pfp, delta_fp<NS>(L, prow, d)) : FP{0, 0};
      for (int b = 0; b < cnt; b += STAGE_ROWS) {
        if (en && rank >= b && rank < b + STAGE_ROWS) materialize<NS>(L, prow, d, pall, cfp, stage + (rank - b) * W);
        wave_sync();
        const int nb = min(STAGE_ROWS, cnt - b);
        uint32_t* dst = out + (obase + b) * (unsigned long long)W;
        for (int w = lane; w < nb * W; w += 64) dst[w] = stage[w];
        wave_sync();
      }
      if (en) out_info[obase + rank] = successor_info(s, d.in_model, d.sub, inst);
    }
  }
}

namespace rtla {

hipError_t launch_build_winners(const WinnerArgs& a) {
  if (!a.max_count) return hipSuccess;
  auto launch = [&](auto kernel) {
    const size_t per = (size_t)build_winners_lds_words(a.L.W, a.L.all_words) * sizeof(uint32_t);
    const int wpb = per * 4 <= 64 * 1024 ? 4 : (per * 2 <= 64 * 1024 ? 2 : 1);
    hipLaunchKernelGGL(kernel, dim3(grid_x(a.max_count, 1024 * wpb), a.nshard), dim3(64 * wpb), (size_t)wpb * per,
                       a.st, a.L, a.cur, (unsigned long long)a.cur_base, a.me, (const unsigned long long*)a.send_ref,
                       a.ans, (const unsigned long long*)a.counts, a.nshard, (unsigned long long)a.cap, a.out.next,
                       (unsigned long long*)a.out.parents, (unsigned long long)a.out.next_base,
                       (unsigned long long)a.out.next_cap, a.ctr, a.exp_rows, (unsigned long long)a.exp_cap);
    return hipGetLastError();
  };
  // the BASELINE layouts bench.py shards (compiled in, as for the level kernel)
  if (same_layout(a.L, specs::CFG2)) return launch(k_build_winners<specs::CFG2.N, specs::CFG2>);
  if (same_layout(a.L, specs::CFG1)) return launch(k_build_winners<specs::CFG1.N, specs::CFG1>);
  if (same_layout(a.L, specs::EXHAUST)) return launch(k_build_winners<specs::EXHAUST.N, specs::EXHAUST>);
  if (same_layout(a.L, specs::CFG3)) return launch(k_build_winners<specs::CFG3.N, specs::CFG3>);
  if (same_layout(a.L, specs::CFG4)) return launch(k_build_winners<specs::CFG4.N, specs::CFG4>);
  switch (a.L.N) {
    case 1: return launch(k_build_winners<1, Layout{}>);
    case 2: return launch(k_build_winners<2, Layout{}>);
    case 3: return launch(k_build_winners<3, Layout{}>);
    case 4: return launch(k_build_winners<4, Layout{}>);
    default: return launch(k_build_winners<5, Layout{}>);
  }
}

hipError_t launch_expand_batch(const Layout& L, const uint32_t* rows, uint64_t n, uint32_t* out, uint64_t* info,
                               uint64_t cap, DevCounters* ctr, hipStream_t st) {
  if (n == 0) return hipSuccess;
  uint64_t blocks = (n + 3) / 4;
  int grid = (int)(blocks < 4096 ? blocks : 4096);
  RTLA_DISPATCH_N(L, k_expand_batch, dim3(grid), dim3(256), expand_lds_bytes(L, 4), st, L, rows,
                  (unsigned long long)n, out, (unsigned long long*)info, (unsigned long long)cap, ctr);
  return hipGetLastError();
}

}  // namespace rtla
