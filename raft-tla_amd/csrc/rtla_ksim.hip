// rtla_ksim.hip -- k_simulate: random walks from the current frontier (TLC's
// -simulate; semantics in rtla_sim.h, the host replay computes the same walks).
//   * one wavefront per walk, two row buffers in LDS (current and next state)
//     plus the per-parent allLogs' words and server-record hashes
//     (parent_setup, rtla_kdev.h, as k_expand's load_parent);
//   * each step the 64 lanes evaluate the state's action instances 64 at a
//     time (k_expand's chunks); every enabled successor is counted and
//     invariant-checked; lane c keeps the ballot of chunk c's in-model
//     successors, so the pick -- the r-th in-model successor in instance
//     order, r drawn from (seed, walk, step) -- is found by popcounts;
//   * the wave copies the row to the other buffer and the chosen lane patches
//     it (child_patches, incremental fingerprint: as materialize does);
//   * global traffic: the start row, the end record, the counters -- and the
//     current row of a walk whose depth is split across launches.
#include "rtla_kdev.h"
#include "rtla_sim.h"

namespace {

// Per-wave LDS words: two rows | allLogs' words (32) | server-record hashes (4 * NMAX).
__host__ __device__ constexpr int sim_wave_words(int W) { return (2 * even_words(W) + 32 + 4 * NMAX + 3) & ~3; }

// Waves per SIMD the register budget is set for.  A walk's step is one long
// dependent chain (LDS reads of the row, divergent families), so resident
// waves, not registers, bound the kernel: on the configs[1] shape (N = 3) 2 / 3
// / 4 waves per SIMD (193 / 168 / 128 VGPRs, 0 / 17 / 85 spilled) ran 2^21 walks
// x 32 steps in 662 / 494 / 446 ms (profiles/r07_sim).  N = 4, 5 spill 118 /
// 215 VGPRs at 128 and were not measured: they stay at 3 (17 / 30 spilled).
constexpr int sim_waves(int ns) { return ns <= 3 ? 4 : 3; }

}  // namespace

// Walks [0, n_walks) of the batch whose first global walk id is `first`, steps
// t0 + 1 .. t1 of `depth`.  t0 == 0: the walk starts at frontier row
// (first + i) mod n_front; otherwise at carry[i] if ends[4 i + 3] says the walk
// is still running (t0 steps taken, stop code 0).
template <int NS>
__global__ void __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(sim_waves(NS))))
k_simulate(Layout L, Ring cur, unsigned long long n_front, unsigned long long seed, unsigned long long first,
           unsigned int n_walks, int t0, int t1, int depth, uint32_t* __restrict__ carry,
           unsigned long long* __restrict__ ends, SimCounters* ctr) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  __shared__ unsigned int taken[COVER_CODES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  const int W = L.W;
  uint32_t* const wbase = lds + wave * sim_wave_words(W);
  uint32_t* const pall = wbase + 2 * even_words(W);
  FP* const hsrv = reinterpret_cast<FP*>(pall + 32);
  cover_zero(taken, COVER_CODES);

  unsigned long long my_steps = 0, my_gen = 0, my_stuck = 0;  // wave-uniform
  const int fixed = L.fam[F_RECEIVE];
  for (unsigned int i = blockIdx.x * wpb + wave; i < n_walks; i += gridDim.x * wpb) {
    const unsigned long long w = first + i;
    uint32_t* a = wbase;                  // current state
    uint32_t* b = wbase + even_words(W);  // next state
    unsigned long long digest = 0;
    const uint32_t* src;
    if (t0 == 0) {
      src = ring_row(cur, w % n_front, W);
    } else {
      const unsigned long long e = ends[4ull * i + 3];
      if ((e >> 32) != SIM_STOP_DEPTH || (uint32_t)e != (uint32_t)t0) continue;  // ended in an earlier launch
      digest = ends[4ull * i + 2];
      src = carry + (unsigned long long)i * W;
    }
    for (int k = lane; k < W; k += 64) a[k] = src[k];
    wave_sync();
    const uint64_t rbase = sim_rng_base(seed, w);
    int len = t0, stop = SIM_STOP_DEPTH;
    for (int t = t0 + 1; t <= t1; t++) {
      // per-parent data: server-record hashes, allLogs' (raft.tla:465) and its fingerprint change
      const FP pfp = parent_setup<NS>(L, a, pall, hsrv, lane);
      const int nmsg = row_nmsg(L, a);
      const int ncand = min(fixed + 3 * nmsg, SIM_MAX_CAND);  // (the host refuses layouts with more)
      unsigned long long my_mask = 0;  // lane c: ballot of chunk c's in-model successors
      int total = 0, last_chunk = 0;
      unsigned long long vkey = SIM_NO_VIOLATION;
      DeltaT<NS> d;
      int inst = 0;
      for (int base = 0, c = 0; base < ncand; base += 64, c++) {
        const int q = base + lane;
        d.enabled = 0;
        d.in_model = 0;
        inst = 0;
        if (q < ncand) {
          inst = candidate_inst(L, q, nmsg);
          compute_delta<NS>(L, a, inst, d);
        }
        const bool en = enabled_ok(&ctr->flags, d.enabled != 0, d.err);
        my_gen += __popcll(__ballot(en));
        const int bad = en ? check_invariants_v<NS>(L, a, d.srv, d.rec[0], d.rec[1], d.elec, d.erec[0]) : 0;
        const unsigned long long mb = __ballot(bad != 0);
        if (mb && vkey == SIM_NO_VIOLATION) {  // the least violating instance: instances ascend with q
          const int fl = __builtin_ctzll(mb);
          vkey = sim_viol_key(i, (uint32_t)t, __shfl(inst, fl), __shfl(d.in_model, fl), __shfl(bad, fl));
        }
        const unsigned long long m = __ballot(en && d.in_model);
        if (lane == c) my_mask = m;
        total += __popcll(m);
        last_chunk = c;
      }
      if (vkey != SIM_NO_VIOLATION) {
        if (lane == 0) atomicMin(&ctr->viol_key, vkey);
        stop = SIM_STOP_VIOLATION;
        break;
      }
      if (total == 0) {  // (not reachable from an in-model state of this spec: Restart is always enabled and stays in-model)
        stop = SIM_STOP_STUCK;
        my_stuck++;
        break;
      }
      int r = (int)sim_draw(rbase, (uint32_t)t, (uint32_t)total);
      int cc = 0;
      unsigned long long cm = 0;
      for (int c = 0; c <= last_chunk; c++) {
        cm = shfl_u64(my_mask, c);
        const int cnt = __popcll(cm);
        if (r < cnt) {
          cc = c;
          break;
        }
        r -= cnt;
      }
      const bool chosen = (cm >> lane & 1ull) && __popcll(cm & ((1ull << lane) - 1ull)) == r;
      const int sel = __builtin_ctzll(__ballot(chosen));
      if (cc != last_chunk && lane == sel) {  // its delta is gone: evaluate the instance again
        inst = candidate_inst(L, cc * 64 + lane, nmsg);
        compute_delta<NS>(L, a, inst, d);
      }
      for (int k = lane; k < W; k += 64) b[k] = a[k];
      wave_sync();
      FP cfp{0, 0};
      if (lane == sel) {
        cfp = fp_add(pfp, delta_fp<NS>(L, a, d, d.srv >= 0 ? &hsrv[d.srv] : nullptr));
        child_patches<NS>(L, a, d, pall, cfp, [&](int x, uint32_t v) { b[x] = v; });
        atomicAdd(&taken[cover_code(L, inst, d.sub)], 1u);
      }
      cfp.a = shfl_u64(cfp.a, sel);
      cfp.b = shfl_u64(cfp.b, sel);
      digest += sim_path_term(cfp, (uint32_t)t);
      wave_sync();
      uint32_t* sw = a;
      a = b;
      b = sw;
      len = t;
      my_steps++;
    }
    if (lane == 0) {
      const FP f = row_fp(a);
      ends[4ull * i] = f.a;
      ends[4ull * i + 1] = f.b;
      ends[4ull * i + 2] = digest;
      ends[4ull * i + 3] = sim_end_word((uint32_t)len, stop);
    }
    if (t1 < depth && stop == SIM_STOP_DEPTH) {  // still running: the next launch continues from this row
      uint32_t* dst = carry + (unsigned long long)i * W;
      for (int k = lane; k < W; k += 64) dst[k] = a[k];
    }
    wave_sync();
  }
  if (lane == 0) {
    if (my_steps) atomicAdd(&ctr->steps, my_steps);
    if (my_gen) atomicAdd(&ctr->generated, my_gen);
    if (my_stuck) atomicAdd(&ctr->stuck, my_stuck);
  }
  cover_flush(taken, COVER_CODES, ctr->taken);
}

namespace rtla {

size_t simulate_lds_bytes(const Layout& L, int wpb) { return (size_t)wpb * sim_wave_words(L.W) * sizeof(uint32_t); }

hipError_t launch_simulate(const Layout& L, const Ring& cur, uint64_t n_front, uint64_t seed, uint64_t first,
                           uint32_t n_walks, int t0, int t1, int depth, uint32_t* carry, uint64_t* ends,
                           SimCounters* ctr, hipStream_t st) {
  const int wpb = 4;
  // enough blocks to fill the device at the kernel's occupancy; the walks of a batch are strided over them
  const unsigned grid = (unsigned)std::min<uint64_t>(((uint64_t)n_walks + wpb - 1) / wpb, (uint64_t)device_cus() * 16);
  RTLA_DISPATCH_N(L, k_simulate, dim3(grid), dim3(64 * wpb), simulate_lds_bytes(L, wpb), st, L, cur,
                  (unsigned long long)n_front, (unsigned long long)seed, (unsigned long long)first, n_walks, t0, t1,
                  depth, carry, (unsigned long long*)ends, ctr);
  return hipGetLastError();
}

}  // namespace rtla
