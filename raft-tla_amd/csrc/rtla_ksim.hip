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
//
// k_simulate<NS, true> (k_simulate_pred) is the same walk carrying user
// properties (rtla_sim.h).  The interpreter reads rows, so inside
// the chunk loop the enabled lanes, ranked by ballot, materialise their child
// (parent + patches) into a per-wave LDS stage, `tc` at a time, as k_pred_step
// does, and the lane whose child is in the stage runs the action program on
// (current row, child) and, if the child is in-model, the state program on the
// child; the child never leaves the CU.  Per wave, after the plain kernel's
// words: tc children at the odd stride W | 1, then tc operand files at
// PRED_STRIDE; both programs are copied once per block into LDS.  Everything
// this adds is under `if constexpr (PRED)`, and the last kernel argument of
// k_simulate<NS, false> is an empty struct: the plain kernel is the code it was.
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

// ---- walks with user properties
constexpr int PRED_STRIDE = PRED_FILE + 1;  // words between two operand files: odd (rtla_kpred.hip)
constexpr int SIM_WPB = 4;
static_assert(PRED_STRIDE % 2 == 1, "conflict-free operand files need an odd stride");
// Waves per SIMD of k_simulate_pred's register budget: the interpreter's state is live across the walk's, so it
// has a budget of its own.  On the configs[1] shape 2 / 3 waves per SIMD (256 / 168 VGPRs, 28 / 333 spilled) ran
// 2^21 walks x 32 steps with LeaderAppendOnly in 1,275 / 1,800 ms (profiles/r11_simpred).
#ifndef SIM_PRED_WAVES
#define SIM_PRED_WAVES 2
#endif
constexpr int sim_pred_waves(int) { return SIM_PRED_WAVES; }
__host__ __device__ constexpr int sim_child_stride(int W) { return W | 1; }
__host__ __device__ constexpr int sim_pred_wave_words(int W, int tc) {
  return (sim_wave_words(W) + tc * (sim_child_stride(W) + PRED_STRIDE) + 3) & ~3;
}
// A block's LDS: the coverage tally, both programs, four waves.
__host__ __device__ constexpr int sim_pred_block_bytes(int W, int tc) {
  return (COVER_CODES + 2 * PRED_MAX_WORDS + SIM_WPB * sim_pred_wave_words(W, tc)) * 4;
}
// Children per tile: the most (at most 64) a block's LDS allows -- 64 KB, and no more than a CU's 160 KB divided by
// the blocks of four waves its register budget lets it hold (one per wave per SIMD), so LDS never lowers them.
__host__ __device__ constexpr int sim_tile_children(int W) {
  const int per_cu = 160 * 1024 / SIM_PRED_WAVES;
  const int budget = (per_cu < 65536 ? per_cu : 65536) / 4 - COVER_CODES - 2 * PRED_MAX_WORDS;
  const int tc = (budget / SIM_WPB - sim_pred_wave_words(W, 0) - 3) / (sim_child_stride(W) + PRED_STRIDE);
  return tc > 64 ? 64 : tc;
}
static_assert(sim_tile_children(WMAX) >= 4 && sim_tile_children(43) >= 4, "the widest row's tile holds a few children");
static_assert(sim_pred_block_bytes(WMAX, sim_tile_children(WMAX)) <= 65536 &&
                  sim_pred_block_bytes(43, sim_tile_children(43)) <= 65536 &&
                  sim_pred_block_bytes(WMAX, sim_tile_children(WMAX)) * SIM_PRED_WAVES <= 160 * 1024 &&
                  sim_pred_block_bytes(43, sim_tile_children(43)) * SIM_PRED_WAVES <= 160 * 1024,
              "a block's LDS, and every block the registers allow on a CU");

// What k_simulate_pred has beside k_simulate's arguments.
struct SimNoArgs {};
struct SimPredArgs {
  const uint32_t* prog;  // the state program, and at PRED_MAX_WORDS the action program
  int n_state, n_step;   // their words (0: no such set)
  int tc;                // children per tile
};

}  // namespace

// Walks [0, n_walks) of the batch whose first global walk id is `first`, steps
// t0 + 1 .. t1 of `depth`.  t0 == 0: the walk starts at frontier row
// (first + i) mod n_front; otherwise at carry[i] if ends[4 i + 3] says the walk
// is still running (t0 steps taken, stop code 0).
//
// PRED (k_simulate_pred below): the walks carry user properties (pa: SimPredArgs, else an empty SimNoArgs); the end
// records have 5 words, and word 4 of a walk that ended in an earlier launch is left alone (as its other words).
template <int NS, bool PRED = false>
__global__ void __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(PRED ? sim_pred_waves(NS) : sim_waves(NS))))
k_simulate(Layout L, Ring cur, unsigned long long n_front, unsigned long long seed, unsigned long long first,
           unsigned int n_walks, int t0, int t1, int depth, uint32_t* __restrict__ carry,
           unsigned long long* __restrict__ ends, SimCounters* ctr,
           std::conditional_t<PRED, SimPredArgs, SimNoArgs> pa) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  __shared__ unsigned int taken[COVER_CODES];
  constexpr unsigned long long EW = PRED ? 5 : 4;  // words of an end record
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  const int W = L.W;
  uint32_t* const code = lds;  // PRED: both programs, before the waves' words
  uint32_t* wbase = lds + wave * sim_wave_words(W);
  if constexpr (PRED) wbase = lds + 2 * PRED_MAX_WORDS + wave * sim_pred_wave_words(W, pa.tc);
  uint32_t* const pall = wbase + 2 * even_words(W);
  FP* const hsrv = reinterpret_cast<FP*>(pall + 32);
  [[maybe_unused]] uint32_t* const stage = wbase + sim_wave_words(W);  // PRED: the children, then their operand files
  if constexpr (PRED) {
    for (int k = threadIdx.x; k < pa.n_state; k += blockDim.x) code[k] = pa.prog[k];
    for (int k = threadIdx.x; k < pa.n_step; k += blockDim.x) code[PRED_MAX_WORDS + k] = pa.prog[PRED_MAX_WORDS + k];
  }
  cover_zero(taken, COVER_CODES);  // (its barrier also publishes the programs)

  unsigned long long my_steps = 0, my_gen = 0, my_stuck = 0;  // wave-uniform
  unsigned long long my_state_eval = 0, my_step_eval = 0;     // PRED, wave-uniform
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
      const unsigned long long e = ends[EW * i + 3];
      if ((e >> 32) != SIM_STOP_DEPTH || (uint32_t)e != (uint32_t)t0) continue;  // ended in an earlier launch
      digest = ends[EW * i + 2];
      src = carry + (unsigned long long)i * W;
    }
    for (int k = lane; k < W; k += 64) a[k] = src[k];
    wave_sync();
    const uint64_t rbase = sim_rng_base(seed, w);
    int len = t0, stop = SIM_STOP_DEPTH;
    [[maybe_unused]] unsigned long long last_vword = 0;  // PRED: word 4 of a walk that stops on a violation
    for (int t = t0 + 1; t <= t1; t++) {
      // per-parent data: server-record hashes, allLogs' (raft.tla:465) and its fingerprint change
      const FP pfp = parent_setup<NS>(L, a, pall, hsrv, lane);
      const int nmsg = row_nmsg(L, a);
      const int ncand = min(fixed + 3 * nmsg, SIM_MAX_CAND);  // (the host refuses layouts with more)
      unsigned long long my_mask = 0;  // lane c: ballot of chunk c's in-model successors
      int total = 0, last_chunk = 0;
      unsigned long long vkey = SIM_NO_VIOLATION, vword = 0;
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
        int sbad = 0, abad = 0;
        if constexpr (PRED) {
          const unsigned long long em = __ballot(en);
          if (em) {  // the enabled lanes' children through the stage, tc at a time
            const int tc = pa.tc, cs = sim_child_stride(W);
            int* const files = reinterpret_cast<int*>(stage + tc * cs);
            const int nen = __popcll(em);
            const int rank = __popcll(em & ((1ull << lane) - 1ull));
            const FP cfp = en ? fp_add(pfp, delta_fp<NS>(L, a, d, d.srv >= 0 ? &hsrv[d.srv] : nullptr)) : FP{0, 0};
            for (int b0 = 0; b0 < nen; b0 += tc) {
              if (en && rank >= b0 && rank < b0 + tc) {
                uint32_t* const child = stage + (rank - b0) * cs;
                int* const file = files + (rank - b0) * PRED_STRIDE;
                materialize<NS>(L, a, d, pall, cfp, child);
                if (pa.n_step) {
                  int err = 0;
                  abad = pred_eval_rows<NS, true>(L, (const uint32_t*)a, (const uint32_t*)child,
                                                  (const uint32_t*)(code + PRED_MAX_WORDS), file, &err);
                  if (err) {
                    atomicOr(&ctr->flags, FLAG_SPEC_ERROR);
                    abad = 0;
                  }
                  if (step_stutters(a, child)) abad = 0;  // (evaluated first, as [A]_vars: an error stays an error)
                }
                if (pa.n_state && d.in_model) {
                  int err = 0;
                  sbad = pred_eval<NS>(L, (const uint32_t*)child, (const uint32_t*)code, file, &err);
                  if (err) {
                    atomicOr(&ctr->flags, FLAG_SPEC_ERROR);
                    sbad = 0;
                  }
                }
              }
              wave_sync();  // the next tile's lanes write the slots this tile's lanes read
            }
            if (pa.n_step) my_step_eval += nen;
            if (pa.n_state) my_state_eval += __popcll(__ballot(en && d.in_model));
          }
        }
        const unsigned long long mb = __ballot((bad | sbad | abad) != 0);
        if (mb && vkey == SIM_NO_VIOLATION) {  // the least violating instance: instances ascend with q
          const int fl = __builtin_ctzll(mb);
          if constexpr (PRED) {  // the key orders by (walk, step, instance); the masks go into the walk's word 4
            const int vi = __shfl(inst, fl);
            vkey = sim_viol_key(i, (uint32_t)t, vi, 0, 0);
            vword = sim_viol_word(vi, __shfl((int)d.in_model, fl), __shfl(bad, fl), __shfl(sbad, fl), __shfl(abad, fl));
          } else {
            vkey = sim_viol_key(i, (uint32_t)t, __shfl(inst, fl), __shfl(d.in_model, fl), __shfl(bad, fl));
          }
        }
        const unsigned long long m = __ballot(en && d.in_model);
        if (lane == c) my_mask = m;
        total += __popcll(m);
        last_chunk = c;
      }
      if (vkey != SIM_NO_VIOLATION) {
        if (lane == 0) atomicMin(&ctr->viol_key, vkey);
        stop = SIM_STOP_VIOLATION;
        if constexpr (PRED) last_vword = vword;
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
      ends[EW * i] = f.a;
      ends[EW * i + 1] = f.b;
      ends[EW * i + 2] = digest;
      ends[EW * i + 3] = sim_end_word((uint32_t)len, stop);
      if constexpr (PRED) ends[EW * i + 4] = stop == SIM_STOP_VIOLATION ? last_vword : 0;
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
    if constexpr (PRED) {
      if (my_state_eval) atomicAdd(&ctr->state_evaluated, my_state_eval);
      if (my_step_eval) atomicAdd(&ctr->step_evaluated, my_step_eval);
    }
  }
  cover_flush(taken, COVER_CODES, ctr->taken);
}

template <int NS>
constexpr auto k_simulate_pred = k_simulate<NS, true>;

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
                  depth, carry, (unsigned long long*)ends, ctr, SimNoArgs{});
  return hipGetLastError();
}

hipError_t launch_simulate_pred(const Layout& L, const Ring& cur, uint64_t n_front, uint64_t seed, uint64_t first,
                                uint32_t n_walks, int t0, int t1, int depth, uint32_t* carry, uint64_t* ends,
                                SimCounters* ctr, const uint32_t* prog, int n_state, int n_step, hipStream_t st) {
  if (n_state < 0 || n_step < 0 || n_state > PRED_MAX_WORDS || n_step > PRED_MAX_WORDS || !(n_state || n_step))
    return hipErrorInvalidValue;
  const SimPredArgs pa{prog, n_state, n_step, sim_tile_children(L.W)};
  if (pa.tc < 1) return hipErrorInvalidValue;
  const unsigned grid = (unsigned)std::min<uint64_t>(((uint64_t)n_walks + SIM_WPB - 1) / SIM_WPB,
                                                     (uint64_t)device_cus() * 4 * SIM_PRED_WAVES);
  const size_t lds = (size_t)(2 * PRED_MAX_WORDS + SIM_WPB * sim_pred_wave_words(L.W, pa.tc)) * sizeof(uint32_t);
  RTLA_DISPATCH_N(L, k_simulate_pred, dim3(grid), dim3(64 * SIM_WPB), lds, st, L, cur, (unsigned long long)n_front,
                  (unsigned long long)seed, (unsigned long long)first, n_walks, t0, t1, depth, carry,
                  (unsigned long long*)ends, ctr, pa);
  return hipGetLastError();
}

}  // namespace rtla
