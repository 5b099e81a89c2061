// rtla_kpred.hip -- user-defined predicates on the GPU: one compiled predicate
// set (rtla_pred.h's bytecode) evaluated on a batch of rows or on the frontier
// in HBM.  k_pred_state runs audit_row_stream (rtla_kaudit.h): a wave takes 64
// consecutive rows, stages them (in tiles of `tr` rows) into LDS with 16-byte
// loads, each lane interprets the program on its own row there, per-bit ballots
// go into wave-uniform counts, the block's LDS tally and the device counters
// once per block, and the least violation key is one atomicMin per wave.
//
// What is the interpreter's own:
//   * the program is copied once per block into LDS; every lane has its own
//     program counter (trip counts and short-circuits depend on the row);
//   * the operand file (PRED_FILE words per lane, indexed at run time) lives in
//     LDS at the odd per-lane stride PRED_STRIDE: word k of the 64 lanes falls
//     on different banks, and nothing goes to scratch;
//   * an evaluation error raises FLAG_SPEC_ERROR in ctr->flags: the call fails
//     whatever the other lanes found.
// LDS of a block of four waves: 32 B tally + 2 KB program + 4 tiles of at most
// PRED_TILE_BYTES + 4 * 64 operand files of 92 B = 64,544 B of the 64 KB.
//
// k_pred_step, below k_pred_state, runs an action set (two rows: a state and a
// successor materialised in LDS) on every step out of the rows.
#include "rtla_kaudit.h"
#include "rtla_step.h"

namespace {

constexpr int PRED_STRIDE = PRED_FILE + 1;  // words between two lanes' operand files: odd
constexpr int PRED_WPB = 4;
constexpr int PRED_TILE_BYTES = 9728;       // staging tile per wave
static_assert(PRED_STRIDE % 2 == 1, "conflict-free operand files need an odd stride");
static_assert((AUDIT_HEAD + PRED_MAX_WORDS + PRED_WPB * 64 * PRED_STRIDE) * 4 + PRED_WPB * PRED_TILE_BYTES <= 65536,
              "a block's LDS");
static_assert(4 * WMAX * 4 <= PRED_TILE_BYTES, "the widest row's smallest tile fits");
static_assert((AUDIT_HEAD + PRED_MAX_WORDS) % 4 == 0, "tiles start 16-byte aligned");

}  // namespace

// Rows [0, n) of `cur`; masks (may be null): the false-definition mask of each row.
template <int NS>
__global__ void __launch_bounds__(64 * PRED_WPB)
k_pred_state(Layout L, Ring cur, unsigned long long n, int tr, const uint32_t* __restrict__ prog, int nwords,
             int* __restrict__ masks, AuditCounters* ctr) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  const int W = L.W;
  uint32_t* const code = lds + AUDIT_HEAD;
  uint32_t* const tile = code + PRED_MAX_WORDS + wave * tr * W;
  int* const file = reinterpret_cast<int*>(code + PRED_MAX_WORDS + wpb * tr * W) + (wave * 64 + lane) * PRED_STRIDE;
  for (int k = threadIdx.x; k < nwords; k += blockDim.x) code[k] = prog[k];
  cover_zero(lds, AUDIT_HEAD);  // (its barrier also publishes the program)

  unsigned int cnt[PRED_MAX_DEFS] = {};
  unsigned long long evaluated = 0, vkey = AUDIT_NO_VIOLATION;
  audit_row_stream(cur, n, W, tr, tile, masks, cnt, evaluated, vkey, wave, wpb, lane, [&](const uint32_t* row) {
    int err = 0;
    const int bad = pred_eval<NS>(L, row, (const uint32_t*)code, file, &err);
    if (err) atomicOr(&ctr->flags, FLAG_SPEC_ERROR);
    return err ? 0 : bad;
  });
  audit_finish(lds, cnt, evaluated, vkey, ctr, lane);
}

// ---- action properties: an action set on every step out of rows [0, n) of `cur`.
//
// k_pred_step runs audit_succ_stream (rtla_kaudit.h): one wave per state, the parent in LDS (load_parent: with its
// new allLogs words and the fingerprint they give), each lane the Delta of one candidate instance, the enabled
// lanes ranked by ballot.  The interpreter reads rows, so the enabled children are materialised (parent + patches, as
// k_expand_batch's) into a per-wave LDS stage, `tc` at a time, and the lane whose child is in the stage runs
// pred_eval_rows on (parent row, child row), both in LDS; the child never leaves the CU.  Per wave: parent
// (even_words(W)) | allLogs' (32) | server hashes (4 * NMAX) | tc children at stride W | 1 (odd: the lanes' reads
// of word k of their own child fall on different banks) | tc operand files at PRED_STRIDE (indexed by the child's
// slot: a lane without a child in the stage needs none).
constexpr int STEP_WPB = 4;
__host__ __device__ constexpr int step_child_stride(int W) { return W | 1; }
__host__ __device__ constexpr int step_wave_words(int W, int tc) {
  return (even_words(W) + 32 + 4 * NMAX + tc * (step_child_stride(W) + PRED_STRIDE) + 3) & ~3;
}
// Children per tile: the most (at most 64) that four waves' LDS allows beside the tally and the program.
__host__ __device__ constexpr int step_tile_children(int W) {
  const int budget = (65536 / 4 - AUDIT_HEAD - PRED_MAX_WORDS) / STEP_WPB;
  const int tc = (budget - step_wave_words(W, 0)) / (step_child_stride(W) + PRED_STRIDE);
  return tc > 64 ? 64 : tc;
}
static_assert(step_tile_children(WMAX) >= 4, "the widest row's tile holds a few children");
static_assert((AUDIT_HEAD + PRED_MAX_WORDS + STEP_WPB * step_wave_words(WMAX, step_tile_children(WMAX))) * 4 <= 65536 &&
                  (AUDIT_HEAD + PRED_MAX_WORDS + STEP_WPB * step_wave_words(43, step_tile_children(43))) * 4 <= 65536,
              "a block's LDS");

// masks (may be null): the OR of the false-definition masks over each row's steps.
template <int NS>
__global__ void __launch_bounds__(64 * STEP_WPB)
k_pred_step(Layout L, Ring cur, unsigned long long n, int tc, const uint32_t* __restrict__ prog, int nwords,
            int* __restrict__ masks, AuditCounters* ctr) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  const int W = L.W, cs = step_child_stride(W);
  uint32_t* const code = lds + AUDIT_HEAD;
  uint32_t* const prow = code + PRED_MAX_WORDS + wave * step_wave_words(W, tc);
  uint32_t* const pall = prow + even_words(W);
  FP* const hsrv = reinterpret_cast<FP*>(pall + 32);
  uint32_t* const stage = pall + 32 + 4 * NMAX;
  int* const files = reinterpret_cast<int*>(stage + tc * cs);
  for (int k = threadIdx.x; k < nwords; k += blockDim.x) code[k] = prog[k];
  cover_zero(lds, AUDIT_HEAD);  // (its barrier also publishes the program)

  unsigned int cnt[PRED_MAX_DEFS] = {};
  unsigned long long evaluated = 0, vkey = AUDIT_NO_VIOLATION;
  FP pfp{0, 0};  // the parent's fingerprint with allLogs' applied
  audit_succ_stream<NS>(
      L, n, prow, masks, cnt, evaluated, vkey, ctr, wave, wpb, lane,
      [&](unsigned long long s) { pfp = load_parent<NS>(L, ring_row(cur, s, W), prow, pall, hsrv, lane); },
      [&](bool en, unsigned long long m, int, const DeltaT<NS>& d) {
        const int nen = __popcll(m);
        const int rank = __popcll(m & ((1ull << lane) - 1ull));
        const FP cfp = en ? fp_add(pfp, delta_fp<NS>(L, prow, d, d.srv >= 0 ? &hsrv[d.srv] : nullptr)) : FP{0, 0};
        int bad = 0;
        for (int b = 0; b < nen; b += tc) {
          if (en && rank >= b && rank < b + tc) {
            uint32_t* const child = stage + (rank - b) * cs;
            materialize<NS>(L, prow, d, pall, cfp, child);
            int err = 0;
            bad = pred_eval_rows<NS, true>(L, (const uint32_t*)prow, (const uint32_t*)child, (const uint32_t*)code,
                                           files + (rank - b) * PRED_STRIDE, &err);
            if (err) {
              atomicOr(&ctr->flags, FLAG_SPEC_ERROR);
              bad = 0;
            }
            if (step_stutters(prow, child)) bad = 0;  // (evaluated first, as [A]_vars: an error stays an error)
          }
          wave_sync();  // the next tile's lanes write the slots this tile's lanes read
        }
        return bad;
      });
  audit_finish(lds, cnt, evaluated, vkey, ctr, lane);
}

namespace rtla {

hipError_t launch_pred_step(const Layout& L, const Ring& cur, uint64_t n, const uint32_t* prog, int nwords,
                            int* masks, AuditCounters* ctr, hipStream_t st) {
  if (!n) return hipSuccess;
  if (nwords < 1 || nwords > PRED_MAX_WORDS) return hipErrorInvalidValue;
  const int tc = step_tile_children(L.W);
  const unsigned grid = (unsigned)std::min<uint64_t>((n + STEP_WPB - 1) / STEP_WPB, (uint64_t)device_cus() * 8);
  const size_t lds = (size_t)(AUDIT_HEAD + PRED_MAX_WORDS + STEP_WPB * step_wave_words(L.W, tc)) * sizeof(uint32_t);
  RTLA_DISPATCH_N(L, k_pred_step, dim3(grid), dim3(64 * STEP_WPB), lds, st, L, cur, (unsigned long long)n, tc, prog,
                  nwords, masks, ctr);
  return hipGetLastError();
}

hipError_t launch_pred(const Layout& L, const Ring& cur, uint64_t n, const uint32_t* prog, int nwords, int* masks,
                       AuditCounters* ctr, hipStream_t st) {
  if (!n) return hipSuccess;
  if (nwords < 1 || nwords > PRED_MAX_WORDS) return hipErrorInvalidValue;
  const int tr = audit_tile_rows(L.W, PRED_TILE_BYTES);
  const uint64_t ngroup = (n + 63) / 64;
  const unsigned grid = (unsigned)std::min<uint64_t>((ngroup + PRED_WPB - 1) / PRED_WPB, (uint64_t)device_cus() * 4);
  const size_t lds = (size_t)(AUDIT_HEAD + PRED_MAX_WORDS + PRED_WPB * tr * L.W + PRED_WPB * 64 * PRED_STRIDE) *
                     sizeof(uint32_t);
  RTLA_DISPATCH_N(L, k_pred_state, dim3(grid), dim3(64 * PRED_WPB), lds, st, L, cur, (unsigned long long)n, tr, prog,
                  nwords, masks, ctr);
  return hipGetLastError();
}

}  // namespace rtla
