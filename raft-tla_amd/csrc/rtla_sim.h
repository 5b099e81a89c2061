// rtla_sim.h -- random-walk simulation (TLC's -simulate): the definitions the
// kernel (rtla_ksim.hip) and the host replay (rtla_host.cpp) share, so both
// compute the same walks bit for bit.
//
// Walk w (a global 64-bit id) starts at row w mod n of the n start rows (the
// current BFS frontier; {Init} right after rtla_init).  Step t = 1..depth from
// state s:
//   * every action instance is evaluated in ascending instance number; each
//     enabled successor counts as generated and is invariant-checked on
//     parent + delta, as the BFS does for new and out-of-model successors;
//   * a successor with a spec / row-capacity error raises the level kernels'
//     flag (the call fails: a walk is never silently truncated);
//   * if any successor violates an invariant the walk ends: its violation is
//     (step t, least violating instance);
//   * otherwise, with M the in-model successors in instance order, the walk
//     ends "stuck" if M is empty, else it moves to M[draw(t, |M|)] -- draw is
//     counter-based, a function of (seed, w, t) only -- materialised with the
//     incremental fingerprint exactly as the level kernels do.
// End record of a walk: 4 u64 = last state's fingerprint a, b | path digest
// (sum mod 2^64 of sim_path_term over the states entered) | steps taken |
// stop code << 32.
//
// Walks that carry user properties (rtla_simulate_pred,
// rtla_sim_replay_pred, rtla_sim_walk_pred).  A simulation may carry a compiled
// state set P (rtla_pred_compile) and / or a compiled action set A
// (rtla_pred_compile_step), each of up to 8 definitions and bound to the row
// layout.  At step t from state s, for every enabled successor u in ascending
// instance number:
//   * the built-ins are checked as above (cfg.inv_mask, on parent + delta, in-
//     and out-of-model);
//   * A is evaluated on the step (s, u) for every enabled u, in- or
//     out-of-model, exactly as rtla_pred_step_* does: a definition is false iff
//     its expression is FALSE and u is not s (step_stutters); the program runs
//     on a stuttering step all the same, so an evaluation error there is still
//     an error;
//   * P is evaluated on u only when u is in-model: the states a BFS would store
//     and rtla_pred_frontier would audit (out-of-model successors stay the
//     built-ins' business);
//   * a successor's spec or row-capacity error, or an evaluation error of
//     either program, fails the call whatever else was found;
//   * if any u has a nonzero built-in mask, P mask or A mask the walk ends with
//     SIM_STOP_VIOLATION at (step t, least such instance); the three masks
//     reported are that instance's own, not an OR over the step;
//   * otherwise the pick is unchanged: M[draw(t, |M|)].
// So a set never changes which walk is taken: every state a walk enters before
// it ends is the plain walk's, with the same draws, fingerprints and digest
// terms.  The start row itself is not evaluated (it was not for the built-ins
// either).  These walks' end record has a fifth word: 0 unless the walk stopped
// on a violation, then sim_viol_word.  Their violation key orders by (walk,
// step, instance) alone (its low six bits are 0); the masks are read from that
// walk's fifth word, so nothing depends on scheduling.
#pragma once
#include "rtla_audit.h"
#include "rtla_step.h"
#include "rtla_synth.h"

namespace rtla {

enum { SIM_STOP_DEPTH = 0, SIM_STOP_STUCK = 1, SIM_STOP_VIOLATION = 2 };
constexpr int SIM_MAX_DEPTH = 65535;          // the step is a 16-bit field of the violation key
constexpr uint64_t SIM_BATCH = 1ull << 18;    // walks per batch: no further batch after one that found a violation
constexpr uint64_t SIM_LAUNCH_STEPS = 1ull << 23;  // walks x steps of one kernel launch, at most
constexpr uint64_t SIM_NO_VIOLATION = ~0ull;
constexpr int SIM_MAX_CAND = 512;             // candidates of one state, at most (fixed families + 3 per bag slot)

// The walk's generator: its t-th below() call picks step t.
RTLA_HD uint64_t sim_rng_base(uint64_t seed, uint64_t w) {
  return mix_b(seed * 0x9E3779B97F4A7C15ull ^ mix_a(w + 0x243f6a8885a308d3ull));
}
RTLA_HD uint32_t sim_draw(uint64_t base, uint32_t t, uint32_t n) {  // t >= 1
  SynthRng g{base, (uint64_t)t - 1};
  return g.below(n);
}

// Path digest term of the state entered at step t.
RTLA_HD uint64_t sim_path_term(FP f, uint32_t t) {
  return mix_a(f.a ^ mix_b(f.b + (uint64_t)t * 0x9E3779B97F4A7C15ull));
}

RTLA_HD uint64_t sim_end_word(uint32_t length, int stop) { return (uint64_t)length | (uint64_t)stop << 32; }

// Violation key, least first: walk (its index in the batch, < 2^18) << 38 |
// step << 22 | instance << 6 | in_model << 5 | violated-invariant mask.  The
// low six bits are a function of (walk, step, instance), so the order is theirs.
RTLA_HD uint64_t sim_viol_key(uint64_t rel_walk, uint32_t step, int inst, int in_model, int mask) {
  return rel_walk << 38 | (uint64_t)step << 22 | (uint64_t)inst << 6 | (uint64_t)(in_model ? 32 : 0) |
         (uint64_t)(mask & INV_ALL);
}
RTLA_HD uint64_t sim_key_walk(uint64_t key) { return key >> 38; }
RTLA_HD int sim_key_step(uint64_t key) { return (int)(key >> 22 & 0xffff); }
RTLA_HD int sim_key_inst(uint64_t key) { return (int)(key >> 6 & 0xffff); }
RTLA_HD int sim_key_in_model(uint64_t key) { return (int)(key >> 5 & 1); }
RTLA_HD int sim_key_mask(uint64_t key) { return (int)(key & INV_ALL); }

// Fifth end word of a walk with user properties that stopped on a violation.
RTLA_HD uint64_t sim_viol_word(int inst, int in_model, int inv_mask, int state_mask, int step_mask) {
  return (uint64_t)inst | (uint64_t)(in_model ? 1 : 0) << 16 | (uint64_t)(inv_mask & INV_ALL) << 24 |
         (uint64_t)(state_mask & 255) << 32 | (uint64_t)(step_mask & 255) << 40;
}
RTLA_HD int sim_word_inv_mask(uint64_t w) { return (int)(w >> 24 & 255); }
RTLA_HD int sim_word_state_mask(uint64_t w) { return (int)(w >> 32 & 255); }
RTLA_HD int sim_word_step_mask(uint64_t w) { return (int)(w >> 40 & 255); }
RTLA_HD int sim_word_in_model(uint64_t w) { return (int)(w >> 16 & 1); }
static_assert(INV_ALL <= 255 && PRED_MAX_DEFS <= 8, "each mask has eight bits of the word");

// Device counters of one rtla_simulate batch.
struct SimCounters {
  unsigned long long steps, generated, stuck;
  unsigned long long viol_key;  // SIM_NO_VIOLATION, or the least sim_viol_key (atomicMin)
  int flags, pad;
  unsigned long long taken[COVER_CODES];
  unsigned long long state_evaluated, step_evaluated;  // walks with user properties: evaluations of P / of A
};

// Host tally of the same quantities.
struct SimTally {
  uint64_t steps = 0, generated = 0, stuck = 0;
  uint64_t viol_key = SIM_NO_VIOLATION;
  int flags = 0;
  uint64_t taken[COVER_CODES] = {};
  uint64_t state_evaluated = 0, step_evaluated = 0;
  uint64_t viol_word = 0;  // walks with user properties: the fifth end word of viol_key's walk
};

struct SimEnd {
  FP last;
  uint64_t digest;
  uint32_t length;
  int stop;
  // stop == SIM_STOP_VIOLATION: the violation, at step length + 1
  int viol_inst, viol_sub, viol_mask, viol_in_model;
  int viol_state_mask, viol_step_mask;  // walks with user properties
};

// One walk on the host, serially.  buf: 3 * L.W words.  on_state(t, row,
// label, violating) is called for every state entered (label = sub << 16 |
// instance) and, on a violation, for the violating successor.  rel_walk: the
// walk's index in its batch (violation key).  sprog / aprog: the programs of P
// and A, or null; with either, every enabled successor is materialised once
// and both programs run on it.
template <int NS, class F>
static inline SimEnd sim_walk_serial(const Layout& L, const uint32_t* start, uint64_t seed, uint64_t w,
                                     uint64_t rel_walk, int depth, uint32_t* buf, SimTally& tl, F on_state,
                                     const uint32_t* sprog = nullptr, const uint32_t* aprog = nullptr) {
  constexpr int NR = NS ? NS : NMAX;
  const int W = L.W;
  const bool pred = sprog || aprog;
  uint32_t* cur = buf;
  uint32_t* nxt = buf + W;
  uint32_t* const stage = buf + 2 * W;
  int file[PRED_FILE];
  uint32_t pall[33];
  uint16_t model[SIM_MAX_CAND];
  for (int k = 0; k < W; k++) cur[k] = start[k];
  const uint64_t base = sim_rng_base(seed, w);
  SimEnd e{};
  e.stop = SIM_STOP_DEPTH;
  e.viol_inst = -1;
  for (int t = 1; t <= depth; t++) {
    const FP pfp = fp_add(row_fp(cur), alllogs_delta<NS>(L, cur, pall));
    uint32_t total = 0;  // |M|; model[]: its instances, ascending
    bool violated = false;
    for_each_successor<NS>(L, cur, tl.flags, [&](int inst, const auto& d) {
      tl.generated++;
      const int bad = check_invariants_v<NS>(L, cur, d.srv, d.rec[0], d.rec[1], d.elec, d.erec[0]);
      int sbad = 0, abad = 0;
      if (pred) {
        materialize<NS>(L, cur, d, pall, fp_add(pfp, delta_fp<NS>(L, cur, d)), stage);
        if (aprog) {
          int err = 0;
          abad = pred_eval_rows<NS, true>(L, (const uint32_t*)cur, (const uint32_t*)stage, aprog, file, &err);
          tl.step_evaluated++;
          if (err) {
            tl.flags |= FLAG_SPEC_ERROR;
            abad = 0;
          }
          if (step_stutters(cur, stage)) abad = 0;  // (evaluated first, as [A]_vars: an error stays an error)
        }
        if (sprog && d.in_model) {
          int err = 0;
          sbad = pred_eval<NS>(L, (const uint32_t*)stage, sprog, file, &err);
          tl.state_evaluated++;
          if (err) {
            tl.flags |= FLAG_SPEC_ERROR;
            sbad = 0;
          }
        }
      }
      if ((bad | sbad | abad) && !violated) {
        violated = true;
        e.viol_inst = inst; e.viol_sub = d.sub; e.viol_mask = bad; e.viol_in_model = d.in_model;
        e.viol_state_mask = sbad; e.viol_step_mask = abad;
        const FP cfp = fp_add(pfp, delta_fp<NS>(L, cur, d));
        materialize<NS>(L, cur, d, pall, cfp, nxt);
      }
      if (d.in_model) model[total++] = (uint16_t)inst;
    });
    if (violated) {
      e.stop = SIM_STOP_VIOLATION;
      const uint64_t key = pred ? sim_viol_key(rel_walk, (uint32_t)t, e.viol_inst, 0, 0)
                                : sim_viol_key(rel_walk, (uint32_t)t, e.viol_inst, e.viol_in_model, e.viol_mask);
      if (key < tl.viol_key) {
        tl.viol_key = key;
        tl.viol_word = sim_viol_word(e.viol_inst, e.viol_in_model, e.viol_mask, e.viol_state_mask, e.viol_step_mask);
      }
      on_state(t, (const uint32_t*)nxt, (int32_t)(e.viol_sub << 16 | e.viol_inst), true);
      break;
    }
    if (!total) {  // (not reachable from an in-model state of this spec: Restart is always enabled and stays in-model)
      e.stop = SIM_STOP_STUCK;
      tl.stuck++;
      break;
    }
    {
      const int inst = model[sim_draw(base, (uint32_t)t, total)];
      DeltaT<NR> d;
      compute_delta<NS>(L, cur, inst, d);
      const FP cfp = fp_add(pfp, delta_fp<NS>(L, cur, d));
      materialize<NS>(L, cur, d, pall, cfp, nxt);
      e.digest += sim_path_term(cfp, (uint32_t)t);
      tl.taken[cover_code(L, inst, d.sub)]++;
      tl.steps++;
      e.length = (uint32_t)t;
      on_state(t, (const uint32_t*)nxt, (int32_t)(d.sub << 16 | inst), false);
    }
    uint32_t* sw = cur; cur = nxt; nxt = sw;
  }
  e.last = row_fp(cur);
  return e;
}

}  // namespace rtla
