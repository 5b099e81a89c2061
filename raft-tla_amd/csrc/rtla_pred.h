// rtla_pred.h -- user-defined state predicates: the instruction set the
// predicate compiler (rtla_pred.cpp) emits and the ONE interpreter that runs it,
// on the host (rtla_pred_replay) and per lane on the GPU (rtla_kpred.hip).
// Grammar, typing and the termination bound: DESIGN.md section 13.
//
// A program is a sequence of u32 instructions: op (bits 0-7) | a (bits 8-15) |
// imm (bits 16-31; a jump target, or PUSHI's signed literal).  It evaluates
// every definition of a set in turn on one packed row and ends in P_HALT.  The
// machine is a stack machine over int32: Booleans are 0 / 1, servers 0..N-1
// (Nil = 7, the wide format's), states and message types their enum values, a
// log entry its 5-bit wide code (term | value << 3), a message its bag slot, an
// election its record index.  Its operand file has PRED_FILE words: the bound
// variables (PRED_VARS), then the stack (PRED_STACK; a quantifier keeps its
// upper limit there while its body runs).  Every jump is forward except
// QNEXT's, whose trip count the quantifier's domain bounds; the compiler has
// checked variable numbers, the stack depth and the step bound, and the
// interpreter counts its steps all the same (PRED_MAX_STEPS).
//
// An action set (rtla_pred_compile_step) is the same bytecode over two rows, see
// pred_eval_rows below.
//
// Evaluation errors (TLC's, never FALSE): a server index outside Server
// (votedFor's Nil), log[i][n] with n outside 1..Len(log[i]), a per-type
// message field read on a message of another type.
#pragma once
#include "rtla_model.h"

namespace rtla {

constexpr int PRED_MAX_DEFS = 8;              // rtla_audit_stats.counts
constexpr int PRED_VARS = 6;                  // variables bound at once
constexpr int PRED_STACK = 16;                // operand depth
constexpr int PRED_FILE = PRED_VARS + PRED_STACK;
constexpr int PRED_MAX_WORDS = 512;           // program words
constexpr uint32_t PRED_MAX_STEPS = 1u << 20; // worst-case instructions per row, all definitions
constexpr int PRED_RANGE_MAX = 15;            // integer ranges are intersected with 0..15

enum PredOp {
  P_HALT = 0,
  P_PUSHI,    // push imm (signed)
  P_LOADV,    // push var[a]
  P_ADD, P_SUB, P_EQ, P_NE, P_LT, P_LE, P_GT, P_GE, P_MIN, P_MAX,  // pop y, pop x, push x op y
  P_NOT,      // top = !top
  P_JMP,      // pc = imm
  P_JZ,       // pop; if 0: pc = imm
  P_JFK,      // top == 0: pc = imm (kept); else pop
  P_JTK,      // top != 0: pc = imm (kept); else pop
  P_DOM,      // push 0, push |domain a| - 1 (a: PD_SERVER / PD_MESSAGES / PD_ELECTIONS)
  P_CLAMP,    // (lo, hi) on the stack: lo = max(lo, 0), hi = min(hi, PRED_RANGE_MAX)
  P_QINIT_A,  // pop hi, pop lo; lo > hi: push 1 (\A over {}), pc = imm; else var[a] = lo, push hi
  P_QINIT_E,  // the same, pushing 0 (\E over {})
  P_QNEXT_A,  // pop r (hi below): !r or var[a] == hi: hi := r, go on; else var[a]++, pc = imm (the body)
  P_QNEXT_E,  // the same, deciding on r
  P_SRV,      // pop i; push field a of server i (PS_*)
  P_VIN,      // pop i, pop j; push j \in votesResponded[i] (a = 0) / votesGranted[i] (a = 1)
  P_LOGLEN,   // pop i; push Len(log[i])
  P_LOGENT,   // pop n, pop i; push log[i][n]                      (error: n outside 1..Len)
  P_ENT,      // pop entry; push its term (a = 0) / value (a = 1)
  P_NM,       // pop j, pop i; push nextIndex[i][j] (a = 0) / matchIndex[i][j] (a = 1)
  P_BAGCARD,  // push BagCardinality(messages)
  P_NELEC,    // push Cardinality(elections)
  P_MSG,      // pop m; push field a of the message in bag slot m (PM_*)  (error: field of another type)
  P_ELEC,     // pop e; push eterm (a = 0) / eleader (a = 1) of election record e
  P_DEFEND,   // pop r; !r: definition a is false on this row
  P_OPCOUNT
};
enum { PD_SERVER = 0, PD_MESSAGES, PD_ELECTIONS };
enum { PS_TERM = 0, PS_STATE, PS_VOTED, PS_COMMIT, PS_NRESPONDED, PS_NGRANTED };
enum {
  PM_COUNT = 0, PM_TYPE, PM_TERM, PM_SOURCE, PM_DEST,
  PM_LASTLOGTERM, PM_LASTLOGINDEX,                             // RequestVoteRequest
  PM_VOTEGRANTED,                                              // RequestVoteResponse
  PM_PREVLOGINDEX, PM_PREVLOGTERM, PM_COMMITINDEX, PM_NENTRIES,  // AppendEntriesRequest
  PM_SUCCESS, PM_MATCHINDEX,                                   // AppendEntriesResponse
  PM_FIELDS
};

RTLA_HD uint32_t pred_ins(int op, int a, int imm) {
  return (uint32_t)op | (uint32_t)(a & 255) << 8 | (uint32_t)(imm & 0xffff) << 16;
}
RTLA_HD int pred_op(uint32_t w) { return (int)(w & 255u); }
RTLA_HD int pred_a(uint32_t w) { return (int)(w >> 8 & 255u); }
RTLA_HD int pred_target(uint32_t w) { return (int)(w >> 16); }
RTLA_HD int pred_imm(uint32_t w) { return (int)(int16_t)(w >> 16); }

// The message type whose payload holds field f (-1: a header field, on every message).
RTLA_HD int pred_field_type(int f) {
  return f < PM_LASTLOGTERM ? -1 : f < PM_VOTEGRANTED ? RVREQ : f < PM_PREVLOGINDEX ? RVRESP : f < PM_SUCCESS ? AEREQ : AERESP;
}

// An action program reads two rows, a step's state and
// its successor: the instructions that read a row (P_DOM, P_SRV, P_VIN,
// P_LOGLEN, P_LOGENT, P_NM, P_BAGCARD, P_NELEC, P_MSG, P_ELEC) read the primed
// row when PRED_PRIME is set in their `a` field.  A state program never sets it.
constexpr int PRED_PRIME = 128;

// Runs `prog` on one row (STEP: on the step row -> row2).  file: PRED_FILE int32
// words of this evaluation's own (file[k] an lvalue).  Returns the mask of the
// definitions that are FALSE on the row (bit k = definition k); *err = 1 on an
// evaluation error (the mask then means nothing).  Without STEP row2 is never
// read and the code is the one-row interpreter's.
template <int NS, bool STEP, class P, class Q, class F>
RTLA_HD int pred_eval_rows(const Layout& L, P row1, P row2, Q prog, F file, int* err) {
  const int N = NS ? NS : L.N;
  int nmsg1 = row_nmsg(L, row1), nelec1 = row_nelec(L, row1);
  if (nmsg1 > L.K) nmsg1 = L.K;  // (a valid row's are within; no read past the row either way)
  if (nelec1 > L.E) nelec1 = L.E;
  int nmsg2 = 0, nelec2 = 0;
  if (STEP) {
    nmsg2 = row_nmsg(L, row2);
    nelec2 = row_nelec(L, row2);
    if (nmsg2 > L.K) nmsg2 = L.K;
    if (nelec2 > L.E) nelec2 = L.E;
  }
  int mask = 0, bad = 0, pc = 0, sp = PRED_VARS;  // sp: the next free word of the file
  for (uint32_t steps = 0;; steps++) {
    if (steps > PRED_MAX_STEPS) { bad = 1; break; }
    const uint32_t w = prog[pc++];
    const int op = pred_op(w);
    const bool primed = STEP && (pred_a(w) & PRED_PRIME);
    const int a = STEP ? pred_a(w) & (PRED_PRIME - 1) : pred_a(w);
    const P row = primed ? row2 : row1;
    const int nmsg = primed ? nmsg2 : nmsg1, nelec = primed ? nelec2 : nelec1;
    if (op == P_HALT) break;
    switch (op) {
      case P_PUSHI: file[sp++] = pred_imm(w); break;
      case P_LOADV: file[sp++] = file[a]; break;
      case P_ADD: case P_SUB: case P_EQ: case P_NE: case P_LT: case P_LE: case P_GT: case P_GE: case P_MIN:
      case P_MAX: {
        const int y = file[--sp], x = file[sp - 1];
        int r;
        switch (op) {
          case P_ADD: r = x + y; break;
          case P_SUB: r = x - y; break;
          case P_EQ: r = x == y; break;
          case P_NE: r = x != y; break;
          case P_LT: r = x < y; break;
          case P_LE: r = x <= y; break;
          case P_GT: r = x > y; break;
          case P_GE: r = x >= y; break;
          case P_MIN: r = x < y ? x : y; break;
          default: r = x > y ? x : y; break;
        }
        file[sp - 1] = r;
        break;
      }
      case P_NOT: file[sp - 1] = !file[sp - 1]; break;
      case P_JMP: pc = pred_target(w); break;
      case P_JZ: if (!file[--sp]) pc = pred_target(w); break;
      case P_JFK: if (!file[sp - 1]) pc = pred_target(w); else sp--; break;
      case P_JTK: if (file[sp - 1]) pc = pred_target(w); else sp--; break;
      case P_DOM:
        file[sp++] = 0;
        file[sp++] = (a == PD_SERVER ? N : a == PD_MESSAGES ? nmsg : nelec) - 1;
        break;
      case P_CLAMP:
        if (file[sp - 2] < 0) file[sp - 2] = 0;
        if (file[sp - 1] > PRED_RANGE_MAX) file[sp - 1] = PRED_RANGE_MAX;
        break;
      case P_QINIT_A: case P_QINIT_E: {
        const int hi = file[--sp], lo = file[--sp];
        if (lo > hi) {
          file[sp++] = op == P_QINIT_A;
          pc = pred_target(w);
        } else {
          file[a] = lo;
          file[sp++] = hi;
        }
        break;
      }
      case P_QNEXT_A: case P_QNEXT_E: {
        const int r = file[--sp];
        const bool decided = op == P_QNEXT_A ? !r : r != 0;
        if (decided || file[a] >= file[sp - 1]) {
          file[sp - 1] = r;
        } else {
          file[a] = file[a] + 1;
          pc = pred_target(w);
        }
        break;
      }
      case P_SRV: {
        const int i = file[sp - 1];
        if ((unsigned)i >= (unsigned)N) { bad = 1; break; }
        const uint32_t w0 = srv_w0(L, row, i);
        file[sp - 1] = a == PS_TERM ? (int)s_term(w0) : a == PS_STATE ? (int)s_role(w0) : a == PS_VOTED ? (int)s_voted(w0)
                     : a == PS_COMMIT ? (int)s_commit(w0) : a == PS_NRESPONDED ? __builtin_popcount(s_vresp(w0))
                     : __builtin_popcount(s_vgrant(w0));
        break;
      }
      case P_VIN: {
        const int i = file[--sp], j = file[sp - 1];
        if ((unsigned)i >= (unsigned)N) { bad = 1; break; }
        const uint32_t w0 = srv_w0(L, row, i);
        const uint32_t set = a ? s_vgrant(w0) : s_vresp(w0);
        file[sp - 1] = (unsigned)j < (unsigned)N ? (int)(set >> j & 1u) : 0;  // (Nil is in no set of servers)
        break;
      }
      case P_LOGLEN: {
        const int i = file[sp - 1];
        if ((unsigned)i >= (unsigned)N) { bad = 1; break; }
        file[sp - 1] = (int)log_len(srv_log(L, row, i));
        break;
      }
      case P_LOGENT: {
        const int n = file[--sp], i = file[sp - 1];
        if ((unsigned)i >= (unsigned)N) { bad = 1; break; }
        const uint32_t lg = srv_log(L, row, i);
        if (n < 1 || n > (int)log_len(lg)) { bad = 1; break; }
        file[sp - 1] = (int)log_entry(lg, (uint32_t)n);
        break;
      }
      case P_ENT: file[sp - 1] = a ? file[sp - 1] >> 3 : file[sp - 1] & 7; break;
      case P_NM: {
        const int j = file[--sp], i = file[sp - 1];
        if ((unsigned)i >= (unsigned)N || (unsigned)j >= (unsigned)N) { bad = 1; break; }
        const uint32_t nm = srv_nm(L, row, i);
        file[sp - 1] = (int)(a ? nm_match(nm, j) : nm_next(nm, j));
        break;
      }
      case P_BAGCARD: {
        int tot = 0;
        for (int k = 0; k < nmsg; k++) tot += (int)raw_count(L, slot_raw(L, row, k));
        file[sp++] = tot;
        break;
      }
      case P_NELEC: file[sp++] = nelec; break;
      case P_MSG: {
        const int m = file[sp - 1];
        if ((unsigned)m >= (unsigned)nmsg) { bad = 1; break; }
        const uint64_t v = msg_unpack(L, slot_raw(L, row, m));
        const int ft = pred_field_type(a);
        if (ft >= 0 && ft != (int)m_type(v)) { bad = 1; break; }
        int r;
        switch (a) {
          case PM_COUNT: r = (int)m_count(v); break;
          case PM_TYPE: r = (int)m_type(v); break;
          case PM_TERM: r = (int)m_term(v); break;
          case PM_SOURCE: r = (int)m_src(v); break;
          case PM_DEST: r = (int)m_dst(v); break;
          case PM_LASTLOGTERM: r = (int)m_f(v, 12, 4); break;
          case PM_LASTLOGINDEX: r = (int)m_f(v, 16, 3); break;
          case PM_VOTEGRANTED: r = (int)m_f(v, 12, 1); break;
          case PM_PREVLOGINDEX: r = (int)m_f(v, 12, 3); break;
          case PM_PREVLOGTERM: r = (int)m_f(v, 15, 4); break;
          case PM_COMMITINDEX: r = (int)m_f(v, 25, 3); break;
          case PM_NENTRIES: r = (int)m_f(v, 19, 1); break;
          case PM_SUCCESS: r = (int)m_f(v, 12, 1); break;
          default: r = (int)m_f(v, 13, 3); break;
        }
        file[sp - 1] = r;
        break;
      }
      case P_ELEC: {
        const int e = file[sp - 1];
        if ((unsigned)e >= (unsigned)nelec) { bad = 1; break; }
        const uint32_t e0 = elec_w0(L, row, e);
        file[sp - 1] = a ? (int)(e0 >> 4 & 7u) : (int)(e0 & 15u);
        break;
      }
      case P_DEFEND: if (!file[--sp]) mask |= 1 << a; break;
      default: bad = 1; break;
    }
    if (bad) break;
  }
  *err = bad;
  return mask;
}
template <int NS, class P, class Q, class F>
RTLA_HD int pred_eval(const Layout& L, P row, Q prog, F file, int* err) {
  return pred_eval_rows<NS, false>(L, row, row, prog, file, err);
}

}  // namespace rtla
