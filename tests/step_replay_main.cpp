// step_replay_main.cpp -- action properties as a stand-alone host program, for a
// sanitizer build (tests/test_step_host.py): the step compiler
// (raft-tla_amd/csrc/rtla_pred.cpp, pred_compile_step) on every text of a corpus
// file (texts separated by '\x1e'), the error cases included, and each compiled
// set run by the host replay's per-row function (step_row_serial, rtla_step.h:
// enumerate, materialise, interpret on two rows) on random rows of the layout.
// Every compile ends in a program within the limits or a line:col message;
// every replay ends in counts or an evaluation-error flag.
#include <cstdio>
#include <string>
#include <vector>

#include "rtla_predc.h"
#include "rtla_step.h"
#include "rtla_synth.h"

using namespace rtla;

template <int NS>
static int row_steps(const Layout& L, const uint32_t* row, uint64_t k, const rtla_pred& p, AuditCounters& t) {
  return step_row_serial<NS>(L, row, k, p.code.data(), t);
}

static int dispatch(const Layout& L, const uint32_t* row, uint64_t k, const rtla_pred& p, AuditCounters& t) {
  switch (L.N) {
    case 1: return row_steps<1>(L, row, k, p, t);
    case 2: return row_steps<2>(L, row, k, p, t);
    case 3: return row_steps<3>(L, row, k, p, t);
    case 4: return row_steps<4>(L, row, k, p, t);
    default: return row_steps<5>(L, row, k, p, t);
  }
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::string all;
  char buf[4096];
  for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) all.append(buf, n);
  fclose(f);
  std::vector<std::string> texts;
  for (size_t at = 0; at <= all.size();) {
    const size_t end = std::min(all.find('\x1e', at), all.size());
    texts.push_back(all.substr(at, end - at));
    at = end + 1;
  }
  Layout layouts[3];
  if (make_layout(&layouts[0], 3, 2, 4, 3, 2, 0, 12, 9, 0) || make_layout(&layouts[1], 2, 2, 3, 2, 1, 0, 20, 4, 0) ||
      make_layout(&layouts[2], 5, 1, 3, 2, 1, 0, 64, 32, 0))
    return 2;
  constexpr int ROWS = 40;
  size_t programs = 0, errors = 0, flagged = 0;
  unsigned long long steps = 0, falses = 0;
  for (const Layout& L : layouts) {
    std::vector<uint32_t> rows((size_t)ROWS * L.W);  // (an exact-size buffer: a read past a row's end of the last row
    for (int k = 0; k < ROWS; k++)                    // is a read past an allocation)
      random_state(L, 0x5AF72025ull, synth_state_id(0x5AF72025ull, (uint64_t)k, 0), rows.data() + (size_t)k * L.W);
    for (const std::string& t : texts) {
      std::vector<char> copy(t.begin(), t.end());
      rtla_pred p;
      std::string err;
      if (!pred_compile_step(L, copy.data(), copy.size(), &p, &err)) {
        if (err.empty() || err.find(':') == std::string::npos) {
          fprintf(stderr, "no line:col message: %s\n", t.c_str());
          return 1;
        }
        errors++;
        continue;
      }
      if (!p.step || p.code.empty() || p.code.size() > (size_t)PRED_MAX_WORDS || pred_op(p.code.back()) != P_HALT ||
          p.depth > PRED_STACK || p.steps > PRED_MAX_STEPS || p.names.empty() || p.names.size() > (size_t)PRED_MAX_DEFS) {
        fprintf(stderr, "a program outside the limits: %s\n", t.c_str());
        return 1;
      }
      programs++;
      AuditCounters tl;
      tl = AuditCounters{};
      tl.viol_key = AUDIT_NO_VIOLATION;
      for (int k = 0; k < ROWS; k++) dispatch(L, rows.data() + (size_t)k * L.W, (uint64_t)k, p, tl);
      steps += tl.evaluated;
      for (int d = 0; d < AUDIT_COUNTS; d++) falses += tl.counts[d];
      flagged += tl.flags ? 1 : 0;
    }
  }
  printf("%zu texts, %zu programs, %zu compile errors, %zu replays with an evaluation error, %llu steps, %llu false: ok\n",
         texts.size(), programs, errors, flagged, steps, falses);
  return 0;
}
