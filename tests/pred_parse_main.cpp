// pred_parse_main.cpp -- the predicate compiler (raft-tla_amd/csrc/rtla_pred.cpp)
// as a stand-alone host program, for a sanitizer build (tests/test_pred_host.py):
// compiles every text of a corpus file (texts separated by '\x1e') and each of
// them truncated at every byte offset, for several layouts.  Every compile must
// end in a status -- a program within the limits, or a line:col message.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "rtla_predc.h"

using namespace rtla;

static bool check(const Layout& L, const char* text, size_t len, size_t* ok) {
  // (an exact-size copy: a read past the text's end is a read past an allocation)
  std::vector<char> copy(text, text + len);
  rtla_pred p;
  std::string err;
  if (pred_compile(L, copy.data(), copy.size(), &p, &err)) {
    if (p.code.empty() || p.code.size() > (size_t)PRED_MAX_WORDS || pred_op(p.code.back()) != P_HALT ||
        p.depth > PRED_STACK || p.steps > PRED_MAX_STEPS || p.names.size() > (size_t)PRED_MAX_DEFS) {
      fprintf(stderr, "a program outside the limits: %.*s\n", (int)len, text);
      return false;
    }
    for (uint32_t w : p.code) {  // jumps stay inside the program, variables inside the file
      const int op = pred_op(w);
      const bool jump = op == P_JMP || op == P_JZ || op == P_JFK || op == P_JTK || (op >= P_QINIT_A && op <= P_QNEXT_E);
      const bool var = op == P_LOADV || (op >= P_QINIT_A && op <= P_QNEXT_E);
      if (op >= P_OPCOUNT || (jump && pred_target(w) >= (int)p.code.size()) || (var && pred_a(w) >= PRED_VARS)) {
        fprintf(stderr, "a bad instruction %08x: %.*s\n", w, (int)len, text);
        return false;
      }
    }
    ++*ok;
  } else if (err.empty() || err.find(':') == std::string::npos) {
    fprintf(stderr, "no line:col message: %.*s\n", (int)len, text);
    return false;
  }
  return true;
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
  if (make_layout(&layouts[0], 3, 2, 4, 3, 2, 0, 12, 9, 0) || make_layout(&layouts[1], 1, 1, 1, 0, 1, 0, 1, 1, 0) ||
      make_layout(&layouts[2], 5, 1, 3, 2, 1, 0, 64, 32, 0))
    return 2;
  size_t compiles = 0, ok = 0;
  for (const std::string& t : texts)
    for (const Layout& L : layouts) {
      if (!check(L, t.data(), t.size(), &ok)) return 1;
      compiles++;
      if (&L != &layouts[0]) continue;
      for (size_t cut = 0; cut < t.size(); cut++, compiles++)
        if (!check(L, t.data(), cut, &ok)) return 1;
    }
  printf("%zu texts, %zu compiles, %zu programs: ok\n", texts.size(), compiles, ok);
  return 0;
}
