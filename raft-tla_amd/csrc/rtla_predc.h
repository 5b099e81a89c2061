// rtla_predc.h -- a compiled predicate set and the compiler's entry point
// (rtla_pred.cpp: host only, no HIP).  The C ABI around them (rtla_pred_*) is
// rtla_predhost.cpp.
#pragma once
#include <string>
#include <vector>

#include "rtla_pred.h"

struct rtla_pred {
  rtla::Layout L{};                // the layout the set was compiled for (and is bound to)
  std::vector<uint32_t> code;      // the program, P_HALT last
  std::vector<std::string> names;  // definition k = bit k
  uint64_t steps = 0;              // worst-case instructions per row
  int depth = 0;                   // operand depth reached
  bool step = false;               // an action set: the program reads a step's two rows (pred_eval_rows)
};

namespace rtla {

// Compiles `text` (len bytes) for layout L.  false: *err = "line:col: message".
bool pred_compile(const Layout& L, const char* text, size_t len, rtla_pred* out, std::string* err);
// The same for the text's action definitions `Name == [][ expr ]_vars`; its state
// definitions are parsed, type-checked and skipped.  A text without an action definition is an error.
bool pred_compile_step(const Layout& L, const char* text, size_t len, rtla_pred* out, std::string* err);


// A set is bound to the row format it was compiled for: the model's bounds and capacities (make_layout derives
// every offset and width from them).
inline bool pred_bound_to(const rtla_pred* p, const Layout& L) {
  const Layout& q = p->L;
  return q.N == L.N && q.V == L.V && q.T == L.T && q.L == L.L && q.C == L.C && q.M == L.M && q.K == L.K &&
         q.E == L.E && q.W == L.W;
}

}  // namespace rtla
