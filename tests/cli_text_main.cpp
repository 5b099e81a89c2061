// cli_text_main.cpp -- the command line's text code (raft-tla_amd/csrc/rtla_cli_text.h) as a stand-alone program,
// built with the host sanitizers by tests/test_cli_text_host.py.  Every file named on the command line goes
// through every function -- as a cfg, as a predicate file, and through the trace printer's name substitution --
// whatever it is: a well-formed input prints what was parsed, a hostile one only has to end clean.
#include "rtla_cli_text.h"

static std::string joined(const std::vector<std::string>& v) {
  std::string s;
  for (auto& x : v) s += (s.empty() ? "" : ",") + x;
  return "[" + s + "]";
}

int main(int argc, char** argv) {
  printf("sha256(abc) = %s\n", Sha256().digest("abc").c_str());
  if (read_pred_file("").readable || !read_pred_file("").defs.empty()) return 3;  // no -predicates: nothing read
  for (int a = 1; a < argc; a++) {
    const PredFile f = read_pred_file(argv[a]);
    if (!f.readable) { printf("cannot read %s\n", argv[a]); return 1; }
    const std::string name = std::string(argv[a]).substr(std::string(argv[a]).rfind('/') + 1);
    printf("@@ %s: %zu bytes, %zu tokens\n", name.c_str(), f.text.size(), tokenize(strip_comments(f.text)).size());
    CfgFile c;
    std::string err;
    if (parse_cfg(f.text, &c, &err)) {
      printf("cfg: spec=%s sym=%s inv=%s cons=%s %s=%s", c.specification.c_str(), c.symmetry.c_str(),
             joined(c.invariants).c_str(), joined(c.constraints).c_str(), c.property_keyword.c_str(),
             joined(c.properties).c_str());
      for (auto& s : c.sets) printf(" %s=%s", s.first.c_str(), joined(s.second).c_str());
      for (auto& s : c.scalars) printf(" %s=%s", s.first.c_str(), s.second.c_str());
      printf("\n");
    } else {
      printf("cfg error: %s\n", err.c_str());
    }
    printf("defs: states=%s actions=%s end=%zu\n", joined(definitions_of_kind(f, false)).c_str(),
           joined(definitions_of_kind(f, true)).c_str(), f.end);
    // every other definition kept, both ways: the selection differs from the text in blanks only
    std::vector<std::string> keep;
    for (size_t d = 0; d < f.defs.size(); d += 2) keep.push_back(f.defs[d].name);
    for (int states_only = 0; states_only < 2; states_only++) {
      const std::string sel = select_definitions(f, keep, states_only != 0);
      size_t blanked = 0;
      if (sel.size() != f.text.size()) return 2;
      for (size_t i = 0; i < sel.size(); i++) {
        if (sel[i] == f.text[i]) continue;
        if (sel[i] != ' ' || f.text[i] == '\n') return 2;
        blanked++;
      }
      printf("select(%s, states_only=%d): %zu blanked, %zu definitions left\n", joined(keep).c_str(), states_only,
             blanked, scan_pred_file("", sel, true).defs.size());
    }
    const std::string sub = subst_names(f.text, {"r1", "r2"}, {"x1"});
    if (f.text.size() < 200) printf("subst: %s\n", sub.c_str());
  }
  printf("ok\n");
  return 0;
}
