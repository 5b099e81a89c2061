// rtla_cli.cpp -- TLC-compatible command line over librtla.so.
//
// Replaces the reference's invocation (reference README.md:5, raft.cfg:1-15,
// .vscode/settings.json:5):
//     java tlc2.TLC [-workers W] [-coverage M] -config raft.cfg raft.tla
// with
//     rtla [-workers W] [-coverage M] [-gpus G] [-fpbits B] -config X.cfg SPEC.tla
// and TLC's simulation mode (-simulate [num=N] -depth D -seed S) with
//     rtla -simulate [num=N[,first=F]] [-depth D] [-seed S] [-bfs-levels K] -config X.cfg SPEC.tla
// and an audit of the last BFS level for invariants the search did not carry
//     rtla -audit Name[,Name...] [-bfs-levels K] -config X.cfg SPEC.tla
// (after the BFS stops -- exhausted, out of capacity, or after K levels -- the
// named invariants are evaluated over the states of the level last produced).
// -simulate runs K BFS levels (default 1: Init only, TLC's plain -simulate) and
// then N random walks of up to D steps from the states of level K (walk w
// starts at state w mod |level K|).  Walk ids are global: processes given
// disjoint [F, F + N) ranges and the same seed explore disjoint walks, so a
// large simulation can be split over GPUs by hand (-gpus > 1 is refused).
// TLC's "add an operator to MC.tla and name it under INVARIANT" is
//     rtla -predicates FILE -config X.cfg SPEC.tla
// a name under INVARIANT(S) or -audit that is not built in is looked up in FILE
// (the predicate language of DESIGN.md section 13), compiled, and checked on
// every level of the search right after it is produced (-gpus 1 only).
// A name under PROPERTY / PROPERTIES is accepted when it is an action definition
// `Name == [][A]_vars` of FILE: it is checked on every
// step out of every level; -audit may name one too (the steps out of the last level).
// With -simulate the same sets go into the walks.
// A name under CONSTRAINT(S) beside StateConstraint is a state definition of FILE
// (specs/MCConstraints.tla) and prunes every level right after its invariants
// were checked; not with -simulate.
//
// SPEC.tla is either the reference's raft.tla (sha256 checked: the semantics
// are compiled into the kernels, not parsed) or a wrapper module that
// EXTENDS raft and defines the model-checking operators of specs/MC.tla
// (StateConstraint, NoTwoLeaders, ElectionSafety, LogMatching,
// StateMachineSafety, LeaderCompleteness); the raft.tla
// next to it is then hash-checked.  The cfg grammar is TLC's subset used by
// raft.cfg: SPECIFICATION, INVARIANT(S), CONSTRAINT(S), CONSTANT(S) with
// `Name = {a, b}` / `Name = "str"` / `Name = 3` / `Name = mv`, and \* / (* *)
// comments.  Output follows TLC's stdout lines.  Exit codes: 0 = no error,
// 12 = safety violation, 150/151 = spec/config errors, 255 = other errors
// (TLC's ExitStatus values as we understand them; not verified against a
// live TLC here).
#include <ctype.h>
#include <errno.h>
#include <signal.h>
#include <spawn.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/wait.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <filesystem>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/rtla.h"

extern char** environ;

static const char* RAFT_SHA256 = "683a120af29e3e5a805e291f756229d65914f8fb73dddd8c78bafef50a6f6b81";

// ------------------------------------------------------------- sha256 ----
namespace {
struct Sha256 {
  uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
  static uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
  void block(const uint8_t* p) {
    static const uint32_t k[64] = {
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
        0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
        0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
        0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
        0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
        0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
        0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
        0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
    uint32_t w[64];
    for (int i = 0; i < 16; i++) w[i] = (uint32_t)p[4 * i] << 24 | p[4 * i + 1] << 16 | p[4 * i + 2] << 8 | p[4 * i + 3];
    for (int i = 16; i < 64; i++) {
      uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3);
      uint32_t s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
      w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
    for (int i = 0; i < 64; i++) {
      uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + k[i] + w[i];
      uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
      hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
  }
  std::string digest(const std::string& data) {
    std::string m = data;
    uint64_t bits = (uint64_t)data.size() * 8;
    m.push_back((char)0x80);
    while (m.size() % 64 != 56) m.push_back(0);
    for (int i = 7; i >= 0; i--) m.push_back((char)(bits >> (8 * i)));
    for (size_t o = 0; o < m.size(); o += 64) block((const uint8_t*)m.data() + o);
    char out[65];
    for (int i = 0; i < 8; i++) snprintf(out + 8 * i, 9, "%08x", h[i]);
    return out;
  }
};

std::string read_file(const std::string& p, bool* ok) {
  std::ifstream f(p, std::ios::binary);
  *ok = (bool)f;
  std::stringstream ss;
  ss << f.rdbuf();
  return ss.str();
}

std::string now_str() {
  time_t t = time(nullptr);
  char b[64];
  strftime(b, sizeof b, "%Y-%m-%d %H:%M:%S", localtime(&t));
  return b;
}

// ------------------------------------------------------------ cfg parse ----
struct CfgFile {
  std::string specification;
  std::string symmetry;  // SYMMETRY operator name ("" = none)
  std::vector<std::string> invariants, constraints;
  std::vector<std::string> properties;  // PROPERTY / PROPERTIES names (action definitions of the -predicates file)
  std::string property_keyword;         // the keyword they stood under, for the refusal
  std::map<std::string, std::vector<std::string>> sets;  // Name = {a, b}
  std::map<std::string, std::string> scalars;            // Name = "x" | 3 | mv
};

std::string strip_comments(const std::string& s) {
  std::string o;
  for (size_t i = 0; i < s.size();) {
    if (s.compare(i, 2, "\\*") == 0) {
      while (i < s.size() && s[i] != '\n') i++;
    } else if (s.compare(i, 2, "(*") == 0) {
      size_t j = s.find("*)", i + 2);
      i = j == std::string::npos ? s.size() : j + 2;
    } else {
      o.push_back(s[i++]);
    }
  }
  return o;
}

std::vector<std::string> tokenize(const std::string& s) {
  std::vector<std::string> t;
  for (size_t i = 0; i < s.size();) {
    char c = s[i];
    if (isspace((unsigned char)c)) { i++; continue; }
    if (c == '"') {
      size_t j = s.find('"', i + 1);
      if (j == std::string::npos) j = s.size() - 1;
      t.push_back(s.substr(i, j - i + 1));
      i = j + 1;
      continue;
    }
    if (c == '{' || c == '}' || c == ',' || c == '=') { t.push_back(std::string(1, c)); i++; continue; }
    if (c == '<' && s.compare(i, 2, "<-") == 0) { t.push_back("<-"); i += 2; continue; }
    size_t j = i;
    while (j < s.size() && !isspace((unsigned char)s[j]) && strchr("{},=\"", s[j]) == nullptr) j++;
    t.push_back(s.substr(i, j - i));
    i = j;
  }
  return t;
}

bool parse_cfg(const std::string& text, CfgFile* c, std::string* err) {
  auto t = tokenize(strip_comments(text));
  static const char* KW[] = {"SPECIFICATION", "INVARIANT", "INVARIANTS", "CONSTRAINT", "CONSTRAINTS",
                             "CONSTANT", "CONSTANTS", "INIT", "NEXT", "PROPERTY", "PROPERTIES",
                             "SYMMETRY", "VIEW", "CHECK_DEADLOCK", "ACTION_CONSTRAINT", "ACTION_CONSTRAINTS"};
  auto is_kw = [&](const std::string& s) {
    for (auto k : KW) if (s == k) return true;
    return false;
  };
  std::string mode;
  for (size_t i = 0; i < t.size();) {
    if (is_kw(t[i])) { mode = t[i++]; continue; }
    if (mode == "SPECIFICATION") { c->specification = t[i++]; continue; }
    if (mode == "INVARIANT" || mode == "INVARIANTS") { c->invariants.push_back(t[i++]); continue; }
    if (mode == "CONSTRAINT" || mode == "CONSTRAINTS") { c->constraints.push_back(t[i++]); continue; }
    if (mode == "CONSTANT" || mode == "CONSTANTS") {
      if (i + 2 >= t.size() || (t[i + 1] != "=" && t[i + 1] != "<-")) { *err = "bad CONSTANT near '" + t[i] + "'"; return false; }
      std::string name = t[i];
      i += 2;
      if (t[i] == "{") {
        std::vector<std::string> v;
        i++;
        while (i < t.size() && t[i] != "}") {
          if (t[i] != ",") v.push_back(t[i]);
          i++;
        }
        i++;
        c->sets[name] = v;
      } else {
        c->scalars[name] = t[i++];
      }
      continue;
    }
    if (mode == "SYMMETRY") { c->symmetry = t[i++]; continue; }
    if (mode == "PROPERTY" || mode == "PROPERTIES") {  // (accepted or refused once the predicate file is known)
      c->property_keyword = mode;
      c->properties.push_back(t[i++]);
      continue;
    }
    if (mode == "VIEW" || mode == "INIT" || mode == "NEXT" || mode == "ACTION_CONSTRAINT" ||
        mode == "ACTION_CONSTRAINTS") {
      *err = mode + " is not supported by this checker";
      return false;
    }
    if (mode == "CHECK_DEADLOCK") { i++; continue; }
    *err = "unexpected token '" + t[i] + "'";
    return false;
  }
  return true;
}

void usage() {
  fprintf(stderr,
          "usage: rtla [-workers W] [-coverage M] [-gpus G] [-fpbits B] [-membudget BYTES] [-dump-levels]\n"
          "            [-raft PATH/raft.tla] [-skip-spec-check]\n"
          "            [-checkpoint MINUTES] [-checkpointdir PREFIX] [-recover PREFIX]\n"
          "            [-simulate [num=N[,first=F]]] [-depth D] [-seed S] [-bfs-levels K]\n"
          "            [-audit Name[,Name...]] [-predicates FILE]\n"
          "            -config FILE.cfg SPEC.tla\n"
          "  -simulate: after K BFS levels (default 1 = Init only) run N random walks (default 1000000) of up to\n"
          "  D steps (default 100) from the states of level K; walk ids F .. F+N-1 are global, so runs with\n"
          "  disjoint ranges and the same seed compose; one GPU only.  With -predicates FILE the cfg's user\n"
          "  INVARIANT and PROPERTY names are checked in the walks too: the action properties on every step out of\n"
          "  every state a walk visits, the invariants on every in-model successor.\n"
          "  -predicates FILE: definitions in the predicate language (specs/MCPredicates.tla) that INVARIANT(S) and\n"
          "          -audit may name beside the built-in invariants; checked on every level of the search (-gpus 1).\n"
          "          Its action definitions `Name == [][A]_vars` (specs/MCActions.tla) may be named under\n"
          "          PROPERTY / PROPERTIES, and are then checked on every step out of every level, or under -audit\n"
          "          (the steps out of the last level).  A state definition (specs/MCConstraints.tla) may be named\n"
          "          under CONSTRAINT(S) beside StateConstraint: it prunes every level of the search (no -simulate)\n"
          "  -audit: when the BFS stops (exhausted, out of capacity, or after -bfs-levels K) evaluate the named\n"
          "  invariants -- any of the specification's, not only the cfg's -- over the states of the last level;\n"
          "  one GPU only.\n");
}

std::string subst_names(const std::string& s, const std::vector<std::string>& servers,
                         const std::vector<std::string>& values) {
  // The row printer names servers s1..sN and values v1..vV; map them to the
  // cfg's model values.
  std::string o;
  for (size_t i = 0; i < s.size();) {
    char c = s[i];
    bool boundary = i == 0 || !(isalnum((unsigned char)s[i - 1]) || s[i - 1] == '_' || s[i - 1] == '"');
    if (boundary && (c == 's' || c == 'v') && i + 1 < s.size() && isdigit((unsigned char)s[i + 1]) &&
        (i + 2 >= s.size() || !isalnum((unsigned char)s[i + 2]))) {
      int k = s[i + 1] - '1';
      const auto& names = c == 's' ? servers : values;
      if (k >= 0 && k < (int)names.size()) { o += names[k]; i += 2; continue; }
    }
    o.push_back(c);
    i++;
  }
  return o;
}

// ---- -gpus N: one process per GPU.  The launcher (this process, which never
// touches a GPU) spawns N copies of itself with RTLA_RANK / RTLA_WORLD /
// RTLA_RENDEZVOUS in the environment and relays rank 0's exit status.  Rank 0
// creates the RCCL unique id and publishes it through the rendezvous file;
// every rank opens its context with it (rtla_open, one shard per rank).
int launch_ranks(int n, char** argv) {
  char dir[] = "/tmp/rtla-rdv-XXXXXX";
  if (!mkdtemp(dir)) { perror("mkdtemp"); return 255; }
  const std::string rdv = std::string(dir) + "/comm_id";
  std::vector<pid_t> pids;
  for (int r = 0; r < n; r++) {
    std::vector<std::string> env;
    for (char** e = environ; *e; e++)
      if (strncmp(*e, "RTLA_RANK=", 10) && strncmp(*e, "RTLA_WORLD=", 11) && strncmp(*e, "RTLA_RENDEZVOUS=", 16))
        env.push_back(*e);
    env.push_back("RTLA_RANK=" + std::to_string(r));
    env.push_back("RTLA_WORLD=" + std::to_string(n));
    env.push_back("RTLA_RENDEZVOUS=" + rdv);
    std::vector<char*> envp;
    for (auto& e : env) envp.push_back((char*)e.c_str());
    envp.push_back(nullptr);
    pid_t pid = 0;
    if (posix_spawn(&pid, "/proc/self/exe", nullptr, nullptr, argv, envp.data()) != 0) {
      perror("posix_spawn");
      return 255;
    }
    pids.push_back(pid);
  }
  // Reap ranks in whatever order they end.  A rank killed by a signal, or
  // ending with an error status other than the ones every rank reaches
  // together (0, 12 = invariant violated, 150/151 = spec/cfg errors), may
  // leave the others blocked in a collective: they get a grace period to end
  // on their own, then SIGTERM, then SIGKILL.  No rank is ever restarted.
  int code0 = 0, worst = 0, left = n;
  std::vector<bool> done(n, false);
  double abort_at = -1.0;  // monotonic seconds at which the survivors are terminated
  bool termed = false;
  auto now = []() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + ts.tv_nsec * 1e-9;
  };
  while (left > 0) {
    int st = 0;
    const pid_t pid = waitpid(-1, &st, WNOHANG);
    if (pid > 0) {
      int r = 0;
      while (r < n && pids[r] != pid) r++;
      if (r == n || done[r]) continue;
      done[r] = true;
      left--;
      const int code = WIFEXITED(st) ? WEXITSTATUS(st) : 255;
      if (r == 0) code0 = code;
      else if (code && !worst) worst = code;
      const bool abnormal = !WIFEXITED(st) || (code != 0 && code != 12 && code != 150 && code != 151);
      if (abnormal && abort_at < 0 && left > 0) {
        fprintf(stderr, "rtla: rank %d ended abnormally (%s %d); stopping the other ranks in 10 s\n", r,
                WIFEXITED(st) ? "exit status" : "signal", WIFEXITED(st) ? code : WTERMSIG(st));
        abort_at = now() + 10.0;
      }
      continue;
    }
    if (pid < 0 && errno != EINTR) break;
    if (abort_at >= 0 && now() > abort_at) {
      for (int r = 0; r < n; r++)
        if (!done[r]) kill(pids[r], termed ? SIGKILL : SIGTERM);
      abort_at = now() + 5.0;
      termed = true;
    }
    usleep(20000);
  }
  (void)remove(rdv.c_str());
  (void)rmdir(dir);
  return code0 ? code0 : worst;
}

// This rank's RCCL id: rank 0 makes it (dry run: a fixed pattern, no GPU) and
// publishes it atomically (write + rename); the others wait for the file.
bool rendezvous(int rank, const char* path, bool dry, unsigned char id[128]) {
  if (rank == 0) {
    if (dry) {
      for (int k = 0; k < 128; k++) id[k] = (unsigned char)k;
    } else if (rtla_comm_id(id) != RTLA_OK) {
      return false;
    }
    const std::string tmp = std::string(path) + ".tmp";
    FILE* f = fopen(tmp.c_str(), "wb");
    if (!f || fwrite(id, 1, 128, f) != 128) return false;
    if (fclose(f) != 0 || rename(tmp.c_str(), path) != 0) return false;
    return true;
  }
  for (int t = 0; t < 1200; t++) {  // up to 120 s
    FILE* f = fopen(path, "rb");
    if (f) {
      const bool ok = fread(id, 1, 128, f) == 128;
      fclose(f);
      if (ok) return true;
    }
    usleep(100000);
  }
  return false;
}

// The invariants of specs/MC.tla, in RTLA_INV_* bit order.
const struct { const char* name; int32_t bit; } INVARIANTS[] = {
    {"NoTwoLeaders", RTLA_INV_NO_TWO_LEADERS},
    {"ElectionSafety", RTLA_INV_ELECTION_SAFETY},
    {"LogMatching", RTLA_INV_LOG_MATCHING},
    {"StateMachineSafety", RTLA_INV_STATE_MACHINE_SAFETY},
    {"LeaderCompleteness", RTLA_INV_LEADER_COMPLETENESS}};
int32_t invariant_bit(const std::string& name) {
  for (auto& i : INVARIANTS)
    if (name == i.name) return i.bit;
  return 0;
}

// ---- -predicates FILE: user-defined invariants

// `text` with every definition whose name is not in `keep` blanked out (line breaks kept, so a compile error's
// line:col is the file's): the set compiled is the set named, and only it is evaluated.  A definition starts at
// an identifier followed by `==` outside comments and ends where the next one, or the module's closing line, starts.
struct Def {
  size_t at;
  std::string name;
  bool action;  // Name == [][ ... ]_vars
};
// The definitions of a predicate file, in file order; *end: where the module's closing line starts.
std::vector<Def> scan_definitions(const std::string& text, size_t* end) {
  std::vector<Def> defs;
  *end = text.size();
  for (size_t i = 0; i < text.size();) {
    if (text.compare(i, 2, "\\*") == 0) {
      while (i < text.size() && text[i] != '\n') i++;
    } else if (text.compare(i, 2, "(*") == 0) {
      int deep = 0;
      do {
        if (text.compare(i, 2, "(*") == 0) { deep++; i += 2; }
        else if (text.compare(i, 2, "*)") == 0) { deep--; i += 2; }
        else i++;
      } while (deep > 0 && i < text.size());
    } else if (text.compare(i, 4, "====") == 0) {
      *end = i;
      break;
    } else if (isalpha((unsigned char)text[i]) || text[i] == '_') {
      size_t j = i;
      while (j < text.size() && (isalnum((unsigned char)text[j]) || text[j] == '_')) j++;
      size_t k = j;
      while (k < text.size() && (text[k] == ' ' || text[k] == '\t')) k++;
      if (text.compare(k, 2, "==") == 0 && text.compare(k, 3, "===") != 0) {
        std::string head;  // the body's first three characters that are not blanks
        for (size_t q = k + 2; q < text.size() && head.size() < 3; q++)
          if (!isspace((unsigned char)text[q])) head.push_back(text[q]);
        defs.push_back({i, text.substr(i, j - i), head == "[]["});
      }
      i = j;
    } else {
      i++;
    }
  }
  return defs;
}
std::string select_definitions(const std::string& text, const std::vector<std::string>& keep) {
  size_t end = 0;
  const std::vector<Def> defs = scan_definitions(text, &end);
  std::string out = text;
  for (size_t d = 0; d < defs.size(); d++) {
    if (std::find(keep.begin(), keep.end(), defs[d].name) != keep.end()) continue;
    const size_t stop = d + 1 < defs.size() ? defs[d + 1].at : end;
    for (size_t i = defs[d].at; i < stop; i++)
      if (out[i] != '\n') out[i] = ' ';
  }
  return out;
}

// The names of the file's definitions of one kind (action: Name == [][ ... ]_vars), in file order.
std::vector<std::string> definitions_of_kind(const std::string& text, bool action) {
  size_t end = 0;
  std::vector<std::string> out;
  for (const Def& d : scan_definitions(text, &end))
    if (d.action == action) out.push_back(d.name);
  return out;
}

// The action definitions `names` of the predicate file (PROPERTY, -audit), compiled for *c as a step set.  The
// caller has checked that every name is an action definition of the file.
rtla_pred* load_actions(const rtla_cfg* c, const std::string& path, const std::vector<std::string>& names) {
  bool ok = false;
  const std::string text = read_file(path, &ok);
  if (!ok) { printf("Error: cannot read the predicate file %s\n", path.c_str()); exit(150); }
  char err[512];
  rtla_pred* set = nullptr;
  if (rtla_pred_compile_step(c, select_definitions(text, names).c_str(), &set, err, sizeof err) != RTLA_OK) {
    printf("Error: %s:%s\n", path.c_str(), err[0] ? err : " the configuration is outside the row format");
    exit(150);
  }
  return set;
}

// The state definitions `names` of the predicate file, compiled for *c; exits as for an undefined invariant.
// The file is split by kind first: its action definitions are blanked out, INVARIANT names none of them.
rtla_pred* load_predicates(const rtla_cfg* c, const std::string& path, const std::vector<std::string>& names) {
  std::ifstream in(path);
  if (!in) { printf("Error: cannot read the predicate file %s\n", path.c_str()); exit(150); }
  std::stringstream file;
  file << in.rdbuf();
  std::stringstream ss;
  ss << select_definitions(file.str(), definitions_of_kind(file.str(), false));
  char err[512];
  rtla_pred* all = nullptr;
  if (rtla_pred_compile(c, ss.str().c_str(), &all, err, sizeof err) != RTLA_OK) {
    printf("Error: %s:%s\n", path.c_str(), err[0] ? err : " the configuration is outside the row format");
    exit(150);
  }
  for (auto& nm : names) {
    bool found = false;
    char buf[256];
    for (int k = 0; k < rtla_pred_count(all); k++)
      found |= rtla_pred_name(all, k, buf, sizeof buf) >= 0 && nm == buf;
    if (!found) {
      printf("Error: The invariant %s specified in the configuration file is not defined in the specification.\n",
             nm.c_str());
      exit(150);
    }
  }
  rtla_pred_free(all);
  rtla_pred* set = nullptr;
  if (rtla_pred_compile(c, select_definitions(ss.str(), names).c_str(), &set, err, sizeof err) != RTLA_OK) {
    printf("Error: %s:%s\n", path.c_str(), err);
    exit(150);
  }
  return set;
}
std::string pred_name(const rtla_pred* p, int k) {
  char buf[256] = "";
  rtla_pred_name(p, k, buf, sizeof buf);
  return buf;
}

const char* COVER[] = {"Restart", "Timeout", "RequestVote", "BecomeLeader", "ClientRequest",
                       "AdvanceCommitIndex", "AppendEntries", "Receive", "DuplicateMessage", "DropMessage",
                       "UpdateTerm", "HandleRequestVoteRequest", "HandleRequestVoteResponse",
                       "HandleAppendEntriesRequest", "HandleAppendEntriesResponse", "DropStaleResponse"};
}  // namespace

int main(int argc, char** argv) {
  std::string cfgpath, spec;
  int coverage = 0, gpus = 1, fpbits = 0, workers = 1;
  bool dump_levels = false, skip_spec_check = false;
  std::string raft_opt;
  uint64_t membudget = 0;
  // TLC -checkpoint <minutes> / -recover <path> (the reference's .gitignore:2 states/ dir)
  double ckpt_minutes = 0;
  std::string ckpt_prefix = "states/ckpt", recover_prefix;
  // TLC -simulate [num=N] / -depth D / -seed S, here from the states of BFS level -bfs-levels K
  bool simulate = false;
  uint64_t sim_num = 1000000, sim_first = 0, sim_seed = 0;
  bool have_seed = false;
  int sim_depth = 100, bfs_levels = 1;
  bool have_levels = false;
  // -audit Name[,Name...]: invariants evaluated over the last BFS level
  bool audit = false;
  std::vector<std::string> audit_names;
  // -predicates FILE: definitions that INVARIANT(S) and -audit may name beside the built-in ones
  std::string pred_file;
  for (int i = 1; i < argc; i++) {
    std::string a = argv[i];
    auto next = [&]() -> std::string {
      if (i + 1 >= argc) { usage(); exit(255); }
      return argv[++i];
    };
    if (a == "-config") cfgpath = next();
    else if (a == "-coverage") coverage = atoi(next().c_str());
    else if (a == "-workers") { std::string w = next(); workers = w == "auto" ? 0 : atoi(w.c_str()); }
    else if (a == "-gpus") gpus = atoi(next().c_str());
    else if (a == "-fpbits") fpbits = atoi(next().c_str());
    else if (a == "-membudget") membudget = strtoull(next().c_str(), nullptr, 10);
    else if (a == "-dump-levels") dump_levels = true;
    else if (a == "-raft") raft_opt = next();
    else if (a == "-skip-spec-check") skip_spec_check = true;
    else if (a == "-checkpoint") ckpt_minutes = atof(next().c_str());
    else if (a == "-checkpointdir") ckpt_prefix = next();
    else if (a == "-recover") recover_prefix = next();
    else if (a == "-simulate") {
      simulate = true;
      if (i + 1 < argc && (!strncmp(argv[i + 1], "num=", 4) || !strncmp(argv[i + 1], "first=", 6))) {
        std::stringstream opts(argv[++i]);
        for (std::string kv; std::getline(opts, kv, ',');) {
          if (kv.compare(0, 4, "num=") == 0) sim_num = strtoull(kv.c_str() + 4, nullptr, 10);
          else if (kv.compare(0, 6, "first=") == 0) sim_first = strtoull(kv.c_str() + 6, nullptr, 10);
          else { fprintf(stderr, "Error: -simulate: unknown option %s\n", kv.c_str()); return 255; }
        }
      }
    }
    else if (a == "-depth") sim_depth = atoi(next().c_str());
    else if (a == "-seed") { sim_seed = strtoull(next().c_str(), nullptr, 10); have_seed = true; }
    else if (a == "-bfs-levels") { bfs_levels = atoi(next().c_str()); have_levels = true; }
    else if (a == "-audit") {
      audit = true;
      std::stringstream names(next());
      for (std::string nm; std::getline(names, nm, ',');)
        if (!nm.empty()) audit_names.push_back(nm);
    }
    else if (a == "-predicates") pred_file = next();
    else if (a == "-h" || a == "-help") { usage(); return 0; }
    else if (!a.empty() && a[0] == '-') { fprintf(stderr, "Error: unsupported option %s\n", a.c_str()); return 255; }
    else spec = a;
  }
  (void)workers;
  if (gpus < 1) { usage(); return 255; }
  if (simulate && gpus > 1) {
    fprintf(stderr, "Error: -simulate runs on one GPU; split the walks over processes instead "
                    "(-simulate num=N,first=F with disjoint ranges and the same -seed)\n");
    return 255;
  }
  if (audit && (gpus > 1 || simulate || audit_names.empty())) {
    fprintf(stderr, "Error: -audit names at least one invariant and runs on one GPU, without -simulate\n");
    return 255;
  }
  if (!pred_file.empty() && gpus > 1) {
    fprintf(stderr, "Error: -predicates checks user-defined invariants on one GPU (a single shard); use -gpus 1\n");
    return 255;
  }
  if (audit && bfs_levels < 1) {
    fprintf(stderr, "Error: -bfs-levels must be at least 1\n");
    return 255;
  }
  if (simulate && (sim_depth < 0 || sim_depth > 65535 || bfs_levels < 1)) {
    fprintf(stderr, "Error: -depth must be 0..65535 and -bfs-levels at least 1\n");
    return 255;
  }
  if (simulate && !have_seed) sim_seed = (uint64_t)time(nullptr) ^ (uint64_t)getpid() << 32;  // printed, as TLC does
  if (gpus > 1 && !getenv("RTLA_RANK")) return launch_ranks(gpus, argv);
  const int rank = getenv("RTLA_RANK") ? atoi(getenv("RTLA_RANK")) : 0;
  const int world = getenv("RTLA_WORLD") ? atoi(getenv("RTLA_WORLD")) : 1;
  if (world != gpus || rank < 0 || rank >= world) {
    fprintf(stderr, "Error: rank %d of %d does not match -gpus %d\n", rank, world, gpus);
    return 255;
  }
  if (rank > 0 && !freopen("/dev/null", "w", stdout)) return 255;  // rank 0 prints TLC's output
  const bool dry = getenv("RTLA_CLI_DRYRUN") != nullptr;
  if (dry) {  // launch / rendezvous check only (CPU tests)
    unsigned char id[128];
    const char* rdv = getenv("RTLA_RENDEZVOUS");
    const bool ok = world == 1 || (rdv && rendezvous(rank, rdv, true, id));
    fprintf(stderr, "rtla rank %d of %d ready (id %02x%02x%02x%02x)\n", rank, world, ok ? id[0] : 255, ok ? id[1] : 255,
            ok ? id[2] : 255, ok ? id[3] : 255);
    return ok ? 0 : 255;
  }
  if (spec.empty()) { usage(); return 255; }
  if (cfgpath.empty()) {
    cfgpath = spec.substr(0, spec.size() > 4 && spec.compare(spec.size() - 4, 4, ".tla") == 0 ? spec.size() - 4 : spec.size()) + ".cfg";
  }
  printf("rtla (MI355X-native explicit-state checker for raft.tla), ABI %d\n", rtla_abi_version());
  // --- spec identity
  bool ok = false;
  std::string spec_text = read_file(spec, &ok);
  if (!ok) { printf("Error: cannot read %s\n", spec.c_str()); return 150; }
  std::string dir = spec.find('/') == std::string::npos ? "." : spec.substr(0, spec.rfind('/'));
  std::string base = spec.substr(spec.find('/') == std::string::npos ? 0 : spec.rfind('/') + 1);
  bool wrapper = base != "raft.tla";
  std::string raft_path = !raft_opt.empty() ? raft_opt : wrapper ? dir + "/raft.tla" : spec;
  std::string raft_text = raft_path == spec ? spec_text : read_file(raft_path, &ok);
  if (!ok && !skip_spec_check) {
    printf("Error: %s EXTENDS raft but %s is missing (give -raft PATH)\n", spec.c_str(), raft_path.c_str());
    return 150;
  }
  std::string h = skip_spec_check ? std::string(RAFT_SHA256) : Sha256().digest(raft_text);
  if (skip_spec_check) printf("Warning: -skip-spec-check: the identity of raft.tla is NOT verified\n");
  if (h != RAFT_SHA256) {
    printf("Error: %s has sha256 %s; this checker compiles the semantics of raft.tla %s only.\n",
           raft_path.c_str(), h.c_str(), RAFT_SHA256);
    return 150;
  }
  if (wrapper && spec_text.find("EXTENDS raft") == std::string::npos) {
    printf("Error: %s does not EXTEND raft\n", spec.c_str());
    return 150;
  }
  printf("Parsing file %s (raft.tla sha256 %.12s... verified)\n", spec.c_str(), h.c_str());
  // --- cfg
  std::string cfg_text = read_file(cfgpath, &ok);
  if (!ok) { printf("Error: cannot read config %s\n", cfgpath.c_str()); return 151; }
  CfgFile cf;
  std::string err;
  if (!parse_cfg(cfg_text, &cf, &err)) { printf("Error: %s: %s\n", cfgpath.c_str(), err.c_str()); return 151; }
  // PROPERTY names are the action definitions of the -predicates file; anything else is refused as ever
  std::vector<std::string> action_names;
  if (!pred_file.empty()) {
    bool pf_ok = false;
    action_names = definitions_of_kind(read_file(pred_file, &pf_ok), true);
  }
  auto is_action = [&](const std::string& nm) {
    return std::find(action_names.begin(), action_names.end(), nm) != action_names.end();
  };
  if (!cf.properties.empty() && !std::all_of(cf.properties.begin(), cf.properties.end(), is_action)) {
    printf("Error: %s: %s is not supported by this checker\n", cfgpath.c_str(), cf.property_keyword.c_str());
    return 151;
  }
  if (!cf.specification.empty() && cf.specification != "Spec") {
    printf("Error: SPECIFICATION %s: only Spec (raft.tla:469) is supported\n", cf.specification.c_str());
    return 151;
  }
  // Operators available: raft.tla defines none of the MC operators.
  auto defined = [&](const std::string& op) {
    if (!wrapper) return false;
    return op == "StateConstraint" || invariant_bit(op) != 0;
  };
  rtla_cfg c;
  memset(&c, 0, sizeof c);
  std::vector<std::string> user_invs, user_audit;  // names to look up in the predicate file
  for (auto& inv : cf.invariants) {
    if (!pred_file.empty() && !defined(inv)) { user_invs.push_back(inv); continue; }
    if (!defined(inv) || inv == "StateConstraint") {
      printf("Error: The invariant %s specified in the configuration file is not defined in the specification.\n",
             inv.c_str());
      return 150;
    }
    c.inv_mask |= invariant_bit(inv);
  }
  int32_t audit_mask = 0;
  std::vector<std::string> audit_actions;  // -audit names that are action definitions of the predicate file
  for (auto& inv : audit_names) {
    if (is_action(inv)) { audit_actions.push_back(inv); continue; }
    if (!pred_file.empty() && !defined(inv)) { user_audit.push_back(inv); continue; }
    if (!defined(inv) || inv == "StateConstraint") {
      printf("Error: The invariant %s specified in the configuration file is not defined in the specification.\n",
             inv.c_str());
      return 150;
    }
    audit_mask |= invariant_bit(inv);
  }
  // CONSTRAINT names StateConstraint (the compiled-in bounds); any further name is a state definition of the
  // -predicates file, and prunes every level on the GPU (rtla_pred_constrain)
  std::vector<std::string> user_cons;
  bool built_in_constraint = false;
  {
    std::vector<std::string> state_names;
    if (!pred_file.empty()) {
      bool pf_ok = false;
      state_names = definitions_of_kind(read_file(pred_file, &pf_ok), false);
    }
    for (auto& k : cf.constraints) {
      if (k == "StateConstraint" && defined(k)) { built_in_constraint = true; continue; }
      if (is_action(k)) {
        printf("Error: The constraint %s is an action definition; a CONSTRAINT is a state predicate "
               "(ACTION_CONSTRAINT is not supported by this checker).\n", k.c_str());
        return 150;
      }
      if (std::find(state_names.begin(), state_names.end(), k) == state_names.end()) {
        printf("Error: The constraint %s specified in the configuration file is not defined in the specification.\n",
               k.c_str());
        return 150;
      }
      if (std::find(user_cons.begin(), user_cons.end(), k) == user_cons.end()) user_cons.push_back(k);
    }
  }
  if (!user_cons.empty() && simulate) {
    printf("Error: -simulate with a user-defined CONSTRAINT (%s) is not supported: the random walks do not honour "
           "constraints, and are not run unconstrained in their place.\n", user_cons[0].c_str());
    return 150;
  }
  if (!cf.symmetry.empty()) {
    if (!wrapper || cf.symmetry != "Perms") {
      printf("Error: The symmetry %s specified in the configuration file is not defined in the specification.\n",
             cf.symmetry.c_str());
      return 150;
    }
    c.symmetry = 1;  // Perms == Permutations(Server) (specs/MC.tla)
  }
  if (!built_in_constraint) {
    printf("Error: no CONSTRAINT: raft.tla's state space is infinite (Timeout raft.tla:180 and Send raft.tla:106-110 "
           "are unbounded); add CONSTRAINT StateConstraint from specs/MC.tla.\n");
    return 151;
  }
  auto need_set = [&](const char* n) -> std::vector<std::string> {
    auto it = cf.sets.find(n);
    if (it == cf.sets.end()) { printf("Error: constant %s is not assigned a set in %s\n", n, cfgpath.c_str()); exit(151); }
    return it->second;
  };
  auto need_int = [&](const char* n) -> int {
    auto it = cf.scalars.find(n);
    if (it == cf.scalars.end()) { printf("Error: constant %s is not assigned in %s\n", n, cfgpath.c_str()); exit(151); }
    return atoi(it->second.c_str());
  };
  std::vector<std::string> servers = need_set("Server"), values = need_set("Value");
  c.n_server = (int)servers.size();
  c.n_value = (int)values.size();
  c.max_term = need_int("MaxTerm");
  c.max_log = need_int("MaxLogLen");
  c.max_copies = need_int("MaxCopies");
  c.max_msgs = cf.scalars.count("MaxInFlight") ? need_int("MaxInFlight") : 0;
  c.fpset_log2 = fpbits;
  c.mem_budget = membudget;
  static const char* strs[][2] = {{"Follower", "\"Follower\""}, {"Candidate", "\"Candidate\""},
                                  {"Leader", "\"Leader\""}, {"Nil", "\"Nil\""},
                                  {"RequestVoteRequest", "\"RequestVoteRequest\""},
                                  {"RequestVoteResponse", "\"RequestVoteResponse\""},
                                  {"AppendEntriesRequest", "\"AppendEntriesRequest\""},
                                  {"AppendEntriesResponse", "\"AppendEntriesResponse\""}};
  for (auto& p : strs) {
    auto it = cf.scalars.find(p[0]);
    if (it == cf.scalars.end() || it->second != p[1]) {
      printf("Error: constant %s must be bound to %s as in raft.cfg:8-15\n", p[0], p[1]);
      return 151;
    }
  }
  rtla_pred* preds = user_invs.empty() ? nullptr : load_predicates(&c, pred_file, user_invs);
  rtla_pred* audit_preds = user_audit.empty() ? nullptr : load_predicates(&c, pred_file, user_audit);
  rtla_pred* actions = cf.properties.empty() ? nullptr : load_actions(&c, pred_file, cf.properties);
  rtla_pred* audit_acts = audit_actions.empty() ? nullptr : load_actions(&c, pred_file, audit_actions);
  rtla_pred* constraint = user_cons.empty() ? nullptr : load_predicates(&c, pred_file, user_cons);
  if (constraint) {
    std::string line = "Constraining the search by: ";
    for (int k = 0; k < rtla_pred_count(constraint); k++) line += (k ? ", " : "") + pred_name(constraint, k);
    printf("%s.\n", line.c_str());
  }
  bool pred_violation = false;  // the violation reported is a predicate set's: its mask holds definition bits
  const rtla_pred* viol_set = nullptr;
  // user-defined invariants: the level just produced is audited in place (rtla_pred_frontier); then the action
  // properties on the steps out of it (rtla_pred_step_frontier), so every step out of every reachable in-model
  // state is checked before the next level is produced.  Between the two the user CONSTRAINT prunes the level
  // (the invariants see it whole, as TLC checks them on states it then discards; the steps are the kept rows'),
  // and the level's figures become the post-drop ones.
  auto check_level = [&](rtla_ctx* x, int st_level, rtla_level_stats& lv) -> int {
    if (st_level != RTLA_OK || lv.new_states == 0) return st_level;
    const rtla_pred* const sets[2] = {preds, actions};
    for (int q = 0; q < 2; q++) {
      const rtla_pred* const set = sets[q];
      if (q == 1 && constraint) {
        rtla_constrain_stats cs;
        const int rc = rtla_pred_constrain(x, constraint, &cs);
        if (rc < 0) return rc;
        lv.new_states = cs.kept;
        lv.distinct_total = cs.distinct_total;
        if (rc == RTLA_DONE) return rc;
      }
      if (!set) continue;
      const int rc = rtla_pred_is_step(set) ? rtla_pred_step_frontier(x, set, nullptr) : rtla_pred_frontier(x, set, nullptr);
      if (rc == RTLA_VIOLATION) { pred_violation = true; viol_set = set; }
      if (rc != RTLA_OK) return rc;
    }
    return st_level;
  };
  unsigned char comm_id[128];
  if (world > 1 && !rendezvous(rank, getenv("RTLA_RENDEZVOUS"), false, comm_id)) {
    fprintf(stderr, "Error: rank %d: RCCL rendezvous failed\n", rank);
    return 255;
  }
  rtla_ctx* ctx = nullptr;
  int st = rtla_open(&c, rank, world, world > 1 ? comm_id : nullptr, &ctx);
  if (st < 0) { printf("Error: %s\n", rtla_strerror(st)); return 255; }
  char info[1024];
  rtla_device_info(ctx, info, sizeof info);
  printf("Running breadth-first search Model-Checking with 128-bit fingerprints on %d GPU%s: %s\n", world,
         world > 1 ? "s (fingerprint-sharded, RCCL)" : "", info);
  printf("Starting... (%s)\n", now_str().c_str());
  printf("Computing initial states...\n");
  auto t0 = std::chrono::steady_clock::now();
  rtla_level_stats ls;
  memset(&ls, 0, sizeof ls);
  if (!recover_prefix.empty()) {
    st = rtla_recover(ctx, recover_prefix.c_str());
    if (st < 0) { printf("Error: cannot recover from %s: %s\n", recover_prefix.c_str(), rtla_strerror(st)); return 255; }
    printf("Recovering from checkpoint %s (completed).\n", recover_prefix.c_str());
  } else {
    st = rtla_init(ctx, &ls);
    printf("Finished computing initial states: 1 distinct state generated at %s.\n", now_str().c_str());
    st = check_level(ctx, st, ls);
  }
  auto last_progress = t0, last_ckpt = t0;
  // With several ranks the checkpoint (a collective) must be decided alike
  // everywhere: the clock is then the job's device time (the per-level
  // maximum over ranks, identical on every rank), not this rank's wall clock.
  double dev_s = 0, dev_ckpt = 0;
  // -bfs-levels K stops the search for what follows it: the walks, or the audit
  const bool stop_at_level = simulate || (audit && have_levels);
  while (st == RTLA_OK && !(stop_at_level && ls.level >= bfs_levels)) {
    st = rtla_step(ctx, &ls);
    if (st < 0) break;
    st = check_level(ctx, st, ls);
    if (st < 0) break;
    dev_s += ls.kernel_ms / 1e3;
    const double since = world > 1 ? dev_s - dev_ckpt
                                   : std::chrono::duration<double>(std::chrono::steady_clock::now() - last_ckpt).count();
    if (ckpt_minutes > 0 && st == RTLA_OK && since >= ckpt_minutes * 60) {
      dev_ckpt = dev_s;
      // in-process (no shell from a GPU-initialised process)
      std::error_code ec;
      if (ckpt_prefix.find('/') != std::string::npos)
        std::filesystem::create_directories(ckpt_prefix.substr(0, ckpt_prefix.rfind('/')), ec);
      printf("Checkpointing of run %s\n", ckpt_prefix.c_str());
      if (rtla_checkpoint(ctx, ckpt_prefix.c_str()) != RTLA_OK) printf("Warning: checkpoint failed\n");
      else printf("Checkpointing completed at (%s)\n", now_str().c_str());
      last_ckpt = std::chrono::steady_clock::now();
    }
    if (dump_levels)
      printf("  level %d: frontier %llu, new %llu, generated %llu, %.3f ms\n", ls.level,
             (unsigned long long)ls.frontier, (unsigned long long)ls.new_states, (unsigned long long)ls.generated,
             ls.seconds * 1e3);
    auto now = std::chrono::steady_clock::now();
    if (std::chrono::duration<double>(now - last_progress).count() >= 60.0 || st != RTLA_OK) {
      double mins = std::chrono::duration<double>(now - t0).count() / 60.0;
      printf("Progress(%d) at %s: %llu states generated (%.0f s/min), %llu distinct states found (%.0f ds/min), "
             "%llu states left on queue.\n",
             ls.level, now_str().c_str(), (unsigned long long)ls.generated_total, ls.generated_total / mins,
             (unsigned long long)ls.distinct_total, ls.distinct_total / mins,
             (unsigned long long)(st == RTLA_OK ? ls.new_states : 0));
      last_progress = now;
    }
  }
  double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  int exit_code = 0;
  // -audit after a search that ran out of capacity: the level last completed is still the frontier
  const bool audit_after_overflow = audit && st == RTLA_E_OVERFLOW;
  if (audit_after_overflow) {
    printf("Warning: %s (%s) while producing level %d; the search stops here.\n", rtla_strerror(st),
           ls.flags & RTLA_CAP_FRONTIER ? "frontier" : ls.flags & RTLA_CAP_FPSET ? "fingerprint set" : "row / outbox",
           ls.level);
    ls.level--;  // (the level that did not complete is dropped)
  } else if (st < 0) {
    printf("Error: %s\n", rtla_strerror(st));
    rtla_close(ctx);
    return 255;
  }
  // -audit: the BFS stopped (exhausted: the last non-empty level is gone, so there is nothing to audit)
  bool audited = false;
  if (audit && (st == RTLA_OK || audit_after_overflow)) {
    size_t nfront = 0;
    rtla_frontier(ctx, nullptr, 0, &nfront);
    if (audit_after_overflow) ls.new_states = nfront;  // still on the queue
    rtla_audit_stats as;
    memset(&as, 0, sizeof as);
    st = rtla_check_frontier(ctx, audit_mask, 0, &as);
    if (st < 0) {
      printf("Error: audit: %s\n", rtla_strerror(st));
      rtla_close(ctx);
      return 255;
    }
    audited = true;
    printf("Auditing the %llu states of BFS level %d: %.3f ms on the GPU.\n", (unsigned long long)as.audited,
           ls.level, as.kernel_ms);
    for (int b = 0; b < (int)(sizeof INVARIANTS / sizeof INVARIANTS[0]); b++)
      if (audit_mask & INVARIANTS[b].bit) {
        if (as.counts[b]) printf("Error: Invariant %s is violated by %llu of the %llu states.\n", INVARIANTS[b].name,
                                 (unsigned long long)as.counts[b], (unsigned long long)as.audited);
        else printf("Invariant %s holds in all %llu states.\n", INVARIANTS[b].name, (unsigned long long)as.audited);
      }
    if (audit_preds) {  // the names the predicate file defines, in the same form
      rtla_audit_stats ps;
      memset(&ps, 0, sizeof ps);
      const int pst = rtla_pred_frontier(ctx, audit_preds, &ps);
      if (pst < 0) {
        printf("Error: audit: %s\n", rtla_strerror(pst));
        rtla_close(ctx);
        return 255;
      }
      for (int k = 0; k < rtla_pred_count(audit_preds); k++) {
        if (ps.counts[k]) printf("Error: Invariant %s is violated by %llu of the %llu states.\n",
                                 pred_name(audit_preds, k).c_str(), (unsigned long long)ps.counts[k],
                                 (unsigned long long)ps.audited);
        else printf("Invariant %s holds in all %llu states.\n", pred_name(audit_preds, k).c_str(),
                    (unsigned long long)ps.audited);
      }
      if (pst == RTLA_VIOLATION) {
        st = pst;
        pred_violation = true;
        viol_set = audit_preds;
      } else if (st == RTLA_VIOLATION) {  // (the trace reported is the last audit's: the built-ins' again)
        st = rtla_check_frontier(ctx, audit_mask, 0, &as);
      }
    }
    if (audit_acts) {  // action definitions: the steps out of the level
      rtla_audit_stats ps;
      memset(&ps, 0, sizeof ps);
      const int pst = rtla_pred_step_frontier(ctx, audit_acts, &ps);
      if (pst < 0) {
        printf("Error: audit: %s\n", rtla_strerror(pst));
        rtla_close(ctx);
        return 255;
      }
      for (int k = 0; k < rtla_pred_count(audit_acts); k++) {
        if (ps.counts[k]) printf("Error: Action property %s is violated by %llu of the %llu steps.\n",
                                 pred_name(audit_acts, k).c_str(), (unsigned long long)ps.counts[k],
                                 (unsigned long long)ps.evaluated);
        else printf("Action property %s holds on all %llu steps.\n", pred_name(audit_acts, k).c_str(),
                    (unsigned long long)ps.evaluated);
      }
      if (pst == RTLA_VIOLATION && st != RTLA_VIOLATION) {  // (a violated invariant's trace comes first)
        st = pst;
        pred_violation = true;
        viol_set = audit_acts;
      } else if (st == RTLA_VIOLATION) {  // (the trace reported is the last audit's: run that one again)
        if (pred_violation) st = rtla_pred_frontier(ctx, audit_preds, nullptr);
        else st = rtla_check_frontier(ctx, audit_mask, 0, &as);
      }
    }
    secs =std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  } else if (audit && st == RTLA_DONE) {
    printf("Audit: the search is complete and its last level is empty; nothing to audit.\n");
  }
  // -simulate: the BFS stopped at level K with nothing found (a BFS that
  // finished or violated first is reported below as without -simulate)
  bool simulated = false, sim_with_sets = false;
  rtla_sim_pred_stats sps;  // the walks' violation when they carried the user's sets: three masks
  memset(&sps, 0, sizeof sps);
  if (simulate && st == RTLA_OK) {
    simulated = true;
    size_t nfront = 0;
    rtla_frontier(ctx, nullptr, 0, &nfront);
    printf("Running Random Simulation with seed %llu from the %zu states of BFS level %d: %llu walks of depth %d "
           "(walk ids %llu..%llu).\n",
           (unsigned long long)sim_seed, nfront, ls.level, (unsigned long long)sim_num, sim_depth,
           (unsigned long long)sim_first, (unsigned long long)(sim_first + sim_num - (sim_num ? 1 : 0)));
    rtla_sim_stats ss;
    memset(&ss, 0, sizeof ss);
    if (preds || actions) {  // the cfg's user INVARIANTs and PROPERTYs go into the walks: the sets check_level audits
      std::string line = "Checking in the walks:";
      const rtla_pred* sets[2] = {preds, actions};
      for (int q = 0; q < 2; q++) {
        if (!sets[q]) continue;
        line += q == 0 ? " invariants " : preds ? "; action properties " : " action properties ";
        for (int k = 0; k < rtla_pred_count(sets[q]); k++) line += (k ? ", " : "") + pred_name(sets[q], k);
      }
      printf("%s.\n", line.c_str());
      sim_with_sets = true;
      st = rtla_simulate_pred(ctx, sim_seed, sim_first, sim_num, sim_depth, preds, actions, nullptr, &ss, &sps);
    } else {
      st = rtla_simulate(ctx, sim_seed, sim_first, sim_num, sim_depth, nullptr, &ss);
    }
    if (st < 0) {
      printf("Error: %s\n", rtla_strerror(st));
      rtla_close(ctx);
      return 255;
    }
    printf("Simulation: %llu walks, %llu steps taken, %llu states generated, %llu stuck; %.3f s on the GPU: "
           "%.3g steps/s, %.3g generated/s.\n",
           (unsigned long long)ss.walks, (unsigned long long)ss.steps, (unsigned long long)ss.generated,
           (unsigned long long)ss.stuck, ss.kernel_ms / 1e3, ss.kernel_ms > 0 ? ss.steps / (ss.kernel_ms / 1e3) : 0.0,
           ss.kernel_ms > 0 ? ss.generated / (ss.kernel_ms / 1e3) : 0.0);
    if (st == RTLA_VIOLATION)
      printf("Walk %llu (start state %llu of level %d) violates at step %d; rerun it with -seed %llu -simulate "
             "num=1,first=%llu -depth %d -bfs-levels %d.\n",
             (unsigned long long)ss.viol_walk, (unsigned long long)(nfront ? ss.viol_walk % nfront : 0), ls.level,
             ss.viol_step, (unsigned long long)sim_seed, (unsigned long long)ss.viol_walk, ss.viol_step, ls.level);
    secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }
  int depth = 0;
  // depth = levels with new states; the last level returns new == 0 on DONE
  depth = st == RTLA_DONE ? ls.level - 1 : ls.level;
  if (st == RTLA_VIOLATION) {
    int32_t mask = 0, inm = 0;
    rtla_violation(ctx, &mask, &inm);
    if (simulated && sim_with_sets) {  // every false thing of the reported successor: built-ins first
      for (auto& i : INVARIANTS)
        if (sps.viol_inv_mask & i.bit) printf("Error: Invariant %s is violated.\n", i.name);
      for (int k = 0; preds && k < rtla_pred_count(preds); k++)
        if (sps.viol_state_mask >> k & 1) printf("Error: Invariant %s is violated.\n", pred_name(preds, k).c_str());
      for (int k = 0; actions && k < rtla_pred_count(actions); k++)
        if (sps.viol_step_mask >> k & 1)
          printf("Error: Action property %s is violated.\n", pred_name(actions, k).c_str());
    } else if (pred_violation) {
      for (int k = 0; k < rtla_pred_count(viol_set); k++)  // every false definition of the state, in file order
        if (mask >> k & 1)
          printf("Error: %s %s is violated.\n", rtla_pred_is_step(viol_set) ? "Action property" : "Invariant",
                 pred_name(viol_set, k).c_str());
    } else {
      for (auto& i : INVARIANTS)  // every violated name, in bit order
        if (mask & i.bit) printf("Error: Invariant %s is violated.\n", i.name);
    }
    printf("Error: The behavior up to this point is:\n");
    size_t n = 0;
    rtla_trace(ctx, nullptr, nullptr, 0, &n);
    int W = rtla_row_words(&c);
    std::vector<uint32_t> rows(n * W);
    std::vector<int32_t> labels(n);
    if (rtla_trace(ctx, rows.data(), labels.data(), n, &n) == RTLA_OK) {
      std::vector<char> buf(1 << 20);
      for (size_t k = 0; k < n; k++) {
        std::string lab = "Initial predicate";
        if (labels[k] >= 0) {
          char lb[256];
          rtla_action_name(&c, labels[k] & 0xffff, (labels[k] >> 16) & 0x7fff, lb, sizeof lb);
          lab = lb;
        }
        rtla_state_text(&c, rows.data() + k * W, buf.data(), buf.size());
        printf("State %zu: <%s>\n%s\n\n", k + 1, subst_names(lab, servers, values).c_str(),
               subst_names(buf.data(), servers, values).c_str());
      }
    }
    exit_code = 12;
  } else if (audited) {
    printf("Audit completed. No error has been found in the audited level (not an exhaustive search).\n");
  } else if (simulated) {
    printf("Simulation completed. No error has been found in %d BFS levels and the walks above "
           "(not an exhaustive search).\n", ls.level);
  } else {
    printf("Model checking completed. No error has been found.\n");
    printf("  Estimates of the probability that TLC did not check all reachable states\n"
           "  because two distinct states had the same fingerprint:\n"
           "  calculated (optimistic):  val = %.1E\n",
           // TLC's formula (distinct x (generated - distinct) / 2^64), kept so
           // tools that parse this line read the quantity TLC reports
           (double)ls.distinct_total * (double)(ls.generated_total - ls.distinct_total) / 1.8446744073709552e19);
    // this checker's own estimate: the set stores 63 key bits (fp.b | 1) at
    // a slot chosen by fp.a; a probe compares each generated state with ~2
    // random keys at the loads used
    printf("  rtla 63-bit-key estimate:  val = %.1E\n", (double)ls.generated_total * 2.0 / 9.223372036854775808e18);
  }
  if (coverage) {
    uint64_t g[16], d[16];
    rtla_coverage(ctx, g, d, 16);
    printf("The coverage statistics at %s\n", now_str().c_str());
    for (int k = 0; k < 16; k++) {
      if (k == 7) continue;
      printf("<%s of module raft>: %llu:%llu\n", COVER[k], (unsigned long long)d[k], (unsigned long long)g[k]);
    }
    printf("End of statistics.\n");
  }
  printf("%llu states generated, %llu distinct states found, %llu states left on queue.\n",
         (unsigned long long)ls.generated_total, (unsigned long long)ls.distinct_total,
         (unsigned long long)(simulated || audited ? ls.new_states : 0));
  if (audited) printf("The depth of the breadth-first search before the audit is %d.\n", depth);
  else if (simulated) printf("The depth of the breadth-first search before the simulation is %d.\n", depth);
  else printf("The depth of the complete state graph search is %d.\n", depth);
  printf("Finished in %.2fs at (%s)\n", secs, now_str().c_str());
  rtla_close(ctx);
  return exit_code;
}
