// rtla_cli.cpp -- TLC-compatible command line over librtla.so.
//
// Replaces the reference's invocation (reference README.md:5, raft.cfg:1-15, .vscode/settings.json:5):
//     java tlc2.TLC [-workers W] [-coverage M] -config raft.cfg raft.tla
// with
//     rtla [-workers W] [-coverage M] [-gpus G] [-fpbits B] -config X.cfg SPEC.tla
// and TLC's simulation mode (-simulate [num=N] -depth D -seed S) with
//     rtla -simulate [num=N[,first=F]] [-depth D] [-seed S] [-bfs-levels K] -config X.cfg SPEC.tla
// and an audit of the last BFS level for invariants the search did not carry
//     rtla -audit Name[,Name...] [-bfs-levels K] -config X.cfg SPEC.tla
// (after the BFS stops -- exhausted, out of capacity, or after K levels).  TLC's "add an operator to MC.tla and
// name it under INVARIANT" is
//     rtla -predicates FILE -config X.cfg SPEC.tla
// where INVARIANT(S), PROPERTY / PROPERTIES, CONSTRAINT(S) and -audit may name definitions of FILE (DESIGN.md
// sections 13 to 16).  What each option means is usage(), below.
//
// SPEC.tla is either the reference's raft.tla (sha256 checked: the semantics are compiled into the kernels, not
// parsed) or a wrapper module that EXTENDS raft and defines the model-checking operators of specs/MC.tla
// (StateConstraint, NoTwoLeaders, ElectionSafety, LogMatching, StateMachineSafety, LeaderCompleteness); the
// raft.tla next to it is then hash-checked.  Output follows TLC's stdout lines.  Exit codes: 0 = no error,
// 12 = safety violation, 150/151 = spec/config errors, 255 = other errors (TLC's ExitStatus values as we
// understand them; not verified against a live TLC here).
//
// main runs the stages of DESIGN.md section 9: parse_args, check_spec, resolve, load_sets, then with a device search,
// audit_level, simulate, report; each returns GO_ON or the exit code.  The text code is rtla_cli_text.h.
#include <errno.h>
#include <signal.h>
#include <spawn.h>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>
#include <sys/wait.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <filesystem>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/rtla.h"
#include "rtla_cli_text.h"

extern char** environ;

static const char* RAFT_SHA256 = "683a120af29e3e5a805e291f756229d65914f8fb73dddd8c78bafef50a6f6b81";

namespace {

std::string now_str() {
  time_t t = time(nullptr);
  char b[64];
  strftime(b, sizeof b, "%Y-%m-%d %H:%M:%S", localtime(&t));
  return b;
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

const int GO_ON = -1;  // a stage before the device: no exit code yet
typedef unsigned long long ull;  // (printf's %llu)

struct Options {
  std::string cfgpath, spec, raft_opt, pred_file;  // (-predicates FILE: what the cfg and -audit may name)
  int coverage = 0, gpus = 1, fpbits = 0;
  bool dump_levels = false, skip_spec_check = false;
  uint64_t membudget = 0;
  double ckpt_minutes = 0;  // TLC -checkpoint <minutes> / -recover <path> (the reference's .gitignore:2 states/ dir)
  std::string ckpt_prefix = "states/ckpt", recover_prefix;
  // TLC -simulate [num=N] / -depth D / -seed S, here from the states of BFS level -bfs-levels K
  bool simulate = false, have_seed = false, have_levels = false;
  uint64_t sim_num = 1000000, sim_first = 0, sim_seed = 0;
  int sim_depth = 100, bfs_levels = 1;
  std::vector<std::string> audit_names;  // -audit Name[,Name...]: evaluated over the last BFS level
  bool audit = false;
  int rank = 0, world = 1;  // this process among the -gpus ranks
};

// An error line; returns `code`, the exit code that goes with it.  A command line refused is told on stderr, as
// usage() is; from the banner on the lines go to stdout, where TLC prints its own.
FILE* errors = stderr;
__attribute__((format(printf, 2, 3))) int error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  fprintf(errors, "Error: ");
  vfprintf(errors, fmt, ap);
  fprintf(errors, "\n");
  va_end(ap);
  return code;
}

int parse_args(int argc, char** argv, Options* o) {
  for (int i = 1; i < argc; i++) {
    std::string a = argv[i];
    auto next = [&]() -> std::string {
      if (i + 1 >= argc) { usage(); exit(255); }
      return argv[++i];
    };
    if (a == "-config") o->cfgpath = next();
    else if (a == "-coverage") o->coverage = atoi(next().c_str());
    else if (a == "-workers") next();  // (TLC's; the GPU has its own)
    else if (a == "-gpus") o->gpus = atoi(next().c_str());
    else if (a == "-fpbits") o->fpbits = atoi(next().c_str());
    else if (a == "-membudget") o->membudget = strtoull(next().c_str(), nullptr, 10);
    else if (a == "-dump-levels") o->dump_levels = true;
    else if (a == "-raft") o->raft_opt = next();
    else if (a == "-skip-spec-check") o->skip_spec_check = true;
    else if (a == "-checkpoint") o->ckpt_minutes = atof(next().c_str());
    else if (a == "-checkpointdir") o->ckpt_prefix = next();
    else if (a == "-recover") o->recover_prefix = next();
    else if (a == "-simulate") {
      o->simulate = true;
      if (i + 1 < argc && (!strncmp(argv[i + 1], "num=", 4) || !strncmp(argv[i + 1], "first=", 6))) {
        std::stringstream opts(argv[++i]);
        for (std::string kv; std::getline(opts, kv, ',');) {
          if (kv.compare(0, 4, "num=") == 0) o->sim_num = strtoull(kv.c_str() + 4, nullptr, 10);
          else if (kv.compare(0, 6, "first=") == 0) o->sim_first = strtoull(kv.c_str() + 6, nullptr, 10);
          else return error(255, "-simulate: unknown option %s", kv.c_str());
        }
      }
    }
    else if (a == "-depth") o->sim_depth = atoi(next().c_str());
    else if (a == "-seed") { o->sim_seed = strtoull(next().c_str(), nullptr, 10); o->have_seed = true; }
    else if (a == "-bfs-levels") { o->bfs_levels = atoi(next().c_str()); o->have_levels = true; }
    else if (a == "-audit") {
      o->audit = true;
      std::stringstream names(next());
      for (std::string nm; std::getline(names, nm, ',');)
        if (!nm.empty()) o->audit_names.push_back(nm);
    }
    else if (a == "-predicates") o->pred_file = next();
    else if (a == "-h" || a == "-help") { usage(); return 0; }
    else if (!a.empty() && a[0] == '-') return error(255, "unsupported option %s", a.c_str());
    else o->spec = a;
  }
  if (o->gpus < 1) { usage(); return 255; }
  if (o->simulate && o->gpus > 1)
    return error(255, "-simulate runs on one GPU; split the walks over processes instead "
                  "(-simulate num=N,first=F with disjoint ranges and the same -seed)");
  if (o->audit && (o->gpus > 1 || o->simulate || o->audit_names.empty()))
    return error(255, "-audit names at least one invariant and runs on one GPU, without -simulate");
  if (!o->pred_file.empty() && o->gpus > 1)
    return error(255, "-predicates checks user-defined invariants on one GPU (a single shard); use -gpus 1");
  if (o->audit && o->bfs_levels < 1) return error(255, "-bfs-levels must be at least 1");
  if (o->simulate && (o->sim_depth < 0 || o->sim_depth > 65535 || o->bfs_levels < 1))
    return error(255, "-depth must be 0..65535 and -bfs-levels at least 1");
  if (o->simulate && !o->have_seed)
    o->sim_seed = (uint64_t)time(nullptr) ^ (uint64_t)getpid() << 32;  // printed, as TLC does
  return GO_ON;
}

// --- spec identity: the semantics are compiled in, so raft.tla is checked by hash; *wrapper: SPEC.tla is a
// module that EXTENDS raft and defines the operators of specs/MC.tla
int check_spec(const Options& o, bool* wrapper) {
  bool ok = false;
  const std::string& spec = o.spec;
  const std::string spec_text = read_file(spec, &ok);
  if (!ok) return error(150, "cannot read %s", spec.c_str());
  std::string dir = spec.find('/') == std::string::npos ? "." : spec.substr(0, spec.rfind('/'));
  std::string base = spec.substr(spec.find('/') == std::string::npos ? 0 : spec.rfind('/') + 1);
  *wrapper = base != "raft.tla";
  std::string raft_path = !o.raft_opt.empty() ? o.raft_opt : *wrapper ? dir + "/raft.tla" : spec;
  std::string raft_text = raft_path == spec ? spec_text : read_file(raft_path, &ok);
  if (!ok && !o.skip_spec_check)
    return error(150, "%s EXTENDS raft but %s is missing (give -raft PATH)", spec.c_str(), raft_path.c_str());
  std::string h = o.skip_spec_check ? std::string(RAFT_SHA256) : Sha256().digest(raft_text);
  if (o.skip_spec_check) printf("Warning: -skip-spec-check: the identity of raft.tla is NOT verified\n");
  if (h != RAFT_SHA256)
    return error(150, "%s has sha256 %s; this checker compiles the semantics of raft.tla %s only.",
                 raft_path.c_str(), h.c_str(), RAFT_SHA256);
  if (*wrapper && spec_text.find("EXTENDS raft") == std::string::npos)
    return error(150, "%s does not EXTEND raft", spec.c_str());
  printf("Parsing file %s (raft.tla sha256 %.12s... verified)\n", spec.c_str(), h.c_str());
  return GO_ON;
}

// What the cfg and the predicate file ask for: the configuration, the model values' names, a list of names per set.
struct Model {
  rtla_cfg c{};
  std::vector<std::string> servers, values;
  int32_t audit_mask = 0;               // -audit's built-in names
  std::vector<std::string> user_invs;   // INVARIANT names that are not built in
  std::vector<std::string> user_audit;  // -audit names that are not built in
  std::vector<std::string> properties;  // PROPERTY names: action definitions
  std::vector<std::string> audit_acts;  // -audit names that are action definitions
  std::vector<std::string> user_cons;   // CONSTRAINT names beside StateConstraint: state definitions
};

int undefined(const char* what, const std::string& name) {
  return error(150, "The %s %s specified in the configuration file is not defined in the specification.", what,
               name.c_str());
}

// INVARIANT and -audit names: the built-in ones into *mask (raft.tla defines none of the MC operators: only a
// wrapper has them and StateConstraint); with a predicate file every other one into *user (load_set reports what
// the file does not define), -audit's action definitions into *acts.
int sort_invariants(const std::vector<std::string>& names, bool wrapper, const PredFile& pf, int32_t* mask,
                    std::vector<std::string>* user, std::vector<std::string>* acts) {
  for (auto& inv : names) {
    const int32_t bit = wrapper ? invariant_bit(inv) : 0;
    if (acts && pf.defines(inv, true)) acts->push_back(inv);
    else if (!pf.path.empty() && !bit && !(wrapper && inv == "StateConstraint")) user->push_back(inv);
    else if (!bit) return undefined("invariant", inv);
    else *mask |= bit;
  }
  return GO_ON;
}

// The CONSTANTS of raft.cfg: the two sets, the bounds of StateConstraint, and the strings as raft.cfg binds them.
int bind_constants(const Options& o, const CfgFile& cf, Model* m) {
  for (const char* n : {"Server", "Value"})
    if (!cf.sets.count(n)) return error(151, "constant %s is not assigned a set in %s", n, o.cfgpath.c_str());
  for (const char* n : {"MaxTerm", "MaxLogLen", "MaxCopies"})
    if (!cf.scalars.count(n)) return error(151, "constant %s is not assigned in %s", n, o.cfgpath.c_str());
  auto bound = [&](const char* n) { return cf.scalars.count(n) ? atoi(cf.scalars.at(n).c_str()) : 0; };
  m->servers = cf.sets.at("Server");
  m->values = cf.sets.at("Value");
  m->c.n_server = (int)m->servers.size();
  m->c.n_value = (int)m->values.size();
  m->c.max_term = bound("MaxTerm");
  m->c.max_log = bound("MaxLogLen");
  m->c.max_copies = bound("MaxCopies");
  m->c.max_msgs = bound("MaxInFlight");  // (optional: 0 when the cfg has none)
  m->c.fpset_log2 = o.fpbits;
  m->c.mem_budget = o.membudget;
  for (std::string s : {"Follower", "Candidate", "Leader", "Nil", "RequestVoteRequest", "RequestVoteResponse",
                        "AppendEntriesRequest", "AppendEntriesResponse"}) {
    auto it = cf.scalars.find(s);
    const std::string want = '"' + s + '"';
    if (it == cf.scalars.end() || it->second != want)
      return error(151, "constant %s must be bound to %s as in raft.cfg:8-15", s.c_str(), want.c_str());
  }
  return GO_ON;
}

// The order of the refusals is the program's behaviour: PROPERTY, SPECIFICATION, INVARIANT names, -audit names,
// CONSTRAINT names, -simulate with a constraint, SYMMETRY, no StateConstraint, constants, string constants.
int resolve(const Options& o, const CfgFile& cf, const PredFile& pf, bool wrapper, Model* m) {
  // PROPERTY names are the action definitions of the -predicates file; anything else is refused as ever
  for (auto& p : cf.properties)
    if (!pf.defines(p, true))
      return error(151, "%s: %s is not supported by this checker", o.cfgpath.c_str(), cf.property_keyword.c_str());
  m->properties = cf.properties;
  if (!cf.specification.empty() && cf.specification != "Spec")
    return error(151, "SPECIFICATION %s: only Spec (raft.tla:469) is supported", cf.specification.c_str());
  int rc = sort_invariants(cf.invariants, wrapper, pf, &m->c.inv_mask, &m->user_invs, nullptr);
  if (rc == GO_ON) rc = sort_invariants(o.audit_names, wrapper, pf, &m->audit_mask, &m->user_audit, &m->audit_acts);
  if (rc != GO_ON) return rc;
  // CONSTRAINT names StateConstraint (the compiled-in bounds); any further name is a state definition of the
  // -predicates file, and prunes every level on the GPU (rtla_pred_constrain)
  bool built_in_constraint = false;
  for (auto& k : cf.constraints) {
    if (wrapper && k == "StateConstraint") { built_in_constraint = true; continue; }
    if (pf.defines(k, true))
      return error(150, "The constraint %s is an action definition; a CONSTRAINT is a state predicate "
                        "(ACTION_CONSTRAINT is not supported by this checker).", k.c_str());
    if (!pf.defines(k, false)) return undefined("constraint", k);
    if (std::find(m->user_cons.begin(), m->user_cons.end(), k) == m->user_cons.end()) m->user_cons.push_back(k);
  }
  if (!m->user_cons.empty() && o.simulate)
    return error(150, "-simulate with a user-defined CONSTRAINT (%s) is not supported: the random walks do not "
                      "honour constraints, and are not run unconstrained in their place.", m->user_cons[0].c_str());
  if (!cf.symmetry.empty() && (!wrapper || cf.symmetry != "Perms")) return undefined("symmetry", cf.symmetry);
  m->c.symmetry = !cf.symmetry.empty();  // Perms == Permutations(Server) (specs/MC.tla)
  if (!built_in_constraint)
    return error(151, "no CONSTRAINT: raft.tla's state space is infinite (Timeout raft.tla:180 and Send "
                      "raft.tla:106-110 are unbounded); add CONSTRAINT StateConstraint from specs/MC.tla.");
  return bind_constants(o, cf, m);
}

struct PredFree { void operator()(rtla_pred* p) const { rtla_pred_free(p); } };
struct CtxClose { void operator()(rtla_ctx* x) const { rtla_close(x); } };
using PredPtr = std::unique_ptr<rtla_pred, PredFree>;
using CtxPtr = std::unique_ptr<rtla_ctx, CtxClose>;

// The compiled sets of the predicate file (null: nothing named).  check_level runs preds, constraint, actions.
struct Sets {
  PredPtr preds, actions;            // the cfg's user INVARIANTs / PROPERTYs: every level, and the walks
  PredPtr audit_preds, audit_acts;   // -audit's: the last level
  PredPtr constraint;                // the cfg's user CONSTRAINTs: prune every level
};

std::string pred_name(const rtla_pred* p, int k) {
  char buf[256] = "";
  rtla_pred_name(p, k, buf, sizeof buf);
  return buf;
}
std::string pred_names(const rtla_pred* p) {
  std::string s;
  for (int k = 0; k < rtla_pred_count(p); k++) s += (k ? ", " : "") + pred_name(p, k);
  return s;
}

// The definitions `names` of the predicate file, compiled: a step set of action definitions (the caller has checked
// the names), or a state set, which first compiles all state definitions of the file: an error in one nobody
// named is reported too, and a name is looked up among them.
int load_set(const Model& m, const PredFile& pf, const std::vector<std::string>& names, bool step, PredPtr* out) {
  if (names.empty()) return GO_ON;
  if (!pf.readable) return error(150, "cannot read the predicate file %s", pf.path.c_str());
  auto compile = [&](const std::vector<std::string>& keep, PredPtr* set, bool fallback) {
    char err[512];
    rtla_pred* p = nullptr;
    const std::string text = select_definitions(pf, keep, !step);
    if ((step ? rtla_pred_compile_step : rtla_pred_compile)(&m.c, text.c_str(), &p, err, sizeof err) != RTLA_OK)
      return error(150, "%s:%s", pf.path.c_str(),
                   err[0] || !fallback ? err : " the configuration is outside the row format");
    set->reset(p);
    return GO_ON;
  };
  if (!step) {
    PredPtr all;
    if (compile(definitions_of_kind(pf, false), &all, true) != GO_ON) return 150;
    for (auto& nm : names) {
      bool found = false;
      for (int k = 0; k < rtla_pred_count(all.get()); k++) found |= nm == pred_name(all.get(), k);
      if (!found) return undefined("invariant", nm);
    }
  }
  return compile(names, out, step);
}

int load_sets(const Model& m, const PredFile& pf, Sets* s) {
  int rc = load_set(m, pf, m.user_invs, false, &s->preds);
  if (rc == GO_ON) rc = load_set(m, pf, m.user_audit, false, &s->audit_preds);
  if (rc == GO_ON) rc = load_set(m, pf, m.properties, true, &s->actions);
  if (rc == GO_ON) rc = load_set(m, pf, m.audit_acts, true, &s->audit_acts);
  if (rc == GO_ON) rc = load_set(m, pf, m.user_cons, false, &s->constraint);
  if (rc == GO_ON && s->constraint)
    printf("Constraining the search by: %s.\n", pred_names(s->constraint.get()).c_str());
  return rc;
}

const char* COVER[] = {"Restart", "Timeout", "RequestVote", "BecomeLeader", "ClientRequest",
                       "AdvanceCommitIndex", "AppendEntries", "Receive", "DuplicateMessage", "DropMessage",
                       "UpdateTerm", "HandleRequestVoteRequest", "HandleRequestVoteResponse",
                       "HandleAppendEntriesRequest", "HandleAppendEntriesResponse", "DropStaleResponse"};

// Whose violation is reported: the stage that got RTLA_VIOLATION says so, report prints by it.
struct Violation {
  enum Source { NONE, BUILT_IN, SET, WALKS } source = NONE;
  const rtla_pred* set = nullptr;  // SET: rtla_violation's mask holds this set's definition bits
  rtla_sim_pred_stats walk{};      // WALKS (walks that carried the user's sets): three masks
};
struct Run {  // what the stages after rtla_open share; each returns GO_ON, or 255 once it has printed the error
  rtla_ctx* ctx = nullptr;
  std::chrono::steady_clock::time_point t0;
  rtla_level_stats ls{};    // the level last produced
  int st = RTLA_OK;         // the library's last verdict
  bool audited = false, simulated = false;
  Violation viol;
  double secs = 0;
  void stop_clock() { secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
};

int run_set(rtla_ctx* x, const rtla_pred* set, rtla_audit_stats* out) {
  return rtla_pred_is_step(set) ? rtla_pred_step_frontier(x, set, out) : rtla_pred_frontier(x, set, out);
}

// The level just produced, checked in place: the user's invariants over the whole level (as TLC checks them on
// states it then discards), then the user CONSTRAINT prunes it and the level's figures become the post-drop ones,
// then the action properties on the steps out of the kept rows, before the next level is produced.
int check_level(rtla_ctx* x, const Sets& s, int st_level, rtla_level_stats* lv, Violation* v) {
  if (st_level != RTLA_OK || lv->new_states == 0) return st_level;
  auto check = [&](const rtla_pred* set) {
    const int rc = set ? run_set(x, set, nullptr) : RTLA_OK;
    if (rc == RTLA_VIOLATION) *v = {Violation::SET, set, {}};
    return rc;
  };
  if (const int rc = check(s.preds.get()); rc != RTLA_OK) return rc;
  if (s.constraint) {
    rtla_constrain_stats cs;
    const int rc = rtla_pred_constrain(x, s.constraint.get(), &cs);
    if (rc < 0) return rc;
    lv->new_states = cs.kept;
    lv->distinct_total = cs.distinct_total;
    if (rc == RTLA_DONE) return rc;
  }
  if (const int rc = check(s.actions.get()); rc != RTLA_OK) return rc;
  return st_level;
}

// The breadth-first search: until it is complete, violated, failed, or (for the walks or the audit) at level K.
int search(const Options& o, const Sets& sets, Run* r) {
  rtla_level_stats& ls = r->ls;
  int& st = r->st;
  auto checked = [&](int st_level) {  // a level was produced: the search's own verdict, then the user's sets
    if (st_level == RTLA_VIOLATION) r->viol.source = Violation::BUILT_IN;
    return check_level(r->ctx, sets, st_level, &ls, &r->viol);
  };
  if (!o.recover_prefix.empty()) {
    st = rtla_recover(r->ctx, o.recover_prefix.c_str());
    if (st < 0) return error(255, "cannot recover from %s: %s", o.recover_prefix.c_str(), rtla_strerror(st));
    printf("Recovering from checkpoint %s (completed).\n", o.recover_prefix.c_str());
  } else {
    st = rtla_init(r->ctx, &ls);
    printf("Finished computing initial states: 1 distinct state generated at %s.\n", now_str().c_str());
    st = checked(st);
  }
  auto last_progress = r->t0, last_ckpt = r->t0;
  // With several ranks the checkpoint (a collective) must be decided alike
  // everywhere: the clock is then the job's device time (the per-level
  // maximum over ranks, identical on every rank), not this rank's wall clock.
  double dev_s = 0, dev_ckpt = 0;
  // -bfs-levels K stops the search for what follows it: the walks, or the audit
  const bool stop_at_level = o.simulate || (o.audit && o.have_levels);
  while (st == RTLA_OK && !(stop_at_level && ls.level >= o.bfs_levels)) {
    st = checked(rtla_step(r->ctx, &ls));
    if (st < 0) break;
    dev_s += ls.kernel_ms / 1e3;
    const double since = o.world > 1 ? dev_s - dev_ckpt
                                     : std::chrono::duration<double>(std::chrono::steady_clock::now() - last_ckpt).count();
    if (o.ckpt_minutes > 0 && st == RTLA_OK && since >= o.ckpt_minutes * 60) {
      dev_ckpt = dev_s;
      std::error_code ec;  // in-process (no shell from a GPU-initialised process)
      if (o.ckpt_prefix.find('/') != std::string::npos)
        std::filesystem::create_directories(o.ckpt_prefix.substr(0, o.ckpt_prefix.rfind('/')), ec);
      printf("Checkpointing of run %s\n", o.ckpt_prefix.c_str());
      if (rtla_checkpoint(r->ctx, o.ckpt_prefix.c_str()) != RTLA_OK) printf("Warning: checkpoint failed\n");
      else printf("Checkpointing completed at (%s)\n", now_str().c_str());
      last_ckpt = std::chrono::steady_clock::now();
    }
    if (o.dump_levels)
      printf("  level %d: frontier %llu, new %llu, generated %llu, %.3f ms\n", ls.level,
             (ull)ls.frontier, (ull)ls.new_states, (ull)ls.generated, ls.seconds * 1e3);
    auto now = std::chrono::steady_clock::now();
    if (std::chrono::duration<double>(now - last_progress).count() >= 60.0 || st != RTLA_OK) {
      double mins = std::chrono::duration<double>(now - r->t0).count() / 60.0;
      printf("Progress(%d) at %s: %llu states generated (%.0f s/min), %llu distinct states found (%.0f ds/min), "
             "%llu states left on queue.\n",
             ls.level, now_str().c_str(), (ull)ls.generated_total, ls.generated_total / mins,
             (ull)ls.distinct_total, ls.distinct_total / mins, (ull)(st == RTLA_OK ? ls.new_states : 0));
      last_progress = now;
    }
  }
  r->stop_clock();
  if (o.audit && st == RTLA_E_OVERFLOW) {  // the level last completed is still the frontier: it is audited
    printf("Warning: %s (%s) while producing level %d; the search stops here.\n", rtla_strerror(st),
           ls.flags & RTLA_CAP_FRONTIER ? "frontier" : ls.flags & RTLA_CAP_FPSET ? "fingerprint set" : "row / outbox",
           ls.level);
    ls.level--;  // (the level that did not complete is dropped)
    return GO_ON;
  }
  return st < 0 ? error(255, "%s", rtla_strerror(st)) : GO_ON;
}

void audit_line(bool step, const std::string& name, uint64_t bad, uint64_t of) {
  const char* noun = step ? "Action property" : "Invariant";
  const char* unit = step ? "steps" : "states";
  if (bad) printf("Error: %s %s is violated by %llu of the %llu %s.\n", noun, name.c_str(), (ull)bad, (ull)of, unit);
  else printf("%s %s holds %s all %llu %s.\n", noun, name.c_str(), step ? "on" : "in", (ull)of, unit);
}

// One compiled set over the last level (an action set: over the steps out of it), a line per definition.
int audit_set(rtla_ctx* x, const rtla_pred* set) {
  rtla_audit_stats ps{};
  const int rc = run_set(x, set, &ps);
  const bool step = rtla_pred_is_step(set);
  for (int k = 0; rc >= 0 && k < rtla_pred_count(set); k++)
    audit_line(step, pred_name(set, k), ps.counts[k], step ? ps.evaluated : ps.audited);
  return rc;
}

// -audit: the BFS stopped; the built-in invariants (always), the user's state set, the user's action set over the
// level last produced.  Whose violation is reported is decided after all have run: states, built-ins, actions.
// The library reports the trace of the last pass that ran, so the winner runs once more unless it was the last.
int audit_level(const Model& m, const Sets& sets, Run* r) {
  if (r->st == RTLA_DONE)  // (exhausted: the last non-empty level is gone)
    printf("Audit: the search is complete and its last level is empty; nothing to audit.\n");
  const bool overflowed = r->st == RTLA_E_OVERFLOW;  // (search went on for us: the level before is still the frontier)
  if (r->st != RTLA_OK && !overflowed) return GO_ON;
  size_t nfront = 0;
  rtla_frontier(r->ctx, nullptr, 0, &nfront);
  if (overflowed) r->ls.new_states = nfront;  // still on the queue
  enum { BUILT_IN, STATES, STEPS, PASSES };
  const rtla_pred* const user[PASSES] = {nullptr, sets.audit_preds.get(), sets.audit_acts.get()};
  int found[PASSES] = {RTLA_OK, RTLA_OK, RTLA_OK}, last = BUILT_IN;
  rtla_audit_stats as{};
  found[BUILT_IN] = rtla_check_frontier(r->ctx, m.audit_mask, 0, &as);
  if (found[BUILT_IN] < 0) return error(255, "audit: %s", rtla_strerror(found[BUILT_IN]));
  r->audited = true;
  printf("Auditing the %llu states of BFS level %d: %.3f ms on the GPU.\n", (ull)as.audited, r->ls.level,
         as.kernel_ms);
  for (int b = 0; b < (int)(sizeof INVARIANTS / sizeof INVARIANTS[0]); b++)
    if (m.audit_mask & INVARIANTS[b].bit) audit_line(false, INVARIANTS[b].name, as.counts[b], as.audited);
  for (int q = STATES; q < PASSES; q++) {
    if (!user[q]) continue;
    found[q] = audit_set(r->ctx, user[q]);
    if (found[q] < 0) return error(255, "audit: %s", rtla_strerror(found[q]));
    last = q;
  }
  const int winner = found[STATES] == RTLA_VIOLATION ? STATES : found[BUILT_IN] == RTLA_VIOLATION ? BUILT_IN
                     : found[STEPS] == RTLA_VIOLATION ? STEPS : PASSES;
  r->st = winner == PASSES ? RTLA_OK : RTLA_VIOLATION;
  if (winner != PASSES && winner != last)
    r->st = user[winner] ? run_set(r->ctx, user[winner], nullptr) : rtla_check_frontier(r->ctx, m.audit_mask, 0, &as);
  if (winner != PASSES) r->viol = {user[winner] ? Violation::SET : Violation::BUILT_IN, user[winner], {}};
  r->stop_clock();
  return GO_ON;
}

// -simulate: the BFS stopped at level K with nothing found; the walks carry the sets check_level audits.
int simulate(const Options& o, const Sets& sets, Run* r) {
  r->simulated = true;
  size_t nfront = 0;
  rtla_frontier(r->ctx, nullptr, 0, &nfront);
  printf("Running Random Simulation with seed %llu from the %zu states of BFS level %d: %llu walks of depth %d "
         "(walk ids %llu..%llu).\n",
         (ull)o.sim_seed, nfront, r->ls.level, (ull)o.sim_num, o.sim_depth, (ull)o.sim_first,
         (ull)(o.sim_first + o.sim_num - (o.sim_num ? 1 : 0)));
  rtla_sim_stats ss{};
  const rtla_pred *preds = sets.preds.get(), *actions = sets.actions.get();
  if (preds || actions) {
    std::string line = "Checking in the walks:";
    if (preds) line += " invariants " + pred_names(preds);
    if (actions) line += (preds ? "; action properties " : " action properties ") + pred_names(actions);
    printf("%s.\n", line.c_str());
    r->viol.source = Violation::WALKS;
    r->st = rtla_simulate_pred(r->ctx, o.sim_seed, o.sim_first, o.sim_num, o.sim_depth, preds, actions, nullptr, &ss,
                               &r->viol.walk);
  } else {
    r->viol.source = Violation::BUILT_IN;
    r->st = rtla_simulate(r->ctx, o.sim_seed, o.sim_first, o.sim_num, o.sim_depth, nullptr, &ss);
  }
  if (r->st < 0) return error(255, "%s", rtla_strerror(r->st));
  printf("Simulation: %llu walks, %llu steps taken, %llu states generated, %llu stuck; %.3f s on the GPU: "
         "%.3g steps/s, %.3g generated/s.\n",
         (ull)ss.walks, (ull)ss.steps, (ull)ss.generated, (ull)ss.stuck, ss.kernel_ms / 1e3,
         ss.kernel_ms > 0 ? ss.steps / (ss.kernel_ms / 1e3) : 0.0,
         ss.kernel_ms > 0 ? ss.generated / (ss.kernel_ms / 1e3) : 0.0);
  if (r->st == RTLA_VIOLATION)
    printf("Walk %llu (start state %llu of level %d) violates at step %d; rerun it with -seed %llu -simulate "
           "num=1,first=%llu -depth %d -bfs-levels %d.\n",
           (ull)ss.viol_walk, (ull)(nfront ? ss.viol_walk % nfront : 0), r->ls.level, ss.viol_step,
           (ull)o.sim_seed, (ull)ss.viol_walk, ss.viol_step, r->ls.level);
  r->stop_clock();
  return GO_ON;
}

// Every violated name of the reported state or step, then the behaviour that leads to it.
void report_violation(const Model& m, const Sets& sets, const Run& r) {
  int32_t mask = 0, inm = 0;
  rtla_violation(r.ctx, &mask, &inm);
  auto of_set = [](const rtla_pred* set, uint32_t bits) {  // every false definition, in file order
    for (int k = 0; set && k < rtla_pred_count(set); k++)
      if (bits >> k & 1)
        printf("Error: %s %s is violated.\n", rtla_pred_is_step(set) ? "Action property" : "Invariant",
               pred_name(set, k).c_str());
  };
  const Violation& v = r.viol;
  if (v.source != Violation::SET)  // every violated built-in name, in bit order
    for (auto& i : INVARIANTS)
      if ((v.source == Violation::WALKS ? v.walk.viol_inv_mask : mask) & i.bit)
        printf("Error: Invariant %s is violated.\n", i.name);
  if (v.source == Violation::WALKS) {  // every false thing of the reported successor: built-ins first
    of_set(sets.preds.get(), v.walk.viol_state_mask);
    of_set(sets.actions.get(), v.walk.viol_step_mask);
  } else if (v.source == Violation::SET) {
    of_set(v.set, mask);
  }
  printf("Error: The behavior up to this point is:\n");
  size_t n = 0;
  rtla_trace(r.ctx, nullptr, nullptr, 0, &n);
  int W = rtla_row_words(&m.c);
  std::vector<uint32_t> rows(n * W);
  std::vector<int32_t> labels(n);
  if (rtla_trace(r.ctx, rows.data(), labels.data(), n, &n) != RTLA_OK) return;
  std::vector<char> buf(1 << 20);
  for (size_t k = 0; k < n; k++) {
    std::string lab = "Initial predicate";
    if (labels[k] >= 0) {
      char lb[256];
      rtla_action_name(&m.c, labels[k] & 0xffff, (labels[k] >> 16) & 0x7fff, lb, sizeof lb);
      lab = lb;
    }
    rtla_state_text(&m.c, rows.data() + k * W, buf.data(), buf.size());
    printf("State %zu: <%s>\n%s\n\n", k + 1, subst_names(lab, m.servers, m.values).c_str(),
           subst_names(buf.data(), m.servers, m.values).c_str());
  }
}

// The verdict in TLC's lines, the coverage, the totals; returns the exit code.
int report(const Options& o, const Model& m, const Sets& sets, const Run& r) {
  const rtla_level_stats& ls = r.ls;
  // depth = levels with new states; the last level returns new == 0 on DONE
  const int depth = r.st == RTLA_DONE ? ls.level - 1 : ls.level;
  if (r.st == RTLA_VIOLATION) {
    report_violation(m, sets, r);
  } else if (r.audited) {
    printf("Audit completed. No error has been found in the audited level (not an exhaustive search).\n");
  } else if (r.simulated) {
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
  if (o.coverage) {
    uint64_t g[16], d[16];
    rtla_coverage(r.ctx, g, d, 16);
    printf("The coverage statistics at %s\n", now_str().c_str());
    for (int k = 0; k < 16; k++) {
      if (k == 7) continue;
      printf("<%s of module raft>: %llu:%llu\n", COVER[k], (ull)d[k], (ull)g[k]);
    }
    printf("End of statistics.\n");
  }
  printf("%llu states generated, %llu distinct states found, %llu states left on queue.\n",
         (ull)ls.generated_total, (ull)ls.distinct_total,
         (ull)(r.simulated || r.audited ? ls.new_states : 0));
  if (r.audited) printf("The depth of the breadth-first search before the audit is %d.\n", depth);
  else if (r.simulated) printf("The depth of the breadth-first search before the simulation is %d.\n", depth);
  else printf("The depth of the complete state graph search is %d.\n", depth);
  printf("Finished in %.2fs at (%s)\n", r.secs, now_str().c_str());
  return r.st == RTLA_VIOLATION ? 12 : 0;
}
}  // namespace

int main(int argc, char** argv) {
  Options o;
  if (const int rc = parse_args(argc, argv, &o); rc != GO_ON) return rc;
  if (o.gpus > 1 && !getenv("RTLA_RANK")) return launch_ranks(o.gpus, argv);
  o.rank = getenv("RTLA_RANK") ? atoi(getenv("RTLA_RANK")) : 0;
  o.world = getenv("RTLA_WORLD") ? atoi(getenv("RTLA_WORLD")) : 1;
  if (o.world != o.gpus || o.rank < 0 || o.rank >= o.world)
    return error(255, "rank %d of %d does not match -gpus %d", o.rank, o.world, o.gpus);
  if (o.rank > 0 && !freopen("/dev/null", "w", stdout)) return 255;  // rank 0 prints TLC's output
  if (getenv("RTLA_CLI_DRYRUN")) {  // launch / rendezvous check only (CPU tests)
    unsigned char id[128];
    const char* rdv = getenv("RTLA_RENDEZVOUS");
    const bool ok = o.world == 1 || (rdv && rendezvous(o.rank, rdv, true, id));
    fprintf(stderr, "rtla rank %d of %d ready (id %02x%02x%02x%02x)\n", o.rank, o.world, ok ? id[0] : 255,
            ok ? id[1] : 255, ok ? id[2] : 255, ok ? id[3] : 255);
    return ok ? 0 : 255;
  }
  if (o.spec.empty()) { usage(); return 255; }
  if (o.cfgpath.empty()) {
    const size_t n = o.spec.size();
    o.cfgpath = o.spec.substr(0, n > 4 && o.spec.compare(n - 4, 4, ".tla") == 0 ? n - 4 : n) + ".cfg";
  }
  printf("rtla (MI355X-native explicit-state checker for raft.tla), ABI %d\n", rtla_abi_version());
  errors = stdout;
  bool wrapper = false, ok = false;
  if (const int rc = check_spec(o, &wrapper); rc != GO_ON) return rc;
  CfgFile cf;
  const std::string cfg_text = read_file(o.cfgpath, &ok);
  std::string err;
  if (!ok) return error(151, "cannot read config %s", o.cfgpath.c_str());
  if (!parse_cfg(cfg_text, &cf, &err)) return error(151, "%s: %s", o.cfgpath.c_str(), err.c_str());
  const PredFile pf = read_pred_file(o.pred_file);
  Model model;
  if (const int rc = resolve(o, cf, pf, wrapper, &model); rc != GO_ON) return rc;
  Sets sets;
  if (const int rc = load_sets(model, pf, &sets); rc != GO_ON) return rc;
  unsigned char comm_id[128];
  if (o.world > 1 && !rendezvous(o.rank, getenv("RTLA_RENDEZVOUS"), false, comm_id)) {
    fprintf(stderr, "Error: rank %d: RCCL rendezvous failed\n", o.rank);
    return 255;
  }
  Run run;
  const int opened = rtla_open(&model.c, o.rank, o.world, o.world > 1 ? comm_id : nullptr, &run.ctx);
  const CtxPtr ctx(run.ctx);  // from here on every path closes the context, then frees the sets
  if (opened < 0) return error(255, "%s", rtla_strerror(opened));
  char info[1024];
  rtla_device_info(run.ctx, info, sizeof info);
  printf("Running breadth-first search Model-Checking with 128-bit fingerprints on %d GPU%s: %s\n", o.world,
         o.world > 1 ? "s (fingerprint-sharded, RCCL)" : "", info);
  printf("Starting... (%s)\n", now_str().c_str());
  printf("Computing initial states...\n");
  run.t0 = std::chrono::steady_clock::now();
  int rc = search(o, sets, &run);
  if (rc == GO_ON && o.audit) rc = audit_level(model, sets, &run);
  if (rc == GO_ON && o.simulate && run.st == RTLA_OK) rc = simulate(o, sets, &run);
  return rc == GO_ON ? report(o, model, sets, run) : rc;
}
