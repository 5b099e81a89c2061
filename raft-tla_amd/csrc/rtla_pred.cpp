// rtla_pred.cpp -- the predicate compiler: lexer, parser, type check and code
// generator of the predicate language, in one pass over
// the text.  Host only: no HIP, no context; its output is a program for
// pred_eval (rtla_pred.h).
//
// Every parse function emits the code of what it parsed and returns its type,
// the static interval of an integer and its worst-case instruction count; the
// emitter tracks the operand depth.  A set is rejected (line:col: message) when
// the program, the depth or the step bound exceeds rtla_pred.h's limits.
#include <ctype.h>
#include <string.h>

#include <algorithm>

#include "rtla_predc.h"

namespace rtla {
namespace {

enum Tok {
  K_EOF, K_IDENT, K_NUM, K_DEF /* == */, K_AND, K_OR, K_NOT, K_IMP, K_IFF, K_EQ, K_NE, K_LT, K_LE, K_GT, K_GE,
  K_PLUS, K_MINUS, K_DOTDOT, K_DOT, K_COMMA, K_COLON, K_LP, K_RP, K_LB, K_RB, K_FORALL, K_EXISTS, K_IN,
  K_DASHES, K_EQUALS, K_UNSUPPORTED, K_BAD
};
struct Token {
  Tok k = K_EOF;
  std::string s;
  long v = 0;
  int line = 1, col = 1;
};

enum Type {
  T_BOOL, T_INT, T_SERVER, T_STATE, T_MTYPE, T_ENTRY, T_VALUE, T_MSG, T_ELEC,
  T_LOG, T_MENTRIES, T_VSET, T_ELECTIONS  // only as the argument of Len / Cardinality / a further index
};
const char* type_name(int t) {
  static const char* const n[] = {"Boolean", "integer", "server", "server state", "message type", "log entry", "value",
                                  "message", "election", "log", "entries", "set of servers", "elections"};
  return n[t];
}

struct Err {
  int line, col;
  std::string msg;
};

constexpr uint64_t COST_CAP = 1ull << 40;
uint64_t cadd(uint64_t a, uint64_t b) { return std::min(COST_CAP, a + b); }
uint64_t cmul(uint64_t a, uint64_t b) { return a && b > COST_CAP / a ? COST_CAP : std::min(COST_CAP, a * b); }

struct Val {
  int type = T_BOOL;
  long lo = 0, hi = 0;  // T_INT: static interval
  uint64_t cost = 0;    // worst-case instructions
  int aux = 0;          // T_VSET: 1 = votesGranted, 0 = votesResponded (only the server index is emitted so far)
  int row = 0;          // T_MSG / T_ELEC / T_MENTRIES / T_VSET / T_LOG / T_ELECTIONS: PRED_PRIME if of the primed row
};

struct Bound {
  std::string name;
  int type;
  long lo, hi;
  int row = 0;  // T_MSG / T_ELEC: the row whose domain the variable ranges over (PRED_PRIME: the primed row)
};

struct Compiler {
  const Layout& L;
  std::vector<Token> toks;
  size_t p = 0;
  std::vector<uint32_t> code;
  int depth = 0, max_depth = 0, nest = 0;
  std::vector<Bound> scope;
  const bool step;         // pred_compile's step: action definitions are compiled, state definitions skipped
  bool in_action = false;  // inside [][ ... ]_vars: state variables may carry a prime

  Compiler(const Layout& l, bool step_) : L(l), step(step_) {}

  [[noreturn]] void fail(const Token& t, const std::string& msg) { throw Err{t.line, t.col, msg}; }
  const Token& cur() const { return toks[p]; }
  const Token& peek(size_t n = 1) const { return toks[std::min(p + n, toks.size() - 1)]; }
  Token take() {
    Token t = toks[p];
    if (p + 1 < toks.size()) p++;
    return t;
  }
  bool is_ident(const char* s) const { return cur().k == K_IDENT && cur().s == s; }
  void expect(Tok k, const char* what) {
    if (cur().k == K_UNSUPPORTED && k != K_UNSUPPORTED) fail(cur(), "'" + cur().s + "' is not supported");
    if (cur().k != k) fail(cur(), std::string("expected ") + what);
    take();
  }
  void expect_ident(const char* s) {
    if (!is_ident(s)) fail(cur(), std::string("expected ") + s);
    take();
  }
  // After a state variable's name: its prime, if any (PRED_PRIME), allowed inside [][ ... ]_vars only.
  bool at_prime() const { return cur().k == K_UNSUPPORTED && cur().s == "'"; }
  int prime() {
    if (!at_prime()) return 0;
    if (!in_action) fail(cur(), "''' is not supported");
    take();
    return PRED_PRIME;
  }
  static const char* row_name(int row) { return row ? "the primed row" : "the unprimed row"; }

  // ---- lexer
  void lex(const char* s, size_t n) {
    size_t i = 0;
    int line = 1, col = 1;
    auto adv = [&](size_t k) {
      for (size_t q = 0; q < k && i < n; q++, i++) {
        if (s[i] == '\n') { line++; col = 1; } else col++;
      }
    };
    auto at = [&](const char* lit) {
      const size_t m = strlen(lit);
      return i + m <= n && memcmp(s + i, lit, m) == 0;
    };
    auto word_end = [&](size_t m) {  // a backslash keyword must not run on into an identifier
      return i + m >= n || !(isalnum((unsigned char)s[i + m]) || s[i + m] == '_');
    };
    for (;;) {
      while (i < n && (s[i] == ' ' || s[i] == '\t' || s[i] == '\r' || s[i] == '\n')) adv(1);
      Token t;
      t.line = line;
      t.col = col;
      if (i >= n) { toks.push_back(t); return; }
      if (at("\\*")) {
        while (i < n && s[i] != '\n') adv(1);
        continue;
      }
      if (at("(*")) {
        int deep = 0;
        do {
          if (at("(*")) { deep++; adv(2); }
          else if (at("*)")) { deep--; adv(2); }
          else adv(1);
        } while (deep > 0 && i < n);
        if (deep > 0) fail(t, "unterminated comment");
        continue;
      }
      const unsigned char c = (unsigned char)s[i];
      if (isalpha(c) || c == '_') {
        size_t j = i;
        while (j < n && (isalnum((unsigned char)s[j]) || s[j] == '_')) j++;
        t.k = K_IDENT;
        t.s.assign(s + i, j - i);
        adv(j - i);
      } else if (isdigit(c)) {
        size_t j = i;
        long v = 0;
        while (j < n && isdigit((unsigned char)s[j])) {
          v = std::min(v * 10 + (s[j] - '0'), 1000000L);
          j++;
        }
        t.k = K_NUM;
        t.v = v;
        adv(j - i);
      } else {
        static const struct { const char* lit; Tok k; bool word; } sym[] = {
            {"\\A", K_FORALL, true}, {"\\E", K_EXISTS, true}, {"\\in", K_IN, true},
            {"/\\", K_AND, false}, {"\\/", K_OR, false}, {"<=>", K_IFF, false}, {"=>", K_IMP, false},
            {"=<", K_LE, false}, {"<=", K_LE, false}, {">=", K_GE, false}, {"/=", K_NE, false},
            {"..", K_DOTDOT, false}, {"#", K_NE, false}, {"<", K_LT, false}, {">", K_GT, false},
            {"~", K_NOT, false}, {"+", K_PLUS, false}, {".", K_DOT, false},
            {",", K_COMMA, false}, {":", K_COLON, false}, {"(", K_LP, false}, {")", K_RP, false},
            {"[", K_LB, false}, {"]", K_RB, false}};
        if (c == '-' || c == '=') {
          size_t j = i;
          while (j < n && (unsigned char)s[j] == c) j++;
          const size_t run = j - i;
          if (run >= 4) {
            t.k = c == '-' ? K_DASHES : K_EQUALS;
            adv(run);
          } else if (c == '=' && at("=>")) {
            t.k = K_IMP; adv(2);
          } else if (c == '=' && at("=<")) {
            t.k = K_LE; adv(2);
          } else if (c == '=' && run == 2) {
            t.k = K_DEF; adv(2);
          } else if (run == 1) {
            t.k = c == '-' ? K_MINUS : K_EQ; adv(1);
          } else {
            t.k = K_BAD; t.s.assign(s + i, run); adv(run);
          }
        } else {
          bool hit = false;
          for (const auto& e : sym) {
            const size_t m = strlen(e.lit);
            if (at(e.lit) && (!e.word || word_end(m))) {
              t.k = e.k;
              t.s = e.lit;
              adv(m);
              hit = true;
              break;
            }
          }
          if (!hit) {
            t.k = (c == '{' || c == '}' || c == '\'' || c == '\\' || c == '|' || c == '@' || c == '"') ? K_UNSUPPORTED
                                                                                                      : K_BAD;
            t.s.assign(1, (char)c);
            adv(1);
            if (c == '\\')  // a TLA+ operator this language does not have (\cup, \subseteq, ...)
              while (i < n && isalpha((unsigned char)s[i])) { t.s.push_back(s[i]); adv(1); }
          }
        }
      }
      toks.push_back(t);
    }
  }

  // ---- emitter
  int emit(int op, int a, int imm, int delta) {
    if ((int)code.size() >= PRED_MAX_WORDS - 1)
      fail(cur(), "the set's program exceeds " + std::to_string(PRED_MAX_WORDS) + " words");
    code.push_back(pred_ins(op, a, imm));
    depth += delta;
    if (depth > max_depth) max_depth = depth;
    if (depth > PRED_STACK) fail(cur(), "operand depth exceeds " + std::to_string(PRED_STACK));
    return (int)code.size() - 1;
  }
  void patch(int at) { code[(size_t)at] = (code[(size_t)at] & 0xffffu) | (uint32_t)code.size() << 16; }

  struct Nest {
    Compiler& c;
    explicit Nest(Compiler& c_) : c(c_) {
      if (++c.nest > 256) c.fail(c.cur(), "expression nested too deeply");
    }
    ~Nest() { c.nest--; }
  };

  void want(const Val& v, int type, const Token& at) {
    if (v.type != type)
      fail(at, std::string("type error: expected ") + type_name(type) + ", found " + type_name(v.type));
  }

  // ---- expressions, lowest precedence first
  // TLA+'s table: `=>` (1-1) binds looser than `<=>` (2-2), and neither has a chain.
  Val expr() {
    Nest g(*this);
    Val a = iff();
    if (cur().k == K_IMP) {
      const Token op = take();
      want(a, T_BOOL, op);
      emit(P_NOT, 0, 0, 0);
      const int j = emit(P_JTK, 0, 0, -1);
      Val b = iff();
      want(b, T_BOOL, op);
      patch(j);
      a.cost = cadd(cadd(a.cost, b.cost), 2);
      if (cur().k == K_IMP) fail(cur(), "'a => b => c' has no parse in TLA+: parenthesise one of the two");
    }
    return a;
  }
  Val iff() {
    Nest g(*this);
    Val a = disj();
    if (cur().k == K_IFF) {
      const Token op = take();
      want(a, T_BOOL, op);
      Val b = disj();
      want(b, T_BOOL, op);
      emit(P_EQ, 0, 0, -1);
      a.cost = cadd(cadd(a.cost, b.cost), 1);
      if (cur().k == K_IFF) fail(cur(), "'a <=> b <=> c' has no parse in TLA+: parenthesise one of the two");
    }
    return a;
  }
  Val disj() {
    Val a = conj();
    while (cur().k == K_OR) {
      const Token op = take();
      want(a, T_BOOL, op);
      const int j = emit(P_JTK, 0, 0, -1);
      Val b = conj();
      want(b, T_BOOL, op);
      patch(j);
      a.cost = cadd(cadd(a.cost, b.cost), 1);
    }
    return a;
  }
  Val conj() {
    Val a = neg();
    while (cur().k == K_AND) {
      const Token op = take();
      want(a, T_BOOL, op);
      const int j = emit(P_JFK, 0, 0, -1);
      Val b = neg();
      want(b, T_BOOL, op);
      patch(j);
      a.cost = cadd(cadd(a.cost, b.cost), 1);
    }
    return a;
  }
  Val neg() {
    if (cur().k == K_NOT) {
      Nest g(*this);
      const Token op = take();
      Val a = neg();
      want(a, T_BOOL, op);
      emit(P_NOT, 0, 0, 0);
      a.cost = cadd(a.cost, 1);
      return a;
    }
    return cmp();
  }
  static bool scalar(int t) { return t <= T_ELEC; }
  Val cmp() {
    const Token first = cur();
    Val a = sum();
    const Tok k = cur().k;
    if (k == K_IN) {
      const Token op = take();
      want(a, T_SERVER, first);
      const Token set = cur();
      int which;
      if (is_ident("votesResponded")) which = 0;
      else if (is_ident("votesGranted")) which = 1;
      else fail(set, "expected votesResponded[i] or votesGranted[i] after \\in");
      take();
      const int pr = prime();
      expect(K_LB, "[");
      const Token it = cur();
      Val i = expr();
      want(i, T_SERVER, it);
      expect(K_RB, "]");
      emit(P_VIN, which | pr, 0, -1);
      Val r;
      r.cost = cadd(cadd(a.cost, i.cost), 1);
      (void)op;
      return r;
    }
    if (k == K_EQ || k == K_NE || k == K_LT || k == K_LE || k == K_GT || k == K_GE) {
      const Token op = take();
      if (!scalar(a.type)) fail(first, std::string("type error: a ") + type_name(a.type) + " cannot be compared");
      const Token second = cur();
      Val b = sum();
      if (a.type != b.type)
        fail(second, std::string("type error: ") + type_name(a.type) + " compared with " + type_name(b.type));
      if ((a.type == T_MSG || a.type == T_ELEC) && a.row != b.row)
        fail(second, std::string("type error: a ") + type_name(a.type) + " of " + row_name(a.row) +
                         " compared with one of " + row_name(b.row));
      if (k != K_EQ && k != K_NE && a.type != T_INT)
        fail(op, std::string("type error: a ") + type_name(a.type) + " is compared only with = and #");
      emit(k == K_EQ ? P_EQ : k == K_NE ? P_NE : k == K_LT ? P_LT : k == K_LE ? P_LE : k == K_GT ? P_GT : P_GE, 0, 0,
           -1);
      Val r;
      r.cost = cadd(cadd(a.cost, b.cost), 1);
      return r;
    }
    if (!scalar(a.type)) fail(first, std::string("type error: a ") + type_name(a.type) + " is not a value here");
    return a;
  }
  Val sum() {
    const Token first = cur();
    Val a = prim();
    while (cur().k == K_PLUS || cur().k == K_MINUS) {
      const Token op = take();
      want(a, T_INT, first);
      const Token second = cur();
      Val b = prim();
      want(b, T_INT, second);
      if (op.k == K_PLUS) { a.lo += b.lo; a.hi += b.hi; } else { a.lo -= b.hi; a.hi -= b.lo; }
      a.lo = std::max(a.lo, -10000000L);
      a.hi = std::min(a.hi, 10000000L);
      emit(op.k == K_PLUS ? P_ADD : P_SUB, 0, 0, -1);
      a.cost = cadd(cadd(a.cost, b.cost), 1);
    }
    return a;
  }

  Val constant(int type, int v) {
    emit(P_PUSHI, 0, v, 1);
    Val r;
    r.type = type;
    r.lo = r.hi = v;
    r.cost = 1;
    return r;
  }
  Val ival(long lo, long hi, uint64_t cost) {
    Val r;
    r.type = T_INT;
    r.lo = lo;
    r.hi = hi;
    r.cost = cost;
    return r;
  }
  Val typed(int type, uint64_t cost) {
    Val r;
    r.type = type;
    r.cost = cost;
    return r;
  }
  // `[ server-expression ]`
  uint64_t server_index() {
    expect(K_LB, "[");
    const Token it = cur();
    Val i = expr();
    want(i, T_SERVER, it);
    expect(K_RB, "]");
    return i.cost;
  }

  Val quant() {
    Nest g(*this);
    const Token q = take();
    const bool all = q.k == K_FORALL;
    struct Open { int slot, init, body; uint64_t dom_cost, trips; };
    std::vector<Open> open;
    const size_t scope0 = scope.size();
    for (;;) {  // groups `x, y \in D` separated by commas
      std::vector<Token> names;
      for (;;) {
        if (cur().k != K_IDENT) fail(cur(), "expected a variable name");
        names.push_back(take());
        if (cur().k == K_COMMA) { take(); continue; }
        break;
      }
      expect(K_IN, "\\in");
      const size_t dom_at = p;
      size_t dom_end = p;
      for (const Token& nm : names) {
        if (known_name(nm.s)) fail(nm, "'" + nm.s + "' is already defined");
        for (const Bound& b : scope)
          if (b.name == nm.s) fail(nm, "'" + nm.s + "' is already bound");
        if (scope.size() >= (size_t)PRED_VARS)
          fail(nm, "more than " + std::to_string(PRED_VARS) + " variables bound at once");
        p = dom_at;  // every variable of the group ranges over the same domain: its code is emitted again
        Bound b;
        b.name = nm.s;
        uint64_t dom_cost = 1, trips;
        if (is_ident("Server")) {
          take();
          emit(P_DOM, PD_SERVER, 0, 2);
          b.type = T_SERVER; b.lo = 0; b.hi = L.N - 1;
          trips = (uint64_t)L.N;
        } else if (is_ident("DOMAIN")) {
          take();
          expect_ident("messages");
          b.row = prime();
          emit(P_DOM, PD_MESSAGES | b.row, 0, 2);
          b.type = T_MSG; b.lo = 0; b.hi = L.K - 1;
          trips = (uint64_t)L.K;
        } else if (is_ident("elections")) {
          take();
          b.row = prime();
          emit(P_DOM, PD_ELECTIONS | b.row, 0, 2);
          b.type = T_ELEC; b.lo = 0; b.hi = L.E - 1;
          trips = (uint64_t)L.E;
        } else {
          const Token lt = cur();
          Val lo = sum();
          want(lo, T_INT, lt);
          expect(K_DOTDOT, "..");
          const Token ht = cur();
          Val hi = sum();
          want(hi, T_INT, ht);
          emit(P_CLAMP, 0, 0, 0);
          b.type = T_INT;
          b.lo = std::max(lo.lo, 0L);
          b.hi = std::min(hi.hi, (long)PRED_RANGE_MAX);
          trips = b.hi >= b.lo ? (uint64_t)(b.hi - b.lo + 1) : 0;
          dom_cost = cadd(cadd(lo.cost, hi.cost), 1);
        }
        dom_end = p;
        Open o;
        o.slot = (int)scope.size();
        o.init = emit(all ? P_QINIT_A : P_QINIT_E, o.slot, 0, -1);
        o.body = (int)code.size();
        o.dom_cost = dom_cost;
        o.trips = trips;
        open.push_back(o);
        scope.push_back(b);
      }
      p = dom_end;
      if (cur().k == K_COMMA) { take(); continue; }
      break;
    }
    expect(K_COLON, ":");
    const Token bt = cur();
    Val body = expr();
    want(body, T_BOOL, bt);
    uint64_t cost = body.cost;
    for (size_t k = open.size(); k-- > 0;) {
      emit(all ? P_QNEXT_A : P_QNEXT_E, open[k].slot, open[k].body, -1);
      patch(open[k].init);
      cost = cadd(cadd(open[k].dom_cost, 1), cmul(open[k].trips, cadd(cost, 1)));
    }
    scope.resize(scope0);
    return typed(T_BOOL, cost);
  }

  static bool known_name(const std::string& s) {
    static const char* const words[] = {
        "TRUE", "FALSE", "IF", "THEN", "ELSE", "Server", "DOMAIN", "messages", "elections", "Len", "Cardinality",
        "BagCardinality", "Min", "Max", "Follower", "Candidate", "Leader", "Nil", "RequestVoteRequest",
        "RequestVoteResponse", "AppendEntriesRequest", "AppendEntriesResponse", "currentTerm", "state", "votedFor",
        "commitIndex", "log", "nextIndex", "matchIndex", "votesResponded", "votesGranted", "MODULE", "EXTENDS",
        "allLogs", "voterLog", "SubSeq", "LET", "IN", "CHOOSE", "EXCEPT", "UNCHANGED", "SUBSET", "UNION", "CASE",
        "OTHER", "ENABLED"};
    for (const char* w : words)
      if (s == w) return true;
    return false;
  }
  static bool unsupported_name(const std::string& s) {
    static const char* const words[] = {"mlog", "elog", "voterLog", "evotes", "evoterLog", "allLogs", "SubSeq", "LET",
                                        "IN", "CHOOSE", "EXCEPT", "UNCHANGED", "SUBSET", "UNION", "CASE", "OTHER",
                                        "ENABLED"};
    for (const char* w : words)
      if (s == w) return true;
    return false;
  }

  Val msg_field(const Token& f, uint64_t cost, int row) {
    static const struct { const char* name; int field, type; } fields[] = {
        {"mtype", PM_TYPE, T_MTYPE}, {"mterm", PM_TERM, T_INT}, {"msource", PM_SOURCE, T_SERVER},
        {"mdest", PM_DEST, T_SERVER}, {"mlastLogTerm", PM_LASTLOGTERM, T_INT},
        {"mlastLogIndex", PM_LASTLOGINDEX, T_INT}, {"mvoteGranted", PM_VOTEGRANTED, T_BOOL},
        {"mprevLogIndex", PM_PREVLOGINDEX, T_INT}, {"mprevLogTerm", PM_PREVLOGTERM, T_INT},
        {"mcommitIndex", PM_COMMITINDEX, T_INT}, {"msuccess", PM_SUCCESS, T_BOOL},
        {"mmatchIndex", PM_MATCHINDEX, T_INT}};
    if (f.s == "mentries") {  // (Len emits the read)
      Val r = typed(T_MENTRIES, cost);
      r.row = row;
      return r;
    }
    for (const auto& e : fields)
      if (f.s == e.name) {
        emit(P_MSG, e.field | row, 0, 0);
        Val r = typed(e.type, cadd(cost, 1));
        if (e.type == T_INT) {
          r.lo = e.field == PM_TERM ? 1 : 0;
          r.hi = (e.field == PM_TERM || e.field == PM_LASTLOGTERM || e.field == PM_PREVLOGTERM) ? L.T : L.L;
        }
        return r;
      }
    if (unsupported_name(f.s)) fail(f, "'" + f.s + "' is not supported");
    fail(f, "unknown message field '" + f.s + "'");
  }

  Val prim() {
    Val v = prim_unprimed();
    if (in_action && at_prime()) fail(cur(), "only a state variable may carry a prime");
    return v;
  }
  Val prim_unprimed() {
    Nest g(*this);
    const Token t = cur();
    switch (t.k) {
      case K_NUM:
        take();
        if (t.v > 32767) fail(t, "integer literal out of range");
        return constant(T_INT, (int)t.v);
      case K_MINUS: {
        take();
        emit(P_PUSHI, 0, 0, 1);
        const Token at = cur();
        Val a = prim();
        want(a, T_INT, at);
        emit(P_SUB, 0, 0, -1);
        return ival(-a.hi, -a.lo, cadd(a.cost, 2));
      }
      case K_LP: {
        take();
        Val a = expr();
        expect(K_RP, ")");
        return a;
      }
      case K_FORALL: case K_EXISTS: return quant();
      case K_UNSUPPORTED: fail(t, "'" + t.s + "' is not supported");
      case K_IDENT: break;
      case K_EOF: fail(t, "expected an expression, found the end of the text");
      default: fail(t, "expected an expression");
    }
    take();
    const std::string& s = t.s;
    if (cur().k == K_DEF) fail(t, "expected an expression");  // (the next definition's name)
    if (s == "TRUE") return constant(T_BOOL, 1);
    if (s == "FALSE") return constant(T_BOOL, 0);
    if (s == "Follower") return constant(T_STATE, FOLLOWER);
    if (s == "Candidate") return constant(T_STATE, CANDIDATE);
    if (s == "Leader") return constant(T_STATE, LEADER);
    if (s == "Nil") return constant(T_SERVER, (int)NIL);
    if (s == "RequestVoteRequest") return constant(T_MTYPE, RVREQ);
    if (s == "RequestVoteResponse") return constant(T_MTYPE, RVRESP);
    if (s == "AppendEntriesRequest") return constant(T_MTYPE, AEREQ);
    if (s == "AppendEntriesResponse") return constant(T_MTYPE, AERESP);
    if (s == "IF") {
      const Token ct = cur();
      Val c = expr();
      want(c, T_BOOL, ct);
      expect_ident("THEN");
      const int jz = emit(P_JZ, 0, 0, -1);
      const int d0 = depth;
      Val a = expr();
      expect_ident("ELSE");
      const int jmp = emit(P_JMP, 0, 0, 0);
      patch(jz);
      depth = d0;
      const Token et = cur();
      Val b = expr();
      if (a.type != b.type)
        fail(et, std::string("type error: THEN is a ") + type_name(a.type) + ", ELSE a " + type_name(b.type));
      if ((a.type == T_MSG || a.type == T_ELEC) && a.row != b.row)
        fail(et, std::string("type error: THEN is a ") + type_name(a.type) + " of " + row_name(a.row) +
                     ", ELSE one of " + row_name(b.row));
      patch(jmp);
      a.lo = std::min(a.lo, b.lo);
      a.hi = std::max(a.hi, b.hi);
      a.cost = cadd(cadd(c.cost, 2), std::max(a.cost, b.cost));
      return a;
    }
    if (s == "Min" || s == "Max") {
      expect(K_LP, "(");
      const Token at = cur();
      Val a = expr();
      want(a, T_INT, at);
      expect(K_COMMA, ", (Min and Max take two integers)");
      const Token bt = cur();
      Val b = expr();
      want(b, T_INT, bt);
      expect(K_RP, ")");
      const bool mn = s == "Min";
      emit(mn ? P_MIN : P_MAX, 0, 0, -1);
      return ival(mn ? std::min(a.lo, b.lo) : std::max(a.lo, b.lo), mn ? std::min(a.hi, b.hi) : std::max(a.hi, b.hi),
                  cadd(cadd(a.cost, b.cost), 1));
    }
    if (s == "Len") {
      expect(K_LP, "(");
      const Token at = cur();
      Val a = sum();
      expect(K_RP, ")");
      if (a.type == T_LOG) {
        emit(P_LOGLEN, a.row, 0, 0);
        return ival(0, L.L + 1, cadd(a.cost, 1));
      }
      if (a.type == T_MENTRIES) {
        emit(P_MSG, PM_NENTRIES | a.row, 0, 0);
        return ival(0, 1, cadd(a.cost, 1));
      }
      fail(at, std::string("type error: Len of a ") + type_name(a.type));
    }
    if (s == "Cardinality") {
      expect(K_LP, "(");
      const Token at = cur();
      Val a = sum();
      expect(K_RP, ")");
      if (a.type == T_VSET) {
        emit(P_SRV, (a.aux ? PS_NGRANTED : PS_NRESPONDED) | a.row, 0, 0);
        return ival(0, L.N, cadd(a.cost, 1));
      }
      if (a.type == T_ELECTIONS) {
        emit(P_NELEC, a.row, 0, 1);
        return ival(0, L.E, 1);
      }
      fail(at, std::string("type error: Cardinality of a ") + type_name(a.type));
    }
    if (s == "BagCardinality") {
      expect(K_LP, "(");
      expect_ident("messages");
      const int pr = prime();
      expect(K_RP, ")");
      emit(P_BAGCARD, pr, 0, 1);
      return ival(0, (long)L.K * (L.C + 1), 1);
    }
    if (s == "elections") {
      Val r = typed(T_ELECTIONS, 0);
      r.row = prime();
      return r;
    }
    if (s == "currentTerm" || s == "state" || s == "votedFor" || s == "commitIndex") {
      const int pr = prime();
      const uint64_t c = server_index();
      const int f = s == "currentTerm" ? PS_TERM : s == "state" ? PS_STATE : s == "votedFor" ? PS_VOTED : PS_COMMIT;
      emit(P_SRV, f | pr, 0, 0);
      if (f == PS_TERM) return ival(1, L.T + 1, cadd(c, 1));
      if (f == PS_COMMIT) return ival(0, L.L, cadd(c, 1));
      return typed(f == PS_STATE ? T_STATE : T_SERVER, cadd(c, 1));
    }
    if (s == "votesResponded" || s == "votesGranted") {
      const int pr = prime();
      Val r = typed(T_VSET, server_index());
      r.aux = s == "votesGranted";
      r.row = pr;
      return r;
    }
    if (s == "log") {
      const int pr = prime();
      uint64_t c = server_index();
      if (cur().k != K_LB) {
        Val r = typed(T_LOG, c);
        r.row = pr;
        return r;
      }
      take();
      const Token nt = cur();
      Val n = expr();
      want(n, T_INT, nt);
      expect(K_RB, "]");
      emit(P_LOGENT, pr, 0, -1);
      c = cadd(cadd(c, n.cost), 1);
      if (cur().k != K_DOT) return typed(T_ENTRY, c);
      take();
      const Token f = cur();
      if (f.k == K_IDENT && f.s == "term") {
        take();
        emit(P_ENT, 0, 0, 0);
        return ival(1, L.T, cadd(c, 1));
      }
      if (f.k == K_IDENT && f.s == "value") {
        take();
        emit(P_ENT, 1, 0, 0);
        return typed(T_VALUE, cadd(c, 1));
      }
      fail(f, "expected .term or .value");
    }
    if (s == "nextIndex" || s == "matchIndex") {
      const int pr = prime();
      uint64_t c = server_index();
      c = cadd(c, server_index());
      emit(P_NM, (s == "matchIndex" ? 1 : 0) | pr, 0, -1);
      return s == "nextIndex" ? ival(1, L.L + 1, cadd(c, 1)) : ival(0, L.L, cadd(c, 1));
    }
    if (s == "messages") {
      const int pr = prime();
      expect(K_LB, "[");
      const Token mt = cur();
      Val m = expr();
      want(m, T_MSG, mt);
      if (m.row != pr)
        fail(mt, std::string("type error: a message of ") + row_name(m.row) + " indexes the bag of " + row_name(pr));
      expect(K_RB, "]");
      emit(P_MSG, PM_COUNT | pr, 0, 0);
      return ival(1, L.C + 1, cadd(m.cost, 1));
    }
    for (size_t k = scope.size(); k-- > 0;) {
      if (scope[k].name != s) continue;
      emit(P_LOADV, (int)k, 0, 1);
      Val r = typed(scope[k].type, 1);
      r.lo = scope[k].lo;
      r.hi = scope[k].hi;
      r.row = scope[k].row;
      if (cur().k != K_DOT) return r;
      take();
      const Token f = cur();
      if (f.k != K_IDENT) fail(f, "expected a field name");
      take();
      if (r.type == T_MSG) return msg_field(f, 1, r.row);
      if (r.type == T_ELEC) {
        if (f.s == "eterm") { emit(P_ELEC, r.row, 0, 0); return ival(1, L.T, 2); }
        if (f.s == "eleader") { emit(P_ELEC, 1 | r.row, 0, 0); return typed(T_SERVER, 2); }
        if (unsupported_name(f.s)) fail(f, "'" + f.s + "' is not supported");
        fail(f, "unknown election field '" + f.s + "'");
      }
      fail(f, std::string("type error: a ") + type_name(r.type) + " has no fields");
    }
    if (unsupported_name(s)) fail(t, "'" + s + "' is not supported");
    fail(t, "unknown identifier '" + s + "'");
  }

  // ---- a predicate file
  void file(rtla_pred* out) {
    if (cur().k == K_DASHES) {  // ---- MODULE Name ----
      take();
      expect_ident("MODULE");
      expect(K_IDENT, "a module name");
      expect(K_DASHES, "----");
    }
    if (is_ident("EXTENDS")) {
      take();
      for (;;) {
        expect(K_IDENT, "a module name");
        if (cur().k != K_COMMA) break;
        take();
      }
    }
    uint64_t steps = 1;  // P_HALT
    std::vector<std::string> defined;  // every definition's name (a step set compiles the action definitions only)
    while (cur().k != K_EOF && cur().k != K_EQUALS) {
      const Token name = cur();
      if (name.k != K_IDENT) fail(name, "expected a definition (Name == expression)");
      take();
      expect(K_DEF, "==");
      static const char* const builtin[] = {"NoTwoLeaders", "ElectionSafety", "LogMatching", "StateMachineSafety",
                                            "LeaderCompleteness"};
      for (const char* b : builtin)
        if (name.s == b) fail(name, "'" + name.s + "' is a built-in invariant's name");
      if (known_name(name.s)) fail(name, "'" + name.s + "' is reserved");
      for (const std::string& n : defined)
        if (n == name.s) fail(name, "'" + name.s + "' is defined twice");
      defined.push_back(name.s);
      // Name == [][ expr ]_vars: an action definition, compiled by a step set only
      const bool action = step && cur().k == K_LB && peek().k == K_RB && peek(2).k == K_LB;
      if (step && !action) {  // a state definition of a step set's text: parsed, type-checked, not compiled
        const size_t code0 = code.size();
        const int depth0 = max_depth;
        const Token bt = cur();
        Val v = expr();
        if (v.type != T_BOOL)
          fail(bt, std::string("type error: a definition must be Boolean, this is a ") + type_name(v.type));
        code.resize(code0);
        depth = 0;
        max_depth = depth0;
        continue;
      }
      if (out->names.size() >= (size_t)PRED_MAX_DEFS)
        fail(name, "more than " + std::to_string(PRED_MAX_DEFS) + (step ? " action definitions" : " definitions"));
      if (action) {
        take(); take(); take();
        in_action = true;
      }
      const Token bt = cur();
      Val v = expr();
      if (v.type != T_BOOL) fail(bt, std::string("type error: a definition must be Boolean, this is a ") + type_name(v.type));
      if (action) {
        in_action = false;
        expect(K_RB, "]_vars");
        if (!is_ident("_vars")) fail(cur(), "expected _vars (the only subscript of an action definition)");
        take();
      }
      emit(P_DEFEND, (int)out->names.size(), 0, -1);
      steps = cadd(steps, cadd(v.cost, 1));
      if (steps > PRED_MAX_STEPS)
        fail(name, "the set's worst case is " + (steps >= COST_CAP ? std::string("over 2^40") : std::to_string(steps)) +
                       " steps per row, above the bound of " + std::to_string(PRED_MAX_STEPS));
      out->names.push_back(name.s);
    }
    if (cur().k == K_EQUALS) {
      take();
      if (cur().k != K_EOF) fail(cur(), "text after the end of the module");
    }
    code.push_back(pred_ins(P_HALT, 0, 0));
    out->steps = steps;
  }
};

}  // namespace

static bool compile_set(const Layout& L, const char* text, size_t len, bool step, rtla_pred* out, std::string* err) {
  Compiler c(L, step);
  out->L = L;
  out->step = step;
  out->names.clear();
  out->code.clear();
  try {
    c.lex(text, len);
    c.file(out);
    if (step && out->names.empty()) throw Err{1, 1, "the text holds no action definition (Name == [][ expr ]_vars)"};
  } catch (const Err& e) {
    if (err) *err = std::to_string(e.line) + ":" + std::to_string(e.col) + ": " + e.msg;
    out->names.clear();
    return false;
  }
  out->code = std::move(c.code);
  out->depth = c.max_depth;
  return true;
}

bool pred_compile(const Layout& L, const char* text, size_t len, rtla_pred* out, std::string* err) {
  return compile_set(L, text, len, false, out, err);
}
bool pred_compile_step(const Layout& L, const char* text, size_t len, rtla_pred* out, std::string* err) {
  return compile_set(L, text, len, true, out, err);
}

}  // namespace rtla
