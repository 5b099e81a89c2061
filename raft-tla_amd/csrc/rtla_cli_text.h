// rtla_cli_text.h -- the text code of the command line (rtla_cli.cpp): sha256 of the spec, TLC's cfg grammar, the
// definitions of a -predicates file, the trace printer's name substitution.  Strings in, strings out: it needs
// neither the library nor a device header, so tests/cli_text_main.cpp runs it under the host sanitizers.
#pragma once
#include <ctype.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

// ------------------------------------------------------------- sha256 ----
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

inline std::string read_file(const std::string& p, bool* ok) {
  std::ifstream f(p, std::ios::binary);
  *ok = (bool)f;
  std::stringstream ss;
  ss << f.rdbuf();
  return ss.str();
}

// ------------------------------------------------------------ cfg parse ----
// The cfg grammar is TLC's subset used by raft.cfg: SPECIFICATION, INVARIANT(S), CONSTRAINT(S), PROPERTY /
// PROPERTIES, SYMMETRY, CONSTANT(S) with `Name = {a, b}` / `Name = "str"` / `Name = 3` / `Name = mv`, and
// \* / (* *) comments.
struct CfgFile {
  std::string specification;
  std::string symmetry;  // SYMMETRY operator name ("" = none)
  std::vector<std::string> invariants, constraints;
  std::vector<std::string> properties;  // PROPERTY / PROPERTIES names (action definitions of the -predicates file)
  std::string property_keyword;         // the keyword they stood under, for the refusal
  std::map<std::string, std::vector<std::string>> sets;  // Name = {a, b}
  std::map<std::string, std::string> scalars;            // Name = "x" | 3 | mv
};

inline std::string strip_comments(const std::string& s) {
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

inline std::vector<std::string> tokenize(const std::string& s) {
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

inline bool parse_cfg(const std::string& text, CfgFile* c, std::string* err) {
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

// The row printer names servers s1..sN and values v1..vV; map them to the cfg's model values.
inline std::string subst_names(const std::string& s, const std::vector<std::string>& servers,
                               const std::vector<std::string>& values) {
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

// ---- -predicates FILE: its definitions (DESIGN.md sections 13 and 14).  A definition starts at an identifier
// followed by `==` outside comments and ends where the next one, or the module's closing line, starts.
struct Def {
  size_t at;
  std::string name;
  bool action;  // Name == [][ ... ]_vars
};
// The definitions of a predicate file, in file order; *end: where the module's closing line starts.
inline std::vector<Def> scan_definitions(const std::string& text, size_t* end) {
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

// The predicate file, read and scanned once.  A file that cannot be read holds no definitions: a name looked
// up in it is not there, and loading a set from it is the error.
struct PredFile {
  std::string path, text;
  bool readable = false;
  std::vector<Def> defs;
  size_t end = 0;
  bool defines(const std::string& name, bool action) const {
    return std::any_of(defs.begin(), defs.end(), [&](const Def& d) { return d.action == action && d.name == name; });
  }
};
inline PredFile scan_pred_file(const std::string& path, const std::string& text, bool readable) {
  PredFile f{path, text, readable, {}, 0};
  f.defs = scan_definitions(f.text, &f.end);
  return f;
}
inline PredFile read_pred_file(const std::string& path) {  // ("" = no -predicates: nothing read)
  bool ok = false;
  const std::string text = path.empty() ? std::string() : read_file(path, &ok);  // (sets ok before it is passed on)
  return scan_pred_file(path, text, ok);
}

// The names of the file's definitions of one kind, in file order.
inline std::vector<std::string> definitions_of_kind(const PredFile& f, bool action) {
  std::vector<std::string> out;
  for (const Def& d : f.defs)
    if (d.action == action) out.push_back(d.name);
  return out;
}

// The file's text with every definition blanked out (line breaks kept, so a compile error's line:col is the
// file's) but those named in `keep`: the set compiled is the set named, and only it is evaluated.  states_only
// keeps a name only if a state definition carries it: INVARIANT and CONSTRAINT name no action definition.
inline std::string select_definitions(const PredFile& f, const std::vector<std::string>& keep, bool states_only) {
  std::string out = f.text;
  for (size_t d = 0; d < f.defs.size(); d++) {
    const bool named = std::find(keep.begin(), keep.end(), f.defs[d].name) != keep.end();
    if (named && (!states_only || f.defines(f.defs[d].name, false))) continue;
    const size_t stop = d + 1 < f.defs.size() ? f.defs[d + 1].at : f.end;
    for (size_t i = f.defs[d].at; i < stop; i++)
      if (out[i] != '\n') out[i] = ' ';
  }
  return out;
}
