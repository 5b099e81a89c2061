"""A generator, a printer and an evaluator for the predicate language (DESIGN.md
sections 13 and 14), in plain Python: nothing here imports the product.

* `corpus(seed, n_state, n_action)` draws definitions as typed trees from a
  splitmix64 stream (no use of Python's `random`: the corpus is the same on every
  Python), driven by the type a position needs and a node budget, and within the
  language's limits by construction and by the static model below (`depth`,
  `words`, `cost`, `nvars`): at most 6 bound variables, integer ranges inside
  0..15, literals at most 15, an operand depth of at most 16.
* `text(node)` prints a tree with the fewest parentheses TLA+ allows, by the
  precedence table of "Specifying Systems" (table 6) in `PREC`; `text(node,
  full=True)` parenthesises every composite node.
* `evaluate(node, cfg, s, t)` walks a tree over value-oracle states (`t`: the
  successor of a step) and returns TRUE, FALSE, ERR or ORDER.

A tree is a tuple `(kind, ...)`; `KINDS` below lists the kinds with their types.
"""
import raft_values as rv

TRUE, FALSE, ERR, ORDER = "TRUE", "FALSE", "ERR", "ORDER"

BOOL, INT, SERVER, STATE, MTYPE, ENTRY, VALUE, MSG, ELEC = ("Boolean", "integer", "server", "server state",
                                                            "message type", "entry", "value", "message", "election")

# ---- Specifying Systems, table 6 (operator precedence ranges; the language's operators only).  Of two adjacent
# operators the one with the higher range binds tighter; overlapping or equal ranges need parentheses unless the
# operator is associative with itself.
PREC = {"=>": 1, "<=>": 2, "/\\": 3, "\\/": 3, "~": 4,
        "=": 5, "#": 5, "/=": 5, "<": 5, "<=": 5, "=<": 5, ">": 5, ">=": 5, "\\in": 5,
        "..": 9, "+": 10, "-": 11, "neg": 12}
ASSOC = {"/\\", "\\/", "+", "-"}  # a op b op c is (a op b) op c; every other operator of PREC has no chain

STATES = [rv.FOLLOWER, rv.CANDIDATE, rv.LEADER]
MTYPES = [rv.RVREQ, rv.RVRESP, rv.AEREQ, rv.AERESP]
# message fields: name -> (type, the message type that carries it or None, the family of an integer field)
MFIELDS = {
    "mtype": (MTYPE, None, None), "mterm": (INT, None, "term"), "msource": (SERVER, None, None),
    "mdest": (SERVER, None, None),
    "mlastLogTerm": (INT, rv.RVREQ, "term"), "mlastLogIndex": (INT, rv.RVREQ, "index"),
    "mvoteGranted": (BOOL, rv.RVRESP, None),
    "mprevLogIndex": (INT, rv.AEREQ, "index"), "mprevLogTerm": (INT, rv.AEREQ, "term"),
    "mcommitIndex": (INT, rv.AEREQ, "index"), "mentries": (INT, rv.AEREQ, "count"),
    "msuccess": (BOOL, rv.AERESP, None), "mmatchIndex": (INT, rv.AERESP, "index"),
}
CMP_ALL = ["=", "#", "/=", "<", "<=", "=<", ">", ">="]
CMP_EQ = ["=", "#", "/="]

# KINDS (p: 0 the state, 1 the successor)
#  Boolean: ("true",) ("false",) ("and", a, b) ("or", a, b) ("imp", a, b) ("iff", a, b) ("not", a)
#           ("cmp", op, a, b) ("vin", j, which, p, i) ("q", "A" | "E", [([names], dom)], body) ("mf", m, field)
#  dom:     ("Server",) ("msgs", p) ("elecs", p) ("range", lo, hi)
#  integer: ("num", k) ("neg", a) ("add", a, b) ("sub", a, b) ("min", a, b) ("max", a, b) ("var", name)
#           ("srv", "currentTerm" | "commitIndex", p, i) ("len", p, i) ("lenme", m) ("term", p, i, n)
#           ("nm", "nextIndex" | "matchIndex", p, i, j) ("card", which, p, i) ("nelec", p) ("bagcard", p)
#           ("mcount", p, m) ("mf", m, field) ("ef", e, "eterm")
#  server:  ("var", name) ("nil",) ("srv", "votedFor", p, i) ("mf", m, "msource" | "mdest") ("ef", e, "eleader")
#  others:  ("const", name) ("srv", "state", p, i) ("mf", m, "mtype") ("entry", p, i, n) ("value", p, i, n)
#  any:     ("if", c, a, b)


# ---------------------------------------------------------------- the random stream

class Stream:
    """splitmix64."""

    def __init__(self, seed):
        self.x = seed & 0xFFFFFFFFFFFFFFFF

    def next(self):
        self.x = (self.x + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        z = self.x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        return z ^ (z >> 31)

    def below(self, n):
        return self.next() % n

    def chance(self, p):
        return self.next() % 10000 < int(p * 10000)

    def pick(self, items):
        return items[self.below(len(items))]


# ---------------------------------------------------------------- the printer

ATOMS = {"true", "false", "num", "var", "nil", "const", "srv", "len", "lenme", "term", "nm", "card", "nelec",
         "bagcard", "mcount", "mf", "ef", "entry", "value", "min", "max"}
BINOP = {"and": "/\\", "or": "\\/", "imp": "=>", "iff": "<=>", "add": "+", "sub": "-"}


def _p(p):
    return "'" if p else ""


def op_of(node):
    k = node[0]
    return BINOP.get(k) or (node[1] if k == "cmp" else "\\in" if k == "vin" else "~" if k == "not" else
                            "neg" if k == "neg" else None)


def text(node, full=False):
    """The text of a tree: minimal parentheses, or (full) every composite node parenthesised."""

    def inner(n):  # between delimiters: nothing binds from outside
        return show(n, 0, True, False)

    def operand(n, parent, right, tail):
        """An operand of the operator `parent`: parenthesised where table 6 needs it."""
        k = n[0]
        if full:
            return show(n, 0, True, False)
        if k in ("q", "if"):  # they extend as far as they can: bare only where nothing follows
            return show(n, 0, True, False) if tail and parent != "neg" else "(" + show(n, 0, True, False) + ")"
        mine = op_of(n)
        if mine is None:
            return show(n, 0, True, False)
        need = PREC[mine] < PREC[parent]
        if PREC[mine] == PREC[parent]:
            need = not (mine == parent and mine in ASSOC and not right)
        if parent == "neg" and mine == "neg":
            need = True
        s = show(n, 0, tail, False)
        return "(" + s + ")" if need else s

    def show(n, _, tail, top):
        k = n[0]
        s = body(n, tail)
        if full and k not in ATOMS and not top:
            return "(" + s + ")"
        return s

    def body(n, tail):
        k = n[0]
        if k in BINOP:
            o = BINOP[k]
            return "%s %s %s" % (operand(n[1], o, False, False), o, operand(n[2], o, True, tail))
        if k == "cmp":
            return "%s %s %s" % (operand(n[2], n[1], False, False), n[1], operand(n[3], n[1], True, tail))
        if k == "not":
            return "~ " + operand(n[1], "~", True, tail)
        if k == "neg":
            return "-" + operand(n[1], "neg", True, tail)
        if k == "vin":
            return "%s \\in %s%s[%s]" % (operand(n[1], "\\in", False, False), n[2], _p(n[3]), inner(n[4]))
        if k == "q":
            groups = []
            for names, dom in n[2]:
                if dom[0] == "range":
                    d = "%s..%s" % (operand(dom[1], "..", False, False), operand(dom[2], "..", True, False))
                else:
                    d = {"Server": "Server", "msgs": "DOMAIN messages" + _p(dom[-1]),
                         "elecs": "elections" + _p(dom[-1])}[dom[0]]
                groups.append("%s \\in %s" % (", ".join(names), d))
            return "\\%s %s : %s" % (n[1], ", ".join(groups), inner(n[3]))
        if k == "if":
            return "IF %s THEN %s ELSE %s" % (inner(n[1]), inner(n[2]), inner(n[3]))
        if k == "true" or k == "false":
            return k.upper()
        if k == "num":
            return str(n[1])
        if k == "var" or k == "const":
            return n[1]
        if k == "nil":
            return "Nil"
        if k == "srv":
            return "%s%s[%s]" % (n[1], _p(n[2]), inner(n[3]))
        if k == "len":
            return "Len(log%s[%s])" % (_p(n[1]), inner(n[2]))
        if k == "lenme":
            return "Len(%s.mentries)" % n[1]
        if k in ("term", "value", "entry"):
            return "log%s[%s][%s]%s" % (_p(n[1]), inner(n[2]), inner(n[3]), "" if k == "entry" else "." + k)
        if k == "nm":
            return "%s%s[%s][%s]" % (n[1], _p(n[2]), inner(n[3]), inner(n[4]))
        if k == "card":
            return "Cardinality(%s%s[%s])" % (n[1], _p(n[2]), inner(n[3]))
        if k == "nelec":
            return "Cardinality(elections%s)" % _p(n[1])
        if k == "bagcard":
            return "BagCardinality(messages%s)" % _p(n[1])
        if k == "mcount":
            return "messages%s[%s]" % (_p(n[1]), inner(n[2]))
        if k == "mf" or k == "ef":
            return "%s.%s" % (n[1], n[2])
        if k in ("min", "max"):
            return "%s(%s, %s)" % (k.capitalize(), inner(n[1]), inner(n[2]))
        raise ValueError(k)

    return show(node, 0, True, True)


def definition(name, node, action, full=False):
    return "%s == %s" % (name, "[][ %s ]_vars" % text(node, full) if action else text(node, full))


# ---------------------------------------------------------------- the static model of a program

def children(n):
    k = n[0]
    if k == "q":
        out = []
        for _, dom in n[2]:
            if dom[0] == "range":
                out += [dom[1], dom[2]]
        return out + [n[3]]
    return [c for c in n[1:] if isinstance(c, tuple)]


def walk(n):
    yield n
    for c in children(n):
        yield from walk(c)


def depth(n, full=False):
    """Operand words in use at the deepest point (instruction set): a binary operator
    holds its left operand while the right one runs, `/\\`, `\\/` and `=>` drop it first, a quantifier holds
    its upper limit per variable while the body runs, and a domain is two words.  full: of the fully
    parenthesised text."""
    k = n[0]
    if k == "add" and n[2][0] == "sub" and not full:
        # printed a + b - c, which the compiler reads (a + b) - c: the same value, the left operand dropped sooner
        return depth(("sub", ("add", n[1], n[2][1]), n[2][2]))
    if k in ("and", "or", "imp"):
        return max(depth(n[1], full), depth(n[2], full))
    if k in ("iff", "add", "sub", "min", "max"):
        return max(depth(n[1], full), 1 + depth(n[2], full))
    if k == "cmp":
        return max(depth(n[2], full), 1 + depth(n[3], full))
    if k == "not":
        return depth(n[1], full)
    if k == "neg":
        return 1 + depth(n[1], full)
    if k == "vin":
        return max(depth(n[1], full), 1 + depth(n[4], full))
    if k == "if":
        return max(depth(n[1], full), depth(n[2], full), depth(n[3], full))
    if k == "q":
        held, top = 0, 0
        for names, dom in n[2]:
            d = max(depth(dom[1], full), 1 + depth(dom[2], full)) if dom[0] == "range" else 2
            for _ in names:
                top = max(top, held + d)
                held += 1
        return max(top, held + depth(n[3], full))
    if k in ("srv", "len", "card"):
        return depth(n[3] if k != "len" else n[2], full)
    if k in ("term", "value", "entry"):
        return max(depth(n[2], full), 1 + depth(n[3], full))
    if k == "nm":
        return max(depth(n[3], full), 1 + depth(n[4], full))
    if k == "mcount":
        return depth(n[2], full)
    return 1


def words(n):
    """Program words of a tree (one per instruction)."""
    k = n[0]
    if k in ("and", "or", "iff", "add", "sub", "min", "max"):
        return words(n[1]) + words(n[2]) + 1
    if k == "imp":
        return words(n[1]) + words(n[2]) + 2
    if k == "cmp":
        return words(n[2]) + words(n[3]) + 1
    if k == "not":
        return words(n[1]) + 1
    if k == "neg":
        return words(n[1]) + 2
    if k == "vin":
        return words(n[1]) + words(n[4]) + 1
    if k == "if":
        return words(n[1]) + words(n[2]) + words(n[3]) + 2
    if k == "q":
        w = words(n[3])
        for names, dom in n[2]:
            d = words(dom[1]) + words(dom[2]) + 1 if dom[0] == "range" else 1
            w += len(names) * (d + 2)
        return w
    if k in ("srv", "card"):
        return words(n[3]) + 1
    if k == "len":
        return words(n[2]) + 1
    if k in ("term", "value"):
        return words(n[2]) + words(n[3]) + 2
    if k == "entry":
        return words(n[2]) + words(n[3]) + 1
    if k == "nm":
        return words(n[3]) + words(n[4]) + 1
    if k == "mcount":
        return words(n[2]) + 1
    if k in ("mf", "ef", "lenme"):
        return 2
    return 1


MAX_LOG = 3  # the longest MaxLogLen of the shapes the corpus is compiled for


def _upper(n):
    """A static upper bound of a range's upper limit: a literal, Len(log[i]) <= MaxLogLen + 1, Min of two; else 15."""
    if n[0] == "num":
        return n[1]
    if n[0] == "len":
        return MAX_LOG + 1
    if n[0] == "min":
        return min(_upper(n[1]), _upper(n[2]))
    return 15


def cost(n, N, K, E):
    """An upper bound of the compiler's worst-case step count (termination): its
    formula, with the static bound of `_upper` for an integer range."""
    k = n[0]
    if k == "q":
        c = cost(n[3], N, K, E)
        for names, dom in reversed(n[2]):
            if dom[0] == "range":
                dc = cost(dom[1], N, K, E) + cost(dom[2], N, K, E) + 1
                trips = max(0, _upper(dom[2]) - (dom[1][1] if dom[1][0] == "num" else 0) + 1)
            else:
                dc, trips = 1, {"Server": N, "msgs": K, "elecs": E}[dom[0]]
            for _ in names:
                c = dc + 1 + trips * (c + 1)
        return c
    if k == "if":
        return cost(n[1], N, K, E) + 2 + max(cost(n[2], N, K, E), cost(n[3], N, K, E))
    return words(n) - sum(words(c) for c in children(n)) + sum(cost(c, N, K, E) for c in children(n))


def nvars(n, held=0):
    """The most variables bound at once."""
    if n[0] == "q":
        h = held + sum(len(names) for names, _ in n[2])
        return max([h] + [nvars(c, h) for c in children(n)])
    return max([held] + [nvars(c, held) for c in children(n)])


def census(n):
    """The features of a tree, as strings (tests/test_predfuzz_host.py counts them per definition)."""
    out = set()
    for x in walk(n):
        k = x[0]
        if k in BINOP:
            out.add("op " + BINOP[k])
        elif k == "cmp":
            out.add("op " + x[1])
        elif k == "vin":
            out.add("op \\in")
            out.add(("read %s'" if x[3] else "read %s") % x[2])
        elif k == "not":
            out.add("op ~")
        elif k == "neg":
            out.add("unary minus")
        elif k in ("min", "max"):
            out.add(k.capitalize())
        elif k == "if":
            out.add("IF")
        elif k == "q":
            for _, dom in x[2]:
                d = dom[0] + ("'" if dom[0] in ("msgs", "elecs") and dom[1] else "")
                out.add("\\%s over %s" % (x[1], d))
                out.add("domain " + d)
        elif k in ("true", "false"):
            out.add("constant " + k.upper())
        elif k == "nil":
            out.add("constant Nil")
        elif k == "const":
            out.add("constant " + x[1])
        elif k in ("srv", "nm", "card"):
            out.add(("read %s'" if x[2] else "read %s") % x[1])
        elif k in ("len", "term", "value", "entry"):
            out.add("read log'" if x[1] else "read log")
            if k != "len":
                out.add("log " + k)
        elif k == "nelec":
            out.add("read elections'" if x[1] else "read elections")
        elif k in ("bagcard", "mcount"):
            out.add("read messages'" if x[1] else "read messages")
        elif k == "mf":
            out.add("field " + x[2])
        elif k == "lenme":
            out.add("field mentries")
        elif k == "ef":
            out.add("field " + x[2])
    return out


def census_items(action):
    """Everything the census must find (state definitions: no primes)."""
    items = ["op " + o for o in list(BINOP.values()) + CMP_ALL + ["\\in", "~"]]
    items += ["unary minus", "Min", "Max", "IF", "log term", "log value", "log entry"]
    items += ["constant " + c for c in ["TRUE", "FALSE", "Nil"] + STATES + MTYPES]
    items += ["field " + f for f in list(MFIELDS) + ["eterm", "eleader"]]
    doms = ["Server", "msgs", "elecs", "range"] + (["msgs'", "elecs'"] if action else [])
    items += ["domain " + d for d in doms] + ["\\%s over %s" % (q, d) for q in "AE" for d in doms]
    reads = ["currentTerm", "state", "votedFor", "commitIndex", "log", "nextIndex", "matchIndex", "votesResponded",
             "votesGranted", "messages", "elections"]
    items += ["read " + r for r in reads] + (["read %s'" % r for r in reads] if action else [])
    return items


# ---------------------------------------------------------------- the evaluator

class _Err(Exception):
    pass


def _bad(*vals):
    """The outcome of an operator that evaluates all of `vals` (the machine stops at the first error: if any
    operand surely errors so does the operator; else an operand whose outcome hangs on the order hands that on)."""
    if any(v is ERR for v in vals):
        return ERR
    if any(v is ORDER for v in vals):
        return ORDER
    return None


def _ev(n, X, env):
    """The value of a tree: a Python value, ERR or ORDER.  X = (cfg, s, t)."""
    k = n[0]
    if k == "var":
        return env[n[1]]
    if k == "mf":
        m = env[n[1]][1]
        return m[n[2]] if n[2] in m else ERR
    if k == "const" or k == "num":
        return n[1]
    if k == "true":
        return True
    if k == "false":
        return False
    if k in ("and", "or", "imp"):
        a = _ev(n[1], X, env)
        if a is ERR or a is ORDER:
            return a
        if k == "and" and not a:
            return False
        if k == "or" and a:
            return True
        if k == "imp" and not a:
            return True
        return _ev(n[2], X, env)
    if k == "not":
        a = _ev(n[1], X, env)
        return a if a is ERR or a is ORDER else not a
    if k == "neg":
        a = _ev(n[1], X, env)
        return a if a is ERR or a is ORDER else -a
    if k in ("iff", "add", "sub", "min", "max", "cmp"):
        a, b = (_ev(n[2], X, env), _ev(n[3], X, env)) if k == "cmp" else (_ev(n[1], X, env), _ev(n[2], X, env))
        bad = _bad(a, b)
        if bad:
            return bad
        if k == "iff":
            return a == b
        if k == "add":
            return a + b
        if k == "sub":
            return a - b
        if k == "min":
            return min(a, b)
        if k == "max":
            return max(a, b)
        o = n[1]
        return (a == b if o == "=" else a != b if o in ("#", "/=") else a < b if o == "<" else
                a <= b if o in ("<=", "=<") else a > b if o == ">" else a >= b)
    if k == "if":
        c = _ev(n[1], X, env)
        if c is ERR or c is ORDER:
            return c
        return _ev(n[2] if c else n[3], X, env)
    if k == "nil":
        return rv.NIL
    if k == "q":
        return _quant(n, 0, X, env)
    if k == "lenme":
        m = env[n[1]][1]
        return len(m["mentries"]) if "mentries" in m else ERR
    if k == "ef":
        return env[n[1]][1][n[2]]
    if k == "nelec":
        return len(X[1 + n[1]][rv.IX["elections"]])
    if k == "bagcard":
        return sum(c for _, c in X[1 + n[1]][rv.IX["messages"]].items())
    if k == "mcount":
        m = _ev(n[2], X, env)
        return m if m is ERR or m is ORDER else X[1 + n[1]][rv.IX["messages"]][m[1]]
    # reads of a function on Server: the index is evaluated first, Nil is outside the domain
    st = X[1 + n[1]] if k in ("len", "term", "value", "entry") else X[1 + n[2]] if k in ("srv", "nm", "card") else \
        X[1 + n[3]]
    if k == "vin":
        j, i = _ev(n[1], X, env), _ev(n[4], X, env)
        bad = _bad(j, i)
        if bad:
            return bad
        return ERR if i == rv.NIL else j in st[rv.IX[n[2]]][i]
    if k in ("srv", "card"):
        i = _ev(n[3], X, env)
        if i is ERR or i is ORDER:
            return i
        if i == rv.NIL:
            return ERR
        v = st[rv.IX[n[1]]][i]
        return len(v) if k == "card" else v
    if k == "len":
        i = _ev(n[2], X, env)
        if i is ERR or i is ORDER:
            return i
        return ERR if i == rv.NIL else len(st[rv.IX["log"]][i])
    if k in ("term", "value", "entry"):
        i, x = _ev(n[2], X, env), _ev(n[3], X, env)
        bad = _bad(i, x)
        if bad:
            return bad
        if i == rv.NIL:
            return ERR
        lg = st[rv.IX["log"]][i]
        if not 1 <= x <= len(lg):
            return ERR
        return lg[x - 1] if k == "entry" else lg[x - 1][k]
    if k == "nm":
        i, j = _ev(n[3], X, env), _ev(n[4], X, env)
        bad = _bad(i, j)
        if bad:
            return bad
        return ERR if i == rv.NIL or j == rv.NIL else st[rv.IX[n[1]]][i][j]
    raise ValueError(k)


_FLAT = {}


def _quant(n, at, X, env):
    """Binder `at` of a quantifier's flattened variable list, then the body."""
    flat = _FLAT.get(id(n))
    if flat is None:
        flat = _FLAT[id(n)] = ([(name, dom) for names, dom in n[2] for name in names], n)  # (n: keeps the id alive)
    flat = flat[0]
    if at == len(flat):
        return _ev(n[3], X, env)
    name, dom = flat[at]
    all_ = n[1] == "A"
    if dom[0] in ("Server", "range"):
        if dom[0] == "Server":
            items = range(X[0].n_server)
        else:
            lo, hi = _ev(dom[1], X, env), _ev(dom[2], X, env)
            bad = _bad(lo, hi)
            if bad:
                return bad
            assert lo > hi or (0 <= lo and hi <= 15), "the generator keeps ranges inside 0..15"
            items = range(lo, hi + 1)
        for v in items:  # ascending, to the first deciding element
            env[name] = v
            r = _quant(n, at + 1, X, env)
            if r is ERR or r is ORDER:
                return r
            if r != all_:
                return r
        return all_
    # DOMAIN messages / elections: the order is the row encoding's, not the state's -- every element
    st = X[1 + dom[1]]
    if dom[0] == "msgs":
        items = [(dom[1], m) for m in st[rv.IX["messages"]].domain()]
    else:
        items = [(dom[1], e) for e in st[rv.IX["elections"]]]
    res = []
    for v in items:
        env[name] = v
        res.append(_quant(n, at + 1, X, env))
    if any(r is ORDER for r in res):
        return ORDER
    errs = any(r is ERR for r in res)
    decides = any(r is not ERR and r != all_ for r in res)
    if errs:
        return ORDER if decides else ERR
    return (not all_) if decides else all_


def evaluate(node, cfg, s, t=None):
    """TRUE, FALSE, ERR or ORDER of a definition's expression on the state s (an action's: on the step s -> t).
    ORDER: the outcome depends on the order in which a bag's or the election set's elements are visited."""
    r = _ev(node, (cfg, s, t), {})
    return r if r is ERR or r is ORDER else TRUE if r else FALSE


# ---------------------------------------------------------------- the generator

# Guard probabilities, tuned on the reference (tests/test_predfuzz_host.py states the conditions).  A state
# definition guards a per-type field with P_GUARD (unguarded under a bag quantifier the outcome is mostly ORDER)
# and log[i][n] / f[votedFor[i]] with P_GUARD_SERVER (unguarded under a Server quantifier: ERR).  An action
# definition always guards: one error among a parent's thirty-odd steps takes the parent out of its set's
# comparison.  The error witnesses are the "bare" definitions, which never guard the latter two; they are the last
# of the corpus, so that the rows they lose are lost to the last sets only.
P_GUARD = 0.97
P_GUARD_SERVER = 0.93


class Ctx:
    def __init__(self, action):
        self.action = action
        self.vars = []      # (name, type, row)
        self.mtype = {}     # message variable -> its known type
        self.logok = []     # (p, i, n): n is known to lie in 1..Len(log<p>[i])
        self.voted = []     # (p, i): votedFor<p>[i] is known not to be Nil
        self.nonneg = set() # integer variables (all are within 0..15)

    def copy(self):
        c = Ctx(self.action)
        c.vars, c.mtype, c.logok, c.voted = list(self.vars), dict(self.mtype), list(self.logok), list(self.voted)
        return c

    def of(self, type_):
        return [v for v in self.vars if v[1] == type_]


class Gen:
    def __init__(self, seed, N=2, T=3, L=2):
        self.r = Stream(seed)
        self.N, self.T, self.L = N, T, L   # the smallest of the shapes' bounds: literals are drawn below them
        self.used = {}                     # feature -> draws, to prefer what the corpus lacks
        self.fresh = 0
        self.profile, self.deep_pending = None, False

    # -- choice, weighted against what was drawn often
    def choose(self, options):
        """options: [(key, weight)] -> key.  A key's weight falls with the times it was chosen."""
        tot, acc = 0, []
        for key, w in options:
            w = max(1, int(1000 * w / (1 + self.used.get(key, 0))))
            tot += w
            acc.append((tot, key))
        x = self.r.below(tot)
        for edge, key in acc:
            if x < edge:
                self.used[key] = self.used.get(key, 0) + 1
                return key
        raise AssertionError

    def p(self, c, what=""):
        """The row a read of `what` takes: in an action, the one the corpus has read it from less often."""
        if not c.action:
            return 0
        return int(self.choose([("row 0 " + what, 1.0), ("row 1 " + what, 1.0)])[4])

    def name(self, stem):
        self.fresh += 1
        return "%s%d" % (stem, self.fresh)

    # -- servers
    def server(self, c, b, index=True):
        """A server expression; index: it will index a function, so it must not be Nil."""
        opts = [("var", 6.0 * bool(c.of(SERVER))), ("msrc", 1.0 * bool(c.of(MSG))), ("mdst", 1.0 * bool(c.of(MSG))),
                ("eleader", 1.5 * bool(c.of(ELEC))), ("ifs", 0.4 * (b >= 4 and bool(c.of(SERVER))))]
        if index:
            opts += [("votedidx", 1.0 * bool(c.voted)), ("votedbare", 0.08 * (self.profile == "bare" and bool(c.of(SERVER))))]
        else:
            opts += [("voted", 2.0 * bool(c.of(SERVER))), ("nil", 0.7)]
        opts = [(k, w) for k, w in opts if w > 0]
        if not opts:
            return None
        k = self.choose(opts)
        if k == "var":
            return ("var", self.r.pick(c.of(SERVER))[0])
        if k in ("msrc", "mdst"):
            return ("mf", self.r.pick(c.of(MSG))[0], "msource" if k == "msrc" else "mdest")
        if k == "eleader":
            return ("ef", self.r.pick(c.of(ELEC))[0], "eleader")
        if k == "votedidx":
            p, i = self.r.pick(c.voted)
            return ("srv", "votedFor", p, i)
        if k in ("voted", "votedbare"):
            return ("srv", "votedFor", self.p(c, "votedFor"), ("var", self.r.pick(c.of(SERVER))[0]))
        if k == "nil":
            return ("nil",)
        return ("if", self.boolean(c, b // 3), self.server(c, 1, index), self.server(c, 1, index))

    # -- integers
    def lit(self, fam):
        hi = {"term": self.T + 1, "index": self.L + 1, "count": 3, "any": 4}[fam]
        return ("num", self.r.below(hi + 1))

    def integer(self, c, b, fam="any"):
        if fam == "any":
            fam = self.r.pick(["term", "index", "count"])
        if b >= 3:
            if self.profile == "deep":
                k = self.r.pick(["add", "sub", "add", "sub", "min", "max"])
            else:
                k = self.choose([("atom", 1.0), ("add", 1.0), ("sub", 1.0), ("neg", 0.5), ("min", 0.7), ("max", 0.7),
                                 ("ifi", 0.7)])
            if k in ("add", "sub", "min", "max"):
                lb = 1 + self.r.below(b - 2) if not self.r.chance(0.6) and self.profile != "deep" else 1
                return (k, self.integer(c, lb, fam), self.integer(c, b - 1 - lb, fam))
            if k == "neg":
                return ("neg", self.integer(c, b - 1, fam))
            if k == "ifi":
                return ("if", self.boolean(c, b // 3), self.integer(c, b // 3, fam), self.integer(c, b // 3, fam))
        return self.int_atom(c, fam)

    def int_atom(self, c, fam):
        srv = bool(c.of(SERVER)) or bool(c.of(MSG)) or bool(c.of(ELEC))
        ints = c.of(INT)
        msgs = c.of(MSG)
        opts = [("lit", 1.2), ("ivar", 2.0 * bool(ints))]
        if self.profile == "deep" and self.r.chance(0.6):
            return self.lit(fam)
        if fam == "term":
            opts += [("currentTerm", 3.0 * srv), ("logterm", 2.0 * bool(c.logok)), ("mterm", 2.0 * bool(msgs)),
                     ("eterm", 2.0 * bool(c.of(ELEC)))]
            opts += [("f:" + f, 1.5) for f in ("mlastLogTerm", "mprevLogTerm") if self.field_ok(c, f)]
        elif fam == "index":
            opts += [("commitIndex", 2.0 * srv), ("len", 2.0 * srv), ("nextIndex", 1.5 * srv),
                     ("matchIndex", 1.5 * srv)]
            opts += [("f:" + f, 1.5) for f in ("mlastLogIndex", "mprevLogIndex", "mcommitIndex", "mmatchIndex")
                     if self.field_ok(c, f)]
        else:
            opts += [("votesResponded", 1.5 * srv), ("votesGranted", 1.5 * srv), ("nelec", 1.0), ("bagcard", 1.0),
                     ("mcount", 1.5 * bool(msgs))]
            opts += [("f:mentries", 1.5)] if self.field_ok(c, "mentries") else []
        k = self.choose([(k, w) for k, w in opts if w > 0])
        if k == "lit":
            return self.lit(fam)
        if k == "ivar":
            return ("var", self.r.pick(ints)[0])
        if k in ("currentTerm", "commitIndex"):
            return ("srv", k, self.p(c, k), self.server(c, 1))
        if k == "len":
            return ("len", self.p(c, "log"), self.server(c, 1))
        if k in ("nextIndex", "matchIndex"):
            return ("nm", k, self.p(c, k), self.server(c, 1), self.server(c, 1))
        if k in ("votesResponded", "votesGranted"):
            return ("card", k, self.p(c, k), self.server(c, 1))
        if k == "logterm":
            p, i, n = self.r.pick(c.logok)
            return ("term", p, i, n)
        if k == "mterm":
            return ("mf", self.r.pick(msgs)[0], "mterm")
        if k == "eterm":
            return ("ef", self.r.pick(c.of(ELEC))[0], "eterm")
        if k == "nelec":
            return ("nelec", self.p(c, "elections"))
        if k == "bagcard":
            return ("bagcard", self.p(c, "messages"))
        if k == "mcount":
            m = self.r.pick(msgs)
            return ("mcount", m[2], ("var", m[0]))
        f = k[2:]
        m = self.r.pick([v for v in msgs if c.mtype.get(v[0]) == MFIELDS[f][1]])
        return ("lenme", m[0]) if f == "mentries" else ("mf", m[0], f)

    def field_ok(self, c, f):
        return any(c.mtype.get(v[0]) == MFIELDS[f][1] for v in c.of(MSG))

    # -- Booleans
    def boolean(self, c, b):
        if self.profile == "nest" and len(c.vars) < 5 + self.r.below(2):
            return self.quant(c, b)
        if b >= 4:
            k = self.choose([("and", 2.0), ("or", 1.5), ("imp", 1.5), ("iff", 1.0), ("not", 0.8), ("q", 3.0),
                             ("ifb", 0.5), ("atom", 2.0)])
            if k in ("and", "or", "imp", "iff"):
                lb = 1 + self.r.below(b - 2)
                return (k, self.boolean(c, lb), self.boolean(c, b - 1 - lb))
            if k == "not":
                return ("not", self.boolean(c, b - 1))
            if k == "ifb":
                return ("if", self.boolean(c, b // 3), self.boolean(c, b // 3), self.boolean(c, b // 3))
            if k == "q":
                return self.quant(c, b - 1)
        if not c.vars and b >= 2:
            return self.quant(c, b)
        return self.atom(c, b)

    def quant(self, c, b):
        if len(c.vars) >= 6:
            return self.atom(c, b)
        q = self.choose([("A", 1.0), ("E", 1.0)])
        c = c.copy()
        groups, pending = [], []
        room = 6 - len(c.vars)
        ngroups = 1 if room < 2 or not self.r.chance(0.2) or self.profile == "nest" else 2
        for g in range(ngroups):
            servers = bool(c.of(SERVER))
            opts = [("Server", 3.0 if not servers else 1.2), ("msgs", 1.6), ("elecs", 1.0), ("range", 1.0),
                    ("logrange", 1.5 * (servers and not groups))]
            if c.action:
                opts += [("msgs'", 1.6), ("elecs'", 1.0)]
            if self.profile == "nest" and c.of(MSG):   # (one bag at the most: the step bound)
                opts = [(k, w) for k, w in opts if not k.startswith("msgs")]
            d = self.choose([(k, w) for k, w in opts if w])
            if not servers and (self.profile == "bare" or self.r.chance(0.45)):
                d = "Server"   # (most reads need a server)
            elif not c.of(MSG) and self.profile is None and self.r.chance(0.3):
                d = "msgs'" if c.action and self.r.chance(0.5) else "msgs"
            many = 2 if room - (ngroups - 1 - g) >= 2 and d in ("Server", "msgs", "msgs'") and self.r.chance(0.15) else 1
            stem = {"Server": "i", "msgs": "m", "msgs'": "m", "elecs": "e", "elecs'": "e"}.get(d, "n")
            names = [self.name(stem) for _ in range(many)]
            if d == "Server":
                dom, ty, row = ("Server",), SERVER, 0
            elif d in ("msgs", "msgs'"):
                dom, ty, row = ("msgs", int(d[-1] == "'")), MSG, int(d[-1] == "'")
            elif d in ("elecs", "elecs'"):
                dom, ty, row = ("elecs", int(d[-1] == "'")), ELEC, int(d[-1] == "'")
            elif d == "range":
                lo = self.r.below(3)
                dom, ty, row = ("range", ("num", lo), ("num", lo + self.r.below(3))), INT, 0
            else:  # 1..Len(log[i]) (or the least of two logs): log[i][n] is in its domain
                p = self.p(c)
                i = ("var", self.r.pick(c.of(SERVER))[0])
                hi = ("len", p, i)
                facts = [(p, i)]
                if len(c.of(SERVER)) > 1 and self.r.chance(0.4):
                    p2, j = self.p(c), ("var", self.r.pick(c.of(SERVER))[0])
                    hi = ("min", hi, ("len", p2, j))
                    facts.append((p2, j))
                dom, ty, row = ("range", ("num", 1), hi), INT, 0
                for fp, fi in facts:
                    c.logok.append((fp, fi, ("var", names[0])))
            groups.append((names, dom))
            pending += [(nm, ty, row) for nm in names]
            room -= many
        c.vars += pending  # (a group's domain does not see the variables of its own quantifier)
        return ("q", q, groups, self.boolean(c, max(1, b - len(groups))))

    def ibudget(self):
        return self.r.pick([1, 1, 2, 3, 5, 8])

    def compare(self, c, left, fam):
        """`left` against an integer of its family, on either side."""
        op = self.choose([("cmp " + o, 1.0) for o in CMP_ALL])[4:]
        other = self.integer(c, self.ibudget(), fam)
        return ("cmp", op, left, other) if self.r.chance(0.6) else ("cmp", op, other, left)

    def forced(self, c, force):
        """An atom that reads what a planned guard protects."""
        eq = lambda: self.choose([("cmp " + o, 1.0) for o in CMP_EQ])[4:]
        if force[0] == "field":
            _, m, ty = force
            f = self.choose([("field " + f, 1.0) for f, d in MFIELDS.items() if d[1] == ty])[6:]
            if MFIELDS[f][0] == BOOL:
                return ("mf", m, f) if self.r.chance(0.7) else ("not", ("mf", m, f))
            return self.compare(c, ("lenme", m) if f == "mentries" else ("mf", m, f), MFIELDS[f][2])
        if force[0] == "log":
            _, p, i, n = force
            k = self.choose([("log term", 1.0), ("log value", 1.0), ("log entry", 1.0)])[4:]
            if k == "term":
                return self.compare(c, ("term", p, i, n), "term")
            # another server's entry at the same position where it has one (n >= 1 is known), else this one
            p2, j = self.p(c), ("var", self.r.pick(c.of(SERVER))[0])
            other = ("if", ("cmp", "<=", n, ("len", p2, j)), (k, p2, j, n), (k, p, i, n))
            return ("cmp", eq(), (k, p, i, n), other)
        _, p, i = force
        vf = ("srv", "votedFor", p, i)
        k = self.choose([("via currentTerm", 1.0), ("via commitIndex", 1.0), ("via state", 1.0), ("via len", 1.0),
                         ("via nextIndex", 1.0), ("via vin", 1.0), ("via card", 1.0)])[4:]
        if k == "currentTerm":
            return self.compare(c, ("srv", k, self.p(c, k), vf), "term")
        if k == "commitIndex":
            return self.compare(c, ("srv", k, self.p(c, k), vf), "index")
        if k == "len":
            return self.compare(c, ("len", self.p(c), vf), "index")
        if k == "nextIndex":
            which = self.r.pick(["nextIndex", "matchIndex"])
            return self.compare(c, ("nm", which, self.p(c, which), vf, i) if self.r.chance(0.5) else
                                ("nm", which, self.p(c, which), i, vf), "index")
        if k == "card":
            return self.compare(c, ("card", self.r.pick(["votesResponded", "votesGranted"]), self.p(c), vf), "count")
        if k == "vin":
            return ("vin", i, self.r.pick(["votesResponded", "votesGranted"]), self.p(c), vf)
        return ("cmp", eq(), ("srv", "state", self.p(c), vf), self.typed(c, STATE, 1))

    def delta(self, c):
        """An action's atom: a variable's value after the step against its value before."""
        servers = [("var", v[0]) for v in c.of(SERVER)]
        opts = [("delta messages", 1.0), ("delta elections", 1.0)]
        if servers:
            opts += [("delta " + f, 1.0) for f in ("currentTerm", "state", "votedFor", "commitIndex", "log", "nextIndex",
                                                   "matchIndex", "votesResponded", "votesGranted")]
        f = self.choose(opts)[6:]
        op = self.choose([("cmp " + o, 1.0) for o in CMP_ALL])[4:]
        eq = self.choose([("cmp " + o, 1.0) for o in CMP_EQ])[4:]
        if f == "messages":
            return ("cmp", op, ("bagcard", 1), ("bagcard", 0))
        if f == "elections":
            return ("cmp", op, ("nelec", 1), ("nelec", 0))
        i, j = self.r.pick(servers), self.r.pick(servers)
        if f in ("currentTerm", "commitIndex"):
            return ("cmp", op, ("srv", f, 1, i), ("srv", f, 0, i))
        if f in ("state", "votedFor"):
            return ("cmp", eq, ("srv", f, 1, i), ("srv", f, 0, i))
        if f == "log":
            return ("cmp", op, ("len", 1, i), ("len", 0, i))
        if f in ("nextIndex", "matchIndex"):
            return ("cmp", op, ("nm", f, 1, i, j), ("nm", f, 0, i, j))
        if self.r.chance(0.5):
            return ("cmp", op, ("card", f, 1, i), ("card", f, 0, i))
        return ("imp", ("vin", j, f, 0, i), ("vin", j, f, 1, i))

    def atom(self, c, b, force=None):
        """A comparison, a membership or a Boolean field, guarded where it could err."""
        for _ in range(4):
            a = self.atom1(c, b, force)
            if not (a[0] == "cmp" and a[2] == a[3]):   # (x = x: constant)
                break
        return a

    def atom1(self, c, b, force):
        b = max(b, 1)
        if self.deep_pending:   # the deep profile: one right-nested integer chain
            self.deep_pending = False
            fam = self.r.pick(["term", "index", "count"])
            return ("cmp", self.r.pick(CMP_ALL), self.integer(c, 1, fam), self.integer(c, 30, fam))
        if force:
            return self.forced(c, force)
        msgs = c.of(MSG)
        unknown = [v for v in msgs if v[0] not in c.mtype]
        srv = bool(c.of(SERVER)) or bool(msgs) or bool(c.of(ELEC))
        # plan a guard first: the comparison below is generated under what the guard makes known
        if unknown and self.r.chance(0.7):
            m = self.r.pick(unknown)
            ty = self.choose([("guard " + t, sum(1.0 for d in MFIELDS.values() if d[1] == t)) for t in MTYPES])[6:]
            c2 = c.copy()
            c2.mtype[m[0]] = ty
            inner = self.atom(c2, b, ("field", m[0], ty) if self.r.chance(0.85) else None)
            g = ("cmp", "=", ("mf", m[0], "mtype"), ("const", ty))
            if not (c.action or self.r.chance(P_GUARD)):
                return inner
            if self.r.chance(0.2):  # the guard spelled as the negation's disjunct
                return ("or", ("cmp", self.r.pick(["#", "/="]), ("mf", m[0], "mtype"), ("const", ty)), inner)
            return (self.r.pick(["imp", "and"]), g, inner)
        bare = self.profile == "bare"
        if c.of(SERVER) and self.r.chance(0.6 if bare else 0.25):   # a log position
            p = self.p(c)
            i = ("var", self.r.pick(c.of(SERVER))[0])
            ints = [v for v in c.of(INT)]
            n = ("var", self.r.pick(ints)[0]) if ints and self.r.chance(0.5) else ("num", 1 + self.r.below(2))
            c2 = c.copy()
            c2.logok.append((p, i, n))
            inner = self.atom(c2, b, ("log", p, i, n) if self.r.chance(0.75) else None)
            if bare or not (c.action or self.r.chance(P_GUARD_SERVER)):
                return inner
            g = ("cmp", self.r.pick(["<=", "=<"]), n, ("len", p, i))
            if n[0] == "var":
                g = ("and", ("cmp", ">=", n, ("num", 1)), g)
            return (self.r.pick(["imp", "and"]), g, inner)
        if c.of(SERVER) and self.r.chance(0.6 if bare else 0.12):   # f[votedFor[i]]
            p = self.p(c)
            i = ("var", self.r.pick(c.of(SERVER))[0])
            c2 = c.copy()
            c2.voted.append((p, i))
            inner = self.atom(c2, b, ("voted", p, i) if self.r.chance(0.75) else None)
            if bare or not (c.action or self.r.chance(P_GUARD_SERVER)):
                return inner
            g = ("cmp", self.r.pick(["#", "/="]), ("srv", "votedFor", p, i), ("nil",))
            return (self.r.pick(["imp", "and"]), g, inner)
        bools = [f for f in ("mvoteGranted", "msuccess") if self.field_ok(c, f)]
        opts = [("int", 4.0), ("server", 2.0 * srv), ("state", 2.0 * srv), ("mtype", 1.5 * bool(msgs)),
                ("vin", 2.0 * bool(c.of(SERVER))), ("entry", 1.5 * bool(c.logok)), ("value", 1.5 * bool(c.logok)),
                ("msg", 1.0 * (len(msgs) > 1)), ("elec", 1.0 * (len(c.of(ELEC)) > 1)), ("bfield", 2.5 * bool(bools)),
                ("booleq", 0.3 * (b >= 3)), ("const", 0.25)]
        if c.action and self.r.chance(0.35):
            return self.delta(c)
        k = self.choose([(k, w) for k, w in opts if w > 0])
        if k == "int":
            fam = self.r.pick(["term", "index", "count"])
            op = self.choose([("cmp " + o, 1.0) for o in CMP_ALL])[4:]
            return ("cmp", op, self.integer(c, self.ibudget(), fam), self.integer(c, self.ibudget(), fam))
        eq = lambda: self.choose([("cmp " + o, 1.0) for o in CMP_EQ])[4:]
        if k == "server":
            return ("cmp", eq(), self.server(c, b // 2, True), self.server(c, b // 2, False))
        if k == "state":
            return ("cmp", eq(), self.typed(c, STATE, b // 2, read=True), self.typed(c, STATE, b // 2))
        if k == "mtype":
            return ("cmp", eq(), self.typed(c, MTYPE, b // 2, read=True), self.typed(c, MTYPE, b // 2))
        if k == "vin":
            which = self.choose([("votesResponded", 1.0), ("votesGranted", 1.0)])
            return ("vin", self.server(c, 1, False), which, self.p(c, which), self.server(c, 1))
        if k in ("entry", "value"):
            return ("cmp", eq(), self.typed(c, ENTRY if k == "entry" else VALUE, b // 2),
                    self.typed(c, ENTRY if k == "entry" else VALUE, b // 2))
        if k in ("msg", "elec"):
            ty = MSG if k == "msg" else ELEC
            a = self.r.pick(c.of(ty))
            same = [v for v in c.of(ty) if v[2] == a[2]]
            if len(same) < 2:
                return ("cmp", eq(), ("var", a[0]), ("var", a[0]))
            x = self.typed(c, ty, b // 2, row=a[2])
            return ("cmp", eq(), x, ("var", self.r.pick(same)[0]))
        if k == "bfield":
            f = self.r.pick(bools)
            m = self.r.pick([v for v in msgs if c.mtype.get(v[0]) == MFIELDS[f][1]])
            return ("mf", m[0], f)
        if k == "booleq":
            return ("cmp", eq(), self.boolean(c, b // 2), self.boolean(c, b // 2))
        return (self.choose([("true", 1.0), ("false", 1.0)]),)

    def typed(self, c, ty, b, row=0, read=False):
        """A server state, message type, entry, value, message or election (read: no constant if it can be helped)."""
        if b >= 4 and self.r.chance(0.3):
            return ("if", self.boolean(c, b // 3), self.typed(c, ty, 1, row, read), self.typed(c, ty, 1, row))
        if ty == STATE:
            if not read and self.r.chance(0.45):
                return ("const", self.choose([("s" + s, 1.0) for s in STATES])[1:])
            i = self.server(c, 1)
            return ("srv", "state", self.p(c, "state"), i) if i else ("const", rv.LEADER)
        if ty == MTYPE:
            if not c.of(MSG) or (not read and self.r.chance(0.6)):
                return ("const", self.choose([("t" + s, 1.0) for s in MTYPES])[1:])
            return ("mf", self.r.pick(c.of(MSG))[0], "mtype")
        if ty in (ENTRY, VALUE):
            p, i, n = self.r.pick(c.logok)
            return ("entry" if ty == ENTRY else "value", p, i, n)
        return ("var", self.r.pick([v for v in c.of(ty) if v[2] == row])[0])

    def define(self, action, budget, profile=None):
        """profile: None; "deep": one comparison holds a right-nested chain of about 14 integer operators;
        "nest": five or six quantifiers, one inside the other; "bare": log[i][n] and f[votedFor[i]] unguarded."""
        self.profile, self.deep_pending = profile, profile == "deep"
        tree = self.boolean(Ctx(action), budget)
        self.profile, self.deep_pending = None, False
        return tree


def corpus(seed, n_state, n_action, limits=(5, 20, 10), max_words=58, max_cost=6000):
    """[(name, tree, is_action)]: n_state state definitions, then n_action action definitions, each within the
    language's limits at a layout of at most `limits` = (N, K, E); max_cost (the compiler's worst-case steps,
    2^17 a definition if eight are to fit a set) is far lower: the Python evaluator visits every element of a bag."""
    g = Gen(seed)
    out = []
    for action, n, stem in ((False, n_state, "S"), (True, n_action, "A")):
        made = 0
        while made < n:
            saved = dict(g.used)
            budget = ([9, 12, 16, 22, 22] if action else [6, 9, 12, 16, 22])[g.r.below(5)]
            profile = {5: "deep", 11: "nest"}.get(made % 16)
            if made >= n - (8 if action else 16):   # the last sets: an erring row leaves its set's comparison
                profile = "bare"
            tree = g.define(action, budget if profile in (None, "bare") else 4, profile)
            if (depth(tree) > 16 or depth(tree, True) > 16 or nvars(tree) > 6 or words(tree) > max_words
                    or cost(tree, *limits) > (max_cost if profile != "nest" else 1 << 16)):
                g.used = saved
                continue
            if action and not any("'" in f for f in census(tree)):
                g.used = saved
                continue
            out.append(("%s%03d" % (stem, made), tree, action))
            made += 1
    return out


SEED = 0x7072656466757a7e  # (of six neighbouring seeds the one whose census has the widest margin)
N_STATE, N_ACTION = 160, 64
_STANDARD = []


def standard_corpus():
    """The corpus of tests/test_predfuzz_host.py and tests/test_predfuzz_gpu.py (and the sample the sanitizer
    programs of tests/test_pred_host.py and tests/test_step_host.py compile): generated once."""
    if not _STANDARD:
        _STANDARD.extend(corpus(SEED, N_STATE, N_ACTION))
    return _STANDARD
