"""CPU tests of the user-defined predicates: the compiler (rtla_pred.cpp) and
the interpreter on the host (rtla_pred_replay).  No kernel is launched.

The five built-ins restated in the language (specs/MCPredicates.tla) are pinned
to rtla_check_replay, which has its own oracle (tests/test_safety_host.py); the
fields no built-in reads are pinned by predicates paired with Python functions
over value-oracle states, written from the TLA+ text alone."""
import os
import shutil
import subprocess

import pytest

import limits
import predgen
import raft_values as rv
import rtla
from test_safety_host import ALL, SHAPES, py_mask
from test_safety_host import setup as make_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MCPRED = open(os.path.join(ROOT, "specs", "MCPredicates.tla")).read()
RESTATED = {"P" + n: n for n in ALL}


@pytest.fixture(scope="module", params=SHAPES, ids=lambda p: "n%d" % p[0][0])
def case(request):
    return make_case(*request.param)


def test_builtins_restated_equal_check_replay(case):
    cfg, _, rows, _ = case
    with rtla.Predicates(cfg, MCPRED) as preds:
        assert preds.names[:5] == ["P" + n for n in ALL] and len(preds.names) == 8
        masks, counts = rtla.pred_replay(preds, rows)
    want_masks, want_counts = rtla.check_replay(cfg, rows, ALL)
    bit = {k: rtla.INV_BITS[RESTATED[n]] for k, n in enumerate(preds.names[:5])}
    assert [sum(b for k, b in bit.items() if m >> k & 1) for m in masks] == want_masks  # mask for mask
    assert {RESTATED[n]: counts[n] for n in RESTATED} == want_counts                    # count for count
    assert sum(want_counts.values()) > 0


# ---- fields the built-ins never read: (name, text, the same in Python from the TLA+ text)

def _v(s, name):
    return s[rv.IX[name]]


def _msgs(s):
    return list(_v(s, "messages").items())  # [(message record, count)]


def _servers(c):
    return range(c.n_server)


FIELD_PREDICATES = [
    ("SomeoneHasNotVoted", r"\E i \in Server : votedFor[i] = Nil",
     lambda c, s: any(_v(s, "votedFor")[i] == rv.NIL for i in _servers(c))),
    ("VotedForAnother", r"\A i \in Server : votedFor[i] # Nil => votedFor[i] # i",
     lambda c, s: all(_v(s, "votedFor")[i] == rv.NIL or _v(s, "votedFor")[i] != i for i in _servers(c))),
    ("CandidatesCountThemselves", r"\A i \in Server : state[i] = Candidate => i \in votesGranted[i]",
     lambda c, s: all(_v(s, "state")[i] != rv.CANDIDATE or i in _v(s, "votesGranted")[i] for i in _servers(c))),
    ("EveryResponseGranted",
     r"\A i, j \in Server : j \in votesResponded[i] => j \in votesGranted[i]",
     lambda c, s: all(j not in _v(s, "votesResponded")[i] or j in _v(s, "votesGranted")[i]
                      for i in _servers(c) for j in _servers(c))),
    ("AtMostOneRefusal",
     r"\A i \in Server : Cardinality(votesGranted[i]) + 1 >= Cardinality(votesResponded[i])",
     lambda c, s: all(len(_v(s, "votesGranted")[i]) + 1 >= len(_v(s, "votesResponded")[i]) for i in _servers(c))),
    ("NextAboveMatch", r"\A i, j \in Server : nextIndex[i][j] > matchIndex[i][j]",
     lambda c, s: all(_v(s, "nextIndex")[i][j] > _v(s, "matchIndex")[i][j] for i in _servers(c) for j in _servers(c))),
    ("NoSelfAddressedMessage", r"\A m \in DOMAIN messages : m.msource # m.mdest",
     lambda c, s: all(m["msource"] != m["mdest"] for m, _ in _msgs(s))),
    ("MessagesWithinDestTerm", r"\A m \in DOMAIN messages : m.mterm <= currentTerm[m.mdest]",
     lambda c, s: all(m["mterm"] <= _v(s, "currentTerm")[m["mdest"]] for m, _ in _msgs(s))),
    ("SingleCopies", r"\A m \in DOMAIN messages : messages[m] = 1",
     lambda c, s: all(n == 1 for _, n in _msgs(s))),
    ("VoteRequestsCarryTheLog",
     r"\A m \in DOMAIN messages : m.mtype = RequestVoteRequest => "
     r"(m.mlastLogIndex = Len(log[m.msource]) /\ m.mlastLogTerm <= m.mterm)",
     lambda c, s: all(m["mtype"] != rv.RVREQ or (m["mlastLogIndex"] == len(_v(s, "log")[m["msource"]])
                                                  and m["mlastLogTerm"] <= m["mterm"]) for m, _ in _msgs(s))),
    ("SomeVoteGranted", r"\E m \in DOMAIN messages : m.mtype = RequestVoteResponse /\ m.mvoteGranted",
     lambda c, s: any(m["mtype"] == rv.RVRESP and m["mvoteGranted"] for m, _ in _msgs(s))),
    ("AppendRequestsAreConsistent",
     r"\A m \in DOMAIN messages : m.mtype = AppendEntriesRequest => "
     r"((m.mprevLogIndex = 0 <=> m.mprevLogTerm = 0) /\ m.mcommitIndex <= m.mprevLogIndex + Len(m.mentries))",
     lambda c, s: all(m["mtype"] != rv.AEREQ or (((m["mprevLogIndex"] == 0) == (m["mprevLogTerm"] == 0))
                                                  and m["mcommitIndex"] <= m["mprevLogIndex"] + len(m["mentries"]))
                      for m, _ in _msgs(s))),
    ("FailedAppendsMatchNothing",
     r"\A m \in DOMAIN messages : m.mtype = AppendEntriesResponse => (m.msuccess \/ m.mmatchIndex = 0)",
     lambda c, s: all(m["mtype"] != rv.AERESP or m["msuccess"] or m["mmatchIndex"] == 0 for m, _ in _msgs(s))),
    ("OneTermPerSenderAndType",
     r"\A m1, m2 \in DOMAIN messages : (m1.mtype = m2.mtype /\ m1.msource = m2.msource) => m1.mterm = m2.mterm",
     lambda c, s: all(a["mtype"] != b["mtype"] or a["msource"] != b["msource"] or a["mterm"] == b["mterm"]
                      for a, _ in _msgs(s) for b, _ in _msgs(s))),
    ("QuietOrElected", r"BagCardinality(messages) <= 6 \/ Cardinality(elections) >= 2",
     lambda c, s: sum(n for _, n in _msgs(s)) <= 6 or len(_v(s, "elections")) >= 2),
    ("ElectedStillLeads", r"\E e \in elections : e.eterm >= 2 /\ state[e.eleader] = Leader",
     lambda c, s: any(e["eterm"] >= 2 and _v(s, "state")[e["eleader"]] == rv.LEADER for e in _v(s, "elections"))),
    ("CommitWithinLog",
     r"\A i \in Server : (IF state[i] = Leader THEN commitIndex[i] ELSE Min(commitIndex[i], 1)) "
     r"<= Max(Len(log[i]) - 1, 0)",
     lambda c, s: all((_v(s, "commitIndex")[i] if _v(s, "state")[i] == rv.LEADER else min(_v(s, "commitIndex")[i], 1))
                      <= max(len(_v(s, "log")[i]) - 1, 0) for i in _servers(c))),
]
FIELD_SETS = [FIELD_PREDICATES[:8], FIELD_PREDICATES[8:16], FIELD_PREDICATES[16:]]  # at most 8 definitions a set
FRACTION = {}  # name -> the fraction of rows on which it is true, per shape


def test_field_predicates_match_the_python_functions(case):
    cfg, vc, rows, states = case
    for group in FIELD_SETS:
        text = "\n".join("%s == %s" % (name, src) for name, src, _ in group)
        with rtla.Predicates(cfg, text) as preds:
            assert preds.names == [name for name, _, _ in group]
            masks, counts = rtla.pred_replay(preds, rows)
        for k, (name, _, fn) in enumerate(group):
            want = [fn(vc, s) for s in states]
            assert [not (m >> k & 1) for m in masks] == want, name
            assert counts[name] == want.count(False)
            FRACTION.setdefault(name, []).append(want.count(True) / len(want))


def test_field_predicates_take_both_values():
    """Each predicate is true on >= 5 % and false on >= 5 % of the rows of at
    least one shape (from the Python side alone): none is constant on the generator."""
    assert len(FIELD_PREDICATES) >= 10
    for name, _, _ in FIELD_PREDICATES:
        fr = FRACTION[name]
        assert len(fr) == len(SHAPES) and any(0.05 <= f <= 0.95 for f in fr), (name, fr)


# ---- the row format's limits (tests/limits.py): the interpreter reads every field by the layout

@pytest.mark.parametrize("name", limits.TWO)
def test_limit_shapes_predicates_match_the_python_functions(name):
    """At 3-bit terms with 2-bit values, and at L = 4 with all 64 bag slots and 32 election records: the
    restated built-ins against the Python predicates of test_safety_host.py, the field predicates against
    their Python functions, over the sample's rows and a spread of the host model's successor rows in and
    out of the model (terms of T + 1, logs of L + 1 entries, counts of C + 1, full bags)."""
    c = limits.case(name)
    limits.assert_witnessed(c, "pred_replay")
    succ = limits.host_expand(name)
    succ = limits.spread([x for x in succ if not x[3]], 150) + limits.spread([x for x in succ if x[3]], 250)
    rows = list(c.rows) + [r for _, _, _, _, r in succ]
    states = list(c.states) + [c.state_of(k, r) for k, _, _, _, r in succ]
    with rtla.Predicates(c.cfg, MCPRED) as preds:
        masks, counts = rtla.pred_replay(preds, rows)
        bit = {k: rtla.INV_BITS[RESTATED[n]] for k, n in enumerate(preds.names[:5])}
    want = [py_mask(c.vc, s) for s in states]
    assert [sum(b for k, b in bit.items() if m >> k & 1) for m in masks] == want
    assert {RESTATED[n]: counts[n] for n in RESTATED} == {n: sum(1 for w in want if w & b)
                                                          for n, b in rtla.INV_BITS.items()}
    assert all(counts[n] for n in RESTATED), counts
    for group in FIELD_SETS:
        text = "\n".join("%s == %s" % (nm, src) for nm, src, _ in group)
        with rtla.Predicates(c.cfg, text) as preds:
            masks, counts = rtla.pred_replay(preds, rows)
        for k, (nm, _, fn) in enumerate(group):
            want = [fn(c.vc, s) for s in states]
            assert [not (m >> k & 1) for m in masks] == want, nm
            assert counts[nm] == want.count(False)


# ---- evaluation errors

UNGUARDED = [
    (r"\A i \in Server : log[i][1].term >= 1", r"\A i \in Server : Len(log[i]) >= 1 => log[i][1].term >= 1"),
    (r"\A i \in Server : \A n \in 0..Len(log[i]) : log[i][n].term >= 1",
     r"\A i \in Server : \A n \in 1..Len(log[i]) : log[i][n].term >= 1"),
    (r"\A m \in DOMAIN messages : m.mlastLogIndex >= 0",
     r"\A m \in DOMAIN messages : m.mtype = RequestVoteRequest => m.mlastLogIndex >= 0"),
    (r"\A m \in DOMAIN messages : ~ m.msuccess \/ m.mtype = AppendEntriesResponse",
     r"\A m \in DOMAIN messages : m.mtype # AppendEntriesResponse \/ ~ m.msuccess \/ TRUE"),
    (r"\A i \in Server : currentTerm[votedFor[i]] >= 1",
     r"\A i \in Server : votedFor[i] # Nil => currentTerm[votedFor[i]] >= 1"),
]


@pytest.mark.parametrize("bad,good", UNGUARDED)
def test_evaluation_errors_are_errors(bad, good):
    cfg, _, rows, _ = make_case(*SHAPES[1])
    with rtla.Predicates(cfg, "P == " + bad) as preds:
        with pytest.raises(rtla.RtlaError) as e:
            rtla.pred_replay(preds, rows)
        assert e.value.status == rtla.E_SPEC and e.value.flags & rtla.CAP_SPEC_ERROR
    with rtla.Predicates(cfg, "P == " + good) as preds:
        masks, counts = rtla.pred_replay(preds, rows)
        assert counts == {"P": 0} and not any(masks)


# ---- compile errors

def nested(depth, body="TRUE", dom=r"DOMAIN messages"):
    return "".join(r"\A m%d \in %s : " % (k, dom) for k in range(depth)) + body


COMPILE_ERRORS = [
    ("P == \\A i \\in Server : term[i] = 1", "1:24: unknown identifier 'term'"),
    ("P == TRUE\nQ == \\A i \\in Server : state[i] + 1 = 2", "2:24: type error: expected integer, found server state"),
    ("P == \\A i \\in Server :\n  state[i] = 1", "2:14: type error"),
    ("P == 1 + 1", "1:6: type error: a definition must be Boolean"),
    ("\n".join("P%d == TRUE" % k for k in range(9)), "9:1: more than 8 definitions"),
    ("P == " + nested(7, dom="Server"), "1:123: more than 6 variables bound at once"),
    ("NoTwoLeaders == TRUE", "1:1: 'NoTwoLeaders' is a built-in invariant's name"),
    ("P == \\A m \\in DOMAIN messages : Len(m.mlog) = 0", "1:39: 'mlog' is not supported"),
    ("P == \\E e \\in elections : e.evotes = e.evotes", "1:29: 'evotes' is not supported"),
    ("P == allLogs = allLogs", "1:6: 'allLogs' is not supported"),
    ("P == \\A i \\in Server : currentTerm'[i] = 1", "1:35: ''' is not supported"),
    ("P == \\A i \\in {1, 2} : TRUE", "1:15: '{' is not supported"),
    ("P == TRUE /\\", "1:13: expected an expression"),
    ("P == (* never closed", "1:6: unterminated comment"),
    ("P == TRUE\nP == FALSE", "2:1: 'P' is defined twice"),
    ("P == \\A i \\in Server : i < i", "1:26: type error"),
    ("P == Min(1) = 1", "1:11: expected ,"),
    # TLA+ has no parse for a chain of => or of <=>
    ("P == TRUE => FALSE => TRUE", "1:20: 'a => b => c' has no parse in TLA+: parenthesise one of the two"),
    ("P == TRUE <=> FALSE\n  <=> TRUE", "2:3: 'a <=> b <=> c' has no parse in TLA+: parenthesise one of the two"),
    ("P == TRUE => FALSE <=> TRUE => FALSE", "1:29: 'a => b => c' has no parse in TLA+"),
]


@pytest.mark.parametrize("text,message", COMPILE_ERRORS)
def test_compile_errors_give_line_and_column(text, message):
    with pytest.raises(rtla.RtlaError) as e:
        rtla.Predicates(rtla.Config(3, 2, 3, 2, 1, 0, ()), text)
    assert e.value.status == rtla.E_ARG
    assert "rtla_pred_compile: " + message in str(e.value), str(e.value)


def test_the_step_bound_is_pinned():
    """Three nested message quantifiers at bag_cap = 64 run their body 64^3 =
    2^18 times.  Worst-case steps of a set: a quantifier
    costs 2 + trips * (body + 1), a definition its body + 1, the program's end
    1 -- with a body of b steps, steps(b) below: a body of 3 steps stays under
    2^20 and one of 5 steps goes over."""
    cfg = rtla.Config(2, 1, 3, 1, 1, 0, (), bag_cap=64)

    def steps(b):
        return 2 + 64 * (3 + 64 * (3 + 64 * (b + 1))) + 2

    def steps2(b):  # the same with two quantifiers
        return 2 + 64 * (3 + 64 * (b + 1)) + 2

    # a first definition of 64^3 bodies of 2 steps, a second of 64^2 bodies of b steps (`~ ... ~ TRUE`: b - 1
    # negations), b the largest that keeps the set (the program's end counted once) within 2^20
    first = nested(3, "~ TRUE")
    b = max(k for k in range(1, 200) if steps(2) + steps2(k) - 1 <= 1 << 20)
    below = "P == %s\nQ == %s" % (first, nested(2, "~ " * (b - 1) + "TRUE"))
    above = "P == %s\nQ == %s" % (first, nested(2, "~ " * b + "TRUE"))
    total = steps(2) + steps2(b + 1) - 1
    assert (1 << 20) - 4096 <= steps(2) + steps2(b) - 1 <= 1 << 20 < total <= (1 << 20) + 4096
    with rtla.Predicates(cfg, below) as preds:
        assert preds.names == ["P", "Q"]
    with pytest.raises(rtla.RtlaError) as e:
        rtla.Predicates(cfg, above)
    assert "2:1: the set's worst case is %d steps per row, above the bound of 1048576" % total in str(e.value)
    with pytest.raises(rtla.RtlaError) as e:   # program words
        rtla.Predicates(cfg, "P == " + " /\\ ".join(["TRUE"] * 300))
    assert "the set's program exceeds 512 words" in str(e.value)
    with pytest.raises(rtla.RtlaError) as e:   # operand depth
        rtla.Predicates(cfg, "P == 0 <= " + "(1 + " * 17 + "1" + ")" * 17)
    assert "operand depth exceeds 16" in str(e.value)


def test_threads_empty_batch_and_layout_binding():
    cfg, _, rows, _ = make_case(*SHAPES[0])
    with rtla.Predicates(cfg, MCPRED) as preds:
        assert rtla.pred_replay(preds, rows, threads=1) == rtla.pred_replay(preds, rows, threads=0)
        assert rtla.pred_replay(preds, []) == ([], dict.fromkeys(preds.names, 0))
        other = rtla.Config(2, 2, 3, 2, 1, 0, (), bag_cap=20)
        orows = rtla.random_rows(other, 0, 4)
        import ctypes as C
        cc = other.c()
        flat, n = rtla._flat_rows(orows, rtla.row_words(other))
        masks = (C.c_int32 * n)()
        assert rtla._lib.rtla_pred_replay(C.byref(cc), preds._h, flat, n, 0, masks, None) == rtla.E_ARG
        # the invariants of the configuration are not part of the layout a set is bound to
        same = rtla.Config(3, 2, 4, 3, 2, 0, ALL, bag_cap=12)
        cc = same.c()
        flat, n = rtla._flat_rows(rows[:4], rtla.row_words(same))
        assert rtla._lib.rtla_pred_replay(C.byref(cc), preds._h, flat, n, 0, masks, None) == rtla.OK
    with pytest.raises(rtla.RtlaError) as e:
        rtla.Predicates(rtla.Config(n_server=6), "P == TRUE")
    assert e.value.status == rtla.E_CONFIG


# ---- the parser under a sanitizer: host code, a stand-alone program

def corpus():
    texts = [MCPRED] + [t for t, _ in COMPILE_ERRORS] + [a for a, _ in UNGUARDED] + [b for _, b in UNGUARDED]
    texts += ["%s == %s" % (n, s) for n, s, _ in FIELD_PREDICATES]
    generated = [d for d in predgen.standard_corpus() if not d[2]]   # every fourth generated state definition
    texts += [predgen.definition(*d) for d in generated[::4]]
    assert len(texts) >= 40 + 45
    return texts


def test_parser_under_address_and_undefined_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "pred_parse")
    csrc = os.path.join(ROOT, "raft-tla_amd", "csrc")
    build = subprocess.run([cxx, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", csrc, os.path.join(ROOT, "tests", "pred_parse_main.cpp"),
                            os.path.join(csrc, "rtla_pred.cpp"), "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr):
        pytest.skip("the compiler has no sanitizer runtime")
    assert build.returncode == 0, build.stderr
    path = tmp_path / "corpus.txt"
    path.write_bytes(b"\x1e".join(t.encode() for t in corpus()))
    run = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "texts" in run.stdout and "ok" in run.stdout
