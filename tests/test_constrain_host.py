"""Host tests of user-defined CONSTRAINTs (no GPU): specs/MCConstraints.tla
compiles for every golden layout and says what its comments say, the Python
mirror of the new calls, and the host-only logic of the constraint pass (chunk
size, chunk plan, the batch ring's argument check: rtla_constrain.h) as a
stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import json
import os
import shutil
import subprocess

import pytest

import constrainref
import rtla

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "bfs_counts.json")))
MCCON = open(os.path.join(ROOT, "specs", "MCConstraints.tla")).read()
NAMES = ["TermsUpTo2", "LogsUpTo1", "CopiesUpTo1", "InFlightUpTo1", "OneCandidate", "OneElection", "NobodyCommits"]


def test_mcconstraints_compiles_for_every_golden_layout():
    shapes = sorted({(g["n_server"], g["n_value"], g["max_term"], g["max_log"], g["max_copies"], g["max_msgs"],
                      bool(g.get("symmetry"))) for g in GOLD.values()})
    assert len(shapes) > 20
    for *shape, sym in shapes:
        with rtla.Predicates(rtla.Config(*shape, invariants=(), symmetry=sym), MCCON) as preds:
            assert preds.names == NAMES and not preds.step


def test_mcconstraints_definitions_say_what_their_names_say():
    """On generator rows of a layout with terms to 4, logs to 3 and two copies: each definition against the
    state's text (the four bounds restated) or against the reference's spelling of it."""
    cfg = rtla.Config(3, 2, 4, 3, 2, 0, (), bag_cap=12)
    rows = rtla.random_rows(cfg, 0, 600)
    with rtla.Predicates(cfg, MCCON) as preds, rtla.Predicates(cfg, "\n".join([
            r"A == \A i \in Server : currentTerm[i] <= 2", r"B == \A i \in Server : Len(log[i]) <= 1",
            r"C == \A m \in DOMAIN messages : messages[m] <= 1", r"D == BagCardinality(messages) <= 1",
            constrainref.ONE_CANDIDATE, constrainref.ONE_ELECTION,
            r"G == ~ \E i \in Server : commitIndex[i] > 0"])) as same:
        masks, counts = rtla.pred_replay(preds, rows)
        assert masks == rtla.pred_replay(same, rows)[0]
        assert all(0 < c < len(rows) for c in counts.values()), counts  # every definition decides something here
    init = rtla.init_row(cfg)
    with rtla.Predicates(cfg, MCCON) as preds:
        assert rtla.pred_replay(preds, [init])[0] == [0]  # Init satisfies every example


def test_python_mirror_of_the_new_calls():
    assert rtla._lib.rtla_abi_version() == 12  # new symbols only
    st = rtla._ConstrainStats()
    assert C.sizeof(st) == 4 + 4 + 3 * 8 + 8 * 8 + 8 + 2 * 8 + 8 + 4 + 4
    r = rtla.ConstrainResult()
    assert (r.status, r.kept, r.dropped, r.counts) == (rtla.OK, 0, 0, {})
    import inspect
    assert "constraint" in inspect.signature(rtla.check).parameters
    assert "constraint" in inspect.signature(rtla.Checker.run).parameters
    # the arguments rtla_constrain_batch refuses before it touches a device
    cfg = rtla.Config(2, 1, 2, 1, 1, 1, ())
    w = rtla.row_words(cfg)
    row = (C.c_uint32 * w)(*rtla.init_row(cfg))
    out, side, kept = (C.c_uint32 * w)(), (C.c_uint64 * 1)(), C.c_size_t(0)
    with rtla.Predicates(cfg, "T == TRUE") as preds, rtla.Actions(
            cfg, r"A == [][ \A i \in Server : currentTerm'[i] >= currentTerm[i] ]_vars") as acts:
        cc = cfg.c()
        call = lambda h, cap, start, k=kept: rtla._lib.rtla_constrain_batch(
            C.byref(cc), h, row, 1, cap, start, 64, out, side, C.byref(k) if k is not None else None, None)
        assert call(acts._h, 64, 0) == rtla.E_ARG and call(None, 64, 0) == rtla.E_ARG
        assert call(preds._h, 0, 0) == call(preds._h, 100, 0) == call(preds._h, 128, 32) == rtla.E_ARG
        assert call(preds._h, 128, 128) == rtla.E_ARG and call(preds._h, 64, 0, None) == rtla.E_ARG
        bad = rtla.Config(n_server=6).c()
        assert rtla._lib.rtla_constrain_batch(C.byref(bad), preds._h, row, 1, 64, 0, 64, out, side, C.byref(kept),
                                              None) == rtla.E_CONFIG
        assert rtla._lib.rtla_pred_constrain(None, preds._h, None) == rtla.E_ARG
        # no rows: nothing to lay out, no device needed
        assert rtla.constrain_batch(preds, []) == ([], [], {"T": 0})


def test_reference_bfs_without_a_constraint_is_the_golden():
    """The test-side reference (tests/constrainref.py) with a constraint that keeps everything reproduces the C
    oracle's golden: what the GPU tests compare against is a BFS of this model."""
    g = GOLD["n2_v1_t2_l1_m1"]
    cfg = rtla.Config(2, 1, 2, 1, 1, 1, ())
    ref = constrainref.bfs(cfg, "T == TRUE", 100)
    assert [[len(lv.kept), lv.generated] for lv in ref] == g["levels"]
    assert ["%016x" % rtla.rows_text_hash(cfg, lv.kept) for lv in ref] == g["level_text_hash"]


def test_plan_under_address_and_undefined_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "constrain_plan")
    csrc = os.path.join(ROOT, "raft-tla_amd", "csrc")
    build = subprocess.run([cxx, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", csrc, os.path.join(ROOT, "tests", "constrain_plan_main.cpp"), "-o", exe],
                           capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr):
        pytest.skip("the compiler has no sanitizer runtime")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "constrain plan: ok" in run.stdout, run.stdout + run.stderr
