"""Tests of the command line's -predicates option (raft-tla_amd/rtla): names
under INVARIANT(S) that are not built in are looked up in the predicate file
and checked on every level of the search."""
import os
import re

import pytest

from cli_util import CLI, ROOT, model_dir, run

pytestmark = pytest.mark.skipif(not os.path.exists(CLI), reason="build raft-tla_amd/rtla first")
PRED = os.path.join(ROOT, "specs", "MCPredicates.tla")
SMALL = ["-skip-spec-check", "-fpbits", "22", "-membudget", str(1 << 30)]


@pytest.mark.gpu
def test_user_invariant_prints_tlc_error_trace_and_exit_code(tmp_path):
    spec, cfg = model_dir(str(tmp_path), 3, 1, 3, 1, 1, 1, ["PNoTwoLeaders"])
    r = run(SMALL + ["-predicates", PRED, "-config", cfg, spec])
    assert r.returncode == 12, r.stdout + r.stderr
    assert "Error: Invariant PNoTwoLeaders is violated.\n" in r.stdout
    assert "Error: The behavior up to this point is:" in r.stdout
    states = re.findall(r"^State (\d+): <(.*)>$", r.stdout, re.M)
    assert len(states) == 19 and states[0] == ("1", "Initial predicate")  # golden n3_v1_t3_l1_m1_ntl: level 19
    assert r.stdout.count('"Leader"') >= 2 and "The depth of the complete state graph search is 19." in r.stdout
    # a built-in and a user-defined name side by side; a name that holds changes nothing
    spec, cfg = model_dir(str(tmp_path / "b"), 2, 1, 2, 1, 1, 1, ["NoTwoLeaders", "MessagesWithinSenderTerm"])
    r = run(SMALL + ["-predicates", PRED, "-config", cfg, spec])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Model checking completed. No error has been found." in r.stdout
    assert "13797 states generated, 1760 distinct states found" in r.stdout  # golden n2_v1_t2_l1_m1


@pytest.mark.gpu
def test_audit_accepts_user_defined_names(tmp_path):
    spec, cfg = model_dir(str(tmp_path), 3, 1, 3, 1, 1, 1, ["ElectionSafety"])
    r = run(SMALL + ["-predicates", PRED, "-audit", "PNoTwoLeaders,StateMachineSafety,NoCommit", "-bfs-levels", "19",
                     "-config", cfg, spec])
    assert r.returncode == 12, r.stdout + r.stderr
    assert re.search(r"^Error: Invariant PNoTwoLeaders is violated by \d+ of the \d+ states\.$", r.stdout, re.M)
    assert re.search(r"^Invariant StateMachineSafety holds in all \d+ states\.$", r.stdout, re.M)
    assert re.search(r"^(Error: )?Invariant NoCommit (holds in all|is violated by) \d+", r.stdout, re.M)
    assert "Error: Invariant PNoTwoLeaders is violated.\n" in r.stdout
    assert len(re.findall(r"^State (\d+): <(.*)>$", r.stdout, re.M)) == 19


def test_unknown_names_and_more_gpus_are_refused_at_start_up(tmp_path):
    spec, cfg = model_dir(str(tmp_path), 2, 1, 2, 1, 1, 1, ["PNoTwoLeaders"])
    r = run(["-skip-spec-check", "-config", cfg, spec])  # without -predicates: the error it is today
    assert r.returncode == 150
    assert "The invariant PNoTwoLeaders specified in the configuration file is not defined" in r.stdout
    r = run(["-gpus", "2", "-predicates", PRED, "-config", cfg, spec])
    assert r.returncode == 255 and "-predicates" in r.stderr and "one GPU" in r.stderr
    # a name the predicate file does not define either, and a file with an error: before any device is opened
    spec2, cfg2 = model_dir(str(tmp_path / "b"), 2, 1, 2, 1, 1, 1, ["NoSuchThing"])
    r = run(["-skip-spec-check", "-predicates", PRED, "-config", cfg2, spec2])
    assert r.returncode == 150 and "The invariant NoSuchThing specified" in r.stdout
    bad = tmp_path / "bad.tla"
    bad.write_text("PNoTwoLeaders == \\A i \\in Server :\n  state[i] = 1\n")
    r = run(["-skip-spec-check", "-predicates", str(bad), "-config", cfg, spec])
    assert r.returncode == 150 and "bad.tla:2:14: type error" in r.stdout
