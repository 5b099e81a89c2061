"""Tests of the command line's user-defined CONSTRAINTs (raft-tla_amd/rtla): a
name under CONSTRAINT(S) beside StateConstraint is a state definition of the
-predicates file and prunes the search; everything else is refused before a
device is opened."""
import os
import re

import pytest

import constrainref
from cli_util import CLI, ROOT, model_dir, run

pytestmark = pytest.mark.skipif(not os.path.exists(CLI), reason="build raft-tla_amd/rtla first")
CON = os.path.join(ROOT, "specs", "MCConstraints.tla")
ACT = os.path.join(ROOT, "specs", "MCActions.tla")
SMALL = ["-skip-spec-check", "-fpbits", "20", "-membudget", str(1 << 29)]
UNDEFINED = "Error: The constraint %s specified in the configuration file is not defined in the specification."


def model(tmp, constraints, shape=(2, 1, 3, 1, 1, 1), invariants=("NoTwoLeaders",), extra=""):
    return model_dir(str(tmp), *shape, list(invariants), constraint=False,
                     extra="CONSTRAINT " + " ".join(constraints) + "\n" + extra)


def test_refusals_before_a_device_is_opened(tmp_path):
    # an unknown name with no file: today's message and exit code, unchanged
    spec, cfg = model(tmp_path / "a", ["StateConstraint", "OneCandidate"])
    r = run(["-skip-spec-check", "-config", cfg, spec])
    assert r.returncode == 150 and UNDEFINED % "OneCandidate" in r.stdout, r.stdout
    # an unknown name with a file: the same message
    spec, cfg = model(tmp_path / "b", ["StateConstraint", "NoSuchThing"])
    r = run(["-skip-spec-check", "-predicates", CON, "-config", cfg, spec])
    assert r.returncode == 150 and UNDEFINED % "NoSuchThing" in r.stdout, r.stdout
    # StateConstraint must still be named
    spec, cfg = model(tmp_path / "c", ["OneCandidate"])
    r = run(["-skip-spec-check", "-predicates", CON, "-config", cfg, spec])
    assert r.returncode == 151 and "no CONSTRAINT" in r.stdout, r.stdout
    # an action definition is no constraint
    spec, cfg = model(tmp_path / "d", ["StateConstraint", "TermsNeverDecrease"])
    r = run(["-skip-spec-check", "-predicates", ACT, "-config", cfg, spec])
    assert r.returncode == 150 and "The constraint TermsNeverDecrease is an action definition" in r.stdout, r.stdout
    # ACTION_CONSTRAINT stays refused
    spec, cfg = model(tmp_path / "e", ["StateConstraint"], extra="ACTION_CONSTRAINT OneCandidate\n")
    r = run(["-skip-spec-check", "-predicates", CON, "-config", cfg, spec])
    assert r.returncode == 151 and "ACTION_CONSTRAINT is not supported by this checker" in r.stdout, r.stdout
    # more than one GPU with -predicates stays refused
    spec, cfg = model(tmp_path / "f", ["StateConstraint", "OneCandidate"])
    r = run(["-gpus", "2", "-predicates", CON, "-config", cfg, spec])
    assert r.returncode == 255 and "-predicates" in r.stderr and "one GPU" in r.stderr
    # the walks do not honour a user constraint: refused, not run unconstrained
    r = run(["-skip-spec-check", "-simulate", "num=10", "-predicates", CON, "-config", cfg, spec])
    assert r.returncode == 150 and "-simulate with a user-defined CONSTRAINT (OneCandidate)" in r.stdout, r.stdout
    assert "Running Random Simulation" not in r.stdout
    # a type error in the file is reported with its place, as for INVARIANT
    bad = tmp_path / "bad.tla"
    bad.write_text("OneCandidate == \\A i \\in Server :\n  state[i] = 1\n")
    r = run(["-skip-spec-check", "-predicates", str(bad), "-config", cfg, spec])
    assert r.returncode == 150 and "bad.tla:2:14: type error" in r.stdout, r.stdout


@pytest.mark.gpu
def test_constrained_search_prints_post_drop_totals(tmp_path):
    _, _, ref = constrainref.case((2, 1, 3, 1, 1, 1), "one_candidate", 100)
    distinct, generated = sum(len(lv.kept) for lv in ref), sum(lv.generated for lv in ref)
    depth = sum(1 for lv in ref if lv.kept)
    spec, cfg = model(tmp_path, ["StateConstraint", "OneCandidate"])
    r = run(SMALL + ["-predicates", CON, "-config", cfg, spec])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Constraining the search by: OneCandidate.\n" in r.stdout
    assert r.stdout.index("Constraining the search by:") < r.stdout.index("Computing initial states")
    assert "Model checking completed. No error has been found." in r.stdout
    assert "%d states generated, %d distinct states found, 0 states left on queue." % (generated, distinct) in r.stdout
    assert "The depth of the complete state graph search is %d." % depth in r.stdout
    progress = re.findall(r"^Progress\(\d+\).*?(\d+) states generated.*?(\d+) distinct states found", r.stdout, re.M)
    assert progress and progress[-1] == (str(generated), str(distinct))


@pytest.mark.gpu
def test_two_constraints_and_a_user_invariant(tmp_path):
    """CONSTRAINTS with two user names beside StateConstraint (the bounds of n2_v1_t2_l1_m1 restated over wider
    ones: the golden's totals), and a user INVARIANT that still sees the unfiltered levels."""
    spec, cfg = model(tmp_path / "a", ["StateConstraint", "TermsUpTo2", "InFlightUpTo1"], shape=(2, 1, 3, 1, 1, 2))
    r = run(SMALL + ["-predicates", CON, "-config", cfg, spec])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Constraining the search by: TermsUpTo2, InFlightUpTo1.\n" in r.stdout
    assert "13797 states generated, 1760 distinct states found" in r.stdout  # golden n2_v1_t2_l1_m1
    # NobodyCommits as an INVARIANT is violated by a state OneElection would keep: found, with its trace
    spec, cfg = model(tmp_path / "b", ["StateConstraint", "OneCandidate"], invariants=("NoTwoLeaders", "NobodyCommits"))
    r = run(SMALL + ["-predicates", CON, "-config", cfg, spec])
    assert r.returncode == 12 and "Error: Invariant NobodyCommits is violated.\n" in r.stdout, r.stdout + r.stderr
    assert "Constraining the search by: OneCandidate.\n" in r.stdout
