"""Tests of the command line's PROPERTY path (raft-tla_amd/rtla): a name under
PROPERTY / PROPERTIES is accepted when -predicates FILE is given and the name
is an action definition of the file (specs/MCActions.tla); it is then checked
on every step out of every level of the search."""
import os
import re

import pytest

from cli_util import CLI, ROOT, model_dir, run

pytestmark = pytest.mark.skipif(not os.path.exists(CLI), reason="build raft-tla_amd/rtla first")
ACTIONS = os.path.join(ROOT, "specs", "MCActions.tla")
PRED = os.path.join(ROOT, "specs", "MCPredicates.tla")
SMALL = ["-skip-spec-check", "-fpbits", "18", "-membudget", str(1 << 28)]
REFUSAL = " is not supported by this checker"


def model(tmp, invariants, properties, keyword="PROPERTY"):
    """model_dir's output plus a PROPERTY line (n2_v1_t2_l1_m1's bounds)."""
    spec, cfg = model_dir(str(tmp), 2, 1, 2, 1, 1, 1, invariants)
    with open(cfg, "a") as f:
        f.write("%s %s\n" % (keyword, " ".join(properties)))
    return spec, cfg


def both_kinds(tmp):
    """A predicate file holding both kinds: specs/MCActions.tla's definitions and a state definition."""
    path = tmp / "Both.tla"
    text = open(ACTIONS).read()
    at = text.index("\\* ---- laws")
    path.write_text(text[:at] + "NoTwoLeadersAgain == \\A i, j \\in Server :\n"
                    "    (state[i] = Leader /\\ state[j] = Leader) => i = j\n\n" + text[at:])
    return str(path)


@pytest.mark.gpu
def test_a_false_action_property_prints_the_step_and_exits_12(tmp_path):
    spec, cfg = model(tmp_path, [], ["LeadersStay"])
    r = run(SMALL + ["-predicates", ACTIONS, "-config", cfg, spec])
    assert r.returncode == 12, r.stdout + r.stderr
    assert "Error: Action property LeadersStay is violated.\n" in r.stdout
    assert "Error: The behavior up to this point is:" in r.stdout
    states = re.findall(r"^State (\d+): <(.*)>$", r.stdout, re.M)
    assert len(states) == 11 and states[0] == ("1", "Initial predicate") and states[-1][1].startswith("Restart")
    blocks = r.stdout.split("State 11:")
    assert blocks[0].split("State 10:")[1].count('"Leader"') > blocks[1].count('"Leader"')


@pytest.mark.gpu
def test_laws_beside_an_invariant_change_nothing(tmp_path):
    spec, cfg = model(tmp_path / "a", ["NoTwoLeaders"], ["LeaderAppendOnly", "TermsNeverDecrease"])
    r = run(SMALL + ["-predicates", ACTIONS, "-config", cfg, spec])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Model checking completed. No error has been found." in r.stdout
    assert "13797 states generated, 1760 distinct states found" in r.stdout  # golden n2_v1_t2_l1_m1
    # a file of both kinds: INVARIANT names are looked up among its state definitions, PROPERTIES among its actions
    spec, cfg = model(tmp_path / "b", ["NoTwoLeaders", "NoTwoLeadersAgain"], ["LeaderAppendOnly", "TermsNeverDecrease"],
                      keyword="PROPERTIES")
    r = run(SMALL + ["-predicates", both_kinds(tmp_path), "-config", cfg, spec])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "13797 states generated, 1760 distinct states found" in r.stdout


@pytest.mark.gpu
def test_audit_accepts_action_definitions(tmp_path):
    spec, cfg = model_dir(str(tmp_path), 2, 1, 2, 1, 1, 1, [])
    r = run(SMALL + ["-predicates", ACTIONS, "-audit", "LeaderAppendOnly,LeadersStay,NoTwoLeaders", "-bfs-levels", "10",
                     "-config", cfg, spec])
    assert r.returncode == 12, r.stdout + r.stderr
    assert "Action property LeaderAppendOnly holds on all 1124 steps.\n" in r.stdout
    assert "Error: Action property LeadersStay is violated by 4 of the 1124 steps.\n" in r.stdout
    assert re.search(r"^Invariant NoTwoLeaders holds in all \d+ states\.$", r.stdout, re.M)
    assert "Error: Action property LeadersStay is violated.\n" in r.stdout
    assert len(re.findall(r"^State (\d+): <(.*)>$", r.stdout, re.M)) == 11


def test_property_is_refused_as_ever_in_every_other_case(tmp_path):
    spec, cfg = model(tmp_path / "a", [], ["LeadersStay"])
    r = run(["-skip-spec-check", "-config", cfg, spec])  # no -predicates file
    assert r.returncode == 151 and "MC.cfg: PROPERTY" + REFUSAL in r.stdout
    spec, cfg = model(tmp_path / "b", [], ["NoSuchAction"])  # an unknown name
    r = run(["-skip-spec-check", "-predicates", ACTIONS, "-config", cfg, spec])
    assert r.returncode == 151 and "MC.cfg: PROPERTY" + REFUSAL in r.stdout
    spec, cfg = model(tmp_path / "c", [], ["LeadersStay", "NoCommit"], keyword="PROPERTIES")  # a state definition
    r = run(["-skip-spec-check", "-predicates", PRED, "-config", cfg, spec])
    assert r.returncode == 151 and "MC.cfg: PROPERTIES" + REFUSAL in r.stdout
    spec, cfg = model(tmp_path / "d", [], ["LeadersStay"])  # more than one GPU: -predicates' own refusal
    r = run(["-gpus", "2", "-predicates", ACTIONS, "-config", cfg, spec])
    assert r.returncode == 255 and "-predicates" in r.stderr and "one GPU" in r.stderr
    # an action definition named under INVARIANT is no invariant; an error in the file is reported with line:col
    spec, cfg = model_dir(str(tmp_path / "e"), 2, 1, 2, 1, 1, 1, ["LeadersStay"])
    r = run(["-skip-spec-check", "-predicates", ACTIONS, "-config", cfg, spec])
    assert r.returncode == 150 and "The invariant LeadersStay specified" in r.stdout
    bad = tmp_path / "bad.tla"
    bad.write_text("Frozen == [][ \\A i \\in Server :\n  i' = i ]_vars\n")
    spec, cfg = model(tmp_path / "f", [], ["Frozen"])
    r = run(["-skip-spec-check", "-predicates", str(bad), "-config", cfg, spec])
    assert r.returncode == 150 and "bad.tla:2:4: only a state variable may carry a prime" in r.stdout
