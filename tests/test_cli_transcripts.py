"""The whole output of the command line (raft-tla_amd/rtla), pinned: for every scenario of tests/cli_scenarios.py
the exit code and the normalised stdout and stderr of each command equal the fixture under tests/golden/cli/.
The fixtures were written by tests/golden/make_cli_golden.py from the binary of the commit before the program was
split into stages, so they pin that commit's behaviour -- the lines tools parse, the order of the refusals, whose
violation an -audit reports -- not the behaviour of the code under test."""
import json
import os

import pytest

import cli_scenarios
from cli_util import CLI

pytestmark = pytest.mark.skipif(not os.path.exists(CLI), reason="build raft-tla_amd/rtla first")


def params():
    for s in cli_scenarios.SCENARIOS:
        yield pytest.param(s, id=s.name, marks=[pytest.mark.gpu] if s.gpu else [])


@pytest.mark.parametrize("scenario", params())
def test_transcript_equals_the_golden(scenario, tmp_path):
    want = json.load(open(cli_scenarios.golden_path(scenario.name)))
    said = "\n".join(want["runs"][-1]["stdout"] + want["runs"][-1]["stderr"])
    assert scenario.expect in said  # the golden holds what the scenario's name promises
    got = cli_scenarios.transcript(CLI, scenario, tmp_path / "run")
    assert len(got) == len(want["runs"])
    for g, w in zip(got, want["runs"]):
        assert g["args"] == w["args"]
        assert g["stdout"] == w["stdout"]
        assert g["stderr"] == w["stderr"]
        assert g["returncode"] == w["returncode"]


def test_the_normaliser_masks_figures_only():
    """What the masks may touch: clock times, durations, rates, the device's description, the directory, and a
    coverage line's distinct count."""
    text = ("Starting... (2025-01-02 03:04:05)\n  level 3: frontier 7, new 9, generated 40, 0.123 ms\n"
            "Progress(3) at 2025-01-02 03:04:05: 40 states generated (1234 s/min), 9 distinct states found (56 ds/min), "
            "9 states left on queue.\nSimulation: 5 walks, 6 steps taken, 7 states generated, 0 stuck; 0.004 s on the "
            "GPU: 1.5e+03 steps/s, 1.75e+03 generated/s.\nRunning on 1 GPU: gfx950 256 CUs\nFinished in 0.42s at "
            "(2025-01-02 03:04:05)\nError: /tmp/x/bad.tla:2:14: type error\n40 states generated, 9 distinct\n"
            "<Timeout of module raft>: 12:34\n")
    assert cli_scenarios.normalise("rtla rank 1 of 2 ready\nrtla rank 0 of 2 ready\n", "/tmp/x", sort_ranks=True) == [
        "rtla rank 0 of 2 ready", "rtla rank 1 of 2 ready", ""]
    assert cli_scenarios.normalise(text, "/tmp/x") == [
        "Starting... (<TIME>)", "  level 3: frontier 7, new 9, generated 40, <MS> ms",
        "Progress(3) at <TIME>: 40 states generated (<RATE> s/min), 9 distinct states found (<RATE> ds/min), "
        "9 states left on queue.",
        "Simulation: 5 walks, 6 steps taken, 7 states generated, 0 stuck; <S> s on the GPU: <RATE> steps/s, "
        "<RATE> generated/s.", "Running on 1 GPU: <DEVICE>", "Finished in <S>s at (<TIME>)",
        "Error: <TMP>/bad.tla:2:14: type error", "40 states generated, 9 distinct",
        "<Timeout of module raft>: <DISTINCT>:34", ""]
    trace = "Error: x\nState 1: <Initial predicate>\n/\\ a = 1\n/\\ b = 2\n\nState 2: <Timeout(r1)>\n/\\ a = 2\n\n9 states\n"
    assert cli_scenarios.normalise(trace + "State 3: <Restart(r1)>\n/\\ a = 3\n\n", "/tmp/x", mask_states=2) == [
        "Error: x", "State 1: <Initial predicate>", "/\\ a = 1", "/\\ b = 2", "", "State 2: <STATE>", "", "9 states",
        "State 3: <Restart(r1)>", "/\\ a = 3", "", ""]
