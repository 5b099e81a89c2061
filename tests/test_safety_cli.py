"""CPU tests of the command line's part in the two safety invariants and the
audit: what is decided before any GPU work (cfg operator checks, -audit name
checks, usage)."""
import os

import pytest

from cli_util import CLI, model_dir, run

pytestmark = pytest.mark.skipif(not os.path.exists(CLI), reason="build raft-tla_amd/rtla first")


def test_cfg_naming_the_new_invariants_is_accepted_up_to_the_gpu(tmp_path):
    tla, cfg = model_dir(str(tmp_path), 3, 1, 2, 1, 1, 1, ["StateMachineSafety", "LeaderCompleteness", "LogMatching"])
    text = open(tla).read()
    assert "StateMachineSafety ==" in text and "LeaderCompleteness ==" in text  # specs/MC.tla defines both
    r = run(["-skip-spec-check", "-config", cfg, tla])
    assert "not defined" not in r.stdout, r.stdout
    assert r.returncode in (0, 255)  # 255: no GPU where the CPU tests run
    # and, like the old three, raft.tla itself defines neither
    open(tmp_path / "raft.tla", "w").write(text.replace("MODULE MC", "MODULE raft"))
    r = run(["-skip-spec-check", "-config", cfg, str(tmp_path / "raft.tla")])
    assert r.returncode == 150 and "The invariant StateMachineSafety specified" in r.stdout


def test_audit_names_are_checked_like_cfg_invariants(tmp_path):
    tla, cfg = model_dir(str(tmp_path), 3, 1, 2, 1, 1, 1, ["ElectionSafety"])
    r = run(["-skip-spec-check", "-audit", "TypeOK", "-config", cfg, tla])
    assert r.returncode == 150, r.stdout + r.stderr
    assert ("Error: The invariant TypeOK specified in the configuration file is not defined in the "
            "specification.") in r.stdout
    r = run(["-skip-spec-check", "-audit", "StateMachineSafety,TypeOK", "-config", cfg, tla])
    assert r.returncode == 150 and "The invariant TypeOK specified" in r.stdout
    r = run(["-skip-spec-check", "-audit", "StateMachineSafety,LeaderCompleteness,NoTwoLeaders", "-bfs-levels", "3",
             "-config", cfg, tla])
    assert "not defined" not in r.stdout and r.returncode in (0, 12, 255), r.stdout


def test_audit_usage_and_refusals(tmp_path):
    r = run([])
    assert r.returncode == 255 and "-audit Name[,Name...]" in r.stderr
    tla, cfg = model_dir(str(tmp_path), 3, 1, 2, 1, 1, 1, ["ElectionSafety"])
    r = run(["-skip-spec-check", "-audit", "LogMatching", "-gpus", "2", "-config", cfg, tla])
    assert r.returncode == 255 and "-audit names at least one invariant and runs on one GPU" in r.stderr
    r = run(["-skip-spec-check", "-audit", "LogMatching", "-simulate", "-config", cfg, tla])
    assert r.returncode == 255 and "-audit" in r.stderr
