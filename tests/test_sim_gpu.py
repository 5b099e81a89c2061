"""GPU tests of the random-walk simulation (Checker.simulate, k_simulate):
the walks the device computes are the host replay's (rtla.sim_replay, pinned
by tests/test_sim_host.py) bit for bit, the BFS is left untouched, and a
violation found beyond the BFS frontier comes back as a full behaviour."""
import json
import os
import re

import pytest

import raft_cpu
import rtla

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "bfs_counts.json")))
SHAPES = [(2, 1, 3, 1, 2, 0),   # Duplicate with MaxCopies = 2
          (3, 2, 3, 2, 1, 3),
          (5, 1, 3, 2, 1, 3)]   # more than 128 candidates per state: several 64-wide chunks
KW = dict(fpset_log2=20, mem_budget=1 << 29)
SEED = 77


def same_as_host(ck, cfg, n_walks, depth, first):
    front = ck.frontier()
    ref = rtla.sim_replay(cfg, front, n_walks, depth, seed=SEED, first=first)
    got = ck.simulate(n_walks, depth, seed=SEED, first=first, ends=True)
    assert got.status == ref.status == rtla.OK and got.walks == ref.walks == n_walks
    bad = [k for k in range(n_walks) if got.ends[k] != ref.ends[k]]
    assert not bad, (len(bad), bad[:5], got.ends[bad[0]], ref.ends[bad[0]])
    assert (got.steps, got.generated, got.stuck) == (ref.steps, ref.generated, ref.stuck)
    assert got.taken == ref.taken and sum(got.taken.values()) == got.steps
    return front, got


@pytest.mark.parametrize("shape", SHAPES)
def test_ends_match_host_replay(shape):
    cfg = rtla.Config(*shape, invariants=(), **KW)
    with rtla.Checker(cfg) as ck:
        ck.init()
        front, got = same_as_host(ck, cfg, 4099, 48, 7)
        assert len(front) == 1 and got.steps == 4099 * 48
        for _ in range(4):
            ck.step()
        front, got = same_as_host(ck, cfg, 4099, 48, 7)
        assert len(front) > 8 and len(front) == ck.levels[-1].new
        # walks w and w + |frontier| share a start row and differ afterwards
        assert len({e[:3] for e in got.ends}) > 4000


def test_depth_split_across_launches_matches_host_replay():
    """4,099 walks x 2,100 steps exceed one launch's walks x steps bound
    (rtla_sim.h SIM_LAUNCH_STEPS = 2^23): the walks' rows are carried through a
    device buffer between launches."""
    cfg = rtla.Config(2, 1, 3, 1, 2, 0, invariants=(), **KW)
    assert 4099 * 2100 > 1 << 23
    with rtla.Checker(cfg) as ck:
        ck.init()
        ck.step()
        same_as_host(ck, cfg, 4099, 2100, 7)


def test_bfs_is_undisturbed_by_a_simulation():
    g = GOLD["n2_v1_t3_l1_m1"]
    cfg = rtla.Config(g["n_server"], g["n_value"], g["max_term"], g["max_log"], g["max_copies"], g["max_msgs"],
                      tuple(g["invariants"]), **KW)
    with rtla.Checker(cfg) as ck:
        ck.init()
        for _ in range(4):
            ck.step()
        assert len(ck.levels) == 5
        res = ck.simulate(5000, 40, seed=SEED)
        assert res.status == rtla.OK and res.steps == 5000 * 40
        assert ck.violation() == (None, False)
        assert ck.run() == rtla.DONE
        assert [[lv.new, lv.generated] for lv in ck.levels] == g["levels"]
        assert (ck.distinct, ck.generated) == (g["distinct"], g["generated"])
        assert sum(1 for lv in ck.levels if lv.new > 0) == g["depth"]
        cov = ck.coverage()
        assert sum(v[0] for v in cov.values()) == g["generated"] - 1


def test_violation_through_the_frontier():
    """BFS finds NoTwoLeaders violated at level 19 of this model; one walk of
    depth 4 from each state of level 17 finds it by sampling."""
    g = GOLD["n3_v1_t3_l1_m1_ntl"]
    cfg = rtla.Config(3, 1, 3, 1, 1, 1, ("NoTwoLeaders",), fpset_log2=22, mem_budget=1 << 30)
    with rtla.Checker(cfg) as ck:
        ck.init()
        for _ in range(16):
            assert ck.step() == rtla.OK
        front = ck.frontier()
        n = len(front)
        assert len(ck.levels) == 17 and n == g["levels"][16][0]
        ref = rtla.sim_replay(cfg, front, n, 4, seed=1)
        violating = [k for k, e in enumerate(ref.ends) if e[4] == rtla.SIM_STOP_VIOLATION]
        print("violating walks (host replay): %d of %d" % (len(violating), n))
        assert len(violating) >= 1 and ref.status == rtla.VIOLATION and ref.viol_walk == violating[0]
        got = ck.simulate(n, 4, seed=1, ends=True)
        assert got.status == rtla.VIOLATION and got.violation == "NoTwoLeaders"
        assert (got.viol_walk, got.viol_step, got.viol_inst, got.viol_mask, got.viol_in_model) == \
               (ref.viol_walk, ref.viol_step, ref.viol_inst, ref.viol_mask, ref.viol_in_model)
        assert got.ends == ref.ends and (got.steps, got.generated) == (ref.steps, ref.generated)
        assert ck.violation() == ("NoTwoLeaders", got.viol_in_model)
        tr = ck.trace()
        assert len(tr) == 17 + got.viol_step and tr[0][0] == "Initial predicate"
        assert tr[16][1] == rtla.state_text(cfg, front[got.viol_walk % n])
        walk = raft_cpu.Walk(raft_cpu.cfg_of(3, 1, 3, 1, 1, 1, ("NoTwoLeaders",)))
        assert walk.text() == tr[0][1] and walk.invariants() == 0
        for k, (label, text) in enumerate(tr[1:], 1):
            assert text in [t for _, t in walk.successors()], label
            walk.goto(text)
            assert (walk.invariants() != 0) == (k == len(tr) - 1), k
        assert tr[-1][1].count('"Leader"') >= 2
        # the BFS goes on from level 17 as if nothing had happened
        assert ck.step() == rtla.OK and ck.levels[-1].new == g["levels"][17][0]
        assert ck.violation() == (None, False)


def test_refusals():
    small = dict(fpset_log2=16, mem_budget=1 << 28)
    with rtla.Checker(rtla.Config(2, 1, 2, 1, 1, 1, (), **small)) as ck:
        with pytest.raises(rtla.RtlaError) as e:   # before init
            ck.simulate(10, 5)
        assert e.value.status == rtla.E_STATE
    with rtla.Checker(rtla.Config(2, 1, 2, 1, 1, 1, (), shards=2, **small)) as ck:
        ck.init()
        with pytest.raises(rtla.RtlaError) as e:
            ck.simulate(10, 5)
        assert e.value.status == rtla.E_STATE
    with rtla.Checker(rtla.Config(2, 1, 2, 1, 1, 1, (), dedup_only=True, **small)) as ck:
        with pytest.raises(rtla.RtlaError) as e:
            ck.simulate(10, 5)
        assert e.value.status == rtla.E_STATE


def test_cli_simulate_finds_the_violation_beyond_the_bfs():
    from cli_util import run
    n = GOLD["n3_v1_t3_l1_m1_ntl"]["levels"][16][0]
    r = run(["-skip-spec-check", "-fpbits", "22", "-membudget", str(1 << 30), "-simulate", "num=%d" % n, "-depth", "4",
             "-seed", "1", "-bfs-levels", "17", "-config", os.path.join(ROOT, "specs", "raft3_v1_t3_l1_m1_ntl.cfg"),
             os.path.join(ROOT, "specs", "MC.tla")])
    assert r.returncode == 12, r.stdout + r.stderr
    assert "Running Random Simulation with seed 1 " in r.stdout
    assert "Error: Invariant NoTwoLeaders is violated." in r.stdout
    states = re.findall(r"^State (\d+): <(.*)>$", r.stdout, re.M)
    assert states[0] == ("1", "Initial predicate") and 17 < len(states) <= 21
    assert [int(k) for k, _ in states] == list(range(1, len(states) + 1))
    assert "r1" in r.stdout and '"Leader"' in r.stdout


def test_cli_simulate_without_violation(tmp_path):
    from cli_util import model_dir, run
    tla, cfg = model_dir(str(tmp_path), 3, 1, 2, 1, 1, 1, ["NoTwoLeaders"])
    r = run(["-skip-spec-check", "-fpbits", "20", "-membudget", str(1 << 29), "-simulate", "num=1000", "-depth", "20",
             "-config", cfg, tla])
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"^Simulation: (\d+) walks, (\d+) steps taken, (\d+) states generated, ", r.stdout, re.M)
    assert m and (int(m.group(1)), int(m.group(2))) == (1000, 20000) and int(m.group(3)) > 20000, r.stdout
    assert re.search(r"^Running Random Simulation with seed \d+ from the 1 states of BFS level 1", r.stdout, re.M)
    assert "No error has been found" in r.stdout
    r2 = run(["-skip-spec-check", "-simulate", "-gpus", "2", "-config", cfg, tla])
    assert r2.returncode == 255 and "-simulate runs on one GPU" in r2.stderr
