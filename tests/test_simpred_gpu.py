"""GPU tests of the random walks that carry user properties (DESIGN.md section
15; Checker.simulate(predicates=, actions=), k_simulate<NS, true>): the device
computes the host replay's walks (rtla.sim_replay with the same sets, pinned by
tests/test_simpred_host.py) bit for bit -- 5-word records, counters, reported
violation -- and a false definition found beyond the BFS frontier comes back
as a full behaviour."""
import json
import os
import re

import pytest

import limits
import raft_cpu
import raft_values as rv
import rtla
from test_simpred_host import (BUILTINS_TEXT, LAWS, LAWS_TEXT, MCACTIONS, MCPRED, RESTATED, WITNESS_ACTIONS,
                               WITNESS_STATES, witness_sets)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "bfs_counts.json")))
SHAPES = [(2, 1, 3, 1, 2, 0), (3, 2, 3, 2, 1, 3), (5, 1, 3, 2, 1, 3)]
KW = dict(fpset_log2=20, mem_budget=1 << 29)
SEED = 77
VIOL = rtla.SIM_STOP_VIOLATION
BAG_NEVER_SHRINKS = WITNESS_ACTIONS.split("\n")[2]
TERMS_BELOW_3 = WITNESS_ACTIONS.split("\n")[1]


def definition(text, name, until):
    return text[text.index(name + " =="):text.index(until)]


def fields(r):
    return (r.status, r.walks, r.steps, r.generated, r.stuck, r.taken, r.state_evaluated, r.step_evaluated,
            r.violation, r.viol_walk, r.viol_step, r.viol_inst, r.viol_mask, r.viol_in_model, r.viol_state_mask,
            r.viol_step_mask)


def same_as_host(ck, cfg, front, n_walks, depth, first=0, seed=SEED, **sets):
    """The device's walks against the host replay's: (reference, device result)."""
    ref = rtla.sim_replay(cfg, front, n_walks, depth, seed=seed, first=first, **sets)
    got = ck.simulate(n_walks, depth, seed=seed, first=first, ends=True, **sets)
    bad = [k for k in range(min(len(got.ends), len(ref.ends))) if got.ends[k] != ref.ends[k]]
    assert not bad, (len(bad), bad[:5], got.ends[bad[0]], ref.ends[bad[0]])
    assert len(got.ends) == len(ref.ends) and fields(got) == fields(ref)
    assert sum(got.taken.values()) == got.steps
    if sets.get("actions") is not None:
        assert got.step_evaluated == got.generated
    return ref, got


def tile_children(words):
    """k_simulate<NS, true>'s children per tile (rtla_ksim.hip sim_tile_children, at 2 waves per SIMD)."""
    even = (words + 1) & ~1
    wave0 = (((2 * even + 32 + 20 + 3) & ~3) + 3) & ~3
    return min(64, (((65536 // 4 - 16 - 2 * 512) // 4) - wave0 - 3) // ((words | 1) + 23))


# ---- 5. device equals host

@pytest.mark.parametrize("shape", SHAPES)
def test_walks_with_witnesses_match_host_replay(shape):
    cfg = rtla.Config(*shape, invariants=(), **KW)
    preds, acts = witness_sets(cfg)
    bag = rtla.Actions(cfg, BAG_NEVER_SHRINKS)
    with rtla.Checker(cfg) as ck:
        ck.init()
        front = ck.frontier()
        ref, _ = same_as_host(ck, cfg, front, 4099, 12, 7, predicates=preds, actions=acts)
        assert ref.status == rtla.VIOLATION and len({e[3] for e in ref.ends if e[4] == VIOL}) >= 3
        for _ in range(4):
            ck.step()
        front = ck.frontier()
        assert len(front) > 8
        ref, _ = same_as_host(ck, cfg, front, 4099, 12, 7, predicates=preds, actions=acts)
        assert ref.status == rtla.VIOLATION
        same_as_host(ck, cfg, front, 4099, 12, 7, predicates=preds)
        # BagNeverShrinks alone fails on Receive / Drop, whose instances follow the fixed families
        ref, _ = same_as_host(ck, cfg, front, 4099, 12, 7, actions=bag)
        insts = [e[5] & 0xFFFF for e in ref.ends if e[4] == VIOL]
        assert len(insts) > 1000 and all(e[5] >> 40 == 1 for e in ref.ends if e[4] == VIOL)
        if shape[0] == 5:  # a violation in the second 64-wide chunk of candidates
            assert max(insts) >= 64
        assert ck.violation()[0] == "BagNeverShrinks"


def test_a_second_tile_of_children_on_the_widest_layout():
    """A narrow row's tile holds 64 children, a whole chunk of candidates, so no state of the shapes above needs
    a second tile.  The widest layout's (tests/limits.py) holds 30: its sample has states with more enabled
    successors than that, and the walks from them are the host's.  (A seeded context allows simulate.)"""
    c = limits.case("n3_v4_t6_c14")
    cfg = rtla.Config(3, 4, 6, 2, 14, 0, invariants=(), bag_cap=16, **KW)
    assert cfg.c().bag_cap == c.cfg.c().bag_cap and rtla.row_words(cfg) == len(c.rows[0])
    tc = tile_children(len(c.rows[0]))
    assert 4 <= tc < 64
    room = [k for k, s in enumerate(c.states) if len(s[rv.IX["messages"]]) + 4 < c.K
            and len(s[rv.IX["elections"]]) + 4 < c.E]
    rows = [list(c.rows[k]) for k in room]
    with rtla.Predicates(cfg, BUILTINS_TEXT) as preds, rtla.Actions(cfg, LAWS_TEXT) as acts, \
            rtla.Actions(cfg, BAG_NEVER_SHRINKS) as bag, rtla.Checker(cfg) as ck:
        ck.init(roots=rows)
        front = ck.frontier()
        enabled = [rtla.sim_replay(cfg, [r], 1, 1, seed=SEED, actions=acts).generated for r in front]
        print("tile of %d children; enabled successors of the start rows: max %d" % (tc, max(enabled)))
        assert max(enabled) > tc
        n = 4 * len(front)
        # (the sample's rows are random, not reachable: the restated built-ins are false on some successors)
        ref, got = same_as_host(ck, cfg, front, n, 4, predicates=preds, actions=acts)
        assert 0 < sum(1 for e in ref.ends if e[4] == VIOL) < n
        plain = ck.simulate(n, 4, seed=SEED, ends=True)
        assert all(g[:3] == p[:3] for g, p in zip(got.ends, plain.ends) if g[4] != VIOL)
        # the five laws hold on the steps out of any row: they change nothing, on the widest layout too
        ref, got = same_as_host(ck, cfg, front, n, 4, actions=acts)
        assert got.status == rtla.OK and [e[:5] for e in got.ends] == plain.ends and all(e[5] == 0 for e in got.ends)
        assert (got.steps, got.generated, got.taken) == (plain.steps, plain.generated, plain.taken)
        ref, got = same_as_host(ck, cfg, front, n, 4, actions=bag)
        assert ref.status == rtla.VIOLATION


# ---- 6. laws change nothing, on the device

@pytest.mark.parametrize("shape", SHAPES)
def test_laws_change_nothing_on_the_device(shape):
    cfg = rtla.Config(*shape, invariants=(), **KW)
    with rtla.Predicates(cfg, BUILTINS_TEXT) as preds, rtla.Actions(cfg, LAWS_TEXT) as acts, rtla.Checker(cfg) as ck:
        assert preds.names == RESTATED and acts.names == LAWS
        ck.init()
        for _ in range(4):
            ck.step()
        plain = ck.simulate(4099, 12, seed=SEED, first=7, ends=True)
        got = ck.simulate(4099, 12, seed=SEED, first=7, ends=True, predicates=preds, actions=acts)
        assert got.status == plain.status == rtla.OK and got.violation is None
        assert [e[:5] for e in got.ends] == plain.ends and all(e[5] == 0 for e in got.ends)
        assert (got.steps, got.generated, got.stuck, got.taken) == (plain.steps, plain.generated, plain.stuck,
                                                                    plain.taken)
        assert got.step_evaluated == got.generated and 0 < got.state_evaluated <= got.generated
        assert ck.violation() == (None, False)


# ---- 7. launch split

def test_depth_split_across_launches_matches_host_replay():
    """4,099 walks x 2,100 steps exceed one launch's walks x steps bound (2^23): a walk that ended in the
    first launch keeps its record, word 4 included; the others are carried on."""
    cfg = rtla.Config(2, 1, 3, 1, 2, 0, invariants=(), **KW)
    seg = (1 << 23) // 4099
    assert 4099 * 2100 > 1 << 23 and seg < 2100
    text = definition(MCACTIONS, "TermsNeverDecrease", "\\* Within a term") + BAG_NEVER_SHRINKS
    with rtla.Actions(cfg, text) as acts, rtla.Checker(cfg) as ck:
        assert acts.names == ["TermsNeverDecrease", "BagNeverShrinks"]
        ck.init()
        ck.step()
        ref, got = same_as_host(ck, cfg, ck.frontier(), 4099, 2100, 7, actions=acts)
        early = [e for e in ref.ends if e[4] == VIOL and e[3] < seg]
        assert early and all(e[5] >> 40 == 2 for e in early)
    # walks that end in later launches: a law alone, checked for every one of the 2,100 steps
    law = definition(MCACTIONS, "TermsNeverDecrease", "\\* Within a term")
    with rtla.Actions(cfg, law) as acts, rtla.Checker(cfg) as ck:
        ck.init()
        ck.step()
        ref, got = same_as_host(ck, cfg, ck.frontier(), 4099, 2100, 7, actions=acts)
        assert got.status == rtla.OK and got.steps == 4099 * 2100


# ---- 8. beyond the frontier: a state predicate

def test_state_predicate_violated_beyond_the_frontier():
    """test_sim_gpu.py::test_violation_through_the_frontier with the invariant as a user predicate: BecomeLeader
    touches nothing the constraint reads, so the same successors are in-model."""
    g = GOLD["n3_v1_t3_l1_m1_ntl"]
    cfg = rtla.Config(3, 1, 3, 1, 1, 1, (), fpset_log2=22, mem_budget=1 << 30)
    with rtla.Predicates(cfg, definition(MCPRED, "PNoTwoLeaders", "PElectionSafety")) as preds, \
            rtla.Checker(cfg) as ck:
        assert preds.names == ["PNoTwoLeaders"]
        ck.init()
        for _ in range(16):
            assert ck.step() == rtla.OK
        front = ck.frontier()
        n = len(front)
        assert len(ck.levels) == 17 and n == g["levels"][16][0]
        ref = rtla.sim_replay(cfg, front, n, 4, seed=1, predicates=preds)
        violating = [k for k, e in enumerate(ref.ends) if e[4] == VIOL]
        print("violating walks (host replay): %d of %d" % (len(violating), n))
        assert len(violating) >= 1 and ref.status == rtla.VIOLATION and ref.viol_walk == violating[0]
        got = ck.simulate(n, 4, seed=1, ends=True, predicates=preds)
        assert got.ends == ref.ends and fields(got) == fields(ref)
        assert got.violation == "PNoTwoLeaders" and (got.viol_mask, got.viol_state_mask, got.viol_step_mask) == (0, 1, 0)
        assert ck.violation() == ("PNoTwoLeaders", got.viol_in_model)
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
        assert ck.step() == rtla.OK and ck.levels[-1].new == g["levels"][17][0]
        assert ck.violation() == (None, False)


# ---- 9. beyond the frontier: an action property

def test_action_property_violated_beyond_the_frontier():
    """BFS finds CommitNeverDecreases false at level 16 of this model; one walk of depth 8 from each state of
    level 14 finds it by sampling (the host replay: 4 of the 1,520 walks)."""
    shape = (2, 2, 3, 2, 1, 1)
    cfg = rtla.Config(*shape, invariants=(), **KW)
    text = definition(MCACTIONS, "CommitNeverDecreases", "\\* Violated by the first Timeout")
    with rtla.Actions(cfg, text) as acts, rtla.Checker(cfg) as ck:
        assert acts.names == ["CommitNeverDecreases"]
        ck.init()
        for _ in range(13):
            assert ck.step() == rtla.OK
            assert ck.audit_steps(acts).status == rtla.OK
        front = ck.frontier()
        n = len(front)
        assert len(ck.levels) == 14 and n <= 1 << 18
        ref = rtla.sim_replay(cfg, front, n, 8, seed=1, actions=acts)
        violating = [k for k, e in enumerate(ref.ends) if e[4] == VIOL]
        print("violating walks (host replay): %d of %d" % (len(violating), n))
        assert 1 <= len(violating) < n
        got = ck.simulate(n, 8, seed=1, ends=True, actions=acts)
        assert got.ends == ref.ends and fields(got) == fields(ref)
        assert got.violation == "CommitNeverDecreases" and ck.violation()[0] == "CommitNeverDecreases"
        tr = ck.trace()
        assert len(tr) == 14 + got.viol_step and tr[-1][0].startswith("Restart")
        walk = raft_cpu.Walk(raft_cpu.cfg_of(*shape, ()))
        assert walk.text() == tr[0][1]
        for label, text in tr[1:]:
            assert text in [t for _, t in walk.successors()], label
            walk.goto(text)


# ---- 10. refusals

def test_refusals():
    small = dict(fpset_log2=16, mem_budget=1 << 28)
    for extra, init in ((dict(), False), (dict(shards=2), True), (dict(dedup_only=True), False)):
        cfg = rtla.Config(2, 1, 2, 1, 1, 1, (), **extra, **small)
        with rtla.Actions(cfg, TERMS_BELOW_3) as acts, rtla.Predicates(cfg, WITNESS_STATES) as preds, \
                rtla.Checker(cfg) as ck:
            if init:
                ck.init()
            for kw in (dict(actions=acts), dict(predicates=preds), dict(predicates=preds, actions=acts)):
                with pytest.raises(rtla.RtlaError) as e:
                    ck.simulate(10, 5, **kw)
                assert e.value.status == rtla.E_STATE, (extra, kw)
    cfg = rtla.Config(2, 1, 2, 1, 1, 1, (), **small)
    other = rtla.Config(2, 1, 3, 1, 2, 0, ())
    with rtla.Actions(cfg, TERMS_BELOW_3) as acts, rtla.Predicates(cfg, WITNESS_STATES) as preds, \
            rtla.Actions(other, TERMS_BELOW_3) as oacts, rtla.Checker(cfg) as ck:
        ck.init()
        for kw in (dict(actions=preds), dict(predicates=acts), dict(actions=oacts)):
            with pytest.raises(rtla.RtlaError) as e:
                ck.simulate(10, 5, **kw)
            assert e.value.status == rtla.E_ARG, kw
        assert ck.simulate(10, 5, predicates=preds, actions=acts).status == rtla.VIOLATION


# ---- 11. the command line

def test_cli_carries_the_cfg_properties_into_the_walks(tmp_path):
    from cli_util import model_dir, run
    pred = tmp_path / "Witness.tla"
    pred.write_text(LAWS_TEXT + WITNESS_ACTIONS + WITNESS_STATES + "====\n")
    small = ["-skip-spec-check", "-fpbits", "18", "-membudget", str(1 << 28)]

    def model(sub, properties):
        (tmp_path / sub).mkdir()
        spec, cfg = model_dir(str(tmp_path / sub), 2, 1, 3, 1, 1, 1, [])
        with open(cfg, "a") as f:
            f.write("PROPERTY %s\n" % " ".join(properties))
        return spec, cfg

    spec, cfg = model("a", ["TermsBelow3"])
    r = run(small + ["-predicates", str(pred), "-simulate", "num=1000", "-depth", "8", "-seed", "1", "-config", cfg, spec])
    assert r.returncode == 12, r.stdout + r.stderr
    assert "Checking in the walks: action properties TermsBelow3.\n" in r.stdout
    assert "Error: Action property TermsBelow3 is violated.\n" in r.stdout
    assert re.search(r"^Walk \d+ \(start state 0 of level 1\) violates at step \d+; rerun it with ", r.stdout, re.M)
    states = re.findall(r"^State (\d+): <(.*)>$", r.stdout, re.M)
    assert states[0] == ("1", "Initial predicate") and 3 <= len(states) <= 9 and states[-1][1].startswith("Timeout")
    assert [int(k) for k, _ in states] == list(range(1, len(states) + 1))
    assert "No error has been found" not in r.stdout
    spec, cfg = model("b", LAWS)
    r = run(small + ["-predicates", str(pred), "-simulate", "num=1000", "-depth", "8", "-seed", "1", "-config", cfg, spec])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Checking in the walks: action properties %s.\n" % ", ".join(LAWS) in r.stdout
    assert "No error has been found in 1 BFS levels and the walks above" in r.stdout
