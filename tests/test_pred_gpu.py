"""GPU tests of the user-defined predicates: the interpreter kernel
(rtla_kpred.hip) through rtla_pred_batch and rtla_pred_frontier, and the search
with user invariants (Checker.run / rtla.check with predicates=).  The
reference is the host replay (rtla.pred_replay), which tests/test_pred_host.py
pins to rtla_check_replay and to Python predicates over value-oracle states."""
import json
import os

import pytest

import raft_cpu
import rtla
from test_pred_host import FIELD_SETS, MCPRED
from test_safety_gpu import NTL, SHAPES

pytestmark = pytest.mark.gpu

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "bfs_counts.json")))
FIELD_TEXTS = ["\n".join("%s == %s" % (name, src) for name, src, _ in group) for group in FIELD_SETS]


@pytest.mark.parametrize("shape,kw,n", SHAPES, ids=lambda p: "-".join(map(str, p)) if isinstance(p, tuple) else None)
def test_batch_equals_replay(shape, kw, n):
    """Row counts that are no multiple of 64 or of the staging tile, N = 1..5
    (every instantiation), and the 64-slot / 32-election layout whose tiles
    hold fewer than 64 rows."""
    cfg = rtla.Config(*shape, invariants=(), **kw)
    rows = rtla.random_rows(cfg, 0, n)
    for text in [MCPRED] + FIELD_TEXTS:
        with rtla.Predicates(cfg, text) as preds:
            want = rtla.pred_replay(preds, rows)
            assert rtla.pred_batch(preds, rows) == want, preds.names
            assert shape[0] == 1 or len(set(want[0])) > 1  # (both verdicts, whatever the set holds)
            assert rtla.pred_batch(preds, rows[:1]) == rtla.pred_replay(preds, rows[:1])
            assert rtla.pred_batch(preds, []) == ([], dict.fromkeys(preds.names, 0))


def test_an_evaluation_error_on_any_lane_fails_the_call():
    """Two erroring rows hidden in 500 good ones, at a staging tile's first and
    last lane (rows 64 and 127: the first and last row of a wave's second group
    of 64, whatever power of two the tile holds)."""
    shape, kw, n = SHAPES[0]
    cfg = rtla.Config(*shape, invariants=(), **kw)
    rows = rtla.random_rows(cfg, 0, n)
    with rtla.Predicates(cfg, r"SomeLogEmpty == \E i \in Server : Len(log[i]) = 0") as split:
        empty = [m == 0 for m in rtla.pred_replay(split, rows)[0]]  # (a mask holds the FALSE definitions)
    good = [r for r, e in zip(rows, empty) if not e][:500]
    bad = [r for r, e in zip(rows, empty) if e][:2]
    assert len(good) == 500 and len(bad) == 2
    with rtla.Predicates(cfg, r"FirstEntries == \A i \in Server : log[i][1].term >= 1") as preds:
        assert rtla.pred_batch(preds, good) == rtla.pred_replay(preds, good) == ([0] * 500, {"FirstEntries": 0})
        for places in ((64,), (127,), (64, 127)):
            batch = list(good)
            for k, at in enumerate(places):
                batch[at] = bad[k]
            for run in (rtla.pred_batch, rtla.pred_replay):
                with pytest.raises(rtla.RtlaError) as e:
                    run(preds, batch)
                assert e.value.status == rtla.E_SPEC and e.value.flags & rtla.CAP_SPEC_ERROR, (places, run)


WITNESSES = "\n".join([
    r"NoCandidate == \A i \in Server : state[i] # Candidate",
    r"NoVoteRequest == \A m \in DOMAIN messages : m.mtype # RequestVoteRequest",
    r"FirstTerm == \A i \in Server : currentTerm[i] = 1",
    r"NobodyVoted == \A i \in Server : votedFor[i] = Nil",
    r"NoElection == Cardinality(elections) = 0",
    r"AlwaysTrue == TRUE"])


def test_frontier_audit_in_place():
    g = GOLD["n2_v2_t3_l2_m1"]
    cfg = rtla.Config(g["n_server"], g["n_value"], g["max_term"], g["max_log"], g["max_copies"], g["max_msgs"],
                      tuple(g["invariants"]), fpset_log2=20, mem_budget=1 << 29)
    with rtla.Checker(cfg) as ck, rtla.Predicates(cfg, WITNESSES) as preds, rtla.Predicates(cfg, MCPRED) as mc:
        ck.init()
        res = ck.audit_predicates(preds)  # Init: everything holds
        assert res.status == rtla.OK and res.audited == res.evaluated == 1 and set(res.counts.values()) == {0}
        for _ in range(7):
            assert ck.step() == rtla.OK
        assert len(ck.levels) == 8
        front = ck.frontier()
        masks, counts = rtla.pred_replay(preds, front)
        res = ck.audit_predicates(preds)
        assert res.status == rtla.VIOLATION and res.counts == counts and res.audited == res.evaluated == len(front)
        assert 0 < counts["NoCandidate"] < len(front) and counts["AlwaysTrue"] == 0 and len(set(masks)) > 3
        first = next(k for k, m in enumerate(masks) if m)
        # 258 rows: two blocks (four waves of 64 rows each), both with false rows; the least of them is reported
        assert len(front) > 256 and any(masks[:256]) and any(masks[256:])
        assert (res.viol_index, res.viol_mask, res.viol_inst, res.viol_in_model) == (first, masks[first], -1, True)
        assert res.violation == preds.names_of(masks[first])
        assert ck.violation() == (", ".join(res.violation), True)
        tr = ck.trace()
        assert len(tr) == 8 and tr[0][0] == "Initial predicate" and tr[-1][1] == rtla.state_text(cfg, front[first])
        # the built-ins restated hold where the search's own invariants hold
        res = ck.audit_predicates(mc)
        assert res.status == rtla.OK and ck.violation() == (None, False)
        assert res.counts == rtla.pred_replay(mc, front)[1]
        # a set compiled for another layout is refused; the search was not touched
        with rtla.Predicates(rtla.Config(3, 1, 3, 1, 1, 1, ()), "P == TRUE") as other:
            with pytest.raises(rtla.RtlaError) as e:
                ck.audit_predicates(other)
            assert e.value.status == rtla.E_ARG
        for lv in range(8, 12):
            assert ck.step() == rtla.OK
            assert [ck.levels[-1].new, ck.levels[-1].generated] == g["levels"][lv]


def check_trace(shape, tr):
    """Every step of the trace is a successor of its predecessor (the check
    tests/test_safety_gpu.py applies to an audit's trace)."""
    walk = raft_cpu.Walk(raft_cpu.cfg_of(*shape, ()))
    assert tr[0][0] == "Initial predicate" and walk.text() == tr[0][1]
    for label, text in tr[1:]:
        assert text in [t for _, t in walk.successors()], label
        walk.goto(text)
    return walk


def test_search_with_a_user_invariant():
    """PNoTwoLeaders as the only invariant of n3_v1_t3_l1_m1_ntl's shape: the
    run stops where the golden run with the built-in stops."""
    g = GOLD["n3_v1_t3_l1_m1_ntl"]
    assert g["invariants"] == ["NoTwoLeaders"] and g["violated"] == 1
    shape = (3, 1, 3, 1, 1, 1)
    cfg = rtla.Config(*shape, invariants=(), **NTL)
    text = "\n".join(ln for ln in MCPRED.split("\n\n") if ln.startswith("PNoTwoLeaders"))
    with rtla.Predicates(cfg, text) as preds:
        assert preds.names == ["PNoTwoLeaders"]
        res = rtla.check(cfg, predicates=preds)
    assert res.violation == "PNoTwoLeaders" and res.violation_in_model
    assert len(res.levels) == g["depth"] == 19 and len(res.trace) == g["trace_len"] == 19
    # (every level up to the violation is complete: the audit runs after the level, not inside it)
    assert [[lv.new, lv.generated] for lv in res.levels[:18]] == g["levels"][:18]
    check_trace(shape, res.trace)
    assert res.trace[-1][1].count('"Leader"') >= 2
    # without the argument nothing is checked: the same levels, no violation
    with rtla.Checker(cfg) as ck:
        assert ck.run(max_levels=6) == rtla.OK and ck.violation() == (None, False)


# The level at which the value oracle (oracle/raft_values.py next_states / in_model, a plain BFS of the in-model
# states of Cfg(2, 2, 3, 2, 1, (), 1)) first meets a state with a leader whose commitIndex >= 1, and how many states
# of that level are such: recorded from that run (levels 1..15 hold none; level 16 has 2292 states, as the golden
# n2_v2_t3_l2_m1 counts say).
NOCOMMIT_LEVEL, NOCOMMIT_HITS = 16, 4


def test_witness_idiom_finds_the_first_commit():
    shape = (2, 2, 3, 2, 1, 1)
    cfg = rtla.Config(*shape, invariants=(), fpset_log2=20, mem_budget=1 << 29)
    text = r"NoCommit == ~ \E i \in Server : state[i] = Leader /\ commitIndex[i] >= 1"
    with rtla.Checker(cfg) as ck, rtla.Predicates(cfg, text) as preds:
        assert ck.run(predicates=preds) == rtla.VIOLATION
        assert len(ck.levels) == NOCOMMIT_LEVEL and ck.violation() == ("NoCommit", True)
        assert ck.audit_predicates(preds).counts == {"NoCommit": NOCOMMIT_HITS}
        tr = ck.trace()
    assert len(tr) == NOCOMMIT_LEVEL
    walk = check_trace(shape, tr)
    import raft_values as rv
    import tla_text
    last = tla_text.parse_state(rv.Cfg(2, 2, 3, 2, 1, (), 1), walk.text())
    assert any(last[rv.IX["state"]][i] == rv.LEADER and last[rv.IX["commitIndex"]][i] >= 1 for i in range(2))


def test_preconditions():
    small = dict(fpset_log2=16, mem_budget=1 << 28)
    base = rtla.Config(2, 1, 2, 1, 1, 1, (), **small)
    with rtla.Predicates(base, "P == TRUE") as preds:
        for kw, init in ((dict(shards=2), True), (dict(dedup_only=True), False), ({}, False)):
            with rtla.Checker(rtla.Config(2, 1, 2, 1, 1, 1, (), **kw, **small)) as ck:
                if init:
                    ck.init()
                with pytest.raises(rtla.RtlaError) as e:
                    ck.audit_predicates(preds)
                assert e.value.status == rtla.E_STATE
        with rtla.Checker(base) as ck:  # a complete search: every level audited, the empty last one skipped
            assert ck.run(predicates=preds) == rtla.DONE
            assert ck.distinct == GOLD["n2_v1_t2_l1_m1"]["distinct"]
