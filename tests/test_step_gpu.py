"""GPU tests of the action properties: the step kernel
(k_pred_step, rtla_kpred.hip) through rtla_pred_step_batch and
rtla_pred_step_frontier, and the search with actions= (Checker.run /
rtla.check).  The reference is the host replay (rtla.pred_step_replay), which
tests/test_step_host.py pins to Python functions over value-oracle steps."""
import json
import os

import pytest

import hostmodel
import raft_cpu
import raft_values as rv
import rtla
import tla_text
from test_safety_gpu import SHAPES
from test_step_host import LAWS, MC_PY, MCACTIONS, PROBE_SETS, _act, probe_text

pytestmark = pytest.mark.gpu

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "bfs_counts.json")))
SMALL = dict(fpset_log2=20, mem_budget=1 << 29)


def only(names):
    """The definitions `names` of specs/MCActions.tla, as a text of their own."""
    chunks = [c for c in MCACTIONS.split("\n\n") if any(ln.startswith(n + " ==") for n in names for ln in c.split("\n"))]
    text = "\n".join(ln for c in chunks for ln in c.split("\n") if not ln.startswith(("\\*", "====")))
    return text


@pytest.mark.parametrize("shape,kw,n", SHAPES, ids=lambda p: "-".join(map(str, p)) if isinstance(p, tuple) else None)
def test_batch_equals_replay(shape, kw, n):
    """N = 1..5 (every instantiation; N = 5: more than 64 fixed candidates,
    several candidate batches per state), row counts that are no multiple of
    the waves per block, and the 64-slot / 32-election layout whose child tile
    holds fewer rows than a state has enabled successors (several tiles per
    batch)."""
    cfg = rtla.Config(*shape, invariants=(), **kw)
    rows = rtla.random_rows(cfg, 0, n)[:300]
    for text in [MCACTIONS] + [probe_text(g) for g in PROBE_SETS]:
        with rtla.Actions(cfg, text) as acts:
            want = rtla.pred_step_replay(acts, rows)
            assert rtla.pred_step_batch(acts, rows) == want, acts.names
            assert shape[0] == 1 or (len(set(want[0])) > 1 and want[2] > 4 * len(rows))  # (both verdicts)
            assert rtla.pred_step_batch(acts, rows[:1]) == rtla.pred_step_replay(acts, rows[:1])
            assert rtla.pred_step_batch(acts, []) == ([], dict.fromkeys(acts.names, 0), 0)


def test_an_evaluation_error_on_any_step_fails_the_call():
    """One row with an erroring step hidden among 500 good rows, at a block's
    first and last wave."""
    shape, kw, n = SHAPES[0]
    cfg = rtla.Config(*shape, invariants=(), **kw)
    rows = rtla.random_rows(cfg, 0, n)
    with rtla.Actions(cfg, "A == " + _act(r"\A i \in Server : log'[i][1].term >= 1")) as acts:
        good, bad = [], []
        for r in rows:
            try:
                rtla.pred_step_replay(acts, [r])
                good.append(r)
            except rtla.RtlaError:
                bad.append(r)
        good = good[:500]
        assert len(good) == 500 and bad
        assert rtla.pred_step_batch(acts, good) == rtla.pred_step_replay(acts, good)
        for at in (0, 64, 67, 499):
            batch = list(good)
            batch[at] = bad[0]
            for run in (rtla.pred_step_batch, rtla.pred_step_replay):
                with pytest.raises(rtla.RtlaError) as e:
                    run(acts, batch)
                assert e.value.status == rtla.E_SPEC and e.value.flags & rtla.CAP_SPEC_ERROR, (at, run)


def check_trace(shape, tr):
    """Every step of the trace is a successor of its predecessor."""
    walk = raft_cpu.Walk(raft_cpu.cfg_of(*shape, ()))
    assert tr[0][0] == "Initial predicate" and walk.text() == tr[0][1]
    for label, text in tr[1:]:
        assert text in [t for _, t in walk.successors()], label
        walk.goto(text)
    return walk


def test_frontier_steps_in_place():
    g = GOLD["n2_v2_t3_l2_m1"]
    shape = (g["n_server"], g["n_value"], g["max_term"], g["max_log"], g["max_copies"], g["max_msgs"])
    cfg = rtla.Config(*shape, tuple(g["invariants"]), **SMALL)
    vc = rv.Cfg(shape[0], shape[1], shape[2], shape[3], shape[4], (), shape[5])
    with rtla.Checker(cfg) as ck, rtla.Actions(cfg, MCACTIONS) as acts:
        ck.init()
        res = ck.audit_steps(acts)  # Init: 2 Restarts that only change allLogs, 2 Timeouts
        assert res.status == rtla.VIOLATION and (res.audited, res.evaluated) == (1, 4)
        assert res.counts == dict(dict.fromkeys(acts.names, 0), TermsFrozen=2)
        for _ in range(11):
            assert ck.step() == rtla.OK
        assert len(ck.levels) == 12
        front = ck.frontier()
        masks, counts, evaluated = rtla.pred_step_replay(acts, front)
        res = ck.audit_steps(acts)
        assert res.status == rtla.VIOLATION and res.counts == counts
        assert (res.audited, res.evaluated) == (len(front), evaluated)
        assert [counts[n] for n in LAWS] == [0] * 5 and counts["TermsFrozen"] > 0 and len(set(masks)) > 1
        first = next(k for k, m in enumerate(masks) if m)
        # 840 rows, many of them with a false step, found by different blocks (four states each): the least is reported
        assert len(front) > 256 and len({k // 4 for k, m in enumerate(masks) if m}) > 1
        # the least false instance of that row, from the Python functions over the row's successors in instance order
        s = tla_text.parse_state(vc, rtla.state_text(cfg, front[first]))
        inst, mask, in_model = next(
            (i, m, im) for i, m, im in (
                (i, sum(1 << k for k, n in enumerate(acts.names) if t != s and not MC_PY[n](vc, s, t)), im)
                for _, i, _, im, row in hostmodel.expand(cfg, [front[first]], rtla.row_words(cfg))
                for t in [tla_text.parse_state(vc, rtla.state_text(cfg, row))]) if m)
        assert (res.viol_index, res.viol_inst, res.viol_mask, res.viol_in_model) == (first, inst, mask, in_model)
        assert res.violation == acts.names_of(mask) and ck.violation() == (", ".join(res.violation), in_model)
        tr = ck.trace()
        assert len(tr) == 13 and tr[-2][1] == rtla.state_text(cfg, front[first])
        check_trace(shape, tr)
        # a set compiled for another layout, and a set of the other kind, are refused
        with rtla.Actions(rtla.Config(3, 1, 3, 1, 1, 1, ()), MCACTIONS) as other, \
                rtla.Predicates(cfg, "P == TRUE") as preds:
            for call, arg in ((ck.audit_steps, other), (ck.audit_steps, preds), (ck.audit_predicates, acts)):
                with pytest.raises(rtla.RtlaError) as e:
                    call(arg)
                assert e.value.status == rtla.E_ARG
        # the search was not touched
        for lv in range(12, 16):
            assert ck.step() == rtla.OK
            assert [ck.levels[-1].new, ck.levels[-1].generated] == g["levels"][lv]


def test_search_with_actions():
    shape = (2, 1, 2, 1, 1, 1)
    cfg = rtla.Config(*shape, (), fpset_log2=16, mem_budget=1 << 28)
    with rtla.Actions(cfg, only(LAWS)) as laws:
        assert laws.names == LAWS
        res = rtla.check(cfg, actions=laws)
    assert res.violation is None and res.distinct == GOLD["n2_v1_t2_l1_m1"]["distinct"]
    assert [[lv.new, lv.generated] for lv in res.levels] == GOLD["n2_v1_t2_l1_m1"]["levels"]
    with rtla.Actions(cfg, only(["LeadersStay"])) as acts:
        assert acts.names == ["LeadersStay"]
        res = rtla.check(cfg, actions=acts)
    assert res.violation == "LeadersStay" and len(res.levels) == 10 and len(res.trace) == 11
    assert res.trace[-1][0].startswith("Restart")
    assert res.trace[-2][1].count('"Leader"') > res.trace[-1][1].count('"Leader"')
    check_trace(shape, res.trace)


def test_commit_never_decreases_fails_where_the_first_commit_is():
    shape = (2, 2, 3, 2, 1, 1)
    cfg = rtla.Config(*shape, invariants=(), **SMALL)
    with rtla.Checker(cfg) as ck, rtla.Actions(cfg, only(["CommitNeverDecreases"])) as acts:
        assert ck.run(actions=acts) == rtla.VIOLATION
        assert len(ck.levels) == 16 and ck.violation()[0] == "CommitNeverDecreases"
        assert ck.audit_steps(acts).counts == {"CommitNeverDecreases": 4}
        tr = ck.trace()
    assert len(tr) == 17 and tr[-1][0].startswith("Restart")
    check_trace(shape, tr)


def test_preconditions():
    small = dict(fpset_log2=16, mem_budget=1 << 28)
    base = rtla.Config(2, 1, 2, 1, 1, 1, (), **small)
    with rtla.Actions(base, only(LAWS)) as acts:
        for kw, init in ((dict(shards=2), True), (dict(dedup_only=True), False), ({}, False)):
            with rtla.Checker(rtla.Config(2, 1, 2, 1, 1, 1, (), **kw, **small)) as ck:
                if init:
                    ck.init()
                with pytest.raises(rtla.RtlaError) as e:
                    ck.audit_steps(acts)
                assert e.value.status == rtla.E_STATE
