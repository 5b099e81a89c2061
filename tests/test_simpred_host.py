"""CPU tests of the random walks that carry user properties (DESIGN.md section
15): the host replay rtla_sim_replay_pred / rtla_sim_walk_pred, the reference
the GPU walks (tests/test_simpred_gpu.py) are compared with bit for bit.

The walks are re-derived here: successors from the host-compiled model
(hostmodel), the draw from its published formulas (test_sim_host), and the
witnesses below evaluated in Python on states parsed from their text, written
from the TLA+ alone as MC_PY in test_step_host.py."""
import ctypes as C
import os

import pytest

import hostmodel
import raft_values as rv
import rtla
import tla_text
from test_sim_host import SHAPES, draw, path_term
from test_step_host import MCACTIONS, UNGUARDED, _act, _bag, _v, model_levels  # noqa: F401 (a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MCPRED = open(os.path.join(ROOT, "specs", "MCPredicates.tla")).read()
LAWS_TEXT = MCACTIONS[:MCACTIONS.index("\\* ---- witnesses")]      # the five laws of specs/MCActions.tla
BUILTINS_TEXT = MCPRED[:MCPRED.index("(* The witness idiom")]      # the five built-ins restated
LAWS = ["LeaderAppendOnly", "TermsNeverDecrease", "OneVotePerTerm", "BagChangesByOne", "ElectionsGrow"]
RESTATED = ["PNoTwoLeaders", "PElectionSafety", "PLogMatching", "PStateMachineSafety", "PLeaderCompleteness"]
M64 = (1 << 64) - 1
SEED = 20261021

# Witnesses: definitions that are no laws.  (specs/MCActions.tla is full at 8.)
WITNESS_ACTIONS = r"""
TermsBelow3 == [][\A i \in Server : currentTerm'[i] <= 2]_vars
BagNeverShrinks == [][BagCardinality(messages') >= BagCardinality(messages)]_vars
"""
WITNESS_STATES = r"""
NoVoteRequest == \A m \in DOMAIN messages : m.mtype # RequestVoteRequest
"""
ACTIONS_PY = [  # (name, f(cfg, s, t)), in definition order
    ("TermsBelow3", lambda c, s, t: all(_v(t, "currentTerm")[i] <= 2 for i in range(c.n_server))),
    ("BagNeverShrinks", lambda c, s, t: _bag(t) >= _bag(s)),
]
STATES_PY = [  # (name, f(cfg, s))
    ("NoVoteRequest", lambda c, s: all(m["mtype"] != rv.RVREQ for m, _ in _v(s, "messages").items())),
]


def word4(inst, in_model, inv, smask, amask):
    return inst | int(in_model) << 16 | inv << 24 | smask << 32 | amask << 40


class Rederivation:
    """The walks of one shape in Python."""

    def __init__(self, shape, invariants=()):
        n, v, t, l, c, m = shape
        self.cfg = rtla.Config(n, v, t, l, c, m, tuple(invariants))
        self.vc = rv.Cfg(n, v, t, l, c, (), m)
        self.words = rtla.row_words(self.cfg)
        self._succ, self._state, self.expanded = {}, {}, []

    def state(self, row):
        key = tuple(row)
        if key not in self._state:
            self._state[key] = tla_text.parse_state(self.vc, rtla.state_text(self.cfg, row))
        return self._state[key]

    def successors(self, row):
        """[(instance, in_model, row, built-in mask, state mask, step mask)] in instance order."""
        key = tuple(row)
        if key not in self._succ:
            s, out = self.state(row), []
            for _, inst, _, in_model, child in hostmodel.expand(self.cfg, [row], self.words):
                t = self.state(child)
                amask = 0 if t == s else sum(1 << k for k, (_, f) in enumerate(ACTIONS_PY) if not f(self.vc, s, t))
                smask = sum(1 << k for k, (_, f) in enumerate(STATES_PY) if not f(self.vc, t)) if in_model else 0
                out.append((inst, in_model, child, rtla.invariants_violated(self.cfg, child), smask, amask))
            assert [x[0] for x in out] == sorted(x[0] for x in out)
            self._succ[key] = out
        return self._succ[key]

    def walk(self, start, w, depth, seed):
        """(rows entered, the 5 fields + word 4 of its end record, the violating row or None); self.expanded
        gains the successor lists the walk evaluated."""
        row, rows = start, []
        for t in range(1, depth + 1):
            succ = self.successors(row)
            self.expanded.append(succ)
            bad = [x for x in succ if x[3] | x[4] | x[5]]
            if bad:
                inst, in_model, child, inv, smask, amask = bad[0]
                return rows, self.record(row, rows, rtla.SIM_STOP_VIOLATION, word4(inst, in_model, inv, smask, amask)), child
            model = [x for x in succ if x[1]]
            if not model:
                return rows, self.record(row, rows, rtla.SIM_STOP_STUCK, 0), None
            row = model[draw(seed, w, t, len(model))][2]
            rows.append(row)
        return rows, self.record(row, rows, rtla.SIM_STOP_DEPTH, 0), None

    @staticmethod
    def record(last, rows, stop, w4):
        digest = sum(path_term(rtla.stored_fingerprint(r), t + 1) for t, r in enumerate(rows)) & M64
        return rtla.stored_fingerprint(last) + (digest, len(rows), stop, w4)


def witness_sets(cfg):
    return rtla.Predicates(cfg, WITNESS_STATES), rtla.Actions(cfg, WITNESS_ACTIONS)


# ---- 1. re-derivation

@pytest.mark.parametrize("shape", SHAPES)
def test_walks_match_independent_rederivation(shape):
    rd = Rederivation(shape)
    cfg, init, walks, depth = rd.cfg, rtla.init_row(rd.cfg), 64, 6
    preds, acts = witness_sets(cfg)
    assert preds.names == [n for n, _ in STATES_PY] and acts.names == [n for n, _ in ACTIONS_PY]
    res = rtla.sim_replay(cfg, [init], walks, depth, seed=SEED, predicates=preds, actions=acts)
    mine = [rd.walk(init, w, depth, SEED) for w in range(walks)]
    # what the reference must show: violations at >= 3 distinct steps, one at step >= 3, a walk that runs to depth
    stops = [(len(rows) + 1) for rows, rec, _ in mine if rec[4] == rtla.SIM_STOP_VIOLATION]
    assert len(set(stops)) >= 3 and max(stops) >= 3, stops
    assert any(rec[4] == rtla.SIM_STOP_DEPTH and rec[3] == depth for _, rec, _ in mine)
    assert len({rec[5] >> 32 for _, rec, _ in mine}) >= 2  # more than one combination of masks
    # every field of the 5-word records: fingerprint, digest, stop step, stop code; instance, in_model, three masks
    assert res.ends == [rec for _, rec, _ in mine]
    for w in range(walks):
        rows, rec, last = mine[w]
        violating, steps = rtla.sim_walk(cfg, init, w, depth, seed=SEED, predicates=preds, actions=acts)
        assert violating == (last is not None)
        assert [r for _, _, r in steps] == rows + ([last] if violating else [])
        if violating:
            assert steps[-1][0] == rec[5] & 0xFFFF
    # the reported violation: the least walk's, with the names of every false thing of that successor
    first = next(w for w in range(walks) if mine[w][1][4] == rtla.SIM_STOP_VIOLATION)
    w4 = mine[first][1][5]
    assert res.status == rtla.VIOLATION
    assert (res.viol_walk, res.viol_step, res.viol_inst) == (first, mine[first][1][3] + 1, w4 & 0xFFFF)
    assert (res.viol_in_model, res.viol_mask, res.viol_state_mask, res.viol_step_mask) == \
           (bool(w4 >> 16 & 1), w4 >> 24 & 255, w4 >> 32 & 255, w4 >> 40 & 255)
    assert res.violation == ", ".join(preds.names_of(res.viol_state_mask) + acts.names_of(res.viol_step_mask))
    # the counters, from the states the Python walks visited
    assert res.generated == res.step_evaluated == sum(len(s) for s in rd.expanded)
    assert res.state_evaluated == sum(1 for s in rd.expanded for x in s if x[1])
    assert res.steps == sum(len(rows) for rows, _, _ in mine)


def test_terms_below_3_first_fails_one_step_after_the_first_timeout():
    """From Init, Restart changes only allLogs and Timeout is always enabled."""
    rd = Rederivation(SHAPES[0])
    cfg, init = rd.cfg, rtla.init_row(rd.cfg)
    with rtla.Actions(cfg, WITNESS_ACTIONS.split("\n")[1]) as acts:
        assert acts.names == ["TermsBelow3"]
        res = rtla.sim_replay(cfg, [init], 64, 6, seed=SEED, actions=acts)
        seen = 0
        for w in range(64):
            _, steps = rtla.sim_walk(cfg, init, w, 6, seed=SEED, actions=acts)
            names = [rtla.action_name(cfg, i, sub) for i, sub, _ in steps]
            if res.ends[w][4] == rtla.SIM_STOP_VIOLATION:
                first = next(k for k, nm in enumerate(names) if nm.startswith("Timeout"))
                assert first == len(names) - 2 and names[-1].startswith("Timeout") and res.ends[w][5] >> 40 == 1
                seen += 1
            else:
                assert not any(nm.startswith("Timeout") for nm in names[:-1])
        assert seen >= 32


# ---- 2. agreement with the level passes

def test_depth_one_walks_agree_with_the_level_passes(model_levels):
    cfg, vc, levels = model_levels
    words = rtla.row_words(cfg)
    preds, acts = witness_sets(cfg)
    false_steps = false_states = 0
    for rows, _ in levels:
        n = len(rows)
        masks, _, evaluated = rtla.pred_step_replay(acts, rows)
        res = rtla.sim_replay(cfg, rows, n, 1, seed=SEED, predicates=preds, actions=acts)
        only_a = rtla.sim_replay(cfg, rows, n, 1, seed=SEED, actions=acts)
        only_p = rtla.sim_replay(cfg, rows, n, 1, seed=SEED, predicates=preds)
        assert res.step_evaluated == only_a.step_evaluated == evaluated == res.generated
        succ = hostmodel.expand(cfg, rows, words)
        children = [x for x in succ if x[3]]
        cmasks = rtla.pred_replay(preds, [x[4] for x in children])[0] if children else []
        assert res.state_evaluated == only_p.state_evaluated == len(children)
        state_bad = [False] * n
        for x, m in zip(children, cmasks):
            state_bad[x[0]] |= m != 0
        for w in range(n):
            assert (only_a.ends[w][4] == rtla.SIM_STOP_VIOLATION) == (masks[w] != 0)
            assert (only_p.ends[w][4] == rtla.SIM_STOP_VIOLATION) == state_bad[w]
            assert (res.ends[w][4] == rtla.SIM_STOP_VIOLATION) == (masks[w] != 0 or state_bad[w])
            if masks[w]:
                assert only_a.ends[w][5] >> 40 and not only_a.ends[w][5] >> 32 & 255
        false_steps += sum(1 for m in masks if m)
        false_states += sum(state_bad)
    assert false_steps > 100 and false_states > 100


# ---- 3. laws change nothing

@pytest.mark.parametrize("shape", SHAPES)
def test_laws_change_nothing(shape):
    n, v, t, l, c, m = shape
    cfg = rtla.Config(n, v, t, l, c, m, ())
    init = rtla.init_row(cfg)
    words = rtla.row_words(cfg)
    rows = [init] + [x[4] for x in hostmodel.expand(cfg, [init], words) if x[3]]
    plain = rtla.sim_replay(cfg, rows, 200, 25, seed=SEED, first=3)
    with rtla.Predicates(cfg, BUILTINS_TEXT) as preds, rtla.Actions(cfg, LAWS_TEXT) as acts:
        assert preds.names == RESTATED and acts.names == LAWS
        res = rtla.sim_replay(cfg, rows, 200, 25, seed=SEED, first=3, predicates=preds, actions=acts)
    assert res.status == plain.status == rtla.OK and res.violation is None
    assert [e[:5] for e in res.ends] == plain.ends and all(e[5] == 0 for e in res.ends)
    assert (res.steps, res.generated, res.stuck, res.taken) == (plain.steps, plain.generated, plain.stuck, plain.taken)
    assert res.step_evaluated == res.generated and 0 < res.state_evaluated <= res.generated
    assert (res.viol_state_mask, res.viol_step_mask) == (0, 0)


# ---- 4. errors, arguments and determinism

def test_a_stuttering_step_satisfies_every_action(model_levels):
    cfg, _, levels = model_levels
    rows = levels[1][0]  # level 2: 16 steps, 4 of them stuttering (test_step_host)
    with rtla.Actions(cfg, "Stutter == [][FALSE]_vars") as acts:
        res = rtla.sim_replay(cfg, rows, len(rows), 1, seed=SEED, actions=acts)
        assert res.step_evaluated == 16 and all(e[4] == rtla.SIM_STOP_VIOLATION for e in res.ends)
        # a row whose least instance stutters stops on a later one
        words = rtla.row_words(cfg)
        stutter_first = 0
        for w, row in enumerate(rows):
            succ = hostmodel.expand(cfg, [row], words)
            moving = [x[1] for x in succ if x[4] != row]
            assert res.ends[w][5] & 0xFFFF == moving[0]
            stutter_first += moving[0] != succ[0][1]
        assert stutter_first >= 1


@pytest.mark.parametrize("bad,good", UNGUARDED)
def test_an_evaluation_error_fails_the_call(bad, good):
    cfg = rtla.Config(3, 2, 3, 2, 1, 3, ())
    init = rtla.init_row(cfg)
    with rtla.Actions(cfg, "A == " + _act(bad)) as acts:
        with pytest.raises(rtla.RtlaError) as e:
            rtla.sim_replay(cfg, [init], 20, 6, seed=SEED, actions=acts)
        assert e.value.status == rtla.E_SPEC and e.value.flags & rtla.CAP_SPEC_ERROR
        with pytest.raises(rtla.RtlaError) as e:
            rtla.sim_walk(cfg, init, 0, 6, seed=SEED, actions=acts)
        assert e.value.status == rtla.E_SPEC
    with rtla.Actions(cfg, "A == " + _act(good)) as acts:
        res = rtla.sim_replay(cfg, [init], 20, 6, seed=SEED, actions=acts)
        assert res.status == rtla.OK and res.step_evaluated == res.generated
    # a state program's error, too: votedFor is Nil in Init's successors
    with rtla.Predicates(cfg, r"P == \A i \in Server : currentTerm[votedFor[i]] >= 1") as preds:
        with pytest.raises(rtla.RtlaError) as e:
            rtla.sim_replay(cfg, [init], 20, 6, seed=SEED, predicates=preds)
        assert e.value.status == rtla.E_SPEC


def test_argument_errors():
    cfg, other = rtla.Config(3, 2, 3, 2, 1, 3, ()), rtla.Config(2, 1, 3, 1, 2, 0, ())
    init = rtla.init_row(cfg)
    w = rtla.row_words(cfg)
    preds, acts = witness_sets(cfg)
    opreds, oacts = witness_sets(other)
    for kw in (dict(predicates=acts), dict(actions=preds), dict(predicates=preds, actions=preds),
               dict(predicates=opreds), dict(actions=oacts), dict(predicates=preds, actions=oacts)):
        with pytest.raises(rtla.RtlaError) as e:
            rtla.sim_replay(cfg, [init], 4, 3, **kw)
        assert e.value.status == rtla.E_ARG, kw
        with pytest.raises(rtla.RtlaError) as e:
            rtla.sim_walk(cfg, init, 0, 3, **kw)
        assert e.value.status == rtla.E_ARG, kw
    # both sets NULL: the C ABI refuses (Python makes the plain call instead)
    cc, arr = cfg.c(), (C.c_uint32 * w)(*init)
    ends, st, pst, n = (C.c_uint64 * 20)(), rtla._SimStats(), rtla._SimPredStats(), C.c_size_t(0)
    assert rtla._lib.rtla_sim_replay_pred(C.byref(cc), arr, 1, 1, 0, 4, 3, 1, None, None, ends, C.byref(st),
                                          C.byref(pst)) == rtla.E_ARG
    assert rtla._lib.rtla_sim_walk_pred(C.byref(cc), arr, 1, 0, 3, None, None, None, None, 0, C.byref(n)) == rtla.E_ARG
    assert rtla._lib.rtla_simulate_pred(None, 1, 0, 4, 3, preds._h, acts._h, None, None, None) == rtla.E_ARG
    # without the new arguments: today's call, today's result
    plain = rtla.sim_replay(cfg, [init], 4, 3)
    assert len(plain.ends[0]) == 5 and (plain.state_evaluated, plain.step_evaluated) == (0, 0)
    assert rtla._lib.rtla_abi_version() == 12


def test_replay_is_independent_of_threads_and_of_how_the_range_is_split():
    cfg = rtla.Config(3, 2, 3, 2, 1, 3, ())
    init = rtla.init_row(cfg)
    preds, acts = witness_sets(cfg)
    kw = dict(seed=SEED, predicates=preds, actions=acts)
    one = rtla.sim_replay(cfg, [init], 300, 8, first=11, threads=1, **kw)
    many = rtla.sim_replay(cfg, [init], 300, 8, first=11, threads=16, **kw)
    fields = lambda r: (r.status, r.ends, r.steps, r.generated, r.stuck, r.taken, r.state_evaluated, r.step_evaluated,
                        r.violation, r.viol_walk, r.viol_step, r.viol_inst, r.viol_mask, r.viol_state_mask,
                        r.viol_step_mask, r.viol_in_model)
    assert fields(one) == fields(many) and one.status == rtla.VIOLATION
    assert len({e[4] for e in one.ends}) == 2  # walks that stop on a violation and walks that run to depth
    a = rtla.sim_replay(cfg, [init], 120, 8, first=11, **kw)
    b = rtla.sim_replay(cfg, [init], 180, 8, first=131, **kw)
    assert a.ends + b.ends == one.ends
    assert a.steps + b.steps == one.steps and a.generated + b.generated == one.generated
    assert a.state_evaluated + b.state_evaluated == one.state_evaluated
    assert a.step_evaluated + b.step_evaluated == one.step_evaluated
    assert (a.viol_walk, a.viol_step, a.viol_inst, a.violation) == (one.viol_walk, one.viol_step, one.viol_inst,
                                                                    one.violation)
