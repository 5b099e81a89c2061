"""GPU tests of the predicate kernels (k_pred_state / k_pred_step, rtla_kpred.hip)
against the Python reference of tests/predgen.py directly, not against the host
replay: the generated corpus of tests/test_predfuzz_host.py through
rtla_pred_batch and rtla_pred_step_batch.  Only the existing batch entry points
are launched.

* the three host shapes: the clean rows bit for bit, counts, evaluated; an erring row among 70 fails the call;
* 300 rows of shape 0: two blocks, all four waves' operand files live, a different trip count on every lane;
* the other three instantiations of test_safety_gpu.SHAPES (N = 1, N = 4, the 64-slot / 32-election layout whose
  step tile holds fewer children than a state has successors: the operand files are reused tile after tile):
  batch equals replay on the full row set, replay equals the reference on 60 rows / 10 parents (wide: 3);
* the limit texts (operand depth 16, six variables, 8 definitions within 32 words of 512) on 300 rows: a lane
  that wrote past its operand file would change its neighbour's verdict.
"""
import functools

import pytest

import predgen as pg
import rtla
import test_predfuzz_host as host
from test_predfuzz_host import IDS, SETS, build_case, check_limit_sets, check_set, reference, shape_case
from test_safety_gpu import SHAPES as GPU_SHAPES

pytestmark = pytest.mark.gpu

OTHERS = GPU_SHAPES[3:]   # N = 1, N = 4, bag_cap 64 / elec_cap 32
OTHER_IDS = ["-".join(map(str, s[0])) + ("-wide" if "elec_cap" in s[1] else "") for s in OTHERS]
RUN = {"state": (rtla.pred_batch, rtla.pred_replay), "step": (rtla.pred_step_batch, rtla.pred_step_replay)}


@pytest.mark.parametrize("kind", ["state", "step"])
@pytest.mark.parametrize("k", range(3), ids=IDS)
def test_the_kernels_match_the_reference(k, kind):
    for g, group in enumerate(SETS[kind]):
        check_set(kind, group, reference(kind, k, g), shape_case(k), RUN[kind][0])


def test_two_blocks_of_state_rows_match_the_reference():
    case = shape_case(0, 300, 0)
    compared = 0
    for group in SETS["state"]:
        compared += check_set("state", group, host.verdicts("state", group, case), case, rtla.pred_batch, errors=1)[0]
    assert compared > 257 * len(SETS["state"]) // 2


def test_the_limit_texts_match_the_reference_on_two_blocks():
    check_limit_sets(shape_case(0, 300, 0), rtla.pred_batch)


@functools.lru_cache(maxsize=None)
def regrouped(limits):
    """The corpus for a layout of `limits` = (N, K, E): the definitions whose worst-case step count leaves room
    for eight of them, in sets of at most 8 (the wide layout drops those with several bag quantifiers)."""
    out = {}
    for kind, sets in SETS.items():
        fit = [d for group in sets for d in group if pg.cost(d[1], *limits) <= (1 << 20) // 8 - 2]
        out[kind] = [fit[g:g + 8] for g in range(0, len(fit), 8)]
    return out


def clean_rows(run, preds, rows):
    """(the rows on which the set evaluates without an error, the replay's result on them): by the host replay,
    row by row if some row errs."""
    try:
        return list(range(len(rows))), run(preds, rows)
    except rtla.RtlaError as e:
        assert e.status == rtla.E_SPEC
    out = []
    for k, r in enumerate(rows):
        try:
            run(preds, [r])
            out.append(k)
        except rtla.RtlaError as e:
            assert e.status == rtla.E_SPEC
    return out, run(preds, [rows[k] for k in out])


def other_sets(shape, kw, kind):
    limits = (shape[0], kw["bag_cap"], kw.get("elec_cap") or max(1, (shape[2] - 1) * shape[0]))
    sets = regrouped(limits)[kind]
    assert sum(map(len, sets)) >= (0.7 if "elec_cap" in kw else 1.0) * sum(map(len, SETS[kind]))
    return sets


@pytest.mark.parametrize("kind", ["state", "step"])
@pytest.mark.parametrize("shape,kw,n", OTHERS, ids=OTHER_IDS)
def test_the_other_instantiations_batch_equals_replay(shape, kw, n, kind):
    """On the full row set: the rows on which the replay reports no evaluation error give the same masks,
    counts and evaluated, and the whole set fails alike when a row errs."""
    cfg = rtla.Config(*shape, (), **kw)
    batch, replay = RUN[kind]
    rows = rtla.random_rows(cfg, 0, n)
    for group in other_sets(shape, kw, kind):
        with host.compile_set(cfg, group) as preds:
            ok, want = clean_rows(replay, preds, rows)
            assert batch(preds, [rows[k] for k in ok]) == want, host.set_text(group)
            if len(ok) < len(rows):
                with pytest.raises(rtla.RtlaError) as e:
                    batch(preds, rows)
                assert e.value.status == rtla.E_SPEC


@pytest.mark.parametrize("kind", ["state", "step"])
@pytest.mark.parametrize("shape,kw,n", OTHERS, ids=OTHER_IDS)
def test_the_other_instantiations_replay_equals_the_reference(shape, kw, n, kind):
    """60 rows / 10 parents of the same row stream (host work: it is what makes the comparison above one with
    the reference).  The wide layout: 3 parents -- its bags hold up to 64 messages, the reference visits every
    element of every bag quantifier on each of a parent's hundred-odd steps, and 10 parents took 27 s."""
    case = build_case(shape, kw, 60, 3 if "elec_cap" in kw else 10)
    assert case[2] == rtla.random_rows(case[0], 0, n)[:60]
    for group in other_sets(shape, kw, kind):
        check_set(kind, group, host.verdicts(kind, group, case), case, RUN[kind][1], errors=1)
