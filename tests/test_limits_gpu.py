"""GPU parity at the limits of the packed row format (tests/limits.py): 3-bit
terms, 2-bit values, 5-entry own logs, 4-bit message counts up to C + 1 = 15,
20- to 26-word allLogs masks, two-word bag slots, all 64 bag slots and 32
election records in use, and the 256-instance boundary between the compacting
level kernel and the wave-per-state kernel.

The host tests (test_model_host.py and the other *_host.py files) pin the
shared model code at these shapes against the value oracle; here the same cases
run through the code that only the GPU has: the level kernel's per-lane child
row assembly (every successor row word for word against the host model's, as
tests/test_rowbuild_gpu.py does for whole searches), its LDS tiles, SYMMETRY's
patched signatures, the audit / predicate / step kernels' field reads and the
fingerprint set behind the dedup-only kernel.  Every comparison is exact."""
import collections
import json

import pytest

import hostmodel
import limits
import raft_values as rv
import rtla
import tla_text
from test_model_host import assert_full_bag_successors
from test_pred_host import MCPRED
from test_safety_host import ALL as ALL_INV
from test_step_host import MCACTIONS

pytestmark = pytest.mark.gpu


def assert_rows_equal(got, want, what):
    """Two successor listings (input, instance, receive-sub, in_model, row), entry for entry; a differing
    row is reported by its words."""
    assert len(got) == len(want), "%s: %d successors, the host model derives %d" % (what, len(got), len(want))
    for g, h in zip(got, want):
        assert tuple(g[:4]) == tuple(h[:4]), "%s: %s, the host model has %s" % (what, g[:4], h[:4])
        if tuple(g[4]) != tuple(h[4]):
            diff = [w for w in range(len(h[4])) if g[4][w] != h[4][w]]
            raise AssertionError("%s: successor %d of input %d differs in words %s: word %d is %#x, the host model "
                                 "has %#x" % (what, g[1], g[0], diff, diff[0], g[4][diff[0]], h[4][diff[0]]))


@pytest.mark.parametrize("name", limits.ALL)
def test_driver_runs_the_kernel_the_table_names(name):
    """The level kernel that serves each shape, by the driver's own choice: a sharded context sizes its
    overflow list for the compacting kernel's groups, 0 when the wave-per-state kernel runs the layout
    (the rule by which expand_batch picks its kernel too)."""
    c = limits.case(name)
    assert limits.kernel_of(c.cfg)[0] == c.kernel
    with rtla.Checker(c.with_cfg(shards=2, fpset_log2=16, mem_budget=1 << 28)) as ck:
        info = json.loads(ck.device_info())
    assert (info["overflow_records"] > 0) == c.kernel.startswith("compact"), info


@pytest.mark.parametrize("name", limits.ALL)
def test_successors_match_value_oracle_and_host_rows(name):
    """rtla.expand_batch over a limit shape's sample: the value oracle's successors state by state (texts
    and in-model flags), and every successor row the host model's word for word, stored fingerprint
    included -- a child-row assembly bug that still decodes to a plausible text shows as a named word."""
    c = limits.case(name)
    limits.assert_witnessed(c, "expand_batch")
    got = rtla.expand_batch(c.cfg, [list(r) for r in c.rows])
    by = collections.defaultdict(list)
    for k, _, _, im, r in got:
        by[k].append((im, rtla.state_text(c.cfg, r)))
    for k in range(len(c.rows)):
        assert sorted(by[k]) == list(c.ref[k]), "input state %d" % k
    assert_rows_equal(got, limits.host_expand(name), name)


@pytest.mark.parametrize("name", limits.SYMMETRIC)
def test_symmetry_successors_and_orbits(name):
    """The same through the SYMMETRY instantiation of the level kernel (N = 5 and N = 4), and the successors
    grouped into orbits by the product's orbit key exactly as by the value oracle's orbit text."""
    c = limits.case(name)
    limits.assert_witnessed(c, "expand_batch, SYMMETRY")
    cfg = c.with_cfg(symmetry=True)
    # inputs whose successors are grouped (the oracle's orbit text is a brute force over N! images: 64 ms a
    # state at N = 5, 4 ms at N = 4)
    n_in = 2 if c.shape[0] == 5 else 8
    rotation = list(range(1, c.shape[0])) + [0]
    got = rtla.expand_batch(cfg, [list(r) for r in c.rows])
    by = collections.defaultdict(list)
    for k, _, _, im, r in got:
        by[k].append((im, rtla.state_text(cfg, r)))
    for k in range(len(c.rows)):
        assert sorted(by[k]) == list(c.ref[k]), "input state %d" % k
    assert_rows_equal(got, limits.host_expand(name), name + " (symmetry)")
    by_key, by_orbit, grouped = {}, {}, 0
    for k, _, _, im, r in got:
        if k >= n_in or not im:
            continue
        key = rtla.orbit_key(cfg, r)[0]
        assert rtla.orbit_key(cfg, rtla.permute_row(cfg, r, rotation))[0] == key
        orbit = rv.orbit_text(c.vc, c.state_of(k, r))
        by_key.setdefault(key, set()).add(orbit)
        by_orbit.setdefault(orbit, set()).add(key)
        grouped += 1
    assert all(len(v) == 1 for v in by_key.values()) and all(len(v) == 1 for v in by_orbit.values())
    assert grouped >= 60 and len(by_key) == len(by_orbit)


@pytest.mark.parametrize("name", limits.ALL)
def test_audit_matches_host_replay(name):
    """check_batch equals check_replay, all five invariants: on the sample's rows and every successor row
    (succ = 0), and on the sample's rows as parent + delta (succ = 1) -- the 64-slot / 32-election shape
    and the shapes the wave-per-state kernel expands included."""
    c = limits.case(name)
    rows = [list(r) for r in c.rows]
    every = rows + [list(r) for _, _, _, _, r in limits.host_expand(name)]
    want = rtla.check_replay(c.cfg, every, ALL_INV)
    assert rtla.check_batch(c.cfg, every, ALL_INV) == want and all(want[1].values()), want[1]
    want = rtla.check_replay(c.cfg, rows, ALL_INV, succ=True)
    assert rtla.check_batch(c.cfg, rows, ALL_INV, succ=True) == want and all(want[1].values()), want[1]


@pytest.mark.parametrize("name", limits.TWO)
def test_predicates_and_steps_match_host_replay(name):
    """pred_batch equals pred_replay (the restated built-ins and the three field definitions of
    specs/MCPredicates.tla, over the sample's rows and every successor row) and pred_step_batch equals
    pred_step_replay (specs/MCActions.tla: masks, counts, evaluated steps)."""
    c = limits.case(name)
    rows = [list(r) for r in c.rows]
    every = rows + [list(r) for _, _, _, _, r in limits.host_expand(name)]
    with rtla.Predicates(c.cfg, MCPRED) as preds:
        want = rtla.pred_replay(preds, every)
        assert rtla.pred_batch(preds, every) == want
        assert sum(1 for v in want[1].values() if v) >= 5, want[1]
    with rtla.Actions(c.cfg, MCACTIONS) as acts:
        want = rtla.pred_step_replay(acts, rows)
        assert rtla.pred_step_batch(acts, rows) == want
        assert want[2] == c.n_succ and sum(1 for v in want[1].values() if v) >= 3, want


@pytest.mark.parametrize("name", limits.TWO)
def test_dedup_through_the_fingerprint_set(name):
    """Checker.synthetic_step at a limit shape, two batches sharing the set, half of the inputs drawn from
    a pool so that the second batch meets states of the first: generated successors, probes (in-model
    successors that differ from their parent) and new states against the value oracle's counts."""
    c = limits.case(name)
    n, pool = 24, 8
    cfg = c.with_cfg(fpset_log2=20, mem_budget=1 << 30)
    rows = rtla.random_rows(cfg, 0, 2 * n, pool=pool)
    seen, expect = set(), []
    for b in range(2):
        gen = probes = 0
        before = len(seen)
        for r in rows[b * n:(b + 1) * n]:
            text = rtla.state_text(cfg, r)
            for _, t in rv.next_states(c.vc, tla_text.parse_state(c.vc, text)):
                gen += 1
                tt = rv.state_text(c.vc, t)
                if rv.in_model(c.vc, t) and tt != text:
                    probes += 1
                    seen.add(tt)
        expect.append((gen, probes, len(seen) - before))
    with rtla.Checker(cfg) as ck:
        got = [ck.synthetic_step(b * n, n, pool) for b in range(2)]
    assert [(lv.generated, lv.probes, lv.new) for lv in got] == expect
    assert expect[1][2] < expect[1][1] and expect[0][0] > 20 * n, expect  # (the second batch has hits)


@pytest.mark.parametrize("name", limits.BOUNDARY)
def test_full_bag_states_at_the_instance_boundary(name):
    """States with all K bag slots in use at 255 and 256 instances (the compacting kernel: DropMessage of
    slot K - 1 is the id 254 / 255 of its 8-bit ring and new-list entries) and at 258 and 264 (the
    wave-per-state kernel): the value oracle's successors with their labels, and the host model's rows."""
    c = limits.case(name)
    full = limits.full_bag_rows(name)
    got = {}

    def expand(rows):
        got["rows"] = rtla.expand_batch(c.cfg, rows)
        return got["rows"]

    last = assert_full_bag_successors(c, full, expand)
    assert last == {"n4_v4_k64": 255, "n5_k60": 254, "n5_k61": 257, "n5_k63": 263}[name]
    assert_rows_equal(got["rows"], hostmodel.expand(c.cfg, [list(r) for r, _ in full], len(full[0][0])), name)
