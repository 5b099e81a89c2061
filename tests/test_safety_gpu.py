"""GPU tests of StateMachineSafety / LeaderCompleteness in the search and of
the audit (rtla_check_batch, Checker.audit: rtla_kaudit.hip).  The reference
is the host replay (rtla.check_replay), which tests/test_safety_host.py pins
to the Python predicates and the value oracle."""
import json
import os
import re
import subprocess
import sys

import pytest

import raft_cpu
import rtla

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "bfs_counts.json")))
ALL = tuple(rtla.INV_BITS)
# the host test's three shapes, an N = 1 and an N = 4 shape (every instantiation), and the widest
# row the wave-per-state kernels serve: 64 bag slots, 32 election records (state tiles of fewer
# than 64 rows; N = 5: more than 64 action instances, several candidate chunks)
SHAPES = [((3, 2, 4, 3, 2, 0), dict(bag_cap=12), 2000),
          ((2, 2, 3, 2, 1, 0), dict(bag_cap=20), 500),
          ((5, 1, 3, 2, 1, 0), dict(bag_cap=20), 500),
          ((1, 2, 3, 2, 1, 0), dict(bag_cap=8), 131),
          ((4, 2, 3, 2, 1, 0), dict(bag_cap=20), 300),
          ((5, 1, 3, 2, 1, 0), dict(bag_cap=64, elec_cap=32), 203)]


@pytest.mark.parametrize("shape,kw,n", SHAPES, ids=lambda p: "-".join(map(str, p)) if isinstance(p, tuple) else None)
def test_batch_equals_replay(shape, kw, n):
    cfg = rtla.Config(*shape, invariants=(), **kw)
    rows = rtla.random_rows(cfg, 0, n)
    if kw.get("elec_cap"):
        assert rtla.row_layout(cfg)["W"] > 96  # state tiles of 16 rows or fewer
    for succ, sub in ((False, rows), (True, rows[:300])):
        want = rtla.check_replay(cfg, sub, ALL, succ=succ)
        got = rtla.check_batch(cfg, sub, ALL, succ=succ)
        assert got == want, succ
        assert shape[0] == 1 or (len(set(want[0])) > 2 and all(want[1].values()))  # (one server: nothing to violate)
    # a mask of its own, independent of the configuration's
    both = ("StateMachineSafety", "LeaderCompleteness")
    assert rtla.check_batch(cfg, rows, both) == rtla.check_replay(cfg, rows, both)
    assert rtla.check_batch(cfg, [], ALL) == ([], dict.fromkeys(ALL, 0))


BFS_CODE = ("import json, rtla, sys; g = json.load(open(sys.argv[1]))[sys.argv[2]];"
            "r = rtla.check(rtla.Config(g['n_server'], g['n_value'], g['max_term'], g['max_log'], g['max_copies'],"
            " g['max_msgs'], tuple(rtla.INV_BITS), fpset_log2=20, mem_budget=1 << 29), trace=False);"
            "print(json.dumps([[[lv.new, lv.generated] for lv in r.levels], r.distinct, r.generated, r.violation]))")


@pytest.mark.parametrize("name", ["n2_v1_t3_l1_m1", "n2_v2_t3_l2_m1"])
def test_bfs_with_all_five_invariants(name):
    """No false positive in the in-kernel path: the counts are the golden ones
    (which no invariant influences unless one is violated), nothing violates,
    and the default level kernel and the wave-per-state kernel (RTLA_XFLAGS =
    2048, read once: a child process) agree."""
    g = GOLD[name]
    gold = os.path.join(os.path.dirname(__file__), "golden", "bfs_counts.json")
    outs = []
    for xflags in ("0", "2048"):
        env = dict(os.environ, RTLA_XFLAGS=xflags,
                   PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "raft-tla_amd"), os.environ.get("PYTHONPATH", "")]))
        out = subprocess.run([sys.executable, "-c", BFS_CODE, gold, name], env=env, capture_output=True, text=True,
                             timeout=100)
        assert out.returncode == 0, out.stdout + out.stderr
        outs.append(json.loads(out.stdout.strip().splitlines()[-1]))
    assert outs[0] == outs[1] == [g["levels"], g["distinct"], g["generated"], None]


NTL = dict(fpset_log2=22, mem_budget=1 << 30)


def two_leaders(cfg, flat):
    """Indexes of the rows of a flat frontier whose text names two leaders."""
    import ctypes as C
    cc, w = cfg.c(), rtla.row_words(cfg)
    buf = C.create_string_buffer(1 << 14)
    out = []
    for k in range(len(flat) // w):
        row = C.cast(C.addressof(flat) + 4 * k * w, C.POINTER(C.c_uint32))
        assert rtla._lib.rtla_state_text(C.byref(cc), row, buf, len(buf)) > 0
        if buf.value.count(b'"Leader"') >= 2:
            out.append(k)
    return out


def row_at(cfg, flat, k):
    w = rtla.row_words(cfg)
    return list(flat[k * w:(k + 1) * w])


def test_audit_finds_a_violation_the_search_did_not_look_for():
    cfg = rtla.Config(3, 1, 3, 1, 1, 1, ("ElectionSafety",), **NTL)
    with rtla.Checker(cfg) as ck, rtla.Checker(cfg) as plain:
        ck.init()
        plain.init()
        for _ in range(17):
            assert ck.step() == rtla.OK and plain.step() == rtla.OK
        assert len(ck.levels) == 18
        res = ck.audit(("NoTwoLeaders",))
        assert res.status == rtla.OK and res.audited == res.evaluated == ck.levels[-1].new
        assert set(res.counts.values()) == {0} and res.violation is None and ck.violation() == (None, False)
        assert ck.step() == rtla.OK and plain.step() == rtla.OK
        front = ck.frontier_flat()
        bad = two_leaders(cfg, front)
        assert bad, "level 19 holds a state with two leaders (golden n3_v1_t3_l1_m1_ntl)"
        # several, found by different blocks (four waves of 64 rows each): the least of them is the one reported
        assert len({k // 256 for k in bad}) > 1 and bad[0] // 256 < bad[-1] // 256
        res = ck.audit(("NoTwoLeaders",))
        assert res.status == rtla.VIOLATION and res.violation == ["NoTwoLeaders"]
        assert res.counts["NoTwoLeaders"] == len(bad) and res.audited == ck.frontier_size()
        assert (res.viol_index, res.viol_inst, res.viol_mask, res.viol_in_model) == (bad[0], -1, 1, True)
        assert ck.violation() == ("NoTwoLeaders", True)
        tr = ck.trace()
        assert len(tr) == 19 and tr[0][0] == "Initial predicate"
        assert tr[-1][1] == rtla.state_text(cfg, row_at(cfg, front, bad[0]))
        walk = raft_cpu.Walk(raft_cpu.cfg_of(3, 1, 3, 1, 1, 1, ("NoTwoLeaders",)))
        assert walk.text() == tr[0][1]
        for label, text in tr[1:]:
            assert text in [t for _, t in walk.successors()], label
            walk.goto(text)
        assert walk.invariants() & 1
        # the search goes on as the run without the audit does
        assert ck.step() == plain.step() == rtla.OK
        assert ck.violation() == (None, False)
        a, b = ck.levels[-1], plain.levels[-1]
        assert (a.level, a.new, a.generated) == (b.level, b.new, b.generated) == (20, b.new, b.generated)
        assert (ck.distinct, ck.generated) == (plain.distinct, plain.generated)


def test_successor_audit_reports_the_violating_successor():
    cfg = rtla.Config(3, 1, 3, 1, 1, 1, ("ElectionSafety",), **NTL)
    with rtla.Checker(cfg) as ck:
        ck.init()
        for _ in range(17):
            ck.step()
        front = ck.frontier_flat()
        masks, counts = rtla.check_replay(cfg, front, ("NoTwoLeaders",), succ=True)
        first = next(k for k, m in enumerate(masks) if m)
        # several rows with a violating successor, found by different blocks (four states each): the least is reported
        assert len({k // 4 for k, m in enumerate(masks) if m}) > 1
        res = ck.audit(("NoTwoLeaders",), succ=True)
        assert res.status == rtla.VIOLATION and res.violation == ["NoTwoLeaders"]
        assert res.counts == counts and res.viol_index == first and res.audited == len(masks) < res.evaluated
        parent = row_at(cfg, front, first)
        succ = rtla.expand_batch(cfg, [parent])
        viol = [x for x in succ if rtla.invariants_violated(rtla.Config(3, 1, 3, 1, 1, 1, ("NoTwoLeaders",)), x[4])]
        assert (res.viol_inst, res.viol_in_model) == (viol[0][1], viol[0][3])
        tr = ck.trace()
        assert len(tr) == 19 and tr[17][1] == rtla.state_text(cfg, parent)
        assert tr[18][1] == rtla.state_text(cfg, viol[0][4]) and tr[18][1].count('"Leader"') >= 2
        assert ck.step() == rtla.OK and ck.violation() == (None, False)


def test_audit_with_the_new_invariants_on_the_flagship_shape():
    """Level 12 of the configs[1] shape (1,703,901 states): both new invariants
    hold, and the device counts are the host replay's over the same rows."""
    cfg = rtla.Config(3, 2, 3, 2, 1, 0, ("ElectionSafety", "LogMatching"), bag_cap=18, elec_cap=6, fpset_log2=26,
                      mem_budget=3 << 30)
    new = ("StateMachineSafety", "LeaderCompleteness")
    with rtla.Checker(cfg) as ck:
        ck.init()
        for _ in range(11):
            assert ck.step() == rtla.OK
        assert len(ck.levels) == 12
        for succ in (False, True):
            res = ck.audit(new, succ=succ)
            assert res.status == rtla.OK and res.audited == ck.levels[-1].new == ck.frontier_size()
            assert set(res.counts.values()) == {0}
            print("audit succ=%d: %d states, %d evaluated, %.3f ms" % (succ, res.audited, res.evaluated, res.kernel_ms))
        flat = ck.frontier_flat()
        masks, counts = rtla.check_replay(cfg, flat, new)
        assert counts == ck.audit(new).counts and not any(masks)
        every = ck.audit(ALL)
        assert every.counts == rtla.check_replay(cfg, flat, ALL)[1]


def test_preconditions():
    small = dict(fpset_log2=16, mem_budget=1 << 28)
    for kw, init in ((dict(shards=2), True), (dict(dedup_only=True), False), ({}, False)):
        with rtla.Checker(rtla.Config(2, 1, 2, 1, 1, 1, (), **kw, **small)) as ck:
            if init:
                ck.init()
            with pytest.raises(rtla.RtlaError) as e:
                ck.audit(ALL)
            assert e.value.status == rtla.E_STATE
    with rtla.Checker(rtla.Config(2, 1, 2, 1, 1, 1, (), **small)) as ck:
        ck.init()
        assert ck.audit(ALL).status == rtla.OK and ck.audit(ALL, succ=True).evaluated > 1
        with pytest.raises(rtla.RtlaError) as e:
            ck.audit(32)
        assert e.value.status == rtla.E_ARG


def test_cli_audit_reports_counts_and_the_trace():
    from cli_util import run
    cfgp = os.path.join(ROOT, "specs", "raft3_v1_t3_l1_m1_es.cfg")
    base = ["-skip-spec-check", "-fpbits", "22", "-membudget", str(1 << 30), "-config", cfgp,
            os.path.join(ROOT, "specs", "MC.tla")]
    r = run(["-audit", "NoTwoLeaders,StateMachineSafety", "-bfs-levels", "19"] + base)
    assert r.returncode == 12, r.stdout + r.stderr
    assert re.search(r"^Error: Invariant NoTwoLeaders is violated by \d+ of the \d+ states\.$", r.stdout, re.M)
    assert re.search(r"^Invariant StateMachineSafety holds in all \d+ states\.$", r.stdout, re.M)
    assert "Error: Invariant NoTwoLeaders is violated.\n" in r.stdout
    states = re.findall(r"^State (\d+): <(.*)>$", r.stdout, re.M)
    assert len(states) == 19 and states[0] == ("1", "Initial predicate")
    r = run(["-audit", "NoTwoLeaders,LeaderCompleteness", "-bfs-levels", "18"] + base)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Invariant NoTwoLeaders holds in all" in r.stdout and "Audit completed. No error has been found" in r.stdout
