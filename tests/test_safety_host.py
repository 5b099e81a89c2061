"""CPU tests of StateMachineSafety and LeaderCompleteness (specs/MC.tla) and of
the host audit (rtla_check_replay).  The two predicates are written here in
Python over value-oracle states, from the TLA+ text alone, and compared bit
for bit with the C++ evaluation: on rows (rtla_invariants, check_replay
succ=0) and on successors evaluated as parent + delta (check_replay succ=1
against the predicates over raft_values.next_states)."""
import pytest

import hostmodel
import limits
import raft_values as rv
import rtla
import tla_text

ALL = tuple(rtla.INV_BITS)  # bit order
SMS, LC = rtla.INV_BITS.get("StateMachineSafety", 0), rtla.INV_BITS.get("LeaderCompleteness", 0)
# (shape, bag_cap, random rows): the synthetic layout, an N = 2 and an N = 5 shape
SHAPES = [((3, 2, 4, 3, 2, 0), 12, 2000), ((2, 2, 3, 2, 1, 0), 20, 500), ((5, 1, 3, 2, 1, 0), 20, 500)]
SUCC_ROWS = 150


def state_machine_safety(cfg, s):
    """\\A i, j : \\A n \\in 1..Min(commitIndex[i], commitIndex[j]) :
         (n <= Len(log[i]) /\\ n <= Len(log[j])) => log[i][n] = log[j][n]"""
    log, ci = s[rv.IX["log"]], s[rv.IX["commitIndex"]]
    for i in range(cfg.n_server):
        for j in range(cfg.n_server):
            for n in range(1, min(ci[i], ci[j]) + 1):
                if n <= len(log[i]) and n <= len(log[j]) and log[i][n - 1] != log[j][n - 1]:
                    return False
    return True


def leader_completeness(cfg, s):
    """\\A i, j : (state[i] = Leader /\\ currentTerm[j] <= currentTerm[i]) =>
         \\A n \\in 1..commitIndex[j] : n <= Len(log[j]) => (n <= Len(log[i]) /\\ log[i][n] = log[j][n])"""
    log, ci = s[rv.IX["log"]], s[rv.IX["commitIndex"]]
    role, term = s[rv.IX["state"]], s[rv.IX["currentTerm"]]
    for i in range(cfg.n_server):
        for j in range(cfg.n_server):
            if role[i] == rv.LEADER and term[j] <= term[i]:
                for n in range(1, ci[j] + 1):
                    if n <= len(log[j]) and not (n <= len(log[i]) and log[i][n - 1] == log[j][n - 1]):
                        return False
    return True


PREDICATES = dict(rv.INVARIANTS, StateMachineSafety=state_machine_safety, LeaderCompleteness=leader_completeness)


def py_mask(vc, s):
    return sum(rtla.INV_BITS[n] for n in ALL if not PREDICATES[n](vc, s))


def setup(shape, bag_cap, n_rows):
    n, v, t, l, c, m = shape
    cfg = rtla.Config(n, v, t, l, c, m, (), bag_cap=bag_cap)
    vc = rv.Cfg(n, v, t, l, c, (), m)
    rows = rtla.random_rows(cfg, 0, n_rows)
    states = [tla_text.parse_state(vc, rtla.state_text(cfg, r)) for r in rows]
    return cfg, vc, rows, states


@pytest.fixture(scope="module", params=SHAPES, ids=lambda p: "n%d" % p[0][0])
def case(request):
    return setup(*request.param)


def test_random_rows_match_the_python_predicates(case):
    cfg, vc, rows, states = case
    full = rtla.Config(*[getattr(cfg, f) for f in ("n_server", "n_value", "max_term", "max_log", "max_copies",
                                                   "max_msgs")], invariants=ALL, bag_cap=cfg.bag_cap)
    want = [py_mask(vc, s) for s in states]
    assert [rtla.invariants_violated(full, r) for r in rows] == want  # every row, none left out
    masks, counts = rtla.check_replay(cfg, rows, ALL)
    assert masks == want
    assert counts == {n: sum(1 for w in want if w & b) for n, b in rtla.INV_BITS.items()}
    for bit in (SMS, LC):  # the generator exercises both verdicts of both new invariants
        hit = sum(1 for w in want if w & bit)
        assert 0.1 * len(rows) <= hit <= 0.9 * len(rows), (bit, hit)
    # a subset of the invariants: the audit's mask is its own, not the configuration's
    sub, _ = rtla.check_replay(full, rows, ("StateMachineSafety", "NoTwoLeaders"))
    assert sub == [w & (SMS | 1) for w in want]


def test_successor_mode_is_the_or_over_materialised_successors(case):
    """parent + delta evaluation == evaluation of the materialised successor,
    the old three invariants included."""
    cfg, vc, rows, states = case
    want, per_bit, evaluated = [], dict.fromkeys(ALL, 0), 0
    for s in states[:SUCC_ROWS]:
        acc = 0
        for _, t in rv.next_states(vc, s):
            m = py_mask(vc, t)
            acc |= m
            evaluated += 1
            for n, b in rtla.INV_BITS.items():
                per_bit[n] += 1 if m & b else 0
        want.append(acc)
    masks, counts = rtla.check_replay(cfg, rows[:SUCC_ROWS], ALL, succ=True)
    assert masks == want and counts == per_bit
    assert evaluated > 10 * SUCC_ROWS and len(set(want)) > 4


def test_threads_agree(case):
    cfg, _, rows, _ = case
    for succ in (False, True):
        sub = rows[:600]
        assert rtla.check_replay(cfg, sub, ALL, succ=succ, threads=1) == rtla.check_replay(cfg, sub, ALL, succ=succ,
                                                                                           threads=0)


# ---- the row format's limits (tests/limits.py)

@pytest.mark.parametrize("name", limits.ALL)
def test_limit_shapes_check_replay(name):
    """check_replay at the widest fields and full capacities, succ 0 and 1, against the Python predicates
    over the value oracle's states and reference successors; every invariant is violated on some row."""
    c = limits.case(name)
    limits.assert_witnessed(c, "check_replay")
    want = [py_mask(c.vc, s) for s in c.states]
    masks, counts = rtla.check_replay(c.cfg, c.rows, ALL)
    assert masks == want
    assert counts == {n: sum(1 for w in want if w & b) for n, b in rtla.INV_BITS.items()}
    assert all(counts.values()), counts
    want, per_bit = [], dict.fromkeys(ALL, 0)
    for nxt in c.succ:
        acc = 0
        for _, t in nxt:
            m = py_mask(c.vc, t)
            acc |= m
            for n, b in rtla.INV_BITS.items():
                per_bit[n] += 1 if m & b else 0
        want.append(acc)
    masks, counts = rtla.check_replay(c.cfg, c.rows, ALL, succ=True)
    assert masks == want and counts == per_bit
    assert all(per_bit.values()), per_bit
    print("%s: violating rows %s, violating successors %s" % (name, dict(counts), per_bit))


# ---- hand cases: rows built by editing packed fields of the Init row (rtla_model.h make_layout / srv_pack)

def bits_for(x):
    return x.bit_length()


class Packer:
    def __init__(self, cfg):
        self.cfg, self.lay = cfg, rtla.row_layout(cfg)
        n, t, l, v = cfg.n_server, cfg.max_term, cfg.max_log, cfg.n_value
        self.b_tcur, self.b_tm1, self.b_vote, self.b_idx = bits_for(t), bits_for(t - 1), bits_for(n), bits_for(l)
        self.b_ent = self.b_tm1 + bits_for(v - 1)
        self.lenbits = bits_for(l + 1)
        self.sb_log = self.b_tcur + 2 + self.b_vote + self.b_idx + 3 * n

    def put(self, row, i, bit, nbits, val):
        base = self.lay["off_srv"] + i * self.lay["srv_words"]
        x = 0
        for w in range(self.lay["srv_words"]):
            x |= row[base + w] << (32 * w)
        x = (x & ~(((1 << nbits) - 1) << bit)) | (val << bit)
        for w in range(self.lay["srv_words"]):
            row[base + w] = (x >> (32 * w)) & 0xFFFFFFFF

    def server(self, row, i, term, role, commit, log):
        """log: [(term, value index)]"""
        self.put(row, i, 0, self.b_tcur, term - 1)
        self.put(row, i, self.b_tcur, 2, role)
        self.put(row, i, self.b_tcur + 2 + self.b_vote, self.b_idx, commit)
        code = len(log)
        for k, (et, ev) in enumerate(log):
            code |= ((et - 1) | ev << self.b_tm1) << (self.lenbits + k * self.b_ent)
        self.put(row, i, self.sb_log, self.lenbits + (self.cfg.max_log + 1) * self.b_ent, code)


FOLLOWER, LEADER = 0, 2


def test_hand_built_rows_isolate_each_invariant():
    cfg = rtla.Config(3, 2, 3, 2, 1, 0, ALL)
    vc = rv.Cfg(3, 2, 3, 2, 1, ALL, 0)
    pk = Packer(cfg)

    def verdict(row):
        s = tla_text.parse_state(vc, rtla.state_text(cfg, row))
        got = rtla.invariants_violated(cfg, row)
        assert got == py_mask(vc, s) == rtla.check_replay(cfg, [row], ALL)[0][0]
        return got, s

    assert verdict(rtla.init_row(cfg))[0] == 0
    # two followers committed index 1 with entries of different terms: only StateMachineSafety fails
    # (LogMatching holds: the terms differ; no leader)
    row = rtla.init_row(cfg)
    pk.server(row, 0, 2, FOLLOWER, 1, [(1, 0)])
    pk.server(row, 1, 2, FOLLOWER, 1, [(2, 0)])
    got, s = verdict(row)
    assert got == SMS
    assert s[rv.IX["commitIndex"]] == (1, 1, 0) and [len(x) for x in s[rv.IX["log"]]] == [1, 1, 0]
    # uncommitted on one side: nothing fails
    pk.server(row, 1, 2, FOLLOWER, 0, [(2, 0)])
    assert verdict(row)[0] == 0
    # a leader with an empty log, a follower of the SAME term with a longer committed log: only
    # LeaderCompleteness fails (StateMachineSafety holds: the leader committed nothing)
    row = rtla.init_row(cfg)
    pk.server(row, 0, 2, LEADER, 0, [])
    pk.server(row, 1, 2, FOLLOWER, 1, [(1, 1)])
    got, s = verdict(row)
    assert got == LC and s[rv.IX["state"]][0] == rv.LEADER and s[rv.IX["currentTerm"]][:2] == (2, 2)
    # the same follower in a term AHEAD of the leader's (the leader is the stale one): the antecedent
    # currentTerm[j] <= currentTerm[i] is false, nothing fails
    pk.server(row, 1, 3, FOLLOWER, 1, [(1, 1)])
    assert verdict(row)[0] == 0
    # ... and in a term behind the leader's it fails again (the formula's <=)
    pk.server(row, 0, 3, LEADER, 0, [])
    pk.server(row, 1, 2, FOLLOWER, 1, [(1, 1)])
    assert verdict(row)[0] == LC
    # the leader holds the entry: holds
    pk.server(row, 0, 3, LEADER, 0, [(1, 1)])
    assert verdict(row)[0] == 0


def test_value_oracle_bfs_finds_no_violation(monkeypatch):
    """n2_v1_t3_l1_m1 under the two new invariants (and the old three): the
    expected "holds" verdict of the GPU runs, from the Python oracle alone."""
    monkeypatch.setitem(rv.INVARIANTS, "StateMachineSafety", state_machine_safety)
    monkeypatch.setitem(rv.INVARIANTS, "LeaderCompleteness", leader_completeness)
    res = rv.bfs(rv.Cfg(2, 1, 3, 1, 1, ("ElectionSafety", "LogMatching", "StateMachineSafety", "LeaderCompleteness"), 1))
    assert res.violation is None and res.distinct == 25164


# ---- the violation key of every pass over rows (rtla_audit.h audit_key), through tests/hostmodel.cpp

IDX39 = (1 << 39) - 1


def _key_fields(key):
    out = (hostmodel.C.c_uint64 * 4)()
    hostmodel.lib().hm_audit_key_fields(key, out)
    return tuple(out)


def test_the_one_violation_key_round_trips_and_orders_by_row_then_instance():
    """index << 25 | instance << 9 | in_model << 8 | mask at the limits of every field (index 2^39 - 1, instance
    65535, mask 255, both in_model values); the accessors invert it; the least key is the least row's, and within
    a row the least instance's, whatever in_model and the mask are."""
    enc = hostmodel.lib().hm_audit_key
    indexes, insts, masks = (0, 1, 12345, IDX39 - 1, IDX39), (0, 1, 63, 64, 65534, 65535), (0, 1, 31, 128, 255)
    for index in indexes:
        for inst in insts:
            for im in (0, 1):
                for mask in masks:
                    key = enc(index, inst, im, mask)
                    assert key == index << 25 | inst << 9 | im << 8 | mask < 1 << 64
                    assert _key_fields(key) == (index, inst, im, mask)
    low = [(im, mask) for im in (0, 1) for mask in masks]
    for index in indexes:
        for a in insts:
            for b in insts:
                for la in low:
                    for lb in low:
                        if a != b:  # (one key per (row, instance): equal instances are the same step)
                            assert (enc(index, a, *la) < enc(index, b, *lb)) == (a < b)
    for index in indexes[:-1]:  # any key of row i is below any key of row i + 1
        assert max(enc(index, 65535, im, mask) for im, mask in low) < min(enc(index + 1, 0, im, mask) for im, mask in low)


def test_bad_arguments():
    cfg = rtla.Config(2, 1, 3, 1, 1, 1, ())
    row = rtla.init_row(cfg)
    for kw in ({"invariants": 32}, {"invariants": -1}, {"succ": 2}, {"threads": -1}):
        args = dict(invariants=31, succ=0, threads=0)
        args.update(kw)
        with pytest.raises(rtla.RtlaError) as e:
            rtla.check_replay(cfg, [row], args["invariants"], succ=args["succ"], threads=args["threads"])
        assert e.value.status == rtla.E_ARG
    cc = cfg.c()
    import ctypes as C
    masks = (C.c_int32 * 1)()
    assert rtla._lib.rtla_check_replay(C.byref(cc), None, 1, 31, 0, 0, masks, None) == rtla.E_ARG
    arr = (C.c_uint32 * len(row))(*row)
    assert rtla._lib.rtla_check_replay(C.byref(cc), arr, 1, 31, 0, 0, None, None) == rtla.E_ARG
    assert rtla._lib.rtla_check_frontier(None, 31, 0, None) == rtla.E_ARG
    assert rtla.check_replay(cfg, [], 31) == ([], dict.fromkeys(ALL, 0))
    with pytest.raises(rtla.RtlaError) as e:
        rtla.check_replay(rtla.Config(n_server=6), [row], 31)
    assert e.value.status == rtla.E_CONFIG
