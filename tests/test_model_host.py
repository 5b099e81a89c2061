"""CPU checks of the model code the level kernel evaluates (rtla_model.h,
compiled for the host by tests/hostmodel.py -- test infrastructure): the
successor multisets of lockstep random walks equal the C oracle's, the
successors of random synthetic states equal the value oracle's, and every
incrementally derived fingerprint equals a from-scratch hash.  The same
checks run on the GPU through the hot kernel (tests/test_gpu.py)."""
import collections
import random

import pytest

import hostmodel
import limits
import raft_cpu
import raft_values as rv
import rtla
import tla_text

INV = ("NoTwoLeaders", "ElectionSafety", "LogMatching")
WALKS = [(2, 2, 3, 2, 1, 1), (3, 1, 2, 1, 1, 2), (3, 2, 3, 2, 1, 3), (3, 2, 4, 3, 2, 4),
         (5, 1, 3, 2, 1, 3), (2, 1, 3, 1, 2, 0), (4, 2, 3, 2, 1, 0)]


@pytest.mark.parametrize("shape", WALKS)
def test_host_model_walk_matches_oracle(shape):
    n, v, t, l, c, m = shape
    cfg = rtla.Config(n, v, t, l, c, m, INV, bag_cap=16 if m == 0 else 0)
    w = rtla.row_words(cfg)
    walk = raft_cpu.Walk(raft_cpu.cfg_of(n, v, t, l, c, m, INV))
    rnd = random.Random(hash(shape) & 0xFFFF)
    row = rtla.init_row(cfg)
    for step in range(150):
        succ = hostmodel.expand(cfg, [row], w)
        mine = sorted((im, rtla.state_text(cfg, r)) for _, _, _, im, r in succ)
        assert mine == sorted(walk.successors()), "successor multiset differs at step %d" % step
        for _, _, _, _, r in succ:
            assert rtla.stored_fingerprint(r) == rtla.row_fingerprint(cfg, r)
        inm = [x for x in succ if x[3]]
        if not inm:
            break
        row = rnd.choice(inm)[4]
        walk.goto(rtla.state_text(cfg, row))


def test_host_model_synthetic_states_match_value_oracle():
    cfg = rtla.Config(3, 2, 4, 3, 2, 0, ("ElectionSafety", "LogMatching"), bag_cap=12)
    vc = rv.Cfg(3, 2, 4, 3, 2, ("ElectionSafety", "LogMatching"), 0)
    w = rtla.row_words(cfg)
    rows = rtla.random_rows(cfg, 0, 120, pool=30)
    by = collections.defaultdict(list)
    for k, inst, sub, im, r in hostmodel.expand(cfg, rows, w):
        by[k].append((im, rtla.state_text(cfg, r)))
        assert rtla.stored_fingerprint(r) == rtla.row_fingerprint(cfg, r)
    for k, r in enumerate(rows):
        s = tla_text.parse_state(vc, rtla.state_text(cfg, r))
        ref = sorted((rv.in_model(vc, t), rv.state_text(vc, t)) for _, t in rv.next_states(vc, s))
        assert sorted(by[k]) == ref, "input state %d" % k


# ---- the row format's limits (tests/limits.py): widest fields, full capacities, the 256-instance boundary

@pytest.mark.parametrize("name", limits.ALL)
def test_limit_shapes_expand_as_the_value_oracle(name):
    """hostmodel.expand over a limit shape's sample equals raft_values.next_states state by state (texts and
    in-model flags), every stored fingerprint equals a from-scratch hash, and the sample shows every witness
    of tests/limits.py -- counted on the value oracle's states, printed here."""
    c = limits.case(name)
    limits.assert_witnessed(c, "host model")
    assert limits.kernel_of(c.cfg)[0] == c.kernel  # the table's kernel column, by the launch rule
    by = collections.defaultdict(list)
    for k, _, _, im, r in limits.host_expand(name):
        by[k].append((im, rtla.state_text(c.cfg, r)))
        assert rtla.stored_fingerprint(r) == rtla.row_fingerprint(c.cfg, r)
    for k in range(len(c.rows)):
        assert sorted(by[k]) == list(c.ref[k]), "input state %d" % k
    assert sum(len(v) for v in by.values()) == c.n_succ > 20 * len(c.rows)


@pytest.mark.parametrize("name", limits.ALL)
def test_limit_shapes_text_round_trip(name):
    """rtla.state_text -> tla_text.parse_state -> raft_values.state_text is the identity: values up to v4,
    terms up to 7, counts up to 15, logs of 5 entries.  On every input row, and on successor rows that print
    each extreme plus an even spread in and out of the model (the parser takes ~5 ms a state; the text of
    EVERY successor row is compared with the value oracle's print of its own successor by
    test_limit_shapes_expand_as_the_value_oracle, and here the parse must give that very state)."""
    c = limits.case(name)
    limits.assert_witnessed(c, "text round trip")
    n, v, t, l, cc, _ = c.shape
    succ = [(k, r, rtla.state_text(c.cfg, r), im) for k, _, _, im, r in limits.host_expand(name)]
    extremes = {
        "log entry (T, V)": lambda ln: ln.startswith("/\\ log = ") and "[term |-> %d, value |-> v%d]" % (t, v) in ln,
        "count C+1": lambda ln: ln.startswith("/\\ messages = ") and "] :> %d" % (cc + 1) in ln,
        "currentTerm T+1": lambda ln: ln.startswith("/\\ currentTerm = ") and ":> %d" % (t + 1) in ln,
        "own log of L+1": lambda ln: ln.startswith("/\\ log = ") and any(
            x.count("[term") == l + 1 for x in ln.split("<<")),
    }
    picked = {}
    for what, fn in extremes.items():
        hits = [x for x in succ if any(fn(ln) for ln in x[2].split("\n"))]
        assert hits, what
        picked[what] = len(hits)
        for x in hits[:10]:
            picked.setdefault("rows", []).append(x)
    sample = picked.pop("rows") + limits.spread([x for x in succ if not x[3]], 100) + \
        limits.spread([x for x in succ if x[3]], 150)
    print("%s: successor texts printing each extreme: %s; %d successors parsed back" % (name, picked, len(sample)))
    for r, s in zip(c.rows, c.states):
        assert rv.state_text(c.vc, s) == rtla.state_text(c.cfg, r)
    for k, r, text, _ in sample:
        s = tla_text.parse_state(c.vc, text)
        assert s == c.by_text[k][text] and rv.state_text(c.vc, s) == text


def assert_full_bag_successors(c, rows_states, expand):
    """expand(rows) -- hostmodel.expand or rtla.expand_batch -- over full-bag states (limits.full_bag_rows):
    per state the value oracle's successors (texts, in-model flags), among them DuplicateMessage and
    DropMessage of every slot, that of slot K - 1 under the layout's highest instance id."""
    cfg, vc = c.cfg, c.vc
    ninst = limits.n_instances(cfg)
    assert rows_states, "no full-bag state in the sample"
    got = collections.defaultdict(list)
    for k, inst, sub, im, r in expand([list(r) for r, _ in rows_states]):
        got[k].append((inst, sub, im, rtla.state_text(cfg, r)))
    for k, (_, s) in enumerate(rows_states):
        ref = rv.next_states(vc, s)
        assert sorted((im, t) for _, _, im, t in got[k]) == sorted((rv.in_model(vc, u), rv.state_text(vc, u))
                                                                   for _, u in ref), "full-bag state %d" % k
        for label, first in (("DuplicateMessage", ninst - 2 * c.K), ("DropMessage", ninst - c.K)):
            mine = [(inst, t) for inst, sub, _, t in got[k] if rtla.action_name(cfg, inst, sub) == label]
            assert [inst for inst, _ in mine] == list(range(first, first + c.K)), label
            assert sorted(t for _, t in mine) == sorted(rv.state_text(vc, u) for lab, u in ref if lab == label)
        assert got[k][-1][0] == ninst - 1  # (sorted by instance: the last successor is DropMessage of slot K - 1)
    return ninst - 1


@pytest.mark.parametrize("name", limits.BOUNDARY)
def test_full_bag_drop_of_the_last_slot_is_the_highest_instance(name):
    """At the 256-instance boundary (255, 256, 258 and 264 instances): the host model on states whose bag
    holds K messages."""
    c = limits.case(name)
    last = assert_full_bag_successors(c, limits.full_bag_rows(name),
                                      lambda rows: hostmodel.expand(c.cfg, rows, len(rows[0])))
    print("%s: %d full-bag states, highest instance id %d" % (name, len(limits.full_bag_rows(name)), last))
    assert last == {"n4_v4_k64": 255, "n5_k60": 254, "n5_k61": 257, "n5_k63": 263}[name]


# ---- the three 64-bit records (rtla_device.h), through tests/hostmodel.cpp

R_NONE = 6  # rtla_model.h: the receive-sub of a successor that is no Receive
IDX40 = (1 << 40) - 1
PARENTS = [(0, 0, 0), (7, IDX40, 255), (7, 0, 0), (0, IDX40, 0), (0, 0, 255), (3, 0x123456789A, 44), (1, 1 << 39, 1)]
SUCCESSORS = [(0, 0, 0, 0), ((1 << 32) - 1, 1, R_NONE, 255), (5, 1, 0, 7), (5, 0, R_NONE, 7), (63, 0, 0, 255),
              (1 << 31, 1, 3, 200), (2, 0, 5, 0)]
REFS = [(0, 0), (IDX40, 255), (1, 0), (0, 255), (0x123456789A, 44)]


def _fields(kind, r):
    out = (hostmodel.C.c_uint64 * 4)()
    hostmodel.lib().hm_record_fields(kind, r, out)
    return tuple(out[:3])


class _FakeLib:
    """A C library whose expand call returns the given successor records (no rows)."""

    def __init__(self, real, records):
        self.real, self.records = real, records

    def __getattr__(self, name):
        return getattr(self.real, name)

    def _fill(self, info):
        for k, r in enumerate(self.records):
            info[k] = r
        return len(self.records)

    def hm_expand(self, *a):
        return self._fill(a[-2])

    def rtla_expand_batch(self, cc, flat, n, succ, info, cap, nout):
        nout._obj.value = self._fill(info)
        return 0


def test_record_formats_match_the_documented_layouts(monkeypatch):
    """parent_record / successor_info / outbox_ref equal the literal formulas
    (include/rtla.h: input index << 32 | in_model << 31 | receive-sub << 16 |
    instance; rtla_host.cpp: parent shard in bits 56-63, index in 16-55,
    instance in 0-15; ShardBox::send_ref: parent << 16 | instance) at the
    extremes of every field, and the accessors invert them; hostmodel.expand
    and rtla.expand_batch take successor records apart into the same fields."""
    enc = hostmodel.lib().hm_record
    for shard, index, inst in PARENTS:
        r = enc(0, shard, index, inst, 0)
        assert r == shard << 56 | index << 16 | inst
        assert _fields(0, r) == (shard, index, inst)
    for inp, im, sub, inst in SUCCESSORS:
        r = enc(1, inp, im, sub, inst)
        assert r == inp << 32 | im << 31 | sub << 16 | inst
        assert _fields(1, r) == (inp, r & 0x7FFFFFFF, inst)  # the label rtla_trace returns: the low 31 bits
    for parent, inst in REFS:
        r = enc(2, parent, inst, 0, 0)
        assert r == parent << 16 | inst
        assert _fields(2, r)[:2] == (parent, inst)
    # the Python decoders, fed the encoded records through a stub of the C call
    cfg = rtla.Config(2, 1, 2, 1, 1, 1, INV)
    w = rtla.row_words(cfg)
    records = [hostmodel.lib().hm_record(1, *s) for s in SUCCESSORS]
    want = [(inp, inst, sub, bool(im)) for inp, im, sub, inst in SUCCESSORS]
    real = hostmodel.lib()
    monkeypatch.setattr(hostmodel, "lib", lambda: _FakeLib(real, records))
    monkeypatch.setattr(rtla, "_lib", _FakeLib(rtla._lib, records))
    rows = [[0] * w]
    assert [t[:4] for t in hostmodel.expand(cfg, rows, w)] == want
    assert [t[:4] for t in rtla.expand_batch(cfg, rows)] == want
