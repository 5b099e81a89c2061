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
