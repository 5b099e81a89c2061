"""The level kernel's row build (build_all, rtla_klevel.h), word for word.

Every word of a child row is stored once, by the child's own lane: the words
in which it differs from its parent as child_write (rtla_model.h) defines
them, the others read from the parent row (child_word / child_store).  A
word taken from the wrong side -- a patch missed, a parent word where the
child differs -- shows here as a differing word of a named row; the level
digests of test_gpu.py would only say that a level differs.

Each BFS step's new frontier (Checker.frontier_flat) is compared, row by
row, with the in-model, not-yet-seen successors the host model
(tests/hostmodel.cpp: compute_delta + materialize of rtla_model.h) derives
from the previous level's rows -- for every instantiation of the kernel, at
the boundaries of a 64-child batch, across the ring arena's wrap and up to a
partial slot reservation.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import hostmodel
import rtla

pytestmark = pytest.mark.gpu

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "bfs_counts.json")))
MAX_ROWS = 50_000   # levels are followed while the frontier stays under this many rows
NEWCAP = 512        # rtla_klevel.h: the per-wave list of pending new states ...
NEWFLUSH = NEWCAP - 3 * 64  # ... built into rows mid-group once it holds more than this many
# Without a mid-group flush a group ends with at most NEWFLUSH pending states plus what its last two chunks'
# probes add while they drain (<= 2 x 64): a group with more new states than this must have flushed.
NO_FLUSH_MAX = NEWFLUSH + 2 * 64
_U32P = C.POINTER(C.c_uint32)
_U64P = C.POINTER(C.c_uint64)


def _ninst(cfg):
    n, v, k = cfg.n_server, cfg.n_value, hostmodel._params(cfg)[6]
    return 4 * n + 2 * n * n + n * v + 3 * k


def host_successors(cfg, rows):
    """hm_expand over a (n, W) u32 array: (parent index, in_model) per enabled successor and the
    successor rows, in (parent, instance) order."""
    n, w = rows.shape
    per, chunk = _ninst(cfg), 2048
    out = np.empty((chunk * per, w), np.uint32)
    info = np.empty(chunk * per, np.uint64)
    par, inm, succ = [], [], []
    for k in range(0, n, chunk):
        part = np.ascontiguousarray(rows[k:k + chunk])
        got = hostmodel.lib().hm_expand(*hostmodel._params(cfg), part.ctypes.data_as(_U32P), len(part),
                                        out.ctypes.data_as(_U32P), info.ctypes.data_as(_U64P), len(info))
        assert got >= 0, "hm_expand: %d" % got
        par.append((info[:got] >> np.uint64(32)).astype(np.int64) + k)
        inm.append((info[:got] >> np.uint64(31) & np.uint64(1)).astype(bool))
        succ.append(out[:got].copy())
    return np.concatenate(par), np.concatenate(inm), np.concatenate(succ)


def row_keys(rows):
    """One u64 per row from its stored 128-bit fingerprint (words 0-3): the sort and lookup key.  Rows
    are always compared in full."""
    r = rows.astype(np.uint64)
    a = r[:, 0] | r[:, 1] << np.uint64(32)
    b = r[:, 2] | r[:, 3] << np.uint64(32)
    return a ^ (b * np.uint64(0x9E3779B97F4A7C15))


def assert_rows_generated(got, host, hkeys, what):
    """Every row of got (the GPU's, any order) is, word for word, one of the rows `host` (sorted by their
    keys hkeys) -- and got holds each of host's states exactly once.  A row is not canonical for its state
    (the bag's slot order depends on the path), so a state may have several rows in host: the GPU keeps
    the one generated first."""
    gkeys = row_keys(got)
    ukeys = np.unique(hkeys)
    assert len(got) == len(ukeys), "%s: %d rows, the host model derives %d states" % (what, len(got), len(ukeys))
    assert np.array_equal(np.sort(gkeys), ukeys), "%s: other states (fingerprints) than the host model's" % what
    lo, hi = np.searchsorted(hkeys, gkeys, "left"), np.searchsorted(hkeys, gkeys, "right")
    found = np.zeros(len(got), bool)
    for j in range(int((hi - lo).max(initial=0))):
        at = np.minimum(lo + j, len(host) - 1)
        found |= (lo + j < hi) & (host[at] == got).all(axis=1)
    if not found.all():
        k = int(np.flatnonzero(~found)[0])
        diff = np.flatnonzero(host[lo[k]] != got[k])
        w = int(diff[0])
        raise AssertionError("%s: row %d differs from every generation of its state; from the first in words %s: "
                             "word %d is %#x, the host model has %#x (%d rows differ)" %
                             (what, k, diff.tolist(), w, got[k, w], host[lo[k], w], int((~found).sum())))


def expected_level(cfg, prev, seen):
    """The next level as the host model derives it from the rows `prev`: every generation of an in-model
    successor that is in no earlier level (`seen`: sorted keys) -- rows sorted by key, their keys, and
    the index in prev of each one's parent."""
    par, inm, succ = host_successors(cfg, prev)
    par, succ = par[inm], succ[inm]
    key = row_keys(succ)
    pos = np.minimum(np.searchsorted(seen, key), len(seen) - 1)
    new = seen[pos] != key
    order = np.argsort(key[new], kind="stable")
    return succ[new][order], key[new][order], par[new][order]


def frontier(ck, cfg):
    w = rtla.row_words(cfg)
    return np.frombuffer(ck.frontier_flat(), np.uint32).reshape(-1, w).copy()


def follow(cfg, sizes, max_rows=MAX_ROWS, what="", on_level=None):
    """Run the BFS while the frontier stays under max_rows, each new level row-exact against the host
    model; the levels' sizes are appended to `sizes` as they pass.  on_level(level number, the new rows
    in the GPU's order, key and parent index -- in the expanded level's GPU order -- of every generation
    of a new state) is called per level."""
    with rtla.Checker(cfg) as ck:
        st = ck.init()
        prev = frontier(ck, cfg)
        assert len(prev) == 1
        seen = np.sort(row_keys(prev))
        sizes.append(1)
        while st == rtla.OK:
            host, hkeys, par = expected_level(cfg, prev, seen)
            ukeys = np.unique(hkeys)
            if len(ukeys) >= max_rows:
                break
            st = ck.step()
            got = frontier(ck, cfg)
            assert_rows_generated(got, host, hkeys, "%s level %d" % (what, len(sizes) + 1))
            if on_level:
                on_level(len(sizes) + 1, got, hkeys, par)
            sizes.append(len(got))
            if not len(got):
                break
            seen = np.sort(np.concatenate((seen, ukeys)))
            prev = got
    return sizes


KW = dict(fpset_log2=22, mem_budget=1 << 30)
ES_LM = ("ElectionSafety", "LogMatching")
# the kernel instantiations (rtla_kdev.h specs): shape, invariants, bag slots
SHAPES = {
    "cfg2": ((3, 2, 3, 2, 1, 0), ES_LM, 18),              # specs::CFG2: 43-word rows, 64-row groups
    "cfg1": ((3, 1, 2, 1, 1, 0), ("NoTwoLeaders",), 24),  # specs::CFG1
    "cfg3": ((3, 2, 4, 3, 2, 0), (), 20),                 # specs::CFG3: max copies 2, 32-row groups
    "exhaust": ((3, 2, 2, 2, 1, 2), ES_LM, 0),            # specs::EXHAUST: narrow rows, 4 waves/SIMD
    "runtime": ((2, 2, 3, 2, 1, 1), ES_LM, 0),            # n2_v2_t3_l2_m1: the run-time layout
}


def shape_cfg(name, **kw):
    shape, inv, bag = SHAPES[name]
    return rtla.Config(*shape, inv, bag_cap=bag, **dict(KW, **kw))


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_rows_are_the_host_models_word_for_word(name):
    """1. Row-exact build, per instantiation; and 2.: each run has a level of fewer than 64 new states
    (one partial batch) and a level whose new states are no multiple of 64 -- then some group's are not."""
    sizes = follow(shape_cfg(name), [], what=name)
    assert len(sizes) >= 8 and max(sizes) > 64 * 64, sizes  # several groups, several batches per group
    assert any(0 < n < 64 for n in sizes[1:])
    assert any(n > 64 and n % 64 for n in sizes[1:])


def test_symmetry_rows_are_generated_states_word_for_word():
    """1. under SYMMETRY (build_one): a level keeps one state per new orbit, whichever of its members was
    generated first -- every stored row is, word for word, a successor the host model derives from a row
    of the previous level, rows are distinct, and each level has the oracle's size."""
    g = GOLD["n3_v1_t2_l1_m1_sym"]
    cfg = rtla.Config(g["n_server"], g["n_value"], g["max_term"], g["max_log"], g["max_copies"], g["max_msgs"],
                      tuple(g["invariants"]), symmetry=True, **KW)
    last = 22
    with rtla.Checker(cfg) as ck:
        st = ck.init()
        prev = frontier(ck, cfg)
        level = 1
        while st == rtla.OK and level < last:
            _, inm, succ = host_successors(cfg, prev)
            hkeys = row_keys(succ[inm])
            order = np.argsort(hkeys, kind="stable")
            host, hkeys = succ[inm][order], hkeys[order]
            st = ck.step()
            level += 1
            got = frontier(ck, cfg)
            assert len(got) == g["levels"][level - 1][0] < MAX_ROWS
            gkeys = row_keys(got)
            assert len(np.unique(gkeys)) == len(got), "level %d: a state stored twice" % level
            lo, hi = np.searchsorted(hkeys, gkeys, "left"), np.searchsorted(hkeys, gkeys, "right")
            found = np.zeros(len(got), bool)
            for j in range(int((hi - lo).max(initial=0))):
                found |= (lo + j < hi) & (host[np.minimum(lo + j, len(host) - 1)] == got).all(axis=1)
            if not found.all():
                k = int(np.flatnonzero(~found)[0])
                diff = np.flatnonzero(host[min(lo[k], len(host) - 1)] != got[k]).tolist() if lo[k] < hi[k] else "all"
                raise AssertionError("level %d: row %d is no generated successor (words %s)" % (level, k, diff))
            prev = got
    assert level == last and len(prev) > 64 * 64


def _generating_groups(pkeys, par, group=64):
    """Per new state (key): the least and the greatest group of the expanded level, in the GPU's own row
    order, among the parents that generate it."""
    grp = par // group
    order = np.lexsort((grp, pkeys))
    k, gs = pkeys[order], grp[order]
    start = np.flatnonzero(np.concatenate(([True], k[1:] != k[:-1])))
    return k[start], np.minimum.reduceat(gs, start), np.maximum.reduceat(gs, start)


@pytest.mark.parametrize("name,level", [("exhaust", 5), ("runtime", 7), ("cfg2", 4)])
def test_group_flushes_mid_group(name, level):
    """2. A group with more than NO_FLUSH_MAX pending states has built rows mid-group.  No BFS level under
    MAX_ROWS rows is known to have one: over the five shapes above the host model (levels in its own
    breadth-first order) counts at most 242 new
    states that one group of parents alone generates (cfg2, level 5; what a group must find) and at most
    652 that it generates at all (cfg2, level 8; what it may find, when it wins every state it shares
    with other groups) -- a flush may happen there, none has to.  So the level's rows go through the
    successor listing (expand_batch: the level kernel with every enabled successor taken as new, built by
    the same build_all): the host model's per-parent successor counts put every full group of 64 parents
    above the bound, and every row is compared in place."""
    cfg = shape_cfg(name)
    assert not int(os.environ.get("RTLA_XFLAGS", "0")) & 2048  # (the switch to the wave-per-state kernel)
    with rtla.Checker(shape_cfg(name, shards=2)) as ck:
        # a sharded driver sizes its overflow list for k_expand_compact's groups, 0 when the wave-per-state
        # kernel runs this layout: the rule by which expand_batch picks the level kernel too
        assert json.loads(ck.device_info())["overflow_records"] > 0
    with rtla.Checker(cfg) as ck:
        ck.init()
        for _ in range(level - 1):
            ck.step()
        rows = ck.frontier()
    want = hostmodel.expand(cfg, rows, rtla.row_words(cfg))
    per_group = np.bincount(np.array([k for k, _, _, _, _ in want]) // 64)
    assert len(rows) > 64 and per_group[:-1].min() > NO_FLUSH_MAX and per_group[-1] % 64, per_group
    got = [tuple(t) for t in rtla.expand_batch(cfg, rows)]
    assert len(got) == len(want)
    for g, h in zip(got, want):
        assert g[:4] == h[:4], (g[:4], h[:4])
        diff = [w for w in range(len(h[4])) if g[4][w] != h[4][w]]
        assert not diff, "successor %s of input %d differs in words %s" % (g[1], g[0], diff)


def _round64(n):
    return (n + 63) // 64 * 64


def test_ring_wrap_inside_a_batch():
    """3. The arena barely holds the largest (current + next) pair of levels, so the levels walk around
    it (a level starts where the one before ends, rounded up to a group) and most levels cross its end.
    Level starts are multiples of 64 rows, but a wave's batches count from its own slot reservation:
    where the rows on both sides of the arena's end come from the same group's parents alone, the run of
    that group's rows up to the end is one reservation, and its length tells where in a batch the end
    falls -- at least once not at a multiple of 64."""
    g = GOLD["n2_v2_t3_l2_m1"]
    x = [n for n, _ in g["levels"]]
    cap = _round64(max(_round64(x[i]) + x[i + 1] for i in range(len(x) - 1)))
    starts = [0]
    for n in x[:-1]:
        starts.append((starts[-1] + _round64(n)) % cap)
    # the levels that cross the arena's end, and after how many of their rows (a consequence of the level
    # sizes alone: 21760 rows of arena; level 20 crosses after 704 of its 4558 rows, level 26 after 4416 of 9672)
    crossing = {k + 1: cap - starts[k] for k in range(len(x)) if 0 < cap - starts[k] < x[k]}
    assert cap == 21760 and sorted(crossing) == [20, 23, 26, 28, 30, 32, 35, 39] and crossing[20] == 704
    inside = []

    def wrap(level, got, pkeys, par):
        if level not in crossing:
            return
        end = crossing[level]  # rows of this level before the arena's end
        keys, lo, hi = _generating_groups(pkeys, par)
        at = np.searchsorted(keys, row_keys(got))
        own = np.where(lo[at] == hi[at], lo[at], -1)  # the one group that generates row k, or -1
        grp = own[end]
        if grp < 0 or own[end - 1] != grp:
            return
        first = end - 1
        while first > 0 and own[first - 1] == grp:
            first -= 1
        assert (own[first:end] == grp).all()
        inside.append((level, (end - first) % 64))

    sizes = follow(shape_cfg("runtime", frontier_cap=cap, chunk=1024), [], what="ring", on_level=wrap)
    assert sizes == x[:len(sizes)] and sum(sizes) == g["distinct"]
    # (a reservation that happens to put the end on a batch boundary is possible, on all eight levels not)
    assert any(off for _, off in inside), inside


def test_partial_reservation_keeps_complete_levels_exact():
    """4. frontier_cap = 4096: the level that no longer fits raises the frontier-full error as before
    (children past the capacity get no row); every level before it is row-exact."""
    g = GOLD["n2_v2_t3_l2_m1"]
    x = [n for n, _ in g["levels"]]
    sizes = []
    with pytest.raises(rtla.RtlaError) as e:
        follow(shape_cfg("runtime", frontier_cap=4096), sizes, what="cap 4096")
    assert e.value.status == -3 and e.value.flags & 4
    assert sizes == x[:len(sizes)] and len(sizes) >= 12 and max(sizes) > 1024  # (several groups per level)
    assert _round64(sizes[-1]) + x[len(sizes)] > 4096  # the level that failed is the first that cannot fit
