"""The fingerprint set (rtla_kdev.h) full, clustered, contended and overflowing.

1. The three device insert protocols -- fpset_insert, home CAS + fpset_resolve, home load +
   fpset_resolve_loaded -- and k_insert_remote run on chosen fingerprints through rtla_fpset_probe and are compared with a
   sequential linear-probing set written here (RefSet: key b | 1, home a >> (64 - log2), no probe limit).
   The GPU inserts in an arbitrary order; two facts about linear probing without deletion make the
   comparison exact all the same: the set of occupied slots does not depend on the insertion order, and
   no key, in any order, probes more slots than the longest occupied run plus one.
2. The BFS on a nearly full set gives the golden counts, on an overfull one RTLA_E_OVERFLOW with
   RTLA_CAP_FPSET and exact levels up to there -- for the run-time and the compiled-in level kernels, the
   wave-per-state kernel and the sharded exchange.  Before a set is filled on the GPU, the reference set
   of the model's own seen-set keys must have no occupied run of 4096 slots (the probe limit) at that
   size; the run is compared with that of as many seeded random keys.

Longest occupied runs of the BFS cases (slots; the model's own keys | as many random keys, seed 1):

    model                                   keys   table   load   model  random
    n2_v1_t2_l1_m1                         1,760    2^11   0.86     139     159
    n1_v2_t3_l2                            3,524    2^12   0.86     141     150
    n2_v1_t3_l1_m1                        25,164    2^15   0.77     143     147
    n2_v1_t3_l1_m1_sym                    12,600    2^14   0.77     118      97
    n2_v2_t3_l2_m1 (also the wave kernel) 177,760   2^18   0.68     102      94
    cfg1, 12 levels                      251,980    2^19   0.48      43      39
    cfg2, 10 levels                      246,177    2^19   0.47      39      32
    cfg3, 9 levels                       205,451    2^18   0.78     252     207
    exhaust, 15 levels                   381,643    2^19   0.73     165     148
    n2_v1_t3_l1_m1, shard 0 of 2          13,546    2^14   0.83     148     175
    n2_v1_t3_l1_m1, shard 1 of 2          11,618    2^14   0.71      68     100
    n2_v1_t3_l1_m1, shard 2 of 8 (most)    3,903    2^12   0.95     494     884
    n2_v1_t3_l1_m1, shard 0 of 8           3,764    2^12   0.92     432     606
    n2_v1_t3_l1_m1, shard 5 of 8 (least)   2,534    2^12   0.62      41      31

(The owner is a hash of a state's server and log variables alone, so the shards' shares differ.)  The
random keys of section 1 in 2^16 slots, seed 1: runs of 29, 135, 961 and 2,158 slots at loads 0.5, 0.75,
0.9 and 0.95.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import rtla
from test_rowbuild_gpu import SHAPES

pytestmark = pytest.mark.gpu

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "bfs_counts.json")))
LIMIT = 4096  # rtla_kdev.h FPSET_PROBE_LIMIT: slots an insert examines at most
# fpset_insert | home CAS + fpset_resolve | home load + fpset_resolve_loaded | k_insert_remote (the exchange's
# owner side: the third protocol under its own thread mapping, with its own flag)
PROTOCOLS = [0, 1, 2, 3]
CAP_FPSET = 8
U64 = np.uint64


# ---- the reference

class RefSet:
    """A sequential linear-probing set of 2^log2 slots, no probe limit."""

    def __init__(self, log2, table=None):
        self.log2, self.n = log2, 1 << log2
        self.slots = [0] * self.n if table is None else [int(v) for v in table]

    def _find(self, v, lo, hi):
        try:
            return self.slots.index(v, lo, hi)
        except ValueError:
            return -1

    def insert(self, a, b):
        """True if (a, b) was new."""
        key, home = b | 1, a >> (64 - self.log2)
        for lo, hi in ((home, self.n), (0, home)):  # from the home slot to the table's end, then from slot 0
            z = self._find(0, lo, hi)
            if self._find(key, lo, hi if z < 0 else z) >= 0:
                return False
            if z >= 0:
                self.slots[z] = key
                return True
        raise AssertionError("the reference set is full")

    def insert_all(self, fps):
        return np.array([self.insert(int(a), int(b)) for a, b in fps], bool)

    def table(self):
        return np.array(self.slots, U64)


def longest_run(occupied):
    """The longest circular run of True."""
    occ = np.asarray(occupied, bool)
    if occ.all():
        return len(occ)
    occ = np.roll(occ, -int(np.flatnonzero(~occ)[0]))  # starts at an empty slot
    edge = np.flatnonzero(np.diff(np.concatenate(([False], occ, [False])).astype(np.int8)))
    return int((edge[1::2] - edge[::2]).max(initial=0))


def occupied_slots(log2, homes):
    """The slots that keys with these home slots (one entry per distinct key) occupy, in any insertion
    order: sorted by home, key i takes slot max(home i, slot of key i - 1, + 1); what runs past the last
    slot starts again at slot 0."""
    n = 1 << log2
    h = np.sort(np.asarray(homes, np.int64))
    assert len(h) <= n
    wrapped = 0
    while True:
        hh = np.concatenate((np.zeros(wrapped, np.int64), h))
        i = np.arange(len(hh))
        p = np.maximum.accumulate(hh - i) + i
        over = int((p >= n).sum())
        if over == wrapped:
            break
        wrapped = over
    occ = np.zeros(n, bool)
    occ[p[p < n]] = True
    assert int(occ.sum()) == len(h)
    return occ


def homes_of(log2, a):
    return (np.asarray(a, U64) >> U64(64 - log2)).astype(np.int64)


def random_fps(seed, n, log2=None, homes=None):
    """n fingerprints with distinct keys: random (a, b), or homes (slot numbers at `log2`) as given."""
    rng = np.random.default_rng(seed)
    b = np.unique(rng.integers(0, 1 << 63, 2 * n + 16, dtype=np.int64).astype(U64) << U64(1))
    rng.shuffle(b)
    assert len(b) >= n
    a = rng.integers(0, 1 << 63, n, dtype=np.int64).astype(U64) << U64(1) | rng.integers(0, 2, n).astype(U64)
    if homes is not None:
        low = U64((1 << (64 - log2)) - 1)
        a = np.asarray(homes, np.int64).astype(U64) << U64(64 - log2) | (a & low)
    return np.stack((a, b[:n]), axis=1)


def reference_table(log2, fps):
    ref = RefSet(log2)
    assert ref.insert_all(fps).all()
    return ref.table()


def check_against_reference(log2, fps, new, table, flags, want=None):
    """One launch of distinct-key fingerprints into an empty set against the reference's table `want`."""
    want = reference_table(log2, fps) if want is None else want
    assert flags == 0
    assert int(new.sum()) == len(fps) == int((want != 0).sum())
    assert np.array_equal(table != 0, want != 0), "other slots occupied than the reference's"
    assert np.array_equal(np.sort(table), np.sort(want)), "other keys stored than presented"
    # every stored key is reachable: the slots from its home to its position are occupied
    n = 1 << log2
    home = dict(zip((fps[:, 1] | U64(1)).tolist(), homes_of(log2, fps[:, 0]).tolist()))
    occ2 = np.concatenate(([0], np.cumsum(np.tile(table != 0, 2))))
    for pos in np.flatnonzero(table).tolist():
        h = home[int(table[pos])]
        d = (pos - h) % n
        assert occ2[h + d + 1] - occ2[h] == d + 1, "key at slot %d is cut off from its home %d" % (pos, h)
    return want


def assert_all_present(log2, fps, table, protocol, seed=7):
    """The same keys in another order on the returned table: nothing new, the table unchanged."""
    again = fps[np.random.default_rng(seed).permutation(len(fps))]
    new, after, flags = rtla.fpset_probe(log2, again, protocol, table)
    assert flags == 0 and not new.any() and np.array_equal(after, table)


# ---- 1. the three protocols on chosen keys

LOAD_SEED = {0.5: 1, 0.75: 1, 0.9: 1, 0.95: 1}  # seeds whose reference set passes the precondition


@functools.lru_cache(maxsize=None)
def keys_at_load(load):
    fps = random_fps(LOAD_SEED[load], int(load * (1 << 16)))
    run = longest_run(occupied_slots(16, homes_of(16, fps[:, 0])))
    return fps, run, (reference_table(16, fps) if run < LIMIT else None)


@pytest.mark.parametrize("protocol", PROTOCOLS)
@pytest.mark.parametrize("load", sorted(LOAD_SEED))
def test_random_keys_at_load(load, protocol):
    fps, run, want = keys_at_load(load)
    assert run < LIMIT, "precondition: longest occupied run %d at load %s" % (run, load)
    assert longest_run(want != 0) == run
    new, table, flags = rtla.fpset_probe(16, fps, protocol)
    check_against_reference(16, fps, new, table, flags, want)
    for other in PROTOCOLS:  # a table built by one protocol, probed by each
        assert_all_present(16, fps, table, other, seed=other)


def _strided(fps, copies, stride, filler):
    """Each of fps `copies` times, the copies of one `stride` inputs apart (chunks of `stride`
    fingerprints, each chunk repeated row after row); the last chunk's rows are filled up with `filler`."""
    out = []
    for k in range(0, len(fps), stride):
        row = fps[k:k + stride]
        row = np.concatenate((row, np.repeat(filler, stride - len(row), axis=0)))
        out.append(np.tile(row, (copies, 1)))
    return np.concatenate(out)


@pytest.mark.parametrize("protocol", PROTOCOLS)
@pytest.mark.parametrize("arrangement", ["wave", "blocks", "all-equal"])
def test_duplicates_are_new_exactly_once(arrangement, protocol):
    """64 copies of a fingerprint in one wave, or 256 inputs apart (in different blocks), and 64,000
    copies of one: exactly one copy is reported new, and the key is stored once."""
    log2 = 13
    base = random_fps(11, 1001)
    if arrangement == "wave":
        fps = np.repeat(base[:1000], 64, axis=0)
    elif arrangement == "blocks":
        fps = _strided(base[:1000], 64, 256, base[1000:])
        assert (fps[256:256 + 256] == fps[:256]).all() and len(fps) == 4 * 256 * 64
    else:
        fps = np.repeat(base[:1], 64000, axis=0)
    new, table, flags = rtla.fpset_probe(log2, fps, protocol)
    assert flags == 0
    distinct, inverse = np.unique(fps, axis=0, return_inverse=True)
    assert (np.bincount(inverse.ravel(), weights=new, minlength=len(distinct)) == 1).all()
    assert np.array_equal(np.sort(table[table != 0]), np.sort(distinct[:, 1] | U64(1)))
    ref = RefSet(log2)
    ref.insert_all(distinct)
    assert np.array_equal(table != 0, ref.table() != 0)
    assert_all_present(log2, distinct, table, protocol)


@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_cluster_wraps_past_the_last_slot(protocol):
    """600 keys whose homes are the table's last 8 slots: the cluster runs across slot 0."""
    log2 = 13
    rng = np.random.default_rng(5)
    fps = random_fps(5, 600, log2, (1 << log2) - 8 + rng.integers(0, 8, 600))
    occ = occupied_slots(log2, homes_of(log2, fps[:, 0]))
    assert occ[:500].all() and occ[-1] and not occ[1000] and longest_run(occ) < LIMIT
    new, table, flags = rtla.fpset_probe(log2, fps, protocol)
    check_against_reference(log2, fps, new, table, flags)
    for other in PROTOCOLS:
        assert_all_present(log2, fps, table, other)


@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_probe_limit_is_4096_slots(protocol):
    """Keys of one home in a 2^14 table: 4096 all fit (the last one examines 4096 slots); of 4097 in one
    launch one is dropped with RTLA_CAP_FPSET; so is a 4097th presented to the table of 4096."""
    log2, home = 14, (1 << 14) - 1000  # (the cluster wraps as well)
    fps = random_fps(3, LIMIT + 1, log2, np.full(LIMIT + 1, home))
    st, new, table, flags = rtla.fpset_probe_status(log2, fps[:LIMIT], protocol)
    assert st == rtla.OK and flags == 0 and new.all()
    check_against_reference(log2, fps[:LIMIT], new, table, flags)

    st, new1, table1, flags1 = rtla.fpset_probe_status(log2, fps, protocol)
    assert int(new1.sum()) == LIMIT and flags1 & CAP_FPSET and st == rtla.E_OVERFLOW
    assert int((table1 != 0).sum()) == LIMIT and np.array_equal(table1 != 0, table != 0)
    assert np.isin(table1[table1 != 0], fps[:, 1] | U64(1)).all()

    st, new2, table2, flags2 = rtla.fpset_probe_status(log2, fps[LIMIT:], protocol, table)
    assert not new2.any() and flags2 & CAP_FPSET and st == rtla.E_OVERFLOW
    assert np.array_equal(table2, table)


@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_equal_b_in_different_homes(protocol):
    """The set's key is fp.b | 1 within a cluster: equal b with homes 2^12 slots apart (different
    clusters) are two states, with adjacent homes inside one occupied cluster they are merged by design
    -- as the reference models it."""
    log2, sh = 13, U64(64 - 13)
    b = U64(0x1234567890ABCDEE)
    apart = np.array([[U64(100) << sh, b], [U64(100 + 4096) << sh, b]], U64)
    new, table, flags = rtla.fpset_probe(log2, apart, protocol)
    assert flags == 0 and new.all() and RefSet(log2).insert_all(apart).all()
    assert (table[[100, 100 + 4096]] == (b | U64(1))).all() and int((table != 0).sum()) == 2

    cluster = random_fps(9, 20, log2, np.full(20, 3000))  # occupies slots 3000 .. 3019
    new, table, flags = rtla.fpset_probe(log2, cluster, protocol)
    assert flags == 0 and new.all() and (table[3000:3020] != 0).all()
    pair = np.array([[U64(3003) << sh, b], [U64(3004) << sh, b]], U64)
    ref = RefSet(log2, table)
    assert ref.insert_all(pair).tolist() == [True, False]
    new, after, flags = rtla.fpset_probe(log2, pair, protocol, table)
    assert flags == 0 and int(new.sum()) == 1
    assert np.array_equal(after, ref.table()) and after[3020] == (b | U64(1))


def test_probe_seam_rejects_bad_arguments():
    fps = random_fps(1, 4)
    for log2 in (9, 31):  # (the table is not touched)
        with pytest.raises(rtla.RtlaError) as e:
            rtla.fpset_probe(log2, fps, 0)
        assert e.value.status == rtla.E_ARG
    with pytest.raises(rtla.RtlaError) as e:
        rtla.fpset_probe(10, fps, 4)
    assert e.value.status == rtla.E_ARG


def test_probe_bench_overflow_is_an_error():
    """2^16 + 1 random keys cannot all enter 2^16 slots: RTLA_E_OVERFLOW, not a short count."""
    for bench in (rtla.probe_bench, rtla.probe_bench2):
        with pytest.raises(rtla.RtlaError) as e:
            bench(16, (1 << 16) + 1)
        assert e.value.status == rtla.E_OVERFLOW


# ---- 2. the BFS on a nearly full and an overfull set

KW = dict(mem_budget=1 << 30)
ROOMY = 22


def gold_cfg(name, **kw):
    g = GOLD[name]
    return rtla.Config(g["n_server"], g["n_value"], g["max_term"], g["max_log"], g["max_copies"], g["max_msgs"],
                       tuple(g["invariants"]), symmetry=bool(g.get("symmetry", False)), **dict(KW, **kw))


def level_keys(cfg, ck):
    """The seen-set keys (a, b) of the level last produced: the stored fingerprints, or under SYMMETRY
    the orbit keys."""
    rows = np.frombuffer(ck.frontier_flat(), np.uint32).reshape(-1, rtla.row_words(cfg))
    if cfg.symmetry:
        return np.array([rtla.orbit_key(cfg, r.tolist())[0] for r in rows], U64).reshape(-1, 2)
    r = rows[:, :4].astype(U64)
    return np.stack((r[:, 0] | r[:, 1] << U64(32), r[:, 2] | r[:, 3] << U64(32)), axis=1)


def roomy_keys(cfg, levels):
    """Keys of the first `levels` levels of a run with a roomy set, whose counts are the fixture's."""
    keys = []
    with rtla.Checker(cfg) as ck:
        st = ck.init()
        while True:
            keys.append(level_keys(cfg, ck))
            if st != rtla.OK or len(keys) >= levels:
                break
            st = ck.step()
        counts = [[lv.new, lv.generated] for lv in ck.levels]
    return np.concatenate(keys), counts


@functools.lru_cache(maxsize=None)
def model_keys(name):
    g = GOLD[name]
    keys, counts = roomy_keys(gold_cfg(name, fpset_log2=ROOMY), len(g["levels"]))
    assert counts == g["levels"] and len(keys) == g["distinct"]
    return keys


def precondition(keys, log2, what):
    """The reference set of these keys at 2^log2 slots stays under the probe limit in any insertion
    order; its longest occupied run against that of as many random keys.  A model's run of more than 4 x
    the random keys' would say that the top bits of fp.a, the home slot, are badly mixed for real states
    (runs of random key sets differ by ~1.5 x between seeds)."""
    assert len(np.unique(keys[:, 1] | U64(1))) == len(keys), "%s: two states share a key" % what
    run = longest_run(occupied_slots(log2, homes_of(log2, keys[:, 0])))
    rnd = longest_run(occupied_slots(log2, homes_of(log2, random_fps(1, len(keys))[:, 0])))
    msg = "%s: %d keys in 2^%d slots (load %.2f): longest occupied run %d, of random keys %d" % (
        what, len(keys), log2, len(keys) / (1 << log2), run, rnd)
    print(msg)
    assert run < LIMIT, msg
    assert run <= 4 * rnd, msg
    return run


def run_levels(cfg, digest=None):
    """ck.run(): (the complete levels' counts, distinct, generated, the error or None, digests)."""
    err, digests = None, []
    with rtla.Checker(cfg) as ck:
        try:
            st = ck.init()
            while True:
                if digest is not None and len(digests) < len(digest):
                    digests.append("%016x" % ck.level_text_hash())
                if st != rtla.OK:
                    break
                st = ck.step()
        except rtla.RtlaError as e:
            err = e
        return [[lv.new, lv.generated] for lv in ck.levels], ck.distinct, ck.generated, err, digests


HIGH_LOAD = [("n2_v1_t2_l1_m1", 11), ("n1_v2_t3_l2", 12), ("n2_v1_t3_l1_m1", 15), ("n2_v1_t3_l1_m1_sym", 14),
             ("n2_v2_t3_l2_m1", 18)]


@pytest.mark.parametrize("name,log2", HIGH_LOAD)
def test_bfs_exact_at_high_load(name, log2):
    g = GOLD[name]
    assert 0.66 < g["distinct"] / (1 << log2) < 0.87
    precondition(model_keys(name), log2, name)
    want = g["level_text_hash"] if name == "n2_v2_t3_l2_m1" else None
    levels, distinct, generated, err, digests = run_levels(gold_cfg(name, fpset_log2=log2), want)
    assert err is None, err
    assert levels == g["levels"] and (distinct, generated) == (g["distinct"], g["generated"])
    if want:
        assert digests == want[:len(digests)] and len(digests) >= len(want) - 1


SPEC_PREFIX = {"cfg1": "n3_v1_t2_l1_c1_prefix", "cfg2": "n3_v2_t3_l2_c1_prefix", "cfg3": "n3_v2_t4_l3_c2_prefix",
               "exhaust": "n3_v2_t2_l2_m2_prefix"}


@pytest.mark.parametrize("name", sorted(SPEC_PREFIX))
def test_compiled_in_kernels_fill_their_set(name):
    """The compiled-in instantiations of the level kernel: the first K levels (under 5e5 states) exact in
    the smallest set that they load to at most 0.9; from there on a level is exact or the set is full, at
    the latest when there are more states than slots."""
    g = GOLD[SPEC_PREFIX[name]]
    shape, inv, bag = SHAPES[name]
    assert (g["n_server"], g["n_value"], g["max_term"], g["max_log"], g["max_copies"], g["max_msgs"]) == shape
    assert tuple(g["invariants"]) == tuple(inv)
    cum = np.cumsum([n for n, _ in g["levels"]])
    K = int(np.searchsorted(cum, 500_000))  # levels whose cumulative count stays under 5e5
    log2 = next(b for b in range(10, 31) if cum[K - 1] <= 0.9 * (1 << b))
    over = int(np.searchsorted(cum, 1 << log2, "right"))  # 0-based level that no longer fits
    assert 3 <= K <= over < len(cum) and cum[K - 1] < 500_000 <= cum[K]
    keys, counts = roomy_keys(rtla.Config(*shape, inv, bag_cap=bag, fpset_log2=ROOMY, **KW), K)
    assert counts == g["levels"][:K]
    precondition(keys, log2, "%s, %d levels" % (name, K))
    levels, _, _, err, _ = run_levels(rtla.Config(*shape, inv, bag_cap=bag, fpset_log2=log2, **KW))
    assert err is not None and err.status == rtla.E_OVERFLOW and err.flags & CAP_FPSET, err
    assert K <= len(levels) <= over and levels == g["levels"][:len(levels)]


_CHILD = """
import json, sys, rtla
g = json.load(open(sys.argv[1]))[sys.argv[2]]
cfg = rtla.Config(g['n_server'], g['n_value'], g['max_term'], g['max_log'], g['max_copies'], g['max_msgs'],
                  tuple(g['invariants']), fpset_log2=int(sys.argv[3]), mem_budget=1 << 30)
out = {'status': 0, 'flags': 0}
with rtla.Checker(cfg) as ck:
    try:
        ck.run()
    except rtla.RtlaError as e:
        out = {'status': e.status, 'flags': e.flags}
    out.update(levels=[[lv.new, lv.generated] for lv in ck.levels], distinct=ck.distinct, generated=ck.generated)
print(json.dumps(out))
"""


def wave_kernel_run(name, log2):
    """The BFS under the wave-per-state kernel (RTLA_XFLAGS=2048, read once: a child process)."""
    here = os.path.dirname(__file__)
    env = dict(os.environ, RTLA_XFLAGS="2048",
               PYTHONPATH=os.pathsep.join([os.path.join(here, "..", "raft-tla_amd"), os.environ.get("PYTHONPATH", "")]))
    out = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(here, "golden", "bfs_counts.json"), name,
                          str(log2)], env=env, capture_output=True, text=True, timeout=100)
    assert out.returncode == 0, out.stdout + out.stderr
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_wave_kernel_exact_at_high_load():
    name, log2 = "n2_v2_t3_l2_m1", 18
    g = GOLD[name]
    precondition(model_keys(name), log2, name)
    got = wave_kernel_run(name, log2)
    assert got["status"] == 0 and got["levels"] == g["levels"]
    assert (got["distinct"], got["generated"]) == (g["distinct"], g["generated"])


def owner_of(keys, shards):
    """rtla_device.h fp_owner: the low 32 bits of fp.a scaled to the shards."""
    return ((keys[:, 0] & U64(0xFFFFFFFF)) * U64(shards) >> U64(32)).astype(np.int64)


@pytest.mark.parametrize("sent", [1, 0])
@pytest.mark.parametrize("shards", [2, 8])
def test_virtual_shards_exact_at_high_load(monkeypatch, shards, sent):
    """Each shard's set holds the keys it owns (fp_owner): the smallest size that holds the fullest
    shard's keys, every shard's reference set within the precondition -- a load of 0.83 of 2^14 slots at
    2 shards, of 0.95 of 2^12 at 8."""
    monkeypatch.setenv("RTLA_SENT_CACHE", str(sent))
    name = "n2_v1_t3_l1_m1"
    g = GOLD[name]
    keys = model_keys(name)
    owner = owner_of(keys, shards)
    most = int(np.bincount(owner, minlength=shards).max())
    log2 = next(b for b in range(10, 31) if most < 1 << b)
    assert most / (1 << log2) > 0.8
    for p in range(shards):
        precondition(keys[owner == p], log2, "%s, shard %d of %d" % (name, p, shards))
    levels, distinct, generated, err, _ = run_levels(gold_cfg(name, fpset_log2=log2, shards=shards))
    assert err is None, err
    assert levels == g["levels"] and (distinct, generated) == (g["distinct"], g["generated"])


def assert_overfull(levels, err, g):
    assert err is not None and err.status == rtla.E_OVERFLOW and err.flags & CAP_FPSET, err
    assert levels == g["levels"][:len(levels)] and 0 < len(levels) < len(g["levels"])


@pytest.mark.parametrize("name,log2,shards", [("n2_v1_t2_l1_m1", 10, 0), ("n2_v1_t3_l1_m1", 14, 0),
                                              ("n2_v1_t3_l1_m1", 13, 2)])
def test_overfull_set_is_an_error(name, log2, shards):
    """More states than slots (2^10 is the smallest set rtla_open accepts, smaller than the probe limit:
    a probe of the full table goes round it four times and ends): RTLA_E_OVERFLOW with RTLA_CAP_FPSET,
    never a short count -- whichever shard's set filled -- and every level before it exact."""
    g = GOLD[name]
    assert g["distinct"] > max(shards, 1) << log2
    levels, _, _, err, _ = run_levels(gold_cfg(name, fpset_log2=log2, shards=shards))
    assert_overfull(levels, err, g)
    cum = np.cumsum([n for n, _ in g["levels"]])
    assert cum[len(levels)] > 0.5 * (max(shards, 1) << log2)  # (it did not give up on a half-empty set)


def test_overfull_set_is_an_error_under_the_wave_kernel():
    name = "n2_v1_t3_l1_m1"
    got = wave_kernel_run(name, 14)
    assert got["status"] == rtla.E_OVERFLOW and got["flags"] & CAP_FPSET, got
    assert got["levels"] == GOLD[name]["levels"][:len(got["levels"])] and 0 < len(got["levels"]) < len(GOLD[name]["levels"])
