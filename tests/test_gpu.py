"""GPU parity tests: the HIP path (through the C ABI) against the oracle.

* per-level (new, generated) counts, distinct, generated, depth and verdict
  against the committed golden fixtures (tests/golden/bfs_counts.json);
* exact level CONTENTS: the sum of FNV-1a(state text) over each level's
  states, decoded from the GPU frontier rows, equals the oracle's;
* lockstep random walks: at every step the multiset of successor texts (with
  in-model flags) from rtla_expand_batch equals the C oracle's;
* counterexample traces: shortest length, every step a legal transition in
  the oracle, the last state violating the invariant.
"""
import functools
import json
import os
import random

import pytest

import raft_cpu
import raft_values as rv
import rtla

pytestmark = pytest.mark.gpu

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "bfs_counts.json")))
SMALL = sorted(k for k, v in GOLD.items() if v["distinct"] < 3_000_000 and not v.get("prefix"))
HASHED = sorted(k for k in SMALL if "level_text_hash" in GOLD[k] or "level_orbit_hash" in GOLD[k])


def level_digests(g):
    """The fixture's per-level content digests and the checker's matching
    method: state texts, or (SYMMETRY) orbit texts -- the text of the image
    whose rotated text is least over all server permutations, the same for
    whichever member of an orbit the GPU or the oracle keeps."""
    if g.get("symmetry"):
        return g.get("level_orbit_hash", []), lambda ck: ck.level_orbit_hash()
    return g.get("level_text_hash", []), lambda ck: ck.level_text_hash()


def cfg_of(g, **kw):
    kw.setdefault("symmetry", bool(g.get("symmetry", False)))
    return rtla.Config(g["n_server"], g["n_value"], g["max_term"], g["max_log"], g["max_copies"],
                       g["max_msgs"], tuple(g["invariants"]), **kw)


def small_kw(g):
    log2 = max(16, (int(g["distinct"] * 2)).bit_length())
    return dict(fpset_log2=log2, mem_budget=(8 << log2) * 3 + (1 << 28))


@pytest.mark.parametrize("name", SMALL)
def test_bfs_counts_match_golden(name):
    g = GOLD[name]
    res = rtla.check(cfg_of(g, **small_kw(g)), trace=False)
    assert [[lv.new, lv.generated] for lv in res.levels] == g["levels"]
    assert (res.distinct, res.generated, res.depth) == (g["distinct"], g["generated"], g["depth"])
    assert (res.violation is not None) == bool(g["violated"])


@pytest.mark.parametrize("name", HASHED)
def test_level_contents_match_oracle(name):
    g = GOLD[name]
    cfg = cfg_of(g, **small_kw(g))
    want, digest = level_digests(g)
    got = []
    with rtla.Checker(cfg) as ck:
        st = ck.init()
        while True:
            got.append("%016x" % digest(ck))
            if st != rtla.OK or len(got) >= len(want):
                break
            st = ck.step()
    n = min(len(got), len(want))
    assert n >= len(want) - 1 and got[:n] == want[:n]


WALKS = [(2, 2, 3, 2, 1, 1), (3, 1, 2, 1, 1, 2), (3, 2, 3, 2, 1, 3), (3, 2, 4, 3, 2, 4),
         (5, 1, 3, 2, 1, 3), (2, 1, 3, 1, 2, 0)]


@pytest.mark.parametrize("shape", WALKS)
def test_lockstep_walk_successors_match_oracle(shape):
    n, v, t, l, c, m = shape
    cfg = rtla.Config(n, v, t, l, c, m, ("NoTwoLeaders", "ElectionSafety", "LogMatching"))
    walk = raft_cpu.Walk(raft_cpu.cfg_of(n, v, t, l, c, m, ("NoTwoLeaders", "ElectionSafety", "LogMatching")))
    rnd = random.Random(hash(shape) & 0xFFFF)
    row = rtla.init_row(cfg)
    assert rtla.state_text(cfg, row) == walk.text()
    for step in range(120):
        gpu = rtla.expand_batch(cfg, [row])
        mine = sorted((im, rtla.state_text(cfg, r)) for _, _, _, im, r in gpu)
        ref = sorted(walk.successors())
        assert mine == ref, "successor multiset differs at step %d" % step
        inm = [x for x in gpu if x[3]]
        if not inm:
            break
        pick = rnd.choice(inm)
        row = pick[4]
        text = rtla.state_text(cfg, row)
        walk.goto(text)
        assert rtla.invariants_violated(cfg, row) == walk.invariants()


# BASELINE configs[0]-[3] shapes (N, V, T, L, C, in-flight bound) with the bag slots bench.py compiles for them
BASELINE_WALKS = [((3, 1, 2, 1, 1, 0), 24), ((3, 2, 3, 2, 1, 0), 18), ((3, 2, 4, 3, 2, 0), 20), ((5, 1, 3, 2, 1, 0), 20)]


@pytest.mark.parametrize("shape,bag", BASELINE_WALKS)
def test_walk_successors_match_value_oracle(shape, bag):
    """At every BASELINE shape, N = 5 (configs[3]) included: along a random
    walk, the successor multiset the level kernel generates for a state
    (rtla_expand_batch: k_expand_compact in its all-successors mode; texts and
    in-model flags) equals the VALUE oracle's -- raft_values.next_states, the
    literal transcription of raft.tla's Next -- on the state parsed from its
    text; no C-oracle code in the loop."""
    import tla_text
    n, v, t, l, c, m = shape
    cfg = rtla.Config(n, v, t, l, c, m, (), bag_cap=bag)
    vc = rv.Cfg(n, v, t, l, c, (), m)
    rnd = random.Random(sum(shape) * 17 + n)
    row = rtla.init_row(cfg)
    checked = 0
    for step in range(60):
        text = rtla.state_text(cfg, row)
        ref = sorted((rv.in_model(vc, x), rv.state_text(vc, x))
                     for _, x in rv.next_states(vc, tla_text.parse_state(vc, text)))
        gpu = rtla.expand_batch(cfg, [row])
        mine = sorted((bool(im), rtla.state_text(cfg, r)) for _, _, _, im, r in gpu)
        assert mine == ref, "shape %s step %d" % (shape, step)
        checked += len(mine)
        # continue through an in-model successor whose bag leaves room for the next step
        nxt = [x for x in gpu if x[3] and rtla.state_text(cfg, x[4]).split("\n", 1)[0].count(" :> ") < bag - 1]
        if not nxt:
            break
        row = rnd.choice(nxt)[4]
    assert checked > 300


@pytest.mark.parametrize("shape", [(5, 1, 3, 2, 1, 0), (4, 1, 2, 1, 1, 2), (3, 2, 3, 2, 1, 3)])
def test_symmetric_lockstep_walk_orbit_keys_match_oracle(shape):
    """SYMMETRY at the successor level, N = 5 (BASELINE configs[3]'s shape)
    included: along a random walk, the successors the GPU generates
    (rtla_expand_batch runs the level kernel) are grouped into orbits by the
    product's orbit key (rtla_model.h sym_key, the seen-set key the kernel
    probes) exactly as the C oracle groups them by its least orbit
    serialisation over all N! permutations; and each successor's orbit text
    (rtla_orbit_text) equals the oracle's."""
    n, v, t, l, c, m = shape
    cfg = rtla.Config(n, v, t, l, c, m, (), symmetry=True, bag_cap=20)
    walk = raft_cpu.Walk(raft_cpu.cfg_of(n, v, t, l, c, m, (), symmetry=True))
    rnd = random.Random(sum(shape))
    row = rtla.init_row(cfg)
    checked = 0
    for step in range(60):
        gpu = [x for x in rtla.expand_batch(cfg, [row]) if x[3]]
        texts = walk.successors()
        orbits = walk.orbits()          # (oracle key, orbit text) per successor, in texts' order
        ref = {}
        for (im, tx), (okey, otext) in zip(texts, orbits):
            if im:
                ref[tx] = (okey, otext)
        mine_key, mine_orb = {}, {}
        for x in gpu:
            tx = rtla.state_text(cfg, x[4])
            okey, otext = ref[tx]
            assert rtla.orbit_text(cfg, x[4]) == otext, "step %d" % step
            mine_key.setdefault(rtla.orbit_key(cfg, x[4])[0], set()).add(okey)
            mine_orb.setdefault(okey, set()).add(rtla.orbit_key(cfg, x[4])[0])
            checked += 1
        # the two partitions of the successors into orbits coincide
        assert all(len(v) == 1 for v in mine_key.values()) and all(len(v) == 1 for v in mine_orb.values())
        if not gpu:
            break
        row = rnd.choice(gpu)[4]
        walk.goto(rtla.state_text(cfg, row))
    assert checked > 200


def test_incremental_fingerprint_equals_full_rehash():
    """The kernel derives each successor's fingerprint from its parent's; the
    stored fingerprint of every successor row (in-model or not) must equal a
    from-scratch hash of the row, the same state reached along different
    paths must carry the same fingerprint, and distinct states distinct ones."""
    cfg = rtla.Config(3, 1, 2, 1, 1, 2, ())
    row = rtla.init_row(cfg)
    seen = {}
    frontier = [row]
    checked = 0
    for _ in range(6):
        succ = rtla.expand_batch(cfg, frontier)
        frontier = []
        for _, _, _, im, r in succ:
            assert rtla.stored_fingerprint(r) == rtla.row_fingerprint(cfg, r), rtla.state_text(cfg, r)
            checked += 1
            if not im:
                continue
            text = rtla.state_text(cfg, r)
            fp = tuple(r[:4])
            if text in seen:
                assert seen[text] == fp
            else:
                seen[text] = fp
                frontier.append(r)
    assert checked > 1000
    fps = {}
    for text, fp in seen.items():
        assert fp not in fps, "fingerprint collision between distinct states"
        fps[fp] = text


PROJ_VARS = ("currentTerm", "state", "votedFor", "log", "commitIndex")


def _projection(text):
    return tuple(ln for ln in text.split("\n") if ln[3:].split(" = ", 1)[0] in PROJ_VARS)


@pytest.mark.parametrize("shape,bag", BASELINE_WALKS[:3])
def test_shard_owner_is_a_function_of_the_projection(shape, bag):
    """The multi-GPU owner (fp_owner: the low 32 bits of the fingerprint's
    first half) is a hash of the state's serverVars + logVars alone: along a
    random walk, a successor keeps its parent's owner bits exactly when its
    currentTerm / state / votedFor / log / commitIndex lines are unchanged --
    so the bag-only and candidate/leader-var-only actions (RequestVote,
    AppendEntries, the response handlers, Duplicate/Drop) keep successors on
    their parent's shard; the rest move."""
    n, v, t, l, c, m = shape
    cfg = rtla.Config(n, v, t, l, c, m, (), bag_cap=bag)
    rnd = random.Random(n * 31 + t)
    row = rtla.init_row(cfg)
    same = moved = 0
    for step in range(40):
        ptext = rtla.state_text(cfg, row)
        plow = rtla.stored_fingerprint(row)[0] & 0xFFFFFFFF
        assert rtla.row_fingerprint(cfg, row)[0] & 0xFFFFFFFF == plow
        succ = [x for x in rtla.expand_batch(cfg, [row]) if x[3]]
        for x in succ:
            keep = _projection(rtla.state_text(cfg, x[4])) == _projection(ptext)
            assert (rtla.stored_fingerprint(x[4])[0] & 0xFFFFFFFF == plow) == keep, (step, x[1])
            same += keep
            moved += not keep
        nxt = [x for x in succ if rtla.state_text(cfg, x[4]).split("\n", 1)[0].count(" :> ") < bag - 1]
        if not nxt:
            break
        row = rnd.choice(nxt)[4]
    assert same > 100 and moved > 20


@functools.lru_cache(maxsize=None)
def _ntl_check():  # the small NoTwoLeaders counterexample, on the default kernel (shared: one run)
    g = GOLD["n3_v1_t3_l1_m1_ntl"]
    return rtla.check(cfg_of(g, **small_kw(g)))


def test_counterexample_trace():
    g = GOLD["n3_v1_t3_l1_m1_ntl"]
    res = _ntl_check()
    assert res.violation == "NoTwoLeaders"
    assert res.depth == g["depth"]
    tr = res.trace
    assert len(tr) == g["trace_len"] == g["depth"]
    assert tr[0][0] == "Initial predicate"
    walk = raft_cpu.Walk(raft_cpu.cfg_of(3, 1, 3, 1, 1, 1, ("NoTwoLeaders",)))
    assert walk.text() == tr[0][1]
    for label, text in tr[1:]:
        assert text in [t for _, t in walk.successors()], label
        walk.goto(text)
    assert walk.invariants() & 1
    assert tr[-1][1].count('"Leader"') >= 2


def test_out_of_model_violation_is_reported():
    """Out-of-model successors are invariant-checked (TLC semantics): with
    MaxTerm=2 a Timeout to term 3 leaves the model; NoTwoLeaders still holds
    there, so the search completes -- and the counts match the oracle."""
    g = GOLD["n3_v1_t2_l1_m1"]
    res = rtla.check(cfg_of(g, **small_kw(g)), trace=False)
    assert res.violation is None and res.distinct == g["distinct"]


def test_coverage_sums_to_generated():
    g = GOLD["n2_v2_t3_l2_m1"]
    res = rtla.check(cfg_of(g, **small_kw(g)), trace=False)
    cov = res.coverage
    fam = ["Restart", "Timeout", "RequestVote", "BecomeLeader", "ClientRequest", "AdvanceCommitIndex",
           "AppendEntries", "DuplicateMessage", "DropMessage", "UpdateTerm", "HandleRequestVoteRequest",
           "HandleRequestVoteResponse", "HandleAppendEntriesRequest", "HandleAppendEntriesResponse",
           "DropStaleResponse"]
    assert sum(cov[f][0] for f in fam) == res.generated - 1
    assert sum(cov[f][1] for f in fam) == res.distinct - 1


BIG = sorted(k for k, v in GOLD.items() if v["distinct"] >= 3_000_000 and not v.get("prefix"))
PREFIX = sorted(k for k, v in GOLD.items() if v.get("prefix"))


@pytest.mark.parametrize("name", BIG)
def test_full_size_counts_match_golden(name):
    """The oracle's largest exhausted models (up to 1.45e8 states): every
    level's counts, and the set of states of every level (the level digest of
    the decoded GPU rows, rtla_level_text_hash, against the oracle's)."""
    g = GOLD[name]
    cfg = cfg_of(g, fpset_log2=(g["distinct"] * 3).bit_length())
    hashes, digest = level_digests(g)
    with rtla.Checker(cfg) as ck:
        st = ck.init()
        while True:
            k = len(ck.levels) - 1
            if k < len(hashes):
                assert "%016x" % digest(ck) == hashes[k], "level %d" % (k + 1)
            if st != rtla.OK:
                break
            st = ck.step()
        assert [[lv.new, lv.generated] for lv in ck.levels] == g["levels"]
        assert (ck.distinct, ck.generated) == (g["distinct"], g["generated"])


# bench.py's row formats (bag slots) for the prefix models: the same layouts
# the bench runs, i.e. the kernels compiled for them (rtla_kernels.hip specs)
PREFIX_BAG = {"n3_v2_t3_l2_c1_prefix": 18, "n3_v1_t2_l1_c1_prefix": 24, "n5_v1_t3_l2_c1_sym_prefix": 20,
              "n3_v2_t4_l3_c2_prefix": 20}


def level_text_hash(cfg, rows):
    return "%016x" % (sum(raft_cpu.text_hash(rtla.state_text(cfg, r)) for r in rows) & (2**64 - 1))


def test_level_digest_equals_python_recount():
    """rtla_level_text_hash (device rows streamed to host threads) equals the
    digest recomputed row by row through rtla_state_text + the oracle's FNV."""
    g = GOLD["n2_v2_t3_l2_m1"]
    cfg = cfg_of(g, shards=2, chunk=512, **small_kw(g))
    with rtla.Checker(cfg) as ck:
        ck.init()
        for _ in range(7):
            ck.step()
        assert "%016x" % ck.level_text_hash() == level_text_hash(cfg, ck.frontier()) == g["level_text_hash"][7]


@pytest.mark.parametrize("name", PREFIX)
def test_prefix_levels_match_golden(name):
    """Models too large for the CPU oracle to exhaust -- BASELINE configs[0],
    [1] and [2] exactly as stated, to the depth bench.py times them at, the
    exhaust model's first 31 levels, and the SYMMETRY prefixes: per-level
    counts, and the contents of EVERY level: the level digest of the decoded
    GPU rows (SYMMETRY: of their orbit texts -- configs[3] to the 15 levels
    bench.py times) against the oracle's."""
    g = GOLD[name]
    cfg = cfg_of(g, fpset_log2=max(30, (g["distinct"] * 3).bit_length()), bag_cap=PREFIX_BAG.get(name, 0))
    hashes, digest = level_digests(g)
    with rtla.Checker(cfg) as ck:
        st = ck.init()
        while True:
            k = len(ck.levels) - 1
            if k < len(hashes):
                assert "%016x" % digest(ck) == hashes[k], "level %d" % (k + 1)
            if len(ck.levels) >= len(g["levels"]):
                break
            assert st == rtla.OK
            st = ck.step()
        assert [[lv.new, lv.generated] for lv in ck.levels] == g["levels"]


DEEP_SAMPLE = 300


@pytest.mark.parametrize("name", sorted(PREFIX_BAG))
def test_deep_level_successors_match_value_oracle(name):
    """States only deep BFS reaches, checked against the VALUE oracle (the
    literal transcription of raft.tla's Next, raft.tla:454-465), not the C
    oracle that pins the deep level digests: each BASELINE prefix (configs[0]
    L23, [1] L17, [2] L14, [3] L15 -- the levels bench.py times) runs to its
    last benched level, DEEP_SAMPLE rows are drawn uniformly from that level
    (rtla_frontier_rows), and each row's successor multiset from the level
    kernel (rtla_expand_batch: texts + in-model flags) equals
    raft_values.next_states on the row's parsed text.  SYMMETRY (configs[3]):
    the row's orbit text and one in-model successor's orbit text (the C++ host
    code) equal the value oracle's orbit_text (all 120 images in full)."""
    import tla_text
    g = GOLD[name]
    sym = bool(g.get("symmetry"))
    cfg = cfg_of(g, fpset_log2=max(30, (g["distinct"] * 3).bit_length()), bag_cap=PREFIX_BAG[name])
    vc = rv.Cfg(g["n_server"], g["n_value"], g["max_term"], g["max_log"], g["max_copies"], tuple(g["invariants"]),
                g["max_msgs"])
    with rtla.Checker(cfg) as ck:
        st = ck.init()
        while len(ck.levels) < len(g["levels"]):
            assert st == rtla.OK
            st = ck.step()
        assert [[lv.new, lv.generated] for lv in ck.levels] == g["levels"]
        n = ck.frontier_size()
        assert n == g["levels"][-1][0]
        rnd = random.Random(len(g["levels"]) * 7919 + g["n_server"])
        idx = sorted(rnd.sample(range(n), DEEP_SAMPLE))
        rows = ck.frontier_rows(idx)
    assert len({tuple(r) for r in rows}) == DEEP_SAMPLE
    succ = [[] for _ in rows]
    for k in range(0, len(rows), 50):
        for i, _, _, im, r in rtla.expand_batch(cfg, rows[k:k + 50]):
            succ[k + i].append((bool(im), r))
    checked = 0
    for k, row in enumerate(rows):
        text = rtla.state_text(cfg, row)
        s = tla_text.parse_state(vc, text)
        assert rv.state_text(vc, s) == text
        ref = sorted((rv.in_model(vc, x), rv.state_text(vc, x)) for _, x in rv.next_states(vc, s))
        mine = sorted((im, rtla.state_text(cfg, r)) for im, r in succ[k])
        assert mine == ref, "%s: frontier row %d" % (name, idx[k])
        checked += len(mine)
        if sym:
            assert rtla.orbit_text(cfg, row) == rv.orbit_text(vc, s), "row %d" % idx[k]
            inm = [r for im, r in succ[k] if im]
            if inm:
                r = rnd.choice(inm)
                t = rtla.orbit_text(cfg, r)
                assert t == rv.orbit_text(vc, tla_text.parse_state(vc, rtla.state_text(cfg, r))), "row %d" % idx[k]
    assert checked > 10 * DEEP_SAMPLE


def test_bench_model_full_size_sharding_invariant():
    """At the bench model's full size (2.4e9 states, beyond the CPU oracle):
    the search split into 2 fingerprint-owned shards (the multi-GPU exchange
    protocol) must reproduce the single-shard per-level counts exactly."""
    base = dict(n_server=3, n_value=2, max_term=2, max_log=2, max_copies=1, max_msgs=2,
                invariants=("ElectionSafety", "LogMatching"))
    one = rtla.check(rtla.Config(**base, fpset_log2=32), trace=False)
    two = rtla.check(rtla.Config(**base, fpset_log2=31, shards=2, mem_budget=220 << 30), trace=False)
    assert one.violation is None and two.violation is None
    assert [[lv.new, lv.generated] for lv in two.levels] == [[lv.new, lv.generated] for lv in one.levels]
    assert one.distinct > 2_000_000_000


def test_fpset_probe_bench_inserts_all():
    sec, ins = rtla.probe_bench(26, 1 << 24)
    assert ins == 1 << 24 and sec > 0


# ---- fingerprint-sharded search (the multi-GPU protocol on one device) ----
# (the last two: the row format's limits -- 4-bit message counts, 2-bit values -- through the exchange)
SHARDED = ["n2_v2_t3_l2_m1", "n3_v1_t2_l1_m1", "n2_v1_t2_l1_c2_m2", "n1_v2_t3_l2", "n1_v1_t2_l1_c14",
           "n2_v4_t2_l2_m1"]
LIMIT_MODELS = ["n1_v1_t2_l1_c14", "n2_v4_t2_l2_m1"]


@pytest.mark.parametrize("rows_cap,rehome", [("0", "1"), ("40", "1"), ("0", "0")])
@pytest.mark.parametrize("shards", [2, 8])
def test_virtual_shards_rehome_match_golden(monkeypatch, shards, rows_cap, rehome):
    """Owners by projection keep a state's successors mostly on its owner
    only if the state lives there: k_build_winners builds each remote
    winner into its owner's export region and rtla_step moves it at level
    end (rehome).  Golden counts and level contents with re-homing, with
    export regions of 40 rows (RTLA_ROWS_CAP: most winners overflow into the
    sender's own level -- the cut batch -- and the rest still move), and the
    round-5 protocol (RTLA_REHOME=0); rows did move when re-homing."""
    if rows_cap != "0":
        monkeypatch.setenv("RTLA_ROWS_CAP", rows_cap)
    monkeypatch.setenv("RTLA_REHOME", rehome)
    g = GOLD["n3_v1_t2_l1_m1"]
    kw = small_kw(g)
    kw["mem_budget"] *= shards
    want, digest = level_digests(g)
    with rtla.Checker(cfg_of(g, shards=shards, **kw)) as ck:
        st = ck.init()
        got = []
        while True:
            got.append("%016x" % digest(ck))
            if st != rtla.OK:
                break
            st = ck.step()
        assert [[lv.new, lv.generated] for lv in ck.levels] == g["levels"]
        assert got == want[:len(got)] and len(got) >= len(want) - 1
        info = json.loads(ck.device_info())
    assert (info["rehomed_rows"] > 0) == (rehome == "1"), info


@pytest.mark.parametrize("shards", [2, 3, 8])
@pytest.mark.parametrize("name", SHARDED)
def test_virtual_shards_match_golden(name, shards):
    """S fingerprint-owned shards exchanging (fp -> owner, answer -> sender,
    sender materialises) must give the single-shard counts at every level,
    also when each level is cut into many exchange rounds (small chunk)."""
    g = GOLD[name]
    kw = small_kw(g)
    kw["mem_budget"] *= shards
    res = rtla.check(cfg_of(g, shards=shards, chunk=512, **kw), trace=False)
    assert [[lv.new, lv.generated] for lv in res.levels] == g["levels"]
    assert (res.distinct, res.generated, res.depth) == (g["distinct"], g["generated"], g["depth"])


@pytest.mark.parametrize("name", ["n3_v1_t2_l1_m2", "n3_v1_t2_l1_m2_sym"])
def test_many_shards_tiny_sent_cache_match_golden(name):
    """8 fingerprint-owned shards whose sent caches (2^(fpset_log2 - 1)
    slots, overwritten on a miss) are far smaller than the millions of
    fingerprints each ships: duplicates are re-sent and deduplicated by the
    owners -- the counts stay exact, and no capacity error is raised (the
    overwrite-on-miss cache has no probe chain to run out of).  After every
    level the re-balancing leaves each shard within its threshold of an even
    split (1 % of the level over the shards + 64 rows)."""
    g = GOLD[name]
    fpl = (g["distinct"] * 2).bit_length() - 3   # per shard: ~30-40 % load over the 8 shards
    cfg = cfg_of(g, shards=8, chunk=4096, fpset_log2=fpl, mem_budget=24 << 30)
    with rtla.Checker(cfg) as ck:
        st = ck.init()
        while st == rtla.OK:
            st = ck.step()
            shares = json.loads(ck.device_info())["shard_frontier"]
            total = sum(shares)
            if st == rtla.OK:
                assert max(shares) <= total // 8 + 1 + 64 + total // 800, (len(ck.levels), shares)
        assert st == rtla.DONE
        info = json.loads(ck.device_info())
        assert info["sent_cache_slots_log2"] == fpl - 1 and info["rebalanced_rows"] > 0
        assert [[lv.new, lv.generated] for lv in ck.levels] == g["levels"]


@pytest.mark.parametrize("sent", [1, 0])
@pytest.mark.parametrize("shards", [2, 8])
@pytest.mark.parametrize("name", ["n3_v1_t2_l1_m1", "n3_v1_t2_l1_m1_sym", "n3_v1_t2_l1_m2"])
def test_virtual_shards_tiny_outbox_match_golden(monkeypatch, name, shards, sent):
    """Exchange rounds sized by the outbox (no chunk bound): with owner regions
    of only 4096 records (RTLA_OUTBOX_CAP), every big level runs many rounds,
    the level kernel's group guard stops it mid-level, and the records the
    groups in flight still queue past a region's end take the overflow list
    into the next round -- with and without the sent cache.  Golden counts
    and level contents."""
    virtual_shards_tiny_outbox_match_golden(monkeypatch, name, shards, sent)


@pytest.mark.parametrize("shards,sent", [(2, 1), (8, 0)])
def test_virtual_shards_tiny_outbox_match_golden_at_the_limits(monkeypatch, shards, sent):
    """The same with 3-bit terms (n2_v1_t5_l1_m1: the smallest limit model whose levels overflow the
    regions, and whose states spread evenly over 8 owners; its 1.3e6 states make the host digest of the
    levels most of a case's ~10 s)."""
    virtual_shards_tiny_outbox_match_golden(monkeypatch, "n2_v1_t5_l1_m1", shards, sent)


def virtual_shards_tiny_outbox_match_golden(monkeypatch, name, shards, sent):
    monkeypatch.setenv("RTLA_OUTBOX_CAP", "4096")
    monkeypatch.setenv("RTLA_SENT_CACHE", str(sent))
    g = GOLD[name]
    kw = dict(fpset_log2=max(16, (g["distinct"] * 2 // shards).bit_length()), mem_budget=24 << 30)
    want, digest = level_digests(g) if g["distinct"] < 3_000_000 else ([], None)  # (the big model: counts)
    with rtla.Checker(cfg_of(g, shards=shards, **kw)) as ck:
        info = json.loads(ck.device_info())
        assert info["outbox_records_per_owner"] == 4096 and (info["chunk"] == 0 or shards == 8)
        assert info["sent_cache_slots_log2"] == (info["fpset_slots_log2"] - 1 if sent else 0)
        st = ck.init()
        got = []
        while True:
            if len(got) < len(want):
                got.append("%016x" % digest(ck))
            if st != rtla.OK:
                break
            st = ck.step()
        assert [[lv.new, lv.generated] for lv in ck.levels] == g["levels"]
        assert got == want[:len(got)]
        info = json.loads(ck.device_info())
        assert info["exchange_rounds"] > len(g["levels"]) + 20, info  # (levels cut into several rounds)
        assert info["overflowed_records"] > 0, info


@pytest.mark.parametrize("shards", [2, 3, 8])
@pytest.mark.parametrize("name", ["n2_v2_t3_l2_m1", "n3_v1_t2_l1_m1", "n2_v1_t2_l1_m1_sym", "n2_v4_t2_l2_m1"])
def test_virtual_shards_over_rccl_match_golden(monkeypatch, name, shards):
    """The virtual-shard exchange through a one-rank RCCL communicator
    (RTLA_TRANSPORT=rccl): every fingerprint / answer / row transfer is an
    ncclSend/ncclRecv pair to self inside one group, the count and winner
    gathers are ncclAllGather, the level reductions ncclAllReduce -- the RCCL
    call sites of the multi-GPU path, executed on this GPU.  Golden per-level
    counts, as with device copies."""
    monkeypatch.setenv("RTLA_TRANSPORT", "rccl")
    g = GOLD[name]
    kw = small_kw(g)
    kw["mem_budget"] *= shards
    with rtla.Checker(cfg_of(g, shards=shards, chunk=512, **kw)) as ck:
        assert json.loads(ck.device_info())["transport"] == "rccl-local"
        st = ck.init()
        while st == rtla.OK:
            st = ck.step()
        assert [[lv.new, lv.generated] for lv in ck.levels] == g["levels"]
        assert ck.distinct == g["distinct"]


def test_virtual_shards_over_rccl_trace_and_contents(monkeypatch):
    """Through the one-rank RCCL communicator: level contents (text digests,
    whose cross-shard sum is an ncclAllReduce) and a counterexample trace whose
    parent records travel by ncclBroadcast."""
    monkeypatch.setenv("RTLA_TRANSPORT", "rccl")
    g = GOLD["n2_v2_t3_l2_m1"]
    kw = small_kw(g)
    kw["mem_budget"] *= 4
    got = []
    with rtla.Checker(cfg_of(g, shards=4, chunk=1000, **kw)) as ck:
        st = ck.init()
        while True:
            got.append("%016x" % ck.level_text_hash())
            if st != rtla.OK:
                break
            st = ck.step()
    assert got[:len(g["level_text_hash"])] == g["level_text_hash"]
    g = GOLD["n3_v1_t3_l1_m1_ntl"]
    kw = small_kw(g)
    kw["mem_budget"] *= 3
    res = rtla.check(cfg_of(g, shards=3, **kw))
    assert res.violation == "NoTwoLeaders" and len(res.trace) == g["depth"]
    walk = raft_cpu.Walk(raft_cpu.cfg_of(3, 1, 3, 1, 1, 1, ("NoTwoLeaders",)))
    for label, text in res.trace[1:]:
        assert text in [t for _, t in walk.successors()], label
        walk.goto(text)
    assert walk.invariants() & 1


def test_virtual_shards_level_contents():
    g = GOLD["n2_v2_t3_l2_m1"]
    kw = small_kw(g)
    kw["mem_budget"] *= 4
    cfg = cfg_of(g, shards=4, chunk=1000, **kw)
    got = []
    with rtla.Checker(cfg) as ck:
        st = ck.init()
        while True:
            got.append("%016x" % ck.level_text_hash())
            if st != rtla.OK:
                break
            st = ck.step()
    assert got[:len(g["level_text_hash"])] == g["level_text_hash"]


def test_virtual_shards_trace():
    g = GOLD["n3_v1_t3_l1_m1_ntl"]
    kw = small_kw(g)
    kw["mem_budget"] *= 4
    res = rtla.check(cfg_of(g, shards=4, **kw))
    assert res.violation == "NoTwoLeaders" and len(res.trace) == g["depth"]
    walk = raft_cpu.Walk(raft_cpu.cfg_of(3, 1, 3, 1, 1, 1, ("NoTwoLeaders",)))
    for label, text in res.trace[1:]:
        assert text in [t for _, t in walk.successors()], label
        walk.goto(text)
    assert walk.invariants() & 1


@pytest.mark.parametrize("shards", [1, 2])
def test_stored_fingerprints_equal_full_rehash(shards):
    """Every row the search stores carries the fingerprint derived
    incrementally from its parent; it must equal a from-scratch hash of the
    row (a wrong stored fingerprint silently breaks dedup at the next level)."""
    stored_fingerprints_equal_full_rehash("n2_v2_t3_l2_m1", shards)


@pytest.mark.parametrize("shards", [1, 2])
@pytest.mark.parametrize("name", LIMIT_MODELS)
def test_stored_fingerprints_equal_full_rehash_at_the_limits(name, shards):
    """The same with message counts up to 14 (and 15 out of the model) and with 2-bit values."""
    stored_fingerprints_equal_full_rehash(name, shards)


def stored_fingerprints_equal_full_rehash(name, shards):
    g = GOLD[name]
    kw = small_kw(g)
    kw["mem_budget"] *= shards
    cfg = cfg_of(g, shards=shards, chunk=512, **kw)
    with rtla.Checker(cfg) as ck:
        st = ck.init()
        level = 1
        while st == rtla.OK and level < 16:
            st = ck.step()
            level += 1
            rows = ck.frontier()
            bad = [r for r in rows if rtla.stored_fingerprint(r) != rtla.row_fingerprint(cfg, r)]
            assert not bad, "level %d: %d of %d rows carry a wrong fingerprint; first:\n%s" % (
                level, len(bad), len(rows), rtla.state_text(cfg, bad[0]))


# ---- checkpoint / recover (TLC -checkpoint / -recover, reference .gitignore:2) ----
@pytest.mark.parametrize("shards", [1, 2])
def test_checkpoint_recover_continues_identically(tmp_path, shards):
    checkpoint_recover_continues_identically(tmp_path, "n2_v2_t3_l2_m1", shards)


@pytest.mark.parametrize("shards", [1, 2])
@pytest.mark.parametrize("name", LIMIT_MODELS)
def test_checkpoint_recover_continues_identically_at_the_limits(tmp_path, name, shards):
    """The row format's limits through the checkpoint files."""
    checkpoint_recover_continues_identically(tmp_path, name, shards)


def checkpoint_recover_continues_identically(tmp_path, name, shards):
    g = GOLD[name]
    kw = small_kw(g)
    kw["mem_budget"] *= shards
    cfg = cfg_of(g, shards=shards, chunk=512, **kw)
    prefix = str(tmp_path / "ckpt")
    with rtla.Checker(cfg) as a:
        a.init()
        for _ in range(9):
            a.step()
        a.checkpoint(prefix)
        k = len(a.levels)
        a.run()
        tail_a = [[lv.new, lv.generated] for lv in a.levels[k:]]
        cov_a = a.coverage()
        tot_a = (a.distinct, a.generated)
    with rtla.Checker(cfg) as b:
        b.recover(prefix)
        b.run()
        assert [[lv.new, lv.generated] for lv in b.levels] == tail_a
        assert (b.distinct, b.generated) == tot_a == (g["distinct"], g["generated"])
        cov_b = b.coverage()
        # generated per action is deterministic; which action is credited with
        # a distinct state depends on which parent finds it first (as in TLC
        # with several workers), so only the distinct total is compared
        assert {k: v[0] for k, v in cov_b.items()} == {k: v[0] for k, v in cov_a.items()}
        assert sum(v[1] for v in cov_b.values()) == sum(v[1] for v in cov_a.values())


def test_recover_then_counterexample_trace(tmp_path):
    g = GOLD["n3_v1_t3_l1_m1_ntl"]
    cfg = cfg_of(g, **small_kw(g))
    prefix = str(tmp_path / "ckpt")
    with rtla.Checker(cfg) as a:
        a.init()
        for _ in range(10):
            a.step()
        a.checkpoint(prefix)
    with rtla.Checker(cfg) as b:
        b.recover(prefix)
        assert b.run() == rtla.VIOLATION
        tr = b.trace()
    assert len(tr) == g["trace_len"]
    walk = raft_cpu.Walk(raft_cpu.cfg_of(3, 1, 3, 1, 1, 1, ("NoTwoLeaders",)))
    assert walk.text() == tr[0][1]
    for label, text in tr[1:]:
        assert text in [t for _, t in walk.successors()], label
        walk.goto(text)
    assert walk.invariants() & 1


def test_recover_rejects_other_configuration(tmp_path):
    g = GOLD["n2_v2_t3_l2_m1"]
    prefix = str(tmp_path / "ckpt")
    with rtla.Checker(cfg_of(g, **small_kw(g))) as a:
        a.init()
        a.step()
        a.checkpoint(prefix)
    other = GOLD["n2_v1_t3_l1_m1"]
    kw = small_kw(g)
    with rtla.Checker(cfg_of(other, **kw)) as b:
        with pytest.raises(rtla.RtlaError):
            b.recover(prefix)


# ---- SYMMETRY Permutations(Server) (specs/MC.tla Perms) ----
# The golden orbit counts come from the C oracle (least serialisation over
# all server permutations) and, for N=2, the value oracle's orbit BFS; the
# GPU keys the seen set by the least fingerprint over the permutations that
# sort the servers by signature (rtla_model.h sym_key), so agreement checks
# the orbit relation, not a shared implementation.  N = 4 and N = 5
# (BASELINE configs[3]) are covered by the prefix fixtures above.
SYM_SMALL = sorted(k for k in SMALL if GOLD[k].get("symmetry"))


@pytest.mark.parametrize("shards", [2, 3])
@pytest.mark.parametrize("name", SYM_SMALL)
def test_symmetry_virtual_shards_match_golden(name, shards):
    """Orbit-key ownership: the exchange protocol must find each orbit once."""
    g = GOLD[name]
    kw = small_kw(g)
    kw["mem_budget"] *= shards
    res = rtla.check(cfg_of(g, shards=shards, chunk=700, **kw), trace=False)
    assert [[lv.new, lv.generated] for lv in res.levels] == g["levels"]
    assert (res.distinct, res.generated, res.depth) == (g["distinct"], g["generated"], g["depth"])


@pytest.mark.parametrize("shards", [1, 2])
def test_symmetry_counterexample_trace(shards):
    """Same shortest depth as without symmetry; the trace is made of the
    states actually generated, so it replays step by step in the oracle."""
    g = GOLD["n3_v1_t3_l1_m1_ntl_sym"]
    kw = small_kw(g)
    kw["mem_budget"] *= shards
    res = rtla.check(cfg_of(g, shards=shards, **kw))
    assert res.violation == "NoTwoLeaders"
    assert len(res.trace) == g["depth"] == GOLD["n3_v1_t3_l1_m1_ntl"]["depth"]
    walk = raft_cpu.Walk(raft_cpu.cfg_of(3, 1, 3, 1, 1, 1, ("NoTwoLeaders",)))
    assert walk.text() == res.trace[0][1]
    for label, text in res.trace[1:]:
        assert text in [t for _, t in walk.successors()], label
        walk.goto(text)
    assert walk.invariants() & 1


def test_symmetry_stored_rows_are_generated_states():
    """Rows keep the state that was generated (not a canonical image) with
    its own fingerprint; each level holds one state per new orbit."""
    g = GOLD["n3_v1_t2_l1_m1_sym"]
    cfg = cfg_of(g, **small_kw(g))
    with rtla.Checker(cfg) as ck:
        st = ck.init()
        level = 1
        while st == rtla.OK and level < 14:
            st = ck.step()
            level += 1
            rows = ck.frontier()
            assert len(rows) == g["levels"][level - 1][0]
            assert all(rtla.stored_fingerprint(r) == rtla.row_fingerprint(cfg, r) for r in rows)
            assert len({rtla.state_text(cfg, r) for r in rows}) == len(rows)


@pytest.mark.parametrize("name", ["n2_v2_t3_l2_m1", "n3_v1_t2_l1_m1_sym", "n1_v1_t2_l1_c14", "n2_v4_t2_l2_m1_sym"])
def test_wave_kernel_matches_golden(name):
    """The wave-per-state k_expand (the fallback for rows too wide for the
    compacting kernel), forced with RTLA_XFLAGS=2048 in a child process (the
    flag is read once), with and without symmetry."""
    import subprocess
    import sys
    code = ("import json, rtla, sys; g = json.load(open(sys.argv[1]))[sys.argv[2]];"
            "r = rtla.check(rtla.Config(g['n_server'], g['n_value'], g['max_term'], g['max_log'], g['max_copies'],"
            " g['max_msgs'], tuple(g['invariants']), fpset_log2=22, mem_budget=1 << 30,"
            " symmetry=g.get('symmetry', False)), trace=False);"
            "assert [[lv.new, lv.generated] for lv in r.levels] == g['levels'], 'levels differ';"
            "assert (r.distinct, r.generated, r.depth) == (g['distinct'], g['generated'], g['depth']);"
            "print('ok', r.distinct)")
    env = dict(os.environ, RTLA_XFLAGS="2048",
               PYTHONPATH=os.pathsep.join([os.path.join(os.path.dirname(__file__), "..", "raft-tla_amd"),
                                           os.environ.get("PYTHONPATH", "")]))
    out = subprocess.run([sys.executable, "-c", code, os.path.join(os.path.dirname(__file__), "golden",
                                                                   "bfs_counts.json"), name],
                         env=env, capture_output=True, text=True, timeout=100)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout + out.stderr


def test_wave_batch_kernel_matches_host_model(tmp_path):
    """k_expand_batch (the parity seam and trace replay of the wave-per-state
    path, RTLA_XFLAGS=2048 in a child process) against the host model on
    synthetic rows that make it stage a partial 16-row batch after a full one
    and walk a second 64-candidate chunk; and the counterexample trace it
    replays is one the default kernel computes too (see below)."""
    import dataclasses
    import subprocess
    import sys
    import hostmodel
    cfg = rtla.Config(**SYNTH)
    N, V, K = cfg.n_server, cfg.n_value, cfg.bag_cap
    fixed = 4 * N + 2 * N * N + N * V  # instances before Receive; then K Receive, K Duplicate, K Drop slots
    assert rtla.action_name(cfg, fixed - 1, 6).startswith("AppendEntries")
    assert rtla.action_name(cfg, fixed + 2 * K, 6) == "DropMessage" == rtla.action_name(cfg, fixed + 3 * K - 1, 6)
    rows = rtla.random_rows(cfg, 0, 40, pool=40)
    ref = hostmodel.expand(cfg, rows, rtla.row_words(cfg))
    # enabled successors per (input, 64-candidate chunk): the kernel lists the fixed instances, then
    # Receive / Duplicate / Drop over the nmsg used slots (every used slot has its Drop successor)
    insts = {}
    for k, inst, _, _, _ in ref:
        insts.setdefault(k, []).append(inst)
    per_chunk = {}
    for k, ii in insts.items():
        nmsg = sum(i >= fixed + 2 * K for i in ii)
        for i in ii:
            q = i if i < fixed else fixed + (i - fixed) // K * nmsg + (i - fixed) % K
            per_chunk[k, q // 64] = per_chunk.get((k, q // 64), 0) + 1
    assert any(n > 16 and n % 16 for n in per_chunk.values()), "no partial staging batch after a full one"
    assert any(c == 1 for _, c in per_chunk), "no input with more than 64 candidates"
    assert any(n <= 16 for n in per_chunk.values())

    g = GOLD["n3_v1_t3_l1_m1_ntl"]
    job = tmp_path / "job.json"
    job.write_text(json.dumps({"synth": dataclasses.asdict(cfg), "rows": rows,
                               "model": dataclasses.asdict(cfg_of(g, **small_kw(g)))}))
    code = ("import json, rtla, sys; a = json.load(open(sys.argv[1]));"
            "mk = lambda d: rtla.Config(**dict(d, invariants=tuple(d['invariants'])));"
            "succ = rtla.expand_batch(mk(a['synth']), a['rows']);"
            "res = rtla.check(mk(a['model']), trace=True);"
            "json.dump({'succ': succ, 'violation': res.violation, 'trace': res.trace}, sys.stdout)")
    env = dict(os.environ, RTLA_XFLAGS="2048",
               PYTHONPATH=os.pathsep.join([os.path.join(os.path.dirname(__file__), "..", "raft-tla_amd"),
                                           os.environ.get("PYTHONPATH", "")]))
    out = subprocess.run([sys.executable, "-c", code, str(job)], env=env, capture_output=True, text=True, timeout=100)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = json.loads(out.stdout)
    assert [tuple(t) for t in got["succ"]] == ref  # input, instance, sub, in_model, row words
    # Which counterexample a search reports is a race (the first violation claimed, the first parent to
    # reach a state: the wave kernel's trace differed from the default kernel's at step 1 in one run and
    # at step 2 in another, on the library before and after the kernel-header split alike), so the two
    # traces are compared as what they must both be: shortest counterexamples of the same invariant, the
    # child's replayed step by step on the default kernel -- every state and label it reports is the one
    # the level kernel computes for that action from the state before.
    want = _ntl_check()
    assert got["violation"] == want.violation == "NoTwoLeaders"
    trace = [tuple(t) for t in got["trace"]]
    assert len(trace) == len(want.trace) == g["depth"] and trace[0] == tuple(want.trace[0])
    mcfg = cfg_of(g, **small_kw(g))
    row = rtla.init_row(mcfg)
    for label, text in trace[1:]:
        nxt = [(rtla.action_name(mcfg, inst, sub), r) for _, inst, sub, _, r in rtla.expand_batch(mcfg, [row])
               if rtla.state_text(mcfg, r) == text]
        assert label in [n for n, _ in nxt], label
        row = nxt[0][1]
    assert rtla.invariants_violated(mcfg, row) & rtla.INV_BITS["NoTwoLeaders"]


# ---- capacities: the row arena as a ring, overflow is an error, never truncation ----
def _round64(n):
    return (n + 63) // 64 * 64


@pytest.mark.parametrize("shards", [1, 2])
def test_ring_arena_wraps_and_matches_golden(shards):
    """A frontier arena barely larger than the biggest (current + next) level
    pair: every level wraps around the arena at a different offset; counts and
    level contents must still be the oracle's."""
    ring_arena_wraps_and_matches_golden("n2_v2_t3_l2_m1", shards)


@pytest.mark.parametrize("shards", [1, 2])
def test_ring_arena_wraps_and_matches_golden_at_the_limits(shards):
    """The same with 2-bit values (n2_v4_t2_l2_m1)."""
    ring_arena_wraps_and_matches_golden("n2_v4_t2_l2_m1", shards)


def ring_arena_wraps_and_matches_golden(name, shards):
    g = GOLD[name]
    x = [n for n, _ in g["levels"]]
    # multi-shard: each shard holds about 1/shards of a level (plus skew)
    need = max(_round64(x[i]) + x[i + 1] for i in range(len(x) - 1))
    cap = _round64(need // shards + (need // shards) // 4 + 128) if shards > 1 else _round64(need)
    kw = small_kw(g)
    kw["mem_budget"] *= shards
    cfg = cfg_of(g, frontier_cap=cap, shards=shards, chunk=1024, **kw)
    got = []
    with rtla.Checker(cfg) as ck:
        assert '"frontier_cap": %d' % cap in ck.device_info()
        st = ck.init()
        while True:
            got.append("%016x" % ck.level_text_hash())
            if st != rtla.OK:
                break
            st = ck.step()
        assert [[lv.new, lv.generated] for lv in ck.levels] == g["levels"]
    assert got[:len(g["level_text_hash"])] == g["level_text_hash"]


def test_frontier_overflow_is_an_error():
    g = GOLD["n2_v2_t3_l2_m1"]
    cfg = cfg_of(g, frontier_cap=4096, **small_kw(g))
    with rtla.Checker(cfg) as ck:
        with pytest.raises(rtla.RtlaError) as e:
            ck.run()
        assert e.value.status == -3 and e.value.flags & 4
        done = [[lv.new, lv.generated] for lv in ck.levels]
        assert done == g["levels"][:len(done)] and len(done) < len(g["levels"])


def test_bag_overflow_is_an_error():
    """bag_cap = 2 on a model whose states hold 3 distinct messages: the
    kernel raises RTLA_CAP_ROW (rtla_step -> -3), it never truncates."""
    g = GOLD["n3_v1_t2_l1_m1"]
    cfg = rtla.Config(3, 1, 2, 1, 1, 0, ("NoTwoLeaders",), bag_cap=2, fpset_log2=22, mem_budget=1 << 30)
    with rtla.Checker(cfg) as ck:
        with pytest.raises(rtla.RtlaError) as e:
            ck.run()
        assert e.value.status == -3 and e.value.flags & 2
    # the oracle agrees that 3 messages are reachable on that model
    r = raft_cpu.bfs(raft_cpu.cfg_of(3, 1, 2, 1, 1, 0, ("NoTwoLeaders",), max_distinct=100000), threads=4)
    assert r["max_msgs"] >= 3
    del g


# ---- the TLC-style command line on the GPU (reference boundary: raft.cfg, .vscode/settings.json:5) ----
# rtla's coverage codes -> the oracle's action families (oracle/raft_cpu.c A_*)
COVER_TO_ORACLE = {"Restart": 0, "Timeout": 1, "RequestVote": 2, "BecomeLeader": 3, "ClientRequest": 4,
                   "AdvanceCommitIndex": 5, "AppendEntries": 6, "UpdateTerm": 7, "HandleRequestVoteRequest": 8,
                   "HandleRequestVoteResponse": 9, "HandleAppendEntriesRequest": 10,
                   "HandleAppendEntriesResponse": 11, "DropStaleResponse": 12, "DuplicateMessage": 13,
                   "DropMessage": 14}


def _oracle_coverage(g):
    r = raft_cpu.bfs(raft_cpu.cfg_of(g["n_server"], g["n_value"], g["max_term"], g["max_log"], g["max_copies"],
                                     g["max_msgs"], tuple(g["invariants"])), threads=8)
    return r["coverage"]


@pytest.mark.parametrize("name", ["n2_v2_t3_l2_m1", "n2_v1_t2_l1_c2_m2", "n3_v1_t2_l1_m1", "n2_v1_t2_l1_c3_m3",
                                  "n1_v1_t2_l1_c14"])
def test_coverage_per_action_matches_oracle(name):
    """-coverage 1 (.vscode/settings.json:5): states generated per action of
    Next, Receive split by handler, equal the oracle's per-action counts."""
    g = GOLD[name]
    res = rtla.check(cfg_of(g, **small_kw(g)), trace=False)
    ref = _oracle_coverage(g)
    got = {k: res.coverage[k][0] for k in COVER_TO_ORACLE}
    assert got == {k: ref[v] for k, v in COVER_TO_ORACLE.items()}
    assert res.coverage["Receive"] == (0, 0)
    assert sum(v[1] for v in res.coverage.values()) == res.distinct - 1


def test_cli_model_check_matches_golden(tmp_path):
    import re
    from cli_util import model_dir, run
    g = GOLD["n3_v1_t2_l1_m1"]
    tla, cfg = model_dir(str(tmp_path), 3, 1, 2, 1, 1, 1, ["NoTwoLeaders"])
    r = run(["-skip-spec-check", "-coverage", "1", "-fpbits", "23", "-membudget", str(1 << 30), "-config", cfg, tla])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Model checking completed. No error has been found." in r.stdout
    m = re.search(r"^(\d+) states generated, (\d+) distinct states found, 0 states left on queue\.$", r.stdout, re.M)
    assert m and (int(m.group(1)), int(m.group(2))) == (g["generated"], g["distinct"]), r.stdout
    assert "The depth of the complete state graph search is %d." % g["depth"] in r.stdout
    cov = dict((k, int(gen)) for k, d, gen in re.findall(r"^<(\w+) of module raft>: (\d+):(\d+)$", r.stdout, re.M))
    ref = _oracle_coverage(g)
    assert cov == {k: ref[v] for k, v in COVER_TO_ORACLE.items()}


def test_cli_counterexample_and_exit_code(tmp_path):
    import re
    from cli_util import model_dir, run
    g = GOLD["n3_v1_t3_l1_m1_ntl"]
    tla, cfg = model_dir(str(tmp_path), 3, 1, 3, 1, 1, 1, ["NoTwoLeaders"])
    r = run(["-skip-spec-check", "-fpbits", "23", "-membudget", str(1 << 30), "-config", cfg, tla])
    assert r.returncode == 12, r.stdout + r.stderr
    assert "Error: Invariant NoTwoLeaders is violated." in r.stdout
    states = re.findall(r"^State (\d+): <(.*)>$", r.stdout, re.M)
    assert [int(k) for k, _ in states] == list(range(1, g["trace_len"] + 1))
    assert states[0][1] == "Initial predicate"
    # model values of the cfg, not the row printer's s1.. names
    assert "r1" in r.stdout and '"Leader"' in r.stdout


# ---- synthetic microbench (BASELINE configs[4]): random valid states through Next + fingerprint + dedup ----
SYNTH = dict(n_server=3, n_value=2, max_term=4, max_log=3, max_copies=2, max_msgs=0,
             invariants=("ElectionSafety", "LogMatching"), bag_cap=12)


def test_synthetic_states_successors_match_value_oracle():
    """Next on arbitrary (random, unreachable) packed states: the GPU's
    successor multiset -- texts and in-model flags -- equals the value
    oracle's (raft_values.next_states over the parsed state), state by state."""
    import collections
    import tla_text
    cfg = rtla.Config(**SYNTH)
    vc = rv.Cfg(3, 2, 4, 3, 2, ("ElectionSafety", "LogMatching"), 0)
    rows = rtla.random_rows(cfg, 0, 150, pool=40)
    by = collections.defaultdict(list)
    for k, inst, sub, im, r in rtla.expand_batch(cfg, rows):
        by[k].append((im, rtla.state_text(cfg, r)))
    for k, r in enumerate(rows):
        s = tla_text.parse_state(vc, rtla.state_text(cfg, r))
        ref = sorted((rv.in_model(vc, t), rv.state_text(vc, t)) for _, t in rv.next_states(vc, s))
        assert sorted(by[k]) == ref, "input state %d" % k


def test_synthetic_step_dedup_counts():
    """rtla_synthetic_step (the dedup-only level kernel over device-generated
    states) against counts from the VALUE ORACLE over the same rows (each
    input parsed from its text, raft_values.next_states): generated
    successors, fingerprint-set probes (in-model successors that differ from
    their parent) and distinct new states, across two batches that share the
    fingerprint set."""
    import tla_text
    cfg = rtla.Config(**SYNTH, fpset_log2=22, mem_budget=1 << 30)
    vc = rv.Cfg(3, 2, 4, 3, 2, ("ElectionSafety", "LogMatching"), 0)
    n, pool = 320, 60
    rows = rtla.random_rows(cfg, 0, 2 * n, pool=pool)
    seen = set()
    expect = []
    for b in range(2):
        gen = probes = 0
        before = len(seen)
        for r in rows[b * n:(b + 1) * n]:
            text = rtla.state_text(cfg, r)
            for _, t in rv.next_states(vc, tla_text.parse_state(vc, text)):
                gen += 1
                tt = rv.state_text(vc, t)
                if rv.in_model(vc, t) and tt != text:
                    probes += 1
                    seen.add(tt)
        expect.append((gen, probes, len(seen) - before))
    with rtla.Checker(cfg) as ck:
        got = [ck.synthetic_step(b * n, n, pool) for b in range(2)]
    assert [(lv.generated, lv.probes, lv.new) for lv in got] == expect


@pytest.mark.parametrize("name,world", [("n3_v1_t2_l1_m1", 2), ("n3_v1_t2_l1_m1", 3), ("n2_v1_t2_l1_m1_sym", 2),
                                        ("n3_v1_t3_l1_m1_ntl", 2), ("n3_v1_t2_l1_m1", 8),
                                        ("n3_v1_t2_l1_m1_sym", 8), ("n3_v1_t3_l1_m1_ntl", 8)])
def test_ranks_over_shm_transport_match_golden(tmp_path, name, world):
    """The world > 1 protocol (one process per rank: count all-gathers,
    all-to-all-v of fingerprints / answers / rows, reductions, the trace's
    cross-rank broadcasts) over the shared-memory transport, several ranks on
    this one GPU (RCCL refuses two ranks per device): every rank reports the
    golden per-level counts, and a counterexample trace of the golden length,
    the same on every rank.  world = 8 (1, 2, 4 and 8 ranks): the
    8-rank control flow as processes -- open-time agreement over 8 ranks,
    level-end re-balancing plans across 8 ranks (rows do move), a symmetric
    model and a counterexample trace walked across ranks."""
    import subprocess
    import sys
    g = GOLD[name]
    # the transport holds world^2 message slots in /dev/shm
    env = dict(os.environ, RTLA_TRANSPORT="shm", RTLA_SHM_SLOT_MB="32" if world <= 3 else "8")
    idfile = str(tmp_path / "comm_id")
    helper = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rccl_pair.py")
    procs = [subprocess.Popen([sys.executable, helper, str(r), str(world), idfile, name], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(world)]
    outs = []
    for p in procs:
        o, e = p.communicate(timeout=240)
        assert p.returncode == 0, e[-2000:]
        outs.append(json.loads(o.strip().splitlines()[-1]))
    for o in outs:
        assert o["levels"] == g["levels"], "rank %d" % o["rank"]
        assert (o["distinct"], o["generated"]) == (g["distinct"], g["generated"])
        assert '"world": %d' % world in o["info"]
    assert sorted(o["rank"] for o in outs) == list(range(world))
    if world == 8 and not g["violated"]:
        assert sum(json.loads(o["info"])["rebalanced_rows"] for o in outs) > 0
    if g["violated"]:
        assert all(o["status"] == rtla.VIOLATION for o in outs)
        assert all(len(o["trace"]) == g["trace_len"] for o in outs)
        assert all(o["trace"] == outs[0]["trace"] for o in outs)


def test_ranks_with_different_budgets_agree_on_exchange_sizes(tmp_path):
    """Ranks whose own sizing differs (different memory budgets, and a
    re-balancing staging of 16 rows on rank 0 against 40 on rank 1) agree on
    one set of exchange sizes in rtla_open (min over the ranks), so the
    level-end re-balancing moves -- here many times the staging, in
    sub-rounds -- post matching sends and receives: golden counts on every
    rank, no hang (rows_cap from each rank's own budget)."""
    import subprocess
    import sys
    name, world = "n3_v1_t2_l1_m1", 2
    g = GOLD[name]
    idfile = str(tmp_path / "comm_id")
    helper = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rccl_pair.py")
    procs = []
    for r in range(world):
        env = dict(os.environ, RTLA_TRANSPORT="shm", RTLA_SHM_SLOT_MB="32", RTLA_ROWS_CAP=str(16 + 24 * r),
                   RCCL_PAIR_BUDGET_STEP=str(3 << 28))
        procs.append(subprocess.Popen([sys.executable, helper, str(r), str(world), idfile, name], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = []
    for p in procs:
        o, e = p.communicate(timeout=240)
        assert p.returncode == 0, e[-2000:]
        outs.append(json.loads(o.strip().splitlines()[-1]))
    moved = 0
    for o in outs:
        assert o["levels"] == g["levels"], "rank %d" % o["rank"]
        assert (o["distinct"], o["generated"]) == (g["distinct"], g["generated"])
        moved += json.loads(o["info"])["rebalanced_rows"]
    assert moved > 4 * 16  # the re-balancing ran, in several sub-rounds of the agreed 16 rows


def test_ranks_recover_fails_on_every_rank(tmp_path):
    """One rank's checkpoint file is missing: rtla_recover fails on EVERY rank
    and returns promptly -- the local failure travels in the cross-rank
    consistency reduction instead of leaving the other ranks waiting in it."""
    import subprocess
    import sys
    env = dict(os.environ, RTLA_TRANSPORT="shm", RTLA_SHM_SLOT_MB="32", RCCL_PAIR_MODE="recover_missing")
    idfile, prefix = str(tmp_path / "comm_id"), str(tmp_path / "ckpt")
    helper = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rccl_pair.py")
    procs = [subprocess.Popen([sys.executable, helper, str(r), "2", idfile, "n3_v1_t2_l1_m1", prefix], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(2)]
    outs = []
    for p in procs:
        o, e = p.communicate(timeout=120)
        assert p.returncode == 0, e[-2000:]
        outs.append(json.loads(o.strip().splitlines()[-1]))
    assert [o["recover"] for o in outs] == [-5, -6]  # the other rank's failure / the missing file
    assert all(o["seconds"] < 30 for o in outs)


@pytest.mark.parametrize("where,name", [("coverage", "n3_v1_t2_l1_m1"), ("trace", "n3_v1_t3_l1_m1_ntl"),
                                        ("exchange", "n3_v1_t2_l1_m1"), ("launch", "n3_v1_t2_l1_m1")])
def test_ranks_local_failure_fails_every_rank(tmp_path, where, name):
    """One rank's local work fails (RTLA_FAULT=<where>:1) inside a collective
    entry point -- the coverage read-back, a trace record, a level's exchange
    rounds, an actual level-kernel launch that the HIP runtime refuses (ADVICE
    r5: a HIP error inside the rounds must not return before the peers'
    collectives): every rank returns an error from that call, promptly,
    because the failure travels in the call's reductions and count gathers
    (no rank is left waiting in a collective the failed rank never reaches)."""
    import subprocess
    import sys
    env = dict(os.environ, RTLA_TRANSPORT="shm", RTLA_SHM_SLOT_MB="32", RCCL_PAIR_MODE="fault_" + where,
               RTLA_FAULT="%s:1" % where)
    idfile = str(tmp_path / "comm_id")
    helper = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rccl_pair.py")
    procs = [subprocess.Popen([sys.executable, helper, str(r), "2", idfile, name], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(2)]
    outs = []
    for p in procs:
        o, e = p.communicate(timeout=120)
        assert p.returncode == 0, e[-2000:]
        outs.append(json.loads(o.strip().splitlines()[-1]))
    if where in ("exchange", "launch"):  # the level's reduction fails every rank: the local failure's status
        assert [o["step"] for o in outs] == [rtla.E_HIP, rtla.E_HIP], outs
    else:
        assert outs[0]["step"] == outs[1]["step"] == (rtla.VIOLATION if where == "trace" else rtla.DONE)
        assert [o[where] for o in outs] == [rtla.E_COMM, rtla.E_HIP], outs  # the peer's failure / its own
    assert all(o["seconds"] < 30 for o in outs)


def test_synthetic_resident_dedup_matches_step():
    """bench.py's configs[4] path: inputs generated into the row arena once
    (rtla_synthetic_generate), then dedup passes over resident row ranges
    (rtla_synthetic_dedup) -- the same counts as generate-and-dedup steps."""
    cfg = rtla.Config(**SYNTH, fpset_log2=22, mem_budget=1 << 30)
    n, pool = 2560, 400  # range starts are multiples of 64 (level-kernel groups)
    with rtla.Checker(cfg) as ck:
        want = [ck.synthetic_step(b * n, n, pool) for b in range(2)]
        ck.reset()
        ck.synthetic_generate(n, n, pool, at=n)  # out of order: rows land where `at` says
        ck.synthetic_generate(0, n, pool, at=0)
        got = [ck.synthetic_dedup(0, n), ck.synthetic_dedup(n, 2 * n)]
    assert [(lv.frontier, lv.generated, lv.probes, lv.new) for lv in got] == \
        [(lv.frontier, lv.generated, lv.probes, lv.new) for lv in want]
    with pytest.raises(rtla.RtlaError):
        with rtla.Checker(cfg) as ck:
            ck.synthetic_dedup(10, n)  # not a group boundary


@pytest.mark.parametrize("gpus", [2, 4])
def test_bench_gpus_over_shm_matches_golden(gpus):
    """The driver's multi-GPU entry point itself: `bench.py --gpus N` (N
    ranks under torch.distributed.run, gloo control plane, the checker's own
    exchange -- here over the shared-memory transport, every rank on this
    GPU) exhausts a model with the golden counts and prints one JSON line.
    (N = 8 is the driver's own scaling run; 8 rank processes of the checker
    run in test_ranks_over_shm_transport_match_golden.)"""
    import subprocess
    import sys
    g = GOLD["n3_v1_t2_l1_m1"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RTLA_TRANSPORT="shm", RTLA_SHM_SLOT_MB="32" if gpus <= 2 else "8")
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", str(gpus), "--workload",
                        "raft3_v1_t2_l1_m1", "--mem-budget", "8", "--fpset-log2", "24", "--no-cpu", "--steps", "1",
                        "--warmup", "0"],
                       env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    r = json.loads(lines[0])
    c = r["config"]
    assert r["n_gpus"] == gpus and c["parallelism"] == "fp-sharded%d" % gpus and c["exhausted"]
    assert (c["distinct"], c["generated"], c["depth"]) == (g["distinct"], g["generated"], g["depth"])


def test_bench_plain_run_dumps_the_last_steps_levels(tmp_path):
    """A plain `bench.py` run (no --full) times its steps and nothing else --
    no CPU baseline, no secondary line, no live calibration -- and
    --dump-outputs writes the level counts the last timed step returned:
    levels.npy (level, frontier, new, generated, probes) and totals.npy
    (distinct, generated, depth), here the golden counts of an exhausted model."""
    import subprocess
    import sys

    import numpy as np
    g = GOLD["n3_v1_t2_l1_m1"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--workload",
                        "raft3_v1_t2_l1_m1", "--mem-budget", "8", "--fpset-log2", "24", "--steps", "2",
                        "--warmup", "0", "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["steps"] == 2 and r["ms_per_step"] > 0 and r["config"]["exhausted"]
    assert r["value"] == pytest.approx(g["distinct"] / (r["ms_per_step"] / 1e3))
    assert r["cpu_baseline"] is None and "exhaust" not in r and r["roofline"]["random_access"]["calibration"] is None
    assert sorted(os.listdir(tmp_path / "out")) == ["levels.npy", "totals.npy"]
    lv = np.load(tmp_path / "out" / "levels.npy")
    assert lv.dtype == np.float64 and lv.shape == (len(g["levels"]), 5)
    assert lv[:, 0].tolist() == list(range(1, len(g["levels"]) + 1))
    assert lv[:, 2:4].tolist() == g["levels"]
    assert lv[1:, 1].tolist() == lv[:-1, 2].tolist()  # a level's frontier is the level before it
    assert np.load(tmp_path / "out" / "totals.npy").tolist() == [g["distinct"], g["generated"], g["depth"]]
