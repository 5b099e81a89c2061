"""The level kernel's row tile load and its reads of the parent rows (rtla_klevel.h), on every instantiation.

A group's rows come into LDS as 16-byte pieces, one per lane and step, and a tail of one to three words when
the tile's word count is no multiple of 4; the evaluation and the row build then read each lane's parent row
from that tile.  A piece not loaded, loaded to the wrong place or read before it landed leaves a row of the
tile stale or torn: its successors are then another state's, and the step's counts or new states differ.

One seeded BFS step (Checker.init(roots) + step()) against the value oracle (tests/seedref.py: raft_values'
Next and StateConstraint in Python, no product code on the reference side): the generated count, the new-state
count and the set of new states.

Root counts: 1 (a lone row), 2 and 3 (with odd W: tails of 2, 1, 3 words), 63 / 64 / 65 (a last step with few
lanes, exactly one tile of 64, a second group of one row), 127 / 128 / 129 (the same one group further).  For
the 32- and 16-state groups the same counts fall on group boundaries too (64 = 2 x 32 = 4 x 16).
Kernel paths: the compiled-in CFG2 (W = 43, groups of 64), CFG1, EXHAUST (narrow rows, 4 waves/SIMD), SYNTH
(groups of 32), CFG4 under SYMMETRY (groups of 16 as compiled in; roots one per orbit), the CFG2 configuration
forced onto the run-time-layout kernel (RTLA_XFLAGS=4096, one child process) and on two shards (MULTI).
Which kernel ran is not observable through the ABI; each case asserts the rule that chooses it, as
tests/test_seed_gpu.py does.

The roots are the first rows of the sample that are quiet for the layout's compiled-in mask; over the 129 of
them every action family of Next and every server index as the changed server occurs among the oracle's
successors (test_roots_cover_every_family_and_server, no GPU needed): a parent word served from the wrong
server's record cannot go unnoticed.
"""
import collections
import functools
import json
import os

import pytest

import limits
import raft_values as rv
import rtla
import seedref as sr

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "bfs_counts.json")))
MEM = dict(fpset_log2=20, mem_budget=1 << 29)
COUNTS = (1, 2, 3, 63, 64, 65, 127, 128, 129)
FAMILIES = ("Restart", "Timeout", "RequestVote", "BecomeLeader", "ClientRequest", "AdvanceCommitIndex",
            "AppendEntries", "Receive", "DuplicateMessage", "DropMessage")

# path: (layout, symmetry, shards, RTLA_XFLAGS of the process that runs it, the level kernel by limits.kernel_of)
PATHS = {
    "cfg2": (sr.CFG2, False, 0, 0, "compact64"),
    "cfg1": (sr.CFG1, False, 0, 0, "compact64"),
    "exhaust": (sr.EXHAUST, False, 0, 0, "compact64"),
    "synth": (sr.SYNTH, False, 0, 0, "compact32"),
    "cfg4_sym": (sr.CFG4, True, 0, 0, "compact32"),  # (the rule's group; the compiled-in CFG4 runs 16-state groups)
    "cfg2_runtime": (sr.CFG2, False, 0, 4096, "compact64"),
    "cfg2_shards2": (sr.CFG2, False, 2, 0, "compact64"),
}


def mask_names(layout):
    return sr.COMPILED_MASK.get(layout, ())  # CFG4 is compiled in without an invariant


def path_cfg(path):
    layout, sym, shards, _, _ = PATHS[path]
    kw = dict(MEM, mem_budget=MEM["mem_budget"] * max(1, shards))
    return sr.configs(*layout, mask_names(layout), shards=shards, symmetry=sym, **kw)[0]


@functools.lru_cache(maxsize=None)
def path_roots(path):
    """(sample, the 129 roots): the first rows quiet for the compiled-in mask (SYMMETRY: one per orbit)."""
    layout, sym = PATHS[path][:2]
    smp = sr.sample(*layout, sr.ROWS[layout])
    quiet = smp.quiet(path_cfg(path).inv_mask)
    if sym:
        quiet = sr.one_per_orbit(smp, quiet)
    assert len(quiet) >= COUNTS[-1]
    return smp, tuple(quiet[:COUNTS[-1]])


# ---- the oracle's side

def changed_servers(s, t):
    """The servers whose own variables (raft.tla's functions on Server) differ between s and t."""
    first = rv.IX["currentTerm"]
    return {i for i in range(len(s[first])) if any(s[v][i] != t[v][i] for v in range(first, len(rv.VARS)))}


def coverage(smp, roots):
    """(family -> successors, server -> successors that change it) over the oracle's successors of the roots."""
    fam, srv = collections.Counter(), collections.Counter()
    for k in roots:
        for u in smp.succ[k]:
            fam[u.label.split("(")[0].split(":")[0]] += 1
            for i in changed_servers(smp.states[k], u.state):
                srv[i] += 1
    return fam, srv


def server_profile(s):
    """A function of s's orbit under Permutations(Server), cheap: what each server holds with the server names
    dropped, as a sorted list, and the sizes of the rest.  States of one orbit share it."""
    ix = rv.IX

    def nameless(m):
        return repr(sorted((k, repr(v)) for k, v in m.items() if k not in ("msource", "mdest")))

    def other(i, j):
        return "Nil" if j == rv.NIL else "self" if j == i else "other"

    sent, recv = collections.defaultdict(list), collections.defaultdict(list)
    for m, c in s[ix["messages"]].items():
        sent[m["msource"]].append((nameless(m), c))
        recv[m["mdest"]].append((nameless(m), c))
    per = sorted(repr((s[ix["currentTerm"]][i], s[ix["state"]][i], s[ix["log"]][i], s[ix["commitIndex"]][i],
                       other(i, s[ix["votedFor"]][i]), sorted(other(i, j) for j in s[ix["votesResponded"]][i]),
                       sorted(other(i, j) for j in s[ix["votesGranted"]][i]),
                       sorted(repr(v) for _, v in s[ix["voterLog"]][i].items()),
                       sorted(s[ix["nextIndex"]][i]), sorted(s[ix["matchIndex"]][i]), sorted(sent[i]), sorted(recv[i])))
                 for i in range(len(s[ix["state"]])))
    elec = sorted(repr((e["eterm"], e["elog"], len(e["evotes"]), sorted(repr(v) for _, v in e["evoterLog"].items())))
                  for e in s[ix["elections"]])
    return tuple(per), tuple(elec), s[ix["allLogs"]]


class Orbits:
    """Orbit classes of value-oracle states: states of one orbit share server_profile, so only states whose
    profile another state shares are told apart by the brute force over all N! images (raft_values.orbit_key,
    tens of milliseconds a state at N = 5)."""

    def __init__(self, vc, states):
        self.vc = vc
        self.by_profile = collections.defaultdict(set)
        for s in states:
            self.by_profile[server_profile(s)].add(s)
        self.keys = {}

    def of(self, s):
        p = server_profile(s)
        if len(self.by_profile[p]) == 1:
            return p, None
        if s not in self.keys:
            self.keys[s] = rv.orbit_key(self.vc, s)
        return p, self.keys[s]


@functools.lru_cache(maxsize=None)
def reference(path, k):
    """The step's (generated, class of every in-model successor by its text, the new classes) from the
    oracle's successors of the first k roots.  A state's class is its text; under SYMMETRY its orbit."""
    smp, roots = path_roots(path)
    roots = roots[:k]
    sym = PATHS[path][1]
    succ = [u for r in roots for u in smp.succ[r]]
    if sym:
        orb = Orbits(smp.vc, [smp.states[r] for r in roots] + [u.state for u in succ if u.in_model])
        cls = orb.of
    else:
        def cls(s):
            return rv.state_text(smp.vc, s)
    seen = {cls(smp.states[r]) for r in roots}
    assert len(seen) == k, "the roots are distinct states (orbits)"
    by_text, new = {}, set()
    for u in succ:
        if u.in_model:
            c = by_text[u.text] = cls(u.state)
            if c not in seen:
                seen.add(c)
                new.add(c)
    return len(succ), by_text, new


def check_step(path, k, res):
    gen, by_text, new = reference(path, k)
    print("%s, %d roots: generated %d, new %d; got %s" % (path, k, gen, len(new), res["levels"]))
    assert res["status"] == [rtla.OK, rtla.OK] and res["violation"] is None
    assert res["levels"][0] == [k, k]
    assert res["levels"][1][1] == gen
    assert res["levels"][1][0] == len(new)
    got = res["texts"][1]
    unknown = [t for t in got if t not in by_text]
    assert not unknown, "%d new states are no in-model successor of a root; the first:\n%s" % (len(unknown), unknown[0])
    classes = [by_text[t] for t in got]
    assert len(set(classes)) == len(classes), "a state (orbit) stored twice"
    assert set(classes) == new


def path_job(path, k):
    smp, roots = path_roots(path)
    return sr.job(path_cfg(path), smp, list(roots[:k]), steps=1, frontiers=True)


def assert_kernel_rule(path):
    layout, sym, shards, xflags, kernel = PATHS[path]
    cfg = path_cfg(path)
    assert limits.kernel_of(cfg, symmetry=sym)[0] == kernel
    assert cfg.inv_mask == sum(rtla.INV_BITS[n] for n in mask_names(layout))  # compiled in together with its mask


# ---- no GPU needed: what the roots cover

@pytest.mark.parametrize("path", [p for p in PATHS if PATHS[p][2:4] == (0, 0)])
def test_roots_cover_every_family_and_server(path):
    """Over the 129 roots every action family of Next occurs, and every server is the changed one of some
    successor -- by the oracle's successors alone."""
    smp, roots = path_roots(path)
    fam, srv = coverage(smp, roots)
    print(path, dict(fam), dict(srv))
    assert [f for f in FAMILIES if not fam[f]] == []
    assert set(fam) <= set(FAMILIES)
    assert [i for i in range(PATHS[path][0][0][0]) if not srv[i]] == []


# ---- one seeded step on the GPU

@pytest.mark.gpu
@pytest.mark.parametrize("k", COUNTS)
@pytest.mark.parametrize("path", [p for p in PATHS if not PATHS[p][3]])
def test_seeded_step_is_the_oracles(path, k):
    assert_kernel_rule(path)
    assert "RTLA_XFLAGS" not in os.environ
    check_step(path, k, sr.run_job(path_job(path, k)))


@functools.lru_cache(maxsize=None)
def forced_results(tmp):
    return sr.run_jobs_in_child([path_job("cfg2_runtime", k) for k in COUNTS], PATHS["cfg2_runtime"][3], tmp)


@pytest.fixture(scope="module")
def child_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("tile_children"))


@pytest.mark.gpu
@pytest.mark.parametrize("k", COUNTS)
def test_seeded_step_on_the_forced_run_time_kernel(k, child_dir):
    """RTLA_XFLAGS=4096 (read once: one child process runs all nine root counts): the CFG2 configuration on the
    run-time-layout instantiation."""
    assert_kernel_rule("cfg2_runtime")
    check_step("cfg2_runtime", k, forced_results(child_dir)[COUNTS.index(k)])


# ---- tiles next to the arena's end

def _round64(n):
    return (n + 63) // 64 * 64


@pytest.mark.gpu
def test_tiles_at_the_arenas_end():
    """From Init under an arena that barely holds the largest (current + next) pair of levels: a level starts
    where the one before ends, rounded up to a group, so the levels walk around the ring and several of them
    cross its end -- the group before the end is loaded right up to it, the next one from the arena's start.
    Counts and level digests are the golden ones."""
    g = GOLD["n2_v2_t3_l2_m1"]
    x = [n for n, _ in g["levels"]]
    cap = _round64(max(_round64(x[i]) + x[i + 1] for i in range(len(x) - 1)))
    starts = [0]
    for n in x[:-1]:
        starts.append((starts[-1] + _round64(n)) % cap)
    crossing = [k + 1 for k in range(len(x)) if 0 < cap - starts[k] < x[k]]
    assert len(crossing) >= 3, crossing
    cfg = rtla.Config(g["n_server"], g["n_value"], g["max_term"], g["max_log"], g["max_copies"], g["max_msgs"],
                      tuple(g["invariants"]), fpset_log2=22, mem_budget=1 << 30, frontier_cap=cap, chunk=1024)
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
