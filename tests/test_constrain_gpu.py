"""GPU tests of user-defined CONSTRAINTs: the keep
bitmap and the in-place compaction kernels (rtla_kconstrain.hip) through the
stateless seam rtla_constrain_batch against the host's filter, and
Checker.constrain / run(constraint=) against the C oracle's goldens (a wider
configuration plus a constraint that restates a tighter built-in bound) and
against a test-side reference BFS (tests/constrainref.py)."""
import ctypes as C
import functools
import json
import os

import pytest

import constrainref
import hostmodel
import rtla
from limits import LIMITS

pytestmark = pytest.mark.gpu

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "bfs_counts.json")))
NARROW = rtla.Config(3, 2, 4, 3, 2, 0, (), bag_cap=12)
WIDEST = rtla.Config(*LIMITS["n5_l4_c14"][0], (), **LIMITS["n5_l4_c14"][1])  # 175 words: the widest of limits.py
LAYOUTS = {"narrow": NARROW, "widest": WIDEST}
SIZES = [1, 63, 64, 65, 127, 128, 1000]
STEP_SET = r"A == [][ \A i \in Server : currentTerm'[i] >= currentTerm[i] ]_vars"


def round64(n):
    return (n + 63) // 64 * 64


@functools.lru_cache(maxsize=None)
def sample(which):
    """(rows, k, passing rows, failing rows) of a layout: 1000 generator rows and the k for which
    BagCardinality(messages) <= k keeps the share nearest a half.  Shared, read-only."""
    cfg = LAYOUTS[which]
    rows = rtla.random_rows(cfg, 0, 1000)

    def kept_by(k):
        with rtla.Predicates(cfg, "Half == BagCardinality(messages) <= %d" % k) as p:
            return rtla.pred_replay(p, rows)[0]

    lo, hi = 0, 1024  # the share kept grows with k: the least k that keeps half or more
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if kept_by(mid).count(0) * 2 >= len(rows) else (mid + 1, hi)
    k, masks = lo, kept_by(lo)
    share = masks.count(0) / len(rows)
    assert 0.3 <= share <= 0.7, (which, k, share)
    return rows, k, [r for r, m in zip(rows, masks) if m == 0], [r for r, m in zip(rows, masks) if m != 0]


def placements(n, chunk):
    """Ring starts for ring_cap = round64(n) + 64: no wrap; a wrap inside a chunk; a wrap exactly at a chunk
    boundary (where the sizes allow one)."""
    cap, span = round64(n) + 64, round64(n)
    starts = {0}
    for rows_before_wrap in range(64, span, 64):
        if rows_before_wrap % chunk:
            starts.add(cap - rows_before_wrap)  # inside a chunk
            break
    if chunk < span:
        starts.add(cap - chunk)  # the first chunk ends at the arena's end
    return cap, sorted(starts)


def patterns(which, n):
    """name -> (constraint text, rows): which rows survive is decided by the rows passed, or by TRUE / FALSE."""
    rows, k, good, bad = sample(which)
    half = "Half == BagCardinality(messages) <= %d" % k
    g, b = good[:n], bad[:n]
    assert len(g) == min(n, len(good)) and len(b) == min(n, len(bad)) and len(good) >= 300 and len(bad) >= 300
    fill = lambda pool: [pool[i % len(pool)] for i in range(n - 1)]
    return {"all": ("T == TRUE", rows[:n]), "none": ("F == FALSE", rows[:n]),
            "only row 0": (half, [good[0]] + fill(bad)), "only the last": (half, fill(bad) + [good[0]]),
            "all but row 0": (half, [bad[0]] + fill(good)), "all but the last": (half, fill(good) + [bad[0]]),
            "half": (half, rows[:n])}


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("which", sorted(LAYOUTS))
def test_batch_equals_the_host_filter(which, n):
    """Every (chunk, ring placement, keep pattern) at one size: the kept rows and the kept entries of the side
    array arange(n), exactly and in order, and the per-definition counts."""
    cfg = LAYOUTS[which]
    ran = 0
    for name, (text, rows) in patterns(which, n).items():
        with rtla.Predicates(cfg, text) as preds:
            masks, counts = rtla.pred_replay(preds, rows)
            want = [list(r) for r, m in zip(rows, masks) if m == 0], [i for i, m in enumerate(masks) if m == 0], counts
            if name == "half" and n == 1000:
                assert 0.3 <= len(want[0]) / n <= 0.7
            for chunk in sorted({64, 128, round64(n)}):
                cap, starts = placements(n, chunk)
                for start in starts:
                    got = rtla.constrain_batch(preds, rows, ring_cap=cap, ring_start=start, chunk=chunk)
                    assert got == want, (name, chunk, cap, start, len(got[0]), len(want[0]))
                    ran += 1
    assert ran >= 7 * (3 if n > 128 else 1)


def test_batch_wrap_placements_exist():
    """The parametrisation above does reach both kinds of wrap (a host check of the test's own helper)."""
    assert placements(1000, 128) == (1088, [0, 960, 1024]) and placements(1000, 64) == (1088, [0, 1024])
    assert placements(1000, 1024)[1] == [0, 1024] and placements(128, 64)[1] == [0, 128] and placements(64, 64)[1] == [0]


def test_batch_two_definitions_counts_and_errors():
    rows, k, _, _ = sample("narrow")
    text = "Half == BagCardinality(messages) <= %d\nLowTerms == \\A i \\in Server : currentTerm[i] <= 3" % k
    with rtla.Predicates(NARROW, text) as preds:
        masks, counts = rtla.pred_replay(preds, rows)
        assert len(set(masks)) == 4  # neither, either, both
        got = rtla.constrain_batch(preds, rows, ring_cap=1088, ring_start=960, chunk=128)
        assert got == ([list(r) for r, m in zip(rows, masks) if m == 0], [i for i, m in enumerate(masks) if m == 0],
                       counts)
        assert rtla.constrain_batch(preds, []) == ([], [], dict.fromkeys(preds.names, 0))
    # an evaluation error on one row: RTLA_E_SPEC, no output written
    with rtla.Predicates(NARROW, r"SomeLogEmpty == \E i \in Server : Len(log[i]) = 0") as split:
        empty = [m == 0 for m in rtla.pred_replay(split, rows)[0]]
    good = [r for r, e in zip(rows, empty) if not e][:200]
    bad = [r for r, e in zip(rows, empty) if e][0]
    assert len(good) == 200
    w = rtla.row_words(NARROW)
    with rtla.Predicates(NARROW, r"FirstEntries == \A i \in Server : log[i][1].term >= 1") as preds:
        assert rtla.constrain_batch(preds, good, chunk=64)[1] == list(range(200))
        for at in (0, 64, 199):
            batch = list(good)
            batch[at] = bad
            with pytest.raises(rtla.RtlaError) as e:
                rtla.constrain_batch(preds, batch, chunk=64)
            assert e.value.status == rtla.E_SPEC and e.value.flags & rtla.CAP_SPEC_ERROR
            flat, n = rtla._flat_rows(batch, w)
            out = (C.c_uint32 * (n * w))(*([0xA5A5A5A5] * (n * w)))
            side = (C.c_uint64 * n)(*range(7, 7 + n))
            kept, counts = C.c_size_t(12345), (C.c_uint64 * 8)(*([99] * 8))
            cc = NARROW.c()
            rc = rtla._lib.rtla_constrain_batch(C.byref(cc), preds._h, flat, n, 256, 192, 64, out, side, C.byref(kept),
                                                counts)
            assert rc == rtla.E_SPEC and kept.value == 12345 and list(counts) == [99] * 8
            assert set(out) == {0xA5A5A5A5} and list(side) == list(range(7, 7 + n))
    with rtla.Predicates(NARROW, "T == TRUE") as preds, rtla.Actions(NARROW, STEP_SET) as acts:
        cc, kept = NARROW.c(), C.c_size_t(0)
        flat, n = rtla._flat_rows(good, w)
        out, side = (C.c_uint32 * (n * w))(), (C.c_uint64 * n)()
        call = lambda h, cap, start: rtla._lib.rtla_constrain_batch(C.byref(cc), h, flat, n, cap, start, 64, out, side,
                                                                     C.byref(kept), None)
        assert call(preds._h, 256, 0) == rtla.OK and kept.value == n
        assert call(acts._h, 256, 0) == rtla.E_ARG  # a step set
        for cap, start in ((192, 0), (250, 0), (256, 32), (256, 256)):  # too small, no whole groups, bad starts
            assert call(preds._h, cap, start) == rtla.E_ARG
        with rtla.Predicates(WIDEST, "T == TRUE") as other:
            assert call(other._h, 256, 0) == rtla.E_ARG  # another layout's


# ---- oracle-pinned identities: a wider configuration + a constraint that restates a tighter built-in bound

TERM2 = r"C == \A i \in Server : currentTerm[i] <= 2"
TERM3 = r"C == \A i \in Server : currentTerm[i] <= 3"
LOG1 = r"C == \A i \in Server : Len(log[i]) <= 1"
BAG1 = r"C == (\A m \in DOMAIN messages : messages[m] <= 1) /\ BagCardinality(messages) <= 1"


def constrained_search(cfg, text, digest="text"):
    """(levels [[kept, generated]], distinct, generated, depth, violation, per-level digests, constrain results).
    digest: "text" / "orbit" through the checker's own level digest; "rows": the same sum over the rows of
    frontier() (rtla_rows_text_hash), which spares a repeated search the digest's pinned staging buffers."""
    digests, stats = [], []
    with rtla.Checker(cfg) as ck, rtla.Predicates(cfg, text) as con:
        st = ck.init()
        while True:
            if st == rtla.OK and ck.levels[-1].new > 0:
                stats.append(ck.constrain(con))
                st = ck.status
            digests.append("%016x" % (ck.level_orbit_hash() if digest == "orbit" else
                                      rtla.rows_text_hash(cfg, ck.frontier()) if digest == "rows" else
                                      ck.level_text_hash()))
            if st != rtla.OK:
                break
            st = ck.step()
        depth = sum(1 for lv in ck.levels if lv.new > 0)
        viol = ck.violation()[0] if st == rtla.VIOLATION else None
        return [[lv.new, lv.generated] for lv in ck.levels], ck.distinct, ck.generated, depth, viol, digests, stats


def assert_golden(got, g, key="level_text_hash"):
    levels, distinct, generated, depth, viol, digests, _ = got
    assert levels == g["levels"]
    assert (distinct, generated, depth) == (g["distinct"], g["generated"], g["depth"])
    assert viol is None and not g["violated"]
    n = min(len(digests), len(g[key]))
    assert n >= len(g[key]) - 1 and digests[:n] == g[key][:n]


@pytest.mark.parametrize("shape,text", [((2, 1, 3, 1, 1, 1), TERM2), ((2, 1, 2, 4, 1, 1), LOG1),
                                        ((2, 1, 2, 1, 2, 2), BAG1)], ids=["term", "log", "bag"])
def test_tighter_bound_as_a_constraint_reproduces_the_golden(shape, text):
    g = GOLD["n2_v1_t2_l1_m1"]
    assert g["distinct"] == 1760
    cfg = rtla.Config(*shape, invariants=tuple(g["invariants"]), fpset_log2=20, mem_budget=1 << 29)
    assert_golden(constrained_search(cfg, text), g)
    # the same through run(constraint=) / check(constraint=)
    with rtla.Predicates(cfg, text) as con:
        res = rtla.check(cfg, constraint=con)
    assert [[lv.new, lv.generated] for lv in res.levels] == g["levels"]
    assert (res.distinct, res.generated, res.depth, res.violation) == (g["distinct"], g["generated"], g["depth"], None)


def test_term_constraint_under_symmetry_reproduces_the_golden():
    g = GOLD["n2_v1_t2_l1_m1_sym"]
    cfg = rtla.Config(2, 1, 3, 1, 1, 1, tuple(g["invariants"]), symmetry=True, fpset_log2=20, mem_budget=1 << 29)
    assert_golden(constrained_search(cfg, TERM2, digest="orbit"), g, key="level_orbit_hash")


def test_term3_of_term5_default_chunked_and_wrapping(monkeypatch):
    g = GOLD["n2_v1_t3_l1_m1"]
    assert g["distinct"] == 25164
    kw = dict(invariants=tuple(g["invariants"]), fpset_log2=20)
    cfg = rtla.Config(2, 1, 5, 1, 1, 1, mem_budget=1 << 29, **kw)
    first = constrained_search(cfg, TERM3)
    assert_golden(first, g)
    examined = [s.examined for s in first[6]]
    assert max(examined) > 256
    monkeypatch.setenv("RTLA_CONSTRAIN_CHUNK", "128")
    assert_golden(constrained_search(cfg, TERM3, digest="rows"), g)
    monkeypatch.delenv("RTLA_CONSTRAIN_CHUNK")
    # an arena just large enough for any level beside the next one, unfiltered: the ring start advances and wraps
    cap = round64(max(round64(a) + b for a, b in zip(examined, examined[1:] + [0]))) + 64
    small = rtla.Config(2, 1, 5, 1, 1, 1, frontier_cap=cap, **kw)
    wrapped = constrained_search(small, TERM3, digest="rows")
    assert_golden(wrapped, g)
    assert any(s.start + s.examined > cap for s in wrapped[6])
    monkeypatch.setenv("RTLA_CONSTRAIN_CHUNK", "128")
    assert_golden(constrained_search(small, TERM3, digest="rows"), g)


def test_n3_term2_of_the_two_leader_configuration(monkeypatch):
    """The term-3 two-leader states of n3_v1_t3_l1_m1_ntl are checked and dropped, as the T = 2 oracle checks
    them out of model: no violation, and the 2,379,781 states of n3_v1_t2_l1_m1 level by level."""
    g, wide = GOLD["n3_v1_t2_l1_m1"], GOLD["n3_v1_t3_l1_m1_ntl"]
    assert g["distinct"] == 2379781 and len(g["levels"]) == 54 and wide["violated"] and wide["max_term"] == 3
    monkeypatch.setenv("RTLA_CONSTRAIN_CHUNK", "4096")
    cfg = rtla.Config(wide["n_server"], wide["n_value"], wide["max_term"], wide["max_log"], wide["max_copies"],
                      wide["max_msgs"], tuple(wide["invariants"]), fpset_log2=24, mem_budget=3 << 30)
    got = constrained_search(cfg, TERM2)
    assert_golden(got, g)
    assert any(s.examined > 4096 and s.dropped for s in got[6])


# ---- a constraint that is no built-in bound, against the reference BFS

def frontier_is_whole(ck, cfg):
    for row in ck.frontier():
        assert rtla.stored_fingerprint(row) == rtla.row_fingerprint(cfg, row)


@pytest.mark.parametrize("shape,which,cut", [((2, 1, 3, 1, 1, 1), "one_candidate", 100),
                                             ((2, 1, 3, 1, 1, 1), "one_candidate_one_election", 100),
                                             ((3, 1, 2, 1, 1, 1), "one_candidate", 12),
                                             ((3, 1, 2, 1, 1, 1), "one_candidate_one_election", 12)])
def test_constrained_search_equals_the_reference_bfs(shape, which, cut):
    cfg, text, ref = constrainref.case(shape, which, cut)
    assert sum(len(lv.dropped) for lv in ref) > 0 and len(ref) > 8
    with rtla.Checker(cfg) as ck, rtla.Predicates(cfg, text) as con:
        st = ck.init()
        for k, lv in enumerate(ref):
            assert st == rtla.OK or (st == rtla.DONE and k == len(ref) - 1 and not lv.kept), k
            if st == rtla.OK and ck.levels[-1].new > 0:
                res = ck.constrain(con)
                assert (res.examined, res.kept, res.dropped) == (len(lv.kept) + len(lv.dropped), len(lv.kept),
                                                                 len(lv.dropped)), k
                st = ck.status
            assert (ck.levels[-1].new, ck.levels[-1].generated) == (len(lv.kept), lv.generated), k
            assert ck.frontier_size() == len(lv.kept)
            assert ck.level_text_hash() == rtla.rows_text_hash(cfg, lv.kept), k
            if lv.kept:
                audit = ck.audit_predicates(con)
                assert audit.status == rtla.OK and audit.audited == len(lv.kept) and not any(audit.counts.values())
                if len(lv.kept) < 4000:
                    frontier_is_whole(ck, cfg)
            if k + 1 < len(ref):
                st = ck.step()
        assert ck.distinct == sum(len(lv.kept) for lv in ref)
        assert ck.generated == sum(lv.generated for lv in ref)
        if not ref[-1].kept:
            assert st == rtla.DONE


# ---- traces through a constrained search

NO_LEADER = r"NoLeader == \A i \in Server : state[i] # Leader"
NEVER_ALL_CANDIDATES = r"NeverAllCandidates == [][ ~ \A i \in Server : state'[i] = Candidate ]_vars"


def trace_rows(cfg, trace):
    """The rows of a trace's states, each found among hostmodel.expand's successors of the one before it."""
    w = rtla.row_words(cfg)
    rows = [constrainref.init_row(cfg)]
    assert trace[0][1] == rtla.state_text(cfg, rows[0])
    for label, text in trace[1:]:
        nxt = [r for _, _, _, _, r in hostmodel.expand(cfg, [rows[-1]], w) if rtla.state_text(cfg, r) == text]
        assert nxt, label
        rows.append(nxt[0])
    return rows


def test_trace_through_a_constrained_search():
    cfg, text, ref = constrainref.case((3, 1, 2, 1, 1, 1), "one_candidate", 12)
    with rtla.Predicates(cfg, NO_LEADER) as inv, rtla.Predicates(cfg, text) as con:
        # the reference's depth: the first level, unfiltered, that holds a leader
        depth = next(k + 1 for k, lv in enumerate(ref)
                     if any(rtla.pred_replay(inv, list(lv.kept + lv.dropped))[0]))
        assert 3 < depth < len(ref)
        res = rtla.check(cfg, predicates=inv, constraint=con)
        assert res.violation == "NoLeader" and res.depth == depth and len(res.trace) == depth
        rows = trace_rows(cfg, res.trace)
        assert not any(rtla.pred_replay(con, rows[:-1])[0]) and rtla.pred_replay(inv, rows)[0][-1] == 1
        assert [[lv.new, lv.generated] for lv in res.levels[:depth - 1]] == \
            [[len(lv.kept), lv.generated] for lv in ref[:depth - 1]]


def test_action_property_sees_the_kept_rows_steps_only():
    cfg, text, ref = constrainref.case((3, 1, 2, 1, 1, 1), "one_candidate", 12)
    with rtla.Actions(cfg, NEVER_ALL_CANDIDATES) as act, rtla.Predicates(cfg, text) as con:
        dropped = [r for lv in ref[:-1] for r in lv.dropped]
        assert any(rtla.pred_step_replay(act, dropped)[0])  # a dropped state's step would violate it
        for lv in ref[:-1]:
            assert not any(rtla.pred_step_replay(act, list(lv.kept))[0])
        with rtla.Checker(cfg) as ck:
            assert ck.run(max_levels=len(ref) - 1, constraint=con, actions=act) == rtla.OK
            assert [lv.new for lv in ck.levels] == [len(lv.kept) for lv in ref[:-1]]
        with rtla.Checker(cfg) as ck:  # without the constraint the step is reached
            assert ck.run(max_levels=len(ref) - 1, actions=act) == rtla.VIOLATION


# ---- state handling

def test_states_and_arguments(tmp_path):
    cfg = rtla.Config(2, 1, 3, 1, 1, 1, ("NoTwoLeaders",), fpset_log2=18, mem_budget=256 << 20)
    with rtla.Predicates(cfg, "F == FALSE") as never, rtla.Predicates(cfg, TERM2) as con, \
            rtla.Actions(cfg, STEP_SET) as act:
        with rtla.Checker(cfg) as ck:
            with pytest.raises(rtla.RtlaError) as e:
                ck.constrain(con)  # before init
            assert e.value.status == rtla.E_STATE
            ck.init()
            with pytest.raises(rtla.RtlaError) as e:
                ck.constrain(act)
            assert e.value.status == rtla.E_ARG
            with rtla.Predicates(NARROW, "T == TRUE") as other, pytest.raises(rtla.RtlaError) as e:
                ck.constrain(other)
            assert e.value.status == rtla.E_ARG
            res = ck.constrain(never)  # FALSE on Init: the search is over, nothing is distinct
            assert (res.status, res.kept, res.dropped, ck.distinct, ck.status) == (rtla.DONE, 0, 1, 0, rtla.DONE)
            assert ck.levels[-1].new == 0 and ck.frontier_size() == 0
            with pytest.raises(rtla.RtlaError) as e:
                ck.step()
            assert e.value.status == rtla.E_STATE
        with rtla.Checker(rtla.Config(2, 1, 3, 1, 1, 1, ("NoTwoLeaders",), fpset_log2=18, mem_budget=512 << 20,
                                      shards=2)) as ck:
            ck.init()
            with pytest.raises(rtla.RtlaError) as e:
                ck.constrain(con)
            assert e.value.status == rtla.E_STATE
        with rtla.Predicates(cfg, "T == TRUE") as always:
            assert rtla.check(cfg, constraint=always, trace=False).distinct == 25164


def test_an_evaluation_error_leaves_the_level_as_it_was():
    cfg = rtla.Config(2, 1, 3, 1, 1, 1, ("NoTwoLeaders",), fpset_log2=18, mem_budget=256 << 20)
    g = GOLD["n2_v1_t3_l1_m1"]
    with rtla.Checker(cfg) as ck, rtla.Predicates(cfg, r"E == \A i \in Server : log[i][1].term >= 1") as err:
        ck.init()
        for _ in range(9):
            ck.step()
        before = (ck.frontier_size(), ck.level_text_hash(), ck.distinct, ck.levels[-1].new)
        with pytest.raises(rtla.RtlaError) as e:
            ck.constrain(err)
        assert e.value.status == rtla.E_SPEC and e.value.flags & rtla.CAP_SPEC_ERROR
        assert (ck.frontier_size(), ck.level_text_hash(), ck.distinct, ck.levels[-1].new) == before
        while ck.status == rtla.OK:
            ck.step()
        assert [[lv.new, lv.generated] for lv in ck.levels] == g["levels"] and ck.distinct == g["distinct"]


def test_checkpoint_and_recover_after_a_constrained_level(tmp_path):
    g = GOLD["n2_v1_t2_l1_m1"]
    cfg = rtla.Config(2, 1, 3, 1, 1, 1, tuple(g["invariants"]), fpset_log2=18, mem_budget=256 << 20)
    prefix = str(tmp_path / "ck")
    with rtla.Predicates(cfg, TERM2) as con:
        with rtla.Checker(cfg) as ck:
            assert ck.run(max_levels=12, constraint=con) == rtla.OK
            assert [[lv.new, lv.generated] for lv in ck.levels] == g["levels"][:12]
            ck.checkpoint(prefix)
        with rtla.Checker(cfg) as ck:
            ck.recover(prefix)
            assert ck.frontier_size() == g["levels"][11][0]
            assert "%016x" % ck.level_text_hash() == g["level_text_hash"][11]
            assert ck.run(constraint=con) == rtla.DONE
            assert [[lv.new, lv.generated] for lv in ck.levels] == g["levels"][12:]
            assert (ck.distinct, ck.generated) == (g["distinct"], g["generated"])


def test_step_audit_and_simulate_work_on_the_kept_rows():
    cfg, text, ref = constrainref.case((2, 1, 3, 1, 1, 1), "one_candidate", 100)
    k = next(i for i, lv in enumerate(ref) if len(lv.dropped) > 3 and len(lv.kept) > 3)
    with rtla.Checker(cfg) as ck, rtla.Predicates(cfg, text) as con:
        ck.run(max_levels=k, constraint=con)
        ck.step()
        res = ck.constrain(con)
        kept = [list(r) for r in ref[k].kept]
        front = ck.frontier()  # (the level kernel appends new states in no fixed order)
        assert res.kept == len(kept) and sorted(front) == sorted(kept)
        audit = ck.audit(("NoTwoLeaders",))
        assert audit.audited == len(kept)
        n = 2 * len(kept) + 3
        sim = ck.simulate(n, 6, seed=11, ends=True)
        assert sim.ends == rtla.sim_replay(cfg, front, n, 6, seed=11).ends  # walk w starts at kept row w mod kept
        assert ck.step() == rtla.OK
        assert (ck.levels[-1].frontier, ck.levels[-1].generated) == (len(kept), ref[k + 1].generated)
