"""The search's verdict, pinned on every kernel that can give one: a search seeded from chosen roots
(rtla_init_rows / Checker.init(roots)) against the value oracle (tests/seedref.py: raft_values.next_states,
in_model and the five invariants in Python; no product code on the reference side).

From Init Raft violates nothing but NoTwoLeaders, so only a seeded search can make a kernel report the
other invariants, an out-of-model violation, a mask of several bits, or a violation whose parent sits in
a level's second or third 64-row group or on another shard than its successor's owner.

Exact-verdict cases: the roots are every row of the sample that is quiet for the configuration's mask
plus ONE row with exactly one violating successor, so status, mask, in_model and the two-row trace are
determined.  The matrix, kernel path x the invariants it can report (each with the violator as root 0, as
root 64 and as the last root):
    k_expand_compact, layout compiled in   CFG2, SYNTH, EXHAUST: ElectionSafety, LogMatching (their mask is
      (test_compiled_in_*)                 both; the violator violates one); CFG1: NoTwoLeaders
    k_expand_compact, run-time layout      all five: the CFG2 shape with a one-invariant mask (64-state
      (test_run_time_*)                    groups), the same under RTLA_XFLAGS=4096 (and the CFG2 mask, forced
                                           onto the run-time layout), and the narrow (2,2,3,2,1,0) shape
    k_expand (wave per state)              all five: RTLA_XFLAGS=2048 on the CFG2 shape
    k_expand_compact<SYM>, run-time        all five on (5,1,3,2,1,0) with SYMMETRY, roots one per orbit.  The
                                           compiled-in CFG4 has mask 0 and cannot report: it must stay OK
    shards = 2, 3 (k_expand_compact<MULTI> all five, the violating successor owned once by its parent's shard
      and k_build_winners)                 (the level kernel reports it) and once by another (the winners kernel)
No pair is left to the membership form: the generator yields a single-violator root for every pair above,
CFG1 and EXHAUST included (tests/test_seed_host.py asserts each root set exists).

Which kernel ran is not observable through the ABI (rtla_device_info does not tell); each test asserts
the rule that chooses it instead: limits.kernel_of for compact / wave and the group size, the mask for
compiled-in / run-time (rtla_kdev.h specs: a layout is compiled in together with its mask), RTLA_XFLAGS.
"""
import functools
import json
import os

import pytest

import limits
import rtla
import seedref as sr
import tla_text
from test_safety_host import py_mask

pytestmark = pytest.mark.gpu

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "bfs_counts.json")))
ALL = sr.ALL
BIT = rtla.INV_BITS
MEM = dict(fpset_log2=20, mem_budget=1 << 29)


def cfg_of(layout, invariants, shards=0, symmetry=False):
    kw = dict(MEM, mem_budget=MEM["mem_budget"] * max(1, shards))
    return sr.configs(*layout, invariants, shards=shards, symmetry=symmetry, **kw)[0]


def smp_of(layout):
    return sr.sample(*layout, sr.ROWS[layout])


def exact_roots(layout, mask, bit, pos, in_model=True, pick=0, orbits=False):
    """(sample, root ids, the violator's id): every row quiet for `mask` and one whose single violating
    successor violates `bit` alone of `mask`."""
    smp = smp_of(layout)
    quiet, singles = smp.quiet(mask), smp.single(mask, in_model, bit)
    if orbits:
        quiet = sr.one_per_orbit(smp, quiet)
    assert len(quiet) >= 129 and len(singles) > pick, (len(quiet), len(singles))
    return smp, sr.place(quiet, singles[pick], pos), singles[pick]


def check_exact(res, smp, roots, v, mask, bit, in_model=True):
    """One violating step: root v -> its one successor violating `mask`."""
    u, = smp.violators(v, mask)
    print("roots %d, violator %d at %d: %s -> mask %d in_model %s; got %s mask %d" % (
        len(roots), v, roots.index(v), u.label, u.mask & mask, u.in_model, res["status"], res["mask"]))
    assert res["status"] == [rtla.OK, rtla.VIOLATION]
    assert res["levels"][0] == [len(roots), len(roots)]
    assert res["mask"] == bit == u.mask & mask and res["in_model"] is in_model is u.in_model
    assert res["violation"] == rtla.inv_names(bit)[0]
    (l0, t0), (l1, t1) = res["trace"]
    assert (l0, t0) == ("Initial predicate", smp.texts[v])
    assert t1 == u.text
    assert sr.family(l1) in {sr.family(x.label) for x in smp.succ[v] if x.text == u.text}, l1


# ---- the compiled-in compact kernels

COMPILED = [(sr.CFG2, "ElectionSafety"), (sr.CFG2, "LogMatching"), (sr.SYNTH, "ElectionSafety"),
            (sr.SYNTH, "LogMatching"), (sr.EXHAUST, "ElectionSafety"), (sr.EXHAUST, "LogMatching"),
            (sr.CFG1, "NoTwoLeaders")]
LAYOUT_ID = {sr.CFG2: "CFG2", sr.SYNTH: "SYNTH", sr.EXHAUST: "EXHAUST", sr.CFG1: "CFG1", sr.N2: "N2", sr.CFG4: "CFG4"}


@pytest.mark.parametrize("pos", sr.POSITIONS)
@pytest.mark.parametrize("layout,inv", COMPILED, ids=lambda p: LAYOUT_ID.get(p, p))
def test_compiled_in_kernel_reports_its_invariants(layout, inv, pos):
    """k_expand_compact with the layout compiled in (rtla_kdev.h specs): the configuration is the benchmark's,
    mask included, so the dispatch (same_layout) takes the compiled instantiation."""
    names = sr.COMPILED_MASK[layout]
    cfg = cfg_of(layout, names)
    assert limits.kernel_of(cfg)[0].startswith("compact") and "RTLA_XFLAGS" not in os.environ
    mask = cfg.inv_mask
    smp, roots, v = exact_roots(layout, mask, BIT[inv], pos)
    check_exact(sr.run_job(sr.job(cfg, smp, roots)), smp, roots, v, mask, BIT[inv])


# ---- the run-time-layout compact kernel

@pytest.mark.parametrize("pos", sr.POSITIONS)
@pytest.mark.parametrize("inv", ALL)
@pytest.mark.parametrize("layout", [sr.CFG2, sr.N2], ids=LAYOUT_ID.get)
def test_run_time_kernel_reports_each_invariant(layout, inv, pos):
    """k_expand_compact on its run-time layout, groups of 64 states (both shapes): a one-invariant mask is
    no compiled-in layout's (CFG1's NoTwoLeaders belongs to another shape)."""
    cfg = cfg_of(layout, (inv,))
    assert limits.kernel_of(cfg)[0] == "compact64" and layout != sr.CFG1
    smp, roots, v = exact_roots(layout, BIT[inv], BIT[inv], pos)
    check_exact(sr.run_job(sr.job(cfg, smp, roots)), smp, roots, v, BIT[inv], BIT[inv])


def child_cases(xflags):
    """(id, job, check arguments) of the cases run in one child process with RTLA_XFLAGS = xflags."""
    cases = []
    masks = [(inv,) for inv in ALL] + ([sr.COMPILED_MASK[sr.CFG2]] * 2 if xflags == 4096 else [])
    targets = list(ALL) + (list(sr.COMPILED_MASK[sr.CFG2]) if xflags == 4096 else [])
    for names, inv in zip(masks, targets):
        for pos in sr.POSITIONS:
            cfg = cfg_of(sr.CFG2, names)
            smp, roots, v = exact_roots(sr.CFG2, cfg.inv_mask, BIT[inv], pos)
            cases.append(("%s-%s-%s" % ("+".join(names), inv, pos), sr.job(cfg, smp, roots),
                          (smp, roots, v, cfg.inv_mask, BIT[inv], True)))
    if xflags == 2048:  # the out-of-model verdict on the wave-per-state kernel
        for inv in sr.SINGLE_OUT:
            cfg = cfg_of(sr.N2, (inv,))
            smp, roots, v = out_of_model_roots(inv)
            cases.append(("out-of-model-" + inv, sr.job(cfg, smp, roots), (smp, roots, v, BIT[inv], BIT[inv], False)))
    return cases


@functools.lru_cache(maxsize=None)
def child_results(xflags, tmp):
    cases = child_cases(xflags)
    return dict(zip([c[0] for c in cases], sr.run_jobs_in_child([c[1] for c in cases], xflags, tmp)))


@pytest.fixture(scope="module")
def child_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("seed_children"))


CHILD_IDS = {x: ["%s-%s-%s" % ("+".join(n), i, p) for n, i in
                 [((inv,), inv) for inv in ALL] + ([(sr.COMPILED_MASK[sr.CFG2], i) for i in sr.COMPILED_MASK[sr.CFG2]]
                                                   if x == 4096 else [])
                 for p in sr.POSITIONS] + (["out-of-model-" + i for i in sr.SINGLE_OUT] if x == 2048 else [])
             for x in (4096, 2048)}


@pytest.mark.parametrize("case", CHILD_IDS[4096])
def test_run_time_kernel_forced_reports_each_invariant(case, child_dir):
    """RTLA_XFLAGS=4096 (XF_NO_SPECIAL, read once: one child process runs all cases): the run-time layout
    also for the CFG2 configuration with its compiled mask, and for each single invariant."""
    args = {c[0]: c[2] for c in child_cases(4096)}[case]
    check_exact(child_results(4096, child_dir)[case], *args[:5], in_model=args[5])


@pytest.mark.parametrize("case", CHILD_IDS[2048])
def test_wave_kernel_reports_each_invariant(case, child_dir):
    """RTLA_XFLAGS=2048 (XF_WAVE_KERNEL; one child process): k_expand, the wave-per-state kernel, on the CFG2
    shape for all five invariants, and the out-of-model verdict on the narrow shape."""
    args = {c[0]: c[2] for c in child_cases(2048)}[case]
    check_exact(child_results(2048, child_dir)[case], *args[:5], in_model=args[5])


# ---- SYMMETRY

@pytest.mark.parametrize("pos", sr.POSITIONS)
@pytest.mark.parametrize("inv", ALL)
def test_symmetry_kernel_reports_each_invariant(inv, pos):
    """k_expand_compact<SYM> on its run-time layout ((5,1,3,2,1,0) with a one-invariant mask; CFG4, the
    compiled-in one, has mask 0), groups of 32.  Quiet and single are properties of an orbit (the invariants
    do not name servers); the roots hold one row per orbit."""
    cfg = cfg_of(sr.CFG4, (inv,), symmetry=True)
    assert limits.kernel_of(cfg, symmetry=True)[0] == "compact32"
    smp, roots, v = exact_roots(sr.CFG4, BIT[inv], BIT[inv], pos, orbits=True)
    check_exact(sr.run_job(sr.job(cfg, smp, roots)), smp, roots, v, BIT[inv], BIT[inv])


def test_symmetry_roots_of_one_orbit_count_once():
    """Two members of one orbit among the roots: the first is kept (level 1: new = orbits, generated = rows
    given), its row is the one stored, and the verdict is the same."""
    inv = "LogMatching"
    cfg = cfg_of(sr.CFG4, (inv,), symmetry=True)
    smp, roots, v = exact_roots(sr.CFG4, BIT[inv], BIT[inv], "last", orbits=True)
    rows = [list(smp.rows[k]) for k in roots]
    twins = [rtla.permute_row(cfg, rows[k], pi) for k, pi in ((3, [1, 0, 2, 3, 4]), (70, [4, 3, 2, 1, 0]),
                                                              (len(rows) - 1, [1, 2, 3, 4, 0]))]
    moved = [k for k, t in zip((3, 70, len(rows) - 1), twins) if t != rows[k]]
    assert moved, "the images are other rows of the same orbits"
    given = rows[:80] + twins[:2] + rows[80:] + twins[2:]
    with rtla.Checker(cfg) as ck:
        assert ck.init(given) == rtla.OK
        assert (ck.levels[0].new, ck.levels[0].generated) == (len(rows), len(given))
        assert sorted(rtla.state_text(cfg, r) for r in ck.frontier()) == sorted(smp.texts[k] for k in roots)
        assert all(rtla.stored_fingerprint(r) == rtla.row_fingerprint(cfg, r) for r in ck.frontier())
        assert ck.step() == rtla.VIOLATION
        assert ck.trace()[0] == ("Initial predicate", smp.texts[v])
        assert ck.trace()[1][1] == smp.violators(v, BIT[inv])[0].text


def test_compiled_in_symmetry_kernel_has_no_invariant_to_report():
    """CFG4 as compiled in (mask 0): the same roots, a violator of every invariant among them, stay OK."""
    cfg = cfg_of(sr.CFG4, (), symmetry=True)
    smp = smp_of(sr.CFG4)
    roots = sr.one_per_orbit(smp, sorted(set(k for inv in ALL for k in
                                             exact_roots(sr.CFG4, BIT[inv], BIT[inv], "last", orbits=True)[1])))
    assert all(any(smp.violators(k, BIT[inv]) for k in roots) for inv in ALL)
    res = sr.run_job(sr.job(cfg, smp, roots))
    assert res["status"] == [rtla.OK, rtla.OK] and res["mask"] == 0 and res["violation"] is None
    assert res["levels"][0] == [len(roots), len(roots)]
    assert res["levels"][1][1] == sum(len(smp.succ[k]) for k in roots)  # (generated: every successor, orbits or not)


# ---- several shards

@pytest.mark.parametrize("owned", ["by the parent's shard", "by another shard"])
@pytest.mark.parametrize("inv", ALL)
@pytest.mark.parametrize("shards", [2, 3])
def test_shards_report_each_invariant(shards, inv, owned):
    """The CFG2 shape on 2 and 3 virtual shards, one-invariant masks.  Roots live on the shard that owns
    them; the violating successor is owned by that same shard (k_expand_compact<MULTI> builds and reports
    it) or by another (it travels as a record and k_build_winners reports it): the two-row trace then
    crosses the shard boundary."""
    smp = smp_of(sr.CFG2)
    same, other = sr.shard_picks(*sr.CFG2, sr.ROWS[sr.CFG2], BIT[inv], shards)
    v = same if owned.startswith("by the parent") else other
    assert v is not None
    quiet = smp.quiet(BIT[inv])
    assert len(quiet) >= 129
    roots = sr.place(quiet, v, "at 64")
    cfg = cfg_of(sr.CFG2, (inv,), shards=shards)
    check_exact(sr.run_job(sr.job(cfg, smp, roots)), smp, roots, v, BIT[inv], BIT[inv])


# ---- the out-of-model verdict

def out_of_model_roots(inv):
    """The narrow shape's quiet rows and one pinned row whose single violating successor is out of the model."""
    n = sr.ROWS[sr.N2]
    smp = sr.sample(*sr.N2, n, extra=sr.SINGLE_OUT[inv])
    pinned = list(range(n, len(smp.rows)))
    assert pinned and set(pinned) <= set(smp.single(BIT[inv], in_model=False)), "the pinned ids are single-out"
    quiet = smp.quiet(BIT[inv])
    assert len(quiet) >= 129
    return smp, sr.place(quiet, pinned[0], "at 64"), pinned[0]


@pytest.mark.parametrize("shards", [0, 2])
@pytest.mark.parametrize("inv", list(sr.SINGLE_OUT))
def test_out_of_model_violation_is_reported(inv, shards):
    """in_model = 0: the violating successor leaves the StateConstraint (a message count of MaxCopies + 1),
    so it has no row; the trace starts from its parent's record and the pending instance (rtla_trace's
    viol_parent / viol_inst + 1 case).  Run-time compact kernel, one shard and two (the wave kernel's case
    runs with the other RTLA_XFLAGS=2048 cases)."""
    smp, roots, v = out_of_model_roots(inv)
    cfg = cfg_of(sr.N2, (inv,), shards=shards)
    res = sr.run_job(sr.job(cfg, smp, roots))
    check_exact(res, smp, roots, v, BIT[inv], BIT[inv], in_model=False)
    assert sr.family(res["trace"][1][0]) == "HandleAppendEntriesRequest"


# ---- several bits

def test_mask_of_several_bits_is_reported_whole():
    """All five invariants, all-quiet roots and one root whose single violating successor violates at least
    two: the raw mask is that successor's whole py_mask, the name the lowest bit's."""
    smp = smp_of(sr.CFG2)
    several = smp.several()
    assert several, "the sample has a successor violating two invariants at once"
    v = several[0]
    u, = smp.violators(v, sr.ALL_MASK)
    roots = sr.place(smp.quiet(sr.ALL_MASK), v, "at 64")
    res = sr.run_job(sr.job(cfg_of(sr.CFG2, ALL), smp, roots))
    print("successor mask", u.mask, rtla.inv_names(u.mask))
    assert res["status"] == [rtla.OK, rtla.VIOLATION]
    assert res["mask"] == u.mask and bin(u.mask).count("1") >= 2 and res["in_model"] is u.in_model
    assert res["violation"] == rtla.inv_names(u.mask)[0]
    assert res["trace"][0][1] == smp.texts[v] and res["trace"][1][1] == u.text


# ---- many violators: membership

def check_member(res, vc, root_texts, ref, mask):
    """The reported violation is one of the reference's at its level; the trace is a chain of oracle steps."""
    assert ref.viol_level is not None
    assert res["status"] == [rtla.OK] * (ref.viol_level - 1) + [rtla.VIOLATION]
    tr = res["trace"]
    assert len(tr) == ref.viol_level
    assert tr[0][0] == "Initial predicate" and tr[0][1] in root_texts
    for (_, a), (lab, b) in zip(tr, tr[1:]):
        assert sr.is_oracle_step(vc, a, lab, b), lab
    assert (tr[-2][1], tr[-1][1], res["mask"], res["in_model"]) in ref.violations
    assert res["mask"] & mask == res["mask"] != 0


@pytest.mark.parametrize("shards", [0, 2])
@pytest.mark.parametrize("inv", ALL)
def test_many_violators_report_one_of_them(inv, shards):
    """The first 200 rows clean on the invariant, quiet or not: many violating steps race; whichever wins is
    one of the reference's (parent, successor, mask, in_model) at level 2."""
    smp = smp_of(sr.CFG2)
    roots = smp.clean(BIT[inv])[:200]
    ref = sr.ref_search(smp.vc, [smp.states[k] for k in roots], BIT[inv], 2)
    assert ref.viol_level == 2 and len(ref.violations) > 3
    res = sr.run_job(sr.job(cfg_of(sr.CFG2, (inv,), shards=shards), smp, roots))
    print("%d violating steps in the reference; reported mask %d in_model %s" % (
        len(ref.violations), res["mask"], res["in_model"]))
    check_member(res, smp.vc, {smp.texts[k] for k in roots}, ref, BIT[inv])
    assert [tuple(x) for x in res["levels"]] == ref.levels


# ---- one level further down

@functools.lru_cache(maxsize=None)
def level3_case():
    smp = smp_of(sr.N2)
    roots = [k for k in smp.quiet(sr.ALL_MASK)
             if smp.headroom(k) >= 2 and sr.clean_below(smp.vc, smp.states[k], 0, 2)][:48]
    return smp, roots, sr.ref_search(smp.vc, [smp.states[k] for k in roots], sr.ALL_MASK, 3)


def test_violation_one_level_further_down():
    """48 all-quiet roots of the narrow shape, all five invariants: level 2 is clean by construction, and the
    reference finds level 3's violations (the sample yields them: asserted).  The search reports one of
    them with a three-row trace, after a level 2 of the reference's counts."""
    smp, roots, ref = level3_case()
    assert len(roots) == 48 and ref.viol_level == 3, ref.levels
    res = sr.run_job(sr.job(cfg_of(sr.N2, ALL), smp, roots, steps=2))
    print("reference levels", ref.levels, "violating steps", len(ref.violations))
    check_member(res, smp.vc, {smp.texts[k] for k in roots}, ref, sr.ALL_MASK)
    assert [tuple(x) for x in res["levels"]] == ref.levels


# ---- no false positive, and counts

@functools.lru_cache(maxsize=None)
def counts_case():
    smp = smp_of(sr.CFG2)
    deep = list(sr.deep_quiet(*sr.CFG2, sr.ROWS[sr.CFG2], 96))
    roots = deep + deep[3::12][:8]
    return smp, roots, sr.ref_search(smp.vc, [smp.states[k] for k in roots], sr.ALL_MASK, 3)


@pytest.mark.parametrize("names", [ALL, sr.COMPILED_MASK[sr.CFG2]], ids=["run-time", "compiled-in"])
def test_no_false_positive_and_counts(names):
    """96 roots from which two levels violate nothing, 8 of them given twice: the status stays OK, and each
    level's (new, generated) and state texts are the reference's -- on the run-time kernel (five-bit mask) and
    on the compiled-in CFG2."""
    smp, roots, ref = counts_case()
    assert len(roots) == 104 and ref.viol_level is None and ref.levels[0] == (96, 104)
    res = sr.run_job(sr.job(cfg_of(sr.CFG2, names), smp, roots, steps=2, frontiers=True))
    assert res["status"] == [rtla.OK] * 3 and res["mask"] == 0 and res["violation"] is None
    assert [tuple(x) for x in res["levels"]] == ref.levels
    assert res["texts"] == ref.texts


# ---- roots that violate

@pytest.mark.parametrize("shards", [0, 2])
@pytest.mark.parametrize("inv", ALL)
def test_roots_that_violate_end_the_search_at_init(inv, shards):
    """Entries 5 and 70 of the root list violate the invariant: init returns VIOLATION, and the trace is
    entry 5's row alone."""
    smp = smp_of(sr.CFG2)
    bad = [k for k in range(len(smp.rows)) if smp.masks[k] & BIT[inv]]
    quiet = smp.quiet(BIT[inv])[:140]
    assert len(bad) >= 2 and len(quiet) == 140
    roots = quiet[:5] + [bad[0]] + quiet[5:69] + [bad[1]] + quiet[69:]
    assert roots[5] == bad[0] and roots[70] == bad[1]
    res = sr.run_job(sr.job(cfg_of(sr.CFG2, (inv,), shards=shards), smp, roots))
    assert res["status"] == [rtla.VIOLATION] and res["mask"] == BIT[inv] and res["in_model"] is True
    assert res["trace"] == [["Initial predicate", smp.texts[bad[0]]]]
    assert res["levels"] == [[len(roots), len(roots)]]


# ---- the edges of the API

def flat(rows):
    return rtla._flat_rows(rows, len(rows[0]))[0]


def test_init_rows_argument_and_order_errors(tmp_path):
    cfg = cfg_of(sr.CFG2, ("LogMatching",))
    smp = smp_of(sr.CFG2)
    rows = [list(smp.rows[k]) for k in smp.quiet(BIT["LogMatching"])[:10]]
    with rtla.Checker(cfg) as ck:
        assert rtla._lib.rtla_init_rows(ck._h, flat(rows), 0, None) == rtla.E_ARG
        assert rtla._lib.rtla_init_rows(ck._h, None, 3, None) == rtla.E_ARG
        assert ck.init(rows) == rtla.OK
        assert rtla._lib.rtla_init_rows(ck._h, flat(rows), len(rows), None) == rtla.E_STATE  # a second init
        assert rtla._lib.rtla_init(ck._h, None) == rtla.E_STATE
        with pytest.raises(rtla.RtlaError) as e:
            ck.checkpoint(str(tmp_path / "ckpt"))  # no checkpoint holds the roots
        assert e.value.status == rtla.E_STATE and not os.listdir(tmp_path)
        assert ck.step() == rtla.OK


def test_reset_forgets_the_roots():
    """reset, then a plain init: Init's level 1, and five levels of the golden counts."""
    g = GOLD["n2_v2_t3_l2_m1"]
    cfg = rtla.Config(g["n_server"], g["n_value"], g["max_term"], g["max_log"], g["max_copies"], g["max_msgs"],
                      tuple(g["invariants"]), **MEM)
    with rtla.Checker(cfg) as ck:
        rows = [r for r in rtla.random_rows(cfg, 0, 300) if not rtla.invariants_violated(cfg, r)][:70]
        assert len(rows) == 70 and ck.init(rows) == rtla.OK and ck.levels[0].generated == 70
        assert ck.step() in (rtla.OK, rtla.VIOLATION)  # (random rows: the set and the arena are in use either way)
        ck.reset()
        assert ck.init() == rtla.OK
        assert rtla.state_text(cfg, ck.frontier()[0]) == rtla.state_text(cfg, rtla.init_row(cfg))
        for _ in range(4):
            assert ck.step() == rtla.OK
        assert [[lv.new, lv.generated] for lv in ck.levels] == g["levels"][:5]


def test_init_rows_refuses_several_ranks(tmp_path):
    """world > 1: RTLA_E_STATE, on every rank.  Two ranks over the shared-memory transport, each a fresh
    process given the communicator id in a file written beforehand."""
    import subprocess
    import sys
    idfile = str(tmp_path / "comm_id")
    with open(idfile, "wb") as f:
        f.write(os.urandom(128))  # (this transport's id only names the shared-memory segment)
    code = ("import sys, ctypes as C, rtla; rank = int(sys.argv[1]); cid = open(sys.argv[2], 'rb').read();"
            "cfg = rtla.Config(3, 1, 2, 1, 1, 1, ('NoTwoLeaders',), fpset_log2=16, mem_budget=1 << 29);"
            "row = rtla.init_row(cfg); ck = rtla.Checker(cfg, rank=rank, world=2, comm_id=cid);"
            "print(rtla._lib.rtla_init_rows(ck._h, (C.c_uint32 * len(row))(*row), 1, None), ck.init()); ck.close()")
    env = dict(os.environ, RTLA_TRANSPORT="shm", RTLA_SHM_SLOT_MB="32",
               PYTHONPATH=os.pathsep.join([os.path.dirname(rtla.__file__), os.environ.get("PYTHONPATH", "")]))
    procs = [subprocess.Popen([sys.executable, "-c", code, str(r), idfile], env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True) for r in range(2)]
    for p in procs:
        o, e = p.communicate(timeout=120)
        assert p.returncode == 0, e[-2000:]
        assert o.split() == [str(rtla.E_STATE), str(rtla.OK)]


def chain_is_rooted(cfg, vc, trace, root_texts):
    assert trace[0][0] == "Initial predicate" and trace[0][1] in root_texts
    for (_, a), (lab, b) in zip(trace, trace[1:]):
        assert sr.is_oracle_step(vc, a, lab, b), lab


def test_audit_trace_starts_at_a_root():
    """audit(succ=True) after one seeded step of a search that checks nothing itself (the roots of the level-3
    case: level 2's successors violate): its counterexample is a root, one of its successors, and that state's
    violating successor -- one of the reference's."""
    smp, roots, ref = level3_case()
    cfg = cfg_of(sr.N2, ())
    with rtla.Checker(cfg) as ck:
        assert ck.init([smp.rows[k] for k in roots]) == rtla.OK and ck.step() == rtla.OK
        res = ck.audit(ALL, succ=True)
        assert res.status == rtla.VIOLATION and ref.viol_level == 3
        tr = ck.trace()
    assert len(tr) == 3
    chain_is_rooted(cfg, smp.vc, tr, {smp.texts[k] for k in roots})
    assert (tr[1][1], tr[2][1], res.viol_mask, res.viol_in_model) in ref.violations


def test_simulation_trace_starts_at_a_root():
    """simulate from a seeded level 1: the walk's counterexample starts at the root it set out from."""
    smp = smp_of(sr.CFG2)
    roots = smp.clean(sr.ALL_MASK)[:100]
    cfg = cfg_of(sr.CFG2, ALL)
    with rtla.Checker(cfg) as ck:
        assert ck.init([smp.rows[k] for k in roots]) == rtla.OK
        res = ck.simulate(len(roots), 3)
        assert res.status == rtla.VIOLATION, "some of 100 clean rows has a violating successor"
        tr = ck.trace()
    assert len(tr) == res.viol_step + 1
    assert tr[0][1] == smp.texts[roots[res.viol_walk % len(roots)]]
    chain_is_rooted(cfg, smp.vc, tr, {smp.texts[k] for k in roots})
    assert py_mask(smp.vc, tla_text.parse_state(smp.vc, tr[-1][1])) & res.viol_mask == res.viol_mask != 0
