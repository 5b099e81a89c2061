"""CPU tests of the seeded search's reference (tests/seedref.py) and of what rtla_init_rows refuses without a
kernel.  The reference is checked against itself and the value oracle's own BFS; every root set that
tests/test_seed_gpu.py builds is shown to exist in the generator's samples, so a GPU run cannot pass for want
of inputs."""

import pytest

import limits
import raft_values as rv
import rtla
import seedref as sr
import tla_text

BIT = rtla.INV_BITS
ALL = sr.ALL

# rows, all-quiet, single-in per invariant (bit order): the generator's default seed, ids 0..n-1
TABLE = {sr.CFG2: (1200, 196, (60, 20, 128, 53, 69)),
         sr.SYNTH: (1200, 104, (85, 15, 95, 33, 73)),
         sr.N2: (500, 243, (10, 5, 29, 12, 13))}


@pytest.mark.parametrize("layout", list(TABLE), ids=lambda p: "n%d_t%d" % (p[0][0], p[0][2]))
def test_samples_classify_as_measured(layout):
    """The classification is a function of the generator and the value oracle alone; a change in either shows
    here before it silently empties a root set.  No row of these samples has an out-of-model single violator."""
    n, all_quiet, single_in = TABLE[layout]
    assert sr.ROWS[layout] == n
    smp = sr.sample(*layout, n)
    assert len(smp.quiet(sr.ALL_MASK)) == all_quiet
    assert tuple(len(smp.single(b)) for b in BIT.values()) == single_in
    assert [smp.single(b, in_model=False) for b in BIT.values()] == [[]] * 5
    for b in BIT.values():  # the classes are what their names say
        for k in smp.quiet(b)[:50]:
            assert not smp.masks[k] & b and not any(u.mask & b for u in smp.succ[k])
        for k in smp.single(b):
            assert not smp.masks[k] & b and sum(1 for u in smp.succ[k] if u.mask & b) == 1


def test_classification_agrees_with_the_value_oracle_directly():
    smp = sr.sample(*sr.N2, sr.ROWS[sr.N2])
    from test_safety_host import py_mask
    for k in range(0, len(smp.rows), 37):
        s = tla_text.parse_state(smp.vc, rtla.state_text(smp.cfg, list(smp.rows[k])))
        assert smp.texts[k] == rv.state_text(smp.vc, s) and smp.masks[k] == py_mask(smp.vc, s)
        ref = [(lab, rv.state_text(smp.vc, t), rv.in_model(smp.vc, t), py_mask(smp.vc, t))
               for lab, t in rv.next_states(smp.vc, s)]
        assert [(u.label, u.text, u.in_model, u.mask) for u in smp.succ[k]] == ref


@pytest.mark.parametrize("inv", list(sr.SINGLE_OUT))
def test_pinned_single_out_rows(inv):
    """The four pinned rows (two ids, each single-out for both invariants) are what seedref says: clean, one
    violating successor, out of the model by a message count of MaxCopies + 1, made by
    HandleAppendEntriesRequest."""
    n = sr.ROWS[sr.N2]
    smp = sr.sample(*sr.N2, n, extra=sr.SINGLE_OUT[inv])
    pinned = list(range(n, len(smp.rows)))
    assert len(pinned) == 2 and [smp.ids[k] for k in pinned] == list(sr.SINGLE_OUT[inv])
    assert [k for k in smp.single(BIT[inv], in_model=False)] == pinned
    for k in pinned:
        u, = smp.violators(k, BIT[inv])
        assert sr.family(u.label) == "HandleAppendEntriesRequest" and not u.in_model
        assert max(c for _, c in u.state[rv.IX["messages"]].items()) == smp.vc.max_copies + 1
    assert len(smp.quiet(BIT[inv])) >= 129


@pytest.mark.parametrize("layout", list(sr.COMPILED_MASK), ids=lambda p: "n%d_t%d_k%d" % (p[0][0], p[0][2], p[1]))
def test_compiled_in_layouts_have_their_root_sets(layout):
    """For each compiled-in layout and each invariant of its mask: 129 rows quiet for the whole mask and a row
    whose single violating successor violates that invariant alone of the mask -- CFG1 and EXHAUST included
    (so no instantiation is left to the membership form)."""
    mask = rtla.inv_mask_of(sr.COMPILED_MASK[layout])
    smp = sr.sample(*layout, sr.ROWS[layout])
    cfg = sr.configs(*layout, sr.COMPILED_MASK[layout])[0]
    assert limits.kernel_of(cfg)[0].startswith("compact")
    assert len(smp.quiet(mask)) >= 129
    for inv in sr.COMPILED_MASK[layout]:
        assert smp.single(mask, True, BIT[inv]), inv


def test_symmetry_root_sets_exist_per_orbit():
    smp = sr.sample(*sr.CFG4, sr.ROWS[sr.CFG4])
    sym = sr.configs(*sr.CFG4, symmetry=True)[0]
    assert limits.kernel_of(sym, symmetry=True)[0] == "compact32"
    for inv in ALL:
        quiet = sr.one_per_orbit(smp, smp.quiet(BIT[inv]))
        assert len(quiet) >= 129 and smp.single(BIT[inv]), inv
    # the host's orbit text, which tells the roots' orbits apart, is the value oracle's (a few rows: the
    # brute force over 120 images is slow), and a permuted image shares it
    for k in range(0, 60, 10):
        want = rv.orbit_text(smp.vc, smp.states[k])
        assert rtla.orbit_text(sym, list(smp.rows[k])) == want
        assert rtla.orbit_text(sym, rtla.permute_row(sym, list(smp.rows[k]), [2, 0, 4, 1, 3])) == want
    twin = rtla.permute_row(sym, list(smp.rows[0]), [1, 0, 2, 3, 4])
    assert rtla.orbit_key(sym, twin)[0] == rtla.orbit_key(sym, list(smp.rows[0]))[0]


@pytest.mark.parametrize("shards", [2, 3])
def test_shard_picks_exist(shards):
    """For every invariant, a single-in root whose violating successor its own shard owns and one whose
    successor another shard owns."""
    smp = sr.sample(*sr.CFG2, sr.ROWS[sr.CFG2])
    for inv in ALL:
        same, other = sr.shard_picks(*sr.CFG2, sr.ROWS[sr.CFG2], BIT[inv], shards)
        assert same is not None and other is not None and same != other, inv
        assert len(smp.quiet(BIT[inv])) >= 129


def test_other_root_sets_exist():
    smp = sr.sample(*sr.CFG2, sr.ROWS[sr.CFG2])
    several = smp.several()
    assert several
    u, = smp.violators(several[0], sr.ALL_MASK)
    assert bin(u.mask).count("1") >= 2
    for inv in ALL:
        assert len(smp.clean(BIT[inv])) >= 200
        assert sum(1 for m in smp.masks if m & BIT[inv]) >= 2  # two roots that violate it
    n2 = sr.sample(*sr.N2, sr.ROWS[sr.N2])
    for inv in ALL:
        assert len(n2.quiet(BIT[inv])) >= 129 and n2.single(BIT[inv])


def test_deep_quiet_roots_stay_clean_for_two_levels():
    smp = sr.sample(*sr.CFG2, sr.ROWS[sr.CFG2])
    deep = sr.deep_quiet(*sr.CFG2, sr.ROWS[sr.CFG2], 96)
    assert len(deep) == len(set(deep)) == 96
    roots = list(deep) + list(deep[3::12][:8])
    ref = sr.ref_search(smp.vc, [smp.states[k] for k in roots], sr.ALL_MASK, 3)
    assert ref.viol_level is None and ref.levels[0] == (96, 104) and len(ref.levels) == 3
    assert all(new > 0 and gen > new for new, gen in ref.levels[1:])
    assert all(t == sorted(set(t)) for t in ref.texts)


def test_narrow_roots_reach_a_violation_at_level_three():
    smp = sr.sample(*sr.N2, sr.ROWS[sr.N2])
    roots = [k for k in smp.quiet(sr.ALL_MASK)
             if smp.headroom(k) >= 2 and sr.clean_below(smp.vc, smp.states[k], 0, 2)][:48]
    ref = sr.ref_search(smp.vc, [smp.states[k] for k in roots], sr.ALL_MASK, 3)
    assert len(roots) == 48 and ref.viol_level == 3 and ref.violations
    for ptext, ttext, mask, im in ref.violations:
        assert ptext in ref.chains and ref.chains[ptext][0] in {smp.texts[k] for k in roots}
        assert mask and any(sr.is_oracle_step(smp.vc, ptext, u.label, ttext)
                            for u in sr.successors(smp.vc, tla_text.parse_state(smp.vc, ptext)) if u.text == ttext)


@pytest.mark.parametrize("symmetry", [False, True])
def test_ref_search_from_init_is_the_oracle_bfs(symmetry):
    """Seeded with Init alone, the reference is the value oracle's own BFS (and orbit BFS)."""
    vc = rv.Cfg(2, 2, 3, 2, 1, (), 1)
    want, _ = rv.bfs_prefix(vc, 6, symmetric=symmetry)
    ref = sr.ref_search(vc, [rv.init_state(vc)], sr.ALL_MASK, 6, symmetry=symmetry)
    assert ref.levels == [tuple(x) for x in want][:6] and ref.viol_level is None


def test_ref_search_counts_repeated_and_permuted_roots_once():
    vc = rv.Cfg(2, 1, 3, 1, 1, (), 1)
    init = rv.init_state(vc)
    a = next(t for lab, t in rv.next_states(vc, init) if lab == "Timeout(0)")
    b = rv.permute_state(a, [1, 0])
    assert a != b
    plain = sr.ref_search(vc, [a, b, a], 0, 1)
    assert plain.levels == [(2, 3)]
    assert sr.ref_search(vc, [a, b, a], 0, 1, symmetry=True).levels == [(1, 3)]


def test_families():
    assert sr.family("Receive -> UpdateTerm") == sr.family("Receive:UpdateTerm") == "UpdateTerm"
    assert sr.family("Timeout(s3)") == sr.family("Timeout(2)") == "Timeout"
    assert sr.family("DropMessage") == "DropMessage"
    assert sr.place(list(range(130)), 999, "at 64")[64] == 999 and sr.place([1, 2], 9, "last") == [1, 2, 9]
    assert [sr.owner(a, 3) for a in (0, 0x55555556, 0xAAAAAAAB, 0xFFFFFFFF, 1 << 32)] == [0, 1, 2, 2, 0]


def test_init_rows_refuses_without_a_context():
    """What needs no kernel: a null context (the errors of an open context are in test_seed_gpu.py), and the
    binding itself."""
    import ctypes as C
    cfg = rtla.Config(2, 1, 2, 1, 1, 1, ())
    row = rtla.init_row(cfg)
    arr = (C.c_uint32 * len(row))(*row)
    assert rtla._lib.rtla_init_rows(None, arr, 1, None) == rtla.E_ARG
    assert "rtla_init_rows" in rtla.EXPORTED and rtla._lib.rtla_abi_version() == 12
