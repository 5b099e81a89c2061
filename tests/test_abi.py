"""CPU tests of the C-ABI library: it loads, exports every symbol that
include/rtla.h declares, and its host-only helpers (row layout, Init row,
state printer) agree with the oracle.  No kernel is launched here."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "raft-tla_amd", "librtla.so")


def declared_symbols():
    hdr = open(os.path.join(ROOT, "include", "rtla.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(rtla_[a-z_0-9]+)\s*\(", hdr)))


def test_library_exports_every_declared_symbol():
    assert os.path.exists(LIB), "build librtla.so first (__graft_entry__.build())"
    nm = subprocess.check_output(["nm", "-D", "--defined-only", LIB]).decode()
    exported = set(re.findall(r"\bT (rtla_[a-z_0-9]+)", nm))
    missing = [s for s in declared_symbols() if s not in exported]
    assert not missing, missing
    lib = ctypes.CDLL(LIB)
    for s in declared_symbols():
        getattr(lib, s)


def test_python_mirror_binds_every_symbol():
    import rtla
    assert sorted(rtla.EXPORTED) == declared_symbols()
    assert rtla._lib.rtla_abi_version() == 12


def test_row_layout_and_config_errors():
    import rtla
    assert rtla.row_words(rtla.Config(3, 1, 2, 1, 1, 2)) % 2 == 1   # odd stride for LDS staging
    with pytest.raises(rtla.RtlaError):
        rtla.row_words(rtla.Config(n_server=6))
    with pytest.raises(rtla.RtlaError):
        rtla.row_words(rtla.Config(max_log=5))


def test_configuration_limits():
    """rtla_row_layout / rtla_row_words accept each maximum of the row format (rtla_model.h make_layout)
    and the two largest log universes under 1024, and refuse one step past each with RTLA_E_CONFIG."""
    import rtla

    def cfg(n=2, v=1, t=2, l=1, c=1, m=0, **kw):
        return rtla.Config(n, v, t, l, c, m, (), **kw)

    def universe(v, t, l):
        return sum((t * v) ** k for k in range(l + 1))

    for ok in (cfg(n=5), cfg(v=4), cfg(t=6), cfg(l=4), cfg(c=14), cfg(bag_cap=64), cfg(elec_cap=32),
               cfg(n=5, l=4, c=14, t=5, bag_cap=64, elec_cap=32), cfg(m=63, bag_cap=64), cfg(m=3, bag_cap=4)):
        lay = rtla.row_layout(ok)
        assert lay["W"] == rtla.row_words(ok) and lay["W"] % 2 == 1
        assert lay["slot_words"] <= 2 and lay["srv_words"] <= 6 and lay["elec_words"] <= 6
        assert len(rtla.init_row(ok)) == lay["W"]
    for v, t, l, logs in ((4, 6, 2, 601), (1, 5, 4, 781)):
        assert universe(v, t, l) == logs
        assert rtla.row_layout(cfg(v=v, t=t, l=l))["all_words"] == (logs + 31) // 32
    assert universe(1, 6, 4) == 1555 > 1024
    widest = rtla.row_layout(cfg(n=5, v=1, t=5, l=4, c=14, bag_cap=64, elec_cap=32))
    assert widest["W"] <= 4 + 1 + 5 * 6 + 32 + 32 * 6 + 2 * 64  # rtla_model.h WMAX
    for bad in (cfg(n=6), cfg(v=5), cfg(t=7), cfg(l=5), cfg(c=15), cfg(bag_cap=65), cfg(elec_cap=33),
                cfg(v=1, t=6, l=4), cfg(m=3, bag_cap=3), cfg(m=64, bag_cap=64), cfg(n=0), cfg(c=0)):
        for fn in (rtla.row_words, rtla.row_layout, rtla.init_row):
            with pytest.raises(rtla.RtlaError) as e:
                fn(bad)
            assert e.value.status == rtla.E_CONFIG, bad


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_init_row_text_matches_value_oracle(n):
    import raft_values as rv
    import rtla
    cfg = rtla.Config(n, 2, 3, 2, 1, 2)
    row = rtla.init_row(cfg)
    assert rtla.state_text(cfg, row) == rv.state_text(rv.Cfg(n, 2, 3, 2, 1), rv.init_state(rv.Cfg(n, 2, 3, 2, 1)))
    assert rtla.invariants_violated(rtla.Config(n, invariants=("NoTwoLeaders", "ElectionSafety", "LogMatching")), row) == 0


def test_action_names():
    import rtla
    cfg = rtla.Config(3, 2, 2, 1, 1, 2)
    assert rtla.action_name(cfg, 0, 6) == "Restart(s1)"
    assert rtla.action_name(cfg, 3 + 2, 6) == "Timeout(s3)"
    assert rtla.action_name(cfg, 6 + 1, 6) == "RequestVote(s1, s2)"


def test_open_refuses_more_shards_than_the_outbox_holds():
    """rtla_open checks the shard count before touching a device:
    more than SHARD_MAX = 8 owners would overflow the kernels' per-owner state."""
    import rtla
    for kw in ({"shards": 9}, {"shards": 16}):
        with pytest.raises(rtla.RtlaError) as e:
            rtla.Checker(rtla.Config(2, 1, 2, 1, 1, 1, **kw))
        assert e.value.status == -1


def test_rows_text_hash_is_the_oracle_digest():
    """rtla_rows_text_hash (host threads) = the sum of FNV-1a-64 of each row's
    text, the digest the C oracle records per level (raft_cpu.text_hash)."""
    import raft_cpu
    import rtla
    cfg = rtla.Config(3, 2, 4, 3, 2, 0, ("ElectionSafety",), bag_cap=12)
    rows = rtla.random_rows(cfg, 0, 3000, pool=500)
    want = sum(raft_cpu.text_hash(rtla.state_text(cfg, r)) for r in rows) & (2**64 - 1)
    assert rtla.rows_text_hash(cfg, rows) == want
    assert rtla.rows_text_hash(cfg, rows, threads=1) == want
    assert rtla.rows_text_hash(cfg, []) == 0


def test_owner_bits_are_a_function_of_the_projection():
    """The multi-GPU shard owner (fp_owner: the low 32 bits of the
    fingerprint's first half, rtla_model.h proj32) depends on serverVars +
    logVars only: removing a message from a row (a bag-only change) keeps
    those bits and changes the fingerprint; over random valid rows, equal
    currentTerm / state / votedFor / log / commitIndex lines give equal owner
    bits and different ones different bits.  Host code only (rtla_random_rows,
    rtla_row_fingerprint)."""
    import rtla
    cfg = rtla.Config(3, 2, 4, 3, 2, 0, (), bag_cap=12)  # the synthetic microbench's layout
    lay = rtla.row_layout(cfg)
    proj_vars = ("currentTerm", "state", "votedFor", "log", "commitIndex")
    by_proj, checked = {}, 0
    for r in rtla.random_rows(cfg, 0, 400):
        fa, fb = rtla.row_fingerprint(cfg, r)
        text = rtla.state_text(cfg, r)
        proj = tuple(ln for ln in text.split("\n") if ln[3:].split(" = ", 1)[0] in proj_vars)
        assert by_proj.setdefault(proj, fa & 0xFFFFFFFF) == fa & 0xFFFFFFFF
        nmsg = r[lay["off_hdr"]] & 0xFF
        if nmsg:
            q = list(r)
            last = lay["off_bag"] + (nmsg - 1) * lay["slot_words"]
            for w in range(lay["slot_words"]):
                q[last + w] = 0
            q[lay["off_hdr"]] = (q[lay["off_hdr"]] & ~0xFF) | (nmsg - 1)
            ga, gb = rtla.row_fingerprint(cfg, q)
            assert (ga & 0xFFFFFFFF) == (fa & 0xFFFFFFFF) and (ga, gb) != (fa, fb)
            assert rtla.state_text(cfg, q).split("\n", 1)[1:] == text.split("\n", 1)[1:]  # only the bag line moved
            checked += 1
    assert checked > 300
    assert len(set(by_proj.values())) == len(by_proj) > 300
