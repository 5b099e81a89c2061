"""CPU tests of the random-walk simulation's host side (rtla_sim_replay /
rtla_sim_walk: the reference the GPU walks are compared with).  The draw is
re-derived here from its published formulas, the successors come from the
host-compiled model (hostmodel) and every step is checked against the value
oracle (raft_values), so the walk semantics are pinned without a GPU."""
import pytest

import hostmodel
import limits
import raft_values as rv
import rtla
import tla_text

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
SHAPES = [(2, 1, 3, 1, 2, 0), (3, 2, 3, 2, 1, 3), (5, 1, 3, 2, 1, 3)]
SEED = 20251019


def mix_a(z):  # splitmix64 finalizer
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def mix_b(z):  # murmur3 fmix64
    z = ((z ^ (z >> 33)) * 0xFF51AFD7ED558CCD) & M64
    z = ((z ^ (z >> 33)) * 0xC4CEB9FE1A85EC53) & M64
    return z ^ (z >> 33)


def draw(seed, w, t, n):
    """The t-th below(n) of SynthRng{mix_b(seed * G ^ mix_a(w + C)), 0}."""
    base = mix_b(((seed * GOLDEN) & M64) ^ mix_a((w + 0x243F6A8885A308D3) & M64))
    nxt = mix_a((base + GOLDEN * t) & M64)
    return ((nxt >> 32) * n) >> 32


def path_term(fp, t):  # rtla_sim.h sim_path_term
    return mix_a(fp[0] ^ mix_b((fp[1] + t * GOLDEN) & M64))


def python_walk(cfg, words, start, w, depth, seed, flip_at=None):
    """The walk from hostmodel's successors and the Python draw:
    [(instance, row)] -- flip_at: at that step take the next in-model
    successor that is another state (from Init every Restart is a no-op)."""
    row, out = start, []
    for t in range(1, depth + 1):
        model = [x for x in hostmodel.expand(cfg, [row], words) if x[3]]
        assert [x[1] for x in model] == sorted(x[1] for x in model)
        if not model:
            break
        k = draw(seed, w, t, len(model))
        if t == flip_at:
            k = next(j % len(model) for j in range(k + 1, k + len(model)) if model[j % len(model)][4] != model[k][4])
        row = model[k][4]
        out.append((model[k][1], row))
    return out


def digest_of(rows):
    return sum(path_term(rtla.stored_fingerprint(r), t + 1) for t, r in enumerate(rows)) & M64


@pytest.mark.parametrize("shape", SHAPES)
def test_walks_match_independent_rederivation(shape):
    n, v, t, l, c, m = shape
    cfg = rtla.Config(n, v, t, l, c, m, ())
    vcfg = rv.Cfg(n, v, t, l, c, (), m)
    words = rtla.row_words(cfg)
    init = rtla.init_row(cfg)
    ends = rtla.sim_replay(cfg, [init], 20, 30, seed=SEED).ends
    for w in range(20):
        violating, steps = rtla.sim_walk(cfg, init, w, 30, seed=SEED)
        mine = python_walk(cfg, words, init, w, 30, SEED)
        assert not violating and len(steps) == 30
        assert [(i, r) for i, _, r in steps] == mine
        prev = tla_text.parse_state(vcfg, rtla.state_text(cfg, init))
        for _, _, row in steps:
            cur = tla_text.parse_state(vcfg, rtla.state_text(cfg, row))
            assert rv.in_model(vcfg, cur) and cur in [s for _, s in rv.next_states(vcfg, prev)]
            prev = cur
        # the end record is the walk's: length, last fingerprint, stop code, path digest
        assert ends[w] == rtla.stored_fingerprint(steps[-1][2]) + (digest_of([r for _, _, r in steps]), 30, 0)


def test_walks_from_limit_shape_rows_match_independent_rederivation():
    """The same re-derivation at the row format's limits (tests/limits.py: 3-bit terms, 2-bit values,
    counts up to 14), walk w started from a row of the sample instead of Init: the rows whose bag and
    election list have room for one more entry per step (a walk that fills either is a capacity error)."""
    c = limits.case("n3_v4_t6_c14")
    limits.assert_witnessed(c, "walks")
    cfg, words, depth = c.cfg, len(c.rows[0]), 8
    room = [k for k, s in enumerate(c.states) if len(s[rv.IX["messages"]]) + depth < c.K
            and len(s[rv.IX["elections"]]) + depth < c.E]
    rows, walks = [list(c.rows[k]) for k in room], len(room)
    assert walks >= 12
    ends = rtla.sim_replay(cfg, rows, walks, depth, seed=SEED).ends
    lengths = []
    for w in range(walks):
        violating, steps = rtla.sim_walk(cfg, rows[w], w, depth, seed=SEED)
        mine = python_walk(cfg, words, rows[w], w, depth, SEED)
        assert not violating and [(i, r) for i, _, r in steps] == mine
        prev = c.states[room[w]]
        for _, _, row in steps:
            cur = tla_text.parse_state(c.vc, rtla.state_text(cfg, row))
            assert rv.in_model(c.vc, cur) and cur in [s for _, s in rv.next_states(c.vc, prev)]
            prev = cur
        stop = rtla.SIM_STOP_DEPTH if len(steps) == depth else rtla.SIM_STOP_STUCK
        last = steps[-1][2] if steps else rows[w]
        assert ends[w] == rtla.stored_fingerprint(last) + (digest_of([r for _, _, r in steps]), len(steps), stop)
        lengths.append(len(steps))
    assert sum(lengths) > walks * depth // 2, lengths


def test_path_digest_sees_one_changed_intermediate_pick():
    cfg = rtla.Config(3, 2, 3, 2, 1, 3, ())
    words = rtla.row_words(cfg)
    init = rtla.init_row(cfg)
    want = rtla.sim_replay(cfg, [init], 1, 12, seed=SEED, first=3).ends[0]
    base = [r for _, r in python_walk(cfg, words, init, 3, 12, SEED)]
    assert digest_of(base) == want[2]
    for at in (1, 6, 11):
        other = [r for _, r in python_walk(cfg, words, init, 3, 12, SEED, flip_at=at)]
        assert other[at - 1] != base[at - 1] and digest_of(other) != want[2]
    # the same states entered at other steps do not give the digest either
    assert digest_of(base[1:] + base[:1]) != want[2]


def test_replay_is_independent_of_threads_and_of_how_the_range_is_split():
    cfg = rtla.Config(3, 2, 3, 2, 1, 3, ())
    init = rtla.init_row(cfg)
    one = rtla.sim_replay(cfg, [init], 300, 25, seed=SEED, first=11, threads=1)
    many = rtla.sim_replay(cfg, [init], 300, 25, seed=SEED, first=11, threads=16)
    assert one.ends == many.ends and len(set(one.ends)) > 250
    assert (one.steps, one.generated, one.stuck, one.taken) == (many.steps, many.generated, many.stuck, many.taken)
    assert one.steps == 300 * 25 == sum(one.taken.values()) and one.status == rtla.OK
    a = rtla.sim_replay(cfg, [init], 120, 25, seed=SEED, first=11)
    b = rtla.sim_replay(cfg, [init], 180, 25, seed=SEED, first=131)
    assert a.ends + b.ends == one.ends
    assert a.steps + b.steps == one.steps and a.generated + b.generated == one.generated
    assert {k: a.taken[k] + b.taken[k] for k in a.taken} == one.taken
    assert rtla.sim_replay(cfg, [init], 300, 25, seed=SEED + 1, first=11).ends != one.ends


def test_walks_start_at_row_w_mod_n():
    cfg = rtla.Config(3, 2, 3, 2, 1, 3, ())
    words = rtla.row_words(cfg)
    init = rtla.init_row(cfg)
    rows = [list(r) for r in sorted({tuple(x[4]) for x in hostmodel.expand(cfg, [init], words) if x[3]})][:2]
    assert len(rows) == 2 and rows[0] != rows[1]
    both = rtla.sim_replay(cfg, rows, 10, 8, seed=SEED, first=5).ends
    for k, w in enumerate(range(5, 15)):
        assert both[k] == rtla.sim_replay(cfg, [rows[w % 2]], 1, 8, seed=SEED, first=w).ends[0]
        steps = rtla.sim_walk(cfg, rows[w % 2], w, 8, seed=SEED)[1]
        assert both[k][:2] == rtla.stored_fingerprint(steps[-1][2])
    assert rtla.sim_replay(cfg, rows, 3, 0, seed=SEED, first=5).ends == [
        rtla.stored_fingerprint(rows[w % 2]) + (0, 0, 0) for w in (5, 6, 7)]


def test_violating_walk_ends_at_its_least_violating_successor():
    """From a state with one leader and a second candidate holding a quorum,
    BecomeLeader violates NoTwoLeaders: found by walking from BFS-free start
    rows is rare, so the start row is built by hostmodel steps."""
    cfg = rtla.Config(3, 1, 3, 1, 1, 0, ("NoTwoLeaders",))
    words = rtla.row_words(cfg)

    def step(row, name):
        for _, inst, sub, _, r in hostmodel.expand(cfg, [row], words):
            if rtla.action_name(cfg, inst, sub) == name:
                return r
        raise AssertionError(name)

    def drain(row):  # deliver messages (first Receive instance first) until none is left
        for _ in range(32):
            recv = [r for _, inst, sub, _, r in hostmodel.expand(cfg, [row], words)
                    if rtla.action_name(cfg, inst, sub).startswith("Receive")]
            if not recv:
                return row
            row = recv[0]
        raise AssertionError("messages never drain")

    row = rtla.init_row(cfg)
    for name in ("Timeout(s1)", "RequestVote(s1, s1)", "RequestVote(s1, s2)"):
        row = step(row, name)
    row = step(drain(row), "BecomeLeader(s1)")  # votes of s1 and s2, term 2
    # s3 times out twice (term 3 > s1's term 2) and wins the votes of s3 and s2
    for name in ("Timeout(s3)", "Timeout(s3)", "RequestVote(s3, s3)", "RequestVote(s3, s2)"):
        row = step(row, name)
    row = drain(row)
    succ = hostmodel.expand(cfg, [row], words)
    bad = [x for x in succ if rtla.invariants_violated(cfg, x[4])]
    assert bad and rtla.action_name(cfg, bad[0][1], bad[0][2]) == "BecomeLeader(s3)"
    res = rtla.sim_replay(cfg, [row], 5, 10, seed=SEED, first=2)
    assert res.status == rtla.VIOLATION and res.violation == "NoTwoLeaders"
    assert (res.viol_walk, res.viol_step, res.viol_inst, res.viol_mask) == (2, 1, bad[0][1], 1)
    assert res.generated == 5 * len(succ) and res.steps == 0
    assert res.ends == [rtla.stored_fingerprint(row) + (0, 0, rtla.SIM_STOP_VIOLATION)] * 5
    violating, steps = rtla.sim_walk(cfg, row, 2, 10, seed=SEED)
    assert violating and [(i, r) for i, _, r in steps] == [(bad[0][1], bad[0][4])]
