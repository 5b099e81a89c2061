"""The multi-shard driver's level-end plans (raft-tla_amd/csrc/rtla_plan.h,
compiled for the host by tests/hostmodel.py) against a re-statement of their
rules in Python: which rows rebalance moves to even out the shards' next
levels, and where rehome puts the rows each shard built for another owner.
Every rank computes these plans on its own from the same reduced counts, so
they must be functions of their inputs alone.  No GPU."""
import pytest

import hostmodel


def targets(n):
    G, total = len(n), sum(n)
    return [total // G + (1 if k < total % G else 0) for k in range(G)]


def rebalance_rule(n):
    """Skipped while the largest excess over the even split is within 1 % + 64
    rows; else greedy in shard order: the first shard above its target sends
    its last rows to the first shard below its own."""
    G, total, tgt = len(n), sum(n), targets(n)
    m, moves = list(n), []
    if max(max(n[k] - tgt[k], 0) for k in range(G)) <= 64 + total // (100 * G):
        return moves, m
    a = b = 0
    while True:
        while a < G and m[a] <= tgt[a]:
            a += 1
        while b < G and m[b] >= tgt[b]:
            b += 1
        if a >= G or b >= G:
            return moves, m
        c = min(m[a] - tgt[a], tgt[b] - m[b])
        moves.append((a, b, m[a] - c, m[b], c))
        m[a] -= c
        m[b] += c


def rehome_rule(rows_cap, expm, room, n):
    """Each export count min(expm[a][b], rows_cap), in (a, b) order, lands at b
    if it fits b's room, else stays at a if it fits a's, else the plan is full."""
    G, n, moves, full = len(n), list(n), [], False
    for a in range(G):
        for b in range(G):
            c = min(expm[a][b], rows_cap)
            if not c:
                continue
            dst = b if n[b] + c <= room[b] else a if n[a] + c <= room[a] else None
            if dst is None:
                full = True
                continue
            moves.append((a, b, dst, n[dst], c))
            n[dst] += c
    return (None if full else moves), n


# The 64-row allowance of the skip rule puts the smallest level that moves
# anything at a few hundred rows.
UNEVEN = [
    [300, 0], [0, 301], [267, 133],
    [400, 0, 0], [10, 500, 11], [0, 0, 333], [250, 251, 2],
    [900, 0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 803], [300, 5, 280, 0, 7, 310, 1, 2],
    [120, 119, 118, 500, 0, 121, 117, 3],
]
EVEN = [
    [30, 20], [0, 64], [266, 134],           # 266 - 200 == 64 + 400 // 200: still within the rule
    [40, 0, 25], [100, 36, 35],              # 100 - 57 == 43
    [70, 0, 0, 0, 0, 0, 0, 0], [9, 8, 7, 6, 5, 4, 3, 2], [0] * 8,
]


@pytest.mark.parametrize("n", EVEN, ids=str)
def test_rebalance_leaves_an_even_enough_split_alone(n):
    moves, m = hostmodel.plan_rebalance(len(n), n)
    assert moves == [] and m == n
    assert (moves, m) == rebalance_rule(n)


@pytest.mark.parametrize("n", UNEVEN, ids=str)
def test_rebalance_evens_out_by_moving_last_rows(n):
    G = len(n)
    moves, m = hostmodel.plan_rebalance(G, n)
    assert (moves, m) == rebalance_rule(n)
    assert moves and m == targets(n) and sum(m) == sum(n)
    for k in range(G):
        sent = sorted((first, first + cnt) for a, _, first, _, cnt in moves if a == k)
        got = sorted((base, base + cnt) for _, b, _, base, cnt in moves if b == k)
        assert not (sent and got)  # a shard above its target only sends, one below only receives
        # the ranges tile [m, n) -- the end of the sender's level -- and [n, m) -- the end of the receiver's
        for ranges, lo, hi in ((sent, m[k], n[k]), (got, n[k], m[k])):
            if ranges:
                assert ranges[0][0] == lo and ranges[-1][1] == hi
                assert all(r[1] == s[0] and r[0] < r[1] for r, s in zip(ranges, ranges[1:] + [(hi, hi + 1)]))
    assert hostmodel.plan_rebalance(G, n) == (moves, m)


def test_rebalance_threshold_is_one_percent_plus_64_rows():
    assert hostmodel.plan_rebalance(2, [266, 134])[0] == []
    assert hostmodel.plan_rebalance(2, [267, 133])[0] == [(0, 1, 200, 133, 67)]


def grid(G, pairs):
    e = [[0] * G for _ in range(G)]
    for (a, b), c in pairs.items():
        e[a][b] = c
    return e


# (rows_cap, expm, room, n)
REHOME = [
    (16, grid(2, {(0, 1): 5, (1, 0): 7}), [40, 40], [10, 12]),                     # all fit at their owner
    (16, grid(2, {(0, 1): 5, (1, 0): 7}), [40, 14], [10, 12]),                     # owner 1 is full: 0 keeps its rows
    (16, grid(2, {(0, 1): 5, (1, 0): 7}), [12, 14], [10, 12]),                     # neither has room: full
    (4, grid(2, {(0, 1): 9, (1, 0): 3}), [40, 40], [0, 0]),                        # counts past rows_cap are capped
    (16, grid(3, {(0, 1): 6, (0, 2): 6, (1, 2): 6, (2, 0): 1}), [30, 30, 20], [9, 9, 9]),   # 2 takes one, not two
    (16, grid(3, {(0, 1): 16, (1, 0): 16, (2, 1): 16}), [48, 40, 16], [0, 8, 0]),
    (8, grid(8, {(a, (a + 3) % 8): a + 1 for a in range(8)}), [24] * 8, [4 * (k % 3) for k in range(8)]),
    (8, grid(8, {(a, b): (a * b) % 5 for a in range(8) for b in range(8) if a != b}), [30] * 8, [3] * 8),
    (8, grid(8, {(a, 7): 6 for a in range(7)}), [64] * 7 + [20], [2] * 8),         # owner 7 fills up half way
    (8, grid(8, {}), [10] * 8, [1] * 8),                                           # nothing exported
]


@pytest.mark.parametrize("case", REHOME, ids=lambda c: "G%d_cap%d_%d" % (len(c[3]), c[0], sum(map(sum, c[1]))))
def test_rehome_places_each_export_at_its_owner_else_its_sender(case):
    rows_cap, expm, room, n = case
    G = len(n)
    moves, after = hostmodel.plan_rehome(G, rows_cap, expm, room, n)
    assert (moves, after) == rehome_rule(rows_cap, expm, room, n)
    assert hostmodel.plan_rehome(G, rows_cap, expm, room, n) == (moves, after)
    if moves is None:
        return
    at = list(n)  # next-level states of each shard as the plan goes
    todo = [(a, b) for a in range(G) for b in range(G) if expm[a][b]]
    assert [(a, b) for a, b, _, _, _ in moves] == todo
    for a, b, dst, base, cnt in moves:
        assert cnt == min(expm[a][b], rows_cap)
        assert dst == (b if at[b] + cnt <= room[b] else a) and at[dst] + cnt <= room[dst]
        assert base == at[dst]  # contiguous from n[dst]
        at[dst] += cnt
    assert at == after


def test_rehome_cases_cover_every_outcome():
    got = [rehome_rule(*c)[0] for c in REHOME]
    assert any(m is None for m in got)
    assert any(m and all(dst == b for _, b, dst, _, _ in m) for m in got)
    assert any(m and any(dst == a != b for a, b, dst, _, _ in m) for m in got)
    assert any(m == [] for m in got)
