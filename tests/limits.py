"""TEST INFRASTRUCTURE: configurations at the limits of the packed row format
(rtla_model.h make_layout: |Server| <= 5, |Value| <= 4, MaxTerm <= 6, MaxLogLen
<= 4, MaxCopies <= 14, 64 bag slots, 32 election records, an allLogs universe
of <= 1024 logs), shared by the host tests (hostmodel, check_replay, the
predicate interpreter, the walks, the orbit key) and tests/test_limits_gpu.py.

A case is a sample of the synthetic generator's rows (rtla.random_rows) with,
from the VALUE ORACLE alone, each input parsed into a raft_values state and its
reference successors (raft_values.next_states).  `witnesses` counts, over those
oracle states, the values that sit at the end of a field's range; every case
must show every one of them (assert_witnessed), so no test over a case can pass
without the widest encodings having been produced and read.

Which level kernel expands a layout (rtla_klevel.h compact_group, rtla_kernels.hip
expand_compact_wpb), from W = row words and AW = allLogs words: the compacting
kernel's per-wave LDS tile is
    lds(G) = 4*(4G + 32 + 256 + G*W + G*AW + 64) bytes       (no SYMMETRY, multi-shard)
and a layout runs 64-state groups when lds(64) <= 16 KiB, else 32-state groups;
it falls to the wave-per-state kernel when lds(group) > 160 KiB or when its
action instances, rounded up to 64, exceed 256 (8-bit instance ids in the
pair ring and the new-state list).  Under SYMMETRY the group is always 32 and
the tile 4*(8G + 32 + 256 + G*W + G*AW + 128 + 320 + 15G) bytes.  By that rule
(checked by kernel_of below, and on the GPU through the driver's own choice):

    case              W    AW  instances  tile      kernel
    n5_l4_c14        175   25     135     26.9 KiB  compact, groups of 32
    n3_v4_t6_c14      95   19      90     16.1 KiB  compact, groups of 32
    n2_v3_l3_c7       69   26      58     13.8 KiB  compact, groups of 32   (lds(64) = 26.0 KiB)
    n3_t6_l3          77    9      69     12.6 KiB  compact, groups of 32   (lds(64) = 23.9 KiB)
    n2_l4_k64_e32    149   11     212     21.9 KiB  compact, groups of 32
    n4_v4_c9          83    9     112     13.4 KiB  compact, groups of 32   (lds(64) = 25.4 KiB)
    n4_v4_k64        103    5     256     15.4 KiB  compact, groups of 32: instance ids 0..255
    n5_k60           101    1     255     14.6 KiB  compact, groups of 32: instance ids 0..254
    n5_k61           103    1     258        --     wave-per-state (258 instances round up to 320)
    n5_k63           105    1     264        --     wave-per-state
(under SYMMETRY the two shapes that run it, n5_l4_c14 and n4_v4_c9, have tiles of 30.8 and 17.3 KiB.)
(No limit shape is narrow enough for 64-state groups, which need W + AW <= 54; those instantiations
are covered by tests/test_rowbuild_gpu.py.  Every tile is far below the 160 KiB bound: at these widths
only the instance count decides between the two kernels.)

The instance count is 4N + 2N^2 + N*V + 3K (make_layout's fam[]): at N = 5, V = 1
it is 75 + 3K, so 60 bag slots give 255 instances (the last 64-instance window
ends at id 254), 61 give 258 and 63 give 264; N = 4, V = 4 with 64 slots gives
exactly 256, DropMessage of slot 63 being instance 255.
"""
import collections
import dataclasses
import functools

import raft_values as rv
import rtla
import tla_text

# name: (shape (N, V, T, L, C, M), Config keywords, random rows, further generator ids, level kernel)
# The further ids are single states of the same generator (rtla.random_rows(cfg, id, 1)) chosen because
# the first rows alone miss a witness -- mostly the two capacity steps, which need an input with exactly
# K - 1 messages (E - 1 election records) AND an action that adds a new one.
LIMITS = {
    "n5_l4_c14": ((5, 1, 5, 4, 14, 0), dict(bag_cap=20), 60, (), "compact32"),
    "n3_v4_t6_c14": ((3, 4, 6, 2, 14, 0), dict(bag_cap=16), 80, (126,), "compact32"),
    "n2_v3_l3_c7": ((2, 3, 3, 3, 7, 0), dict(bag_cap=12), 80, (85,), "compact32"),
    "n3_t6_l3": ((3, 1, 6, 3, 3, 0), dict(bag_cap=12), 80, (), "compact32"),
    "n2_l4_k64_e32": ((2, 2, 2, 4, 14, 0), dict(bag_cap=64, elec_cap=32), 40, (669, 1606), "compact32"),
    "n4_v4_c9": ((4, 4, 4, 2, 9, 0), dict(bag_cap=16), 60, (216,), "compact32"),
    # the 256-instance boundary of the compacting kernel, both sides
    "n4_v4_k64": ((4, 4, 3, 2, 2, 0), dict(bag_cap=64), 40, (100, 299, 335), "compact32"),
    "n5_k60": ((5, 1, 3, 2, 2, 0), dict(bag_cap=60), 40, (303, 310), "compact32"),
    "n5_k61": ((5, 1, 3, 2, 2, 0), dict(bag_cap=61), 40, (303, 310), "wave"),
    "n5_k63": ((5, 1, 3, 2, 2, 0), dict(bag_cap=63), 40, (303, 310), "wave"),
}
TABLE = ["n5_l4_c14", "n3_v4_t6_c14", "n2_v3_l3_c7", "n3_t6_l3", "n2_l4_k64_e32", "n4_v4_c9"]  # the field widths
BOUNDARY = ["n4_v4_k64", "n5_k60", "n5_k61", "n5_k63"]                                         # the instance count
ALL = TABLE + BOUNDARY
SYMMETRIC = ["n5_l4_c14", "n4_v4_c9"]  # the N = 5 and N = 4 shapes, also run with symmetry=True
# where two shapes are enough: 3-bit terms with 2-bit values; L = 4 with both capacities at their maximum
TWO = ["n3_v4_t6_c14", "n2_l4_k64_e32"]

WITNESSES = ("currentTerm = T+1", "own log of L+1 entries", "message count C+1", "message count C",
             "log entry (term T, value V)", "commitIndex = L", "nextIndex = L+1", "matchIndex = L",
             "mlog of L entries", "K-1 -> K messages", "E-1 -> E elections")


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    shape: tuple
    cfg: rtla.Config        # invariants = ()
    vc: rv.Cfg
    K: int                  # bag slots
    E: int                  # election records
    kernel: str
    rows: tuple             # the sample's rows (tuples of words)
    states: tuple           # the same as value-oracle states, parsed from their text
    succ: tuple             # per input: ((label, successor state), ...) from raft_values.next_states
    ref: tuple              # per input: sorted ((in_model, text), ...) of its successors
    witnesses: dict         # WITNESSES -> count over the oracle states
    by_text: tuple          # per input: {successor text: successor state}

    def with_cfg(self, **kw):
        return dataclasses.replace(self.cfg, **kw)

    def state_of(self, k, row):
        """The value oracle's state of `row`, a successor of input k (by its text: the oracle's own successor,
        not a parse of the product's text)."""
        return self.by_text[k][rtla.state_text(self.cfg, row)]

    @property
    def n_succ(self):
        return sum(len(s) for s in self.succ)


def caps(cfg):
    """(K, E): bag slots and election records of a configuration's row (rtla_host.cpp's defaults)."""
    k = cfg.bag_cap or (cfg.max_msgs + 1 if cfg.max_msgs > 0 else 32)
    e = max(1, cfg.elec_cap or (cfg.max_term - 1) * cfg.n_server)
    return k, e


def n_instances(cfg):
    n, v = cfg.n_server, cfg.n_value
    return 4 * n + 2 * n * n + n * v + 3 * caps(cfg)[0]


def kernel_of(cfg, symmetry=False):
    """The level kernel that serves cfg's layout, by the rule in this module's docstring: (name, lds bytes)."""
    lay = rtla.row_layout(cfg)
    w, aw = lay["W"], lay["all_words"]

    def lds(g, sym):
        words = (4 * g * (2 if sym else 1) + 32 + 256 + g * w + g * aw + 64 * (2 if sym else 1)
                 + (5 * 64 + 15 * g if sym else 0) + 3) & ~3
        return 4 * words

    g = 32 if symmetry or lds(64, False) > 16 * 1024 else 64
    if lds(g, symmetry) > 160 * 1024 or (n_instances(cfg) + 63) // 64 * 64 > 256:
        return "wave", 0
    return "compact%d" % g, lds(g, symmetry)


def count_witnesses(shape, K, E, states, succ):
    """WITNESSES -> how many of the oracle's states (inputs and reference successors; for the two capacity
    steps: inputs) show it."""
    _, v, t, l, c, _ = shape
    ix = rv.IX
    got = collections.Counter()

    def scan(s):
        msgs = s[ix["messages"]]
        logs = s[ix["log"]]
        got["currentTerm = T+1"] += any(x == t + 1 for x in s[ix["currentTerm"]])
        got["own log of L+1 entries"] += any(len(x) == l + 1 for x in logs)
        got["message count C+1"] += any(n == c + 1 for _, n in msgs.items())
        got["message count C"] += any(n == c for _, n in msgs.items())
        got["log entry (term T, value V)"] += any(e["term"] == t and e["value"] == v - 1 for x in logs for e in x)
        got["commitIndex = L"] += any(x == l for x in s[ix["commitIndex"]])
        got["nextIndex = L+1"] += any(x == l + 1 for row in s[ix["nextIndex"]] for x in row)
        got["matchIndex = L"] += any(x == l for row in s[ix["matchIndex"]] for x in row)
        got["mlog of L entries"] += any("mlog" in m and len(m["mlog"]) == l for m, _ in msgs.items())

    for s, nxt in zip(states, succ):
        scan(s)
        for _, u in nxt:
            scan(u)
        got["K-1 -> K messages"] += (len(s[ix["messages"]]) == K - 1
                                     and any(len(u[ix["messages"]]) == K for _, u in nxt))
        got["E-1 -> E elections"] += (len(s[ix["elections"]]) == E - 1
                                      and any(len(u[ix["elections"]]) == E for _, u in nxt))
    return {w: got[w] for w in WITNESSES}


def sample_rows(cfg, n_rows, extra):
    return rtla.random_rows(cfg, 0, n_rows) + [rtla.random_rows(cfg, i, 1)[0] for i in extra]


@functools.lru_cache(maxsize=None)
def case(name):
    """The case `name`, computed once per process and shared: treat it as read-only."""
    shape, kw, n_rows, extra, kernel = LIMITS[name]
    n, v, t, l, c, m = shape
    cfg = rtla.Config(n, v, t, l, c, m, (), **kw)
    vc = rv.Cfg(n, v, t, l, c, (), m)
    K, E = caps(cfg)
    rows = sample_rows(cfg, n_rows, extra)
    states = [tla_text.parse_state(vc, rtla.state_text(cfg, r)) for r in rows]
    succ = [tuple(rv.next_states(vc, s)) for s in states]
    texts = [[rv.state_text(vc, u) for _, u in nxt] for nxt in succ]
    by_text = [{t: u for t, (_, u) in zip(ts, nxt)} for ts, nxt in zip(texts, succ)]
    ref = [tuple(sorted((rv.in_model(vc, u), t) for t, (_, u) in zip(ts, nxt))) for ts, nxt in zip(texts, succ)]
    return Case(name, shape, cfg, vc, K, E, kernel, tuple(tuple(r) for r in rows), tuple(states), tuple(succ),
                tuple(ref), count_witnesses(shape, K, E, states, succ), tuple(by_text))


def spread(items, at_most):
    """At most `at_most` of items, evenly spaced."""
    step = max(1, -(-len(items) // at_most))
    return items[::step]


@functools.lru_cache(maxsize=None)
def host_expand(name):
    """The case's successors from the host-compiled model (tests/hostmodel.py), as rtla.expand_batch lists
    them: ((input, instance, receive-sub, in_model, row), ...) sorted by (input, instance).  Shared, read-only."""
    import hostmodel
    c = case(name)
    return tuple((k, inst, sub, im, tuple(r))
                 for k, inst, sub, im, r in hostmodel.expand(c.cfg, c.rows, len(c.rows[0])))


@functools.lru_cache(maxsize=None)
def full_bag_rows(name):
    """((row, value-oracle state), ...): states with all K bag slots in use, whose expansion needs no further
    slot -- so that DuplicateMessage and DropMessage of slot K - 1 (the highest instance ids of the layout)
    are enabled and the row can be expanded at all (an action that sends a new message from a full bag is a
    capacity error).  Each is an in-model successor with K messages of one of the sample's K - 1 inputs,
    made quiet by editing packed fields (rtla_model.h make_layout: a server record starts with currentTerm - 1
    | state; a bag slot with its type in bits 0-1, 0 and 2 the two requests, and mterm - 1 at bit 2 + 2 *
    bits(N - 1)): every server a Follower in term 1, every request of term 1 moved to term 2 -- so that a
    request is received as UpdateTerm, a response asks for no answer, and nobody sends.  The stored fingerprint
    is set to the from-scratch hash; a row is kept when the value oracle, on its parsed text, still counts K
    messages (the edit made no two equal) and no successor with more."""
    c = case(name)
    lay = rtla.row_layout(c.cfg)
    n, _, t, _, _, _ = c.shape
    b_tcur, b_tm1, mb_term = t.bit_length(), (t - 1).bit_length(), 2 + 2 * (n - 1).bit_length()
    out = []
    for _, _, _, im, r in host_expand(name):
        if not im or r[lay["off_hdr"]] & 0xFF != c.K or len(out) >= 4:
            continue
        for to in range(1, t):  # the term (less 1) the requests of term 1 move to: the first that keeps K messages
            row = list(r)
            for i in range(n):
                row[lay["off_srv"] + i * lay["srv_words"]] &= ~((1 << (b_tcur + 2)) - 1)
            for s in range(c.K):
                w = lay["off_bag"] + s * lay["slot_words"]
                if row[w] & 3 in (0, 2) and not row[w] >> mb_term & ((1 << b_tm1) - 1):
                    row[w] |= to << mb_term
            a, b = rtla.row_fingerprint(c.cfg, row)
            row[0:4] = [a & 0xFFFFFFFF, a >> 32, b & 0xFFFFFFFF, b >> 32]
            state = tla_text.parse_state(c.vc, rtla.state_text(c.cfg, row))
            msgs = state[rv.IX["messages"]]
            if len(msgs) == c.K:
                break
        if len(msgs) == c.K and rv.in_model(c.vc, state):
            assert all(x == 1 for x in state[rv.IX["currentTerm"]]) and set(state[rv.IX["state"]]) == {rv.FOLLOWER}
            assert all(m["mterm"] > 1 for m, _ in msgs.items() if m["mtype"] in (rv.RVREQ, rv.AEREQ))
            assert all(len(u[rv.IX["messages"]]) <= c.K for _, u in rv.next_states(c.vc, state))
            out.append((tuple(row), state))
    return tuple(out)


def assert_witnessed(c, what=""):
    """Print the case's witness counts and require every one (all of them are admitted by every shape of
    LIMITS: L >= 2, C >= 2, and the generator leaves one bag slot and one election record free)."""
    out_of_model = sum(1 for per in c.ref for im, _ in per if not im)
    print("%s%s %s: %d rows, W = %d, %d successors (%d out of model), kernel %s; witnesses: %s" % (
        what and what + ": ", c.name, c.shape, len(c.rows), len(c.rows[0]), c.n_succ, out_of_model, c.kernel,
        ", ".join("%s x%d" % kv for kv in c.witnesses.items())))
    missing = [w for w, k in c.witnesses.items() if not k]
    assert not missing, "%s: the sample never reaches %s" % (c.name, missing)
