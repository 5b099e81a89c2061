"""TEST INFRASTRUCTURE: the value-oracle reference of a search seeded from chosen roots (rtla_init_rows),
shared by tests/test_seed_host.py and tests/test_seed_gpu.py.

Roots are rows of the synthetic generator (rtla.random_rows), each parsed into a raft_values state from its
text.  Everything the reference says comes from three things alone: raft_values.next_states (the literal
transcription of Next), raft_values.in_model (the StateConstraint) and test_safety_host.py_mask (the five
invariants written in Python from the TLA+ text).  Nothing here calls check_replay, expand_batch or the host
model, so a verdict of the kernels is never compared with code they share.

A sample classifies its rows against a set M of invariants (a mask):
    clean       the row itself violates none of M
    quiet       clean, and no successor (in the model or not) violates any of M
    single      clean, and exactly ONE of the successors next_states lists violates any of M
                (single-in: that successor satisfies the StateConstraint; single-out: it does not)
A seeded search over quiet rows plus one single row has exactly one violating step, so the kernels' verdict
-- mask, in_model, parent, successor -- is determined, whichever wave claims it.

The counting rule of ref_search is test_synthetic_step_dedup_counts's: every successor is generated; an
in-model successor is new when no earlier level and no earlier successor of this level holds it; states are
distinct by text -- under SYMMETRY by orbit text (raft_values.orbit_text, what
test_limit_shapes_orbit_key_and_orbit_text compares the orbit key with).
"""
import ctypes as C
import dataclasses
import functools

import raft_values as rv
import rtla
import tla_text
from test_safety_host import py_mask

ALL = tuple(rtla.INV_BITS)  # bit order
ALL_MASK = sum(rtla.INV_BITS.values())

# (shape (N, V, T, L, C, M), bag slots): the layouts rtla_kdev.h compiles in, with the masks compiled with them
CFG2 = ((3, 2, 3, 2, 1, 0), 18)     # ElectionSafety | LogMatching
CFG1 = ((3, 1, 2, 1, 1, 0), 24)     # NoTwoLeaders
EXHAUST = ((3, 2, 2, 2, 1, 2), 3)   # ElectionSafety | LogMatching
SYNTH = ((3, 2, 4, 3, 2, 0), 12)    # ElectionSafety | LogMatching
CFG4 = ((5, 1, 3, 2, 1, 0), 20)     # SYMMETRY, no invariant
N2 = ((2, 2, 3, 2, 1, 0), 20)       # a narrow run-time layout
# rows classified per layout: enough for 130 roots and a violator of every invariant the layout is asked for
ROWS = {CFG2: 1200, SYNTH: 1200, CFG1: 1200, EXHAUST: 600, N2: 500, CFG4: 500}
COMPILED_MASK = {CFG2: ("ElectionSafety", "LogMatching"), SYNTH: ("ElectionSafety", "LogMatching"),
                 EXHAUST: ("ElectionSafety", "LogMatching"), CFG1: ("NoTwoLeaders",)}

# Generator ids (rtla.random_rows(cfg, id, 1)) of the N2 shape's single-out rows: the only ones among ids
# 0..5999, found once by classifying all of them.  Out-of-model first violations are rare by construction:
# only HandleAppendEntriesRequest's "already done" step both moves commitIndex and sends a reply that can
# push a count to MaxCopies + 1, so they exist for StateMachineSafety and LeaderCompleteness alone.
SINGLE_OUT = {"StateMachineSafety": (2475, 5855), "LeaderCompleteness": (2475, 5855)}


def family(name):
    """The action family of a product action name or a value-oracle label ("Receive -> X" / "Receive:X": X)."""
    for sep in (" -> ", ":"):
        if name.startswith("Receive" + sep):
            return name.split(sep, 1)[1]
    return name.split("(", 1)[0]


def configs(shape, bag, invariants=(), **kw):
    n, v, t, l, c, m = shape
    return rtla.Config(n, v, t, l, c, m, tuple(invariants), bag_cap=bag, **kw), rv.Cfg(n, v, t, l, c, (), m)


@dataclasses.dataclass(frozen=True)
class Succ:
    label: str
    state: tuple
    text: str
    in_model: bool
    mask: int       # the full py_mask


@dataclasses.dataclass(frozen=True)
class Sample:
    shape: tuple
    bag: int
    ids: tuple          # generator ids
    cfg: rtla.Config    # invariants = ()
    vc: rv.Cfg
    rows: tuple
    states: tuple
    texts: tuple
    masks: tuple        # py_mask of each row
    succ: tuple         # per row: (Succ, ...)

    def violators(self, k, mask):
        return [u for u in self.succ[k] if u.mask & mask]

    def clean(self, mask):
        return [k for k in range(len(self.rows)) if not self.masks[k] & mask]

    def quiet(self, mask):
        return [k for k in self.clean(mask) if not self.violators(k, mask)]

    def single(self, mask, in_model=True, exactly=None):
        """Rows clean on `mask` with exactly one successor violating any of it -- `exactly`: whose violated
        part of `mask` is that value -- in the model or not."""
        out = []
        for k in self.clean(mask):
            v = self.violators(k, mask)
            if len(v) == 1 and v[0].in_model == in_model and (exactly is None or v[0].mask & mask == exactly):
                out.append(k)
        return out

    def several(self):
        """All-clean rows whose one violating successor violates at least two of the five invariants."""
        return [k for k in self.single(ALL_MASK) if bin(self.violators(k, ALL_MASK)[0].mask).count("1") >= 2]

    def headroom(self, k):
        """Steps below row k that cannot leave the row format: an action adds at most one distinct message
        and one election record, and the product reports a state that needs more bag slots or election records
        than the layout has as a capacity error."""
        from limits import caps
        K, E = caps(self.cfg)
        s = self.states[k]
        return min(K - len(s[rv.IX["messages"]]), E - len(s[rv.IX["elections"]]))


@functools.lru_cache(maxsize=None)
def successors(vc, s):
    """The value oracle's successors of s, each with its text, in-model flag and mask (computed once per state);
    None where Next has a TLC evaluation error (the product's RTLA_E_SPEC: the generator's states are no
    reachable ones, and a few steps below some of them an index leaves its sequence's domain)."""
    try:
        nxt = rv.next_states(vc, s)
    except rv.SpecError:
        return None
    return tuple(Succ(lab, t, rv.state_text(vc, t), rv.in_model(vc, t), py_mask(vc, t)) for lab, t in nxt)


def clean_below(vc, s, mask, steps):
    """Whether no state within `steps` steps of s (through in-model states) violates any of mask, and every
    state expanded on the way has its successors (no evaluation error)."""
    level = [s]
    for _ in range(steps):
        nxt = []
        for p in level:
            if successors(vc, p) is None:
                return False
            for u in successors(vc, p):
                if u.mask & mask:
                    return False
                if u.in_model:
                    nxt.append(u.state)
        level = nxt
    return True


@functools.lru_cache(maxsize=None)
def sample(shape, bag, n, extra=()):
    """The generator's rows 0..n-1 of a layout, then the rows with the ids `extra`, classified.  A row is
    named by its index in the sample (ids[index] is its generator id).  Shared, read-only."""
    cfg, vc = configs(shape, bag)
    ids = tuple(range(n)) + tuple(extra)
    rows = rtla.random_rows(cfg, 0, n) + [rtla.random_rows(cfg, i, 1)[0] for i in extra]
    texts = [rtla.state_text(cfg, r) for r in rows]
    states = [tla_text.parse_state(vc, t) for t in texts]
    return Sample(shape, bag, ids, cfg, vc, tuple(tuple(r) for r in rows), tuple(states), tuple(texts),
                  tuple(py_mask(vc, s) for s in states), tuple(successors(vc, s) for s in states))


def one_per_orbit(smp, ks):
    """Of the rows ks, the first of each orbit.  Orbits are told apart by rtla.orbit_text, the host's orbit
    text, which tests/test_symmetry_key.py and test_seed_host.py hold to the value oracle's brute force over
    all N! images (raft_values.orbit_text: 30 ms a state at N = 5, too slow for every row of a sample)."""
    sym = dataclasses.replace(smp.cfg, symmetry=True)
    seen, out = set(), []
    for k in ks:
        o = rtla.orbit_text(sym, smp.rows[k])
        if o not in seen:
            seen.add(o)
            out.append(k)
    return out


@dataclasses.dataclass
class Search:
    levels: list        # per level (new, generated); level 1 first
    texts: list         # per level: the sorted keys (state texts; SYMMETRY: orbit texts) of its new states
    viol_level: int     # the first level with a generated successor whose mask meets `mask`, or None
    violations: set     # at that level: (parent text, successor text, successor's py_mask & mask, in_model)
    chains: dict        # state text -> (parent text or None, label) of every state stored, for the traces


def ref_search(vc, root_states, mask, max_levels, symmetry=False):
    """The seeded BFS by the value oracle: levels 1..max_levels, ending at the first level that generates a
    successor violating any of `mask` (that level's counts are complete: the kernels finish it too)."""
    key = (lambda s: rv.orbit_text(vc, s)) if symmetry else (lambda s: rv.state_text(vc, s))
    seen, frontier, chains = set(), [], {}
    for s in root_states:
        k = key(s)
        if k not in seen:
            seen.add(k)
            frontier.append(s)
            chains[rv.state_text(vc, s)] = (None, None)
    out = Search([(len(frontier), len(root_states))], [sorted(key(s) for s in frontier)], None, set(), chains)
    for level in range(2, max_levels + 1):
        gen, new, viol = 0, [], set()
        for s in frontier:
            ptext = rv.state_text(vc, s)
            for u in successors(vc, s):
                gen += 1
                lab, t, ttext, im, m = u.label, u.state, u.text, u.in_model, u.mask & mask
                if m:
                    viol.add((ptext, ttext, m, im))
                if im:
                    k = key(t)
                    if k not in seen:
                        seen.add(k)
                        new.append(t)
                        chains.setdefault(ttext, (ptext, lab))
        out.levels.append((len(new), gen))
        out.texts.append(sorted(key(s) for s in new))
        if viol:
            out.viol_level, out.violations = level, viol
            break
        frontier = new
    return out


def is_oracle_step(vc, ptext, label_name, ttext):
    """Whether ttext is a value-oracle successor of ptext by an action of label_name's family."""
    s = tla_text.parse_state(vc, ptext)
    return any(rv.state_text(vc, t) == ttext and family(lab) == family(label_name) for lab, t in rv.next_states(vc, s))


# ---- the product's side of a case, as plain data: run here or (RTLA_XFLAGS is read once) in a child process

def gen_rows(cfg, ids):
    """The generator's rows with these ids."""
    bulk = max(ROWS.values())  # ids below it come from one call, the few pinned ones beyond it one by one
    top = max((i + 1 for i in ids if i < bulk), default=0)
    base = rtla.random_rows(cfg, 0, top)
    return [base[i] if i < top else rtla.random_rows(cfg, i, 1)[0] for i in ids]


def job(cfg, smp, roots, steps=1, frontiers=False):
    """A seeded search to run: the configuration, the roots (rows of the sample, as generator ids), the steps
    after init."""
    return dict(cfg=dataclasses.asdict(cfg), ids=[smp.ids[k] for k in roots], steps=steps, frontiers=frontiers)


def run_job(j):
    """init(roots) and up to `steps` steps (ending at the first status that is not OK).  Returns the statuses,
    per level (new, generated), rtla_violation's raw mask and in_model, Checker.violation()'s name, the trace
    after a violation, and (frontiers) each level's sorted state texts."""
    cfg = rtla.Config(**dict(j["cfg"], invariants=tuple(j["cfg"]["invariants"])))
    out = dict(status=[], texts=[], trace=None)
    with rtla.Checker(cfg) as ck:
        st = ck.init(gen_rows(cfg, j["ids"]))
        for step in range(j["steps"] + 1):
            if step:
                st = ck.step()
            out["status"].append(st)
            if j["frontiers"]:
                out["texts"].append(sorted(rtla.state_text(cfg, r) for r in ck.frontier()))
            if st != rtla.OK:
                break
        m, im = C.c_int32(0), C.c_int32(0)
        rtla._lib.rtla_violation(ck._h, C.byref(m), C.byref(im))
        out.update(levels=[[lv.new, lv.generated] for lv in ck.levels], mask=m.value, in_model=bool(im.value),
                   violation=ck.violation()[0])
        if st == rtla.VIOLATION:
            out["trace"] = [list(t) for t in ck.trace()]
    return out


def run_jobs_in_child(jobs, xflags, tmp):
    """The same for a list of jobs in ONE fresh process started with RTLA_XFLAGS = xflags."""
    import json
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    path = os.path.join(str(tmp), "jobs_%s.json" % xflags)
    with open(path, "w") as f:
        json.dump(jobs, f)
    env = dict(os.environ, RTLA_XFLAGS=str(xflags),
               PYTHONPATH=os.pathsep.join([here, os.path.join(root, "oracle"), os.path.join(root, "raft-tla_amd"),
                                           os.environ.get("PYTHONPATH", "")]))
    code = ("import json, sys, seedref; "
            "print(json.dumps([seedref.run_job(j) for j in json.load(open(sys.argv[1]))]))")
    out = subprocess.run([sys.executable, "-c", code, path], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


# ---- root sets

POSITIONS = ("first", "at 64", "last")


def place(quiet, v, pos):
    """The quiet rows with the violator v as root 0, as root 64 (the second 64-row group) or as the last."""
    at = {"first": 0, "at 64": 64, "last": len(quiet)}[pos]
    return quiet[:at] + [v] + quiet[at:]


def owner(fp_a, shards):
    """rtla_device.h fp_owner: the low 32 bits of the fingerprint's first half scaled to [0, shards)."""
    return ((fp_a & 0xFFFFFFFF) * shards) >> 32


@functools.lru_cache(maxsize=None)
def shard_picks(shape, bag, n, bit, shards):
    """(same, other): the first single-in row for `bit` whose violating successor is owned by the row's own shard,
    and the first whose successor another shard owns (then the winners kernel builds and reports it).  The
    successor's row comes from the host-compiled model; its owner from rtla_row_fingerprint."""
    import hostmodel
    smp = sample(shape, bag, n)
    same = other = None
    for k in smp.single(bit):
        want = smp.violators(k, bit)[0].text
        rows = [r for _, _, _, _, r in hostmodel.expand(smp.cfg, [smp.rows[k]], len(smp.rows[k]))
                if rtla.state_text(smp.cfg, r) == want]
        assert len(rows) == 1
        mine = owner(rtla.row_fingerprint(smp.cfg, smp.rows[k])[0], shards)
        theirs = owner(rtla.row_fingerprint(smp.cfg, rows[0])[0], shards)
        if mine == theirs and same is None:
            same = k
        if mine != theirs and other is None:
            other = k
        if same is not None and other is not None:
            break
    return same, other


@functools.lru_cache(maxsize=None)
def deep_quiet(shape, bag, n, want, steps=2):
    """The first `want` rows of the sample from which `steps` levels violate none of the five invariants and
    stay inside the row format."""
    smp = sample(shape, bag, n)
    out = []
    for k in smp.quiet(ALL_MASK):
        if smp.headroom(k) >= steps and clean_below(smp.vc, smp.states[k], ALL_MASK, steps):
            out.append(k)
            if len(out) == want:
                break
    return tuple(out)
