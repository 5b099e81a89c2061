"""TEST INFRASTRUCTURE: a reference BFS under a user CONSTRAINT, from the
host-compiled model (tests/hostmodel.py) for the successors and the host
interpreter (rtla.pred_replay) for the constraint -- no GPU.  It follows
DESIGN.md section 16: a level holds every new in-model state (dedup on the
stored fingerprint); the constraint then keeps some of them, Init's level
included; only kept rows are expanded.  Dropped states stay in the seen set."""
import dataclasses
import functools

import hostmodel
import rtla

ONE_CANDIDATE = r"OneCandidate == \A i, j \in Server : (state[i] = Candidate /\ state[j] = Candidate) => i = j"
ONE_ELECTION = r"OneElection == Cardinality(elections) <= 1"
CONSTRAINTS = {"one_candidate": ONE_CANDIDATE, "one_candidate_one_election": ONE_CANDIDATE + "\n" + ONE_ELECTION}


@dataclasses.dataclass(frozen=True)
class RefLevel:
    kept: tuple        # rows (tuples of words) the constraint keeps, in generation order
    dropped: tuple     # new in-model rows the constraint drops
    generated: int     # successors generated to produce the level (Init: 1)


def init_row(cfg):
    row = rtla.init_row(cfg)
    a, b = rtla.row_fingerprint(cfg, row)
    row[0:4] = [a & 0xFFFFFFFF, a >> 32, b & 0xFFFFFFFF, b >> 32]
    return row


def bfs(cfg, text, max_levels):
    """The first max_levels levels (fewer if the search ends: the last one then keeps nothing)."""
    w = rtla.row_words(cfg)
    levels = []
    with rtla.Predicates(cfg, text) as preds:
        new, generated = [init_row(cfg)], 1
        seen = {rtla.stored_fingerprint(new[0])}
        while True:
            masks = rtla.pred_replay(preds, new)[0] if new else []
            kept = tuple(tuple(r) for r, m in zip(new, masks) if m == 0)
            levels.append(RefLevel(kept, tuple(tuple(r) for r, m in zip(new, masks) if m != 0), generated))
            if not kept or len(levels) >= max_levels:
                return tuple(levels)
            succ = hostmodel.expand(cfg, kept, w)
            generated, new = len(succ), []
            for _, _, _, in_model, row in succ:
                fp = rtla.stored_fingerprint(row)
                if in_model and fp not in seen:
                    seen.add(fp)
                    new.append(row)


@functools.lru_cache(maxsize=None)
def case(shape, which, max_levels):
    """(cfg, constraint text, levels) of a reference search: computed once per process, shared, read-only."""
    cfg = rtla.Config(*shape, invariants=(), fpset_log2=20, mem_budget=1 << 29)
    return cfg, CONSTRAINTS[which], bfs(cfg, CONSTRAINTS[which], max_levels)
