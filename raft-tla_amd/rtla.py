"""Python host-side mirror of the C ABI (include/rtla.h) over ctypes.

This is the user-facing API of the MI355X model checker for Python callers
(tests, bench.py).  It mirrors TLC's model-checking contract for
/root/reference/raft.tla + a raft.cfg-style model (raft.cfg:1-15):

    res = rtla.check(rtla.Config(n_server=3, n_value=1, max_term=2, max_log=1,
                                 max_copies=1, max_msgs=2,
                                 invariants=("NoTwoLeaders",)))
    res.distinct, res.generated, res.depth, res.violation, res.trace

There is no CPU fallback: every entry point runs the HIP kernels in
librtla.so, and importing this module raises if the library is missing.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RTLA_LIB") or os.path.join(HERE, "librtla.so")  # RTLA_LIB: perf-experiment builds only

OK, DONE, VIOLATION = 0, 1, 2
E_CONFIG, E_HIP, E_OVERFLOW, E_SPEC, E_STATE, E_ARG, E_COMM = -1, -2, -3, -4, -5, -6, -7  # include/rtla.h
INV_BITS = {"NoTwoLeaders": 1, "ElectionSafety": 2, "LogMatching": 4, "StateMachineSafety": 8,
            "LeaderCompleteness": 16}  # specs/MC.tla; in bit order
COVER_NAMES = ["Restart", "Timeout", "RequestVote", "BecomeLeader", "ClientRequest",
               "AdvanceCommitIndex", "AppendEntries", "Receive", "DuplicateMessage",
               "DropMessage", "UpdateTerm", "HandleRequestVoteRequest",
               "HandleRequestVoteResponse", "HandleAppendEntriesRequest",
               "HandleAppendEntriesResponse", "DropStaleResponse"]


# rtla_level_stats.flags: which capacity ran out (include/rtla.h RTLA_CAP_*)
CAP_NAMES = {1: "spec-error", 2: "row", 4: "frontier", 8: "fpset", 16: "outbox"}
CAP_SPEC_ERROR = 1


class RtlaError(RuntimeError):
    def __init__(self, status: int, what: str = "", flags: int = 0):
        self.status = status
        self.flags = flags
        msg = _lib.rtla_strerror(status).decode() if _lib else str(status)
        caps = [n for b, n in CAP_NAMES.items() if flags & b]
        super().__init__("%s: %s (status %d%s)" % (what, msg, status, ", " + "+".join(caps) if caps else ""))


class _Cfg(C.Structure):
    _fields_ = [("n_server", C.c_int32), ("n_value", C.c_int32), ("max_term", C.c_int32),
                ("max_log", C.c_int32), ("max_copies", C.c_int32), ("max_msgs", C.c_int32),
                ("bag_cap", C.c_int32), ("elec_cap", C.c_int32), ("inv_mask", C.c_int32),
                ("symmetry", C.c_int32), ("fpset_log2", C.c_int32), ("shards", C.c_int32),
                ("frontier_cap", C.c_uint64), ("mem_budget", C.c_uint64), ("chunk", C.c_uint64),
                ("mode", C.c_int32), ("reserved", C.c_int32)]


class _Stats(C.Structure):
    _fields_ = [("level", C.c_int32), ("status", C.c_int32), ("frontier", C.c_uint64),
                ("new_states", C.c_uint64), ("generated", C.c_uint64),
                ("distinct_total", C.c_uint64), ("generated_total", C.c_uint64),
                ("seconds", C.c_double), ("kernel_ms", C.c_double), ("probes", C.c_uint64),
                ("row_bytes", C.c_uint64), ("expand_ms", C.c_double), ("flags", C.c_int32),
                ("reserved", C.c_int32)]


class _SimStats(C.Structure):
    _fields_ = [("walks", C.c_uint64), ("steps", C.c_uint64), ("generated", C.c_uint64), ("stuck", C.c_uint64),
                ("kernel_ms", C.c_double), ("viol_walk", C.c_uint64), ("viol_step", C.c_int32),
                ("viol_inst", C.c_int32), ("viol_mask", C.c_int32), ("viol_in_model", C.c_int32),
                ("status", C.c_int32), ("flags", C.c_int32), ("taken", C.c_uint64 * 16)]


class _SimPredStats(C.Structure):
    _fields_ = [("state_evaluated", C.c_uint64), ("step_evaluated", C.c_uint64), ("viol_inv_mask", C.c_int32),
                ("viol_state_mask", C.c_int32), ("viol_step_mask", C.c_int32), ("reserved", C.c_int32)]


class _AuditStats(C.Structure):
    _fields_ = [("audited", C.c_uint64), ("evaluated", C.c_uint64), ("counts", C.c_uint64 * 8),
                ("kernel_ms", C.c_double), ("row_bytes", C.c_uint64), ("viol_index", C.c_uint64),
                ("viol_inst", C.c_int32), ("viol_mask", C.c_int32), ("viol_in_model", C.c_int32),
                ("status", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32)]


class _ConstrainStats(C.Structure):
    _fields_ = [("level", C.c_int32), ("status", C.c_int32), ("examined", C.c_uint64), ("kept", C.c_uint64),
                ("dropped", C.c_uint64), ("counts", C.c_uint64 * 8), ("start", C.c_uint64),
                ("eval_ms", C.c_double), ("move_ms", C.c_double), ("distinct_total", C.c_uint64),
                ("flags", C.c_int32), ("reserved", C.c_int32)]


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError("librtla.so not built at %s (run `make -C raft-tla_amd` or "
                          "__graft_entry__.build())" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    P = C.POINTER
    sig = {
        "rtla_open": (C.c_int, [P(_Cfg), C.c_int, C.c_int, C.c_void_p, P(C.c_void_p)]),
        "rtla_close": (None, [C.c_void_p]),
        "rtla_init": (C.c_int, [C.c_void_p, P(_Stats)]),
        "rtla_init_rows": (C.c_int, [C.c_void_p, P(C.c_uint32), C.c_size_t, P(_Stats)]),
        "rtla_step": (C.c_int, [C.c_void_p, P(_Stats)]),
        "rtla_reset": (C.c_int, [C.c_void_p]),
        "rtla_violation": (C.c_int, [C.c_void_p, P(C.c_int32), P(C.c_int32)]),
        "rtla_trace": (C.c_int, [C.c_void_p, P(C.c_uint32), P(C.c_int32), C.c_size_t, P(C.c_size_t)]),
        "rtla_frontier": (C.c_int, [C.c_void_p, P(C.c_uint32), C.c_size_t, P(C.c_size_t)]),
        "rtla_frontier_rows": (C.c_int, [C.c_void_p, P(C.c_uint64), C.c_size_t, P(C.c_uint32)]),
        "rtla_coverage": (C.c_int, [C.c_void_p, P(C.c_uint64), P(C.c_uint64), C.c_int]),
        "rtla_device_info": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t]),
        "rtla_time_expand": (C.c_int, [C.c_void_p, C.c_int, C.c_int, P(C.c_double)]),
        "rtla_checkpoint": (C.c_int, [C.c_void_p, C.c_char_p]),
        "rtla_recover": (C.c_int, [C.c_void_p, C.c_char_p]),
        "rtla_probe_bench2": (C.c_int, [C.c_int, C.c_uint64, P(C.c_double), P(C.c_double), P(C.c_double),
                                        P(C.c_uint64)]),
        "rtla_probe_bench3": (C.c_int, [C.c_int, C.c_uint64, C.c_uint64, C.c_double, P(C.c_double),
                                        P(C.c_uint64)]),
        "rtla_random_texts": (C.c_int, [P(_Cfg), C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_char_p,
                                        C.c_size_t, P(C.c_size_t)]),
        "rtla_row_words": (C.c_int, [P(_Cfg)]),
        "rtla_row_layout": (C.c_int, [P(_Cfg), P(C.c_int32), C.c_int]),
        "rtla_init_row": (C.c_int, [P(_Cfg), P(C.c_uint32)]),
        "rtla_expand_batch": (C.c_int, [P(_Cfg), P(C.c_uint32), C.c_size_t, P(C.c_uint32),
                                        P(C.c_uint64), C.c_size_t, P(C.c_size_t)]),
        "rtla_state_text": (C.c_int, [P(_Cfg), P(C.c_uint32), C.c_char_p, C.c_size_t]),
        "rtla_action_name": (C.c_int, [P(_Cfg), C.c_int32, C.c_int32, C.c_char_p, C.c_size_t]),
        "rtla_invariants": (C.c_int, [P(_Cfg), P(C.c_uint32)]),
        "rtla_row_fingerprint": (C.c_int, [P(_Cfg), P(C.c_uint32), P(C.c_uint64)]),
        "rtla_strerror": (C.c_char_p, [C.c_int]),
        "rtla_abi_version": (C.c_int, []),
        "rtla_comm_id": (C.c_int, [C.c_void_p]),
        "rtla_probe_bench": (C.c_int, [C.c_int, C.c_uint64, P(C.c_double), P(C.c_uint64)]),
        "rtla_random_rows": (C.c_int, [P(_Cfg), C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, P(C.c_uint32)]),
        "rtla_synthetic_step": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, P(_Stats)]),
        "rtla_synthetic_generate": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64]),
        "rtla_synthetic_dedup": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, P(_Stats)]),
        "rtla_orbit_key": (C.c_int, [P(_Cfg), P(C.c_uint32), P(C.c_uint64), P(C.c_int)]),
        "rtla_permute_row": (C.c_int, [P(_Cfg), P(C.c_uint32), P(C.c_int), P(C.c_uint32)]),
        "rtla_rows_text_hash": (C.c_int, [P(_Cfg), P(C.c_uint32), C.c_size_t, C.c_int, P(C.c_uint64)]),
        "rtla_level_text_hash": (C.c_int, [C.c_void_p, C.c_int, P(C.c_uint64)]),
        "rtla_rows_orbit_hash": (C.c_int, [P(_Cfg), P(C.c_uint32), C.c_size_t, C.c_int, P(C.c_uint64)]),
        "rtla_level_orbit_hash": (C.c_int, [C.c_void_p, C.c_int, P(C.c_uint64)]),
        "rtla_orbit_text": (C.c_int, [P(_Cfg), P(C.c_uint32), C.c_char_p, C.c_size_t]),
        "rtla_simulate": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int32, P(C.c_uint64),
                                    P(_SimStats)]),
        "rtla_sim_replay": (C.c_int, [P(_Cfg), P(C.c_uint32), C.c_size_t, C.c_uint64, C.c_uint64, C.c_uint64,
                                      C.c_int32, C.c_int, P(C.c_uint64), P(_SimStats)]),
        "rtla_sim_walk": (C.c_int, [P(_Cfg), P(C.c_uint32), C.c_uint64, C.c_uint64, C.c_int32, P(C.c_uint32),
                                    P(C.c_int32), C.c_size_t, P(C.c_size_t)]),
        "rtla_simulate_pred": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int32, C.c_void_p,
                                         C.c_void_p, P(C.c_uint64), P(_SimStats), P(_SimPredStats)]),
        "rtla_sim_replay_pred": (C.c_int, [P(_Cfg), P(C.c_uint32), C.c_size_t, C.c_uint64, C.c_uint64, C.c_uint64,
                                           C.c_int32, C.c_int, C.c_void_p, C.c_void_p, P(C.c_uint64), P(_SimStats),
                                           P(_SimPredStats)]),
        "rtla_sim_walk_pred": (C.c_int, [P(_Cfg), P(C.c_uint32), C.c_uint64, C.c_uint64, C.c_int32, C.c_void_p,
                                         C.c_void_p, P(C.c_uint32), P(C.c_int32), C.c_size_t, P(C.c_size_t)]),
        "rtla_check_batch": (C.c_int, [P(_Cfg), P(C.c_uint32), C.c_size_t, C.c_int32, C.c_int32, P(C.c_int32),
                                       P(C.c_uint64)]),
        "rtla_check_replay": (C.c_int, [P(_Cfg), P(C.c_uint32), C.c_size_t, C.c_int32, C.c_int32, C.c_int,
                                        P(C.c_int32), P(C.c_uint64)]),
        "rtla_check_frontier": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, P(_AuditStats)]),
        "rtla_fpset_probe": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p,
                                       P(C.c_int32)]),
        "rtla_pred_compile": (C.c_int, [P(_Cfg), C.c_char_p, P(C.c_void_p), C.c_char_p, C.c_size_t]),
        "rtla_pred_free": (None, [C.c_void_p]),
        "rtla_pred_count": (C.c_int, [C.c_void_p]),
        "rtla_pred_name": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t]),
        "rtla_pred_replay": (C.c_int, [P(_Cfg), C.c_void_p, P(C.c_uint32), C.c_size_t, C.c_int, P(C.c_int32),
                                       P(C.c_uint64)]),
        "rtla_pred_batch": (C.c_int, [P(_Cfg), C.c_void_p, P(C.c_uint32), C.c_size_t, P(C.c_int32), P(C.c_uint64)]),
        "rtla_pred_frontier": (C.c_int, [C.c_void_p, C.c_void_p, P(_AuditStats)]),
        "rtla_pred_compile_step": (C.c_int, [P(_Cfg), C.c_char_p, P(C.c_void_p), C.c_char_p, C.c_size_t]),
        "rtla_pred_is_step": (C.c_int, [C.c_void_p]),
        "rtla_pred_step_replay": (C.c_int, [P(_Cfg), C.c_void_p, P(C.c_uint32), C.c_size_t, C.c_int, P(C.c_int32),
                                            P(C.c_uint64), P(C.c_uint64)]),
        "rtla_pred_step_batch": (C.c_int, [P(_Cfg), C.c_void_p, P(C.c_uint32), C.c_size_t, P(C.c_int32),
                                           P(C.c_uint64), P(C.c_uint64)]),
        "rtla_pred_step_frontier": (C.c_int, [C.c_void_p, C.c_void_p, P(_AuditStats)]),
        "rtla_pred_constrain": (C.c_int, [C.c_void_p, C.c_void_p, P(_ConstrainStats)]),
        "rtla_constrain_batch": (C.c_int, [P(_Cfg), C.c_void_p, P(C.c_uint32), C.c_size_t, C.c_uint64, C.c_uint64,
                                           C.c_uint64, P(C.c_uint32), P(C.c_uint64), P(C.c_size_t), P(C.c_uint64)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


_lib = _load()

EXPORTED = ["rtla_open", "rtla_close", "rtla_comm_id", "rtla_init", "rtla_reset", "rtla_step", "rtla_violation",
            "rtla_trace", "rtla_frontier", "rtla_coverage", "rtla_device_info", "rtla_row_words", "rtla_init_row",
            "rtla_expand_batch", "rtla_state_text", "rtla_action_name", "rtla_invariants", "rtla_row_fingerprint",
            "rtla_strerror", "rtla_abi_version", "rtla_probe_bench", "rtla_time_expand",
            "rtla_probe_bench2", "rtla_checkpoint", "rtla_recover", "rtla_random_rows", "rtla_synthetic_step",
            "rtla_synthetic_generate", "rtla_synthetic_dedup", "rtla_orbit_key", "rtla_permute_row",
            "rtla_rows_text_hash", "rtla_level_text_hash", "rtla_row_layout", "rtla_rows_orbit_hash",
            "rtla_level_orbit_hash", "rtla_orbit_text", "rtla_probe_bench3", "rtla_random_texts",
            "rtla_frontier_rows", "rtla_simulate", "rtla_sim_replay", "rtla_sim_walk", "rtla_check_batch",
            "rtla_check_replay", "rtla_check_frontier", "rtla_fpset_probe", "rtla_pred_compile", "rtla_pred_free",
            "rtla_pred_count", "rtla_pred_name", "rtla_pred_replay", "rtla_pred_batch", "rtla_pred_frontier",
            "rtla_pred_compile_step", "rtla_pred_is_step", "rtla_pred_step_replay", "rtla_pred_step_batch",
            "rtla_pred_step_frontier", "rtla_init_rows", "rtla_simulate_pred", "rtla_sim_replay_pred",
            "rtla_sim_walk_pred", "rtla_pred_constrain", "rtla_constrain_batch"]

SYNTH_SEED = 0x5AF72025  # the synthetic microbench's PRNG seed


@dataclass(frozen=True)
class Config:
    """A raft.cfg-style model: constants + the build's StateConstraint bounds."""
    n_server: int = 3
    n_value: int = 1
    max_term: int = 2
    max_log: int = 1
    max_copies: int = 1
    max_msgs: int = 0
    invariants: Tuple[str, ...] = ("NoTwoLeaders",)
    bag_cap: int = 0
    elec_cap: int = 0
    fpset_log2: int = 0
    frontier_cap: int = 0
    mem_budget: int = 0
    shards: int = 0
    chunk: int = 0
    symmetry: bool = False  # SYMMETRY Permutations(Server) (specs/MC.tla)
    dedup_only: bool = False  # RTLA_MODE_DEDUP: the synthetic microbench's context (no BFS, no parent records)

    @property
    def inv_mask(self) -> int:
        m = 0
        for n in self.invariants:
            m |= INV_BITS[n]
        return m

    def c(self) -> _Cfg:
        return _Cfg(self.n_server, self.n_value, self.max_term, self.max_log, self.max_copies,
                    self.max_msgs, self.bag_cap, self.elec_cap, self.inv_mask, int(self.symmetry),
                    self.fpset_log2, self.shards, self.frontier_cap, self.mem_budget, self.chunk,
                    1 if self.dedup_only else 0, 0)


@dataclass
class Level:
    level: int
    frontier: int
    new: int
    generated: int
    seconds: float
    kernel_ms: float = 0.0
    probes: int = 0
    row_bytes: int = 0
    expand_ms: float = 0.0  # of kernel_ms: the probe kernel alone


@dataclass
class Result:
    distinct: int = 0
    generated: int = 0
    depth: int = 0
    levels: List[Level] = field(default_factory=list)
    violation: Optional[str] = None
    violation_in_model: bool = True
    trace: Optional[List[Tuple[str, str]]] = None   # (action label, state text)
    coverage: Optional[dict] = None
    seconds: float = 0.0


SIM_STOP_DEPTH, SIM_STOP_STUCK, SIM_STOP_VIOLATION = 0, 1, 2
SIM_SEED = 0x5AF72026  # default -seed of the random-walk simulation


@dataclass
class SimResult:
    """One simulate() / sim_replay() call (rtla_sim_stats)."""
    status: int = OK               # OK or VIOLATION
    walks: int = 0                 # walks run (no batch of 2^18 is started after one that found a violation)
    steps: int = 0                 # steps taken
    generated: int = 0             # enabled successors evaluated
    stuck: int = 0
    kernel_ms: float = 0.0         # device time (sim_replay: host wall time)
    violation: Optional[str] = None
    viol_walk: Optional[int] = None
    viol_step: int = 0             # 1-based step whose successor violates
    viol_inst: int = -1
    viol_mask: int = 0
    viol_in_model: bool = True
    taken: dict = field(default_factory=dict)   # steps taken per coverage name
    ends: Optional[List[Tuple[int, ...]]] = None  # per walk: (fp a, fp b, path digest, length, stop)
    # walks that carry user properties (predicates= / actions=): ends are 6-tuples, the five fields plus word 4
    # (instance | in_model << 16 | built-in mask << 24 | state mask << 32 | step mask << 40; 0: no violation);
    # violation is the ", "-joined names of every false thing of the reported successor: built-ins, state
    # definitions, action definitions
    viol_state_mask: int = 0       # its false state definitions (bit k = predicates.names[k])
    viol_step_mask: int = 0        # its false action definitions
    state_evaluated: int = 0       # evaluations of the state set (in-model successors)
    step_evaluated: int = 0        # evaluations of the action set (== generated)


def _sim_result(rc: int, st: _SimStats, ends, n: int, pst=None, predicates=None, actions=None) -> SimResult:
    res = SimResult(status=rc, walks=st.walks, steps=st.steps, generated=st.generated, stuck=st.stuck,
                    kernel_ms=st.kernel_ms, taken={COVER_NAMES[k]: st.taken[k] for k in range(len(COVER_NAMES))})
    if pst is not None:
        res.state_evaluated, res.step_evaluated = pst.state_evaluated, pst.step_evaluated
    if rc == VIOLATION:
        names = [nm for nm, b in INV_BITS.items() if st.viol_mask & b]
        res.violation = names[0] if names else None
        res.viol_walk, res.viol_step, res.viol_inst = st.viol_walk, st.viol_step, st.viol_inst
        res.viol_mask, res.viol_in_model = st.viol_mask, bool(st.viol_in_model)
        if pst is not None:
            res.viol_state_mask, res.viol_step_mask = pst.viol_state_mask, pst.viol_step_mask
            names += predicates.names_of(pst.viol_state_mask) if predicates is not None else []
            names += actions.names_of(pst.viol_step_mask) if actions is not None else []
            res.violation = ", ".join(names)
    if ends is not None:
        m, ew = min(n, st.walks), 4 if pst is None else 5
        res.ends = [(ends[ew * k], ends[ew * k + 1], ends[ew * k + 2], ends[ew * k + 3] & 0xFFFFFFFF,
                     ends[ew * k + 3] >> 32) + ((ends[ew * k + 4],) if pst is not None else ())
                    for k in range(m)]
    return res


def _set_handle(s, step: bool):
    """The handle of an optional set for the *_pred calls (None: NULL); the library checks its kind and layout."""
    if s is None:
        return None
    if not isinstance(s, Predicates) or s._h is None:
        raise RtlaError(E_ARG, "actions=" if step else "predicates=")
    return s._h


def _flat_rows(rows, w: int):
    """(flat u32 array, #rows) of a list of rows -- or of rows already flat (Checker.frontier_flat)."""
    if isinstance(rows, C.Array):
        assert len(rows) % w == 0, "row width mismatch"
        return rows, len(rows) // w
    flat = (C.c_uint32 * max(1, len(rows) * w))()
    for k, r in enumerate(rows):
        assert len(r) == w, "row width mismatch"
        flat[k * w:(k + 1) * w] = list(r)
    return flat, len(rows)


def sim_replay(cfg: Config, start_rows, n_walks: int, depth: int, seed: int = SIM_SEED,
               first: int = 0, threads: int = 0, ends: bool = True, predicates=None, actions=None) -> SimResult:
    """Checker.simulate's walks recomputed on the host (rtla_sim_replay): walk
    w starts at start_rows[w mod len(start_rows)] (a list of rows, or the flat
    array of Checker.frontier_flat).  No GPU, no context.  predicates /
    actions: as Checker.simulate's (rtla_sim_replay_pred)."""
    cc = cfg.c()
    w = row_words(cfg)
    flat, n_start = _flat_rows(start_rows, w)
    if predicates is not None or actions is not None:
        buf = (C.c_uint64 * max(1, 5 * n_walks))() if ends else None
        st, pst = _SimStats(), _SimPredStats()
        rc = _lib.rtla_sim_replay_pred(C.byref(cc), flat, n_start, seed, first, n_walks, depth, threads,
                                       _set_handle(predicates, False), _set_handle(actions, True), buf, C.byref(st),
                                       C.byref(pst))
        if rc < 0:
            raise RtlaError(rc, "rtla_sim_replay_pred", st.flags)
        return _sim_result(rc, st, buf, n_walks, pst, predicates, actions)
    buf = (C.c_uint64 * max(1, 4 * n_walks))() if ends else None
    st = _SimStats()
    rc = _lib.rtla_sim_replay(C.byref(cc), flat, n_start, seed, first, n_walks, depth, threads, buf,
                              C.byref(st))
    if rc < 0:
        raise RtlaError(rc, "rtla_sim_replay", st.flags)
    return _sim_result(rc, st, buf, n_walks)


def sim_walk(cfg: Config, start_row: Sequence[int], walk: int, depth: int, seed: int = SIM_SEED,
             predicates=None, actions=None):
    """One walk from start_row on the host (rtla_sim_walk): (violating, steps)
    with steps = [(instance, receive-sub, row)] of the states it enters and,
    last when `violating`, of its violating successor.  predicates / actions:
    as Checker.simulate's (rtla_sim_walk_pred)."""
    cc = cfg.c()
    w = row_words(cfg)
    arr = (C.c_uint32 * w)(*start_row)
    cap = depth + 1
    rows = (C.c_uint32 * (cap * w))()
    labels = (C.c_int32 * cap)()
    n = C.c_size_t(0)
    if predicates is not None or actions is not None:
        rc = _lib.rtla_sim_walk_pred(C.byref(cc), arr, seed, walk, depth, _set_handle(predicates, False),
                                     _set_handle(actions, True), rows, labels, cap, C.byref(n))
        if rc < 0:
            raise RtlaError(rc, "rtla_sim_walk_pred", CAP_SPEC_ERROR if rc == E_SPEC else 0)
    else:
        rc = _check(_lib.rtla_sim_walk(C.byref(cc), arr, seed, walk, depth, rows, labels, cap, C.byref(n)),
                    "rtla_sim_walk")
    return rc == VIOLATION, [(labels[k] & 0xFFFF, (labels[k] >> 16) & 0x7FFF, list(rows[k * w:(k + 1) * w]))
                             for k in range(n.value)]


def inv_mask_of(invariants) -> int:
    """RTLA_INV_* mask of invariant names (or a mask, passed through)."""
    if isinstance(invariants, int):
        return invariants
    m = 0
    for n in invariants:
        m |= INV_BITS[n]
    return m


def inv_names(mask: int) -> List[str]:
    """The names of a mask's invariants, in bit order."""
    return [n for n, b in INV_BITS.items() if mask & b]


@dataclass
class AuditResult:
    """One Checker.audit() call (rtla_audit_stats)."""
    status: int = OK               # OK or VIOLATION
    audited: int = 0               # rows of the frontier
    evaluated: int = 0             # states evaluated: the rows, or (succ) their enabled successors
    counts: dict = field(default_factory=dict)  # invariant name -> evaluated states that violate it
    kernel_ms: float = 0.0
    row_bytes: int = 0
    violation: Optional[List[str]] = None  # the reported state's violated invariants, in bit order
    viol_index: Optional[int] = None       # the least frontier index with a violation (as frontier() numbers rows)
    viol_inst: int = -1                    # succ: the least violating action instance of that row
    viol_mask: int = 0
    viol_in_model: bool = True


def _check_rows(fn, what: str, cfg: Config, rows, invariants, succ, *extra):
    cc = cfg.c()
    flat, n = _flat_rows(rows, row_words(cfg))
    masks = (C.c_int32 * max(1, n))()
    counts = (C.c_uint64 * 8)()
    _check(fn(C.byref(cc), flat, n, inv_mask_of(invariants), int(succ), *extra, masks, counts), what)
    return list(masks[:n]), {nm: counts[b.bit_length() - 1] for nm, b in INV_BITS.items()}


def check_batch(cfg: Config, rows, invariants, succ: bool = False):
    """Invariants evaluated outside the search, on the GPU (rtla_check_batch):
    (masks, counts) -- masks[k] the violated mask of rows[k] (succ: the OR over
    its enabled successors, evaluated as parent + delta), counts[name] the
    evaluated states violating it.  `invariants` (names or a mask) is
    independent of cfg.invariants."""
    return _check_rows(_lib.rtla_check_batch, "rtla_check_batch", cfg, rows, invariants, succ)


def check_replay(cfg: Config, rows, invariants, succ: bool = False, threads: int = 0):
    """The same on the host (rtla_check_replay): no GPU, no context."""
    return _check_rows(_lib.rtla_check_replay, "rtla_check_replay", cfg, rows, invariants, succ, threads)


def _check(st: int, what: str):
    if st < 0:
        raise RtlaError(st, what)
    return st


class Predicates:
    """A compiled set of user-defined state predicates (rtla_pred_compile):
    `text` holds up to 8 definitions `Name == expr` in the predicate language
    (specs/MCPredicates.tla), compiled for cfg's row
    layout.  A syntax, type or bound error raises RtlaError(E_ARG) whose
    message starts with line:col.  Use as a context manager, or leave it to
    the garbage collector.

    step=True (or the Actions subclass) compiles the text's action definitions
    `Name == [][expr]_vars` instead (rtla_pred_compile_step; DESIGN.md section
    14, specs/MCActions.tla): `names` are the action definitions, the state
    definitions of the same text are checked and skipped.  A set knows its
    kind: a state set goes to pred_replay / pred_batch / audit_predicates, a
    step set to pred_step_replay / pred_step_batch / audit_steps."""

    def __init__(self, cfg: Config, text: str, step: bool = False):
        self.cfg = cfg
        self.step = bool(step)
        self._h = None
        cc = cfg.c()
        h = C.c_void_p()
        err = C.create_string_buffer(512)
        what = "rtla_pred_compile_step" if step else "rtla_pred_compile"
        rc = getattr(_lib, what)(C.byref(cc), text.encode(), C.byref(h), err, len(err))
        if rc < 0:
            raise RtlaError(rc, what + ": " + err.value.decode() if err.value else what)
        self._h = h
        buf = C.create_string_buffer(256)
        self.names: List[str] = []
        for k in range(_check(_lib.rtla_pred_count(h), "rtla_pred_count")):
            _check(_lib.rtla_pred_name(h, k, buf, len(buf)), "rtla_pred_name")
            self.names.append(buf.value.decode())

    def names_of(self, mask: int) -> List[str]:
        """The names of a mask's definitions, in definition order."""
        return [n for k, n in enumerate(self.names) if mask >> k & 1]

    def close(self):
        if self._h:
            _lib.rtla_pred_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Actions(Predicates):
    """A compiled set of action properties: Predicates(cfg, text, step=True)."""

    def __init__(self, cfg: Config, text: str):
        super().__init__(cfg, text, step=True)


def _pred_rows(fn, what: str, preds: Predicates, rows, *extra, steps: bool = False):
    cc = preds.cfg.c()
    flat, n = _flat_rows(rows, row_words(preds.cfg))
    masks = (C.c_int32 * max(1, n))()
    counts = (C.c_uint64 * 8)()
    evaluated = C.c_uint64(0)
    rc = fn(C.byref(cc), preds._h, flat, n, *extra, masks, counts, *([C.byref(evaluated)] if steps else []))
    if rc < 0:
        raise RtlaError(rc, what, CAP_SPEC_ERROR if rc == E_SPEC else 0)
    res = list(masks[:n]), {nm: counts[k] for k, nm in enumerate(preds.names)}
    return res + (evaluated.value,) if steps else res


def pred_replay(preds: Predicates, rows, threads: int = 0):
    """A predicate set evaluated on the host (rtla_pred_replay; no GPU, no
    context): (masks, counts) -- masks[k] the definitions FALSE on rows[k] (bit
    d = preds.names[d]), counts[name] the rows on which it is false.  An
    evaluation error raises RtlaError(E_SPEC)."""
    return _pred_rows(_lib.rtla_pred_replay, "rtla_pred_replay", preds, rows, threads)


def pred_batch(preds: Predicates, rows):
    """The same on the GPU (rtla_pred_batch: rtla_kpred.hip)."""
    return _pred_rows(_lib.rtla_pred_batch, "rtla_pred_batch", preds, rows)


def pred_step_replay(actions: Predicates, rows, threads: int = 0):
    """An action set evaluated on the host (rtla_pred_step_replay) on every step
    (rows[k], enabled successor): (masks, counts, evaluated) -- masks[k] the OR
    over the steps out of rows[k] of the definitions false on the step,
    counts[name] the steps on which it is false, evaluated the steps.  A
    stuttering step satisfies every definition; an evaluation error on any
    step raises RtlaError(E_SPEC)."""
    return _pred_rows(_lib.rtla_pred_step_replay, "rtla_pred_step_replay", actions, rows, threads, steps=True)


def pred_step_batch(actions: Predicates, rows):
    """The same on the GPU (rtla_pred_step_batch: k_pred_step, rtla_kpred.hip)."""
    return _pred_rows(_lib.rtla_pred_step_batch, "rtla_pred_step_batch", actions, rows, steps=True)


@dataclass
class ConstrainResult:
    """One Checker.constrain() call (rtla_constrain_stats)."""
    status: int = OK               # OK, or DONE when no row is kept
    level: int = 0
    examined: int = 0              # rows of the level before the call
    kept: int = 0                  # rows on which every definition is TRUE: the frontier now
    dropped: int = 0
    counts: dict = field(default_factory=dict)  # definition name -> rows on which it is false
    start: int = 0                 # arena row of the level's first state
    eval_ms: float = 0.0
    move_ms: float = 0.0
    distinct_total: int = 0        # after the drop


def constrain_batch(preds: Predicates, rows, side=None, ring_cap: int = 0, ring_start: int = 0, chunk: int = 0):
    """The constraint pass on host rows (rtla_constrain_batch: the kernels of
    Checker.constrain, stateless): the rows are laid into a device ring of
    ring_cap rows (0: just room for them) from row ring_start on, wrapping if
    they must, and compacted in chunks of `chunk` rows (0: the default).
    Returns (kept rows in order, the kept entries of `side` -- one integer per
    row, default range(n) -- and counts[name], the rows on which it is false).
    An evaluation error raises RtlaError(E_SPEC)."""
    cc = preds.cfg.c()
    w = row_words(preds.cfg)
    flat, n = _flat_rows(rows, w)
    par = (C.c_uint64 * max(1, n))(*(range(n) if side is None else side))
    out = (C.c_uint32 * max(1, n * w))()
    kept = C.c_size_t(0)
    counts = (C.c_uint64 * 8)()
    cap = ring_cap or ((n + 63) // 64 * 64 or 64)
    rc = _lib.rtla_constrain_batch(C.byref(cc), preds._h, flat, n, cap, ring_start, chunk, out, par, C.byref(kept),
                                   counts)
    if rc < 0:
        raise RtlaError(rc, "rtla_constrain_batch", CAP_SPEC_ERROR if rc == E_SPEC else 0)
    k = kept.value
    return ([list(out[i * w:(i + 1) * w]) for i in range(k)], list(par[:k]),
            {nm: counts[d] for d, nm in enumerate(preds.names)})


def row_words(cfg: Config) -> int:
    cc = cfg.c()
    return _check(_lib.rtla_row_words(C.byref(cc)), "rtla_row_words")


ROW_LAYOUT_KEYS = ("W", "off_hdr", "off_srv", "srv_words", "off_all", "all_words", "off_elec", "elec_words",
                   "off_bag", "slot_words")


def row_layout(cfg: Config) -> dict:
    """Geometry of the packed row (rtla_model.h make_layout): word offsets and record sizes."""
    cc = cfg.c()
    out = (C.c_int32 * len(ROW_LAYOUT_KEYS))()
    n = _check(_lib.rtla_row_layout(C.byref(cc), out, len(ROW_LAYOUT_KEYS)), "rtla_row_layout")
    return dict(zip(ROW_LAYOUT_KEYS[:n], list(out)[:n]))


def init_row(cfg: Config):
    cc = cfg.c()
    w = row_words(cfg)
    buf = (C.c_uint32 * w)()
    _check(_lib.rtla_init_row(C.byref(cc), buf), "rtla_init_row")
    return list(buf)


def state_text(cfg: Config, row: Sequence[int]) -> str:
    cc = cfg.c()
    arr = (C.c_uint32 * len(row))(*row)
    cap = 1 << 16
    while True:
        buf = C.create_string_buffer(cap)
        st = _lib.rtla_state_text(C.byref(cc), arr, buf, cap)
        if st >= 0:
            return buf.value.decode()
        cap *= 4
        if cap > 1 << 26:
            raise RtlaError(st, "rtla_state_text")


def action_name(cfg: Config, inst: int, sub: int) -> str:
    cc = cfg.c()
    buf = C.create_string_buffer(256)
    _check(_lib.rtla_action_name(C.byref(cc), inst, sub, buf, 256), "rtla_action_name")
    return buf.value.decode()


def invariants_violated(cfg: Config, row: Sequence[int]) -> int:
    cc = cfg.c()
    arr = (C.c_uint32 * len(row))(*row)
    return _check(_lib.rtla_invariants(C.byref(cc), arr), "rtla_invariants")


def row_fingerprint(cfg: Config, row: Sequence[int]):
    """(a, b) recomputed from scratch; the row stores the incrementally derived one in words 0-3."""
    cc = cfg.c()
    arr = (C.c_uint32 * len(row))(*row)
    out = (C.c_uint64 * 2)()
    _check(_lib.rtla_row_fingerprint(C.byref(cc), arr, out), "rtla_row_fingerprint")
    return out[0], out[1]


def orbit_key(cfg: Config, row: Sequence[int]):
    """SYMMETRY seen-set key of the row's orbit and the number of permutation
    images it compared (rtla_model.h sym_key; host)."""
    cc = cfg.c()
    arr = (C.c_uint32 * len(row))(*row)
    out = (C.c_uint64 * 2)()
    n = C.c_int(0)
    _check(_lib.rtla_orbit_key(C.byref(cc), arr, out, C.byref(n)), "rtla_orbit_key")
    return (out[0], out[1]), n.value


def permute_row(cfg: Config, row: Sequence[int], pi: Sequence[int]):
    """The server-permuted image of a row (server i moved to pi[i])."""
    cc = cfg.c()
    arr = (C.c_uint32 * len(row))(*row)
    p = (C.c_int * len(pi))(*pi)
    out = (C.c_uint32 * len(row))()
    _check(_lib.rtla_permute_row(C.byref(cc), arr, p, out), "rtla_permute_row")
    return list(out)


def rows_text_hash(cfg: Config, rows: Sequence[Sequence[int]], threads: int = 0) -> int:
    """Sum mod 2^64 of FNV-1a-64(state_text) over the rows: the oracle's
    per-level digest of a set of states (host threads, rtla_rows_text_hash)."""
    cc = cfg.c()
    w = row_words(cfg)
    n = len(rows)
    flat = (C.c_uint32 * max(1, n * w))()
    for k, r in enumerate(rows):
        flat[k * w:(k + 1) * w] = list(r)
    out = C.c_uint64(0)
    _check(_lib.rtla_rows_text_hash(C.byref(cc), flat, n, threads, C.byref(out)), "rtla_rows_text_hash")
    return out.value


def rows_orbit_hash(cfg: Config, rows: Sequence[Sequence[int]], threads: int = 0) -> int:
    """Sum mod 2^64 of FNV-1a-64 of each row's ORBIT TEXT (rtla_rows_orbit_hash):
    a SYMMETRY level's digest, whichever member of each orbit a row holds."""
    cc = cfg.c()
    w = row_words(cfg)
    n = len(rows)
    flat = (C.c_uint32 * max(1, n * w))()
    for k, r in enumerate(rows):
        flat[k * w:(k + 1) * w] = list(r)
    out = C.c_uint64(0)
    _check(_lib.rtla_rows_orbit_hash(C.byref(cc), flat, n, threads, C.byref(out)), "rtla_rows_orbit_hash")
    return out.value


def orbit_text(cfg: Config, row: Sequence[int]) -> str:
    """The text of the orbit representative whose rotated text is least
    (rtla_orbit_text; the item of a SYMMETRY level digest)."""
    cc = cfg.c()
    arr = (C.c_uint32 * len(row))(*row)
    cap = 1 << 16
    while True:
        buf = C.create_string_buffer(cap)
        st = _lib.rtla_orbit_text(C.byref(cc), arr, buf, cap)
        if st >= 0:
            return buf.value.decode()
        cap *= 4
        if cap > 1 << 26:
            raise RtlaError(st, "rtla_orbit_text")


def random_texts(cfg: Config, first: int, n: int, pool: int = 0, seed: int = SYNTH_SEED) -> bytes:
    """The synthetic input states first .. first + n - 1 as state texts, each
    terminated by '\x1e' (rtla_random_texts; host)."""
    cc = cfg.c()
    need = C.c_size_t(0)
    cap = n * 2048  # a random state's text is ~1 KB; the rare larger batch is rendered again at its exact size
    buf = C.create_string_buffer(cap)
    if _lib.rtla_random_texts(C.byref(cc), seed, first, n, pool, buf, cap, C.byref(need)) != OK:
        buf = C.create_string_buffer(need.value + 1)
        _check(_lib.rtla_random_texts(C.byref(cc), seed, first, n, pool, buf, need.value, C.byref(need)),
               "rtla_random_texts")
    return buf.raw[:need.value]


def stored_fingerprint(row: Sequence[int]):
    return row[0] | row[1] << 32, row[2] | row[3] << 32


def random_rows(cfg: Config, first: int, n: int, pool: int = 0, seed: int = SYNTH_SEED):
    """Rows of the synthetic microbench's input states first .. first + n - 1
    (rtla_synth.h; computed on the host)."""
    w = row_words(cfg)
    cc = cfg.c()
    buf = (C.c_uint32 * max(1, n * w))()
    _check(_lib.rtla_random_rows(C.byref(cc), seed, first, n, pool, buf), "rtla_random_rows")
    return [list(buf[k * w:(k + 1) * w]) for k in range(n)]


def expand_batch(cfg: Config, rows: Sequence[Sequence[int]]):
    """GPU successor generation (TLC getNextStates) for a batch of rows.

    Returns a list of (input index, instance, receive-sub, in_model, row),
    sorted by (input, instance)."""
    cc = cfg.c()
    w = row_words(cfg)
    n = len(rows)
    flat = (C.c_uint32 * (max(n, 1) * w))()
    for k, r in enumerate(rows):
        assert len(r) == w, "row width mismatch"
        flat[k * w:(k + 1) * w] = list(r)
    cap = max(n, 1) * 512
    succ = (C.c_uint32 * (cap * w))()
    info = (C.c_uint64 * cap)()
    nout = C.c_size_t(0)
    _check(_lib.rtla_expand_batch(C.byref(cc), flat, n, succ, info, cap, C.byref(nout)),
           "rtla_expand_batch")
    out = []
    for k in range(nout.value):
        v = info[k]
        out.append((v >> 32, v & 0xFFFF, (v >> 16) & 0x7FFF, bool(v >> 31 & 1),
                    list(succ[k * w:(k + 1) * w])))
    return out


class Checker:
    """One BFS context on one GPU (rank)."""

    def __init__(self, cfg: Config, rank: int = 0, world: int = 1, comm_id: bytes = None):
        self.cfg = cfg
        self._cc = cfg.c()
        h = C.c_void_p()
        cid = C.create_string_buffer(comm_id, 128) if comm_id else None
        _check(_lib.rtla_open(C.byref(self._cc), rank, world, cid, C.byref(h)), "rtla_open")
        self._h = h
        self._recovered = False
        self._pred_viol: Optional[List[str]] = None  # the false definitions of the last audit_predicates violation
        self.levels: List[Level] = []
        self.status = OK

    def close(self):
        if self._h:
            _lib.rtla_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def device_info(self) -> str:
        buf = C.create_string_buffer(4096)
        _check(_lib.rtla_device_info(self._h, buf, 4096), "rtla_device_info")
        return buf.value.decode()

    def _rec(self, st: _Stats):
        self.levels.append(Level(st.level, st.frontier, st.new_states, st.generated, st.seconds,
                                 st.kernel_ms, st.probes, st.row_bytes, st.expand_ms))
        self.distinct, self.generated = st.distinct_total, st.generated_total

    def init(self, roots=None) -> int:
        """Level 1: Init -- or, roots given (a list of rows, or rows already
        flat), those rows (rtla_init_rows: TLC's INIT override for explicit
        states).  Equal roots count once; a root that violates an invariant
        gives VIOLATION and a one-row trace; such a search has no checkpoint."""
        st = _Stats()
        if roots is None:
            self.status = _check(_lib.rtla_init(self._h, C.byref(st)), "rtla_init")
        else:
            flat, n = _flat_rows(roots, row_words(self.cfg))
            self.status = _check(_lib.rtla_init_rows(self._h, flat, n, C.byref(st)), "rtla_init_rows")
        self._rec(st)
        return self.status

    def reset(self):
        _check(_lib.rtla_reset(self._h), "rtla_reset")
        self._pred_viol = None
        self.levels = []
        self.status = OK

    def step(self) -> int:
        """One BFS level.  Raises RtlaError (with .flags naming the capacity
        that ran out) if the level could not be completed."""
        st = _Stats()
        self._pred_viol = None
        rc = _lib.rtla_step(self._h, C.byref(st))
        if rc < 0:
            self.status = rc
            raise RtlaError(rc, "rtla_step", st.flags)
        self.status = rc
        self._rec(st)
        return self.status

    def run(self, max_levels: int = 100000, predicates: Optional[Predicates] = None,
            actions: Optional[Predicates] = None, roots=None, constraint: Optional[Predicates] = None) -> int:
        """BFS until the search ends, a violation or max_levels.  roots: the
        rows level 1 holds instead of Init (init(roots)).  predicates: a
        set audited on every level right after it is produced, Init's included
        (audit_predicates); the run stops with VIOLATION at the first level that
        holds a state on which a definition is false.  constraint: a state set
        that prunes every level, Init's included, after the predicates have
        seen it whole (constrain; TLC's CONSTRAINT): dropped states are neither
        counted nor expanded.  actions: a step set checked after them on the
        steps out of every level's kept rows (audit_steps), before the next
        step(): every step out of every reachable in-model state is checked,
        and the run stops at the first level with a false step."""
        def audited() -> int:
            if self.status == OK and self.levels[-1].new > 0:  # (the last, empty level is skipped)
                if predicates is not None and self.audit_predicates(predicates).status == VIOLATION:
                    self.status = VIOLATION
                elif constraint is not None and self.constrain(constraint).status == DONE:
                    pass  # (constrain set the status: nothing is left to expand)
                elif actions is not None and self.audit_steps(actions).status == VIOLATION:
                    self.status = VIOLATION
            return self.status

        if not self.levels and not self._recovered:
            if self.init(roots) != OK or audited() != OK:
                return self.status
        while self.status == OK and len(self.levels) < max_levels:
            self.step()
            audited()
        return self.status

    def violation(self):
        m, im = C.c_int32(0), C.c_int32(0)
        _lib.rtla_violation(self._h, C.byref(m), C.byref(im))
        if self._pred_viol is not None:  # (definition bits, not RTLA_INV_*)
            return ", ".join(self._pred_viol), bool(im.value)
        names = [n for n, b in INV_BITS.items() if m.value & b]
        return (names[0] if names else None), bool(im.value)

    def trace(self) -> List[Tuple[str, str]]:
        w = row_words(self.cfg)
        n = C.c_size_t(0)
        _lib.rtla_trace(self._h, None, None, 0, C.byref(n))
        cap = n.value
        rows = (C.c_uint32 * (cap * w))()
        labels = (C.c_int32 * cap)()
        _check(_lib.rtla_trace(self._h, rows, labels, cap, C.byref(n)), "rtla_trace")
        out = []
        for k in range(n.value):
            lab = labels[k]
            name = "Initial predicate" if lab < 0 else action_name(self.cfg, lab & 0xFFFF, (lab >> 16) & 0x7FFF)
            out.append((name, state_text(self.cfg, list(rows[k * w:(k + 1) * w]))))
        return out

    def frontier(self):
        """Rows of the level last produced (debug / parity)."""
        w = row_words(self.cfg)
        n = C.c_size_t(0)
        _check(_lib.rtla_frontier(self._h, None, 0, C.byref(n)), "rtla_frontier")
        buf = (C.c_uint32 * max(1, n.value * w))()
        _check(_lib.rtla_frontier(self._h, buf, n.value, C.byref(n)), "rtla_frontier")
        return [list(buf[k * w:(k + 1) * w]) for k in range(n.value)]

    def frontier_flat(self):
        """The same rows as one flat ctypes u32 array (frontier_size() * row_words): a large level without a
        Python list per state, e.g. as sim_replay's start rows."""
        w = row_words(self.cfg)
        n = C.c_size_t(0)
        _check(_lib.rtla_frontier(self._h, None, 0, C.byref(n)), "rtla_frontier")
        buf = (C.c_uint32 * (n.value * w))()
        _check(_lib.rtla_frontier(self._h, buf, n.value, C.byref(n)), "rtla_frontier")
        return buf

    def frontier_size(self) -> int:
        n = C.c_size_t(0)
        _check(_lib.rtla_frontier(self._h, None, 0, C.byref(n)), "rtla_frontier")
        return n.value

    def frontier_rows(self, index: Sequence[int]):
        """Rows index[k] of the level last produced (numbered as frontier()
        lists them): samples of a level too large to copy whole."""
        w = row_words(self.cfg)
        idx = (C.c_uint64 * max(1, len(index)))(*index)
        buf = (C.c_uint32 * max(1, len(index) * w))()
        _check(_lib.rtla_frontier_rows(self._h, idx, len(index), buf), "rtla_frontier_rows")
        return [list(buf[k * w:(k + 1) * w]) for k in range(len(index))]

    def level_text_hash(self, threads: int = 0) -> int:
        """Digest of the level last produced (all shards / ranks): sum mod 2^64
        of FNV-1a-64 of each state's text, decoded on the host from the device
        rows in chunks -- compared with the oracle's level_text_hash."""
        out = C.c_uint64(0)
        _check(_lib.rtla_level_text_hash(self._h, threads, C.byref(out)), "rtla_level_text_hash")
        return out.value

    def level_orbit_hash(self, threads: int = 0) -> int:
        """SYMMETRY: the level's digest over orbit texts (rtla_level_orbit_hash),
        compared with the oracle's per-level orbit digest."""
        out = C.c_uint64(0)
        _check(_lib.rtla_level_orbit_hash(self._h, threads, C.byref(out)), "rtla_level_orbit_hash")
        return out.value

    def checkpoint(self, prefix: str):
        """TLC -checkpoint: write the search to <prefix>.shard<id>.rtla (between levels)."""
        _check(_lib.rtla_checkpoint(self._h, prefix.encode()), "rtla_checkpoint")

    def recover(self, prefix: str):
        """TLC -recover: resume a checkpoint written by a context of the same configuration."""
        _check(_lib.rtla_recover(self._h, prefix.encode()), "rtla_recover")
        self.status = OK
        self._recovered = True

    def time_expand(self, xflags: int, reps: int = 3) -> float:
        """Diagnostic: mean ms of re-expanding the current frontier (pollutes the search)."""
        ms = C.c_double()
        _check(_lib.rtla_time_expand(self._h, xflags, reps, C.byref(ms)), "rtla_time_expand")
        return ms.value

    def synthetic_step(self, first: int, n: int, pool: int = 0, seed: int = SYNTH_SEED) -> Level:
        """BASELINE configs[4]: n random states through Next + fingerprint +
        dedup (one level-kernel launch; the set accumulates across calls)."""
        st = _Stats()
        rc = _lib.rtla_synthetic_step(self._h, seed, first, n, pool, C.byref(st))
        if rc < 0:
            raise RtlaError(rc, "rtla_synthetic_step", st.flags)
        return Level(0, st.frontier, st.new_states, st.generated, st.seconds, st.kernel_ms, st.probes, st.row_bytes,
                     st.expand_ms)

    def synthetic_generate(self, first: int, n: int, pool: int = 0, at: int = 0, seed: int = SYNTH_SEED):
        """Input states first .. first + n - 1 into row-arena rows at .. at + n - 1 (on the device)."""
        _check(_lib.rtla_synthetic_generate(self._h, seed, first, n, pool, at), "rtla_synthetic_generate")

    def synthetic_dedup(self, begin: int, end: int) -> Level:
        """One dedup-only level-kernel launch over the resident arena rows [begin, end)."""
        st = _Stats()
        rc = _lib.rtla_synthetic_dedup(self._h, begin, end, C.byref(st))
        if rc < 0:
            raise RtlaError(rc, "rtla_synthetic_dedup", st.flags)
        return Level(0, st.frontier, st.new_states, st.generated, st.seconds, st.kernel_ms, st.probes, st.row_bytes,
                     st.expand_ms)

    def simulate(self, n_walks: int, depth: int, seed: int = SIM_SEED, first: int = 0, ends: bool = False,
                 predicates=None, actions=None) -> SimResult:
        """TLC -simulate: walks first .. first + n_walks - 1 of up to `depth`
        steps from the states of the level last produced (walk w starts at
        frontier row w mod frontier_size()).  The BFS is left untouched; after
        a VIOLATION result, violation() and trace() give the counterexample.
        predicates / actions: a compiled state set / action set the walks carry
        (rtla_simulate_pred): the action set is checked
        on every step out of every state a walk visits, the state set on every
        in-model successor, and a walk ends at the first successor on which a
        built-in invariant or a definition is false.  The sets never change
        which walk is taken."""
        self._pred_viol = None
        if predicates is not None or actions is not None:
            buf = (C.c_uint64 * max(1, 5 * n_walks))() if ends else None
            st, pst = _SimStats(), _SimPredStats()
            rc = _lib.rtla_simulate_pred(self._h, seed, first, n_walks, depth, _set_handle(predicates, False),
                                         _set_handle(actions, True), buf, C.byref(st), C.byref(pst))
            if rc < 0:
                raise RtlaError(rc, "rtla_simulate_pred", st.flags)
            res = _sim_result(rc, st, buf, n_walks, pst, predicates, actions)
            if rc == VIOLATION:
                self._pred_viol = res.violation.split(", ")
            return res
        buf = (C.c_uint64 * max(1, 4 * n_walks))() if ends else None
        st = _SimStats()
        rc = _lib.rtla_simulate(self._h, seed, first, n_walks, depth, buf, C.byref(st))
        if rc < 0:
            raise RtlaError(rc, "rtla_simulate", st.flags)
        return _sim_result(rc, st, buf, n_walks)

    def audit(self, invariants, succ: bool = False) -> AuditResult:
        """Evaluate `invariants` (names or a mask; independent of the context's
        own) over the states of the level last produced, in place on the GPU --
        or, succ=True, over their enabled successors.  The BFS is left
        untouched; after a VIOLATION result, violation() and trace() give the
        counterexample (for succ, ending in the violating successor)."""
        st = _AuditStats()
        self._pred_viol = None
        rc = _lib.rtla_check_frontier(self._h, inv_mask_of(invariants), int(succ), C.byref(st))
        if rc < 0:
            raise RtlaError(rc, "rtla_check_frontier", st.flags)
        res = AuditResult(status=rc, audited=st.audited, evaluated=st.evaluated, kernel_ms=st.kernel_ms,
                          row_bytes=st.row_bytes,
                          counts={nm: st.counts[b.bit_length() - 1] for nm, b in INV_BITS.items()})
        if rc == VIOLATION:
            res.violation = inv_names(st.viol_mask)
            res.viol_index, res.viol_inst = st.viol_index, st.viol_inst
            res.viol_mask, res.viol_in_model = st.viol_mask, bool(st.viol_in_model)
        return res

    def audit_predicates(self, preds: Predicates) -> AuditResult:
        """Evaluate a compiled predicate set over the states of the level last
        produced, in place on the GPU (rtla_pred_frontier).  counts and
        violation name definitions; otherwise as audit(): the BFS is left
        untouched, and after a VIOLATION result violation() and trace() give the
        counterexample, until the next step, audit or simulation."""
        return self._audit_set(_lib.rtla_pred_frontier, "rtla_pred_frontier", preds)

    def audit_steps(self, actions: Predicates) -> AuditResult:
        """Evaluate a compiled action set on every step out of the states of
        the level last produced, in place on the GPU (rtla_pred_step_frontier):
        audited is the rows, evaluated the steps, counts[name] the steps on
        which it is false.  After a VIOLATION result, viol_index / viol_inst
        name the least (row, action instance) with a false definition, and
        trace() ends in that step: the row, then its successor."""
        return self._audit_set(_lib.rtla_pred_step_frontier, "rtla_pred_step_frontier", actions)

    def constrain(self, preds: Predicates) -> ConstrainResult:
        """Prune the level last produced by a compiled state set, in place on
        the GPU (rtla_pred_constrain; TLC's CONSTRAINT):
        a row is kept iff every definition is TRUE on it; kept rows keep their
        order.  levels[-1].new and distinct become the post-drop values, and
        everything that reads the level afterwards -- step, audits, simulate,
        digests, checkpoint -- sees the kept rows only.  Status DONE: no row is
        kept and the search is finished.  An evaluation error raises
        RtlaError(E_SPEC) and leaves the level as it was."""
        st = _ConstrainStats()
        self._pred_viol = None
        rc = _lib.rtla_pred_constrain(self._h, _set_handle(preds, False), C.byref(st))
        if rc < 0:
            raise RtlaError(rc, "rtla_pred_constrain", st.flags)
        if self.levels:
            self.levels[-1].new = st.kept
        self.distinct = st.distinct_total
        if rc == DONE:
            self.status = DONE
        return ConstrainResult(status=rc, level=st.level, examined=st.examined, kept=st.kept, dropped=st.dropped,
                               counts={nm: st.counts[k] for k, nm in enumerate(preds.names)}, start=st.start,
                               eval_ms=st.eval_ms, move_ms=st.move_ms, distinct_total=st.distinct_total)

    def _audit_set(self, fn, what: str, preds: Predicates) -> AuditResult:
        st = _AuditStats()
        self._pred_viol = None
        rc = fn(self._h, preds._h, C.byref(st))
        if rc < 0:
            raise RtlaError(rc, what, st.flags)
        res = AuditResult(status=rc, audited=st.audited, evaluated=st.evaluated, kernel_ms=st.kernel_ms,
                          row_bytes=st.row_bytes, counts={nm: st.counts[k] for k, nm in enumerate(preds.names)})
        if rc == VIOLATION:
            res.violation = preds.names_of(st.viol_mask)
            res.viol_index, res.viol_inst = st.viol_index, st.viol_inst
            res.viol_mask, res.viol_in_model = st.viol_mask, bool(st.viol_in_model)
            self._pred_viol = res.violation
        return res

    def coverage(self) -> dict:
        n = len(COVER_NAMES)
        g, d = (C.c_uint64 * n)(), (C.c_uint64 * n)()
        _check(_lib.rtla_coverage(self._h, g, d, n), "rtla_coverage")
        return {COVER_NAMES[k]: (g[k], d[k]) for k in range(n)}


def check(cfg: Config, trace: bool = True, predicates: Optional[Predicates] = None,
          actions: Optional[Predicates] = None, roots=None, constraint: Optional[Predicates] = None) -> Result:
    """Exhaustive BFS of the model (TLC `-workers N` breadth-first mode), from
    Init or from the rows `roots` (Checker.init).
    predicates: user-defined invariants checked on every level (Checker.run);
    actions: action properties checked on the steps out of every level;
    Result.violation then names the false definitions.  constraint: a state
    set that prunes every level (TLC's CONSTRAINT; Checker.constrain): the
    counts, the depth and the levels are those of the constrained search."""
    with Checker(cfg) as ck:
        st = ck.run(predicates=predicates, actions=actions, roots=roots, constraint=constraint)
        res = Result(distinct=ck.distinct, generated=ck.generated, levels=list(ck.levels))
        res.depth = sum(1 for lv in ck.levels if lv.new > 0)
        res.seconds = sum(lv.seconds for lv in ck.levels)
        res.coverage = ck.coverage()
        if st == VIOLATION:
            res.violation, res.violation_in_model = ck.violation()
            if trace:
                res.trace = ck.trace()
        return res


def comm_id() -> bytes:
    """A fresh RCCL unique id (rank 0 makes it, every rank passes it to Checker)."""
    buf = C.create_string_buffer(128)
    _check(_lib.rtla_comm_id(buf), "rtla_comm_id")
    return buf.raw


def probe_bench2(log2: int, n: int):
    """(s_insert, s_seen_cas, s_seen_load, inserted) for n random keys, see rtla.h."""
    a, b, c, ins = C.c_double(0), C.c_double(0), C.c_double(0), C.c_uint64(0)
    _check(_lib.rtla_probe_bench2(log2, n, C.byref(a), C.byref(b), C.byref(c), C.byref(ins)), "rtla_probe_bench2")
    return a.value, b.value, c.value, ins.value


def probe_mixed(log2: int, n_present: int, n: int, new_frac: float):
    """(seconds, inserted): n load-first probes into a 2^log2 table holding
    n_present keys, a fraction new_frac of them new keys (rtla_probe_bench3)."""
    sec, ins = C.c_double(0), C.c_uint64(0)
    _check(_lib.rtla_probe_bench3(log2, n_present, n, new_frac, C.byref(sec), C.byref(ins)), "rtla_probe_bench3")
    return sec.value, ins.value


def probe_bench(log2: int, n: int):
    s, ins = C.c_double(0), C.c_uint64(0)
    _check(_lib.rtla_probe_bench(log2, n, C.byref(s), C.byref(ins)), "rtla_probe_bench")
    return s.value, ins.value


FPSET_INSERT, FPSET_CAS_RESOLVE, FPSET_LOAD_RESOLVE, FPSET_REMOTE = 0, 1, 2, 3  # rtla_fpset_probe's protocols


def fpset_probe_status(log2: int, fps, protocol: int, table=None):
    """rtla_fpset_probe as it is: (status, new, table, flags) -- fps an (n, 2)
    numpy u64 array of (a, b) pairs, table 2^log2 u64 (None = empty; left
    unchanged).  Raises only where the call filled no output."""
    import numpy as np
    fps = np.ascontiguousarray(fps, dtype=np.uint64).reshape(-1, 2)
    valid = 10 <= log2 <= 30  # (else the call refuses, and touches no buffer)
    out = np.zeros(1 << log2 if valid else 1, np.uint64) if table is None else np.array(table, dtype=np.uint64)
    if valid and out.shape != (1 << log2,):
        raise ValueError("table must hold 2^log2 u64")
    new = np.zeros(len(fps), np.uint8)
    flags = C.c_int32(0)
    rc = _lib.rtla_fpset_probe(log2, fps.ctypes.data, len(fps), protocol, out.ctypes.data, new.ctypes.data,
                               C.byref(flags))
    if rc < 0 and rc != E_OVERFLOW:
        raise RtlaError(rc, "rtla_fpset_probe", flags.value)
    return rc, new, out, flags.value


def fpset_probe(log2: int, fps, protocol: int, table=None):
    """The kernels' fingerprint-set insert on chosen fingerprints
    (rtla_fpset_probe): input i is inserted by global thread i with protocol
    0 (fpset_insert), 1 (home CAS + fpset_resolve) or 2 (home load +
    fpset_resolve_loaded); 3 runs k_insert_remote on the inputs.  Returns (new, table, flags): one byte per input,
    the table afterwards, RTLA_CAP_FPSET in flags when an insert hit the probe
    limit (the outputs are complete either way)."""
    return fpset_probe_status(log2, fps, protocol, table)[1:]
