/*
 * rtla.h -- C ABI of the MI355X-native Raft model checker (librtla.so).
 *
 * What this boundary replaces.  The reference (bernborgess/raft-tla) is a
 * TLA+ spec run by TLC:
 *     java tlc2.TLC [-workers W] [-coverage 1] -config raft.cfg raft.tla
 * (/root/reference/raft.cfg:1-15 is the model, /root/reference/.vscode/
 * settings.json:5 the "-coverage 1" option).  The hot path behind that command
 * is TLC's breadth-first exploration of Spec == Init /\ [][Next]_vars
 * (/root/reference/raft.tla:469, Next at :454-465): expand every frontier
 * state, fingerprint each successor, deduplicate against the seen set, check
 * invariants, enqueue.  Each entry point below replaces one piece of it:
 *
 *   rtla_open / rtla_close   TLC's model setup from the cfg's CONSTANTS
 *                            (raft.cfg:5-15) and its FPSet / StateQueue
 *                            allocation (the `states/` dir, reference
 *                            .gitignore:2).
 *   rtla_init                "Computing initial states" -- Init (raft.tla:155-160).
 *   rtla_init_rows           an INIT override (TLC: `INIT MyInit` in the cfg), restricted
 *                            to explicit states: the search starts from given rows.
 *   rtla_step                one BFS level of TLC's worker loop: Next
 *                            (raft.tla:454-465), fingerprint, FPSet.put,
 *                            INVARIANT check (raft.cfg:3), enqueue.
 *   rtla_violation,
 *   rtla_trace               "Error: Invariant X is violated" + "The behavior
 *                            up to this point is:" (TLC's trace file).
 *   rtla_checkpoint,
 *   rtla_recover             TLC's -checkpoint / -recover (the `states/` dir,
 *                            reference .gitignore:2).
 *   rtla_coverage            "-coverage 1" (.vscode/settings.json:5): per-action
 *                            generated / distinct counts.
 *   rtla_expand_batch        TLC's Tool.getNextStates(Next, s) for a batch of
 *                            states: the parity seam used by the tests.
 *   rtla_state_text          TLC's state printer ("/\ var = value" lines).
 *   rtla_simulate            TLC's -simulate [num=N] with -depth D and -seed S:
 *                            random behaviours instead of exhaustive search --
 *                            here started from the states of the BFS level
 *                            last produced ({Init} after rtla_init: TLC's plain
 *                            -simulate), so the search samples beyond the depth
 *                            the frontier arena allows.
 *   rtla_check_frontier,
 *   rtla_check_batch,
 *   rtla_check_replay        TLC has no counterpart short of a second run with
 *                            another INVARIANT list: any invariant set evaluated
 *                            outside the search, over the states of the level
 *                            last produced (in place in HBM) or a batch of rows.
 *   rtla_pred_compile,
 *   rtla_pred_frontier ...   an operator added to MC.tla and named under
 *                            INVARIANT: a predicate in a TLA+ subset over the
 *                            spec's variables, compiled to a bounded bytecode
 *                            and evaluated by one interpreter on host and GPU.
 *   rtla_pred_compile_step,
 *   rtla_pred_step_frontier ... an action property `Name == [][A]_vars` named
 *                            under PROPERTY: the same bytecode over a step's two
 *                            states, checked on every step out of a BFS level.
 *   rtla_simulate_pred       -simulate with operators of MC.tla named under
 *                            INVARIANT / PROPERTY: the walks carry a compiled
 *                            state set and / or action set (rtla_sim_replay_pred,
 *                            rtla_sim_walk_pred: the same on the host).
 *   rtla_sim_replay,
 *   rtla_sim_walk            the same walks recomputed on the host from
 *                            (seed, walk id): reproduce one behaviour, as TLC
 *                            does when rerun with the -seed it printed.
 *
 * Conventions: the caller owns host buffers, the library owns device memory.
 * Every function returns an int status (RTLA_OK = 0, >0 informational,
 * <0 error).  Nothing is thrown across the ABI.  Capacity overflow of any
 * fixed-width structure is a hard error (RTLA_E_OVERFLOW), never truncation.
 * A context is used from one host thread; one context per GPU (rank).
 */
#ifndef RTLA_H
#define RTLA_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define RTLA_ABI_VERSION 12

/* status codes */
#define RTLA_OK 0
#define RTLA_DONE 1          /* the last level found no new state: search complete */
#define RTLA_VIOLATION 2     /* an invariant is violated; see rtla_violation / rtla_trace */
#define RTLA_E_CONFIG (-1)   /* configuration outside the supported row format */
#define RTLA_E_HIP (-2)      /* HIP runtime error (no device, launch failure, OOM) */
#define RTLA_E_OVERFLOW (-3) /* bag / elections / frontier / fingerprint-set capacity exceeded */
#define RTLA_E_SPEC (-4)     /* TLC evaluation error while evaluating Next */
#define RTLA_E_STATE (-5)    /* call out of order (e.g. step before init) */
#define RTLA_E_ARG (-6)      /* bad argument / buffer too small */
#define RTLA_E_COMM (-7)     /* RCCL error */

/* invariants (definitions: specs/MC.tla) */
#define RTLA_INV_NO_TWO_LEADERS 1
#define RTLA_INV_ELECTION_SAFETY 2
#define RTLA_INV_LOG_MATCHING 4
#define RTLA_INV_STATE_MACHINE_SAFETY 8
#define RTLA_INV_LEADER_COMPLETENESS 16

typedef struct rtla_ctx rtla_ctx;

typedef struct {
    int32_t n_server;    /* |Server|                         (raft.cfg:6)  <= 5 */
    int32_t n_value;     /* |Value|                          (raft.cfg:7)  <= 4 */
    int32_t max_term;    /* StateConstraint: currentTerm <= max_term        <= 6 */
    int32_t max_log;     /* StateConstraint: Len(log) <= max_log            <= 4 */
    int32_t max_copies;  /* StateConstraint: messages[m] <= max_copies      <= 14 */
    int32_t max_msgs;    /* StateConstraint: BagCardinality <= max_msgs; 0 = unbounded */
    int32_t bag_cap;     /* distinct messages per row; 0 = auto (max_msgs + 1, or 32) */
    int32_t elec_cap;    /* election records per row; 0 = auto ((max_term - 1) * n_server) */
    int32_t inv_mask;    /* RTLA_INV_* */
    int32_t symmetry;    /* 1: SYMMETRY Permutations(Server) (specs/MC.tla Perms): orbit counts */
    int32_t fpset_log2;  /* log2(#8-byte slots) of this rank's fingerprint set; 0 = auto */
    int32_t shards;      /* world == 1 only: split the search on this GPU into this many
                            fingerprint-owned shards (same exchange protocol as multi-GPU,
                            transport = device copies); 0/1 = one shard */
    uint64_t frontier_cap; /* rows of the frontier arena (current + next level, used as a ring;
                              rounded down to a multiple of 64); 0 = all HBM left after the other
                              structures */
    uint64_t mem_budget;   /* bytes of HBM this context may use; 0 = 85% of free */
    uint64_t chunk;        /* multi-shard: at most this many frontier states expanded per exchange
                              round; 0 = as many as the outbox allows */
    int32_t mode;          /* RTLA_MODE_BFS (0), or RTLA_MODE_DEDUP: a context for the synthetic
                              microbench only (rtla_synthetic_*; no parent records, so no BFS:
                              rtla_init / rtla_step return RTLA_E_STATE) */
    int32_t reserved;      /* 0 */
} rtla_cfg;

#define RTLA_MODE_BFS 0
#define RTLA_MODE_DEDUP 1

typedef struct {
    int32_t level;            /* BFS level whose states were just produced (Init = 1) */
    int32_t status;           /* RTLA_OK / RTLA_DONE / RTLA_VIOLATION */
    uint64_t frontier;        /* states expanded to produce this level */
    uint64_t new_states;      /* distinct states first found at this level */
    uint64_t generated;       /* successor states generated (incl. out-of-model) */
    uint64_t distinct_total;  /* distinct states found so far (all ranks) */
    uint64_t generated_total; /* states generated so far, Init included (TLC convention) */
    double seconds;           /* wall time of this level (device work + sync) */
    double kernel_ms;         /* k_expand time of this level (HIP events on the context's stream) */
    uint64_t probes;          /* in-model successors (fingerprint-set probes) */
    uint64_t row_bytes;       /* bytes of one packed state row */
    double expand_ms;         /* of kernel_ms: the probe kernel alone (one shard); the rest builds the rows */
    int32_t flags;            /* on RTLA_E_OVERFLOW / RTLA_E_SPEC: which capacity ran out (RTLA_CAP_*);
                                 the level is then incomplete and the search cannot continue */
    int32_t reserved;
} rtla_level_stats;

/* rtla_level_stats.flags */
#define RTLA_CAP_SPEC_ERROR 1     /* TLC evaluation error in Next (index outside DOMAIN) */
#define RTLA_CAP_ROW 2            /* bag_cap / elec_cap of the row format */
#define RTLA_CAP_FRONTIER 4       /* row arena (current + next level) */
#define RTLA_CAP_FPSET 8          /* fingerprint set probe limit */
#define RTLA_CAP_OUTBOX 16        /* multi-shard exchange outbox */

/* Library / context lifetime.  world > 1: `comm_id` is the 128-byte RCCL
 * unique id shared by all ranks (rank 0 makes it with rtla_comm_id). */
int rtla_open(const rtla_cfg *cfg, int rank, int world, const void *comm_id, rtla_ctx **out);
void rtla_close(rtla_ctx *ctx);
int rtla_comm_id(void *out128);

/* BFS. */
int rtla_init(rtla_ctx *ctx, rtla_level_stats *out);
/* rtla_init with level 1 being the n given rows (the roots) instead of Init:
 * the seeded search.  Preconditions as rtla_init's; world == 1 (any number of
 * virtual shards), else RTLA_E_STATE; n == 0 or rows == NULL: RTLA_E_ARG; roots
 * that do not fit a shard's frontier: RTLA_E_OVERFLOW; a row whose message or
 * election count exceeds the layout's: RTLA_E_ARG.  The rows' first four
 * words (the stored fingerprint) are not trusted: they are recomputed as the
 * level kernel stores them for a generated state.  Roots equal by the seen-set
 * key (the fingerprint; under SYMMETRY the orbit key) count once, the first
 * occurrence kept: out->new_states = distinct roots, out->generated = n.  Each
 * root lives on the shard that owns its key, in the given order.  Every
 * distinct root is checked against the configuration's invariants as Init is;
 * the least violating root ends the search with RTLA_VIOLATION and is the
 * whole trace (label -1).  A trace of the seeded search starts at the root the
 * violation descends from ("Init first" below reads "that root first").
 * rtla_checkpoint of a seeded search returns RTLA_E_STATE: a checkpoint does
 * not hold the roots.  rtla_reset forgets them. */
int rtla_init_rows(rtla_ctx *ctx, const uint32_t *rows, size_t n, rtla_level_stats *out);
/* Forget the search (clear the fingerprint set, frontier, counters) but keep
 * the allocations, so the same model can be checked again from Init. */
int rtla_reset(rtla_ctx *ctx);
int rtla_step(rtla_ctx *ctx, rtla_level_stats *out);
int rtla_violation(rtla_ctx *ctx, int32_t *inv_mask, int32_t *in_model);
/* TLC's -checkpoint / -recover (reference .gitignore:2, the states/ dir):
 * write the search (fingerprint set, parent records, current frontier,
 * counters) between levels to <prefix>.shard<id>.rtla, one file per shard
 * held by this context; recover it into a context opened with the same
 * configuration, then continue with rtla_step.  Collective when world > 1.
 * A search seeded with rtla_init_rows cannot be checkpointed: RTLA_E_STATE. */
int rtla_checkpoint(rtla_ctx *ctx, const char *prefix);
int rtla_recover(rtla_ctx *ctx, const char *prefix);
/* Counterexample, Init first.  rows: n * rtla_row_words() u32; labels: action
 * instance per state (-1 for Init).  *n_rows is set even if cap is too small. */
int rtla_trace(rtla_ctx *ctx, uint32_t *rows, int32_t *labels, size_t cap, size_t *n_rows);
/* Copy the current frontier (the states of the level last produced) to the
 * host: *n = #states; rows needs n * rtla_row_words() u32. */
int rtla_frontier(rtla_ctx *ctx, uint32_t *rows, size_t cap, size_t *n);
/* Rows index[0..n) of that frontier (numbered as rtla_frontier lists them;
 * this rank's shards only) -- samples of a level too large to copy whole, for
 * the parity tests' deep-level checks (TLC counterpart: reading states back
 * from its StateQueue). */
int rtla_frontier_rows(rtla_ctx *ctx, const uint64_t *index, size_t n, uint32_t *rows);
/* gen/distinct per coverage code (10 families, Receive split in 6). */
int rtla_coverage(rtla_ctx *ctx, uint64_t *gen, uint64_t *distinct, int n);
int rtla_device_info(rtla_ctx *ctx, char *buf, size_t cap);

/* Stateless helpers (need a GPU only for rtla_expand_batch). */
int rtla_row_words(const rtla_cfg *cfg);
/* Geometry of the packed row (u32 words; raft-tla_amd/csrc/rtla_model.h):
 * out[0..10) = W, off_hdr, off_srv, srv_words, off_all, all_words, off_elec,
 * elec_words, off_bag, slot_words.  Returns the number of values written. */
int rtla_row_layout(const rtla_cfg *cfg, int32_t *out, int n);
int rtla_init_row(const rtla_cfg *cfg, uint32_t *row);
/* Every enabled successor of each input row.  succ: cap rows; info[k] =
 * input index << 32 | in_model << 31 | receive-sub << 16 | instance. */
int rtla_expand_batch(const rtla_cfg *cfg, const uint32_t *rows, size_t n, uint32_t *succ,
                      uint64_t *info, size_t cap, size_t *n_out);
int rtla_state_text(const rtla_cfg *cfg, const uint32_t *row, char *buf, size_t cap);
/* Level digests for parity: *out = sum (mod 2^64) over the rows of FNV-1a-64 of
 * rtla_state_text -- an order-free digest of a SET of states, the quantity the
 * CPU oracle records per BFS level (oracle/raft_cpu.c level_text_hash; TLC has
 * no counterpart: it is how TLC's per-level state sets are compared here).
 * threads: host threads (0 = the process's CPU allowance, at most 16).
 * rtla_level_text_hash digests the current frontier (the level last produced)
 * of the whole job: device rows are streamed to the host in chunks, every
 * local shard is included, and with world > 1 it is collective (summed over
 * ranks). */
int rtla_rows_text_hash(const rtla_cfg *cfg, const uint32_t *rows, size_t n, int threads, uint64_t *out);
int rtla_level_text_hash(rtla_ctx *ctx, int threads, uint64_t *out);
/* SYMMETRY level digests: the same sums over each state's ORBIT TEXT -- the
 * text of the server-permuted image whose rotated text (the ten per-server
 * "/\ var" lines first, then messages, elections, allLogs) is least over all
 * N! images: a function of the orbit alone, so the orbit-count BFS's levels
 * are compared by content with the CPU oracle's (raft_cpu.c orbit_text),
 * whichever member of an orbit either side keeps.  Computed from the text
 * alone, never from the kernels' orbit key.  rtla_orbit_text: one row's. */
int rtla_rows_orbit_hash(const rtla_cfg *cfg, const uint32_t *rows, size_t n, int threads, uint64_t *out);
int rtla_level_orbit_hash(rtla_ctx *ctx, int threads, uint64_t *out);
int rtla_orbit_text(const rtla_cfg *cfg, const uint32_t *row, char *buf, size_t cap);
int rtla_action_name(const rtla_cfg *cfg, int32_t inst, int32_t sub, char *buf, size_t cap);
int rtla_invariants(const rtla_cfg *cfg, const uint32_t *row);  /* violated mask */
/* Fingerprint of a row recomputed from scratch (the kernels derive it
 * incrementally and store it in the row's first 4 words). */
int rtla_row_fingerprint(const rtla_cfg *cfg, const uint32_t *row, uint64_t out[2]);
/* SYMMETRY Permutations(Server): the seen-set key of a row's orbit (equal
 * for all server permutations of the row; rtla_model.h sym_key) and *perms =
 * the number of permutation images it compared.  rtla_permute_row: the image
 * pi(row), server i moved to pi[i] (pi: a permutation of 0..N-1), with its own
 * fingerprint.  TLC's counterpart: TLCState.permute / fingerPrint under
 * SYMMETRY (tlc2/tool/TLCStateMut.java). */
int rtla_orbit_key(const rtla_cfg *cfg, const uint32_t *row, uint64_t out[2], int *perms);
int rtla_permute_row(const rtla_cfg *cfg, const uint32_t *row, const int *pi, uint32_t *out);
const char *rtla_strerror(int status);
int rtla_abi_version(void);

/* Random-walk simulation (TLC -simulate / -depth / -seed).  Walk w -- a global
 * 64-bit id: disjoint [first_walk, first_walk + n_walks) ranges of separate
 * calls or processes compose -- starts at row w mod n of the current frontier
 * (n states, numbered as rtla_frontier lists them) and takes up to `depth`
 * steps (<= 65535).  At each step every action instance is evaluated in
 * ascending instance number; every enabled successor counts as generated and
 * is invariant-checked; if one violates, the walk ends with the violation
 * (step, least violating instance); otherwise the walk moves to a uniformly
 * drawn in-model successor (the draw depends on seed, w and the step only) or
 * ends "stuck" when there is none.  Normative definition, shared by device and
 * host: raft-tla_amd/csrc/rtla_sim.h.
 * ends (may be NULL; 4 * n_walks u64): per walk the last state's fingerprint
 * (2 words), a path digest over the states entered, steps taken | stop << 32
 * (RTLA_SIM_STOP_*).  Walks run in batches of 2^18; no batch is started after
 * one that found a violation (out->walks = walks run), and the violation
 * reported is the least (walk, step, instance) -- independent of scheduling. */
#define RTLA_SIM_STOP_DEPTH 0
#define RTLA_SIM_STOP_STUCK 1
#define RTLA_SIM_STOP_VIOLATION 2
typedef struct {
    uint64_t walks;        /* walks run */
    uint64_t steps;        /* steps taken (states entered) */
    uint64_t generated;    /* enabled successors evaluated (incl. out-of-model) */
    uint64_t stuck;        /* walks that ended with no in-model successor */
    double kernel_ms;      /* device time of the walks (rtla_sim_replay: host wall time) */
    uint64_t viol_walk;    /* the violation, if status == RTLA_VIOLATION: walk id (else ~0), ... */
    int32_t viol_step;     /* ... step (1-based) whose successor violates, ... */
    int32_t viol_inst;     /* ... its action instance (-1: none), ... */
    int32_t viol_mask;     /* ... the violated RTLA_INV_* and ... */
    int32_t viol_in_model; /* ... whether that successor satisfies the StateConstraint */
    int32_t status;        /* the call's return value */
    int32_t flags;         /* on RTLA_E_SPEC / RTLA_E_OVERFLOW: RTLA_CAP_SPEC_ERROR / RTLA_CAP_ROW */
    uint64_t taken[16];    /* steps taken per coverage code (rtla_coverage's numbering) */
} rtla_sim_stats;
/* On the GPU, from the context's current frontier.  Valid after rtla_init,
 * rtla_step or rtla_recover on a single-shard context with world == 1 in
 * RTLA_MODE_BFS whose frontier is not empty; anything else: RTLA_E_STATE.
 * Touches neither the fingerprint set, the arena nor the BFS counters:
 * rtla_step afterwards continues as if it had not run.  Returns RTLA_OK or
 * RTLA_VIOLATION; after RTLA_VIOLATION, rtla_violation and rtla_trace report
 * the simulated counterexample (the BFS parent chain from Init to the start
 * row, the walk's states -- replayed on the host --, the violating successor)
 * until the next rtla_simulate, rtla_step or rtla_reset. */
int rtla_simulate(rtla_ctx *ctx, uint64_t seed, uint64_t first_walk, uint64_t n_walks, int32_t depth,
                  uint64_t *ends, rtla_sim_stats *out);
/* The same walks on the host from explicit start rows (n_start rows): no
 * context, no GPU.  threads: 0 = the process's CPU allowance; at most 16. */
int rtla_sim_replay(const rtla_cfg *cfg, const uint32_t *start_rows, size_t n_start, uint64_t seed,
                    uint64_t first_walk, uint64_t n_walks, int32_t depth, int threads, uint64_t *ends,
                    rtla_sim_stats *out);
/* One walk from start_row on the host: the states it enters (not the start
 * row) and, last, its violating successor if it ends in one (then returns
 * RTLA_VIOLATION); labels = sub << 16 | instance, as rtla_trace.  *n_rows is
 * set even if cap is too small (RTLA_E_ARG). */
int rtla_sim_walk(const rtla_cfg *cfg, const uint32_t *start_row, uint64_t seed, uint64_t walk, int32_t depth,
                  uint32_t *rows, int32_t *labels, size_t cap, size_t *n_rows);

/* The same walks carrying user properties (normative
 * text: raft-tla_amd/csrc/rtla_sim.h): a compiled state set `states`
 * (rtla_pred_compile) and / or a compiled action set `steps`
 * (rtla_pred_compile_step).  Either may be NULL; both NULL, a set of the wrong
 * kind or one compiled for another row layout: RTLA_E_ARG.  At every step the
 * action set is evaluated on (state, successor) for every enabled successor,
 * as rtla_pred_step_* does (a stuttering step satisfies every definition), the
 * state set on every in-model successor; the walk ends at the least instance
 * whose built-in mask, state mask or step mask is nonzero.  A set never changes
 * which walk is taken.  An evaluation error of either program fails the call
 * (RTLA_E_SPEC).  The start row itself is not evaluated.
 * ends5 (may be NULL; 5 * n_walks u64): words 0-3 as rtla_simulate's; word 4 is
 * 0 unless the walk stopped on a violation, then instance | in_model << 16 |
 * built-in mask << 24 | state mask << 32 | step mask << 40.
 * out->viol_mask keeps meaning the built-in bits; pout names the rest.  After
 * RTLA_VIOLATION from rtla_simulate_pred, rtla_trace replays the walk with the
 * sets (they need not outlive the call) and rtla_violation returns the built-in
 * mask if nonzero, else the state mask, else the step mask. */
typedef struct {
    uint64_t state_evaluated; /* evaluations of the state set (in-model successors) */
    uint64_t step_evaluated;  /* evaluations of the action set (== generated when given) */
    int32_t viol_inv_mask;    /* the reported successor's violated RTLA_INV_*, ... */
    int32_t viol_state_mask;  /* ... its false state definitions (bit k = definition k) and ... */
    int32_t viol_step_mask;   /* ... its false action definitions */
    int32_t reserved;
} rtla_sim_pred_stats;
struct rtla_pred; /* a compiled set: rtla_pred_compile / rtla_pred_compile_step, below */
int rtla_simulate_pred(rtla_ctx *ctx, uint64_t seed, uint64_t first_walk, uint64_t n_walks, int32_t depth,
                       const struct rtla_pred *states, const struct rtla_pred *steps, uint64_t *ends5,
                       rtla_sim_stats *out, rtla_sim_pred_stats *pout);
int rtla_sim_replay_pred(const rtla_cfg *cfg, const uint32_t *start_rows, size_t n_start, uint64_t seed,
                         uint64_t first_walk, uint64_t n_walks, int32_t depth, int threads,
                         const struct rtla_pred *states, const struct rtla_pred *steps, uint64_t *ends5,
                         rtla_sim_stats *out, rtla_sim_pred_stats *pout);
int rtla_sim_walk_pred(const rtla_cfg *cfg, const uint32_t *start_row, uint64_t seed, uint64_t walk, int32_t depth,
                       const struct rtla_pred *states, const struct rtla_pred *steps, uint32_t *rows,
                       int32_t *labels, size_t cap, size_t *n_rows);

/* Audit: invariants evaluated outside the search.  inv_mask (RTLA_INV_*) is the
 * set to evaluate, independent of cfg->inv_mask and of a context's own set.
 * succ == 0: masks[k] = the invariants of inv_mask that rows[k] violates;
 * succ == 1: masks[k] = the OR over every enabled successor of rows[k], in- and
 * out-of-model, each evaluated as parent + delta as the level kernels do,
 * without materialising it.  counts (may be NULL; 8 u64): per invariant bit
 * (counts[b] for 1 << b), the evaluated states -- rows, or successors -- that
 * violate it.  A spec / row-capacity error of a successor fails the call
 * (RTLA_E_SPEC / RTLA_E_OVERFLOW).  rtla_check_batch runs on the GPU and is
 * stateless like rtla_expand_batch (test-sized inputs); rtla_check_replay
 * computes the same on the host, no GPU (threads: 0 = the process's CPU
 * allowance; at most 16). */
int rtla_check_batch(const rtla_cfg *cfg, const uint32_t *rows, size_t n, int32_t inv_mask, int32_t succ,
                     int32_t *masks, uint64_t *counts);
int rtla_check_replay(const rtla_cfg *cfg, const uint32_t *rows, size_t n, int32_t inv_mask, int32_t succ,
                      int threads, int32_t *masks, uint64_t *counts);
typedef struct {
    uint64_t audited;      /* states audited: the rows of the frontier */
    uint64_t evaluated;    /* states evaluated: the same (succ == 0), or their enabled successors */
    uint64_t counts[8];    /* per invariant bit: evaluated states that violate it */
    double kernel_ms;      /* device time of the audit (HIP events on the context's stream) */
    uint64_t row_bytes;    /* bytes of one packed state row */
    uint64_t viol_index;   /* the violation reported, if status == RTLA_VIOLATION: the least frontier index (as
                              rtla_frontier numbers rows; else ~0) with a violation, ... */
    int32_t viol_inst;     /* ... succ == 1: the least violating action instance of that row (else -1), ... */
    int32_t viol_mask;     /* ... the RTLA_INV_* that state violates and ... */
    int32_t viol_in_model; /* ... whether it satisfies the StateConstraint */
    int32_t status;        /* the call's return value */
    int32_t flags;         /* on RTLA_E_SPEC / RTLA_E_OVERFLOW: RTLA_CAP_SPEC_ERROR / RTLA_CAP_ROW */
    int32_t reserved;
} rtla_audit_stats;
/* The same over the context's current frontier, in place on the GPU.  Valid
 * where rtla_simulate is (single shard, world == 1, RTLA_MODE_BFS, a non-empty
 * frontier, no BFS violation pending); anything else: RTLA_E_STATE.  Touches
 * neither the fingerprint set, the arena nor the BFS counters.  Returns
 * RTLA_OK or RTLA_VIOLATION; the violation reported does not depend on
 * scheduling.  After RTLA_VIOLATION, rtla_violation and rtla_trace report the
 * counterexample (the BFS parent chain from Init to the row and, succ == 1,
 * the violating successor after it) until the next rtla_check_frontier,
 * rtla_simulate, rtla_step or rtla_reset. */
int rtla_check_frontier(rtla_ctx *ctx, int32_t inv_mask, int32_t succ, rtla_audit_stats *out);

/* User-defined state predicates (TLC: an operator added to MC.tla and named
 * under INVARIANT).  `text` holds up to 8 definitions `Name == expr` in the
 * predicate language, a TLA+ subset over the spec's variables (grammar,
 * bytecode and the termination bound: DESIGN.md section 13; the built-ins
 * restated in it: specs/MCPredicates.tla); definition k is bit k of every mask
 * and counts[k] below -- definition bits, not RTLA_INV_*.  A mask holds the
 * definitions that are FALSE on a state.
 * rtla_pred_compile: RTLA_E_CONFIG for a cfg outside the row format;
 * RTLA_E_ARG with "line:col: message" in err for a syntax, type or bound error
 * (more than 8 definitions, 6 bound variables, 512 program words, operand depth
 * 16 or 2^20 worst-case steps per row).  A compiled set is bound to the row
 * layout of its cfg: used with another, RTLA_E_ARG.
 * An evaluation error (log[i][n] with n outside 1..Len(log[i]), a per-type
 * message field read on a message of another type, a function applied to Nil)
 * fails the call: RTLA_E_SPEC (RTLA_CAP_SPEC_ERROR), on host and device alike.
 * rtla_pred_replay evaluates on the host (threads as rtla_check_replay),
 * rtla_pred_batch on the GPU, stateless (test-sized inputs); counts may be NULL
 * (8 u64).  rtla_pred_frontier evaluates over the context's current frontier in
 * place, with rtla_check_frontier's preconditions, touching nothing of the
 * search (states only: no successor mode); out->viol_mask and out->counts index
 * definitions.  After RTLA_VIOLATION, rtla_violation (inv_mask = definition
 * bits, in_model = 1) and rtla_trace report the BFS parent chain from Init to
 * the least false row until the next rtla_pred_frontier, rtla_check_frontier,
 * rtla_simulate, rtla_step or rtla_reset. */
typedef struct rtla_pred rtla_pred;
int rtla_pred_compile(const rtla_cfg *cfg, const char *text, rtla_pred **out, char *err, size_t errcap);
void rtla_pred_free(rtla_pred *p);
int rtla_pred_count(const rtla_pred *p);
int rtla_pred_name(const rtla_pred *p, int k, char *buf, size_t cap);
int rtla_pred_replay(const rtla_cfg *cfg, const rtla_pred *p, const uint32_t *rows, size_t n, int threads,
                     int32_t *masks, uint64_t *counts);
int rtla_pred_batch(const rtla_cfg *cfg, const rtla_pred *p, const uint32_t *rows, size_t n, int32_t *masks,
                    uint64_t *counts);
int rtla_pred_frontier(rtla_ctx *ctx, const rtla_pred *p, rtla_audit_stats *out);

/* Action properties (TLC: `Name == [][expr]_vars` named under PROPERTY).  An
 * action definition is a predicate over a step: inside the brackets the spec's
 * variables may carry a prime and then read the successor (grammar, typing of
 * the two rows and the semantics: DESIGN.md section 14; examples:
 * specs/MCActions.tla).  rtla_pred_compile_step compiles the action definitions
 * of `text` (at most 8) into a set of the step kind; the state definitions of
 * the same text are parsed and type-checked but skipped.  Errors as
 * rtla_pred_compile's, and RTLA_E_ARG if the text holds no action definition.
 * rtla_pred_is_step: 1 for such a set, 0 for rtla_pred_compile's.  A set knows
 * its kind: a state set given to a step call is RTLA_E_ARG, and so is a step
 * set given to rtla_pred_replay / _batch / _frontier.
 * What is evaluated: for each row s, every action instance in ascending
 * instance number (as rtla_check_replay with succ = 1); each enabled successor
 * t, in-model or not, is one evaluated step.  Definition k is false on the step
 * iff its expression is FALSE on (s, t) and t is not s (their 128-bit
 * fingerprints differ: a stuttering step satisfies every [A]_vars).  masks[k]
 * is the OR over the steps out of row k, counts[d] the steps on which
 * definition d is false, *evaluated (may be NULL) the steps.  A successor's
 * spec or row-capacity error and a program's evaluation error on any step
 * (a stuttering one included) fail the call, on host and device alike.
 * rtla_pred_step_replay: on the host; rtla_pred_step_batch: on the GPU,
 * stateless; rtla_pred_step_frontier: over the steps out of the current
 * frontier, in place, with rtla_check_frontier's preconditions, touching
 * nothing of the search; out->audited is the rows, out->evaluated the steps,
 * viol_index / viol_inst / viol_in_model the least (row, instance) with a false
 * definition as for succ = 1, viol_mask its definition bits.  After
 * RTLA_VIOLATION rtla_trace gives the BFS parent chain from Init to s, then t. */
int rtla_pred_compile_step(const rtla_cfg *cfg, const char *text, rtla_pred **out, char *err, size_t errcap);
int rtla_pred_is_step(const rtla_pred *p);
int rtla_pred_step_replay(const rtla_cfg *cfg, const rtla_pred *p, const uint32_t *rows, size_t n, int threads,
                          int32_t *masks, uint64_t *counts, uint64_t *evaluated);
int rtla_pred_step_batch(const rtla_cfg *cfg, const rtla_pred *p, const uint32_t *rows, size_t n, int32_t *masks,
                         uint64_t *counts, uint64_t *evaluated);
int rtla_pred_step_frontier(rtla_ctx *ctx, const rtla_pred *p, rtla_audit_stats *out);

/* User-defined CONSTRAINTs (TLC: an operator added to MC.tla and named under
 * CONSTRAINT; DESIGN.md section 16, examples: specs/MCConstraints.tla).
 * rtla_pred_constrain evaluates the state set `p` on every row of the level
 * last produced and keeps row g iff every definition is TRUE on it.  Kept rows
 * keep their order and become rows 0 .. kept-1 of the same level, in place in
 * the arena, their parent records with them; the frontier shrinks to `kept`
 * and distinct_total by `dropped`, so every later count, digest, trace, audit,
 * simulation, checkpoint and rtla_step sees the kept rows only.  Call it after
 * rtla_init / rtla_init_rows / rtla_step (and after auditing user invariants
 * on the unfiltered level, as TLC checks them on states it then discards) and
 * before anything reads the level as a frontier.  Returns RTLA_OK, or RTLA_DONE
 * when no row is kept (the search is finished).
 * Not corrected: the fingerprint set keeps the dropped states' keys (a dropped
 * state met again is "seen"; its load is the pre-drop one), and
 * rtla_coverage's per-action distinct counts still include dropped states.
 * Preconditions: rtla_check_frontier's (else RTLA_E_STATE).  A step set or a
 * set compiled for another layout: RTLA_E_ARG.  An evaluation error on any row:
 * RTLA_E_SPEC, with the frontier, parent records and totals exactly as before
 * the call.  A HIP failure while rows move ends the search.  Under SYMMETRY the
 * constraint must be symmetric under server permutation, as TLC requires.
 * The compaction runs in chunks of RTLA_CONSTRAIN_CHUNK rows (environment;
 * rounded up to 64; default 2^20) through a staging buffer of that many rows,
 * allocated at first use and freed by rtla_close. */
typedef struct {
    int32_t level;           /* the level pruned (rtla_level_stats.level of the call that produced it) */
    int32_t status;          /* the call's return value */
    uint64_t examined;       /* rows of the level before the call */
    uint64_t kept;           /* rows on which every definition is TRUE: the frontier now */
    uint64_t dropped;        /* examined - kept */
    uint64_t counts[8];      /* per definition: rows on which it is FALSE */
    uint64_t start;          /* arena row of the level's first state (the level wraps if start + examined exceeds
                                the arena's rows) */
    double eval_ms;          /* device time of the evaluation and the keep bitmap */
    double move_ms;          /* device time of the compaction (0 when nothing was dropped: nothing is written) */
    uint64_t distinct_total; /* after the drop */
    int32_t flags;           /* on RTLA_E_SPEC: RTLA_CAP_SPEC_ERROR */
    int32_t reserved;
} rtla_constrain_stats;
int rtla_pred_constrain(rtla_ctx *ctx, const rtla_pred *p, rtla_constrain_stats *out);
/* The same pass, stateless (test-sized inputs): the n rows are laid into a
 * device ring of ring_cap rows from row ring_start on, wrapping at its end if
 * they must (ring_cap and ring_start multiples of 64, ring_start < ring_cap,
 * ring_cap >= n rounded up to 64), `parents` (n u64, in/out) stands for the
 * parent records, and the same kernels run with chunks of `chunk` rows
 * (rounded up to 64; 0: the default).  out_rows (room for n rows) gets the kept
 * rows in order, parents[0 .. *kept) their entries, counts (may be NULL; 8 u64)
 * the rows on which each definition is false.  On any error no output is
 * written. */
int rtla_constrain_batch(const rtla_cfg *cfg, const rtla_pred *p, const uint32_t *rows, size_t n, uint64_t ring_cap,
                         uint64_t ring_start, uint64_t chunk, uint32_t *out_rows, uint64_t *parents, size_t *kept,
                         uint64_t *counts);

/* Diagnostic (performance analysis only): re-expand the current frontier
 * `reps` times with the level kernel's experiment switches `xflags` (XF_*
 * in raft-tla_amd/csrc/rtla_device.h: e.g. 1 = no fingerprint-set probe,
 * 2 = no coverage counters, 8 = no successor rows); *ms = mean device time
 * per launch.  Pollutes the search state: use only after the last rtla_step. */
int rtla_time_expand(rtla_ctx *ctx, int xflags, int reps, double *ms);

/* Synthetic microbench (BASELINE.json configs[4]): valid random packed
 * states (counter-based PRNG: state number -> state id, half of them redrawn
 * from [0, pool) so dedup has hits; raft-tla_amd/csrc/rtla_synth.h).
 * rtla_random_rows: rows of input states first .. first + n - 1 (host).
 * rtla_synthetic_step: the same states generated on the device, then one
 * level-kernel launch over them -- Next, fingerprint, probe/insert into the
 * context's fingerprint set, no successor rows kept; out->generated /
 * ->probes / ->new_states / ->kernel_ms describe that launch.  Single shard,
 * before rtla_init (or after rtla_reset).
 * rtla_synthetic_step = rtla_synthetic_generate (input states first ..
 * first + n - 1 into rows [0, n) of the context's row arena, on the device)
 * followed by rtla_synthetic_dedup over rows [0, n): the benchmark generates
 * its inputs once and times only the dedup passes over HBM-resident rows
 * (rtla_reset clears the set, not the arena). */
int rtla_random_rows(const rtla_cfg *cfg, uint64_t seed, uint64_t first, uint64_t n, uint64_t pool, uint32_t *rows);
/* The same input states as state texts ('\x1e'-terminated, *len bytes in
 * all; RTLA_E_ARG when cap is too small): the CPU baseline's input. */
int rtla_random_texts(const rtla_cfg *cfg, uint64_t seed, uint64_t first, uint64_t n, uint64_t pool, char *buf,
                      size_t cap, size_t *len);
int rtla_synthetic_step(rtla_ctx *ctx, uint64_t seed, uint64_t first, uint64_t n, uint64_t pool,
                        rtla_level_stats *out);
int rtla_synthetic_generate(rtla_ctx *ctx, uint64_t seed, uint64_t first, uint64_t n, uint64_t pool, uint64_t at);
int rtla_synthetic_dedup(rtla_ctx *ctx, uint64_t begin, uint64_t end, rtla_level_stats *out);

/* Calibration: n random 8-byte CAS inserts into a table of 2^log2 slots;
 * returns device seconds.  A key that hits the probe limit is not inserted:
 * RTLA_E_OVERFLOW (rtla_probe_bench2 alike), *inserted still set. */
int rtla_probe_bench(int log2, uint64_t n, double *seconds, uint64_t *inserted);
/* n random keys inserted (CAS, all new), then re-probed (all present) with a
 * CAS and with the kernel's load-first protocol; device seconds of each pass. */
int rtla_probe_bench2(int log2, uint64_t n, double *s_insert, double *s_seen_cas, double *s_seen_load,
                      uint64_t *inserted);
/* Mixed-stream calibration of the random-access ceiling: a 2^log2-slot table
 * holding n_present random keys, then n timed probes of which a fraction
 * new_frac are keys not in the table (inserted: load, CAS on an empty slot)
 * and the rest keys it holds (one load) -- the level kernel's load-first
 * protocol at a workload's own insert fraction D/P.  *seconds = the probe
 * pass (HIP events); *inserted = keys it inserted. */
int rtla_probe_bench3(int log2, uint64_t n_present, uint64_t n, double new_frac, double *seconds,
                      uint64_t *inserted);
/* The kernels' fingerprint-set insert on caller-chosen fingerprints (no
 * context; the tests' seam to the set).  fps: n (a, b) pairs; the key stored
 * is b | 1, its home slot the top log2 bits of a (log2 in 10..30, else
 * RTLA_E_ARG).  Input i is inserted by global thread i of 256-thread blocks
 * (n <= 2^31), so the caller's order decides which inputs share a wavefront
 * or a block.  protocol: 0 = one CAS per slot (Init, the wave-per-state
 * kernel); 1 = CAS at the home slot, then CAS probing (the level kernel's
 * pipelined probe); 2 = load the home slot, CAS only an empty slot (the level
 * kernel's default probe); 3 = k_insert_remote itself, the exchange's owner
 * side, on the inputs as one sender's region (its own thread mapping, several
 * records per thread; a fingerprint 0:0 is a hole and never new).  table: 2^log2 u64,
 * in/out -- uploaded before the launch, downloaded after it (all zero = an
 * empty set), so a second call continues on the first call's table.
 * is_new[i] = 1 if input i was inserted, 0 if it was found -- or dropped at
 * the probe limit: then *flags has RTLA_CAP_FPSET and the call returns
 * RTLA_E_OVERFLOW, every output filled all the same. */
int rtla_fpset_probe(int log2, const uint64_t *fps, size_t n, int protocol, uint64_t *table, uint8_t *is_new,
                     int32_t *flags);

#ifdef __cplusplus
}
#endif
#endif
