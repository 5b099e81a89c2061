#!/usr/bin/env python3
"""Cost of a user-defined CONSTRAINT on the GPU (Checker.constrain,
rtla_kconstrain.hip), on the BASELINE configs[1] shape:
BFS through --levels levels (a deep level that still leaves arena room), then
one constrain() of that level with

* (a) a constraint that keeps every row (nothing moves),
* (b) the term constraint (currentTerm[i] <= 2 under MaxTerm = 3),
* (c) a constraint that drops about half (BagCardinality(messages) <= k, k
      chosen on the host from a sample of the level).

constrain() changes the level, so every repetition resets the search and
produces the level anew.  Per constraint, the median of --reps repetitions
after a warm-up of

* eval_ms beside audit_predicates of the same set on the same level in the same
  process (they run the same interpreter kernel; the pass also stores a mask per
  row and packs the keep bitmap),
* move_ms and the bytes the compaction reads and writes over it: every row read
  once, every kept row written to staging, read back and written to its place,
  and the parent records likewise,
* a device-to-device copy that moves as many bytes (half read, half written),
  timed with events in the same process: the yardstick for the move.

    python tools/constrain_bench.py [--levels 16] [--out profiles/<dir>/constrain.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raft-tla_amd"))

SHAPE = (3, 2, 3, 2, 1, 0)   # BASELINE.json configs[1] (bench.py cfg2), bag_cap 18
ES_LM = ("ElectionSafety", "LogMatching")


def median(xs):
    return sorted(xs)[len(xs) // 2]


def copy_yardstick(nbytes, reps):
    """Median ms of a device-to-device copy of nbytes (torch: hipMemcpyAsync on its stream, timed by events)."""
    import torch
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    src.zero_()
    ms = []
    for k in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src, non_blocking=True)
        e1.record()
        e1.synchronize()
        if k:
            ms.append(e0.elapsed_time(e1))
    del src, dst
    torch.cuda.empty_cache()
    return median(ms), [round(m, 3) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fpset-log2", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_constrain", "constrain.json"))
    args = ap.parse_args()
    import rtla

    cfg = rtla.Config(*SHAPE, ES_LM, bag_cap=18, fpset_log2=args.fpset_log2)
    chunk = os.environ.get("RTLA_CONSTRAIN_CHUNK", "")
    out = {"shape": dict(zip(("n_server", "n_value", "max_term", "max_log", "max_copies", "max_msgs"), SHAPE)),
           "bag_cap": 18, "chunk_rows": int(chunk) if chunk else 1 << 20,
           "command": "python tools/constrain_bench.py " + " ".join(sys.argv[1:])}
    with rtla.Checker(cfg) as ck:
        def produce():
            if ck.levels:
                ck.reset()
            ck.init()
            while len(ck.levels) < args.levels:
                assert ck.step() == rtla.OK

        produce()
        last = ck.levels[-1]
        n, rb = last.new, last.row_bytes
        out["bfs"] = {"levels": len(ck.levels), "distinct": ck.distinct, "last_level_states": n,
                      "last_level_kernel_ms": round(last.kernel_ms, 3), "row_bytes": rb}
        print(json.dumps(out["bfs"]), flush=True)
        # k for (c): the median message count of a spread sample of the level
        sample = ck.frontier_rows([i * (n // 4096) for i in range(4096)] if n >= 4096 else list(range(n)))
        lo, hi = 0, 64
        while lo < hi:
            mid = (lo + hi) // 2
            with rtla.Predicates(cfg, "H == BagCardinality(messages) <= %d" % mid) as p:
                keeps = rtla.pred_replay(p, sample)[0].count(0) * 2 >= len(sample)
            lo, hi = (lo, mid) if keeps else (mid + 1, hi)
        texts = (("keeps_all", r"All == \A i \in Server : currentTerm[i] <= 3"),
                 ("terms_up_to_2", r"TermsUpTo2 == \A i \in Server : currentTerm[i] <= 2"),
                 ("about_half", "Half == BagCardinality(messages) <= %d" % lo))
        rows = []
        for name, text in texts:
            with rtla.Predicates(cfg, text) as con:
                audits, runs = [], []
                for k in range(args.reps + 1):  # (the first is the warm-up)
                    if k or name != texts[0][0]:
                        produce()
                    a = ck.audit_predicates(con)
                    a = ck.audit_predicates(con)  # (the second launch: the level is as warm as the pass finds it)
                    r = ck.constrain(con)
                    assert r.examined == n and r.dropped == sum(a.counts.values()) and ck.frontier_size() == r.kept
                    if k:
                        audits.append(a.kernel_ms)
                        runs.append(r)
                r = runs[0]
                moved = (r.examined + 3 * r.kept) * (rb + 8) if r.dropped else 0
                move_ms = median([x.move_ms for x in runs])
                eval_ms = median([x.eval_ms for x in runs])
                row = {"what": name, "constraint": text, "examined": r.examined, "kept": r.kept, "dropped": r.dropped,
                       "eval_ms": round(eval_ms, 3), "eval_ms_all": [round(x.eval_ms, 3) for x in runs],
                       "audit_predicates_ms": round(median(audits), 3), "audit_predicates_ms_all":
                       [round(x, 3) for x in audits], "eval_over_audit": eval_ms / median(audits),
                       "move_ms": round(move_ms, 3), "move_ms_all": [round(x.move_ms, 3) for x in runs],
                       "move_bytes": moved, "move_gb_per_s": moved / (move_ms / 1e3) / 1e9 if moved else None}
                rows.append(row)
                print(json.dumps(row), flush=True)
        ck.reset()
    for row in rows:  # the yardstick, once the checker's memory is free: a copy that moves as many bytes
        if row["move_bytes"]:
            try:
                ms, all_ms = copy_yardstick(row["move_bytes"] // 2, args.reps)
            except Exception as e:  # (no torch, or none that finds the device: the report says so)
                row["copy_ms"], row["copy_not_taken"] = None, "%s: %s" % (type(e).__name__, e)
                print(json.dumps({"what": row["what"], "copy_not_taken": row["copy_not_taken"]}), flush=True)
                continue
            row.update({"copy_ms": round(ms, 3), "copy_ms_all": all_ms,
                        "copy_gb_per_s": row["move_bytes"] / (ms / 1e3) / 1e9, "move_over_copy": row["move_ms"] / ms})
            print(json.dumps({k: row[k] for k in ("what", "move_ms", "copy_ms", "move_over_copy")}), flush=True)
    out["constraints"] = rows
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
