#!/usr/bin/env python3
"""Cost of action properties on the GPU (Checker.audit_steps: k_pred_step,
rtla_kpred.hip) beside the built-in successor audit (Checker.audit(succ=True):
k_audit_succ), on the BASELINE configs[1] shape: BFS through --levels levels,
then, over the steps out of the last level in place and in the same process,
the median device time of --reps launches of

* the built-in successor audit of all five invariants (the yardstick: the same
  enumeration, evaluated as parent + delta, nothing materialised),
* LeaderAppendOnly alone,
* the five laws of specs/MCActions.tla as one set,

with, for each, the steps evaluated, ns per step, the ratio to the yardstick and
the time relative to the level kernel's of the last level (what
`check(..., actions=...)` adds per level).

    python tools/step_bench.py [--levels 14] [--out profiles/<dir>/step.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raft-tla_amd"))

SHAPE = (3, 2, 3, 2, 1, 0)   # BASELINE.json configs[1] (bench.py cfg2), bag_cap 18
ES_LM = ("ElectionSafety", "LogMatching")
LAWS = ("LeaderAppendOnly", "TermsNeverDecrease", "OneVotePerTerm", "BagChangesByOne", "ElectionsGrow")


def median_run(fn, reps):
    fn()  # warm-up (code object, counters)
    runs = sorted((fn() for _ in range(reps)), key=lambda r: r.kernel_ms)
    return runs[len(runs) // 2], [round(r.kernel_ms, 3) for r in runs]


def definitions(text, names):
    blocks = [b for b in text.split("\n\n") if any(ln.startswith(n + " ==") for n in names for ln in b.split("\n"))]
    return "\n".join(ln for b in blocks for ln in b.split("\n") if not ln.startswith(("\\*", "====")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", type=int, default=14)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fpset-log2", type=int, default=28)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_step", "step.json"))
    args = ap.parse_args()
    import rtla

    text = open(os.path.join(ROOT, "specs", "MCActions.tla")).read()
    cfg = rtla.Config(*SHAPE, ES_LM, bag_cap=18, fpset_log2=args.fpset_log2)
    out = {"shape": dict(zip(("n_server", "n_value", "max_term", "max_log", "max_copies", "max_msgs"), SHAPE)),
           "bag_cap": 18, "command": "python tools/step_bench.py " + " ".join(sys.argv[1:])}
    with rtla.Checker(cfg) as ck, rtla.Actions(cfg, definitions(text, LAWS)) as five, \
            rtla.Actions(cfg, definitions(text, LAWS[:1])) as one:
        assert five.names == list(LAWS) and one.names == ["LeaderAppendOnly"]
        ck.init()
        while len(ck.levels) < args.levels:
            assert ck.step() == rtla.OK
        last = ck.levels[-1]
        out["bfs"] = {"levels": len(ck.levels), "distinct": ck.distinct, "last_level_states": last.new,
                      "last_level_kernel_ms": round(last.kernel_ms, 3), "row_bytes": last.row_bytes}
        print(json.dumps(out["bfs"]), flush=True)
        rows = []
        base = None
        for name, fn in (("builtin_successor_audit_all_five", lambda: ck.audit(tuple(rtla.INV_BITS), succ=True)),
                         ("LeaderAppendOnly", lambda: ck.audit_steps(one)),
                         ("five_laws", lambda: ck.audit_steps(five))):
            res, all_ms = median_run(fn, args.reps)
            base = base or res
            r = {"what": name, "states": res.audited, "steps": res.evaluated, "status": res.status,
                 "counts": res.counts, "kernel_ms": round(res.kernel_ms, 3), "kernel_ms_all": all_ms,
                 "ns_per_step": res.kernel_ms * 1e6 / max(1, res.evaluated),
                 "over_builtin_successor_audit": res.kernel_ms / base.kernel_ms,
                 "over_last_level_kernel": res.kernel_ms / last.kernel_ms}
            rows.append(r)
            print(json.dumps(r), flush=True)
        out["audits"] = rows
        ok = rows[0]["steps"] == rows[1]["steps"] == rows[2]["steps"] and not any(rows[2]["counts"].values())
        out["same_steps_and_laws_hold"] = ok
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
