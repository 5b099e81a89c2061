#!/usr/bin/env python3
"""Cost of user-defined predicates on the GPU (Checker.audit_predicates,
rtla_kpred.hip) beside the built-in state audit (Checker.audit,
rtla_kaudit.hip), on the BASELINE configs[1] shape: BFS through the levels
bench.py times (17), then, over the last level's rows in place and in the same
process, the median device time of --reps launches of

* the built-in audit of all five invariants (the yardstick),
* PLogMatching alone,
* the five built-ins restated (specs/MCPredicates.tla) as one set,

with, for each, the ratio to the yardstick, the bytes of the level over that
time beside the HBM peak bench.py's roofline uses, and the time relative to the
level kernel's of the last level (what `check(..., predicates=...)` adds per
level).  The counts of the restated set must equal the built-in audit's.

    python tools/pred_bench.py [--levels 17] [--out profiles/<dir>/pred.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raft-tla_amd"))

SHAPE = (3, 2, 3, 2, 1, 0)   # BASELINE.json configs[1] (bench.py cfg2), bag_cap 18
ES_LM = ("ElectionSafety", "LogMatching")
HBM_PEAK_GBS = 8000.0        # bench.py's roofline peak


def median_run(fn, reps):
    fn()  # warm-up (code object, counters)
    runs = sorted((fn() for _ in range(reps)), key=lambda r: r.kernel_ms)
    return runs[len(runs) // 2], [round(r.kernel_ms, 3) for r in runs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", type=int, default=17)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fpset-log2", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_pred", "pred.json"))
    args = ap.parse_args()
    import rtla

    text = open(os.path.join(ROOT, "specs", "MCPredicates.tla")).read()
    blocks = [b for b in text.split("\n\n") if b.startswith("P")]
    restated = "\n\n".join(blocks)
    cfg = rtla.Config(*SHAPE, ES_LM, bag_cap=18, fpset_log2=args.fpset_log2)
    out = {"shape": dict(zip(("n_server", "n_value", "max_term", "max_log", "max_copies", "max_msgs"), SHAPE)),
           "bag_cap": 18, "command": "python tools/pred_bench.py " + " ".join(sys.argv[1:])}
    with rtla.Checker(cfg) as ck, rtla.Predicates(cfg, restated) as five, \
            rtla.Predicates(cfg, [b for b in blocks if b.startswith("PLogMatching")][0]) as one:
        assert five.names == ["P" + n for n in rtla.INV_BITS] and one.names == ["PLogMatching"]
        ck.init()
        while len(ck.levels) < args.levels:
            assert ck.step() == rtla.OK
        last = ck.levels[-1]
        out["bfs"] = {"levels": len(ck.levels), "distinct": ck.distinct, "last_level_states": last.new,
                      "last_level_kernel_ms": round(last.kernel_ms, 3), "row_bytes": last.row_bytes}
        print(json.dumps(out["bfs"]), flush=True)
        rows = []
        base = None
        for name, fn in (("builtin_audit_all_five", lambda: ck.audit(tuple(rtla.INV_BITS))),
                         ("PLogMatching", lambda: ck.audit_predicates(one)),
                         ("five_restated", lambda: ck.audit_predicates(five))):
            res, all_ms = median_run(fn, args.reps)
            base = base or res
            gbs = res.audited * res.row_bytes / (res.kernel_ms / 1e3) / 1e9
            r = {"what": name, "states": res.audited, "status": res.status, "counts": res.counts,
                 "kernel_ms": round(res.kernel_ms, 3), "kernel_ms_all": all_ms,
                 "over_builtin_audit": res.kernel_ms / base.kernel_ms, "gb_per_s": gbs,
                 "fraction_of_hbm_peak": gbs / HBM_PEAK_GBS,
                 "over_last_level_kernel": res.kernel_ms / last.kernel_ms}
            rows.append(r)
            print(json.dumps(r), flush=True)
        out["audits"] = rows
        equal = {"P" + n: c for n, c in rows[0]["counts"].items()} == rows[2]["counts"]
        out["restated_counts_equal_builtin"] = equal
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
