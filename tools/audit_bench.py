#!/usr/bin/env python3
"""Cost of the audit (Checker.audit, rtla_kaudit.hip) and of the two safety
invariants in the search, on the BASELINE configs[1] shape over the levels
bench.py times (17):

* the audit of the last level with StateMachineSafety + LeaderCompleteness, in
  both modes: device time (median of --reps), the bytes the state pass must
  read over that time beside the HBM peak bench.py's roofline uses, and
  rtla_check_replay on --threads host threads over a strided sample of the
  same rows (whose counts the device's must equal on the sample: the device is
  run on the sample as well, through rtla_check_batch);
* the same BFS with the two new bits in the context's own mask, which runs on
  the run-time-layout level kernel (no compiled-in layout carries the bits),
  against the run without them: the level kernels' summed device time.

    python tools/audit_bench.py [--levels 17] [--sample N] [--out profiles/<dir>/audit.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raft-tla_amd"))

SHAPE = (3, 2, 3, 2, 1, 0)   # BASELINE.json configs[1] (bench.py cfg2), bag_cap 18
ES_LM = ("ElectionSafety", "LogMatching")
NEW = ("StateMachineSafety", "LeaderCompleteness")
HBM_PEAK_GBS = 8000.0        # bench.py's roofline peak


def bfs(rtla, invariants, levels, fpset_log2):
    cfg = rtla.Config(*SHAPE, invariants, bag_cap=18, fpset_log2=fpset_log2)
    ck = rtla.Checker(cfg)
    t = time.time()
    ck.init()
    while len(ck.levels) < levels:
        assert ck.step() == rtla.OK
    return cfg, ck, {"invariants": list(invariants), "levels": len(ck.levels), "distinct": ck.distinct,
                     "generated": ck.generated, "kernel_ms": round(sum(lv.kernel_ms for lv in ck.levels), 3),
                     "last_level_kernel_ms": round(ck.levels[-1].kernel_ms, 3),
                     "wall_ms": round((time.time() - t) * 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", type=int, default=17)
    ap.add_argument("--sample", type=int, default=1 << 21)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fpset-log2", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_audit", "audit.json"))
    args = ap.parse_args()
    import rtla

    out = {"shape": dict(zip(("n_server", "n_value", "max_term", "max_log", "max_copies", "max_msgs"), SHAPE)),
           "bag_cap": 18, "host_threads": args.threads, "xflags": os.environ.get("RTLA_XFLAGS", "0"),
           "command": "python tools/audit_bench.py " + " ".join(sys.argv[1:])}
    for inv in (ES_LM, ES_LM + NEW):  # warm-up: both level kernels' code objects
        bfs(rtla, inv, min(6, args.levels), 24)[1].close()
    cfg, ck, out["bfs"] = bfs(rtla, ES_LM, args.levels, args.fpset_log2)
    print(json.dumps(out["bfs"]))
    w, n = rtla.row_words(cfg), ck.frontier_size()
    mask = rtla.inv_mask_of(NEW)
    audits = []
    for succ in (False, True):
        ck.audit(NEW, succ=succ)  # warm-up (code object, counters)
        runs = sorted((ck.audit(NEW, succ=succ) for _ in range(3 if succ else args.reps)), key=lambda r: r.kernel_ms)
        res = runs[len(runs) // 2]
        a = {"succ": int(succ), "bfs_level": len(ck.levels), "states": res.audited, "evaluated": res.evaluated,
             "status": res.status, "counts": res.counts, "kernel_ms": round(res.kernel_ms, 3),
             "kernel_ms_all": [round(r.kernel_ms, 3) for r in runs],
             "evaluated_per_s": res.evaluated / (res.kernel_ms / 1e3)}
        if not succ:
            a["row_bytes"] = res.row_bytes
            a["bytes_read"] = res.audited * res.row_bytes
            a["gb_per_s"] = a["bytes_read"] / (res.kernel_ms / 1e3) / 1e9
            a["fraction_of_hbm_peak"] = a["gb_per_s"] / HBM_PEAK_GBS
        audits.append(a)
        print(json.dumps(a))
    # the host on a strided sample of the same rows
    m = min(args.sample, n)
    idx = (C.c_uint64 * m)(*[k * n // m for k in range(m)])
    flat = (C.c_uint32 * (m * w))()
    rtla._check(rtla._lib.rtla_frontier_rows(ck._h, idx, m, flat), "rtla_frontier_rows")
    cc = cfg.c()
    for a in audits:
        masks, counts = (C.c_int32 * m)(), (C.c_uint64 * 8)()
        t = time.time()
        rtla._check(rtla._lib.rtla_check_replay(C.byref(cc), flat, m, mask, a["succ"], args.threads, masks, counts),
                    "rtla_check_replay")
        ms = (time.time() - t) * 1e3
        dmasks, dcounts = (C.c_int32 * m)(), (C.c_uint64 * 8)()
        rtla._check(rtla._lib.rtla_check_batch(C.byref(cc), flat, m, mask, a["succ"], dmasks, dcounts),
                    "rtla_check_batch")
        per_state_host = ms / m
        a["host_sample_states"] = m
        a["host_sample_ms"] = round(ms, 3)
        a["host_ms_whole_level_extrapolated"] = round(per_state_host * a["states"], 1)
        a["gpu_over_host"] = per_state_host * a["states"] / a["kernel_ms"]
        a["sample_equal_host"] = list(masks) == list(dmasks) and list(counts) == list(dcounts)
        print(json.dumps({k: a[k] for k in ("succ", "host_sample_states", "host_sample_ms", "gpu_over_host",
                                            "sample_equal_host")}))
    out["audit"] = audits
    ck.close()
    # the search with the two new bits in its own mask (run-time-layout level kernel)
    _, ck5, out["bfs_with_new_bits"] = bfs(rtla, ES_LM + NEW, args.levels, args.fpset_log2)
    assert ck5.status == rtla.OK and ck5.distinct == out["bfs"]["distinct"]
    ck5.close()
    out["bfs_with_new_bits"]["kernel_ms_over_without"] = out["bfs_with_new_bits"]["kernel_ms"] / out["bfs"]["kernel_ms"]
    print(json.dumps(out["bfs_with_new_bits"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0 if all(a["sample_equal_host"] for a in audits) else 1


if __name__ == "__main__":
    sys.exit(main())
