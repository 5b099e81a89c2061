#!/usr/bin/env python3
"""Throughput of the random-walk simulation (Checker.simulate, k_simulate) on
the BASELINE configs[1] shape: BFS to a level whose frontier fits comfortably,
then walks from it -- steps/s and generated/s on the GPU, the same walks on the
host (rtla_sim_replay, 16 threads) as the CPU baseline, and the ratio to the
level kernel's generated/s measured in the same run.  Also checks that both
sides computed the same end records.

    python tools/sim_bench.py [--levels 1,12] [--walks N] [--depth D] [--out profiles/<dir>/sim.json]

Walks that carry user properties: each --predicates /
--actions FILE with its --names A,B adds a line per level after the plain one --
the same walks with those definitions, on the GPU (k_simulate<NS, true>) beside
the 16-thread rtla_sim_replay_pred, records compared.  The options repeat; the
k-th --names belongs to the k-th FILE in command-line order:

    python tools/sim_bench.py --levels 12 --actions specs/MCActions.tla --names LeaderAppendOnly \
        --actions specs/MCActions.tla --names LeaderAppendOnly,TermsNeverDecrease,OneVotePerTerm,BagChangesByOne,ElectionsGrow \
        --predicates specs/MCPredicates.tla --names PLogMatching --out profiles/r11_simpred/sim.json
"""
import argparse
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raft-tla_amd"))

SHAPE = (3, 2, 3, 2, 1, 0)   # BASELINE.json configs[1] (bench.py cfg2), bag_cap 18
LEVEL_KERNEL_REF = {"source": "profiles/r06_v4/bench.json", "generated": 5.275e9, "ms": 171.0}


def select(text, names):
    """The definitions `names` of a predicate file, in the order asked for (each runs to the next blank line)."""
    out = []
    for n in names:
        m = re.search(r"^%s ==.*?(?=\n\s*\n|\n=====|\Z)" % re.escape(n), text, re.M | re.S)
        if not m:
            raise SystemExit("no definition %s" % n)
        out.append(m.group(0))
    return "\n\n".join(out) + "\n"


class SetArg(argparse.Action):
    """--predicates / --actions FILE and --names A,B in command-line order: namespace.sets = [[kind, file, names]]."""

    def __call__(self, parser, ns, value, option=None):
        sets = getattr(ns, "sets", None) or []
        if option == "--names":
            if not sets or sets[-1][2]:
                parser.error("--names follows a --predicates or --actions FILE")
            sets[-1][2] = value.split(",")
        else:
            sets.append([option[2:], value, []])
        ns.sets = sets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--predicates", action=SetArg, metavar="FILE", help="a line with state definitions of FILE")
    ap.add_argument("--actions", action=SetArg, metavar="FILE", help="a line with action definitions of FILE")
    ap.add_argument("--names", action=SetArg, metavar="A,B", help="the definitions of the FILE before it")
    ap.add_argument("--levels", default="1,12", help="BFS levels to simulate from (1 = Init: TLC's plain -simulate)")
    ap.add_argument("--walks", type=int, default=1 << 21)
    ap.add_argument("--depth", type=int, default=32)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3, help="GPU repetitions (the median is reported)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_sim", "sim.json"))
    args = ap.parse_args()
    import rtla

    cfg = rtla.Config(*SHAPE, ("ElectionSafety", "LogMatching"), bag_cap=18, fpset_log2=28, mem_budget=16 << 30)
    levels = sorted(int(x) for x in args.levels.split(","))
    lines = [(None, {})]  # (label, simulate's keyword arguments): the plain walks, then one line per set
    for kind, path, names in getattr(args, "sets", None) or []:
        if not names:
            ap.error("--%s %s needs --names" % (kind, path))
        text = select(open(path).read(), names)
        compiled = rtla.Actions(cfg, text) if kind == "actions" else rtla.Predicates(cfg, text)
        lines.append(("%s %s" % (kind, ",".join(names)), {kind: compiled}))
    out = {"shape": dict(zip(("n_server", "n_value", "max_term", "max_log", "max_copies", "max_msgs"), SHAPE)),
           "bag_cap": 18, "walks": args.walks, "depth": args.depth, "seed": args.seed, "host_threads": args.threads,
           "level_kernel_reference": LEVEL_KERNEL_REF, "runs": []}
    with rtla.Checker(cfg) as ck:
        out["device"] = json.loads(ck.device_info()) if ck.device_info().startswith("{") else ck.device_info()
        ck.init()
        for lv in levels:
            while len(ck.levels) < lv:
                ck.step()
            last = ck.levels[-1]
            level_gen_s = last.generated / (last.kernel_ms / 1e3) if last.kernel_ms else None
            for label, kw in lines:
                ck.simulate(min(args.walks, 1 << 16), args.depth, seed=args.seed, **kw)   # warm-up (buffers, code object)
                gpu = []
                for _ in range(args.reps):
                    t = time.time()
                    res = ck.simulate(args.walks, args.depth, seed=args.seed, **kw)
                    gpu.append((res.kernel_ms, (time.time() - t) * 1e3, res))
                gpu.sort(key=lambda x: x[0])
                kms, wall_ms, res = gpu[len(gpu) // 2]
                ref = rtla.sim_replay(cfg, ck.frontier_flat(), args.walks, args.depth, seed=args.seed,
                                      threads=args.threads, **kw)
                same = (ck.simulate(args.walks, args.depth, seed=args.seed, ends=True, **kw).ends == ref.ends and
                        (res.steps, res.generated, res.taken, res.state_evaluated, res.step_evaluated) ==
                        (ref.steps, ref.generated, ref.taken, ref.state_evaluated, ref.step_evaluated))
                run = {"bfs_level": lv, "sets": label, "state_evaluated": res.state_evaluated,
                       "step_evaluated": res.step_evaluated, "frontier_states": ck.frontier_size(), "steps": res.steps,
                       "generated": res.generated, "status": res.status,
                       "gpu_kernel_ms": round(kms, 3), "gpu_kernel_ms_all": [round(g[0], 3) for g in gpu],
                       "gpu_call_wall_ms": round(wall_ms, 3),
                       "gpu_steps_per_s": res.steps / (kms / 1e3), "gpu_generated_per_s": res.generated / (kms / 1e3),
                       "host_ms": round(ref.kernel_ms, 3), "host_steps_per_s": ref.steps / (ref.kernel_ms / 1e3),
                       "host_generated_per_s": ref.generated / (ref.kernel_ms / 1e3),
                       "gpu_over_host": ref.kernel_ms / kms, "ends_equal_host": same,
                       "level_kernel_generated_per_s_this_level": level_gen_s,
                       "gpu_generated_rate_over_level_kernel_reference":
                           (res.generated / (kms / 1e3)) / (LEVEL_KERNEL_REF["generated"] / (LEVEL_KERNEL_REF["ms"] / 1e3))}
                out["runs"].append(run)
                print(json.dumps(run))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0 if all(r["ends_equal_host"] for r in out["runs"]) else 1


if __name__ == "__main__":
    sys.exit(main())
