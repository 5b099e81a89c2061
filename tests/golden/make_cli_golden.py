"""Write the command line's transcripts, tests/golden/cli/<scenario>.json, from a given build's binary.

The fixtures pin the behaviour of the commit whose binary wrote them, so they are regenerated only when a change
of the output is meant: build that commit (a worktree of it will do) and pass its rtla here.  Every scenario
(tests/cli_scenarios.py) is run --runs times in fresh directories; the normalised transcripts must all be equal,
and the last command must say what the scenario is about.  The same runs, normalised by the clock, rate, device
and directory masks alone, show what else differs between runs of one binary: that is written to EVIDENCE.md
beside the fixtures (one section for the host scenarios, one for the device scenarios, each written afresh by
the run that covers it), and is the reason for every further mask.

    python tests/golden/make_cli_golden.py --cli PATH/rtla [--gpu | --cpu] [--runs N] [--out DIR] [--only=a,b]
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cli_scenarios  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cli", required=True)
    ap.add_argument("--gpu", action="store_true", help="the scenarios that need a device only")
    ap.add_argument("--cpu", action="store_true", help="the scenarios that need none only")
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=cli_scenarios.GOLDEN)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    bad, evidence = 0, {False: [], True: []}  # (by scenario.gpu)
    for s in cli_scenarios.SCENARIOS:
        if (a.gpu and not s.gpu) or (a.cpu and s.gpu) or (a.only and s.name not in a.only.split(",")):
            continue
        runs, strict = [], []
        for k in range(a.runs):
            with tempfile.TemporaryDirectory(prefix="rtla-golden-%d-" % k) as tmp:
                strict.append(cli_scenarios.transcript(a.cli, s, os.path.join(tmp, "run"), strict=True))
            codes = [r["returncode"] for r in strict[-1]]
            if not set(codes) <= {0, 12, 150, 151, 255}:  # killed or crashed: nothing more is started
                print("STOPPED: %s ended with %s\n%s" % (s.name, codes, strict[-1]))
                return 2
            # (the fixture is the same run under the scenario's own masks: normalising is idempotent)
            runs.append([dict(r, stdout=cli_scenarios.normalise("\n".join(r["stdout"]), "<TMP>", s.mask_states),
                              stderr=cli_scenarios.normalise("\n".join(r["stderr"]), "<TMP>", sort_ranks=s.sort_ranks))
                         for r in strict[-1]])
        for k in range(1, a.runs):  # what the strict masks leave different, against the first run
            pairs = [(x, y) for r0, r in zip(strict[0], strict[k]) for key in ("stdout", "stderr")
                     for x, y in zip(r0[key], r[key]) if x != y]
            if pairs:
                evidence[s.gpu].append("- `%s`, run 1 against run %d: %d lines differ, the first `%s` against `%s`"
                                       % (s.name, k + 1, len(pairs), pairs[0][0], pairs[0][1]))
        said = "\n".join(runs[0][-1]["stdout"] + runs[0][-1]["stderr"])
        if any(r != runs[0] for r in runs) or s.expect not in said:
            bad += 1
            print("NOT WRITTEN (runs differ after masking, or %r is not said): %s" % (s.expect, s.name), flush=True)
            continue
        with open(os.path.join(a.out, s.name + ".json"), "w") as f:
            json.dump({"runs": runs[0]}, f, indent=1)
            f.write("\n")
        print("wrote %s: exit %s" % (s.name, [r["returncode"] for r in runs[0]]), flush=True)
    if a.only:  # (a few scenarios are no evidence for a section)
        return 1 if bad else 0
    path, title = os.path.join(a.out, "EVIDENCE.md"), "# What differs between runs of one binary\n"
    kinds = [gpu for gpu in (False, True) if not (a.gpu and not gpu) and not (a.cpu and gpu)]
    old = open(path).read().split("\n## ")[1:] if os.path.exists(path) else []
    keep = [sec for sec in old if not any(sec.startswith("host" if not gpu else "device") for gpu in kinds)]
    new = ["%s scenarios: %d runs of each, compared under the clock, rate, device and directory masks alone\n\n%s\n"
           % ("device" if gpu else "host", a.runs, "\n".join(evidence[gpu]) or "- no line differs") for gpu in kinds]
    with open(path, "w") as f:
        f.write(title + "".join("\n## " + sec.rstrip("\n") + "\n" for sec in sorted(keep + new, reverse=True)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
