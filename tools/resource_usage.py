#!/usr/bin/env python3
"""Device-side resource usage of kernel translation units (hipcc
-Rpass-analysis=kernel-resource-usage): one line per function with its
VGPRs, AGPRs, spilled VGPRs, scratch bytes per lane, occupancy and LDS, and
the bytes of its code (the function symbol's size in the gfx950 code object).

    python tools/resource_usage.py [--src DIR] [unit ...] [-D...]   (units: csrc/*.hip names, default all)

--src DIR: the csrc directory to compile (default: this checkout's), e.g. that
of another commit's worktree, to compare two commits with the same tool.
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "raft-tla_amd", "csrc")
READELF = "/opt/rocm/llvm/bin/llvm-readelf"
FIELDS = [("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("VGPRs Spill", "spill"), ("ScratchSize [bytes/lane]", "scratch"),
          ("Occupancy [waves/SIMD]", "occ"), ("LDS Size [bytes/block]", "lds")]


def code_sizes(obj):
    """{function symbol: bytes} of a device code object."""
    out = subprocess.run([READELF, "-s", "-W", obj], capture_output=True, text=True).stdout
    sizes = {}
    for line in out.splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC" and f[6] != "UND":
            sizes[f[7]] = int(f[2], 0)
    return sizes


def usage(unit, flags, src=SRC):
    with tempfile.TemporaryDirectory() as tmp:
        obj = os.path.join(tmp, unit + ".co")
        cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++20", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-result",
               "-Rpass-analysis=kernel-resource-usage", "--offload-device-only", "--no-gpu-bundle-output", "-c", "-o", obj,
               os.path.join(src, unit + ".hip")] + flags
        err = subprocess.run(cmd, capture_output=True, text=True).stderr
        sizes = code_sizes(obj) if os.path.exists(obj) else {}
    rows, cur = [], None
    for line in err.splitlines():
        m = re.search(r"remark: +Function Name: (\S+)", line)
        if m:
            cur = {"name": m.group(1), "code": sizes.get(m.group(1))}
            rows.append(cur)
            continue
        for key, short in FIELDS:
            m = re.search(r"remark: +%s: (\d+)" % re.escape(key), line)
            if m and cur is not None:
                cur[short] = int(m.group(1))
    return rows


def main():
    args = sys.argv[1:]
    src = SRC
    if "--src" in args:
        k = args.index("--src")
        src = os.path.abspath(args[k + 1])
        del args[k:k + 2]
    units = [a for a in args if not a.startswith("-")]
    flags = [a for a in args if a.startswith("-")]
    if not units:
        units = sorted(f[:-4] for f in os.listdir(src) if f.endswith(".hip"))
    print("# unit | function (mangled prefix) | VGPRs AGPRs | spill VGPR | scratch B/lane | waves/SIMD | LDS B | code B")
    for u in units:
        for r in usage(u, flags, src):
            print("%s | %s | %s %s | %s | %s | %s | %s | %s" % (u, r["name"][:90], r.get("vgpr"), r.get("agpr"),
                                                             r.get("spill"), r.get("scratch"), r.get("occ"),
                                                             r.get("lds"), r.get("code")))


if __name__ == "__main__":
    main()
