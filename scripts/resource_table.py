#!/usr/bin/env python3
"""Table of -Rpass-analysis=kernel-resource-usage remarks of two builds of hc_fgk.hip, one line per
encode_kernel / decode_kernel instantiation (the form of profiles/r1x_resource_usage.txt):
    hipcc <the Makefile's flags> --cuda-device-only -S -Rpass-analysis=kernel-resource-usage \
        [-D...] huffman-codec_amd/csrc/hc_fgk.hip -o /dev/null 2> parent.txt     (and shipped.txt)
    python3 scripts/resource_table.py parent.txt shipped.txt
VGPR / SGPR / scratch bytes per lane / LDS bytes per block / waves per SIMD; * marks a line that
differs, ! one that is worse than the parent's. Exit status 1 if any line is worse."""
import re
import subprocess
import sys

KEYS = [("VGPRs", 1), ("TotalSGPRs", 0), ("ScratchSize [bytes/lane]", 1), ("LDS Size [bytes/block]", 1),
        ("Occupancy [waves/SIMD]", -1)]  # 1: more is worse, -1: fewer is worse, 0: not judged


def parse(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            cur = t.split(":", 1)[1].strip()
            out[cur] = {}
        elif cur and ":" in t:
            k, v = t.rsplit(":", 1)
            out[cur][k.strip()] = v.strip()
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return [re.sub(r"^void hc::\(anonymous namespace\)::|\(hc::Batch\)$", "", s) for s in r.stdout.split("\n")]


def main():
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    names = [n for n in b if re.search(r"13(encode|decode)_kernel", n)]
    worse = 0
    for n, d in zip(names, demangle(names)):
        va = [int(a[n][k]) for k, _ in KEYS]
        vb = [int(b[n][k]) for k, _ in KEYS]
        bad = any(s * (y - x) > 0 for (_, s), x, y in zip(KEYS, va, vb))
        worse += bad
        fmt = lambda v: f"{v[0]:2d} / {v[1]:3d} / {v[2]:2d} / {v[3]:5d} / {v[4]}"
        print(f"{d:<44} parent {fmt(va)}   shipped {fmt(vb)}" + ("   !" if bad else "   *" if va != vb else ""))
    return 1 if worse else 0


if __name__ == "__main__":
    sys.exit(main())
