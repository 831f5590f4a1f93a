#!/usr/bin/env python3
"""profiles/post_rows_resources.py [csrc-dir] -- the compiler's resource report (-Rpass-analysis=kernel-resource-usage) of every kernel of
pt_kernels_filter.hip and pt_kernels_upsample.hip, gfx950, with the flags of csrc/build.sh for each of the two libraries.  No GPU involved.
Prints the report of profiles/post_rows/kernel_resources.txt; with the csrc directory of another commit (git archive) it prints that commit's."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "2015-raytracing_amd", "csrc")
BASE = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-ffp-contract=off", "-fno-fast-math",
        "-fno-slp-vectorize", "-Rpass-analysis=kernel-resource-usage", "-c"]
LIBS = (("libmirt.so (-fhip-fp32-correctly-rounded-divide-sqrt)", ["-fhip-fp32-correctly-rounded-divide-sqrt"]),
        ("libmirt_default.so (-fno-hip-fp32-correctly-rounded-divide-sqrt -DPT_PLAIN_DIV=1)", ["-fno-hip-fp32-correctly-rounded-divide-sqrt", "-DPT_PLAIN_DIV=1"]))
KEEP = ("TotalSGPRs", " VGPRs:", "AGPRs", "ScratchSize", "Dynamic Stack", "Occupancy", "SGPRs Spill", "VGPRs Spill", "LDS Size")


def report(src, flags):
    with tempfile.TemporaryDirectory() as t:
        r = subprocess.run(BASE + flags + [os.path.join(CSRC, src), "-o", os.path.join(t, "x.o")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True)
    out = []
    for l in r.stdout.splitlines():
        m = re.search(r"remark:\s+(.*?)\s+\[-Rpass-analysis", l)
        if not m:
            continue
        text = m.group(1).strip()
        f = re.match(r"Function Name: (\S+)", text)
        if f:
            out.append(subprocess.run(["c++filt", f.group(1)], stdout=subprocess.PIPE, text=True).stdout.strip())
        elif any(k.strip() in text for k in KEEP):
            out.append("  " + text)
    return out


def main():
    for name, flags in LIBS:
        print(f"== {name} ==")
        for src in ("pt_kernels_filter.hip", "pt_kernels_upsample.hip"):
            print("\n".join(report(src, flags)))
        print()


if __name__ == "__main__":
    main()
