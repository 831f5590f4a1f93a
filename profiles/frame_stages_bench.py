#!/usr/bin/env python3
"""profiles/frame_stages_bench.py out.json -- the kernel-by-kernel trace kernels of Assign04 / Assign07 alone, on one device: bench.py's own `frames`
record (k_a04_meshTrace on parliament and teapot at 1024 x 1024, k_a07_meshTrace on parliament at 1080p with n_slabs 2 / 16 / 32) and, measured the
same way (render_frame's HIP events around the trace kernel, median and minimum of five frames after one warm-up), k_a07_molTrace on the 3IZ4
molecule at 1080p, which bench.py does not time.  The library is pyhost's: MIRT_LIB_PATH picks an A/B build.

profiles/frame_stages_bench.py --bands parent1.json new1.json parent2.json new2.json -- the band rule of profiles/post_refactor/README.md over
four such records of one alternating job: per kernel_ms the parent's two runs' [min, max] widened by their difference on each side."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import __graft_entry__ as graft  # noqa: E402
import bench  # noqa: E402


def measure(out):
    graft.load_package()
    from raytracing_amd.pyhost import mirt, render
    ctx = mirt.Context(0)
    rec = bench.frames_record(ctx, lambda *a: None, render, False)
    rec.pop("note", None)
    fx = np.load(os.path.join(ROOT, "tests", "golden", "frame_a07_mol_3IZ4_n16_96x64.npz"))
    fp = render.FramePacked(render.frame_resized(json.loads(bytes(fx["frame_json"]).decode()), 1920, 1080))
    render.render_frame(ctx, fp)
    ms = []
    for _ in range(5):
        t = {}
        render.render_frame(ctx, fp, timing=t)
        ms.append(t["trace_ms"])
    rec["a07_mol_3IZ4_1080p_n16"] = {"kernel": "pt::k_a07_molTrace", "kernel_ms": round(float(np.median(ms)), 4), "kernel_ms_min": round(min(ms), 4)}
    ctx.destroy()
    with open(out, "w") as fh:
        json.dump({"library": os.path.relpath(mirt.LIB_PATH, ROOT), "frames": rec}, fh, indent=1)
        fh.write("\n")
    for tag, r in rec.items():
        print(tag, r["kernel_ms"], r["kernel_ms_min"], flush=True)


def bands(paths):
    p1, n1, p2, n2 = [json.load(open(p))["frames"] for p in paths]
    for tag in p1:
        a, b = p1[tag]["kernel_ms"], p2[tag]["kernel_ms"]
        lo, hi = min(a, b) - abs(a - b), max(a, b) + abs(a - b)
        for r in (n1, n2):
            v = r[tag]["kernel_ms"]
            where = "inside" if lo <= v <= hi else "below" if v < lo else "ABOVE by %.2f %%" % ((v / hi - 1) * 100)
            print("%-28s %-20s parent %.4f %.4f  band [%.4f, %.4f]  new %.4f  %s  (minima: parent %.4f %.4f, new %.4f)" % (
                tag, p1[tag]["kernel"], a, b, lo, hi, v, where, p1[tag]["kernel_ms_min"], p2[tag]["kernel_ms_min"], r[tag]["kernel_ms_min"]))


if __name__ == "__main__":
    if sys.argv[1] == "--bands":
        bands(sys.argv[2:6])
    else:
        measure(sys.argv[1])
