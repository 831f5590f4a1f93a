#!/usr/bin/env python3
"""profiles/frame_one_launch_bench.py [out.json] -- an Assign04 / Assign07 frame as two launches (initTrace + the trace kernel, back to back: the
kernel-by-kernel path, whose kernels this tree leaves untouched) against the one fused launch (mirt_render_frame), on one device.
Per configuration -- BASELINE config 2 (house_of_parliament, brute force, 1024 x 1024), config 3 at n_slabs 2 and 16 (1920 x 1080), the 3IZ4 molecule
at 1920 x 1080 -- three things:
  two_launch_ms   HIP-event time around the two enqueues, buffers resident
  one_launch_ms   HIP-event time around mirt_render_frame (no ray buffer), same buffers
  wall ms         one frame end to end, uploads and pixel read-back included: render_frame_one_launch against render_frame
Each is the median of REPEATS runs after WARMUP; the spread is the interquartile range and min..max of the same runs.  Events on a stream that is
otherwise idle; the two variants alternate so that clock drift hits both.  Writes one JSON record stamped with the csrc hash (bench.csrc_sha256)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import __graft_entry__ as graft  # noqa: E402
import bench  # noqa: E402

WARMUP, REPEATS, WALL_REPEATS = 5, 40, 8


def fixture(name):
    fx = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    return json.loads(bytes(fx["frame_json"]).decode())


def stats(v):
    v = np.sort(np.asarray(v, np.float64))
    q = lambda f: float(v[int(round(f * (len(v) - 1)))])   # noqa: E731
    return {"median": q(0.5), "q1": q(0.25), "q3": q(0.75), "min": float(v[0]), "max": float(v[-1]), "n": len(v)}


def main():
    graft.load_package()
    from raytracing_amd.pyhost import mirt, render
    ctx = mirt.Context(0)
    a04, a07 = fixture("frame_a04_parliament_96x64"), fixture("frame_a07_parliament_n16_160x120")
    jobs = [("config2_a04_parliament_1024x1024", render.frame_resized(a04, 1024, 1024)),
            ("config3_a07_parliament_n2_1920x1080", render.frame_resized(render.frame_regrid(ctx, a07, a04, 2), 1920, 1080)),
            ("config3_a07_parliament_n16_1920x1080", render.frame_resized(a07, 1920, 1080)),
            ("a07_mol_3IZ4_n16_1920x1080", render.frame_resized(fixture("frame_a07_mol_3IZ4_n16_96x64"), 1920, 1080))]
    rows = {}
    for name, d in jobs:
        p = render.FramePacked(d)
        f = render.FrameOneLaunch(ctx, p, keep_rays=True)   # the ray buffer is for the two launches; the fused launch is given none
        rays, f.rays = f.rays, None
        pre = {4: "A04:", 7: "A07:"}[p.assign]
        it = ctx.kernel(pre + "initTrace").set_args(f.pixels, p.cam, rays)
        if p.assign == 7:
            it.set_arg(3, p.bounds)
        u32 = lambda v: np.array([v], np.uint32)   # noqa: E731
        if p.mol:
            mt = ctx.kernel(pre + "molTrace").set_args(f.pixels, p.cam, rays, u32(p.s_size), f.mol["atoms"], f.mol["mindex"], f.mol["mcolor"], p.bounds, u32(p.n_slabs), f.mol["slab_size"])
        else:
            mt = ctx.kernel(pre + "meshTrace").set_args(f.pixels, p.cam, rays, u32(p.t_size), f.mesh["pos"], f.mesh["normal"], f.mesh["mindex"], f.mesh["mcolor"])
            if p.assign == 7:
                mt.set_arg(8, p.bounds).set_arg(9, u32(p.n_slabs)).set_arg(10, f.mesh["slab_size"])
        g = [-(-p.width // 8) * 8, -(-p.height // 8) * 8]

        def two():
            ctx.timer_start()
            it.enqueue(g, [8, 8])
            mt.enqueue(g, [8, 8])
            return ctx.timer_stop_ms()

        def one():
            ctx.timer_start()
            f.render()
            return ctx.timer_stop_ms()
        two(); px2 = f.pixels.read(np.uint8)
        one(); px1 = f.pixels.read(np.uint8)
        assert np.array_equal(px1, px2), name
        t2, t1 = [], []
        for i in range(WARMUP + REPEATS):
            a, b = two(), one()
            if i >= WARMUP:
                t2.append(a); t1.append(b)
        w2, w1 = [], []
        for i in range(2 + WALL_REPEATS):
            ctx.finish(); t = time.perf_counter(); render.render_frame(ctx, p); a = (time.perf_counter() - t) * 1e3
            ctx.finish(); t = time.perf_counter(); render.render_frame_one_launch(ctx, p); b = (time.perf_counter() - t) * 1e3
            if i >= 2:
                w2.append(a); w1.append(b)
        rows[name] = {"two_launch_ms": stats(t2), "one_launch_ms": stats(t1), "wall_render_frame_ms": stats(w2), "wall_render_frame_one_launch_ms": stats(w1),
                      "lit_fraction": float((px1.reshape(-1, 4)[:, :3].max(axis=1) > 0).mean())}
        print(name, json.dumps(rows[name]), flush=True)
        it.release(); mt.release(); rays.release(); f.release()
    rec = {"csrc_sha256": bench.csrc_sha256(), "device": mirt.lib().mirt_version().decode(), "warmup": WARMUP, "repeats": REPEATS, "wall_repeats": WALL_REPEATS,
           "what": "HIP-event ms of initTrace + trace kernel back to back vs the one fused launch; wall ms of one frame end to end (uploads + read-back)", "configs": rows}
    ctx.destroy()
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "frame_one_launch", "timing.json")
    with open(out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
