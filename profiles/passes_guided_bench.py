#!/usr/bin/env python3
"""profiles/passes_guided_bench.py [out.json [run-name]] -- what mirt_render_passes_guided saves over the two calls it stands for.

Per configuration (cornell.xml 1080p x 16, cornell.xml 1080p x 4, cornell_teapot3 1080p x 16; depth 8; 4 passes in one call, fresh, no per-ray
accumulator; each without and with a frame after every pass), each variant between two HIP events (mirt_timer_start / mirt_timer_stop_ms),
medians of 20 calls after 3 warm-ups, the variants alternating inside one loop so that drift hits them alike.  Every variant has its own
renderer, started from the same seeds:
  a  mirt_render_passes + mirt_render_guides
  b  mirt_render_passes_guided                     (left out when the loaded library lacks the entry point: a build of the parent commit,
                                                    MIRT_LIB_PATH -- its a and c are the comparison the unguided kernels must agree with)
  c  mirt_render_passes alone
saved = a - b; guides_cost = a - c (what the second trace costs), in_launch_cost = b - c (what writing the guides from the launch costs).
The comparison the numbers are for takes several processes (this tree, the parent commit's library through MIRT_LIB_PATH, this tree, the
parent's), so out.json holds a list, "runs", and every process ADDS its record to it under run-name ("run_<k>" where none is given); a record of
the same name is replaced.  A fresh measurement starts from no file.  Each record carries the hash of the kernel sources (the recipe of bench.py
csrc_sha256) when the library is this tree's."""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import __graft_entry__ as graft  # noqa: E402
from pass_guided_bench import TIMED, WARM, csrc_sha256, timed  # noqa: E402

PASSES = 4
WHAT = ("profiles/passes_guided_bench.py, one record per process in the order they ran on one MI355X: a, b, c = mirt_render_passes + mirt_render_guides, "
        "mirt_render_passes_guided, mirt_render_passes alone, in ms; one_launch_route false: the route rule sent b to the guide launches, so b is a")


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "passes_guided", "timing.json")
    graft.load_package()
    from raytracing_amd.pyhost import mirt, render, scene
    golden = os.path.join(ROOT, "tests", "golden")
    cornell = scene.PackedScene(open(os.path.join(golden, "scene_cornell_1920x1080_r256.json")).read())
    fx = np.load(os.path.join(golden, "cornell_teapot3_32x24_r4.npz"))
    teapot3 = scene.PackedScene(json.loads(bytes(fx["scene_json"]).decode()))
    configs = [(name, base, rpp, every) for every in (False, True) for name, base, rpp in (("cornell", cornell, 16), ("cornell", cornell, 4), ("cornell_teapot3", teapot3, 16))]
    has_guided = hasattr(mirt.lib(), "mirt_render_passes_guided")
    ctx = mirt.Context(0)
    other = bool(os.environ.get("MIRT_LIB_PATH"))
    res = {"run": None, "tree": "the library of MIRT_LIB_PATH" if other else "this tree", "csrc_sha256": None if other else csrc_sha256(), "library": os.path.basename(mirt.LIB_PATH),
           "width": 1920, "height": 1080, "bounces": 8, "passes": PASSES, "warm_ups": WARM, "timed_calls": TIMED, "configs": []}
    for name, base, rpp, every in configs:
        ps = base.resized(1920, 1080, rpp)
        npix, frames = ps.width * ps.height, (PASSES if every else 1)
        variants = ["a", "b", "c"] if has_guided else ["a", "c"]
        fr = {v: render.FusedRenderer(ctx, ps, keep_acu=False, want_radiance=False, seed_base=1) for v in variants}
        pixel = {v: ctx.buffer(frames * npix * 4) for v in variants}
        radiance = {v: ctx.buffer(frames * npix * 16) for v in variants}
        nh = {v: ctx.buffer(npix * 16) for v in variants if v != "c"}
        ad = {v: ctx.buffer(npix * 16) for v in variants if v != "c"}
        desc = {v: fr[v].dev.pass_desc(fr[v].seeds, None, pixel[v], radiance[v], pass_index=1, bounces=8) for v in variants}

        def two_calls():
            ctx.render_passes(desc["a"], PASSES, fresh=True, every_frame=every)
            ctx.render_guides(desc["a"], nh["a"], ad["a"])
        calls = {"a": two_calls, "b": lambda: ctx.render_passes_guided(desc["b"], PASSES, fresh=True, every_frame=every, normal_hits=nh["b"], albedo_depth=ad["b"]),
                 "c": lambda: ctx.render_passes(desc["c"], PASSES, fresh=True, every_frame=every)}
        before = ctx.guided_passes() if has_guided else 0
        times = {v: [] for v in variants}
        for rep in range(WARM + TIMED):
            for v in variants:
                ms = timed(ctx, calls[v])
                if rep >= WARM:
                    times[v].append(ms)
        rec = {"scene": name, "rays_per_pixel": rpp, "every_frame": every}
        for v in variants:
            rec[f"{v}_ms"] = round(statistics.median(times[v]), 4)
            rec[f"{v}_min_max"] = [round(min(times[v]), 4), round(max(times[v]), 4)]
        rec["guides_cost_ms"] = round(rec["a_ms"] - rec["c_ms"], 4)
        if has_guided:
            rec["one_launch_route"] = ctx.guided_passes() - before == WARM + TIMED
            rec["saved_ms"] = round(rec["a_ms"] - rec["b_ms"], 4)
            rec["in_launch_cost_ms"] = round(rec["b_ms"] - rec["c_ms"], 4)
            same = all(np.array_equal(x["a"].read(np.uint32), x["b"].read(np.uint32)) for x in (nh, ad, radiance, pixel))
            rec["buffers_identical"] = bool(same and np.array_equal(fr["a"].seeds.read(np.uint32), fr["b"].seeds.read(np.uint32)))
        res["configs"].append(rec)
        print(json.dumps(rec), flush=True)
        for b in list(nh.values()) + list(ad.values()) + list(pixel.values()) + list(radiance.values()):
            b.release()
        for r in fr.values():
            r.release()
    ctx.destroy()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    doc = {"what": WHAT, "runs": []}
    if os.path.exists(out_path):
        doc = json.load(open(out_path))
    res["run"] = sys.argv[2] if len(sys.argv) > 2 else f"run_{len(doc['runs']) + 1}"
    doc["runs"] = [r for r in doc["runs"] if r.get("run") != res["run"]] + [res]
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
