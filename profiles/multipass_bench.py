#!/usr/bin/env python3
"""profiles/multipass_bench.py -- P progressive passes as P ordinary calls against ONE mirt_render_passes call.

  python3 profiles/multipass_bench.py [--passes 4] [--reps 5] [--out FILE.json]

Two scenes: cornell.xml 1920x1080 x 256 rays per pixel at depth 8 (the headline frame) and cornell_teapot3.xml 1920x1080 x 16 at depth 5 (the grid
kernel).  For each, the frame of P passes is rendered both ways from the same seeds:
  ordinary: mirt_render_first_pass + (P - 1) x mirt_render_pass into a per-ray accumulator (16 B per ray);
  one call: mirt_render_passes(P, MIRT_PASSES_FRESH) without an accumulator, twice: with primary-hit reuse (one_call_reuse, MIRT_MULTIPASS_REUSE=1:
            passes after the first take segment 0 from LDS) and as the plain loop (one_call_plain, =0; the runtime reads the switch per launch).
Times are device events on the context's stream (mirt_timer_start / mirt_timer_stop_ms), around the passes only (the seed reset before each frame is outside), after one
warm-up frame of each, over --reps repetitions that alternate the three ways; reported as median, min and max.  Bytes: the caller's buffers, and
the device's free memory before the renderer is made minus after its first frame (with what the runtime grew for it: masks, scratch).  `equal`:
pixel, radiance and seeds bitwise equal to the ordinary passes' after the last repetition.  Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import __graft_entry__ as g
    g.load_package()
    from raytracing_amd.pyhost import mirt, render, scene

    torch.cuda.init()
    ctx = mirt.Context(0)
    P = args.passes
    scenes = []
    packed = open(os.path.join(ROOT, "tests", "golden", "scene_cornell_1920x1080_r256.json")).read()
    scenes.append(("cornell_1920x1080_r256_depth8", scene.PackedScene(packed), 8))
    fx = np.load(os.path.join(ROOT, "tests", "golden", "cornell_teapot3_32x24_r4.npz"))
    scenes.append(("cornell_teapot3_1920x1080_r16_depth5", scene.PackedScene(bytes(fx["scene_json"]).decode()).resized(1920, 1080, 16), 5))

    out = {"passes": P, "reps": args.reps, "scenes": {}}
    for name, sc, bounces in scenes:
        rec = {}
        ways = {}

        def frame(way):
            fr = ways[way]
            ctx.seed_fill(fr.seeds, fr.first_ray, fr.nrays, 0)
            fr.passes = 1
            os.environ["MIRT_MULTIPASS_REUSE"] = "0" if way == "one_call_plain" else "1"
            ctx.timer_start()
            if way == "ordinary":
                for p in range(P):
                    fr.execute_render(bounces=bounces, fresh=(p == 0))
            else:
                fr.execute_passes(P, bounces=bounces, fresh=True)
            return ctx.timer_stop_ms()

        for way, keep in (("one_call_reuse", False), ("one_call_plain", False), ("ordinary", True)):
            torch.cuda.synchronize()
            free0 = torch.cuda.mem_get_info()[0]
            fr = render.FusedRenderer(ctx, sc, want_radiance=True, keep_acu=keep)
            ways[way] = fr
            frame(way)   # warm-up; then what the device gave this way (its buffers and whatever the runtime grew for it)
            free1 = torch.cuda.mem_get_info()[0]
            rec[way] = {"caller_bytes": fr.nrays * 4 + (fr.nrays * 16 if keep else 0) + fr.npix * 20, "acu_bytes": fr.nrays * 16 if keep else 0,
                        "device_bytes": int(free0 - free1)}
        ms = {w: [] for w in ways}
        for _ in range(args.reps):
            for way in ("ordinary", "one_call_plain", "one_call_reuse"):
                ms[way].append(frame(way))
        for way in ways:
            v = ms[way]
            rec[way].update({"ms_median": round(float(np.median(v)), 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3),
                             "ms_per_pass_median": round(float(np.median(v)) / P, 3), "ms_all": [round(x, 3) for x in v]})
        deferred = ctx.pass_deferred()   # the last call: the one-call frame with reuse
        b = ways["ordinary"]
        for way in ("one_call_plain", "one_call_reuse"):
            a = ways[way]
            rec[way]["equal"] = bool(np.array_equal(a.pixel.read(np.uint8), b.pixel.read(np.uint8)) and
                                     np.array_equal(a.radiance.read(np.uint32), b.radiance.read(np.uint32)) and
                                     np.array_equal(a.seeds.read(np.int32), b.seeds.read(np.int32)))
            rec[way]["speedup"] = round(rec["ordinary"]["ms_median"] / rec[way]["ms_median"], 4)
        rec["one_call_deferred_samples"] = deferred
        out["scenes"][name] = rec
        for fr in ways.values():
            fr.release()
        print(json.dumps({name: rec}), file=sys.stderr, flush=True)
    ctx.destroy()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
