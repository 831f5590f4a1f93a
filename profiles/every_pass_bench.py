#!/usr/bin/env python3
"""profiles/every_pass_bench.py -- the frame after every pass of one mirt_render_passes call, against the last frame only and against ordinary passes.

  python3 profiles/every_pass_bench.py [--passes 4] [--reps 5] [--out FILE.json]

Two scenes: cornell.xml 1920x1080 x 256 rays per pixel at depth 8 and cornell_teapot3.xml 1920x1080 x 16 at depth 5.  Each frame of P passes is rendered
three ways from the same seeds:
  last_frame:  mirt_render_passes(P, MIRT_PASSES_FRESH) without an accumulator -- the frame after the last pass only;
  every_frame: the same with MIRT_PASSES_EVERY_FRAME -- P frames into caller buffers of P x 20 B per pixel;
  ordinary:    mirt_render_first_pass + (P - 1) x mirt_render_pass with the 16 B per ray accumulator, what a progressive host does today.
Times are device events (mirt_timer_start / mirt_timer_stop_ms) around the passes only, after one warm-up frame of each, over --reps repetitions that
alternate the three ways; median, min and max.  bytes_per_ray: what the caller's buffers hold per ray (seeds, acu, frames).  `equal`: every frame of
every_frame against the ordinary passes' pixel / radiance after each pass (read back after the timed repetitions, from a run of its own).  One JSON line."""
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

    import __graft_entry__ as g
    g.load_package()
    from raytracing_amd.pyhost import mirt, render, scene

    ctx = mirt.Context(0)
    P = args.passes
    fx = np.load(os.path.join(ROOT, "tests", "golden", "cornell_teapot3_32x24_r4.npz"))
    scenes = [("cornell_1920x1080_r256_depth8", scene.PackedScene(open(os.path.join(ROOT, "tests", "golden", "scene_cornell_1920x1080_r256.json")).read()), 8),
              ("cornell_teapot3_1920x1080_r16_depth5", scene.PackedScene(bytes(fx["scene_json"]).decode()).resized(1920, 1080, 16), 5)]
    out = {"passes": P, "reps": args.reps, "scenes": {}}
    for name, sc, bounces in scenes:
        a = render.FusedRenderer(ctx, sc, keep_acu=False)                  # last_frame and every_frame share seeds and buffers
        o = render.FusedRenderer(ctx, sc, keep_acu=True)
        fpix, frad = ctx.buffer(P * a.npix * 4), ctx.buffer(P * a.npix * 16)
        last_d = a.dev.pass_desc(a.seeds, None, a.pixel, a.radiance, pass_index=1, bounces=bounces)
        every_d = a.dev.pass_desc(a.seeds, None, fpix, frad, pass_index=1, bounces=bounces)

        def frame(way):
            fr = o if way == "ordinary" else a
            ctx.seed_fill(fr.seeds, fr.first_ray, fr.nrays, 0)
            fr.passes = 1
            ctx.timer_start()
            if way == "ordinary":
                for p in range(P):
                    fr.execute_render(bounces=bounces, fresh=(p == 0))
            else:
                ctx.render_passes(last_d if way == "last_frame" else every_d, P, fresh=True, every_frame=(way == "every_frame"))
            return ctx.timer_stop_ms()

        ways = ("last_frame", "every_frame", "ordinary")
        for w in ways:
            frame(w)
        ms = {w: [] for w in ways}
        for _ in range(args.reps):
            for w in ways:
                ms[w].append(frame(w))
        rays = a.nrays
        rec = {}
        for w in ways:
            v = ms[w]
            frames_b = (P if w == "every_frame" else 1) * a.npix * 20
            rec[w] = {"ms_median": round(float(np.median(v)), 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3),
                      "ms_per_pass_median": round(float(np.median(v)) / P, 3), "ms_all": [round(x, 3) for x in v],
                      "bytes_per_ray": round((rays * 4 + (rays * 16 if w == "ordinary" else 0) + frames_b) / rays, 4)}
        rec["every_vs_last"] = round(rec["every_frame"]["ms_median"] / rec["last_frame"]["ms_median"], 4)
        rec["every_vs_ordinary"] = round(rec["every_frame"]["ms_median"] / rec["ordinary"]["ms_median"], 4)
        # equality: each frame of the every-frame call against the ordinary passes' frame after that pass
        frame("every_frame")
        ctx.seed_fill(o.seeds, o.first_ray, o.nrays, 0)
        o.passes = 1
        ok = True
        gp, gr = fpix.read(np.uint8).reshape(P, -1), frad.read(np.uint32).reshape(P, -1)
        for p in range(P):
            o.execute_render(bounces=bounces, fresh=(p == 0))
            ok = ok and np.array_equal(gp[p], o.pixel.read(np.uint8)) and np.array_equal(gr[p], o.radiance.read(np.uint32))
        ok = ok and np.array_equal(a.seeds.read(np.int32), o.seeds.read(np.int32))
        rec["equal"] = bool(ok)
        out["scenes"][name] = rec
        print(json.dumps({name: rec}), file=sys.stderr, flush=True)
        for b in (fpix, frad):
            b.release()
        a.release()
        o.release()
    ctx.destroy()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
