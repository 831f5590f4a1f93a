#!/usr/bin/env python3
"""profiles/resolve_counts_bench.py -- a frame's first pass at ray counts above 256 that are not 256 times a power of two, two ways.

  python3 profiles/resolve_counts_bench.py [--ks 17,20,24,31,32] [--reps 5] [--teapot-k 17] [--out FILE.json]

cornell.xml at 1920x1080, one pass, depth 5, k x k rays per pixel for each k of --ks (k = 32, 1024 rays, is the control: it resolved in the pass
before the segment plan), and cornell_teapot3.xml (grid meshes) at --teapot-k.  Two routes from the same seeds, in the same process:
  in_pass:  mirt_render_first_pass without an accumulator: one launch pair per segment of the plan (pt_launch.hpp fused_segment), the pixels
            resolved in the pass -- 4 B per ray resident;
  acu_copy: the same call with a per-ray accumulator on a context made with MIRT_INPASS_RESOLVE=0: one launch pair over every ray, then the
            separate copyToPixel -- 20 B per ray resident.
Times are device events on each context's stream (mirt_timer_start / mirt_timer_stop_ms) around the pass only (the seed reset is outside), after
one warm-up frame of each, over --reps repetitions that alternate the two routes; reported as median, min and max.  `equal`: pixel, radiance and
seeds bitwise equal after the last repetition; `deferred_samples`: mirt_pass_deferred after it (in_pass counts whole blocks of 256).  Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def segments(rpp):
    out, off = [], 0
    while off < rpp:
        left = rpp - off
        n = rpp if rpp <= 256 else (256 if left >= 256 else 1 << (left.bit_length() - 1))
        out.append(n)
        off += n
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="17,20,24,31,32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--teapot-k", type=int, default=17)
    ap.add_argument("--bounces", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import __graft_entry__ as g
    g.load_package()
    from raytracing_amd.pyhost import mirt, render, scene

    ctx = mirt.Context(0)
    os.environ["MIRT_INPASS_RESOLVE"] = "0"
    try:
        sep = mirt.Context(0)
    finally:
        del os.environ["MIRT_INPASS_RESOLVE"]
    cornell = scene.PackedScene(open(os.path.join(ROOT, "tests", "golden", "scene_cornell_1920x1080_r256.json")).read())
    fx = np.load(os.path.join(ROOT, "tests", "golden", "cornell_teapot3_32x24_r4.npz"))
    teapot = scene.PackedScene(bytes(fx["scene_json"]).decode())
    cases = [("cornell", cornell, int(k)) for k in args.ks.split(",")] + ([("cornell_teapot3", teapot, args.teapot_k)] if args.teapot_k else [])

    out = {"width": 1920, "height": 1080, "bounces": args.bounces, "reps": args.reps, "cases": {}}
    for name, sc0, k in cases:
        rpp = k * k
        sc = sc0.resized(1920, 1080, rpp)
        routes = {"in_pass": (ctx, render.FusedRenderer(ctx, sc, keep_acu=False)), "acu_copy": (sep, render.FusedRenderer(sep, sc, keep_acu=True))}

        def frame(route):
            c, fr = routes[route]
            c.seed_fill(fr.seeds, fr.first_ray, fr.nrays, 0)
            fr.passes = 1
            c.timer_start()
            fr.execute_render(bounces=args.bounces, fresh=True)
            return c.timer_stop_ms()

        for r in routes:
            frame(r)   # warm-up
        ms = {r: [] for r in routes}
        for _ in range(args.reps):
            for r in routes:
                ms[r].append(frame(r))
        a, b = routes["in_pass"][1], routes["acu_copy"][1]
        rec = {"k": k, "rays_per_pixel": rpp, "segments": segments(rpp), "rays": a.nrays,
               # what the optimistic kernel handed to the exact one in the last frame of each route: samples (acu_copy), or whole blocks of 256 (in_pass)
               "deferred_samples": {"in_pass": ctx.pass_deferred(), "acu_copy": sep.pass_deferred()},
               "resident_bytes": {"in_pass": a.nrays * 4 + a.npix * 20, "acu_copy": b.nrays * 20 + b.npix * 20},
               "equal": bool(np.array_equal(a.pixel.read(np.uint8), b.pixel.read(np.uint8)) and
                             np.array_equal(a.radiance.read(np.uint32), b.radiance.read(np.uint32)) and
                             np.array_equal(a.seeds.read(np.int32), b.seeds.read(np.int32)))}
        for r in routes:
            v = ms[r]
            rec[r] = {"ms_median": round(float(np.median(v)), 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3), "ms_all": [round(x, 3) for x in v]}
        rec["in_pass_speedup"] = round(rec["acu_copy"]["ms_median"] / rec["in_pass"]["ms_median"], 4)
        out["cases"][f"{name}_k{k}"] = rec
        for _, fr in routes.values():
            fr.release()
        print(json.dumps({f"{name}_k{k}": rec}), file=sys.stderr, flush=True)
    sep.destroy()
    ctx.destroy()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
