#!/usr/bin/env python3
"""profiles/view_ao_bench.py [--out FILE.json] [--size W H K] [--one-launch-only] -- ambient occlusion of a view camera in one launch (mirt_view_ao) against the
by-hand lower bound on the same library WITH THE AO RAYS ALREADY IN HAND: one mirt_view_guides call (the first hit) plus one mirt_trace_occluded
call on the identical, pre-generated AO rays.  Follows profiles/ao_bench.py.

  Cameras  equirect and oblique orthographic (eye at the scene box's centre looking along (0.3, -0.2, -1); the window 0.8 x the box's extents).
  Scenes   cornell (single-cell sets) and cornell_teapot3 (two grid meshes) at 1920 x 1080 x 4 (k = 2), 4 AO rays per hit sample; radius: a
           quarter of the scene box's diagonal; bias 0.001.
  Rays     the baseline's AO rays are built once, outside the timed region, by the composition the definition names: mirt_view_rays and
           mirt_trace_closest, the hits written into a Poi buffer, then bouncePaths x samples through mirt_enqueue on that unchanged buffer; after
           each the directions of the casting samples are read back and appended, with the origin p + n * bias and maxt = radius, as 32-byte
           mirt_ray records.  The baseline's time therefore OMITS mirt_view_rays, mirt_trace_closest's own pass over the rays (the guides call
           stands in for the first hit), the caller's ray generation, the read-backs and the rewrite.
  Check    the rays in hand are the kernel's: the not-occluded among them number what mirt_view_ao's `open` sums to, and there are `cast` of them.
  Method   one MI355X; per case medians of 20 calls between two HIP events (mirt_timer_start / mirt_timer_stop_ms) after 3 warm-ups, the
           variants alternating in one loop; the whole measurement twice (`runs`).
  Recorded without a bound: both medians, their min .. max, the ratio one_launch / (guides + occluded), mirt_view_ao_deferred, AO rays per second
  -- and for scale, per scene, mirt_render_ao of the thin lens at the same size (4 rays per pixel, the same AO descriptor).
  --one-launch-only: mirt_view_ao's medians alone, for an A/B of its launch bounds (MIRT_LIB_PATH names the library; -DPT_VIEW_AO_GRID_WAVES=N)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

WARM, TIMED = 3, 20
SAMPLES, BIAS = 4, 0.001
RAY_DT = np.dtype({"names": ["o", "d", "mint", "maxt"], "formats": [(np.float32, 3), (np.float32, 3), np.float32, np.float32],
                   "offsets": [0, 16, 32, 36], "itemsize": 48})   # the kernels' 48-byte Ray
POI_DT = np.dtype({"names": ["p", "normal", "atte", "matId"], "formats": [(np.float32, 3), (np.float32, 3), (np.float32, 3), np.int32],
                   "offsets": [0, 16, 32, 48], "itemsize": 64})
CAMERAS = ("equirect", "ortho")


def timed(ctx, call):
    ctx.finish()
    ctx.timer_start()
    call()
    return ctx.timer_stop_ms()


def camera(mirt, ps, model, k):
    b = np.asarray(ps.bounds, np.float64)
    lo, hi = b[0:3], b[4:7]
    eye = (lo + hi) / 2
    half = 0.8 * (hi - lo) / 2
    return mirt.view_desc(model, ps.width, ps.height, k=k, eye=eye, look_at=eye + np.array([0.3, -0.2, -1.0]), half_w=half[0], half_h=half[1])


def rays_in_hand(ctx, dev, ps, view, radius, log):
    """-> (a buffer of the casting samples' AO rays, 32 bytes each, sample-major: all of AO ray 0, then all of AO ray 1, ...; their number)"""
    from raytracing_amd.pyhost import render
    n = ps.total_rays
    rb, hb = ctx.buffer(n * 32), ctx.buffer(n * 32)
    gr = render.GranularRenderer(ctx, ps)   # its seeds are mirt_seed_fill(0, n, 0)'s, the ones the timed call reads
    try:
        ctx.view_rays(view, rb)
        ctx.trace_closest(dev.pass_desc(None, None), rb, n, hb, None)
        hits = hb.read(np.float32).reshape(-1, 8)
        pois = np.zeros(n, POI_DT)
        pois["normal"], pois["p"], pois["matId"] = hits[:, 0:3], hits[:, 4:7], np.ascontiguousarray(hits[:, 7]).view(np.int32)
        cast = pois["matId"] >= 0
        ncast = int(cast.sum())
        gr.b["pois"].write(pois)
        origin = (pois["p"][cast] + (pois["normal"][cast] * np.float32(BIAS)).astype(np.float32)).astype(np.float32)   # two fp32 operations
        del pois, hits
        out = ctx.buffer(max(ncast * SAMPLES * 32, 16))
        rec = np.zeros((ncast, 8), np.float32)
        rec[:, 0:3], rec[:, 7] = origin, np.float32(radius)
        for j in range(SAMPLES):
            gr.k["bouncePaths"].enqueue(gr.g1, [64])
            ctx.finish()
            rec[:, 4:7] = gr.read("rays").view(RAY_DT)["d"][cast]
            out.write(rec, offset=j * ncast * 32)
            log(f"  AO ray {j}: {ncast} rays in hand")
        return out, ncast * SAMPLES
    finally:
        gr.release()
        rb.release()
        hb.release()


def measure_one_launch(ctx, dev, ps, model, k, radius):
    from raytracing_amd.pyhost import mirt
    view = camera(mirt, ps, model, k)
    npix, nrays = ps.width * ps.height, ps.total_rays
    seeds, ao_out = ctx.buffer(nrays * 4), ctx.buffer(npix * 8)
    ctx.seed_fill(seeds, 0, nrays)
    d = dev.pass_desc(None, None)
    try:
        t = [timed(ctx, lambda: ctx.view_ao(d, view, seeds, ao_out, SAMPLES, radius, BIAS)) for _ in range(WARM + TIMED)]
        return {"one_launch_ms": round(statistics.median(t[WARM:]), 4), "one_launch_min_max": [round(min(t[WARM:]), 4), round(max(t[WARM:]), 4)],
                "view_ao_deferred_pixels": int(ctx.view_ao_deferred())}
    finally:
        seeds.release()
        ao_out.release()


def measure_view(ctx, dev, ps, model, k, radius, log):
    from raytracing_amd.pyhost import mirt
    view = camera(mirt, ps, model, k)
    npix, nrays = ps.width * ps.height, ps.total_rays
    rays, count = rays_in_hand(ctx, dev, ps, view, radius, log)
    seeds, ao_out = ctx.buffer(nrays * 4), ctx.buffer(npix * 8)
    nh, ad, occ = ctx.buffer(npix * 16), ctx.buffer(npix * 16), ctx.buffer(max(count, 16))
    ctx.seed_fill(seeds, 0, nrays)
    d = dev.pass_desc(None, None)
    try:
        one = lambda: ctx.view_ao(d, view, seeds, ao_out, SAMPLES, radius, BIAS)

        def by_hand():
            ctx.view_guides(d, view, nh, ad)
            ctx.trace_occluded(d, rays, count, occ)
        t_one, t_hand, t_guides = [], [], []
        for _ in range(WARM + TIMED):
            t_one.append(timed(ctx, one))
            t_hand.append(timed(ctx, by_hand))
            t_guides.append(timed(ctx, lambda: ctx.view_guides(d, view, nh, ad)))
        one()
        deferred = ctx.view_ao_deferred()
        by_hand()
        trace_deferred = ctx.trace_deferred()
        pairs = ao_out.read(np.uint32).reshape(-1, 2)
        open_rays = int((occ.read(np.uint8, count=count) == 0).sum())
        a, t, g = (statistics.median(x[WARM:]) for x in (t_one, t_hand, t_guides))
        mm = lambda x: [round(min(x[WARM:]), 4), round(max(x[WARM:]), 4)]
        open_sum, cast_sum = int(pairs[:, 0].astype(np.uint64).sum()), int(pairs[:, 1].astype(np.uint64).sum())
        return {"radius": radius, "samples": SAMPLES, "bias": BIAS, "pixels": npix, "view_rays": nrays, "ao_rays": count,
                "one_launch_ms": round(a, 4), "one_launch_min_max": mm(t_one),
                "guides_plus_occluded_ms": round(t, 4), "guides_plus_occluded_min_max": mm(t_hand), "guides_alone_ms": round(g, 4),
                "ratio_one_launch_over_guides_plus_occluded": round(a / t, 4), "one_launch_not_above": bool(a <= t),
                "view_ao_deferred_pixels": int(deferred), "view_ao_deferred_share": round(deferred / npix, 6), "trace_deferred_rays": int(trace_deferred),
                "M_ao_rays_per_s": round(count / a / 1e3, 1), "open": open_sum, "cast": cast_sum,
                "rays_in_hand_are_the_kernels": bool(cast_sum == count and open_sum == open_rays)}
    finally:
        for x in (rays, seeds, ao_out, nh, ad, occ):
            x.release()


def measure_thin_lens(ctx, dev, ps, radius):
    """mirt_render_ao of the scene's own thin-lens camera at the same size, for scale"""
    npix, nrays = ps.width * ps.height, ps.total_rays
    seeds, ao_out = ctx.buffer(nrays * 4), ctx.buffer(npix * 8)
    ctx.seed_fill(seeds, 0, nrays)
    d = dev.pass_desc(seeds, None)
    try:
        t = [timed(ctx, lambda: ctx.render_ao(d, ao_out, SAMPLES, radius, BIAS)) for _ in range(WARM + TIMED)]
        pairs = ao_out.read(np.uint32).reshape(-1, 2)
        return {"render_ao_ms": round(statistics.median(t[WARM:]), 4), "render_ao_min_max": [round(min(t[WARM:]), 4), round(max(t[WARM:]), 4)],
                "ao_rays": int(pairs[:, 1].astype(np.uint64).sum()), "ao_deferred_pixels": int(ctx.ao_deferred())}
    finally:
        seeds.release()
        ao_out.release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_ao", "timing.json"))
    ap.add_argument("--size", type=int, nargs=3, default=[1920, 1080, 2], metavar=("W", "H", "K"))
    ap.add_argument("--one-launch-only", action="store_true")
    args = ap.parse_args()
    log = lambda s: print(s, file=sys.stderr, flush=True)
    w, h, k = args.size
    graft.load_package()
    from raytracing_amd.pyhost import mirt, scene
    golden = os.path.join(ROOT, "tests", "golden")
    cornell = scene.PackedScene(open(os.path.join(golden, "scene_cornell_1920x1080_r256.json")).read()).resized(w, h, k * k)
    fx = np.load(os.path.join(golden, "cornell_teapot3_32x24_r4.npz"))
    teapot3 = scene.PackedScene(json.loads(bytes(fx["scene_json"]).decode())).resized(w, h, k * k)
    res = {"library": os.path.basename(mirt.LIB_PATH), "width": w, "height": h, "k": k, "warmups": WARM, "timed_calls": TIMED,
           "method": "medians of HIP-event times, mirt_view_ao and mirt_view_guides + mirt_trace_occluded alternating in one loop; two runs; the "
                     "baseline's AO rays are built before the loop and its time omits mirt_view_rays, their generation and the read-backs",
           "runs": []}
    ctx = mirt.Context(0)
    ctx.set_fusion(0)
    ok = True
    for run in range(2):
        rec = {}
        for name, ps in (("cornell", cornell), ("cornell_teapot3", teapot3)):
            b = np.asarray(ps.bounds, np.float64)
            radius = float(np.float32(0.25 * np.linalg.norm(b[4:7] - b[0:3])))
            dev = mirt.DeviceScene(ctx, ps)
            try:
                rec[name] = {}
                for model in CAMERAS:
                    log(f"run {run + 1} {name} {model}")
                    if args.one_launch_only:
                        rec[name][model] = measure_one_launch(ctx, dev, ps, model, k, radius)
                    else:
                        rec[name][model] = measure_view(ctx, dev, ps, model, k, radius, log)
                        ok = ok and rec[name][model]["rays_in_hand_are_the_kernels"]
                    log(json.dumps(rec[name][model]))
                if not args.one_launch_only:
                    rec[name]["thin_lens"] = measure_thin_lens(ctx, dev, ps, radius)
                    log(json.dumps(rec[name]["thin_lens"]))
            finally:
                dev.release()
        res["runs"].append(rec)
    ctx.destroy()
    if not args.one_launch_only:
        res["one_launch_not_above_in_both_runs"] = all(r[s][c]["one_launch_not_above"] for r in res["runs"] for s in r for c in CAMERAS)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
