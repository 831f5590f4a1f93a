#!/usr/bin/env python3
"""profiles/ao_bench.py [--out FILE.json] [--size W H RPP] -- ambient occlusion of the first hit in one launch (mirt_render_ao) against what a
caller pays today WITH THE AO RAYS ALREADY IN HAND: one mirt_render_guides call (the first hit) plus one mirt_trace_occluded call on the same AO rays.

  Scenes   cornell (single-cell sets) and cornell_teapot3 (two grid meshes) at 1920 x 1080 x 16, 4 AO rays per hit sample; radius: a quarter of
           the scene box's diagonal; bias 0.001.
  Rays     the baseline's AO rays are built once, outside the timed region, by the kernel-by-kernel composition the definition names: initTrace and
           the closest-hit kernels through mirt_enqueue, then bouncePaths x samples on the unchanged Poi buffer; after each the 48-byte rays of the
           casting samples are read back, rewritten on the host (origin p + n * bias, mint 0, maxt radius) and appended as 32-byte mirt_ray records.
           The baseline's time therefore OMITS the caller's ray generation, the read-backs and the rewrite.
  Check    the rays in hand are the kernel's: the not-occluded among them number what mirt_render_ao's `open` sums to, and there are `cast` of them.
  Method   one MI355X; per scene medians of 20 calls between two HIP events (mirt_timer_start / mirt_timer_stop_ms) after 3 warm-ups, the two
           variants alternating in one loop; the whole measurement twice (`runs`).
  Recorded without a bound: both medians, their min .. max, the ratio one_launch / (guides + occluded), mirt_ao_deferred, AO rays per second.
  Beside them, for scale: `generation_ms`, the DEVICE time alone of what the baseline omits and the one launch contains -- the closest-hit kernels
  that fill the Poi buffer are not in it, only the `samples` bouncePaths launches that make the rays (each timed between HIP events while the rays
  are being built; no read-back, no rewrite) -- and the ratio with it added to the baseline."""
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


def timed(ctx, call):
    ctx.finish()
    ctx.timer_start()
    call()
    return ctx.timer_stop_ms()


def rays_in_hand(ctx, ps, radius, log):
    """-> (a buffer of the casting samples' AO rays, 32 bytes each, sample-major: all of AO ray 0, then all of AO ray 1, ...; their number;
    the device time of the `samples` bouncePaths launches together, ms)"""
    from raytracing_amd.pyhost import render
    gr = render.GranularRenderer(ctx, ps)
    try:
        gr.k["initTrace"].set_arg(4, ps.cam).enqueue(gr.gws["initTrace"], gr.lws["initTrace"])
        gr._closest()
        ctx.finish()
        pois = gr.read("pois").view(POI_DT)
        cast = pois["matId"] >= 0
        ncast = int(cast.sum())
        p, nrm = pois["p"][cast].astype(np.float32), pois["normal"][cast].astype(np.float32)
        origin = (p + (nrm * np.float32(BIAS)).astype(np.float32)).astype(np.float32)   # two fp32 operations, as the definition has it
        del pois, p, nrm
        out = ctx.buffer(max(ncast * SAMPLES * 32, 16))
        rec = np.zeros((ncast, 8), np.float32)
        rec[:, 0:3], rec[:, 7] = origin, np.float32(radius)
        generation_ms = 0.0
        for j in range(SAMPLES):
            generation_ms += timed(ctx, lambda: gr.k["bouncePaths"].enqueue(gr.g1, [64]))
            ctx.finish()
            rec[:, 4:7] = gr.read("rays").view(RAY_DT)["d"][cast]
            out.write(rec, offset=j * ncast * 32)
            log(f"  AO ray {j}: {ncast} rays in hand")
        return out, ncast * SAMPLES, generation_ms
    finally:
        gr.release()


def measure(ctx, ps, log):
    from raytracing_amd.pyhost import mirt
    b = np.asarray(ps.bounds, np.float64)
    radius = float(np.float32(0.25 * np.linalg.norm(b[4:7] - b[0:3])))
    npix, nrays = ps.width * ps.height, ps.total_rays
    rays, count, generation_ms = rays_in_hand(ctx, ps, radius, log)
    dev = mirt.DeviceScene(ctx, ps)
    seeds, ao_out = ctx.buffer(nrays * 4), ctx.buffer(npix * 8)
    nh, ad, occ = ctx.buffer(npix * 16), ctx.buffer(npix * 16), ctx.buffer(max(count, 16))
    ctx.seed_fill(seeds, 0, nrays)
    d_ao, d_guides = dev.pass_desc(seeds, None), dev.pass_desc(None, None)
    try:
        one = lambda: ctx.render_ao(d_ao, ao_out, SAMPLES, radius, BIAS)

        def today():
            ctx.render_guides(d_guides, nh, ad)
            ctx.trace_occluded(d_guides, rays, count, occ)
        t_one, t_today, t_guides = [], [], []
        for _ in range(WARM + TIMED):
            t_one.append(timed(ctx, one))
            t_today.append(timed(ctx, today))
            t_guides.append(timed(ctx, lambda: ctx.render_guides(d_guides, nh, ad)))
        one()
        deferred = ctx.ao_deferred()
        today()
        trace_deferred = ctx.trace_deferred()
        pairs = ao_out.read(np.uint32).reshape(-1, 2)
        open_rays = int((occ.read(np.uint8, count=count) == 0).sum())
        a, t, g = (statistics.median(x[WARM:]) for x in (t_one, t_today, t_guides))
        mm = lambda x: [round(min(x[WARM:]), 4), round(max(x[WARM:]), 4)]
        return {"radius": radius, "samples": SAMPLES, "bias": BIAS, "pixels": npix, "primary_rays": nrays, "ao_rays": count,
                "one_launch_ms": round(a, 4), "one_launch_min_max": mm(t_one),
                "guides_plus_occluded_ms": round(t, 4), "guides_plus_occluded_min_max": mm(t_today), "guides_alone_ms": round(g, 4),
                "ratio_one_launch_over_guides_plus_occluded": round(a / t, 4), "one_launch_not_above": bool(a <= t),
                "generation_ms": round(generation_ms, 4), "ratio_one_launch_over_guides_plus_occluded_plus_generation": round(a / (t + generation_ms), 4),
                "ao_deferred_pixels": int(deferred), "ao_deferred_share": round(deferred / npix, 6), "trace_deferred_rays": int(trace_deferred),
                "M_ao_rays_per_s": round(count / a / 1e3, 1),
                "open": int(pairs[:, 0].astype(np.uint64).sum()), "cast": int(pairs[:, 1].astype(np.uint64).sum()),
                "rays_in_hand_are_the_kernels": bool(int(pairs[:, 1].astype(np.uint64).sum()) == count and int(pairs[:, 0].astype(np.uint64).sum()) == open_rays)}
    finally:
        for x in (rays, seeds, ao_out, nh, ad, occ):
            x.release()
        dev.release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ao", "timing.json"))
    ap.add_argument("--size", type=int, nargs=3, default=[1920, 1080, 16], metavar=("W", "H", "RPP"))
    args = ap.parse_args()
    log = lambda s: print(s, file=sys.stderr, flush=True)
    w, h, rpp = args.size
    graft.load_package()
    from raytracing_amd.pyhost import mirt, scene
    golden = os.path.join(ROOT, "tests", "golden")
    cornell = scene.PackedScene(open(os.path.join(golden, "scene_cornell_1920x1080_r256.json")).read()).resized(w, h, rpp)
    fx = np.load(os.path.join(golden, "cornell_teapot3_32x24_r4.npz"))
    teapot3 = scene.PackedScene(json.loads(bytes(fx["scene_json"]).decode())).resized(w, h, rpp)
    res = {"library": os.path.basename(mirt.LIB_PATH), "width": w, "height": h, "rays_per_pixel": rpp, "warmups": WARM, "timed_calls": TIMED,
           "method": "medians of HIP-event times, mirt_render_ao and mirt_render_guides + mirt_trace_occluded alternating in one loop; two runs; the "
                     "baseline's AO rays are built before the loop and its time omits their generation and read-backs",
           "runs": []}
    ctx = mirt.Context(0)
    ctx.set_fusion(0)
    ok = True
    for run in range(2):
        rec = {}
        for name, ps in (("cornell", cornell), ("cornell_teapot3", teapot3)):
            log(f"run {run + 1} {name}")
            rec[name] = measure(ctx, ps, log)
            log(json.dumps(rec[name]))
            ok = ok and rec[name]["rays_in_hand_are_the_kernels"]
        res["runs"].append(rec)
    ctx.destroy()
    res["one_launch_not_above_in_both_runs"] = all(r[s]["one_launch_not_above"] for r in res["runs"] for s in r)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
