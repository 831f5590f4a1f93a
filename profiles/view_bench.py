#!/usr/bin/env python3
"""profiles/view_bench.py [--out FILE.json] [--size W H K] [--quick] -- a frame of a panoramic or orthographic camera in one launch
(mirt_render_view) against the three calls it replaces on the same rays: mirt_view_rays (32 B per ray written), mirt_trace_radiance (the rays
read, 16 B per ray of accumulators written) and an enqueued copyToPixel (the accumulators read).

  Scenes   cornell (single-cell sets) and cornell_teapot3 (two grid meshes) at 1920 x 1080, k = 2 (4 rays per pixel), bounces 5.
  Cameras  EQUIRECT from the scene box's centre, and ORTHOGRAPHIC with the oblique basis forward = normalize(0.3, -0.2, -1), right =
           normalize(forward x (0, 1, 0)), up = right x forward, the window 0.8 x the box's extents in x and y.
  Compose  the three calls queued back to back; their pixels and seeds must equal the one launch's bit for bit (`equal`).
  Pass     for scale only: mirt_render_first_pass of the scene's own thin-lens camera at the same size and ray count, resolving its own pixels.
  Method   one MI355X; medians of HIP-event times (mirt_timer_start / mirt_timer_stop_ms) after warm-ups; the one launch, the composition and
           the pass alternate in one loop; the whole measurement twice (`runs`), whose spread per case is the margin (`spread_ms`).
  Condition: the one launch is not slower than the composition on any case, beyond the spread of the two runs of that case
           (`one_launch_not_slower`; exit status 3 where not, or where a case's results differ).  Everything else is recorded without a bound.
--quick: the one-launch medians alone, printed as one JSON line (an A/B of two builds runs it once per library, MIRT_LIB_PATH naming each)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

WARM, TIMED = 2, 9
BOUNCES = 5


def timed(ctx, call):
    ctx.finish()
    ctx.timer_start()
    call()
    return ctx.timer_stop_ms()


def med(x):
    return round(statistics.median(x[WARM:]), 4)


def span(x):
    return [round(min(x[WARM:]), 4), round(max(x[WARM:]), 4)]


def views(mirt, ps, w, h, k):
    b = np.asarray(ps.bounds, np.float64)
    lo, hi = b[0:3], b[4:7]
    eye = (lo + hi) / 2
    tone = 1.0 / (k * k)
    equirect = mirt.view_desc("equirect", w, h, k=k, eye=eye, look_at=eye + [0.0, 0.0, -1.0], tone=tone)
    half = 0.8 * (hi - lo) / 2
    ortho = mirt.view_desc("ortho", w, h, k=k, eye=eye, look_at=eye + [0.3, -0.2, -1.0], half_w=half[0], half_h=half[1], tone=tone)
    return (("equirect", equirect), ("ortho_oblique", ortho))


def measure(ctx, mirt, ps, w, h, k, log, quick):
    from raytracing_amd.pyhost import render
    n_pix, n = w * h, w * h * k * k
    dev = mirt.DeviceScene(ctx, ps)
    desc = dev.pass_desc(None, None, bounces=BOUNCES)
    seeds0 = (np.arange(n, dtype=np.int64) * 7919 + 12345).astype(np.int32)   # (wraps: any int32 is a seed)
    seeds, radiance, pixel = ctx.buffer(n * 4), ctx.buffer(n_pix * 16), ctx.buffer(n_pix * 4)
    rays, acc, seeds2, pixel2 = (None,) * 4
    fr = None
    if not quick:
        rays, acc, seeds2, pixel2 = ctx.buffer(n * 32), ctx.buffer(n * 16), ctx.buffer(n * 4), ctx.buffer(n_pix * 4)
        copy = ctx.kernel("copyToPixel").set_args(pixel2, acc, np.array([1.0 / (k * k)], np.float32), np.array([n_pix], np.uint32), np.array([k * k], np.uint32))
        gws = [-(-n_pix // 64) * 64]
        fr = render.FusedRenderer(ctx, ps, keep_acu=False)
    out = {"rays": n, "bounces": BOUNCES}
    try:
        for label, view in views(mirt, ps, w, h, k):
            def one_launch():
                ctx.render_view(desc, view, seeds, radiance, pixel)

            def composition():
                ctx.view_rays(view, rays)
                ctx.trace_radiance(desc, rays, n, seeds2, acc, samples=1)
                copy.enqueue(gws, [64])

            t_one, t_cmp, t_pass = [], [], []
            for _ in range(WARM + TIMED):
                seeds.write(seeds0)
                t_one.append(timed(ctx, one_launch))
                if quick:
                    continue
                seeds2.write(seeds0)
                t_cmp.append(timed(ctx, composition))
                t_pass.append(timed(ctx, lambda: fr.execute_render(bounces=BOUNCES, fresh=True)))
            rec = {"one_launch_ms": med(t_one), "one_launch_min_max": span(t_one), "deferred_rays": int(ctx.view_deferred()),
                   "M_rays_per_s": round(n / med(t_one) / 1e3, 1)}
            if not quick:
                equal = pixel.read(np.uint8).tobytes() == pixel2.read(np.uint8).tobytes() and seeds.read(np.int32).tobytes() == seeds2.read(np.int32).tobytes()
                rec.update({"composition_ms": med(t_cmp), "composition_min_max": span(t_cmp), "equal": bool(equal),
                            "ratio_composition_over_one_launch": round(med(t_cmp) / med(t_one), 3),
                            "first_pass_ms": med(t_pass), "ratio_one_launch_over_first_pass": round(med(t_one) / med(t_pass), 3)})
            out[label] = rec
            log(f"  {label}: {json.dumps(rec)}")
        return out
    finally:
        if fr:
            fr.release()
        for b in (seeds, radiance, pixel, rays, acc, seeds2, pixel2):
            if b is not None:
                b.release()
        dev.release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view", "timing.json"))
    ap.add_argument("--size", type=int, nargs=3, default=[1920, 1080, 2], metavar=("W", "H", "K"))
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    log = lambda s: print(s, file=sys.stderr, flush=True)
    w, h, k = args.size
    graft.load_package()
    from raytracing_amd.pyhost import mirt, scene
    golden = os.path.join(ROOT, "tests", "golden")
    cornell = scene.PackedScene(open(os.path.join(golden, "scene_cornell_1920x1080_r256.json")).read()).resized(w, h, k * k)
    fx = np.load(os.path.join(golden, "cornell_teapot3_32x24_r4.npz"))
    teapot3 = scene.PackedScene(json.loads(bytes(fx["scene_json"]).decode())).resized(w, h, k * k)
    res = {"library": os.path.basename(mirt.LIB_PATH), "width": w, "height": h, "k": k, "rays_per_pixel": k * k, "warmups": WARM, "timed_calls": TIMED,
           "method": "medians of HIP-event times; mirt_render_view, the composition (mirt_view_rays + mirt_trace_radiance + an enqueued copyToPixel) and "
                     "mirt_render_first_pass alternating in one loop; two runs, whose spread per case is the margin",
           "runs": []}
    ctx = mirt.Context(0)
    ctx.set_fusion(0)
    for run in range(1 if args.quick else 2):
        rec = {}
        for name, ps in (("cornell", cornell), ("cornell_teapot3", teapot3)):
            log(f"run {run + 1} {name}")
            rec[name] = measure(ctx, mirt, ps, w, h, k, log, args.quick)
        res["runs"].append(rec)
    ctx.destroy()
    cases = [(s, c) for s in res["runs"][0] for c in ("equirect", "ortho_oblique")]
    if args.quick:
        print(json.dumps({"library": mirt.LIB_PATH, **{f"{s}_{c}": res["runs"][0][s][c]["one_launch_ms"] for s, c in cases}}))
        return 0
    res["cases"] = {}
    for s, c in cases:
        a, b = (r[s][c] for r in res["runs"])
        spread = round(max(abs(a["one_launch_ms"] - b["one_launch_ms"]), abs(a["composition_ms"] - b["composition_ms"])), 4)
        one, cmp_ = max(a["one_launch_ms"], b["one_launch_ms"]), min(a["composition_ms"], b["composition_ms"])
        res["cases"][f"{s}_{c}"] = {"one_launch_ms": [a["one_launch_ms"], b["one_launch_ms"]], "composition_ms": [a["composition_ms"], b["composition_ms"]],
                                    "spread_ms": spread, "one_launch_not_slower": bool(one <= cmp_ + spread), "equal": bool(a["equal"] and b["equal"])}
    res["one_launch_not_slower_on_every_case"] = all(x["one_launch_not_slower"] for x in res["cases"].values())
    res["equal_on_every_case"] = all(x["equal"] for x in res["cases"].values())
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0 if res["one_launch_not_slower_on_every_case"] and res["equal_on_every_case"] else 3   # (1: an exception)


if __name__ == "__main__":
    sys.exit(main())
