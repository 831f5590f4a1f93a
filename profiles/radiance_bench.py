#!/usr/bin/env python3
"""profiles/radiance_bench.py [--out FILE.json] [--size W H RPP] [--quick] -- path radiance of caller-supplied rays in one launch
(mirt_trace_radiance) against the only route a caller had before it: the kernel-by-kernel enqueues of executeRender without initTrace and
copyToPixel, on the same rays.

  Scenes   cornell (single-cell sets) and cornell_teapot3 (two grid meshes) at 1920 x 1080 x 4 rays, bounces 5, samples 1.
  Rays     the camera's own, read from the Ray buffer an initTrace enqueue leaves and repacked to 32-byte records: COHERENT in that order, and
           the same rays PERMUTED (one seeded permutation: every wave holds rays from all over the image).
  Enqueues the kernel-by-kernel route on those rays: the 48-byte Ray buffer and the reset Poi buffer are written before the timed region (a caller
           has them on the device), then the closest-hit kernels, lightRender, the per-light block and five times bouncePaths, closest hit and
           the per-light block through mirt_enqueue, fusion off.  Its accumulators and seeds must equal the one launch's bit for bit (`equal`).
  Pass     mirt_render_first_pass with acu given on the same scene and size: the camera's rays made inside the launch.
  Samples  cornell_teapot3 and cornell, coherent rays, samples = 1, 4, 16: time per call and per sample.
  Method   one MI355X; medians of HIP-event times (mirt_timer_start / mirt_timer_stop_ms) after warm-ups; the one launch, the pass and the
           enqueues alternate in one loop; the whole measurement twice (`runs`).
  Condition: the one launch is faster than the enqueues in every row (`one_launch_faster`; exit status 3 where not, or where a row's results
           differ).  Everything else is recorded without a bound.
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
WARM_KBK, TIMED_KBK = 1, 3
BOUNCES = 5
RAY_DT = np.dtype({"names": ["o", "d", "mint", "maxt"], "formats": [(np.float32, 3), (np.float32, 3), np.float32, np.float32],
                   "offsets": [0, 16, 32, 36], "itemsize": 48})   # the kernels' 48-byte Ray
POI_DT = np.dtype({"names": ["p", "normal", "atte", "matId"], "formats": [(np.float32, 3), (np.float32, 3), (np.float32, 3), np.int32],
                   "offsets": [0, 16, 32, 48], "itemsize": 64})


def timed(ctx, call):
    ctx.finish()
    ctx.timer_start()
    call()
    return ctx.timer_stop_ms()


def med(x, warm):
    return round(statistics.median(x[warm:]), 4)


def span(x, warm):
    return [round(min(x[warm:]), 4), round(max(x[warm:]), 4)]


class Scene:
    """one scene on the context: the granular renderer (whose buffers the enqueue route runs on), the camera's rays, the call's buffers"""

    def __init__(self, ctx, ps):
        from raytracing_amd.pyhost import render
        self.ctx, self.ps, self.n = ctx, ps, ps.total_rays
        self.gr = render.GranularRenderer(ctx, ps)
        gr = self.gr
        gr.k["initTrace"].set_arg(4, ps.cam).enqueue(gr.gws["initTrace"], gr.lws["initTrace"])
        ctx.finish()
        self.ray48 = gr.read("rays").view(RAY_DT).copy()
        self.seeds0 = gr.read("seeds").copy()
        self.poi0 = np.zeros(self.n, POI_DT)
        self.poi0["matId"] = -1
        self.poi0["atte"] = 1.0
        self.rays, self.seeds, self.radiance = ctx.buffer(self.n * 32), ctx.buffer(self.n * 4), ctx.buffer(self.n * 16)
        self.desc = gr.dev.pass_desc(None, None, bounces=BOUNCES)

    def order(self, perm):
        """the rays (and their seeds) in the order `perm` (None: the camera's) into the call's ray buffer and the enqueue route's"""
        self.r48 = self.ray48 if perm is None else self.ray48[perm]
        self.s = self.seeds0 if perm is None else self.seeds0[perm]
        r = self.r48
        rec = np.zeros((self.n, 8), np.float32)
        rec[:, 0:3], rec[:, 3], rec[:, 4:7], rec[:, 7] = r["o"], r["mint"], r["d"], r["maxt"]
        self.rays.write(rec)

    def one_launch(self, samples=1):
        self.ctx.trace_radiance(self.desc, self.rays, self.n, self.seeds, self.radiance, samples=samples)

    def reset_enqueues(self):
        gr = self.gr
        gr.b["rays"].write(self.r48)
        gr.b["pois"].write(self.poi0)
        gr.b["seeds"].write(self.s)
        self.ctx.zero(gr.b["acu"])

    def enqueues(self):
        gr = self.gr
        gr._closest()
        for l in self.ps.lights:
            gr.k["lightRender"].set_arg(3, l["light"]).enqueue(gr.g1, [64])
        gr._direct()
        for _ in range(BOUNCES):
            gr.k["bouncePaths"].enqueue(gr.g1, [64])
            gr._closest()
            gr._direct()

    def release(self):
        for b in (self.rays, self.seeds, self.radiance):
            b.release()
        self.gr.release()


def measure(ctx, ps, log, quick):
    from raytracing_amd.pyhost import render
    sc = Scene(ctx, ps)
    fr = None if quick else render.FusedRenderer(ctx, ps, want_radiance=False)
    out = {"rays": sc.n, "bounces": BOUNCES}
    try:
        for label, perm in (("coherent", None), ("permuted", np.random.default_rng(11).permutation(sc.n))):
            sc.order(perm)
            t_one, t_kbk, t_pass = [], [], []
            for i in range(WARM + TIMED):
                sc.seeds.write(sc.s)
                t_one.append(timed(ctx, sc.one_launch))
                if quick:
                    continue
                if label == "coherent":
                    t_pass.append(timed(ctx, lambda: fr.execute_render(bounces=BOUNCES, fresh=True)))
                if i < WARM_KBK + TIMED_KBK:
                    sc.reset_enqueues()
                    t_kbk.append(timed(ctx, sc.enqueues))
            rec = {"one_launch_ms": med(t_one, WARM), "one_launch_min_max": span(t_one, WARM), "deferred_rays": int(ctx.radiance_deferred()),
                   "M_rays_per_s": round(sc.n / med(t_one, WARM) / 1e3, 1)}
            if not quick:
                # the last enqueue run and a one launch from the same seeds: the same accumulators and seeds
                sc.seeds.write(sc.s)
                sc.one_launch()
                equal = (sc.radiance.read(np.uint32).tobytes() == sc.gr.read("acu").view(np.uint32).tobytes()
                         and sc.seeds.read(np.int32).tobytes() == sc.gr.read("seeds").tobytes())
                rec.update({"enqueues_ms": med(t_kbk, WARM_KBK), "enqueues_min_max": span(t_kbk, WARM_KBK), "equal": bool(equal),
                            "ratio_enqueues_over_one_launch": round(med(t_kbk, WARM_KBK) / med(t_one, WARM), 2),
                            "one_launch_faster": bool(med(t_one, WARM) < med(t_kbk, WARM_KBK))})
                if t_pass:
                    rec.update({"first_pass_ms": med(t_pass, WARM), "first_pass_min_max": span(t_pass, WARM),
                                "ratio_one_launch_over_first_pass": round(med(t_one, WARM) / med(t_pass, WARM), 3)})
            out[label] = rec
            log(f"  {label}: {json.dumps(rec)}")
        if not quick:
            sc.order(None)
            out["samples"] = {}
            for samples in (1, 4, 16):
                t = []
                for _ in range(WARM + 5):
                    sc.seeds.write(sc.s)
                    t.append(timed(ctx, lambda: sc.one_launch(samples)))
                out["samples"][str(samples)] = {"call_ms": med(t, WARM), "per_sample_ms": round(med(t, WARM) / samples, 4)}
            log(f"  samples: {json.dumps(out['samples'])}")
        return out
    finally:
        if fr:
            fr.release()
        sc.release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radiance", "timing.json"))
    ap.add_argument("--size", type=int, nargs=3, default=[1920, 1080, 4], metavar=("W", "H", "RPP"))
    ap.add_argument("--quick", action="store_true")
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
           "enqueue_warmups": WARM_KBK, "enqueue_timed_runs": TIMED_KBK,
           "method": "medians of HIP-event times; mirt_trace_radiance, mirt_render_first_pass and the kernel-by-kernel enqueues alternating in one loop; "
                     "two runs; the enqueue route's Ray, Poi, seed and accumulator buffers are written before its timed region",
           "runs": []}
    ctx = mirt.Context(0)
    ctx.set_fusion(0)
    for run in range(1 if args.quick else 2):
        rec = {}
        for name, ps in (("cornell", cornell), ("cornell_teapot3", teapot3)):
            log(f"run {run + 1} {name}")
            rec[name] = measure(ctx, ps, log, args.quick)
        res["runs"].append(rec)
    ctx.destroy()
    if args.quick:
        print(json.dumps({"library": mirt.LIB_PATH, **{f"{s}_{o}": res["runs"][0][s][o]["one_launch_ms"] for s in res["runs"][0] for o in ("coherent", "permuted")}}))
        return 0
    rows = [r[s][o] for r in res["runs"] for s in r for o in ("coherent", "permuted")]
    res["one_launch_faster_in_every_row"] = all(x["one_launch_faster"] for x in rows)
    res["equal_in_every_row"] = all(x["equal"] for x in rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0 if res["one_launch_faster_in_every_row"] and res["equal_in_every_row"] else 3   # (1: an exception)


if __name__ == "__main__":
    sys.exit(main())
