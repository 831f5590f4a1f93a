#!/usr/bin/env python3
"""profiles/filter_bench.py [out.json] -- what one mirt_filter_atrous call costs beside one depth-8 pass and one mirt_render_guides call of the
same configuration, and which of the two kernel structures an iteration should run as.

Per configuration (cornell.xml 1080p x 16, cornell_teapot3 1080p x 16, cornell.xml 1080p x 4), on one context:
  * mirt_pass_timing of a depth-8 first pass that resolves its own pixels, median of 5 after 1 warm-up;
  * one mirt_render_guides call between two HIP events (mirt_timer_start / mirt_timer_stop_ms), median of 20 after 3 warm-ups;
  * one mirt_filter_atrous call (shipped parameters, filtered + pixel written) the same way for iterations 0 .. 5, with every iteration forced to
    the direct kernel, forced to the LDS-tile kernel, and as shipped; the three variants alternate inside one loop, so drift hits them alike.
    step_ms[s] = t(s + 1 iterations) - t(s iterations) is the cost of the iteration of step 2^s under that structure (the prepare kernel and
    the output writes are in both terms);
  * share = filter / (pass + guides + filter) for the shipped choice at every iteration count.
Writes the numbers with the hash of the kernel sources (the recipe of bench.py csrc_sha256)."""
import glob
import hashlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

WARM, TIMED = 3, 20


def csrc_sha256():
    h = hashlib.sha256()
    d = os.path.join(ROOT, "2015-raytracing_amd", "csrc")
    for f in sorted(glob.glob(os.path.join(d, "*.hip")) + glob.glob(os.path.join(d, "*.hpp")) + glob.glob(os.path.join(d, "*.cpp")) + glob.glob(os.path.join(d, "*.sh"))):
        h.update(os.path.basename(f).encode() + b"\0" + open(f, "rb").read())
    return h.hexdigest()


def timed(ctx, call):
    ctx.finish()
    ctx.timer_start()
    call()
    return ctx.timer_stop_ms()


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "filter", "timing.json")
    graft.load_package()
    from raytracing_amd.pyhost import mirt, render, scene
    golden = os.path.join(ROOT, "tests", "golden")
    cornell = scene.PackedScene(open(os.path.join(golden, "scene_cornell_1920x1080_r256.json")).read())
    fx = np.load(os.path.join(golden, "cornell_teapot3_32x24_r4.npz"))
    teapot3 = scene.PackedScene(json.loads(bytes(fx["scene_json"]).decode()))
    configs = [("cornell", cornell, 16), ("cornell_teapot3", teapot3, 16), ("cornell", cornell, 4)]
    ctx = mirt.Context(0)
    res = {"csrc_sha256": csrc_sha256(), "library": os.path.basename(mirt.LIB_PATH), "width": 1920, "height": 1080, "bounces": 8,
           "parameters": mirt.FILTER_DEFAULTS, "configs": []}
    for name, base, rpp in configs:
        ps = base.resized(1920, 1080, rpp)
        fr = render.FusedRenderer(ctx, ps, keep_acu=False, want_radiance=True)
        npix = ps.width * ps.height
        nh, ad, out, pix = ctx.buffer(npix * 16), ctx.buffer(npix * 16), ctx.buffer(npix * 16), ctx.buffer(npix * 4)
        d = fr.dev.pass_desc(None, None)
        rec = {"scene": name, "rays_per_pixel": rpp}
        ctx.set_profiling(True)
        t = []
        first = fr.dev.pass_desc(fr.seeds, None, fr.pixel, fr.radiance, pass_index=1, bounces=8)
        for i in range(6):
            ctx.render_pass(first, fresh=True)
            ctx.finish()
            t.append(ctx.pass_timing()[0])
        ctx.set_profiling(False)
        rec["pass_depth8_ms"] = round(statistics.median(t[1:]), 4)
        t = [timed(ctx, lambda: ctx.render_guides(d, nh, ad)) for _ in range(WARM + TIMED)]
        rec["guides_ms"] = round(statistics.median(t[WARM:]), 4)
        rec["live_pixels"] = round(float((nh.read(np.float32).reshape(-1, 4)[:, 3] > 0).mean()), 4)
        tone = np.float32(1.0 / rpp)
        variants = (("direct", "direct"), ("tiled", "tiled"), ("shipped", None))
        times = {v: [[] for _ in range(6)] for v, _ in variants}
        for rep in range(WARM + TIMED):
            for it in range(6):
                for v, structure in variants:
                    ms = timed(ctx, lambda: ctx.filter_atrous(ps.width, ps.height, tone, fr.radiance, nh, ad, filtered=out, pixel=pix, iterations=it, structure=structure))
                    if rep >= WARM:
                        times[v][it].append(ms)
        for v, _ in variants:
            med = [statistics.median(x) for x in times[v]]
            rec[f"filter_{v}_ms"] = [round(x, 4) for x in med]
            rec[f"filter_{v}_min_max"] = [[round(min(x), 4), round(max(x), 4)] for x in times[v]]
            rec[f"step_{v}_ms"] = [round(med[s + 1] - med[s], 4) for s in range(5)]
        base_ms = rec["pass_depth8_ms"] + rec["guides_ms"]
        rec["filter_share"] = [round(f / (base_ms + f), 4) for f in rec["filter_shipped_ms"]]
        rec["filter5_over_pass"] = round(rec["filter_shipped_ms"][5] / rec["pass_depth8_ms"], 4)
        res["configs"].append(rec)
        print(json.dumps(rec), flush=True)
        for b in (nh, ad, out, pix):
            b.release()
        fr.release()
    ctx.destroy()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
