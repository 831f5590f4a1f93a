#!/usr/bin/env python3
"""profiles/guides_bench.py [out.json] -- what one mirt_render_guides call costs beside one depth-8 pass of the same configuration.

Per configuration (cornell.xml 1080p x 16 and x 256, cornell_teapot3 1080p x 16): the time of one mirt_render_guides call between two HIP events
(mirt_timer_start / mirt_timer_stop_ms), median of 20 after 3 warm-ups, with the optimistic pair (the default) and with the exact kernel alone
(mirt_ctx_set_exact_only); and mirt_pass_timing of a depth-8 first pass that resolves its own pixels, median of 5 after 1 warm-up, on the same
build and context.  Writes the numbers with the hash of the kernel sources (the recipe of bench.py csrc_sha256)."""
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


def csrc_sha256():
    h = hashlib.sha256()
    d = os.path.join(ROOT, "2015-raytracing_amd", "csrc")
    for f in sorted(glob.glob(os.path.join(d, "*.hip")) + glob.glob(os.path.join(d, "*.hpp")) + glob.glob(os.path.join(d, "*.cpp")) + glob.glob(os.path.join(d, "*.sh"))):
        h.update(os.path.basename(f).encode() + b"\0" + open(f, "rb").read())
    return h.hexdigest()


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "guides", "timing.json")
    graft.load_package()
    from raytracing_amd.pyhost import mirt, render, scene
    golden = os.path.join(ROOT, "tests", "golden")
    cornell = scene.PackedScene(open(os.path.join(golden, "scene_cornell_1920x1080_r256.json")).read())
    fx = np.load(os.path.join(golden, "cornell_teapot3_32x24_r4.npz"))
    teapot3 = scene.PackedScene(json.loads(bytes(fx["scene_json"]).decode()))
    configs = [("cornell", cornell, 16), ("cornell", cornell, 256), ("cornell_teapot3", teapot3, 16)]
    ctx = mirt.Context(0)
    res = {"csrc_sha256": csrc_sha256(), "library": os.path.basename(mirt.LIB_PATH), "width": 1920, "height": 1080, "bounces": 8, "configs": []}
    for name, base, rpp in configs:
        ps = base.resized(1920, 1080, rpp)
        fr = render.FusedRenderer(ctx, ps, keep_acu=False, want_radiance=True)
        npix = ps.width * ps.height
        nh, ad = ctx.buffer(npix * 16), ctx.buffer(npix * 16)
        d = fr.dev.pass_desc(None, None)
        rec = {"scene": name, "rays_per_pixel": rpp}
        for key, exact in (("guides_ms", False), ("guides_exact_only_ms", True)):
            ctx.set_exact_only(exact)
            t = []
            for i in range(23):
                ctx.finish()
                ctx.timer_start()
                ctx.render_guides(d, nh, ad)
                t.append(ctx.timer_stop_ms())
            rec[key] = round(statistics.median(t[3:]), 4)
            rec[key + "_min_max"] = [round(min(t[3:]), 4), round(max(t[3:]), 4)]
        ctx.set_exact_only(False)
        hits = nh.read(np.float32).reshape(-1, 4)[:, 3]
        rec["mean_hits_per_pixel"] = round(float(hits.mean()), 3)
        ctx.set_profiling(True)
        t = []
        for i in range(6):
            fr.passes = 1
            fr.execute_render(bounces=8, fresh=True)
            ctx.finish()
            t.append(ctx.pass_timing()[0])
        ctx.set_profiling(False)
        rec["pass_depth8_ms"] = round(statistics.median(t[1:]), 4)
        rec["guides_over_pass"] = round(rec["guides_ms"] / rec["pass_depth8_ms"], 4)
        rec["exact_only_over_pair"] = round(rec["guides_exact_only_ms"] / rec["guides_ms"], 4)
        res["configs"].append(rec)
        print(json.dumps(rec), flush=True)
        for b in (nh, ad):
            b.release()
        fr.release()
    ctx.destroy()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
