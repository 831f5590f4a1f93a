#!/usr/bin/env python3
"""profiles/pass_guided_bench.py [out.json] -- what mirt_render_first_pass_guided saves over the two calls it stands for.

Per configuration (cornell.xml 1080p x 16, cornell.xml 1080p x 4, cornell_teapot3 1080p x 16; depth 8; the pass resolves its own pixels, no
per-ray accumulator), each variant between two HIP events (mirt_timer_start / mirt_timer_stop_ms), medians of 20 calls after 3 warm-ups, the
variants alternating inside one loop so that drift hits them alike.  Every variant has its own renderer, started from the same seeds:
  a  mirt_render_first_pass + mirt_render_guides
  b  mirt_render_first_pass_guided                 (left out when the loaded library lacks the entry point: a build of the parent commit,
                                                    MIRT_LIB_PATH -- its a and c are the comparison the unguided kernels must agree with)
  c  mirt_render_first_pass alone
saved = a - b; guides_cost = a - c (what the second trace costs), in_pass_cost = b - c (what writing the guides from the pass costs).
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
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pass_guided", "timing.json")
    graft.load_package()
    from raytracing_amd.pyhost import mirt, render, scene
    golden = os.path.join(ROOT, "tests", "golden")
    cornell = scene.PackedScene(open(os.path.join(golden, "scene_cornell_1920x1080_r256.json")).read())
    fx = np.load(os.path.join(golden, "cornell_teapot3_32x24_r4.npz"))
    teapot3 = scene.PackedScene(json.loads(bytes(fx["scene_json"]).decode()))
    configs = [("cornell", cornell, 16), ("cornell", cornell, 4), ("cornell_teapot3", teapot3, 16)]
    has_guided = hasattr(mirt.lib(), "mirt_render_first_pass_guided")
    ctx = mirt.Context(0)
    res = {"csrc_sha256": csrc_sha256() if not os.environ.get("MIRT_LIB_PATH") else None, "library": os.path.basename(mirt.LIB_PATH),
           "width": 1920, "height": 1080, "bounces": 8, "warm_ups": WARM, "timed_calls": TIMED, "configs": []}
    for name, base, rpp in configs:
        ps = base.resized(1920, 1080, rpp)
        npix = ps.width * ps.height
        variants = ["a", "b", "c"] if has_guided else ["a", "c"]
        fr = {v: render.FusedRenderer(ctx, ps, keep_acu=False, want_radiance=True, seed_base=1) for v in variants}
        nh = {v: ctx.buffer(npix * 16) for v in variants if v != "c"}
        ad = {v: ctx.buffer(npix * 16) for v in variants if v != "c"}
        desc = {v: fr[v].dev.pass_desc(fr[v].seeds, None, fr[v].pixel, fr[v].radiance, pass_index=1, bounces=8) for v in variants}

        def two_calls():
            ctx.render_pass(desc["a"], fresh=True)
            ctx.render_guides(desc["a"], nh["a"], ad["a"])
        calls = {"a": two_calls, "b": lambda: ctx.render_first_pass_guided(desc["b"], nh["b"], ad["b"]), "c": lambda: ctx.render_pass(desc["c"], fresh=True)}
        before = ctx.guided_passes() if has_guided else 0
        times = {v: [] for v in variants}
        for rep in range(WARM + TIMED):
            for v in variants:
                ms = timed(ctx, calls[v])
                if rep >= WARM:
                    times[v].append(ms)
        rec = {"scene": name, "rays_per_pixel": rpp}
        for v in variants:
            rec[f"{v}_ms"] = round(statistics.median(times[v]), 4)
            rec[f"{v}_min_max"] = [round(min(times[v]), 4), round(max(times[v]), 4)]
        rec["guides_cost_ms"] = round(rec["a_ms"] - rec["c_ms"], 4)
        if has_guided:
            rec["one_launch_route"] = ctx.guided_passes() - before == WARM + TIMED
            rec["saved_ms"] = round(rec["a_ms"] - rec["b_ms"], 4)
            rec["in_pass_cost_ms"] = round(rec["b_ms"] - rec["c_ms"], 4)
            same = all(np.array_equal(x["a"].read(np.uint32), x["b"].read(np.uint32)) for x in (nh, ad))
            rec["guides_identical"] = bool(same and np.array_equal(fr["a"].radiance.read(np.uint32), fr["b"].radiance.read(np.uint32)))
        res["configs"].append(rec)
        print(json.dumps(rec), flush=True)
        for b in list(nh.values()) + list(ad.values()):
            b.release()
        for r in fr.values():
            r.release()
    ctx.destroy()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
