#!/usr/bin/env python3
"""profiles/upsample_bench.py [out.json] -- what shading at 1/f resolution and upsampling (mirt_upsample_guided) costs beside the full-resolution
chain it replaces, at 1920x1080, depth 8, 16 rays per traced pixel, on cornell and cornell_teapot3, f = 2 and 4.

Per configuration, on one context, each sequence between two HIP events (mirt_timer_start / mirt_timer_stop_ms), medians of 20 calls after 3
warm-ups, the three variants alternating inside one loop so that drift hits them alike (the method of profiles/filter_bench.py):
  (a) full   the 1920x1080 pass (a first pass that resolves its own pixels), mirt_render_guides, mirt_filter_atrous (shipped parameters);
  (b) low    the (1920 / f) x (1080 / f) pass, its guides, the filter of the low frame, the guides at 1920x1080, the upsampler;
  (c) the upsampler alone, on (b)'s buffers.
Reported: (b) / (a) and the upsampler's share of (b).  Writes the numbers with the hash of the kernel sources (the recipe of bench.py csrc_sha256)."""
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
W, H, RPP, BOUNCES = 1920, 1080, 16, 8


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
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "upsample", "timing.json")
    graft.load_package()
    from raytracing_amd.pyhost import mirt, render, scene
    golden = os.path.join(ROOT, "tests", "golden")
    cornell = scene.PackedScene(open(os.path.join(golden, "scene_cornell_1920x1080_r256.json")).read())
    fx = np.load(os.path.join(golden, "cornell_teapot3_32x24_r4.npz"))
    teapot3 = scene.PackedScene(json.loads(bytes(fx["scene_json"]).decode()))
    ctx = mirt.Context(0)
    res = {"csrc_sha256": csrc_sha256(), "library": os.path.basename(mirt.LIB_PATH), "width": W, "height": H, "rays_per_traced_pixel": RPP, "bounces": BOUNCES,
           "filter_parameters": mirt.FILTER_DEFAULTS, "upsample_parameters": mirt.UPSAMPLE_DEFAULTS, "warm_ups": WARM, "timed_calls": TIMED, "configs": []}
    tone = np.float32(1.0 / RPP)
    for name, base in (("cornell", cornell), ("cornell_teapot3", teapot3)):
        hi = base.resized(W, H, RPP)
        full = render.FusedRenderer(ctx, hi, keep_acu=False, want_radiance=True)
        npix = W * H
        nh, ad, out, pix = ctx.buffer(npix * 16), ctx.buffer(npix * 16), ctx.buffer(npix * 16), ctx.buffer(npix * 4)
        d_full = full.dev.pass_desc(full.seeds, None, full.pixel, full.radiance, pass_index=1, bounces=BOUNCES)
        g_full = full.dev.pass_desc(None, None)

        def chain_full():
            ctx.render_pass(d_full, fresh=True)
            ctx.render_guides(g_full, nh, ad)
            ctx.filter_atrous(W, H, tone, full.radiance, nh, ad, filtered=out, pixel=pix)

        for f in (2, 4):
            wl, hl = W // f, H // f
            low = render.FusedRenderer(ctx, base.resized(wl, hl, RPP), keep_acu=False, want_radiance=True)
            nlo = wl * hl
            nh_lo, ad_lo, fil = ctx.buffer(nlo * 16), ctx.buffer(nlo * 16), ctx.buffer(nlo * 16)
            d_low = low.dev.pass_desc(low.seeds, None, low.pixel, low.radiance, pass_index=1, bounces=BOUNCES)
            g_low = low.dev.pass_desc(None, None)

            def upsampler():
                ctx.upsample_guided(W, H, f, tone, fil, nh_lo, ad_lo, nh, ad, upsampled=out, pixel=pix)

            def chain_low():
                ctx.render_pass(d_low, fresh=True)
                ctx.render_guides(g_low, nh_lo, ad_lo)
                ctx.filter_atrous(wl, hl, tone, low.radiance, nh_lo, ad_lo, filtered=fil)
                ctx.render_guides(g_full, nh, ad)
                upsampler()

            variants = (("full", chain_full), ("low", chain_low), ("upsampler", upsampler))
            times = {v: [] for v, _ in variants}
            for rep in range(WARM + TIMED):
                for v, call in variants:
                    ms = timed(ctx, call)
                    if rep >= WARM:
                        times[v].append(ms)
            med = {v: statistics.median(t) for v, t in times.items()}
            rec = {"scene": name, "factor": f, "low_width": wl, "low_height": hl,
                   "full_chain_ms": round(med["full"], 4), "low_chain_ms": round(med["low"], 4), "upsampler_ms": round(med["upsampler"], 4),
                   "min_max": {v: [round(min(t), 4), round(max(t), 4)] for v, t in times.items()},
                   "low_over_full": round(med["low"] / med["full"], 4), "upsampler_share_of_low_chain": round(med["upsampler"] / med["low"], 4),
                   "live_pixels": round(float((nh.read(np.float32).reshape(-1, 4)[:, 3] > 0).mean()), 4)}
            res["configs"].append(rec)
            print(json.dumps(rec), flush=True)
            for b in (nh_lo, ad_lo, fil):
                b.release()
            low.release()
        for b in (nh, ad, out, pix):
            b.release()
        full.release()
    ctx.destroy()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
