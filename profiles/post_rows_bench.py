#!/usr/bin/env python3
"""profiles/post_rows_bench.py [parent-libmirt.so] -> profiles/post_rows/timing.json -- what the post-process stage in row tiles costs, on one
context: cornell.xml at 1920 x 1080 x 4 rays, shipped parameters, every call between two HIP events (mirt_timer_start / mirt_timer_stop_ms),
medians of 20 calls after 3 warm-ups, the variants alternating inside one loop so that drift hits them alike.

  (a) mirt_filter_atrous (3 and 5 iterations) and mirt_upsample_guided (factor 2, 960 x 540 -> 1920 x 1080) of this tree against the parent
      commit's library (profiles/tools/build_at.sh <commit> <out.so>), measured in child processes of this one run -- a process loads one libmirt
      -- in the order parent, this tree, parent.  Verdict: this tree's median lies inside the min .. max of the parent's calls.
  (b) the _rows calls on the whole frame as one tile, in the same loop as (a)'s calls of this tree.
  (c) the middle tile of 8 (135 rows) beside one eighth of (a): the filter at 3 iterations (halo 14) and at 5 (halo 62), with the shrinking band
      and without it (MIRT_FILTER_ROWS_BAND=0), and the upsampler.
  (d) computed, not measured: bytes into the root and bytes exchanged per device at 8 tiles, for the gather-everything route and for this one.
Nothing here runs on more than one device: scaling over distinct devices remains unmeasured."""
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

WARM, TIMED = 3, 20
W, H, RPP, F, TILES = 1920, 1080, 4, 2, 8


def stats(times):
    t = times[WARM:]
    return {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}


def measure(rows_too):
    """one process, one library: the inputs once, then every variant in one loop"""
    graft.load_package()
    from raytracing_amd.pyhost import mirt, render, scene
    ps = scene.PackedScene(open(os.path.join(ROOT, "tests", "golden", "scene_cornell_1920x1080_r256.json")).read())
    ctx = mirt.Context(0)
    hi, lo = ps.resized(W, H, RPP), ps.resized(W // F, H // F, RPP)
    fh, fl = render.FusedRenderer(ctx, hi, seed_base=3), render.FusedRenderer(ctx, lo, seed_base=3)
    fh.execute_render_guided()
    fl.execute_render_guided()
    tone = np.float32(1.0 / RPP)
    npix = W * H
    out, pix = ctx.buffer(npix * 16), ctx.buffer(npix * 4)
    variants = {
        "filter_3": lambda: ctx.filter_atrous(W, H, tone, fh.radiance, fh.normal_hits, fh.albedo_depth, filtered=out, pixel=pix, iterations=3),
        "filter_5": lambda: ctx.filter_atrous(W, H, tone, fh.radiance, fh.normal_hits, fh.albedo_depth, filtered=out, pixel=pix, iterations=5),
        "upsample_2": lambda: ctx.upsample_guided(W, H, F, tone, fl.radiance, fl.normal_hits, fl.albedo_depth, fh.normal_hits, fh.albedo_depth, upsampled=out, pixel=pix),
    }
    env = {}
    if rows_too:
        q, r = divmod(H, TILES)
        t = TILES // 2 - 1
        own = (t * q + min(t, r), q + (1 if t < r else 0))
        cut = lambda b, w, r0, nr: ctx.buffer_from(np.ascontiguousarray(b.read(np.float32).reshape(-1, w, 4)[r0:r0 + nr]), mirt.MEM_READ_WRITE)
        for it in (3, 5):
            variants[f"filter_rows_whole_{it}"] = (lambda it=it: ctx.filter_atrous_rows(W, H, 0, H, 0, H, tone, fh.radiance, fh.normal_hits, fh.albedo_depth,
                                                                                        filtered=out, pixel=pix, iterations=it))
            win = mirt.filter_window_rows(H, own[0], own[1], it)
            ins = [cut(b, W, *win) for b in (fh.radiance, fh.normal_hits, fh.albedo_depth)]
            call = (lambda it=it, win=win, ins=ins: ctx.filter_atrous_rows(W, H, win[0], win[1], own[0], own[1], tone, *ins, filtered=out, pixel=pix, iterations=it))
            variants[f"filter_rows_tile_{it}_band"] = call
            variants[f"filter_rows_tile_{it}_whole_window"] = call
            env[f"filter_rows_tile_{it}_whole_window"] = "0"
        variants["upsample_rows_whole_2"] = lambda: ctx.upsample_guided_rows(W, H, F, 0, H, 0, H // F, tone, fl.radiance, fl.normal_hits, fl.albedo_depth,
                                                                             fh.normal_hits, fh.albedo_depth, upsampled=out, pixel=pix)
        low = mirt.upsample_low_rows(H, F, *own)
        lo_ins = [cut(b, W // F, *low) for b in (fl.radiance, fl.normal_hits, fl.albedo_depth)]
        hi_ins = [cut(b, W, *own) for b in (fh.normal_hits, fh.albedo_depth)]
        variants["upsample_rows_tile_2"] = lambda: ctx.upsample_guided_rows(W, H, F, own[0], own[1], low[0], low[1], tone, *lo_ins, *hi_ins, upsampled=out, pixel=pix)
    times = {k: [] for k in variants}
    for _ in range(WARM + TIMED):
        for k, call in variants.items():
            if k in env:
                os.environ["MIRT_FILTER_ROWS_BAND"] = env[k]
            ctx.finish()
            ctx.timer_start()
            call()
            times[k].append(ctx.timer_stop_ms())
            os.environ.pop("MIRT_FILTER_ROWS_BAND", None)
    res = {"library": os.path.basename(mirt.LIB_PATH), "calls": {k: stats(v) for k, v in times.items()}}
    ctx.destroy()
    return res


def child(lib, rows_too):
    env = dict(os.environ)
    env.pop("MIRT_LIB_PATH", None)
    if lib:
        env["MIRT_LIB_PATH"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--measure", "1" if rows_too else "0"], env=env, stdout=subprocess.PIPE, text=True, timeout=420)
    if r.returncode != 0:
        raise SystemExit(f"the measuring process for {lib or 'this tree'} ended with {r.returncode}")
    return json.loads(r.stdout.splitlines()[-1])


def tile_rows(height, n, i):
    """mirt_tile_rows's rule"""
    q, r = divmod(height, n)
    return i * q + min(i, r), q + (1 if i < r else 0)


def traffic():
    """(d) bytes at 8 tiles of 1920 x 1080, 3 iterations, from the row arithmetic alone (include/mirt.h): what reaches the root, and what each device
    receives from other devices -- the rows of its window that it does not own"""
    npix, row, low_row, hl = W * H, W * 16, (W // F) * 16, H // F
    halo = 2 * (2 ** 3 - 1)
    foreign = lambda own, win: sum(1 for r in range(win[0], win[0] + win[1]) if not own[0] <= r < own[0] + own[1])
    fil, ups = [], []
    for t in range(TILES):
        own = tile_rows(H, TILES, t)
        fil.append(foreign(own, (max(0, own[0] - halo), min(H, own[0] + own[1] + halo) - max(0, own[0] - halo))) * 3 * row)
        y0 = lambda y: (2 * y + 1 - F) // (2 * F)
        lo = max(0, y0(own[0]))
        ups.append(foreign(tile_rows(hl, TILES, t), (lo, min(hl, y0(own[0] + own[1] - 1) + 2) - lo)) * 3 * low_row)
    return {
        "tiles": TILES, "iterations": 3,
        "denoise_gather_route_bytes_into_root": npix * (4 + 16 + 16 + 16), "denoise_gather_route_bytes_per_pixel": 52,
        "denoise_tiles_route_bytes_into_root_pixel_only": npix * 4, "denoise_tiles_route_bytes_into_root_with_filtered": npix * 20,
        "denoise_tiles_route_halo_bytes_received_per_device": fil,
        "upscale_tiles_route_bytes_into_root_pixel_only": npix * 4, "upscale_tiles_route_bytes_into_root_with_upsampled": npix * 20,
        "upscale_tiles_route_low_window_bytes_received_per_device": ups,
        "note": "a window's own rows are a device-local copy and are not counted; with --denoise before the upscale the filter's halo of the LOW frame comes on top",
    }


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--measure":
        print(json.dumps(measure(sys.argv[2] == "1")), flush=True)
        return
    parent = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else None
    res = {"width": W, "height": H, "rays_per_pixel": RPP, "factor": F, "warmups": WARM, "timed": TIMED, "runs": []}
    if parent:
        res["runs"].append(dict(child(parent, False), role="parent"))
    res["runs"].append(dict(child(None, True), role="this tree"))
    if parent:
        res["runs"].append(dict(child(parent, False), role="parent, again"))
        new = res["runs"][1]["calls"]
        verdict = {}
        for k in ("filter_3", "filter_5", "upsample_2"):
            lo = min(r["calls"][k]["min_ms"] for r in res["runs"] if r["role"] != "this tree")
            hi = max(r["calls"][k]["max_ms"] for r in res["runs"] if r["role"] != "this tree")
            verdict[k] = {"this_tree_median_ms": new[k]["median_ms"], "parent_min_ms": lo, "parent_max_ms": hi, "inside": lo <= new[k]["median_ms"] <= hi}
        res["existing_calls_against_parent"] = verdict
    new = res["runs"][1 if parent else 0]["calls"]
    res["tile_of_8_against_an_eighth"] = {k: {"tile_ms": new[k]["median_ms"], "eighth_of_whole_ms": round(new[whole]["median_ms"] / TILES, 4)}
                                          for k, whole in (("filter_rows_tile_3_band", "filter_3"), ("filter_rows_tile_3_whole_window", "filter_3"),
                                                           ("filter_rows_tile_5_band", "filter_5"), ("filter_rows_tile_5_whole_window", "filter_5"),
                                                           ("upsample_rows_tile_2", "upsample_2"))}
    res["traffic_computed"] = traffic()
    res["not_measured"] = "everything ran on one device: scaling over distinct devices, and the exchange between them, remain unmeasured"
    out = os.path.join(ROOT, "profiles", "post_rows", "timing.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("existing_calls_against_parent", "tile_of_8_against_an_eighth") if k in res}, indent=1))


if __name__ == "__main__":
    main()
