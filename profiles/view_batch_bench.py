#!/usr/bin/env python3
"""profiles/view_batch_bench.py [parent-libmirt.so] [--out FILE.json] [--frames N] -- the frames of N small view cameras in ONE call
(mirt_render_view_batch) beside the N single calls they equal, on the same library.

  Set-up   1024 EQUIRECT cameras (basis +x, +y, -z) on a 16 x 8 x 8 lattice inside the scene box, from 0.15 to 0.85 of each extent; 32 x 16,
           k = 2 (2048 rays a frame, 2.1 M in all), bounces 5; scenes cornell (single-cell sets) and cornell_teapot3 (two grid meshes).
  Calls    (a) batch_ms    one mirt_render_view_batch of the 1024 frames;
           (b) singles_ms  the 1024 mirt_render_view calls, frame f on wrapped slices of the same buffers;
           (c) tall_ms     one mirt_render_view of a 32 x 16384 image: the same ray count and ONE camera -- what the table's upload, the
                           per-lane cameras and the less coherent blocks cost is (a) - (c);
               upload_ms   for the first of those three: mirt_view_rays_batch of 1024 frames of 1 x 1 at k = 1, i.e. the upload's launches
                           and one kernel of 4 blocks -- an upper bound of what the upload adds to (a);
           each between two HIP events (`device`) and, around the same span, on the host's clock from before the first call until
           mirt_finish returns (`host`).  The three alternate in one loop behind the upload of the same seeds; behind the loop, un-timed,
           (a) and (b) must leave the same bytes in seeds, radiance and pixel (`equal`).
  Parent   (d) mirt_render_view at 1920 x 1080, k = 2 (profiles/view_bench.py --quick: the median of 9 calls after 2 warm-ups per case) in child
           processes -- a process loads one libmirt -- `--reps` times per library (default 6), the two libraries alternating: parent, this
           tree, parent, this tree, ...; the parent's library is built by profiles/tools/build_at.sh <commit> <out.so>.
  Method   one MI355X; medians after warm-ups; the whole measurement of (a), (b), (c) twice (`runs`).
  Verdicts `batch_beats_singles`: (a) below (b) in both clocks, on both scenes, in both runs.
           `view_within_parents_spread`: per case, this tree's figure lies within the spread of the parent's own runs -- the figure being the
           median of this tree's per-process medians, the spread the least and the greatest of the parent's per-process medians.  (One
           figure against a range: asking that EVERY one of this tree's processes lie inside the range of as many of the parent's fails
           for two identical libraries more often than not -- a further draw from one distribution lies outside the range of n earlier ones
           with probability 2 / (n + 1).  How many of this tree's processes do lie inside is recorded as `inside_parents_range`.)
           `batch_over_tall` is recorded.  Exit status 3 where a verdict fails or the bytes differ."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

WARM, TIMED, BOUNCES = 2, 7, 5
W, H, K = 32, 16, 2


def both_clocks(ctx, call):
    """-> (device ms between two HIP events, host ms from before the call until the stream has drained)"""
    ctx.finish()
    t0 = time.perf_counter()
    ctx.timer_start()
    call()
    dev = ctx.timer_stop_ms()   # (waits for its event, the last thing on the stream)
    ctx.finish()
    return dev, (time.perf_counter() - t0) * 1e3


def med(x):
    return round(statistics.median(x[WARM:]), 4)


def lattice(ps, frames):
    b = np.asarray(ps.bounds, np.float64)
    lo, hi = b[0:3], b[4:7]
    nx = 16
    ny = nz = int(round((frames / nx) ** 0.5))
    assert nx * ny * nz == frames, "frames = 16 * m * m"
    t = [np.linspace(0.15, 0.85, n) for n in (nx, ny, nz)]
    g = np.stack(np.meshgrid(*t, indexing="ij"), axis=-1).reshape(-1, 3)
    cams = np.zeros((frames, 12), np.float32)
    cams[:, 0:3] = lo + g * (hi - lo)
    cams[:, 3], cams[:, 7], cams[:, 11] = 1.0, 1.0, -1.0
    return cams


def measure(ctx, mirt, ps, frames, log):
    R, P = W * H * K * K, W * H
    n, npx = frames * R, frames * P
    cams = lattice(ps, frames)
    dev = mirt.DeviceScene(ctx, ps)
    desc = dev.pass_desc(None, None, bounces=BOUNCES)
    seeds0 = (np.arange(n, dtype=np.int64) * 7919 + 12345).astype(np.int32)
    seeds, radiance, pixel = ctx.buffer(n * 4), ctx.buffer(npx * 16), ctx.buffer(npx * 4)
    wrapped = []
    try:
        tone = 1.0 / (K * K)
        batch_view = mirt.view_desc("equirect", W, H, k=K, tone=tone)
        tall_view = mirt.view_desc("equirect", W, H * frames, k=K, eye=cams[frames // 2, 0:3], look_at=cams[frames // 2, 0:3] + np.array([0.0, 0.0, -1.0]), tone=tone)
        singles = []
        for f in range(frames):
            v = mirt.view_desc("equirect", W, H, k=K, tone=tone)
            for name, sl in (("eye", slice(0, 3)), ("right", slice(3, 6)), ("up", slice(6, 9)), ("forward", slice(9, 12))):
                setattr(v, name, type(v.eye)(*(float(c) for c in cams[f, sl])))
            bufs = (ctx.wrap(seeds.device_ptr + f * R * 4, R * 4), ctx.wrap(radiance.device_ptr + f * P * 16, P * 16), ctx.wrap(pixel.device_ptr + f * P * 4, P * 4))
            wrapped.extend(bufs)
            singles.append((v,) + bufs)

        def batch():
            ctx.render_view_batch(desc, batch_view, cams, seeds, radiance, pixel)

        def by_singles():
            for v, s, r, p in singles:
                ctx.render_view(desc, v, s, r, p)

        def tall():
            ctx.render_view(desc, tall_view, seeds, radiance, pixel)

        # the table's upload alone, from above: mirt_view_rays_batch of 1 x 1 frames at k = 1 -- the same 16 upload launches and one kernel of 4 blocks
        dot_view = mirt.view_desc("equirect", 1, 1, k=1)
        dot_rays = ctx.buffer(frames * 32)
        wrapped.append(dot_rays)

        def upload():
            ctx.view_rays_batch(dot_view, cams, dot_rays)

        t = {"batch": ([], []), "singles": ([], []), "tall": ([], []), "upload": ([], [])}
        for _ in range(WARM + TIMED):
            for name, call in (("batch", batch), ("singles", by_singles), ("tall", tall), ("upload", upload)):
                seeds.write(seeds0)
                d, h = both_clocks(ctx, call)
                t[name][0].append(d)
                t[name][1].append(h)
        seeds.write(seeds0)
        batch()
        deferred = int(ctx.view_deferred())
        a = (seeds.read(np.int32).tobytes(), radiance.read(np.float32).tobytes(), pixel.read(np.uint8).tobytes())
        seeds.write(seeds0)
        by_singles()
        b = (seeds.read(np.int32).tobytes(), radiance.read(np.float32).tobytes(), pixel.read(np.uint8).tobytes())
        rec = {"frames": frames, "rays": n, "bounces": BOUNCES, "equal": bool(a == b), "batch_deferred_rays": deferred}
        for name in t:
            rec[name + "_ms"] = {"device": med(t[name][0]), "host": med(t[name][1]),
                                 "device_min_max": [round(min(t[name][0][WARM:]), 4), round(max(t[name][0][WARM:]), 4)],
                                 "host_min_max": [round(min(t[name][1][WARM:]), 4), round(max(t[name][1][WARM:]), 4)]}
        rec["singles_over_batch"] = {c: round(rec["singles_ms"][c] / rec["batch_ms"][c], 2) for c in ("device", "host")}
        rec["batch_over_tall"] = {c: round(rec["batch_ms"][c] / rec["tall_ms"][c], 3) for c in ("device", "host")}
        rec["batch_beats_singles"] = bool(all(rec["batch_ms"][c] < rec["singles_ms"][c] for c in ("device", "host")))
        rec["M_rays_per_s_batch"] = round(n / rec["batch_ms"]["device"] / 1e3, 1)
        log(f"  {json.dumps(rec)}")
        return rec
    finally:
        for x in wrapped + [seeds, radiance, pixel]:
            x.release()
        dev.release()


def view_child(lib):
    """profiles/view_bench.py --quick in a process of its own: -> its JSON line"""
    env = dict(os.environ)
    env.pop("MIRT_LIB_PATH", None)
    if lib:
        env["MIRT_LIB_PATH"] = lib
    r = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "view_bench.py"), "--quick"], env=env, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent", nargs="?", help="libmirt.so of the parent commit (profiles/tools/build_at.sh)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_batch", "timing.json"))
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=6, help="child processes per library for (d)")
    args = ap.parse_args()
    log = lambda s: print(s, file=sys.stderr, flush=True)
    graft.load_package()
    from raytracing_amd.pyhost import mirt, scene
    golden = os.path.join(ROOT, "tests", "golden")
    cornell = scene.PackedScene(open(os.path.join(golden, "scene_cornell_1920x1080_r256.json")).read()).resized(W, H, K * K)
    fx = np.load(os.path.join(golden, "cornell_teapot3_32x24_r4.npz"))
    teapot3 = scene.PackedScene(json.loads(bytes(fx["scene_json"]).decode())).resized(W, H, K * K)
    res = {"library": os.path.basename(mirt.LIB_PATH), "width": W, "height": H, "k": K, "warmups": WARM, "timed_calls": TIMED,
           "method": "medians; device: HIP events around the span; host: perf_counter from before the first call until mirt_finish returns; the "
                     "batch call, the N single calls and the one tall frame alternate in one loop; two runs",
           "runs": []}
    ctx = mirt.Context(0)
    ok = True
    for run in range(2):
        rec = {}
        for name, ps in (("cornell", cornell), ("cornell_teapot3", teapot3)):
            log(f"run {run + 1} {name}")
            rec[name] = measure(ctx, mirt, ps, args.frames, log)
            ok = ok and rec[name]["equal"]
        res["runs"].append(rec)
    ctx.destroy()
    res["batch_beats_singles"] = bool(all(r[s]["batch_beats_singles"] for r in res["runs"] for s in r))
    ok = ok and res["batch_beats_singles"]
    if args.parent:
        order = [("parent", os.path.abspath(args.parent)), ("this_tree", None)] * args.reps
        lines = []
        for label, lib in order:
            log(f"mirt_render_view 1920 x 1080 x 4: {label}")
            lines.append({"lib": label, "run": view_child(lib)})
            log(f"  {json.dumps(lines[-1]['run'])}")
        cases = {}
        for scene_name in ("cornell", "cornell_teapot3"):
            for cam in ("equirect", "ortho_oblique"):
                ms = {lab: [l["run"][f"{scene_name}_{cam}"] for l in lines if l["lib"] == lab] for lab in ("parent", "this_tree")}
                lo, hi = min(ms["parent"]), max(ms["parent"])
                figure = round(statistics.median(ms["this_tree"]), 4)
                cases[f"{scene_name}_{cam}"] = {"parent_ms": ms["parent"], "this_tree_ms": ms["this_tree"], "parent_spread_ms": [lo, hi],
                                                "parent_median_ms": round(statistics.median(ms["parent"]), 4), "this_tree_median_ms": figure,
                                                "inside_parents_range": sum(1 for m in ms["this_tree"] if lo <= m <= hi),
                                                "within_parents_spread": bool(lo <= figure <= hi)}
        res["view_1920x1080x4"] = {"order": [l["lib"] for l in lines], "processes_per_library": args.reps, "cases": cases}
        res["view_within_parents_spread"] = bool(all(c["within_parents_spread"] for c in cases.values()))
        ok = ok and res["view_within_parents_spread"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in res if k not in ("runs", "method")}))
    return 0 if ok else 3


if __name__ == "__main__":
    sys.exit(main())
