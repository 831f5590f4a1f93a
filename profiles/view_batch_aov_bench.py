#!/usr/bin/env python3
"""profiles/view_batch_aov_bench.py [parent-libmirt.so] [--out FILE.json] [--frames N] -- the guides, the ambient occlusion and the guided frames
of N small view cameras in ONE call (mirt_view_guides_batch, mirt_view_ao_batch, mirt_render_view_guided_batch) beside the calls they equal,
on the same library.  The set-up, the clocks and the method are profiles/view_batch_bench.py's: 1024 EQUIRECT cameras on the 16 x 8 x 8
lattice, 32 x 16, k = 2, scenes cornell (single-cell sets) and cornell_teapot3 (two grid meshes); medians of 7 calls after 2 warm-ups, the
variants alternating in one loop; device clock (HIP events) and host clock; the whole measurement twice (`runs`).

  (a) guides_batch_ms    one mirt_view_guides_batch of the 1024 frames;
      guides_singles_ms  the 1024 mirt_view_guides calls, frame f on wrapped slices of the same buffers;
      guides_tall_ms     one mirt_view_guides of a 32 x 16384 image: the same pixel count and ONE camera;
  (b) ao_batch_ms        one mirt_view_ao_batch (4 samples, radius 1);
      ao_singles_ms      the 1024 mirt_view_ao calls;
  (c) guided_ms          one mirt_render_view_guided_batch (bounces 5; the one-launch route at k = 2);
      two_calls_ms       mirt_render_view_batch and then mirt_view_guides_batch;
      behind the loop, un-timed, the batch and the singles of (a) and (b), and the two routes of (c), must have left equal bytes (`equal`);
  (d) with the parent's library (profiles/tools/build_at.sh <commit> <out.so>): mirt_render_view_batch of the same 1024 frames in child
      processes (`--child`: a process loads one libmirt), `--reps` per library, the two alternating -- parent, this tree, parent, ...

  Verdicts `batch_beats_singles`: (a) and (b), the batch below the singles on both clocks, both scenes, both runs.
           `one_launch_beats_two`, per scene family: guided_ms below two_calls_ms by more than the spread between the two runs (the greater
           of the two figures' |run 1 - run 2|, device clock), in both runs.  A family that fails goes to the two launches in
           csrc/pt_view_plan.hpp.
           `batch_within_parents_spread`: per scene, the median of this tree's per-process medians lies within the least and the greatest of
           the parent's (view_batch_bench.py's criterion and its reason).
           Exit status 3 where bytes differ, the batch does not beat the singles or (d) fails; (c) is a decision, recorded."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import __graft_entry__ as graft  # noqa: E402
import view_batch_bench as VBB  # noqa: E402  (both_clocks, med, lattice, the sizes)

WARM, TIMED, BOUNCES, W, H, K = VBB.WARM, VBB.TIMED, VBB.BOUNCES, VBB.W, VBB.H, VBB.K
AO_SAMPLES, AO_RADIUS = 4, 1.0


def scenes(mirt_scene):
    golden = os.path.join(ROOT, "tests", "golden")
    cornell = mirt_scene.PackedScene(open(os.path.join(golden, "scene_cornell_1920x1080_r256.json")).read()).resized(W, H, K * K)
    fx = np.load(os.path.join(golden, "cornell_teapot3_32x24_r4.npz"))
    teapot3 = mirt_scene.PackedScene(json.loads(bytes(fx["scene_json"]).decode())).resized(W, H, K * K)
    return (("cornell", cornell), ("cornell_teapot3", teapot3))


def stats(t):
    d, h = t
    return {"device": VBB.med(d), "host": VBB.med(h), "device_min_max": [round(min(d[WARM:]), 4), round(max(d[WARM:]), 4)],
            "host_min_max": [round(min(h[WARM:]), 4), round(max(h[WARM:]), 4)]}


def measure(ctx, mirt, ps, frames, log):
    R, P = W * H * K * K, W * H
    n, npx = frames * R, frames * P
    cams = VBB.lattice(ps, frames)
    dev = mirt.DeviceScene(ctx, ps)
    desc = dev.pass_desc(None, None, bounces=BOUNCES)
    seeds0 = (np.arange(n, dtype=np.int64) * 7919 + 12345).astype(np.int32)
    seeds, radiance, pixel = ctx.buffer(n * 4), ctx.buffer(npx * 16), ctx.buffer(npx * 4)
    nh, ad, ao = ctx.buffer(npx * 16), ctx.buffer(npx * 16), ctx.buffer(npx * 8)
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
            bufs = (ctx.wrap(seeds.device_ptr + f * R * 4, R * 4), ctx.wrap(nh.device_ptr + f * P * 16, P * 16), ctx.wrap(ad.device_ptr + f * P * 16, P * 16),
                    ctx.wrap(ao.device_ptr + f * P * 8, P * 8))
            wrapped.extend(bufs)
            singles.append((v,) + bufs)

        def guides_batch():
            ctx.view_guides_batch(desc, batch_view, cams, nh, ad)

        def guides_singles():
            for v, _s, a, b, _o in singles:
                ctx.view_guides(desc, v, a, b)

        def guides_tall():
            ctx.view_guides(desc, tall_view, nh, ad)

        def ao_batch():
            ctx.view_ao_batch(desc, batch_view, cams, seeds, ao, AO_SAMPLES, AO_RADIUS)

        def ao_singles():
            for v, s, _a, _b, o in singles:
                ctx.view_ao(desc, v, s, o, AO_SAMPLES, AO_RADIUS)

        def guided():
            ctx.render_view_guided_batch(desc, batch_view, cams, seeds, radiance, pixel, nh, ad)

        def two_calls():
            ctx.render_view_batch(desc, batch_view, cams, seeds, radiance, pixel)
            ctx.view_guides_batch(desc, batch_view, cams, nh, ad)

        calls = (("guides_batch", guides_batch), ("guides_singles", guides_singles), ("guides_tall", guides_tall), ("ao_batch", ao_batch), ("ao_singles", ao_singles),
                 ("guided", guided), ("two_calls", two_calls))
        t = {name: ([], []) for name, _c in calls}
        for _ in range(WARM + TIMED):
            for name, call in calls:
                seeds.write(seeds0)
                d, h = VBB.both_clocks(ctx, call)
                t[name][0].append(d)
                t[name][1].append(h)

        def after(call, bufs):
            seeds.write(seeds0)
            for b in bufs:
                ctx.zero(b)
            call()
            ctx.finish()
            return tuple(b.read(np.uint8).tobytes() for b in (seeds,) + tuple(bufs))

        routed0 = ctx.guided_views()
        one = after(guided, (radiance, pixel, nh, ad))
        routed = ctx.guided_views() - routed0
        rec = {"frames": frames, "pixels": npx, "rays": n, "bounces": BOUNCES, "ao_samples": AO_SAMPLES, "ao_radius": AO_RADIUS,
               "guided_took_the_one_launch_route": bool(routed == 1),
               "equal": {"guides": bool(after(guides_batch, (nh, ad)) == after(guides_singles, (nh, ad))), "ao": bool(after(ao_batch, (ao,)) == after(ao_singles, (ao,))),
                         "guided": bool(one == after(two_calls, (radiance, pixel, nh, ad)))}}
        after(ao_batch, (ao,))
        rec["ao_batch_deferred_pixels"] = int(ctx.view_ao_deferred())
        for name in t:
            rec[name + "_ms"] = stats(t[name])
        for kind in ("guides", "ao"):
            rec[f"{kind}_singles_over_batch"] = {c: round(rec[f"{kind}_singles_ms"][c] / rec[f"{kind}_batch_ms"][c], 2) for c in ("device", "host")}
        rec["guides_batch_over_tall"] = {c: round(rec["guides_batch_ms"][c] / rec["guides_tall_ms"][c], 3) for c in ("device", "host")}
        rec["batch_beats_singles"] = bool(all(rec[f"{kind}_batch_ms"][c] < rec[f"{kind}_singles_ms"][c] for kind in ("guides", "ao") for c in ("device", "host")))
        rec["two_calls_minus_guided_ms"] = {c: round(rec["two_calls_ms"][c] - rec["guided_ms"][c], 4) for c in ("device", "host")}
        log(f"  {json.dumps(rec)}")
        return rec
    finally:
        for x in wrapped + [seeds, radiance, pixel, nh, ad, ao]:
            x.release()
        dev.release()


def child(frames):
    """(d), in a process of its own: the median device and host ms of mirt_render_view_batch per scene -> one JSON line"""
    graft.load_package()
    from raytracing_amd.pyhost import mirt, scene
    ctx = mirt.Context(0)
    out = {"library": mirt.LIB_PATH}
    for name, ps in scenes(scene):
        R, P = W * H * K * K, W * H
        n, npx = frames * R, frames * P
        cams = VBB.lattice(ps, frames)
        dev = mirt.DeviceScene(ctx, ps)
        desc = dev.pass_desc(None, None, bounces=BOUNCES)
        seeds0 = (np.arange(n, dtype=np.int64) * 7919 + 12345).astype(np.int32)
        seeds, radiance, pixel = ctx.buffer(n * 4), ctx.buffer(npx * 16), ctx.buffer(npx * 4)
        view = mirt.view_desc("equirect", W, H, k=K, tone=1.0 / (K * K))
        d, h = [], []
        for _ in range(WARM + TIMED):
            seeds.write(seeds0)
            a, b = VBB.both_clocks(ctx, lambda: ctx.render_view_batch(desc, view, cams, seeds, radiance, pixel))
            d.append(a)
            h.append(b)
        out[name] = {"device": VBB.med(d), "host": VBB.med(h)}
        for x in (seeds, radiance, pixel):
            x.release()
        dev.release()
    ctx.destroy()
    print(json.dumps(out), flush=True)
    return 0


def batch_child(lib, frames):
    env = dict(os.environ)
    env.pop("MIRT_LIB_PATH", None)
    if lib:
        env["MIRT_LIB_PATH"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--frames", str(frames)], env=env, capture_output=True, text=True, timeout=120)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent", nargs="?", help="libmirt.so of the parent commit (profiles/tools/build_at.sh)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_batch_aov", "timing.json"))
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=6, help="child processes per library for (d)")
    ap.add_argument("--child", action="store_true", help="(d)'s measurement of the loaded library alone")
    ap.add_argument("--only-parent", action="store_true", help="(d) alone, merged into the --out file that (a), (b), (c) wrote")
    ap.add_argument("--note", default=None, help="a label recorded with the result (a build variant)")
    args = ap.parse_args()
    if args.child:
        return child(args.frames)
    log = lambda s: print(s, file=sys.stderr, flush=True)
    graft.load_package()
    from raytracing_amd.pyhost import mirt, scene
    ok = True
    if args.only_parent:
        res = json.load(open(args.out))
    else:
        res = {"library": os.path.basename(mirt.LIB_PATH), "width": W, "height": H, "k": K, "warmups": WARM, "timed_calls": TIMED,
               "method": "medians; device: HIP events around the span; host: perf_counter from before the first call until mirt_finish returns; all "
                         "variants alternate in one loop; two runs", "runs": []}
        if args.note:
            res["note"] = args.note
        ctx = mirt.Context(0)
        for run in range(2):
            rec = {}
            for name, ps in scenes(scene):
                log(f"run {run + 1} {name}")
                rec[name] = measure(ctx, mirt, ps, args.frames, log)
                ok = ok and all(rec[name]["equal"].values())
            res["runs"].append(rec)
        ctx.destroy()
        res["batch_beats_singles"] = bool(all(r[s]["batch_beats_singles"] for r in res["runs"] for s in r))
        ok = ok and res["batch_beats_singles"]
        verdict = {}
        for s, family in (("cornell", "single_cell"), ("cornell_teapot3", "grid")):
            g = [r[s]["guided_ms"]["device"] for r in res["runs"]]
            two = [r[s]["two_calls_ms"]["device"] for r in res["runs"]]
            spread = max(abs(g[0] - g[1]), abs(two[0] - two[1]))
            gain = [round(b - a, 4) for a, b in zip(g, two)]
            verdict[family] = {"scene": s, "guided_ms": g, "two_calls_ms": two, "spread_between_runs_ms": round(spread, 4), "two_calls_minus_guided_ms": gain,
                               "one_launch_beats_two": bool(all(x > spread for x in gain))}
        res["guided_route"] = verdict
    if args.parent:
        order = [("parent", os.path.abspath(args.parent)), ("this_tree", None)] * args.reps
        lines = []
        for label, lib in order:
            log(f"mirt_render_view_batch, {args.frames} frames: {label}")
            lines.append({"lib": label, "run": batch_child(lib, args.frames)})
            log(f"  {json.dumps(lines[-1]['run'])}")
        cases = {}
        for s in ("cornell", "cornell_teapot3"):
            ms = {lab: [l["run"][s]["device"] for l in lines if l["lib"] == lab] for lab in ("parent", "this_tree")}
            lo, hi = min(ms["parent"]), max(ms["parent"])
            figure = round(statistics.median(ms["this_tree"]), 4)
            cases[s] = {"parent_ms": ms["parent"], "this_tree_ms": ms["this_tree"], "parent_spread_ms": [lo, hi], "parent_median_ms": round(statistics.median(ms["parent"]), 4),
                        "this_tree_median_ms": figure, "inside_parents_range": sum(1 for m in ms["this_tree"] if lo <= m <= hi), "within_parents_spread": bool(lo <= figure <= hi)}
        res["render_view_batch_vs_parent"] = {"order": [l["lib"] for l in lines], "processes_per_library": args.reps, "clock": "device", "cases": cases}
        res["batch_within_parents_spread"] = bool(all(c["within_parents_spread"] for c in cases.values()))
        ok = ok and res["batch_within_parents_spread"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in res if k not in ("runs", "method")}))
    return 0 if ok else 3


if __name__ == "__main__":
    sys.exit(main())
