#!/usr/bin/env python3
"""profiles/view_guided_bench.py [parent-libmirt.so] [--out FILE.json] [--size W H K] -- a view camera's frame and its first-hit guides in one
call (mirt_render_view_guided, the one-launch route) beside the two calls it equals, mirt_render_view then mirt_view_guides, on the same library;
and, for scale and as a check that the unguided frame did not pay for the new template parameter, mirt_render_view of the parent commit's
library (profiles/tools/build_at.sh <commit> <out.so>).

  Scenes   cornell (single-cell sets) and cornell_teapot3 (two grid meshes) at 1920 x 1080, k = 2 (4 rays per pixel), bounces 5.
  Cameras  EQUIRECT from the scene box's centre, and ORTHOGRAPHIC with the oblique basis of profiles/view_bench.py.
  Calls    guided_ms      mirt_render_view_guided as the route rule sends it (pt_view_plan.hpp view_guides_in_pass);
           two_calls_ms   the same call with MIRT_GUIDED_VIEW=0 in the environment (read per call): the frame, then the guide launches;
           view_ms, guides_ms   mirt_render_view and mirt_view_guides alone.
           All four alternate in one loop, each frame call right behind the upload of the same seeds; behind the loop, un-timed, every buffer
           of the guided call must equal the two calls' bit for bit (`equal`).
  Parent   mirt_render_view alone in child processes -- a process loads one libmirt -- in the order parent, this tree, parent, this tree.
  Method   one MI355X; medians of HIP-event times (mirt_timer_start / mirt_timer_stop_ms) after warm-ups; the whole measurement twice (`runs`),
           whose spread per case is the margin (`spread_ms`).
  Verdicts per case: `one_launch_faster` -- the guided call's slower run is below the two calls' faster run by more than the spread; a kernel
           family (single-cell: cornell; grids: cornell_teapot3) one of whose cases fails it goes to the two launches in the route rule.
           `view_not_slower_than_parent` -- the faster of this tree's two mirt_render_view medians is not above the faster of the parent's two by
           more than the spread of the two runs, the larger of the two libraries' (the kernels' resource lines are identical:
           profiles/view_guided/README.md).  Exit status 3 where a case's results differ."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import __graft_entry__ as graft  # noqa: E402
import view_bench as VB  # noqa: E402

WARM, TIMED, BOUNCES = VB.WARM, VB.TIMED, VB.BOUNCES
med = VB.med


def scenes(w, h, k):
    from raytracing_amd.pyhost import scene
    golden = os.path.join(ROOT, "tests", "golden")
    cornell = scene.PackedScene(open(os.path.join(golden, "scene_cornell_1920x1080_r256.json")).read()).resized(w, h, k * k)
    fx = np.load(os.path.join(golden, "cornell_teapot3_32x24_r4.npz"))
    teapot3 = scene.PackedScene(json.loads(bytes(fx["scene_json"]).decode())).resized(w, h, k * k)
    return (("cornell", cornell), ("cornell_teapot3", teapot3))


def set_switch(value):
    """MIRT_GUIDED_VIEW as the library reads it, per call: None removes it"""
    if value is None:
        os.environ.pop("MIRT_GUIDED_VIEW", None)
    else:
        os.environ["MIRT_GUIDED_VIEW"] = value


def measure(ctx, mirt, ps, w, h, k, log, view_only):
    n_pix, n = w * h, w * h * k * k
    dev = mirt.DeviceScene(ctx, ps)
    desc = dev.pass_desc(None, None, bounces=BOUNCES)
    seeds0 = (np.arange(n, dtype=np.int64) * 7919 + 12345).astype(np.int32)
    bufs = [ctx.buffer(b) for b in (n * 4, n_pix * 16, n_pix * 4, n_pix * 16, n_pix * 16)]
    seeds, radiance, pixel, nh, ad = bufs
    out = {}
    try:
        for label, view in VB.views(mirt, ps, w, h, k):
            def guided():
                ctx.render_view_guided(desc, view, seeds, radiance, pixel, nh, ad)

            t = {"view": [], "guided": [], "two_calls": [], "guides": []}
            results = {}
            for _ in range(WARM + TIMED):
                seeds.write(seeds0)
                t["view"].append(VB.timed(ctx, lambda: ctx.render_view(desc, view, seeds, radiance, pixel)))
                if view_only:
                    continue
                for name, env in (("guided", None), ("two_calls", "0")):   # every timed frame call follows the same thing: the seeds' upload
                    seeds.write(seeds0)
                    set_switch(env)
                    t[name].append(VB.timed(ctx, guided))
                set_switch(None)
                t["guides"].append(VB.timed(ctx, lambda: ctx.view_guides(desc, view, nh, ad)))
            if not view_only:   # outside the timed loop: the two routes' buffers, and which route each call took
                for name, env in (("guided", None), ("two_calls", "0")):
                    seeds.write(seeds0)
                    set_switch(env)
                    before = ctx.guided_views()
                    guided()
                    results[name + "_routed"] = ctx.guided_views() - before
                    results[name] = [b.read(np.uint8).tobytes() for b in bufs]
                set_switch(None)
            rec = {"view_ms": med(t["view"]), "view_min_max": VB.span(t["view"])}
            if not view_only:
                rec.update({"guided_ms": med(t["guided"]), "guided_min_max": VB.span(t["guided"]), "two_calls_ms": med(t["two_calls"]),
                            "two_calls_min_max": VB.span(t["two_calls"]), "guides_ms": med(t["guides"]), "deferred_rays": int(ctx.view_deferred()),
                            "guided_took_one_launch": results["guided_routed"] == 1, "switch_took_two_launches": results["two_calls_routed"] == 0,
                            "equal": results["guided"] == results["two_calls"], "ratio_two_calls_over_guided": round(med(t["two_calls"]) / med(t["guided"]), 3)})
            out[label] = rec
            log(f"  {label}: {json.dumps(rec)}")
        return out
    finally:
        for b in bufs:
            b.release()
        dev.release()


def run_all(w, h, k, log, view_only):
    graft.load_package()
    from raytracing_amd.pyhost import mirt
    ctx = mirt.Context(0)
    ctx.set_fusion(0)
    rec = {"library": mirt.LIB_PATH}
    try:
        for name, ps in scenes(w, h, k):
            log(f"{os.path.basename(mirt.LIB_PATH)} {name}")
            rec[name] = measure(ctx, mirt, ps, w, h, k, log, view_only)
    finally:
        ctx.destroy()
    return rec


def child(lib, size):
    env = dict(os.environ)
    env.pop("MIRT_LIB_PATH", None)
    env.pop("MIRT_GUIDED_VIEW", None)
    if lib:
        env["MIRT_LIB_PATH"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--view-only", "--size"] + [str(x) for x in size], env=env, stdout=subprocess.PIPE, text=True, timeout=420)
    if r.returncode:
        raise RuntimeError(f"the child with {lib or 'this tree'} failed")
    return json.loads(r.stdout.splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent", nargs="?", help="libmirt.so of the parent commit (profiles/tools/build_at.sh)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_guided", "timing.json"))
    ap.add_argument("--size", type=int, nargs=3, default=[1920, 1080, 2], metavar=("W", "H", "K"))
    ap.add_argument("--view-only", action="store_true", help="(the child's mode) mirt_render_view alone, one JSON line")
    args = ap.parse_args()
    log = lambda s: print(s, file=sys.stderr, flush=True)
    w, h, k = args.size
    if args.view_only:
        print(json.dumps(run_all(w, h, k, log, True)))
        return 0
    res = {"width": w, "height": h, "k": k, "rays_per_pixel": k * k, "bounces": BOUNCES, "warmups": WARM, "timed_calls": TIMED,
           "method": "medians of HIP-event times; mirt_render_view, mirt_render_view_guided, the same with MIRT_GUIDED_VIEW=0 and mirt_view_guides "
                     "alternating in one loop; two runs, whose spread per case is the margin; the parent's mirt_render_view in child processes",
           "runs": [], "parent_runs": []}
    parent = os.path.abspath(args.parent) if args.parent else None
    if parent:
        res["parent_runs"].append(dict(child(parent, args.size), role="parent"))
    for _ in range(2):
        res["runs"].append(run_all(w, h, k, log, False))
    if parent:
        res["this_tree_child_runs"] = [child(None, args.size)]
        res["parent_runs"].append(dict(child(parent, args.size), role="parent, again"))
        res["this_tree_child_runs"].append(child(None, args.size))
    res["cases"], families = {}, {"cornell": "single_cell", "cornell_teapot3": "grids"}
    for s in families:
        for c in ("equirect", "ortho_oblique"):
            a, b = (r[s][c] for r in res["runs"])
            spread = round(max(abs(a["guided_ms"] - b["guided_ms"]), abs(a["two_calls_ms"] - b["two_calls_ms"])), 4)
            case = {"family": families[s], "guided_ms": [a["guided_ms"], b["guided_ms"]], "two_calls_ms": [a["two_calls_ms"], b["two_calls_ms"]],
                    "view_ms": [a["view_ms"], b["view_ms"]], "guides_ms": [a["guides_ms"], b["guides_ms"]], "spread_ms": spread,
                    "one_launch_faster": bool(max(a["guided_ms"], b["guided_ms"]) + spread < min(a["two_calls_ms"], b["two_calls_ms"])),
                    "equal": bool(a["equal"] and b["equal"]), "guided_took_one_launch": bool(a["guided_took_one_launch"] and b["guided_took_one_launch"])}
            if parent:
                p = [r[s][c]["view_ms"] for r in res["parent_runs"]]
                own = [r[s][c]["view_ms"] for r in res["this_tree_child_runs"]]
                margin = max(abs(p[0] - p[1]), abs(own[0] - own[1]))
                case.update({"parent_view_ms": p, "this_tree_view_ms_in_children": own, "view_spread_ms": round(margin, 4),
                             "view_not_slower_than_parent": bool(min(own) <= min(p) + margin)})
            res["cases"][f"{s}_{c}"] = case
    res["one_launch_faster_by_family"] = {f: all(x["one_launch_faster"] for x in res["cases"].values() if x["family"] == f) for f in families.values()}
    res["equal_on_every_case"] = all(x["equal"] for x in res["cases"].values())
    if parent:
        res["view_not_slower_than_parent_on_every_case"] = all(x["view_not_slower_than_parent"] for x in res["cases"].values())
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("cases", "one_launch_faster_by_family", "equal_on_every_case", "view_not_slower_than_parent_on_every_case") if k in res}, indent=1))
    return 0 if res["equal_on_every_case"] else 3


if __name__ == "__main__":
    sys.exit(main())
