#!/usr/bin/env python3
"""profiles/rays_bench.py [--out FILE.json] [--parent-lib libmirt.so] -- ray queries on caller-supplied rays (mirt_trace_closest,
mirt_trace_occluded) against the only way the library could answer the same question before them: the kernel-by-kernel enqueues on the same rays.

  Scenes   cornell and cornell_teapot3 (single-cell sets; two grid meshes).
  Rays     1920 x 1080 of three kinds: `coherent`, the pinhole camera's primary rays in pixel order; `permuted`, the same rays in a seeded random
           permutation; `axis`, rays straight down (d = (0, -1, 0)) over a 1920 x 1080 grid of origins above the scene box.
  Variants one_launch: one mirt_trace_closest / mirt_trace_occluded call (the optimistic / exact pair); baseline: sphereTrace, triangleTrace and
           every meshTrace (for occlusion: the shadow kernels) through mirt_enqueue on a 48-byte Ray buffer of the same rays, on the same context.
           The baseline's kernels change the rays they trace (Ray.maxt; a blocked shadow ray's mint), so its buffer is rewritten from the host
           before every call, outside the timed region.
  Method   one MI355X; per (scene, kind, query) medians of 20 calls between two HIP events (mirt_timer_start / mirt_timer_stop_ms) after 3
           warm-ups, the two variants alternating in one loop; the whole measurement twice (`runs`).
  Condition (the rule DESIGN.md uses for its route decisions): the one-launch call's median is not above the baseline's in either run, for the
           coherent and the permuted rays.  `condition_met` says so per run; the script exits 1 when it is not met.
  Recorded without a bound: Mrays/s, the deferred share (mirt_trace_deferred / rays) and the ratio of permuted to coherent, per kind; for the
           axis rays, which the ray-side guard refuses whole, also the call under mirt_ctx_set_exact_only (`exact_only_ms`).
  --parent-lib: also `python bench.py` (5 steps after 2 warm-ups) alternately on this tree's library and on that one (MIRT_LIB_PATH): the fused
           kernels are untouched, so the headline should sit inside the min .. max of the parent's calls."""
import argparse
import glob
import hashlib
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

W, H = 1920, 1080
WARM, TIMED = 3, 20
RAY_DT = np.dtype({"names": ["o", "d", "mint", "maxt"], "formats": [(np.float32, 3), (np.float32, 3), np.float32, np.float32],
                   "offsets": [0, 16, 32, 36], "itemsize": 48})   # the kernels' 48-byte Ray


def csrc_sha256():
    h = hashlib.sha256()
    d = os.path.join(ROOT, "2015-raytracing_amd", "csrc")
    for f in sorted(glob.glob(os.path.join(d, "*.hip")) + glob.glob(os.path.join(d, "*.hpp")) + glob.glob(os.path.join(d, "*.cpp")) + glob.glob(os.path.join(d, "*.sh"))):
        h.update(os.path.basename(f).encode() + b"\0" + open(f, "rb").read())
    return h.hexdigest()


def pinhole_rays(ps):
    """the primary rays of the scene's camera through the pixel centres, without a lens: o = eye, d = normalise(sx U + sy V - W), pixel order"""
    cam = np.asarray(ps.cam, np.float64)
    eye, U, V, Wv, cw, ch = cam[0:3], cam[3:6], cam[6:9], cam[9:12], cam[12], cam[13]
    col, row = np.meshgrid(np.arange(W), np.arange(H))
    sx = (-0.5 + (col.ravel() + 0.5) / W) * cw
    sy = (0.5 - (row.ravel() + 0.5) / H) * ch
    d = sx[:, None] * U + sy[:, None] * V - Wv
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.zeros((W * H, 8), np.float32)
    r[:, 0:3], r[:, 4:7], r[:, 7] = eye, d, np.inf
    return r


def axis_rays(ps):
    b = np.asarray(ps.bounds, np.float64)
    lo, hi = b[0:3], b[4:7]
    x, z = np.meshgrid(np.linspace(lo[0], hi[0], W + 2)[1:-1], np.linspace(lo[2], hi[2], H + 2)[1:-1])
    r = np.zeros((W * H, 8), np.float32)
    r[:, 0], r[:, 1], r[:, 2] = x.ravel(), hi[1] + 0.25 * (hi[1] - lo[1]), z.ravel()
    r[:, 5], r[:, 7] = -1.0, np.inf
    return r


def ray48(rays):
    out = np.zeros(len(rays), RAY_DT)
    out["o"], out["mint"], out["d"], out["maxt"] = rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7]
    return out


class Baseline:
    """the kernel-by-kernel enqueues on a 48-byte Ray / 64-byte Poi buffer (pyhost/render.py GranularRenderer._closest and the shadow kernels of ._direct)"""

    def __init__(self, ctx, dev, ps, n):
        u32 = lambda v: np.array([v], np.uint32)
        self.ctx, self.g1 = ctx, [-(-n // 64) * 64]
        self.rays, self.pois = ctx.buffer(self.g1[0] * 48), ctx.buffer(self.g1[0] * 64)
        self.closest, self.shadow = [], []
        k = lambda name, *a: ctx.kernel(name).set_args(*a)
        if ps.has_spheres:
            self.closest.append(k("sphereTrace", u32(n), self.pois, self.rays, dev.sph["prims"], dev.sph["matid"], dev.sph["off"], ps.sphere_bounds, u32(ps.n_slabs)))
            self.shadow.append(k("sphereShadowTrace", u32(n), self.rays, dev.sph["prims"], dev.sph["off"], ps.sphere_bounds, u32(ps.n_slabs)))
        if ps.has_triangles:
            self.closest.append(k("triangleTrace", u32(n), self.pois, self.rays, dev.tri["prims"], dev.tri["normals"], dev.tri["matid"], dev.tri["off"],
                                  ps.triangle_bounds, u32(ps.n_slabs)))
            self.shadow.append(k("triangleShadowTrace", u32(n), self.rays, dev.tri["prims"], dev.tri["off"], ps.triangle_bounds, u32(ps.n_slabs)))
        for m in dev.meshes:
            self.closest.append(k("meshTrace", u32(n), self.pois, self.rays, m["prims"], m["normals"], m["off"], u32(m["matid"]), m["bounds"], u32(m["n"])))
            self.shadow.append(k("triangleShadowTrace", u32(n), self.rays, m["prims"], m["off"], m["bounds"], u32(m["n"])))

    def run(self, kernels):
        for k in kernels:
            k.enqueue(self.g1, [64])

    def release(self):
        for k in self.closest + self.shadow:
            k.release()
        self.rays.release()
        self.pois.release()


def timed(ctx, call):
    ctx.finish()
    ctx.timer_start()
    call()
    return ctx.timer_stop_ms()


def measure(ctx, dev, ps, kinds):
    n = W * H
    desc = dev.pass_desc(None, None)
    rays = ctx.buffer(n * 32)
    hits, occ = ctx.buffer(n * 32), ctx.buffer(n)
    base = Baseline(ctx, dev, ps, n)
    out = {}
    for kind, r in kinds.items():
        rays.write(r)
        r48 = ray48(r)
        rec = {}
        for query, one, kernels in (("closest", lambda: ctx.trace_closest(desc, rays, n, hits), base.closest),
                                    ("occluded", lambda: ctx.trace_occluded(desc, rays, n, occ), base.shadow)):
            t_one, t_base = [], []
            for _ in range(WARM + TIMED):
                t_one.append(timed(ctx, one))
                base.rays.write(r48)          # the baseline's kernels wrote into their rays: the same rays again, outside the timed region
                t_base.append(timed(ctx, lambda: base.run(kernels)))
            one()
            deferred = ctx.trace_deferred()
            a, b = statistics.median(t_one[WARM:]), statistics.median(t_base[WARM:])
            rec[query] = {"one_launch_ms": round(a, 4), "one_launch_min_max": [round(min(t_one[WARM:]), 4), round(max(t_one[WARM:]), 4)],
                          "baseline_ms": round(b, 4), "baseline_min_max": [round(min(t_base[WARM:]), 4), round(max(t_base[WARM:]), 4)],
                          "baseline_launches": len(kernels), "Mrays_per_s": round(n / a / 1e3, 1), "baseline_Mrays_per_s": round(n / b / 1e3, 1),
                          "deferred_share": round(deferred / n, 5), "one_launch_not_above_baseline": bool(a <= b)}
            if kind == "axis":   # what a caller who knows the guard refuses the batch pays with mirt_ctx_set_exact_only: the exact kernel alone
                ctx.set_exact_only(True)
                t = [timed(ctx, one) for _ in range(WARM + TIMED)]
                ctx.set_exact_only(False)
                rec[query]["exact_only_ms"] = round(statistics.median(t[WARM:]), 4)
        if kind == "coherent":
            h = hits.read(np.float32).reshape(-1, 8)
            rec["hit_share"] = round(float((h[:, 7].view(np.int32) >= 0).mean()), 4)
        out[kind] = rec
    for q in ("closest", "occluded"):
        out["permuted"][q]["over_coherent"] = round(out["permuted"][q]["one_launch_ms"] / out["coherent"][q]["one_launch_ms"], 4)
        out["permuted"][q]["baseline_over_coherent"] = round(out["permuted"][q]["baseline_ms"] / out["coherent"][q]["baseline_ms"], 4)
    base.release()
    for b in (rays, hits, occ):
        b.release()
    return out


def headline(parent_lib, log):
    """bench.py's one JSON line, alternately on this tree's library and on the parent's"""
    runs = {"this_tree": [], "parent": []}
    for i in range(7):
        who = "parent" if i % 2 == 0 else "this_tree"
        env = dict(os.environ)
        env.pop("MIRT_LIB_PATH", None)
        if who == "parent":
            env["MIRT_LIB_PATH"] = os.path.abspath(parent_lib)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2"], env=env, capture_output=True, text=True, timeout=300)
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode != 0 or not lines:
            raise RuntimeError(f"bench.py ({who}) failed: {r.stderr[-1000:]}")
        d = json.loads(lines[-1])
        runs[who].append({"value": d["value"], "ms_per_step": d["ms_per_step"], "launch_ms": d["roofline"]["launch_ms"]})
        log(f"bench.py {who}: {d['value']} {d['unit']}, launch {d['roofline']['launch_ms']} ms")
    lo, hi = min(x["launch_ms"] for x in runs["parent"]), max(x["launch_ms"] for x in runs["parent"])
    med = statistics.median(x["launch_ms"] for x in runs["this_tree"])
    return {"command": "python bench.py --gpus 1 --steps 5 --warmup 2", "parent_library": os.path.basename(parent_lib), "calls": runs,
            "parent_launch_ms_min_max": [lo, hi], "this_tree_launch_ms_median": med, "inside_parent_min_max": bool(lo <= med <= hi)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rays", "timing.json"))
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    log = lambda s: print(s, file=sys.stderr, flush=True)
    res = {"csrc_sha256": csrc_sha256(), "width": W, "height": H, "rays": W * H, "warmups": WARM, "timed_calls": TIMED,
           "method": "medians of HIP-event times, the one-launch call and the baseline alternating in one loop; two runs"}
    if args.parent_lib:
        res["headline"] = headline(args.parent_lib, log)
    graft.load_package()
    from raytracing_amd.pyhost import mirt, scene
    res["library"] = os.path.basename(mirt.LIB_PATH)
    golden = os.path.join(ROOT, "tests", "golden")
    cornell = scene.PackedScene(open(os.path.join(golden, "scene_cornell_1920x1080_r256.json")).read()).resized(W, H, 4)
    fx = np.load(os.path.join(golden, "cornell_teapot3_32x24_r4.npz"))
    teapot3 = scene.PackedScene(json.loads(bytes(fx["scene_json"]).decode())).resized(W, H, 4)
    ctx = mirt.Context(0)
    ctx.set_fusion(0)
    res["runs"] = []
    ok = True
    for run in range(2):
        rec = {}
        for name, ps in (("cornell", cornell), ("cornell_teapot3", teapot3)):
            coherent = pinhole_rays(ps)
            kinds = {"coherent": coherent, "permuted": coherent[np.random.default_rng(2025).permutation(len(coherent))], "axis": axis_rays(ps)}
            dev = mirt.DeviceScene(ctx, ps)
            rec[name] = measure(ctx, dev, ps, kinds)
            dev.release()
            log(f"run {run + 1} {name}: " + json.dumps(rec[name]))
        met = all(rec[s][k][q]["one_launch_not_above_baseline"] for s in rec for k in ("coherent", "permuted") for q in ("closest", "occluded"))
        rec["condition_met"] = met
        ok = ok and met
        res["runs"].append(rec)
    ctx.destroy()
    res["condition_met_in_both_runs"] = ok
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
