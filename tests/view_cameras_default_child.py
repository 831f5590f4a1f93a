#!/usr/bin/env python3
"""tests/view_cameras_default_child.py -- run by tests/test_view_cameras_default.py in a process of its own with MIRT_CONTRACT=default, so that
pyhost loads libmirt_default.so (the reference's own build options: AMD's default division and sqrt).  The axis_*, rim_* and mixed_k2 cameras of
tests/view_cameras_common.py on the `staged` and `single_cell` scenes: mirt_view_rays equals the numpy restatement (the view cameras have ONE
contract), and mirt_render_view equals that library's own KERNEL-BY-KERNEL path (radiance_common.kernel_by_kernel: the mirt_enqueue sequence of
executeRender, which existing tests pin to the reference's default build; the CPU oracle restates the correctly rounded contract only) on the
restated rays, then the numpy fold and tone map -- under the optimistic / exact pair and under set_exact_only.  mirt_view_deferred is at least
256 x the blocks that hold a primary ray the guard refuses.  Prints one JSON object per case; exits non-zero on the first difference, naming it."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import __graft_entry__ as graft  # noqa: E402
import radiance_common as RC  # noqa: E402
import rays_common as R  # noqa: E402
import view_cameras_common as VC  # noqa: E402
import view_common as V  # noqa: E402
from conftest import bits  # noqa: E402

STRATA = ("staged", "single_cell")
NAMES = VC.AXIS + VC.RIM + ("mixed_k2",)


def main():
    graft.load_package()
    from raytracing_amd.pyhost import mirt
    assert os.path.basename(mirt.LIB_PATH) == "libmirt_default.so", mirt.LIB_PATH
    ctx = mirt.Context(0)
    ctx.set_fusion(0)
    try:
        for stratum in STRATA:
            sc = R.scene(stratum)
            cap_rays = max(VC.view(stratum, n).n_rays for n in NAMES)
            r = V.Renderer(ctx, sc, cap_rays, max(VC.view(stratum, n).n_pixels for n in NAMES))
            buf = ctx.buffer(cap_rays * 32 + 96)
            try:
                for name in NAMES:
                    case = f"{stratum} {name}"
                    v = VC.view(stratum, name)
                    n = v.n_rays
                    rays, seeds = V.view_rays(v), VC.seeds_of(n)
                    buf.write(np.full(buf.nbytes, V.SENTINEL, np.uint8))
                    ctx.view_rays(v.desc(), buf)
                    raw = buf.read(np.uint8)
                    got = raw[:n * 32].view(np.float32).reshape(-1, 8)
                    bad = np.flatnonzero((bits(got) != bits(rays)).any(axis=1))
                    d = None
                    if bad.size:
                        d = f"{bad.size} of {n} rays differ; first is ray {int(bad[0])}: got {got[bad[0]].tolist()}, want {rays[bad[0]].tolist()}"
                    elif not (raw[n * 32:] == V.SENTINEL).all():
                        d = "bytes behind the ray records were written"
                    if d:
                        print(json.dumps({"case": case, "ok": False, "difference": d}), flush=True)
                        return 1
                    acc, sd = RC.kernel_by_kernel(ctx, r.dev, sc, rays, seeds, 1, VC.BOUNCES)
                    sums = V.fold(acc, v.rpp)
                    want = (sd, sums, V.tone_rgba8(sums, v.tone))
                    refused = VC.blocks_of(R.live(rays) & ~R.guard_accepts(rays))
                    deferred = None
                    for exact_only in (False, True):
                        ctx.set_exact_only(exact_only)
                        out = r.run(v, seeds, bounces=VC.BOUNCES)
                        d = V.differ(f"{case} exact_only={exact_only}", out, want)
                        if d is None and not out[3]:
                            d = f"{case} exact_only={exact_only}: bytes behind the records were written"
                        if d is None and not exact_only:
                            deferred = ctx.view_deferred()
                            if deferred < 256 * len(refused):
                                d = f"{case}: {deferred} rays deferred, {len(refused)} blocks hold a primary ray the guard refuses"
                        if d:
                            ctx.set_exact_only(False)
                            print(json.dumps({"case": case, "ok": False, "difference": d}), flush=True)
                            return 1
                    ctx.set_exact_only(False)
                    with np.errstate(invalid="ignore"):
                        lit = int((sums[:, 3] > 0).sum())
                    print(json.dumps({"case": case, "ok": True, "rays": n, "lit": lit, "advanced": int((sd != seeds).sum()), "deferred": int(deferred),
                                      "refused_blocks": int(len(refused)), "blocks": VC.n_blocks(v)}), flush=True)
            finally:
                buf.release()
                r.release()
    finally:
        ctx.destroy()
    return 0


if __name__ == "__main__":
    sys.exit(main())
