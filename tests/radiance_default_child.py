#!/usr/bin/env python3
"""tests/radiance_default_child.py -- run by tests/test_radiance_default.py in a process of its own with MIRT_CONTRACT=default, so that pyhost loads
libmirt_default.so (the reference's own build options: AMD's default division and sqrt).  mirt_trace_radiance of that library against ITS OWN
kernel-by-kernel path on the same rays and seeds -- 48-byte Ray / 64-byte Poi buffers filled per sample, then the mirt_enqueue sequence of
executeRender without initTrace and copyToPixel (tests/radiance_common.py kernel_by_kernel).  That path is what existing tests pin to the
reference's default build; the CPU oracle restates the correctly rounded contract only.  Every stratum of the random scenes at samples = 2,
bounces = 3, with the optimistic / exact pair and under set_exact_only.  Prints one JSON object per stratum; exits non-zero on the first
difference, naming it."""
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
from random_scenes_common import STRATA  # noqa: E402

SAMPLES, BOUNCES = 2, 3


def main():
    graft.load_package()
    from raytracing_amd.pyhost import mirt
    assert os.path.basename(mirt.LIB_PATH) == "libmirt_default.so", mirt.LIB_PATH
    ctx = mirt.Context(0)
    ctx.set_fusion(0)
    try:
        for stratum in STRATA:
            sc = R.scene(stratum)
            rays, _ = R.rays_of(stratum)
            seeds = RC.seeds_of(stratum)
            t = RC.RadianceTracer(ctx, sc)
            try:
                want = RC.kernel_by_kernel(ctx, t.dev, sc, rays, seeds, SAMPLES, BOUNCES)
                for exact_only in (False, True):
                    ctx.set_exact_only(exact_only)
                    acu, sd, tails = t.run(rays, seeds, samples=SAMPLES, bounces=BOUNCES)
                    d = RC.differ(f"{stratum} exact_only={exact_only}", (acu, sd), want)
                    if d is None and not (RC.untouched(tails[0]) and RC.untouched(tails[1])):
                        d = f"{stratum} exact_only={exact_only}: bytes behind the records were written"
                    if d:
                        print(json.dumps({"stratum": stratum, "ok": False, "difference": d}), flush=True)
                        return 1
                ctx.set_exact_only(False)
                with np.errstate(invalid="ignore"):
                    lit = int((want[0][:, 3] > 0).sum())
                print(json.dumps({"stratum": stratum, "ok": True, "rays": int(len(rays)), "lit": lit, "advanced": int((want[1] != seeds).sum())}), flush=True)
            finally:
                t.release()
    finally:
        ctx.destroy()
    return 0


if __name__ == "__main__":
    sys.exit(main())
