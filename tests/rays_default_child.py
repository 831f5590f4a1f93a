#!/usr/bin/env python3
"""tests/rays_default_child.py -- run by tests/test_rays_default.py in a process of its own with MIRT_CONTRACT=default, so that pyhost loads
libmirt_default.so (the reference's own build options: AMD's default division and sqrt).  mirt_trace_closest and mirt_trace_occluded of that library
against ITS OWN kernel-by-kernel path on the same rays -- a 48-byte Ray / 64-byte Poi buffer filled here, the mirt_enqueue sequence
GranularRenderer._closest issues, and the shadow kernels (tests/rays_common.py kernel_by_kernel).  That path is what existing tests pin to the
reference's default build; the CPU oracle restates the correctly rounded contract only.  Every stratum of the random scenes, with the optimistic /
exact pair and under set_exact_only.  Prints one JSON object per stratum; exits non-zero on the first difference, naming it."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import __graft_entry__ as graft  # noqa: E402
import rays_common as R  # noqa: E402
from random_scenes_common import STRATA  # noqa: E402


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
            t = R.Tracer(ctx, sc)
            try:
                want_hits, want_sets, want_occ = R.kernel_by_kernel(ctx, t.dev, sc, rays)
                for exact_only in (False, True):
                    ctx.set_exact_only(exact_only)
                    hits, sets, tails = t.closest(rays)
                    occ, tail = t.occluded(rays)
                    d = R.hits_differ(f"{stratum} exact_only={exact_only} hits", hits, want_hits)
                    if d is None and not np.array_equal(sets, want_sets):
                        d = f"{stratum} exact_only={exact_only}: sets differ at ray {int(np.flatnonzero(sets != want_sets)[0])}"
                    if d is None and not np.array_equal(occ, want_occ):
                        d = f"{stratum} exact_only={exact_only}: occluded differs at ray {int(np.flatnonzero(occ != want_occ)[0])}"
                    if d is None and not (R.untouched(tails[0]) and R.untouched(tails[1]) and R.untouched(tail)):
                        d = f"{stratum} exact_only={exact_only}: bytes behind the records were written"
                    if d:
                        print(json.dumps({"stratum": stratum, "ok": False, "difference": d}), flush=True)
                        return 1
                ctx.set_exact_only(False)
                hit = want_hits[:, 7].view(np.int32) >= 0
                print(json.dumps({"stratum": stratum, "ok": True, "rays": int(len(rays)), "hits": int(hit.sum()), "occluded": int(want_occ.sum())}), flush=True)
            finally:
                t.release()
    finally:
        ctx.destroy()
    return 0


if __name__ == "__main__":
    sys.exit(main())
