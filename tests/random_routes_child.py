#!/usr/bin/env python3
"""tests/random_routes_child.py <waves> -- run by tests/test_random_scene_routes.py in a process of its own under MIRT_GRID_WAVES=<waves> (read once
per process).  5: the 5-wave build of the optimistic grid kernels on the generated `staged` and `unstaged` scenes (tests/random_scenes_common.py),
37 x 21 x 4 rays, through the routes ordinary, passes n = 2, every frame and first pass guided, and the first scene of each at 289 rays per
pixel on 9 x 5 (the segment kernels, which no scene's own LDS arithmetic pairs with an unstaged 5-wave build).
6: the multi-pass cases among them on the 6-wave build, which launch_fused never pairs with primary-hit reuse on its own (with the reuse rows a grid kernel's block is 7232 + 13 568 + 8192 =
28 992 B of LDS at the least: 23 granules of 1280 B, five blocks a CU; tests/test_random_scene_routes.py asserts the arithmetic).  Each
case against the CPU oracle, with the optimistic pair and with the exact kernel alone.  Prints one JSON object per case; exits non-zero on the
first difference, naming it."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROUTES = ("ordinary", "passes", "every", "first_guided")
STRATA = ("staged", "unstaged")
W, H, RPP = 37, 21, 4


def _cases():
    import random_scenes_common as C
    return ([(s, seed, route, RPP) for s in STRATA for seed in C.SEEDS[s] for route in ROUTES] +
            [(s, C.SEEDS[s][0], route, 289) for s in STRATA for route in ("passes", "every", "first_guided")])


CASES = _cases()


def cases(waves):
    """6: the multi-pass routes alone -- the one-pass launches of these scenes run the 6-wave builds wherever launch_fused picks them itself"""
    return CASES if waves == "5" else [c for c in CASES if c[2] in ("passes", "every")]


def main(waves):
    import __graft_entry__ as graft
    import a10_pass as A
    import random_scenes_common as C
    graft.load_package()
    from raytracing_amd.pyhost import mirt
    assert os.environ.get("MIRT_GRID_WAVES") == waves
    ctx = mirt.Context(0)
    try:
        for stratum, seed, route, rpp in cases(waves):
            sc = C.scene(stratum, seed, *((9, 5) if rpp > 256 else (W, H)), rpp)
            seeds = A.make_seeds(sc.total_rays, seed_base=seed)
            for exact_only in (False, True):
                ctx.set_exact_only(exact_only)
                if route == "ordinary":
                    diffs = C.run_ordinary(ctx, sc, seeds)
                elif route == "first_guided":
                    diffs = C.run_first_guided(ctx, sc, seeds)
                else:
                    diffs = C.run_passes(ctx, sc, seeds, 2, every=(route == "every"))
                print(json.dumps({"stratum": stratum, "seed": seed, "route": route, "rpp": rpp, "exact_only": exact_only, "ok": not diffs, "difference": diffs[:1]}), flush=True)
                if diffs:
                    return 1
    finally:
        ctx.set_exact_only(False)
        ctx.destroy()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
