#!/usr/bin/env python3
"""tests/view_ao_child.py -- run by tests/test_view_ao_default.py in a process of its own with MIRT_CONTRACT=default, so that pyhost loads
libmirt_default.so: mirt_view_ao of the library built for the reference's own build options against the reference's code.cl compiled the same
way (oracle/_ref/a10_gfx950_default.hsaco), device against device.  Both fixtures x three models at 13 x 7, k = 2, 3 AO rays, radius 1.0, with
the pair and with the exact kernel alone: the restatement of tests/view_ao_common.py with the reference binary as the checker -- its closest-hit
kernels, bouncePaths three times, its shadow kernels -- on the rays that library's own mirt_view_rays writes (the reference has no such camera;
the contract decides how their divisions round).  Prints one JSON object per case; exits non-zero on the first difference, naming it."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402
import ref_gpu as G  # noqa: E402
import view_ao_common as VA  # noqa: E402
import view_common as V  # noqa: E402

DEFAULT_HSACO = os.path.join(ROOT, "oracle", "_ref", "a10_gfx950_default.hsaco")


def main():
    graft.load_package()
    from raytracing_amd.pyhost import mirt
    assert os.path.basename(mirt.LIB_PATH) == "libmirt_default.so", mirt.LIB_PATH
    ctx = mirt.Context(0)
    try:
        for name in VA.FIXTURES:
            sc = VA.scene(name)
            ao = VA.Ao(ctx, sc, 13 * 7 * 4, 13 * 7)
            try:
                for model in VA.MODELS:
                    v = V.standard_view(sc, model)
                    rb = ctx.buffer(v.n_rays * 32)
                    k = G.GpuRefKernels(DEFAULT_HSACO)
                    try:
                        ctx.view_rays(v.desc(), rb)
                        want = VA.expected(sc, v, VA.SAMPLES, 1.0, VA.BIAS, k=k, rays=rb.read(np.float32).reshape(-1, 8))
                    finally:
                        k.release()
                        rb.release()
                    d = VA.not_vacuous(f"{name} {model} by the reference's default build", want, VA.SAMPLES, v.rpp)
                    for exact_only in (False, True):
                        if d:
                            break
                        ctx.set_exact_only(exact_only)
                        try:
                            got, clean = ao.run(v)
                        finally:
                            ctx.set_exact_only(False)
                        d = VA.difference(f"{name} {model} exact_only={exact_only}", got, want)
                        if d is None and not clean:
                            d = f"{name} {model} exact_only={exact_only}: the bytes behind ao_out, or the seeds, were written"
                    print(json.dumps({"case": f"{name} {model}", "ok": d is None, "difference": d, "open": int(want[:, 0].sum()), "cast": int(want[:, 1].sum())}), flush=True)
                    if d:
                        return 1
            finally:
                ao.release()
    finally:
        ctx.destroy()
    return 0


if __name__ == "__main__":
    sys.exit(main())
