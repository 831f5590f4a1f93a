#!/usr/bin/env python3
"""tests/view_batch_default_child.py -- run by tests/test_view_batch_default.py in a process of its own with MIRT_CONTRACT=default, so that pyhost
loads libmirt_default.so.  The batch has the single call's ONE contract: mirt_view_rays_batch of that library equals the numpy restatement
per camera, and mirt_render_view_batch equals that library's OWN N single mirt_render_view calls in seeds, radiance and pixel -- both
fixtures x three models at 13 x 7, k = 2, N = 3, bounces 2, with the optimistic / exact pair and under set_exact_only.  Prints one JSON object
per case; exits non-zero on the first difference, naming it."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import __graft_entry__ as graft  # noqa: E402
import a10_pass as A  # noqa: E402
import view_batch_common as VB  # noqa: E402
import view_common as V  # noqa: E402
from conftest import bits, load_fixture  # noqa: E402

FIXTURES, MODELS, N, BOUNCES = ("cornell_32x24_r4", "cornell_teapot3_32x24_r4"), ("ortho", "equirect", "fisheye"), 3, 2


def main():
    graft.load_package()
    from raytracing_amd.pyhost import mirt
    assert os.path.basename(mirt.LIB_PATH) == "libmirt_default.so", mirt.LIB_PATH
    ctx = mirt.Context(0)
    try:
        for name in FIXTURES:
            _, sc = load_fixture(name)
            cams = VB.cameras(sc, N)
            r = VB.BatchRenderer(ctx, sc, N * 13 * 7 * 4, N * 13 * 7)
            try:
                for model in MODELS:
                    v = V.standard_view(sc, model, tone=0.25)
                    total = N * v.n_rays
                    buf = ctx.buffer(total * 32)
                    try:
                        ctx.view_rays_batch(v.desc(), cams, buf)
                        got = buf.read(np.float32).reshape(-1, 8)
                    finally:
                        buf.release()
                    bad = np.flatnonzero((bits(got) != bits(VB.batch_rays(v, cams))).any(axis=1))
                    d = f"{bad.size} of {total} rays differ; first is ray {int(bad[0])}" if bad.size else None
                    print(json.dumps({"case": f"rays {name} {model}", "ok": d is None, "difference": d}), flush=True)
                    if d:
                        return 1
                    seeds = A.make_seeds(total)
                    for exact_only in (False, True):
                        ctx.set_exact_only(exact_only)
                        want = r.singles(v, cams, seeds, bounces=BOUNCES)
                        got = r.run_batch(v, cams, seeds, bounces=BOUNCES)
                        d = V.differ(f"frames {name} {model} exact_only={exact_only}", got, want)
                        if d is None and not got[3]:
                            d = "bytes behind the records were written"
                        print(json.dumps({"case": f"frames {name} {model} exact_only={exact_only}", "ok": d is None, "difference": d,
                                          "lit": int((got[1][:, 3] > 0).sum()), "advanced": int((got[0] != seeds).sum())}), flush=True)
                        if d:
                            return 1
                    ctx.set_exact_only(False)
            finally:
                r.release()
    finally:
        ctx.destroy()
    return 0


if __name__ == "__main__":
    sys.exit(main())
