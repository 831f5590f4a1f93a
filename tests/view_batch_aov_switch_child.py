#!/usr/bin/env python3
"""tests/view_batch_aov_switch_child.py FIXTURE -- run by tests/test_view_guided_batch.py in a process of its own with MIRT_GUIDED_VIEW=0: one
mirt_render_view_guided_batch call (FISHEYE, 13 x 7, k = 2, N = 3, bounces 2, tone 0.25, seeds make_seeds) on the two-launch route.  Prints one
JSON object: by how much mirt_ctx_guided_views rose, and a SHA-256 over seeds, radiance, pixel, normal_hits and albedo_depth."""
import hashlib
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
import view_batch_aov_common as BA  # noqa: E402
import view_batch_common as VB  # noqa: E402
import view_common as V  # noqa: E402


def main():
    graft.load_package()
    from raytracing_amd.pyhost import mirt
    sc = BA.scene(sys.argv[1])
    ctx = mirt.Context(0)
    r = BA.Aov(ctx, sc)
    try:
        v = V.standard_view(sc, "fisheye", tone=0.25)
        before = ctx.guided_views()
        got = r.guided_batch(v, VB.cameras(sc, BA.N), A.make_seeds(BA.N * v.n_rays))
        routed = ctx.guided_views() - before
        h = hashlib.sha256()
        for a in got[0][:3] + got[1][:2]:
            h.update(np.ascontiguousarray(a).tobytes())
        print(json.dumps({"routed": routed, "digest": h.hexdigest(), "clean": bool(got[0][3] and got[1][2])}), flush=True)
        return 0 if got[0][3] and got[1][2] else 1
    finally:
        r.release()
        ctx.destroy()


if __name__ == "__main__":
    sys.exit(main())
