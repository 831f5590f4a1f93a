#!/usr/bin/env python3
"""tests/frame_aa_child.py -- run by tests/test_frame_aa.py in a process of its own, with MIRT_CONTRACT=default so that pyhost loads
libmirt_default.so: every job of test_frame_aa.JOBS at 37 x 23 pixels and 2, 3 and 4 samples per axis through mirt_render_frame_aa against the box
average (tests/frame_aa_common.py) of the fine frame THIS library's mirt_render_frame renders.  One JSON object per frame; exits non-zero on the
first difference."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import __graft_entry__ as graft  # noqa: E402
from frame_aa_common import AAS, box, coarse_job, fine_job  # noqa: E402


def main():
    graft.load_package()
    from raytracing_amd.pyhost import mirt, render
    from test_frame_aa import JOBS
    from test_frame_one_launch import both_job
    from test_frames import fixture
    W, H = 37, 23
    ctx = mirt.Context(0)
    try:
        for name in JOBS:
            d = both_job(ctx, "frame_a07_own_octahedra_n3_96x64", "frame_a07_own_mol_helix_n3_96x64") if name == "both" else fixture(name)[1]
            for aa in AAS:
                fine, _ = render.render_frame_one_launch(ctx, render.FramePacked(fine_job(d, W, H, aa)))
                got, _ = render.render_frame_one_launch(ctx, render.FramePacked(coarse_job(d, W, H)), aa=aa)
                want = box(fine, W, H, aa)
                ok = bool(np.array_equal(got, want))
                print(json.dumps({"frame": name, "aa": aa, "ok": ok, "pixels_differ": int((got != want).any(axis=1).sum()), "lit": int((want[:, :3].max(axis=1) > 0).sum()),
                                  "library": os.path.basename(mirt.LIB_PATH)}), flush=True)
                if not ok:
                    return 1
        return 0
    finally:
        ctx.destroy()


if __name__ == "__main__":
    sys.exit(main())
