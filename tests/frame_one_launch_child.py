#!/usr/bin/env python3
"""tests/frame_one_launch_child.py -- run by tests/test_frame_one_launch.py in a process of its own.
  default          (with MIRT_CONTRACT=default, so that pyhost loads libmirt_default.so) every Assign04 / Assign07 fixture through mirt_render_frame
                   against the reference's code.cl built with ITS defaults (oracle/_ref/a0N_gfx950_default.hsaco, frame_pass.run_frame_gpu): every pixel
                   and every ray's maxt.  One JSON object per frame; exits non-zero on the first difference.
  frames NAME N    N frames of one fixture through mirt_render_frame without a ray buffer and nothing else on the device: what a kernel trace of this
                   process must show is N launches of one kernel."""
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import __graft_entry__ as graft  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def fixture(name):
    fx = np.load(os.path.join(GOLDEN, name + ".npz"))
    return fx, json.loads(bytes(fx["frame_json"]).decode())


def main():
    graft.load_package()
    from raytracing_amd.pyhost import mirt, render
    ctx = mirt.Context(0)
    try:
        if sys.argv[1] == "frames":
            _, d = fixture(sys.argv[2])
            f = render.FrameOneLaunch(ctx, render.FramePacked(d))
            for _ in range(int(sys.argv[3])):
                f.render()
            ctx.finish()
            px = f.pixels.read(np.uint8)
            f.release()
            print(json.dumps({"frames": int(sys.argv[3]), "lit": int((px.reshape(-1, 4)[:, :3].max(axis=1) > 0).sum())}))
            return 0
        import a10_pass as A
        import frame_pass as F
        for path in sorted(glob.glob(os.path.join(GOLDEN, "frame_a0[47]_*.npz"))):
            name = os.path.basename(path)[:-4]
            _, d = fixture(name)
            want_px, want_rays = F.run_frame_gpu(F.Frame(d), default_build=True)
            px, rays = render.render_frame_one_launch(ctx, render.FramePacked(d), keep_rays=True)
            got = np.ascontiguousarray(rays).view(A.RAY_DT)
            g, w = got["maxt"].view(np.uint32), np.ascontiguousarray(want_rays["maxt"]).view(np.uint32)
            ok = bool(np.array_equal(px, want_px)) and bool(np.array_equal(g, w))
            print(json.dumps({"frame": name, "ok": ok, "pixels_differ": int((px != want_px).any(axis=1).sum()), "maxt_differ": int((g != w).sum())}), flush=True)
            if not ok:
                return 1
        return 0
    finally:
        ctx.destroy()


if __name__ == "__main__":
    sys.exit(main())
