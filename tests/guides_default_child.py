#!/usr/bin/env python3
"""tests/guides_default_child.py -- run by tests/test_guides.py in a process of its own with MIRT_CONTRACT=default, so that pyhost loads
libmirt_default.so: mirt_render_guides of the library built for the reference's own build options against the reference's code.cl compiled the same
way (oracle/_ref/a10_gfx950_default.hsaco), device against device.  cornell and cornell_teapot3 at 480x270 x 16: initTrace and the closest-hit
kernels of the reference, reduced per pixel in sample order.  Prints one JSON object per scene; exits non-zero on the first difference, naming it."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402
import a10_pass as A  # noqa: E402
import ref_gpu as G  # noqa: E402
from conftest import load_fixture  # noqa: E402
from guides_common import difference, expected_guides  # noqa: E402

DEFAULT_HSACO = os.path.join(ROOT, "oracle", "_ref", "a10_gfx950_default.hsaco")


def main():
    graft.load_package()
    from raytracing_amd.pyhost import mirt, render, scene
    assert os.path.basename(mirt.LIB_PATH) == "libmirt_default.so", mirt.LIB_PATH
    for name in ("cornell_32x24_r4", "cornell_teapot3_32x24_r4"):
        _, sc0 = load_fixture(name)
        ps = scene.PackedScene(dict(sc0.d)).resized(480, 270, 16)
        k = G.GpuRefKernels(DEFAULT_HSACO)
        ctx = mirt.Context(0)
        fr = render.FusedRenderer(ctx, ps)
        try:
            want = expected_guides(k, A.Scene(ps.d))
            for exact_only in (False, True):
                ctx.set_exact_only(exact_only)
                got = fr.guides()
                for tag, g, w in (("normal_hits", got[0], want[0]), ("albedo_depth", got[1], want[1])):
                    d = difference(f"{name} exact_only={exact_only} {tag}", g, w)
                    if d:
                        print(json.dumps({"scene": name, "ok": False, "difference": d}), flush=True)
                        return 1
            print(json.dumps({"scene": name, "ok": True, "pixels": int(want[0].shape[0])}), flush=True)
        finally:
            k.release()
            fr.release()
            ctx.destroy()
    return 0


if __name__ == "__main__":
    sys.exit(main())
