#!/usr/bin/env python3
"""tests/ao_default_child.py -- run by tests/test_ao.py in a process of its own with MIRT_CONTRACT=default, so that pyhost loads
libmirt_default.so: mirt_render_ao of the library built for the reference's own build options against the reference's code.cl compiled the same
way (oracle/_ref/a10_gfx950_default.hsaco), device against device.  cornell_teapot3 at 96x54 x 16, 2 AO rays per hit sample: the restatement of
tests/ao_common.py (initTrace, the closest-hit kernels, bouncePaths twice, the shadow kernels on the rewritten rays), with the pair and with the
exact kernel alone.  Prints one JSON object; exits non-zero on the first difference, naming it."""
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
from ao_common import Ao, difference, expected_ao  # noqa: E402
from conftest import load_fixture  # noqa: E402

DEFAULT_HSACO = os.path.join(ROOT, "oracle", "_ref", "a10_gfx950_default.hsaco")
NAME, SIZE, SAMPLES, RADIUS, BIAS = "cornell_teapot3_32x24_r4", (96, 54, 16), 2, 1.0, 0.001   # as test_ao.py's case against the reference binary


def main():
    graft.load_package()
    from raytracing_amd.pyhost import mirt, scene
    assert os.path.basename(mirt.LIB_PATH) == "libmirt_default.so", mirt.LIB_PATH
    _, sc0 = load_fixture(NAME)
    ps = scene.PackedScene(dict(sc0.d)).resized(*SIZE)
    k = G.GpuRefKernels(DEFAULT_HSACO)
    ctx = mirt.Context(0)
    ao = Ao(ctx, ps)
    try:
        want = expected_ao(k, A.Scene(ps.d), SAMPLES, RADIUS, BIAS)
        for exact_only in (False, True):
            ctx.set_exact_only(exact_only)
            got, _ = ao.run(SAMPLES, RADIUS, BIAS)
            d = difference(f"{NAME} exact_only={exact_only}", got, want)
            if d:
                print(json.dumps({"scene": NAME, "ok": False, "difference": d}), flush=True)
                return 1
        print(json.dumps({"scene": NAME, "ok": True, "pixels": int(want.shape[0]), "open": int(want[:, 0].sum()), "cast": int(want[:, 1].sum())}), flush=True)
    finally:
        k.release()
        ao.release()
        ctx.destroy()
    return 0


if __name__ == "__main__":
    sys.exit(main())
