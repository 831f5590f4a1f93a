#!/usr/bin/env python3
"""tests/view_default_child.py -- run by tests/test_view_default.py in a process of its own with MIRT_CONTRACT=default, so that pyhost loads
libmirt_default.so (the reference's own build options: AMD's default division and sqrt).  The view cameras have ONE contract: mirt_view_rays of
that library equals the numpy restatement (tests/view_common.py) bit for bit for the three models at 13 x 7 with k = 1, 2, 4, 8, 16, at 1 x 1
and at 65 x 1 with k = 2; and mirt_render_view equals that library's OWN composition -- its mirt_view_rays, its mirt_trace_radiance, then the
numpy fold and tone map -- on cornell_32x24_r4, equirect, at every k, with the optimistic / exact pair and under set_exact_only.  Prints one JSON
object per case; exits non-zero on the first difference, naming it."""
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
import view_common as V  # noqa: E402
from conftest import bits, load_fixture  # noqa: E402

NAME, BOUNCES = "cornell_32x24_r4", 2
SIZES = [(13, 7, k) for k in V.KS] + [(1, 1, 1), (65, 1, 2)]


def main():
    graft.load_package()
    from raytracing_amd.pyhost import mirt
    assert os.path.basename(mirt.LIB_PATH) == "libmirt_default.so", mirt.LIB_PATH
    _, sc = load_fixture(NAME)
    ctx = mirt.Context(0)
    try:
        for model in ("ortho", "equirect", "fisheye"):
            for width, height, k in SIZES:
                v = V.standard_view(sc, model, width=width, height=height, k=k, t_min=0.03125, t_max=1000.0)
                n, tail = v.n_rays, 96
                buf = ctx.buffer(n * 32 + tail)
                try:
                    buf.write(np.full(buf.nbytes, V.SENTINEL, np.uint8))
                    ctx.view_rays(v.desc(), buf)
                    raw = buf.read(np.uint8)
                finally:
                    buf.release()
                got, want = raw[:n * 32].view(np.float32).reshape(-1, 8), V.view_rays(v)
                bad = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
                d = None
                if bad.size:
                    d = f"{bad.size} of {n} rays differ; first is ray {int(bad[0])}: got {got[bad[0]].tolist()}, want {want[bad[0]].tolist()}"
                elif not (raw[n * 32:] == V.SENTINEL).all():
                    d = "bytes behind the records were written"
                print(json.dumps({"case": f"rays {model} {width}x{height} k={k}", "ok": d is None, "difference": d}), flush=True)
                if d:
                    return 1
        r = V.Renderer(ctx, sc, 13 * 7 * 256, 13 * 7)
        try:
            for k in V.KS:
                v = V.standard_view(sc, "equirect", k=k, tone=1.0 / (k * k))
                n = v.n_rays
                seeds = A.make_seeds(n)
                rays, sd, acc = ctx.buffer(n * 32), ctx.buffer(n * 4), ctx.buffer(n * 16)
                try:
                    sd.write(seeds)
                    ctx.view_rays(v.desc(), rays)
                    ctx.trace_radiance(r.scene_desc(BOUNCES), rays, n, sd, acc, samples=1, flags=0)
                    sums = V.fold(acc.read(np.float32).reshape(-1, 4), v.rpp)
                    want = (sd.read(np.int32), sums, V.tone_rgba8(sums, v.tone))
                finally:
                    for b in (rays, sd, acc):
                        b.release()
                for exact_only in (False, True):
                    ctx.set_exact_only(exact_only)
                    got = r.run(v, seeds, bounces=BOUNCES)
                    d = V.differ(f"frame k={k} exact_only={exact_only}", got, want)
                    if d is None and not got[3]:
                        d = f"frame k={k} exact_only={exact_only}: bytes behind the records were written"
                    if d:
                        print(json.dumps({"case": f"frame k={k}", "ok": False, "difference": d}), flush=True)
                        return 1
                ctx.set_exact_only(False)
                print(json.dumps({"case": f"frame k={k}", "ok": True, "lit": int((sums[:, 3] > 0).sum()), "advanced": int((want[0] != seeds).sum())}), flush=True)
        finally:
            r.release()
    finally:
        ctx.destroy()
    return 0


if __name__ == "__main__":
    sys.exit(main())
