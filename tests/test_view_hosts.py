"""The hosts of mirt_view_rays / mirt_render_view:

  * pyhost/rays.py render_view with cuda tensors on a non-default torch stream equals the Buffer path byte for byte, seeds included, fresh and
    continued;
  * the Node binding (queue.renderView) through `cli.js render ... --view equirect` at 13 x 7 x 4, two progressive passes, writes the bytes
    Python's Context.render_view gives, and `cli.js trace ... --view-rays` the rays of Context.view_rays (skipped without node, as the other
    JavaScript tests are);
  * the symbols appear in `nm -D` of both libraries, in pyhost/mirt.py's table and in the addon.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import a10_pass as A
import view_common as V
from conftest import HOST, PAGE, ROOT, load_fixture

PKG_DIR = os.path.join(ROOT, "2015-raytracing_amd")
SYMBOLS = ("mirt_view_rays", "mirt_render_view", "mirt_view_deferred")
node = shutil.which("node")
W, H, K = 13, 7, 2


def box_centre(sc):
    b = np.asarray(sc.bounds, np.float64)
    return [(float(b[c]) + float(b[4 + c])) / 2 for c in range(3)]


@pytest.mark.gpu
def test_torch_tensors_on_a_side_stream_equal_the_buffer_path(pkg):
    import torch
    from raytracing_amd.pyhost import mirt, rays as prays
    _, sc = load_fixture("cornell_teapot3_32x24_r4")
    v = V.standard_view(sc, "fisheye", tone=0.25)
    seeds = A.make_seeds(v.n_rays)
    ctx = mirt.Context(0)
    r = V.Renderer(ctx, sc, v.n_rays, v.n_pixels)
    try:
        first = r.run(v, seeds, bounces=2)
        second = r.run(v.with_(tone=0.125), first[0], bounces=2, carry=first[1])
        assert (second[1][:, 3] > 0).any()
        side = torch.cuda.Stream(device=0)
        with torch.cuda.stream(side):
            st = torch.from_numpy(seeds.copy()).to("cuda:0")
            rad, px = prays.render_view(ctx, r.dev, v.desc(), st, bounces=2, want_pixel=True)
            got = (st.cpu().numpy(), rad.cpu().numpy(), px.cpu().numpy())
            again = prays.render_view(ctx, r.dev, v.with_(tone=0.125).desc(), st, bounces=2, accumulate_into=rad)
            assert again is rad
            got2 = (st.cpu().numpy(), again.cpu().numpy())
        side.synchronize()
        assert got[1].shape == (v.n_pixels, 4) and got[1].dtype == np.float32 and got[2].dtype == np.uint8
        assert got[0].tobytes() == first[0].tobytes() and got[1].tobytes() == first[1].tobytes() and got[2].tobytes() == first[2].tobytes()
        assert got2[0].tobytes() == second[0].tobytes() and got2[1].tobytes() == second[1].tobytes()
        # the context is back on its own stream and works as before
        assert r.run(v, seeds, bounces=2)[1].tobytes() == first[1].tobytes()
        with pytest.raises(ValueError):
            prays.render_view(ctx, r.dev, v.desc(), torch.zeros((4,), dtype=torch.int32, device="cuda:0"))
        with pytest.raises(ValueError):
            prays.render_view(ctx, r.dev, v.desc(), st.to(torch.int64))
    finally:
        r.release()
        ctx.destroy()


@pytest.mark.gpu
@pytest.mark.skipif(node is None, reason="node is not installed")
def test_cli_render_view_writes_the_bytes_the_python_call_does(pkg, tmp_path):
    """the fixture's scene_json is what the JavaScript host packs from tests/scenes/page/scenes/gems.xml; cli.js reaches the library through the
    Node binding (queue.renderView, queue.viewRays) and takes its seeds from mirt_seed_fill(0, count, 0), which a10_pass.make_seeds restates"""
    from raytracing_amd.pyhost import mirt
    _, sc = load_fixture("own_gems_48x36_r4")
    eye = box_centre(sc)
    look = [eye[0] + 0.3, eye[1] - 0.2, eye[2] - 1.0]
    n, npx = W * H * K * K, W * H
    ctx = mirt.Context(0)
    dev = mirt.DeviceScene(ctx, sc)
    sb, rb, pb, yb = ctx.buffer(n * 4), ctx.buffer(npx * 16), ctx.buffer(npx * 4), ctx.buffer(n * 32)
    try:
        sb.write(A.make_seeds(n))
        for p in (1, 2):
            d = mirt.view_desc("equirect", W, H, k=K, eye=eye, look_at=look, tone=1.0 / (K * K * p), flags=mirt.VIEW_ACCUMULATE if p > 1 else 0)
            ctx.render_view(dev.pass_desc(None, None, bounces=5), d, sb, rb, pb)
        want_px, want_rad = pb.read(np.uint8).reshape(-1, 4), rb.read(np.float32).reshape(-1, 4)
        ctx.view_rays(mirt.view_desc("fisheye", W, H, k=K, eye=eye, look_at=look, half_angle=np.float32(100.0 / 2 * np.pi / 180)), yb)
        want_rays = yb.read(np.float32)
    finally:
        for b in (sb, rb, pb, yb):
            b.release()
        dev.release()
        ctx.destroy()
    assert (want_rad[:, 3] > 0).any() and len(np.unique(want_px[:, 0:3], axis=0)) > 4, "the panorama is blank"
    xml = os.path.join(PAGE, "scenes", "gems.xml")
    out = str(tmp_path / "pano.ppm")
    cam = ["--look", ",".join(repr(c) for c in look)]
    r = subprocess.run([node, os.path.join(HOST, "cli.js"), "render", xml, str(W), str(H), str(K * K), "2", out, "--view", "equirect"] + cam, capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    ppm = open(out, "rb").read()
    header = f"P6\n{W} {H}\n255\n".encode()
    assert ppm.startswith(header) and ppm[len(header):] == want_px[:, 0:3].tobytes(), "pixels"
    assert open(out + ".radiance.f32", "rb").read() == want_rad.tobytes(), "radiance sums"
    rf = str(tmp_path / "rays.f32")
    r = subprocess.run([node, os.path.join(HOST, "cli.js"), "trace", xml, f"{W}x{H}x{K * K}", rf, "--view-rays", "--view", "fisheye", "--fov", "100"] + cam, capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert open(rf, "rb").read() == want_rays.tobytes(), "the rays of --view-rays"
    # --view is refused with what is not built for these cameras
    for flag in (["--gpus", "2"], ["--guides", str(tmp_path / "g")], ["--denoise"], ["--upscale", "2"], ["--ao", str(tmp_path / "a")]):
        r = subprocess.run([node, os.path.join(HOST, "cli.js"), "render", xml, str(W), str(H), str(K * K), "1", out, "--view", "equirect"] + flag, capture_output=True)
        assert r.returncode == 2 and b"--view is not available with" in r.stderr, (flag, r.stderr.decode())


def test_the_symbols_are_in_the_header_the_libraries_the_binding_and_the_addon(pkg):
    from raytracing_amd.pyhost import mirt, rays as prays
    header = open(os.path.join(ROOT, "include", "mirt.h")).read()
    for lib in ("libmirt.so", "libmirt_default.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG_DIR, lib)], capture_output=True, text=True, check=True).stdout
        exported = set(re.findall(r"\bT (mirt_\w+)", out))
        for s in SYMBOLS:
            assert s in exported, (lib, s)
    for s in SYMBOLS:
        assert re.search(r"MIRT_API\s+int\s+" + s + r"\s*\(", header), s
        assert s in mirt.SYMBOLS and hasattr(mirt.lib(), s), s
    assert re.search(r"typedef struct mirt_view_desc \{[^}]*\} mirt_view_desc;", header)
    for name, value in (("MIRT_VIEW_ORTHOGRAPHIC", mirt.VIEW_ORTHOGRAPHIC), ("MIRT_VIEW_EQUIRECT", mirt.VIEW_EQUIRECT), ("MIRT_VIEW_FISHEYE", mirt.VIEW_FISHEYE),
                        ("MIRT_VIEW_ACCUMULATE", mirt.VIEW_ACCUMULATE)):
        assert int(re.search(r"#define " + name + r"\s+(\d+)u", header).group(1)) == value, name
    import ctypes as C
    assert C.sizeof(mirt._ViewDesc) == 104
    for method in ("view_rays", "render_view", "view_deferred"):
        assert callable(getattr(mirt.Context, method))
    assert callable(prays.render_view) and callable(mirt.view_desc)
    napi = open(os.path.join(PKG_DIR, "csrc", "addon", "mirt_napi.cc")).read()
    for js, s in zip(("viewRays", "renderView", "viewDeferred"), SYMBOLS):
        assert f'{{"{js}", ' in napi and s + "(" in napi, js
    addon = os.path.join(PKG_DIR, "mirt.node")
    if os.path.exists(addon):   # built where the Node headers are (csrc/addon/build_addon.sh)
        out = subprocess.run(["nm", "-D", "--undefined-only", addon], capture_output=True, text=True, check=True).stdout
        for s in SYMBOLS:
            assert re.search(r"\bU " + s + r"\b", out), ("mirt.node", s)
