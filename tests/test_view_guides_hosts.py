"""The hosts of mirt_view_guides / mirt_render_view_guided:

  * pyhost/rays.py view_guides, render_view(want_guides=True) and denoised_view with cuda tensors equal the C-ABI calls on buffers composed with
    the numpy filter of tests/filter_common.py, byte for byte;
  * the Node binding: queue.renderViewGuided through `cli.js render ... --view fisheye --view-guides PREFIX --view-denoise` at 13 x 7 x 4, two
    progressive passes, writes the guides of Context.view_guides and the filtered picture of that Python chain; queue.viewGuides through
    tests/view_guides_node.js (renderer.viewGuidesFile), both outputs and each alone, writes the same guides; `--view ...
    --upscale` still exits 2, and so do `--guides` and `--denoise` beside `--view`: they are the thin-lens camera's flags (skipped without
    node, as the other JavaScript tests are);
  * the symbols appear in `nm -D` of both libraries, in pyhost/mirt.py's table and in the addon.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import a10_pass as A
import filter_common as F
import view_common as V
import view_guides_common as VG
from conftest import HOST, PAGE, ROOT, load_fixture

PKG_DIR = os.path.join(ROOT, "2015-raytracing_amd")
SYMBOLS = ("mirt_view_guides", "mirt_render_view_guided", "mirt_ctx_guided_views")
node = shutil.which("node")
W, H, K = 13, 7, 2


def box_centre(sc):
    b = np.asarray(sc.bounds, np.float64)
    return [(float(b[c]) + float(b[4 + c])) / 2 for c in range(3)]


@pytest.mark.gpu
def test_torch_tensors_equal_the_buffer_calls_and_the_numpy_filter(pkg):
    import torch
    from raytracing_amd.pyhost import mirt, rays as prays
    _, sc = load_fixture("cornell_teapot3_32x24_r4")
    v = V.standard_view(sc, "fisheye", tone=0.25)
    seeds = A.make_seeds(v.n_rays)
    ctx = mirt.Context(0)
    r = VG.Renderer(ctx, sc, v.n_rays, v.n_pixels)
    try:
        first, guides = r.two_calls(v, seeds, bounces=2)
        second = r.run(v.with_(tone=0.125), first[0], bounces=2, carry=first[1])
        assert (guides[0][:, 3] > 0).any() and (guides[0][:, 3] == 0).any() and (second[1][:, 3] > 0).any()
        nh, ad = prays.view_guides(ctx, r.dev, v.desc())
        assert nh.shape == (v.n_pixels, 4) and nh.dtype == torch.float32 and nh.is_cuda
        assert nh.cpu().numpy().tobytes() == guides[0].tobytes() and ad.cpu().numpy().tobytes() == guides[1].tobytes()
        st = torch.from_numpy(seeds.copy()).to("cuda:0")
        rad, px, nh2, ad2 = prays.render_view(ctx, r.dev, v.desc(), st, bounces=2, want_pixel=True, want_guides=True)
        assert (st.cpu().numpy().tobytes(), rad.cpu().numpy().tobytes(), px.cpu().numpy().tobytes()) == (first[0].tobytes(), first[1].tobytes(), first[2].tobytes())
        assert nh2.cpu().numpy().tobytes() == guides[0].tobytes() and ad2.cpu().numpy().tobytes() == guides[1].tobytes()
        # two progressive frames, then the filter with the shipped defaults and tone 1 / (rpp * passes)
        st = torch.from_numpy(seeds.copy()).to("cuda:0")
        filtered, pixel = prays.denoised_view(ctx, r.dev, v.desc(), st, passes=2, bounces=2)
        assert st.cpu().numpy().tobytes() == second[0].tobytes()
        want_f, want_p = F.atrous(second[1], guides[0], guides[1], v.width, v.height, 1.0 / (v.rpp * 2), **F.DEFAULTS)
        assert F.difference("denoised_view filtered", filtered.cpu().numpy(), want_f) is None
        assert np.array_equal(pixel.cpu().numpy(), want_p), "denoised_view pixel"
        assert not np.array_equal(want_f, second[1]), "the filter changed nothing"
        with pytest.raises(ValueError):
            prays.denoised_view(ctx, r.dev, v.tile(0, 3).desc(), st)
    finally:
        r.release()
        ctx.destroy()


@pytest.mark.gpu
@pytest.mark.skipif(node is None, reason="node is not installed")
def test_cli_view_guides_and_denoise_write_the_bytes_the_python_chain_does(pkg, tmp_path):
    """cli.js reaches the library through the Node binding (queue.renderViewGuided for pass 1, queue.renderView for pass 2, queue.filterFrame) and
    takes its seeds from mirt_seed_fill(0, count, 0), which a10_pass.make_seeds restates"""
    from raytracing_amd.pyhost import mirt
    _, sc = load_fixture("own_gems_48x36_r4")
    eye = box_centre(sc)
    look = [eye[0] + 0.3, eye[1] - 0.2, eye[2] - 1.0]
    n, npx = W * H * K * K, W * H
    ctx = mirt.Context(0)
    dev = mirt.DeviceScene(ctx, sc)
    sb, rb, pb, nb, ab, fb, fpb = (ctx.buffer(b) for b in (n * 4, npx * 16, npx * 4, npx * 16, npx * 16, npx * 16, npx * 4))
    try:
        sb.write(A.make_seeds(n))

        def view(p):
            return mirt.view_desc("fisheye", W, H, k=K, eye=eye, look_at=look, half_angle=np.float32(100.0 / 2 * np.pi / 180), tone=1.0 / (K * K * p),
                                  flags=mirt.VIEW_ACCUMULATE if p > 1 else 0)
        for p in (1, 2):
            ctx.render_view(dev.pass_desc(None, None, bounces=5), view(p), sb, rb, pb)
        ctx.view_guides(dev.pass_desc(None, None), view(1), nb, ab)
        ctx.filter_atrous(W, H, 1.0 / (K * K * 2), rb, nb, ab, fb, fpb)
        want = {"radiance": rb.read(np.float32), "nh": nb.read(np.float32), "ad": ab.read(np.float32), "filtered": fb.read(np.float32),
                "pixel": fpb.read(np.uint8).reshape(-1, 4), "plain": pb.read(np.uint8).reshape(-1, 4)}
    finally:
        for b in (sb, rb, pb, nb, ab, fb, fpb):
            b.release()
        dev.release()
        ctx.destroy()
    nh = want["nh"].reshape(-1, 4)
    assert (nh[:, 3] > 0).any() and (nh[:, 3] == 0).any() and not np.array_equal(want["pixel"], want["plain"]), "nothing hit, nothing missed, or nothing filtered"
    xml = os.path.join(PAGE, "scenes", "gems.xml")
    out, prefix = str(tmp_path / "fish.ppm"), str(tmp_path / "g")
    base = [node, os.path.join(HOST, "cli.js"), "render", xml, str(W), str(H), str(K * K)]
    cam = ["--view", "fisheye", "--fov", "100", "--look", ",".join(repr(c) for c in look)]
    r = subprocess.run(base + ["2", out] + cam + ["--view-guides", prefix, "--view-denoise"], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert b"frames that wrote their guides: 1" in r.stderr, r.stderr.decode()
    ppm = open(out, "rb").read()
    header = f"P6\n{W} {H}\n255\n".encode()
    assert ppm.startswith(header) and ppm[len(header):] == want["pixel"][:, 0:3].tobytes(), "the filtered picture"
    assert open(out + ".radiance.f32", "rb").read() == want["radiance"].tobytes(), "radiance sums"
    assert open(out + ".filtered.f32", "rb").read() == want["filtered"].tobytes(), "filtered sums"
    assert open(prefix + ".normal_hits.f32", "rb").read() == want["nh"].tobytes(), "normal_hits"
    assert open(prefix + ".albedo_depth.f32", "rb").read() == want["ad"].tobytes(), "albedo_depth"
    # queue.viewGuides itself (the N-API viewGuides entry), which the renderer's frame route never calls: both outputs, and each alone
    vg = str(tmp_path / "vg")
    r = subprocess.run([node, os.path.join(ROOT, "tests", "view_guides_node.js"), xml, str(W), str(H), str(K * K), vg, "fisheye", "100", ",".join(repr(c) for c in look)],
                       capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    for call, outs in (("both", ("normal_hits", "albedo_depth")), ("nh_alone", ("normal_hits",)), ("ad_alone", ("albedo_depth",))):
        for name in ("normal_hits", "albedo_depth"):
            f = f"{vg}.{call}.{name}.f32"
            assert os.path.exists(f) == (name in outs), f
            if name in outs:
                assert open(f, "rb").read() == want["nh" if name == "normal_hits" else "ad"].tobytes(), f"queue.viewGuides {call}: {name}"
    # --view-guides alone leaves the picture unfiltered
    r = subprocess.run(base + ["2", out] + cam + ["--view-guides", prefix], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert open(out, "rb").read()[len(header):] == want["plain"][:, 0:3].tobytes() and open(prefix + ".normal_hits.f32", "rb").read() == want["nh"].tobytes()
    # what is still missing for these cameras is still refused, and the message names it
    for flag, word in ((["--upscale", "2"], b"upsampler"), (["--ao", str(tmp_path / "a")], b"AO"), (["--gpus", "2"], b"N devices"),
                       (["--guides", prefix], b"--view-guides"), (["--denoise"], b"--view-denoise")):
        r = subprocess.run(base + ["1", out] + cam + flag, capture_output=True)
        assert r.returncode == 2 and b"--view is not available with" in r.stderr and word in r.stderr, (flag, r.stderr.decode())


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
    assert "NOT BUILT: guides" not in header
    for method in ("view_guides", "render_view_guided", "guided_views"):
        assert callable(getattr(mirt.Context, method))
    assert callable(prays.view_guides) and callable(prays.denoised_view)
    napi = open(os.path.join(PKG_DIR, "csrc", "addon", "mirt_napi.cc")).read()
    for js, s in zip(("viewGuides", "renderViewGuided", "ctxGuidedViews"), SYMBOLS):
        assert f'{{"{js}", ' in napi and s + "(" in napi, js
    webcl = open(os.path.join(HOST, "webcl.js")).read()
    for js in ("viewGuides(", "renderViewGuided(", "guidedViews()", "hasViewGuides()"):
        assert js in webcl, js
    addon = os.path.join(PKG_DIR, "mirt.node")
    if os.path.exists(addon):   # built where the Node headers are (csrc/addon/build_addon.sh)
        out = subprocess.run(["nm", "-D", "--undefined-only", addon], capture_output=True, text=True, check=True).stdout
        for s in SYMBOLS:
            assert re.search(r"\bU " + s + r"\b", out), ("mirt.node", s)
