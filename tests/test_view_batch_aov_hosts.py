"""GPU: the hosts of mirt_view_guides_batch, mirt_render_view_guided_batch and mirt_view_ao_batch, at 5 x 3, k = 2, N = 3.

  * `cli.js views --guides --ao` (renderer.js renderViewBatchFile: queue.renderViewGuidedBatch on the first pass, queue.viewAoBatch before it;
    the addon) writes the bytes the C ABI leaves through pyhost's Context: the sums after two passes, the guides, the AO pairs; and
    tests/view_batch_aov_node.js (renderer.viewGuidesBatchFile: queue.viewGuidesBatch), both outputs and each alone, writes the same guides
    (skipped without node, as the other JavaScript tests are);
  * pyhost/rays.py view_guides_batch, view_ao_batch and render_views(want_guides=True) on cuda tensors equal the buffer path byte for byte;
  * probe_depth at three eyes inside the cornell box, 8 x 4, k = 1, equals depth_sum / hits of mirt_view_guides per probe -- the same fp32
    division in torch, compared exactly -- and is +inf with hit_fraction 0 where nothing was hit.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before the first context of the process: torch finds no GPU when it is first imported after libmirt has opened the device)

import a10_pass as A
import view_batch_aov_common as BA
import view_batch_common as VB
import view_common as V
from conftest import HOST, PAGE, ROOT, load_fixture

pytestmark = pytest.mark.gpu
node = shutil.which("node")
FIXTURE, XML = "own_gems_48x36_r4", os.path.join(PAGE, "scenes", "gems.xml")
W, H, K, N, BOUNCES = 5, 3, 2, 3, 3
AO = dict(samples=2, radius=1.5, bias=0.002)


def by_buffers(ctx, sc, view, cams, seeds):
    """-> (ao pairs from the fresh seeds, (seeds, sums, pixel) after the guided first pass and a plain second one, (normal_hits, albedo_depth))"""
    r = BA.Aov(ctx, sc, len(cams) * view.n_rays, len(cams) * view.n_pixels, tail=0)
    try:
        ao, clean = r.ao_batch(view, cams, seeds, **AO)
        assert clean
        g1, guides = r.guided_batch(view.with_(tone=1.0 / view.rpp), cams, seeds, bounces=BOUNCES)
        r.seeds.write(g1[0])
        ctx.render_view_batch(r.scene_desc(BOUNCES), view.with_(tone=1.0 / (view.rpp * 2)).desc(V.ACCUMULATE), cams, r.seeds, r.radiance, r.pixel)
        g2 = r._frame(len(cams) * view.n_rays, len(cams) * view.n_pixels)
        alone = r.guides_batch(view, cams)
        assert alone[0].tobytes() == guides[0].tobytes() and alone[1].tobytes() == guides[1].tobytes()
        return ao, g1, g2, guides
    finally:
        r.release()


@pytest.mark.skipif(node is None, reason="node is not installed")
def test_cli_views_and_the_queue_write_the_bytes_the_python_calls_leave(pkg, tmp_path):
    from raytracing_amd.pyhost import mirt
    _, sc = load_fixture(FIXTURE)
    cams = VB.cameras(sc, N)
    view = V.standard_view(sc, "equirect", width=W, height=H, k=K)
    seeds = A.make_seeds(N * view.n_rays, seed_base=5)
    ctx = mirt.Context(0)
    try:
        ao, _g1, g2, guides = by_buffers(ctx, sc, view, cams, seeds)
    finally:
        ctx.destroy()
    assert (g2[1][:, 3] > 0).any() and (guides[0][:, 3] > 0).any() and (ao[:, 1] > 0).any(), "nothing lit, hit or cast"
    cf, of, gp, ap = str(tmp_path / "cameras.f32"), str(tmp_path / "out.radiance.f32"), str(tmp_path / "g"), str(tmp_path / "a")
    cams.astype(np.float32).tofile(cf)
    cmd = [node, os.path.join(HOST, "cli.js"), "views", XML, cf, str(W), str(H), str(K * K), "2", of, "--view", "equirect", "--bounces", str(BOUNCES), "--seed-base", "5",
           "--guides", gp, "--ao", ap, "--ao-samples", str(AO["samples"]), "--ao-radius", str(AO["radius"]), "--ao-bias", str(AO["bias"])]
    r = subprocess.run(cmd, capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert b"batch calls that wrote their guides: 1" in r.stderr, r.stderr.decode()
    assert open(of, "rb").read() == g2[1].tobytes(), "the frames' sums after two passes"
    assert open(gp + ".normal_hits.f32", "rb").read() == guides[0].tobytes() and open(gp + ".albedo_depth.f32", "rb").read() == guides[1].tobytes(), "the guides"
    assert open(ap + ".ao.u32", "rb").read() == ao.tobytes(), "the AO pairs"
    # queue.viewGuidesBatch alone
    prefix = str(tmp_path / "vg")
    r = subprocess.run([node, os.path.join(ROOT, "tests", "view_batch_aov_node.js"), XML, cf, str(W), str(H), str(K * K), prefix, "equirect"], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    for call, outs in (("both", ("normal_hits", "albedo_depth")), ("nh_alone", ("normal_hits",)), ("ad_alone", ("albedo_depth",))):
        for out in outs:
            want = guides[0] if out == "normal_hits" else guides[1]
            assert open(f"{prefix}.{call}.{out}.f32", "rb").read() == want.tobytes(), (call, out)


def test_the_torch_helpers_equal_the_buffer_path(pkg):
    import torch
    from raytracing_amd.pyhost import mirt, rays as prays
    _, sc = load_fixture(FIXTURE)
    cams = VB.cameras(sc, N)
    view = V.standard_view(sc, "fisheye", width=W, height=H, k=K, tone=0.25)
    seeds = A.make_seeds(N * view.n_rays)
    ctx = mirt.Context(0)
    dev = mirt.DeviceScene(ctx, sc)
    try:
        ao, g1, _g2, guides = by_buffers(ctx, sc, view, cams, seeds)
        st = torch.from_numpy(seeds.copy()).to("cuda:0")
        nh, ad = prays.view_guides_batch(ctx, dev, view.desc(), torch.from_numpy(cams).to("cuda:0"))
        assert nh.shape == (N, H, W, 4) and ad.shape == (N, H, W, 4) and nh.dtype == torch.float32 and nh.is_cuda
        assert nh.cpu().numpy().tobytes() == guides[0].tobytes() and ad.cpu().numpy().tobytes() == guides[1].tobytes()
        got = prays.view_ao_batch(ctx, dev, view.desc(), cams, st, **AO)
        assert got.shape == (N, H, W, 2) and got.dtype == torch.int32
        assert got.cpu().numpy().tobytes() == ao.tobytes() and st.cpu().numpy().tobytes() == seeds.tobytes(), "the pairs, and the seeds unchanged"
        out, px, gnh, gad = prays.render_views(ctx, dev, view.desc(), cams.tolist(), st, bounces=BOUNCES, want_pixel=True, want_guides=True)
        assert out.cpu().numpy().tobytes() == g1[1].tobytes() and st.cpu().numpy().tobytes() == g1[0].tobytes() and px.cpu().numpy().tobytes() == g1[2].tobytes()
        assert gnh.shape == (N, H, W, 4) and gnh.cpu().numpy().tobytes() == guides[0].tobytes() and gad.cpu().numpy().tobytes() == guides[1].tobytes()
        e1, e2 = prays.view_guides_batch(ctx, dev, view.desc(), np.zeros((0, 12), np.float32))
        assert e1.shape == (0, H, W, 4) and e2.shape == (0, H, W, 4)
        assert prays.view_ao_batch(ctx, dev, view.desc(), np.zeros((0, 12), np.float32), torch.zeros((0,), dtype=torch.int32, device="cuda:0")).shape == (0, H, W, 2)
        with pytest.raises(ValueError):
            prays.view_guides_batch(ctx, dev, view.desc(), cams[:, :11])
        with pytest.raises(ValueError):
            prays.view_ao_batch(ctx, dev, view.desc(), cams, st[:-1])
    finally:
        dev.release()
        ctx.destroy()


def test_probe_depth_is_the_guides_depth_over_hits(pkg):
    import torch
    from raytracing_amd.pyhost import mirt, rays as prays
    _, sc = load_fixture("cornell_32x24_r4")
    width, height, k = 8, 4, 1
    b = np.asarray(sc.bounds, np.float64)
    lo, hi = b[0:3], b[4:7]
    positions = np.array([lo + (hi - lo) * t for t in ((0.5, 0.5, 0.5), (0.3, 0.6, 0.45), (0.7, 0.4, 0.6))], np.float32)
    ctx = mirt.Context(0)
    dev = mirt.DeviceScene(ctx, sc)
    try:
        mean, frac = prays.probe_depth(ctx, dev, positions, width=width, height=height, k=k)
        assert mean.shape == (3, height, width) and frac.shape == (3, height, width) and mean.dtype == torch.float32 and mean.is_cuda
        mean, frac = mean.cpu(), frac.cpu()
        for f, p in enumerate(positions):
            view = mirt.view_desc(mirt.VIEW_EQUIRECT, width, height, k=k)
            view.eye, view.right, view.up, view.forward = ((C.c_float * 3)(*v) for v in (p.tolist(), (1, 0, 0), (0, 1, 0), (0, 0, -1)))
            nh, ad = prays.view_guides(ctx, dev, view)
            hits, depth = nh[:, 3].cpu().reshape(height, width), ad[:, 3].cpu().reshape(height, width)
            hit = hits > 0
            assert bool(hit.any()), f"probe {f} sees nothing"
            assert torch.equal(mean[f][hit], (depth / hits)[hit]), f"probe {f}: mean distance"
            assert bool(torch.isinf(mean[f][~hit]).all()) and bool((mean[f][~hit] > 0).all()) and bool((frac[f][~hit] == 0).all()), f"probe {f}: pixels without a hit"
            assert torch.equal(frac[f], hits / float(k * k)) and bool((mean[f][hit] > 0).all())
    finally:
        dev.release()
        ctx.destroy()
