"""GPU: the hosts of mirt_render_view_batch.

  * `cli.js views` (renderer.js renderViewBatchFile, queue.renderViewBatch, the addon) writes the bytes Context.render_view_batch leaves: the
    N frames of float4 sums after two progressive passes, and with --ppm each frame's picture; --eyes gives the cameras with the basis right =
    +x, up = +y, forward = -z (skipped without node, as the other JavaScript tests are);
  * pyhost/rays.py render_views on cuda tensors, on a side stream, equals the buffer path byte for byte, seeds included, fresh and accumulated;
  * probe_sh equals the float64 projection of the same radiance read back: per coefficient |got - want| <= 1e-4 * sum |L * Y * w| over the
    512 pixels of a 32 x 16 frame.  The fp32 dot-product bound is n * 2^-24 = 3.1e-5 at n = 512 terms; the tolerance is about three times it.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before the first context of the process: torch finds no GPU when it is first imported after libmirt has opened the device)

import a10_pass as A
import view_batch_common as VB
import view_common as V
from conftest import HOST, PAGE, load_fixture

pytestmark = pytest.mark.gpu
node = shutil.which("node")
FIXTURE, XML = "own_gems_48x36_r4", os.path.join(PAGE, "scenes", "gems.xml")
W, H, K, N, BOUNCES = 5, 3, 2, 3, 3


def batch_by_buffers(ctx, sc, view, cams, seeds, passes, bounces):
    """-> (seeds, sums, pixel) after `passes` progressive Context.render_view_batch calls, tone 1 / (rpp * p)"""
    r = VB.BatchRenderer(ctx, sc, len(cams) * view.n_rays, len(cams) * view.n_pixels, tail=0)
    try:
        got = None
        for p in range(1, passes + 1):
            got = r.run_batch(view.with_(tone=1.0 / (view.rpp * p)), cams, seeds if got is None else got[0], bounces=bounces, carry=None if got is None else got[1])
        return got
    finally:
        r.release()


@pytest.mark.skipif(node is None, reason="node is not installed")
@pytest.mark.parametrize("eyes", [False, True], ids=["cameras", "eyes"])
def test_cli_views_writes_the_bytes_the_python_call_leaves(pkg, tmp_path, eyes):
    from raytracing_amd.pyhost import mirt
    _, sc = load_fixture(FIXTURE)
    cams = VB.cameras(sc, N)
    if eyes:
        cams[:, 3:12] = (1, 0, 0, 0, 1, 0, 0, 0, -1)
    view = V.standard_view(sc, "equirect", width=W, height=H, k=K)
    seeds = A.make_seeds(N * view.n_rays, seed_base=5)
    ctx = mirt.Context(0)
    try:
        _, sums, pixel, _ = batch_by_buffers(ctx, sc, view, cams, seeds, 2, BOUNCES)
    finally:
        ctx.destroy()
    assert (sums[:, 3] > 0).any(), "no pixel received light"
    cf, of, prefix = str(tmp_path / "cameras.f32"), str(tmp_path / "out.radiance.f32"), str(tmp_path / "frame")
    (cams[:, 0:3] if eyes else cams).astype(np.float32).tofile(cf)
    cmd = [node, os.path.join(HOST, "cli.js"), "views", XML, cf, str(W), str(H), str(K * K), "2", of, "--view", "equirect", "--bounces", str(BOUNCES), "--seed-base", "5",
           "--ppm", prefix] + (["--eyes"] if eyes else [])
    r = subprocess.run(cmd, capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert open(of, "rb").read() == sums.tobytes(), "the frames' sums"
    for f in range(N):
        raw = open(f"{prefix}.{f}.ppm", "rb").read()
        head = f"P6\n{W} {H}\n255\n".encode()
        assert raw.startswith(head) and raw[len(head):] == pixel[f * W * H:(f + 1) * W * H, 0:3].tobytes(), f"picture of frame {f}"


def test_render_views_on_cuda_tensors_equals_the_buffer_path(pkg):
    import torch
    from raytracing_amd.pyhost import mirt, rays as prays
    _, sc = load_fixture(FIXTURE)
    cams = VB.cameras(sc, N)
    view = V.standard_view(sc, "fisheye", width=W, height=H, k=K, tone=0.25)
    seeds = A.make_seeds(N * view.n_rays)
    ctx = mirt.Context(0)
    dev = mirt.DeviceScene(ctx, sc)
    try:
        w1 = batch_by_buffers(ctx, sc, view.with_(tone=1.0 / 4), cams, seeds, 1, BOUNCES)
        w2 = batch_by_buffers(ctx, sc, view, cams, seeds, 2, BOUNCES)
        side = torch.cuda.Stream(device=0)
        with torch.cuda.stream(side):
            st = torch.from_numpy(seeds.copy()).to("cuda:0")
            out, px = prays.render_views(ctx, dev, view.desc(), torch.from_numpy(cams).to("cuda:0"), st, bounces=BOUNCES, want_pixel=True)
            first, first_seeds, first_px = out.cpu().numpy(), st.cpu().numpy(), px.cpu().numpy()
            d2 = view.desc()
            d2.tone = 1.0 / 8
            again, px2 = prays.render_views(ctx, dev, d2, cams.tolist(), st, bounces=BOUNCES, accumulate_into=out, want_pixel=True)
            assert again is out
            second, second_seeds, second_px = again.cpu().numpy(), st.cpu().numpy(), px2.cpu().numpy()
        side.synchronize()
        assert first.shape == (N, H, W, 4) and first.dtype == np.float32 and first_px.shape == (N, H, W, 4) and first_px.dtype == np.uint8
        assert first.tobytes() == w1[1].tobytes() and first_seeds.tobytes() == w1[0].tobytes() and first_px.tobytes() == w1[2].tobytes()
        assert second.tobytes() == w2[1].tobytes() and second_seeds.tobytes() == w2[0].tobytes() and second_px.tobytes() == w2[2].tobytes()
        empty = prays.render_views(ctx, dev, view.desc(), np.zeros((0, 12), np.float32), torch.zeros((0,), dtype=torch.int32, device="cuda:0"))
        assert empty.shape == (0, H, W, 4)
        with pytest.raises(ValueError):
            prays.render_views(ctx, dev, view.desc(), cams[:, :11], st)
        with pytest.raises(ValueError):
            prays.render_views(ctx, dev, view.desc(), cams, st[:-1])
    finally:
        dev.release()
        ctx.destroy()


def test_probe_sh_equals_the_float64_projection_of_the_same_radiance(pkg):
    import torch
    from raytracing_amd.pyhost import mirt, rays as prays
    _, sc = load_fixture(FIXTURE)
    width, height, k, passes = 32, 16, 2, 2
    b = np.asarray(sc.bounds, np.float64)
    lo, hi = b[0:3], b[4:7]
    positions = np.array([lo + (hi - lo) * t for t in ((0.5, 0.5, 0.5), (0.3, 0.6, 0.45), (0.7, 0.4, 0.6), (0.5, 0.75, 0.35))], np.float32)
    n = len(positions) * height * width * k * k
    seeds = A.make_seeds(n, seed_base=9)
    ctx = mirt.Context(0)
    dev = mirt.DeviceScene(ctx, sc)
    try:
        got = prays.probe_sh(ctx, dev, positions, width=width, height=height, k=k, passes=passes, bounces=BOUNCES, seeds=torch.from_numpy(seeds.copy()).to("cuda:0"))
        assert got.shape == (len(positions), 9, 3) and got.dtype == torch.float32 and got.is_cuda
        got = got.cpu().numpy().astype(np.float64)
        # the same radiance, read back: the same cameras, seeds and calls
        cams = np.zeros((len(positions), 12), np.float32)
        cams[:, 0:3] = positions
        cams[:, 3], cams[:, 7], cams[:, 11] = 1.0, 1.0, -1.0
        st = torch.from_numpy(seeds.copy()).to("cuda:0")
        view = mirt.view_desc(mirt.VIEW_EQUIRECT, width, height, k=k)
        sums = prays.render_views(ctx, dev, view, cams, st, bounces=BOUNCES)
        for _ in range(1, passes):
            prays.render_views(ctx, dev, view, cams, st, bounces=BOUNCES, accumulate_into=sums)
        L = sums.cpu().numpy().astype(np.float64).reshape(len(positions), height * width, 4)[:, :, 0:3] / (k * k * passes)
        drawn = prays.probe_sh(ctx, dev, positions[:1], width=8, height=4, k=1)   # seeds of its own
        assert drawn.shape == (1, 9, 3) and bool(torch.isfinite(drawn).all())
    finally:
        dev.release()
        ctx.destroy()
    assert (L > 0).any(), "no pixel received light"
    Y, w = prays.sh9_basis(width, height), prays.sh9_weights(width, height)
    want = np.einsum("pc,npx->ncx", Y * w[:, None], L)
    scale = np.einsum("pc,npx->ncx", np.abs(Y) * w[:, None], np.abs(L))
    err = np.abs(got - want)
    print(f"probe_sh: max |got - want| / sum |L Y w| = {(err / np.maximum(scale, 1e-300)).max():.3e} (bound 1e-4)")
    assert (err <= 1e-4 * scale).all(), (err.max(), np.argwhere(err > 1e-4 * scale)[:4].tolist())
    assert (np.abs(want[:, 0, :]) > 0).all(), "every probe sees light in its constant term"
