"""GPU: the post-process chain in row tiles, end to end through the Python driver (pyhost/render.py TiledPostRenderer) on rehearsal groups
(MIRT_GROUP_ALLOW_REPEATED_DEVICES=1) of 2, 3 and 5 contexts, on the cornell scene resized as tests/test_upsample.py resizes it: every frame
equals, in every byte, the frame of the single-context chain.

  1. denoise at 48 x 36 x 4 rays: TiledPostRenderer.denoised against FusedRenderer.denoised_first_pass, in pixel and filtered; two passes once,
     against FusedRenderer.denoised_passes;
  2. upscale by 2 from 24 x 18, with and without the filter of the low frame, against UpscaledRenderer.render; two passes once."""
import numpy as np
import pytest

from conftest import load_fixture
from filter_common import difference

pytestmark = pytest.mark.gpu

W, H, RPP, SEED = 48, 36, 4, 3
GROUPS = (2, 3, 5)


def resized(w, h, rpp):
    from raytracing_amd.pyhost import scene
    _, sc0 = load_fixture("cornell_32x24_r4")
    return scene.PackedScene(dict(sc0.d)).resized(w, h, rpp)


@pytest.fixture(scope="module")
def ctx(pkg):
    from raytracing_amd.pyhost import mirt
    c = mirt.Context(0)
    yield c
    c.destroy()


@pytest.fixture()
def groups(pkg, monkeypatch):
    """a rehearsal group of the size asked for, destroyed with the test: with the single context never more than 6 contexts in the process"""
    from raytracing_amd.pyhost import mirt
    monkeypatch.setenv("MIRT_GROUP_ALLOW_REPEATED_DEVICES", "1")
    made = {}

    class Groups:
        def __getitem__(self, n):
            if n not in made:
                made[n] = mirt.DeviceGroup([0] * n)
            return made[n]
    yield Groups()
    for g in made.values():
        g.destroy()


def same(tag, got, want):
    for name, g, w in zip(("pixel", "radiance"), got, want):
        d = difference(f"{tag} {name}", g, w)
        assert d is None, d


_single = {}


def single(ctx, what, passes, denoise=True):
    """the single-context chain, run once per case and left unchanged"""
    from raytracing_amd.pyhost import render
    key = (what, passes, denoise)
    if key not in _single:
        if what == "denoise":
            fr = render.FusedRenderer(ctx, resized(W, H, RPP), seed_base=SEED)
            try:
                _single[key] = fr.denoised_first_pass() if passes == 1 else fr.denoised_passes(passes)
            finally:
                fr.release()
        else:
            u = render.UpscaledRenderer(ctx, resized(W, H, RPP), 2, seed_base=SEED)
            try:
                _single[key] = u.render(passes=passes, denoise=denoise)
            finally:
                u.release()
    return _single[key]


@pytest.mark.parametrize("n", GROUPS)
def test_denoise_in_tiles_equals_the_single_context_frame(ctx, groups, n):
    from raytracing_amd.pyhost import render
    want = single(ctx, "denoise", 1)
    got = render.TiledPostRenderer(groups[n], resized(W, H, RPP), seed_base=SEED).denoised(passes=1)
    same(f"denoise over {n} contexts", got, want)
    assert len(np.unique(want[0], axis=0)) > 50, "the frame is not a picture"


def test_denoise_of_two_passes(ctx, groups):
    from raytracing_amd.pyhost import render
    got = render.TiledPostRenderer(groups[3], resized(W, H, RPP), seed_base=SEED).denoised(passes=2)
    same("denoise of 2 passes over 3 contexts", got, single(ctx, "denoise", 2))


def test_denoise_pixel_alone_and_five_iterations(ctx, groups):
    """halo 62 over 36 rows: every window is the whole image, every tile reads every other"""
    from raytracing_amd.pyhost import render
    fr = render.FusedRenderer(ctx, resized(W, H, RPP), seed_base=SEED)
    try:
        want = fr.denoised_first_pass(iterations=5)
    finally:
        fr.release()
    pixel, filtered = render.TiledPostRenderer(groups[5], resized(W, H, RPP), seed_base=SEED).denoised(passes=1, want_filtered=False, iterations=5)
    assert filtered is None
    d = difference("pixel", pixel, want[0])
    assert d is None, d


@pytest.mark.parametrize("denoise", [True, False])
@pytest.mark.parametrize("n", GROUPS)
def test_upscale_in_tiles_equals_the_single_context_frame(ctx, groups, n, denoise):
    from raytracing_amd.pyhost import render
    want = single(ctx, "upscale", 1, denoise)
    got = render.TiledPostRenderer(groups[n], resized(W, H, RPP), seed_base=SEED).upscaled(2, passes=1, denoise=denoise)
    same(f"upscale by 2 over {n} contexts, denoise={denoise}", got, want)


def test_upscale_of_two_passes(ctx, groups):
    from raytracing_amd.pyhost import render
    got = render.TiledPostRenderer(groups[2], resized(W, H, RPP), seed_base=SEED).upscaled(2, passes=2, denoise=True)
    same("upscale of 2 passes over 2 contexts", got, single(ctx, "upscale", 2))
