"""GPU: mirt_render_first_pass_guided -- a frame's first pass and its first-hit guides in one call (include/mirt.h) -- through the C ABI.  In every
case the expectation is made in the same test by mirt_render_first_pass + mirt_render_guides on a second set of buffers with the same seeds, and
every buffer (seeds, acu, pixel, radiance, normal_hits, albedo_depth) is compared as bits (tests/pass_guided_common.py).  mirt_ctx_guided_passes
proves which route ran: the pass's own launch (4, 16, 64 rays per pixel where the pass resolves its pixels), or the guide launches behind it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_fixture
from guides_common import difference
from pass_guided_common import PATTERN, compare, guided, packed

pytestmark = pytest.mark.gpu

DEFAULT_LIB = os.path.join(ROOT, "2015-raytracing_amd", "libmirt_default.so")


@pytest.fixture(scope="module")
def ctx(pkg):
    from raytracing_amd.pyhost import mirt
    c = mirt.Context(0)
    yield c
    c.destroy()


def both_modes(ctx, ps, tag, **kw):
    """the optimistic pair, then the exact kernel alone: -> what compare returns for the optimistic pair"""
    first = None
    for exact_only in (False, True):
        ctx.set_exact_only(exact_only)
        try:
            r = compare(ctx, ps, f"{tag} exact_only={exact_only}", **kw)
        finally:
            ctx.set_exact_only(False)
        assert r[0] is None, r[0]
        assert r[1] == 1, f"{tag} exact_only={exact_only}: the call did not take the one-launch route"
        first = first or r
    return first


# ---- the smallest shapes where the lane arithmetic can go wrong: 35 pixels, the last block partial at 64, 16 and 4 pixels per block -------------
@pytest.mark.parametrize("keep_acu", [False, True], ids=["acu_null", "acu_given"])
@pytest.mark.parametrize("rpp", [4, 16, 64])
def test_7x5_equals_the_two_calls(ctx, rpp, keep_acu):
    _, _, _, got = both_modes(ctx, packed("cornell_32x24_r4", 7, 5, rpp), f"cornell 7x5 x{rpp}", keep_acu=keep_acu)
    assert (got[0][:, 3] > 0).any(), "no pixel of the picture hits anything"


def test_one_output_alone(ctx):
    from raytracing_amd.pyhost import render
    ps = packed("cornell_32x24_r4", 7, 5, 16)
    _, _, _, want = compare(ctx, ps, "both outputs")
    for outputs in ((True, False), (False, True)):
        fr = render.FusedRenderer(ctx, ps, seed_base=5, keep_acu=False)
        try:
            got = guided(ctx, fr, outputs=outputs)
        finally:
            fr.release()
        for i in (0, 1):
            if outputs[i]:
                assert difference(f"output {i} alone", got[i], want[i]) is None
            else:
                assert (got[i] == PATTERN).all(), "an output that was not asked for was written"


# ---- a row tile with row0 > 0: global ray ids, tile-local pixel index ------------------------------------------------------------------------------
@pytest.mark.parametrize("rpp", [4, 16])
def test_row_tile_equals_the_rows_of_the_whole_frame(ctx, rpp):
    from raytracing_amd.pyhost import render
    ps = packed("cornell_32x24_r4", 7, 6, rpp)
    diff, routed, _, tile = compare(ctx, ps, f"rows 2..4 of 7x6 x{rpp}", row0=2, nrows=3, keep_acu=False)
    assert diff is None, diff
    assert routed == 1
    whole = render.FusedRenderer(ctx, ps)
    try:
        full = whole.guides()
    finally:
        whole.release()
    for i, name in enumerate(("normal_hits", "albedo_depth")):
        d = difference(f"rows 2..4 against the whole frame's {name}", tile[i], full[i][2 * 7:5 * 7])
        assert d is None, d


# ---- pixels that hit nothing ---------------------------------------------------------------------------------------------------------------------
def test_background_pixels_are_all_plus_zero(ctx):
    _, _, _, (nh, ad) = both_modes(ctx, packed("basic_32x24_r4", 24, 16, 16), "basic 24x16 x16", keep_acu=False)
    empty = nh[:, 3] == 0
    assert empty.any() and (~empty).any(), "spheres in front of nothing: both kinds of pixel occur"
    assert not nh[empty].view(np.uint32).any() and not ad[empty].view(np.uint32).any(), "a pixel without a hit is (+0, +0, +0, +0) in both outputs"


# ---- blocks that defer: their guides are the exact kernel's ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rpp", [4, 16])
def test_deferred_blocks_get_the_exact_kernels_guides(ctx, rpp):
    diff, routed, deferred, _ = compare(ctx, packed("own_flat_32x24_r4", 32, 24, rpp), f"own_flat 32x24 x{rpp}", keep_acu=False)
    assert deferred > 0, "own_flat no longer defers: the exact kernel's rewrite of a deferred block's guides is not exercised"
    assert diff is None, diff
    assert routed == 1
    ctx.set_exact_only(True)
    try:
        diff, routed, deferred, _ = compare(ctx, packed("own_flat_32x24_r4", 32, 24, rpp), f"own_flat 32x24 x{rpp}, exact kernel only", keep_acu=False)
    finally:
        ctx.set_exact_only(False)
    assert diff is None, diff
    assert routed == 1 and deferred == 0


# ---- the grid kernels ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rpp", [4, 16])
def test_grid_meshes_with_staged_cell_tables(ctx, rpp):
    _, _, _, (nh, _) = both_modes(ctx, packed("cornell_teapot3_32x24_r4", 24, 16, rpp), f"cornell_teapot3 24x16 x{rpp}")
    assert (nh[:, 3] > 0).any()


def test_grid_meshes_whose_cell_tables_exceed_the_staging(ctx):
    """cornell_teapot3 with its teapot re-binned at n = 17: 4914 table words, more than the block's LDS staging holds (k_fusedPass<*, 2>)"""
    from raytracing_amd.pyhost import scene
    from test_gpu_parity import _regrid_mesh
    _, sc0 = load_fixture("cornell_teapot3_32x24_r4")
    d = dict(sc0.d)
    d["meshes"] = [_regrid_mesh(sc0.d["meshes"][0], 17)] + list(sc0.d["meshes"][1:])
    both_modes(ctx, scene.PackedScene(d).resized(24, 16, 4), "cornell_teapot3 re-binned at 17, 24x16 x4")


def _child(mode, env):
    env = dict(os.environ, **env)
    env.pop("MIRT_LIB_PATH", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pass_guided_child.py"), mode], env=env, capture_output=True, text=True, timeout=600)
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0, (lines[-1:] or r.stderr[-2000:])
    assert len(lines) == 4 and all(l["ok"] for l in lines), lines


def test_five_wave_build_of_the_grid_kernels():
    _child("waves5", {"MIRT_GRID_WAVES": "5"})


@pytest.mark.skipif(not os.path.exists(DEFAULT_LIB), reason="libmirt_default.so not built")
def test_the_default_contract_library():
    _child("default", {"MIRT_CONTRACT": "default"})


# ---- the counts and settings that queue the guide launches behind the pass ----------------------------------------------------------------------------
@pytest.mark.parametrize("rpp", [9, 256, 289])
def test_fallback_counts(ctx, rpp):
    diff, routed, _, _ = compare(ctx, packed("cornell_32x24_r4", 7, 5, rpp), f"cornell 7x5 x{rpp}", keep_acu=(rpp == 9))
    assert diff is None, diff
    assert routed == 0, "the one-launch route exists at 4, 16 and 64 rays per pixel only"


def test_fallback_without_inpass_resolve(pkg):
    from raytracing_amd.pyhost import mirt
    os.environ["MIRT_INPASS_RESOLVE"] = "0"   # read when a context is created
    try:
        sep = mirt.Context(0)
    finally:
        del os.environ["MIRT_INPASS_RESOLVE"]
    try:
        diff, routed, _, _ = compare(sep, packed("cornell_32x24_r4", 7, 5, 16), "cornell 7x5 x16, MIRT_INPASS_RESOLVE=0")
        assert diff is None, diff
        assert routed == 0
    finally:
        sep.destroy()


def test_fallback_with_acu_and_no_output_buffer(ctx):
    from raytracing_amd.pyhost import render
    import a10_pass as A
    ps = packed("cornell_32x24_r4", 7, 5, 16)
    seeds = A.make_seeds(ps.total_rays, seed_base=5)
    _, _, _, want = compare(ctx, ps, "reference")
    fr = render.FusedRenderer(ctx, ps, seeds=seeds)
    ref = render.FusedRenderer(ctx, ps, seeds=seeds)
    nh, ad = ctx.buffer(fr.npix * 16), ctx.buffer(fr.npix * 16)
    try:
        before = ctx.guided_passes()
        ctx.render_first_pass_guided(fr.dev.pass_desc(fr.seeds, fr.acu), nh, ad)
        assert ctx.guided_passes() == before
        ctx.render_pass(ref.dev.pass_desc(ref.seeds, ref.acu), fresh=True)
        assert difference("normal_hits", nh.read(np.float32), want[0]) is None and difference("albedo_depth", ad.read(np.float32), want[1]) is None
        assert difference("acu", fr.acu.read(np.float32), ref.acu.read(np.float32)) is None
        assert np.array_equal(fr.seeds.read(np.int32), ref.seeds.read(np.int32))
    finally:
        for b in (nh, ad):
            b.release()
        fr.release()
        ref.release()


def test_forced_two_call_path_gives_the_same_bits(ctx):
    os.environ["MIRT_GUIDED_PASS"] = "0"   # read per call
    try:
        diff, routed, _, _ = compare(ctx, packed("cornell_32x24_r4", 7, 5, 16), "MIRT_GUIDED_PASS=0")
    finally:
        del os.environ["MIRT_GUIDED_PASS"]
    assert diff is None, diff
    assert routed == 0


# ---- refusals: nothing at all is written ---------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_leave_the_context_working(ctx):
    from raytracing_amd.pyhost import mirt, render
    ps = packed("cornell_32x24_r4", 7, 5, 16)
    fr = render.FusedRenderer(ctx, ps, seed_base=5)
    npix, nrays = fr.npix, fr.nrays
    nh, ad, small = ctx.buffer(npix * 16), ctx.buffer(npix * 16), ctx.buffer(npix * 16 - 1)
    fills = [(fr.seeds, np.arange(nrays, dtype=np.int32) * 7 + 1), (fr.acu, np.full(4 * nrays, 3.25, np.float32)), (fr.pixel, np.full(4 * npix, 0x5A, np.uint8)),
             (fr.radiance, np.full(4 * npix, 2.5, np.float32)), (nh, np.full(4 * npix, PATTERN, np.float32)), (ad, np.full(4 * npix, PATTERN, np.float32)),
             (small, np.full(npix * 16 - 1, 0xA5, np.uint8))]

    def desc(rpp=None):
        d = fr.dev.pass_desc(fr.seeds, fr.acu, fr.pixel, fr.radiance)
        if rpp is not None:
            d.rays_per_pixel = rpp
        return d

    def untouched(what):
        for b, f in fills:
            assert b.read(f.dtype).tobytes() == f.tobytes(), f"{what}: a buffer was written"

    def refused(code, call, word):
        for b, f in fills:
            b.write(f)
        with pytest.raises(mirt.MirtError) as e:
            call()
        assert e.value.code == code and word in str(e.value), str(e.value)
        untouched(word)

    try:
        before = ctx.guided_passes()
        refused(-1, lambda: ctx.render_first_pass_guided(desc(), None, None), "both NULL")
        refused(-1, lambda: ctx.render_first_pass_guided(desc(1), nh, ad), "seeds[col]")
        refused(-5, lambda: ctx.render_first_pass_guided(desc(), small, ad), "normal_hits")
        refused(-5, lambda: ctx.render_first_pass_guided(desc(), nh, small), "albedo_depth")
        refused(-1, lambda: ctx.render_first_pass_guided(desc(), fr.radiance, ad), "aliases")
        refused(-1, lambda: ctx.render_first_pass_guided(desc(), nh, fr.seeds), "aliases")
        refused(-1, lambda: ctx.render_first_pass_guided(desc(), nh, nh), "aliases")
        d = desc()   # (made outside the recording: a new scene would be validated and prepared here)
        for b, f in fills:
            b.write(f)
        ctx.finish()
        ctx.capture_begin()
        try:
            with pytest.raises(mirt.MirtError) as e:
                ctx.render_first_pass_guided(d, nh, ad)
            assert e.value.code == -1 and "capture" in str(e.value)
        finally:
            ctx.graph_release(ctx.capture_end())
        untouched("inside a recording")
        assert ctx.guided_passes() == before
    finally:
        for b in (nh, ad, small):
            b.release()
        fr.release()
    diff, routed, _, _ = compare(ctx, ps, "after the refusals")
    assert diff is None, diff
    assert routed == 1


# ---- the Python hosts ---------------------------------------------------------------------------------------------------------------------------------
def test_renderer_methods(ctx):
    from raytracing_amd.pyhost import render
    ps = packed("cornell_teapot3_32x24_r4", 24, 16, 4)
    a, b = render.FusedRenderer(ctx, ps, seed_base=3), render.FusedRenderer(ctx, ps, seed_base=3)
    try:
        before = ctx.guided_passes()
        got = a.denoised_first_pass(iterations=2)
        assert ctx.guided_passes() == before + 1 and a.passes == 2
        b.execute_render(fresh=True)
        want = b.denoised(iterations=2)
        assert np.array_equal(got[0], want[0]) and difference("filtered", got[1], want[1]) is None
        g = b.guides()
        assert difference("normal_hits", a.normal_hits.read(np.float32), g[0]) is None and difference("albedo_depth", a.albedo_depth.read(np.float32), g[1]) is None
        assert np.array_equal(a.pixel.read(np.uint8), b.pixel.read(np.uint8)) and np.array_equal(a.seeds.read(np.int32), b.seeds.read(np.int32))
    finally:
        a.release()
        b.release()


def test_upscaled_renderer_uses_the_guided_call_for_its_first_pass(ctx):
    from raytracing_amd.pyhost import render
    ps = packed("cornell_32x24_r4", 28, 20, 4)
    a, b = render.UpscaledRenderer(ctx, ps, 2, seed_base=3), render.UpscaledRenderer(ctx, ps, 2, seed_base=3)
    try:
        before = ctx.guided_passes()
        got = a.render(passes=1)
        assert ctx.guided_passes() == before + 1
        os.environ["MIRT_GUIDED_PASS"] = "0"
        try:
            want = b.render(passes=1)
        finally:
            del os.environ["MIRT_GUIDED_PASS"]
        assert ctx.guided_passes() == before + 1
        assert np.array_equal(got[0], want[0]) and difference("upsampled", got[1], want[1]) is None
    finally:
        a.release()
        b.release()
