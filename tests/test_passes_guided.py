"""GPU: mirt_render_passes_guided -- several progressive passes and the frame's first-hit guides in one call (include/mirt.h) -- through the C ABI.
In every case the expectation is made in the same test by mirt_render_passes + mirt_render_guides on a second set of buffers with the same seeds,
and every buffer (seeds, acu, pixel, radiance -- n frames each with a frame after every pass -- normal_hits, albedo_depth) is compared as bits
(tests/passes_guided_common.py).  mirt_ctx_guided_passes proves which route ran: the multi-pass launch's own first pass (4, 16, 64 rays per pixel
where the launch resolves its pixels, default reuse pairing; several passes of a scene with grids are excluded: DESIGN.md section 5), or the guide
launches behind what mirt_render_passes queues."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_fixture
from guides_common import difference
from passes_guided_common import PATTERN, compare, first_difference, packed, run

pytestmark = pytest.mark.gpu

DEFAULT_LIB = os.path.join(ROOT, "2015-raytracing_amd", "libmirt_default.so")


@pytest.fixture(scope="module")
def ctx(pkg):
    from raytracing_amd.pyhost import mirt
    c = mirt.Context(0)
    yield c
    c.destroy()


def both_modes(ctx, ps, tag, n, routed=1, **kw):
    """the optimistic pair, then the exact kernel alone: -> what compare returns for the optimistic pair"""
    first = None
    for exact_only in (False, True):
        ctx.set_exact_only(exact_only)
        try:
            r = compare(ctx, ps, f"{tag} exact_only={exact_only}", n, **kw)
        finally:
            ctx.set_exact_only(False)
        assert r[0] is None, r[0]
        assert r[1] == routed, f"{tag} exact_only={exact_only}: the call took the one-launch route {r[1]} times, not {routed}"
        first = first or r
    return first


# ---- the smallest shapes where the lane arithmetic can go wrong: 35 pixels, the last block partial at 64, 16 and 4 pixels per block -------------
@pytest.mark.parametrize("keep_acu", [False, True], ids=["acu_null", "acu_given"])
@pytest.mark.parametrize("every", [False, True], ids=["last_frame", "every_frame"])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("rpp", [4, 16, 64])
def test_7x5_equals_the_two_calls(ctx, rpp, n, every, keep_acu):
    _, _, _, got = both_modes(ctx, packed("cornell_32x24_r4", 7, 5, rpp), f"cornell 7x5 x{rpp}, {n} passes, every={every}", n, every=every, keep_acu=keep_acu)
    assert (got["normal_hits"][:, 3] > 0).any(), "no pixel of the picture hits anything"


@pytest.mark.parametrize("rpp", [4, 16])
def test_one_pass_equals_the_first_pass_call(ctx, rpp):
    from raytracing_amd.pyhost import render
    import pass_guided_common as one
    ps = packed("cornell_32x24_r4", 7, 5, rpp)
    diff, routed, _, got = compare(ctx, ps, f"cornell 7x5 x{rpp}, 1 pass", 1)
    assert diff is None, diff
    assert routed == 1
    fr = render.FusedRenderer(ctx, ps, seed_base=5)
    try:
        nh, ad = one.guided(ctx, fr)
        want = {"normal_hits": nh, "albedo_depth": ad, "pixel": fr.pixel.read(np.uint8), "radiance": fr.radiance.read(np.float32),
                "seeds": fr.seeds.read(np.int32), "acu": fr.acu.read(np.float32)}
    finally:
        fr.release()
    diff = first_difference("against mirt_render_first_pass_guided", got, want)
    assert diff is None, diff


@pytest.mark.parametrize("every", [False, True], ids=["last_frame", "every_frame"])
def test_a_batch_that_is_not_fresh(ctx, every):
    """an ordinary first pass, then the guided batch at pass_index 2 on the accumulator it left: the guides are still taken in the launch's first pass"""
    diff, routed, _, got = compare(ctx, packed("cornell_32x24_r4", 7, 5, 16), "cornell 7x5 x16, passes 2..4", 3, every=every, first_pass=True)
    assert diff is None, diff
    assert routed == 1
    assert (got["normal_hits"][:, 3] > 0).any()


def test_one_output_alone(ctx):
    from raytracing_amd.pyhost import render
    ps = packed("cornell_32x24_r4", 7, 5, 16)
    _, _, _, want = compare(ctx, ps, "both outputs", 2)
    for outputs in ((True, False), (False, True)):
        fr = render.FusedRenderer(ctx, ps, seed_base=5)
        try:
            got = run(ctx, fr, 2, True, outputs=outputs)
        finally:
            fr.release()
        for i, name in enumerate(("normal_hits", "albedo_depth")):
            if outputs[i]:
                assert difference(f"{name} alone", got[name], want[name]) is None
            else:
                assert (got[name] == PATTERN).all(), "an output that was not asked for was written"
        assert first_difference("the pass's buffers", {k: got[k] for k in ("pixel", "radiance", "seeds", "acu")}, {k: want[k] for k in ("pixel", "radiance", "seeds", "acu")}) is None


# ---- a row tile with row0 > 0: global ray ids, tile-local pixel index ------------------------------------------------------------------------------
@pytest.mark.parametrize("rpp", [4, 16])
def test_row_tile_equals_the_rows_of_the_whole_frame(ctx, rpp):
    from raytracing_amd.pyhost import render
    ps = packed("cornell_32x24_r4", 7, 6, rpp)
    diff, routed, _, tile = compare(ctx, ps, f"rows 2..4 of 7x6 x{rpp}", 2, row0=2, nrows=3, keep_acu=False)
    assert diff is None, diff
    assert routed == 1
    whole = render.FusedRenderer(ctx, ps)
    try:
        full = whole.guides()
    finally:
        whole.release()
    for i, name in enumerate(("normal_hits", "albedo_depth")):
        d = difference(f"rows 2..4 against the whole frame's {name}", tile[name], full[i][2 * 7:5 * 7])
        assert d is None, d


# ---- pixels that hit nothing ---------------------------------------------------------------------------------------------------------------------
def test_background_pixels_are_all_plus_zero(ctx):
    _, _, _, got = both_modes(ctx, packed("basic_32x24_r4", 24, 16, 16), "basic 24x16 x16, 2 passes", 2, keep_acu=False)
    nh, ad = got["normal_hits"], got["albedo_depth"]
    empty = nh[:, 3] == 0
    assert empty.any() and (~empty).any(), "spheres in front of nothing: both kinds of pixel occur"
    assert not nh[empty].view(np.uint32).any() and not ad[empty].view(np.uint32).any(), "a pixel without a hit is (+0, +0, +0, +0) in both outputs"


# ---- blocks that defer, in whichever pass: their guides are the exact kernel's --------------------------------------------------------------------------
@pytest.mark.parametrize("every", [False, True], ids=["last_frame", "every_frame"])
@pytest.mark.parametrize("rpp", [4, 16])
def test_deferred_blocks_get_the_exact_kernels_guides(ctx, rpp, every):
    ps = packed("own_flat_32x24_r4", 32, 24, rpp)
    diff, routed, deferred, _ = compare(ctx, ps, f"own_flat 32x24 x{rpp}, 3 passes, every={every}", 3, every=every, keep_acu=False)
    assert deferred > 0, "own_flat no longer defers: the exact kernel's rewrite of a deferred block's guides is not exercised"
    assert diff is None, diff
    assert routed == 1
    ctx.set_exact_only(True)
    try:
        diff, routed, deferred, _ = compare(ctx, ps, f"own_flat 32x24 x{rpp}, 3 passes, every={every}, exact kernel only", 3, every=every, keep_acu=False)
    finally:
        ctx.set_exact_only(False)
    assert diff is None, diff
    assert routed == 1 and deferred == 0


# ---- the grid kernels: several passes stay on the guide launches (measured slower in the launch), one pass is the first-pass call's route --------------
@pytest.mark.parametrize("every", [False, True], ids=["last_frame", "every_frame"])
@pytest.mark.parametrize("rpp", [4, 16])
def test_grid_meshes_with_staged_cell_tables(ctx, rpp, every):
    _, _, _, got = both_modes(ctx, packed("cornell_teapot3_32x24_r4", 24, 16, rpp), f"cornell_teapot3 24x16 x{rpp}, every={every}", 2, routed=0, every=every)
    assert (got["normal_hits"][:, 3] > 0).any()


def test_grid_meshes_one_pass_takes_the_launch(ctx):
    both_modes(ctx, packed("cornell_teapot3_32x24_r4", 24, 16, 4), "cornell_teapot3 24x16 x4, 1 pass", 1)


def _rebinned():
    from raytracing_amd.pyhost import scene
    from test_gpu_parity import _regrid_mesh
    _, sc0 = load_fixture("cornell_teapot3_32x24_r4")
    d = dict(sc0.d)
    d["meshes"] = [_regrid_mesh(sc0.d["meshes"][0], 17)] + list(sc0.d["meshes"][1:])
    return scene.PackedScene(d).resized(24, 16, 4)


@pytest.mark.parametrize("every", [False, True], ids=["last_frame", "every_frame"])
def test_grid_meshes_whose_cell_tables_exceed_the_staging(ctx, every):
    """cornell_teapot3 with its teapot re-binned at n = 17: 4914 table words, more than the block's LDS staging holds (k_fusedPass<*, 2>)"""
    both_modes(ctx, _rebinned(), f"cornell_teapot3 re-binned at 17, 24x16 x4, every={every}", 2, routed=0, every=every)


def _child(mode, env, cases):
    env = dict(os.environ, **env)
    env.pop("MIRT_LIB_PATH", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "passes_guided_child.py"), mode], env=env, capture_output=True, text=True, timeout=600)
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0, (lines[-1:] or r.stderr[-2000:])
    assert len(lines) == cases and all(l["ok"] for l in lines), lines


def test_five_wave_build_of_the_grid_kernels():
    _child("waves5", {"MIRT_GRID_WAVES": "5"}, 6)


@pytest.mark.skipif(not os.path.exists(DEFAULT_LIB), reason="libmirt_default.so not built")
def test_the_default_contract_library():
    _child("default", {"MIRT_CONTRACT": "default"}, 12)


# ---- the counts and settings that queue the guide launches behind the passes ----------------------------------------------------------------------------
@pytest.mark.parametrize("every", [False, True], ids=["last_frame", "every_frame"])
@pytest.mark.parametrize("rpp", [9, 256, 289])
def test_fallback_counts(ctx, rpp, every):
    diff, routed, _, _ = compare(ctx, packed("cornell_32x24_r4", 7, 5, rpp), f"cornell 7x5 x{rpp}, every={every}", 2, every=every, keep_acu=(rpp == 9))
    assert diff is None, diff
    assert routed == 0, "the one-launch route exists at 4, 16 and 64 rays per pixel only"


def test_fallback_one_pass_with_every_frame_is_an_ordinary_pass(ctx):
    diff, routed, _, _ = compare(ctx, packed("cornell_32x24_r4", 7, 5, 16), "cornell 7x5 x16, 1 pass, every frame", 1, every=True)
    assert diff is None, diff
    assert routed == 0


def test_fallback_without_inpass_resolve(pkg):
    from raytracing_amd.pyhost import mirt
    os.environ["MIRT_INPASS_RESOLVE"] = "0"   # read when a context is created
    try:
        sep = mirt.Context(0)
    finally:
        del os.environ["MIRT_INPASS_RESOLVE"]
    try:
        for every in (False, True):   # (every frame: the ordinary-passes route, the guides' checks with its first pass, their launches behind its last)
            diff, routed, _, _ = compare(sep, packed("cornell_32x24_r4", 7, 5, 16), f"cornell 7x5 x16, MIRT_INPASS_RESOLVE=0, every={every}", 3, every=every)
            assert diff is None, diff
            assert routed == 0
    finally:
        sep.destroy()


def test_fallback_with_acu_and_no_output_buffer(ctx):
    from raytracing_amd.pyhost import render
    import a10_pass as A
    ps = packed("cornell_32x24_r4", 7, 5, 16)
    seeds = A.make_seeds(ps.total_rays, seed_base=5)
    _, _, _, want = compare(ctx, ps, "reference", 2)
    fr = render.FusedRenderer(ctx, ps, seeds=seeds)
    ref = render.FusedRenderer(ctx, ps, seeds=seeds)
    nh, ad = ctx.buffer(fr.npix * 16), ctx.buffer(fr.npix * 16)
    try:
        before = ctx.guided_passes()
        ctx.render_passes_guided(fr.dev.pass_desc(fr.seeds, fr.acu), 2, fresh=True, normal_hits=nh, albedo_depth=ad)
        assert ctx.guided_passes() == before
        ctx.render_passes(ref.dev.pass_desc(ref.seeds, ref.acu), 2, fresh=True)
        assert difference("normal_hits", nh.read(np.float32), want["normal_hits"]) is None and difference("albedo_depth", ad.read(np.float32), want["albedo_depth"]) is None
        assert difference("acu", fr.acu.read(np.float32), ref.acu.read(np.float32)) is None
        assert difference("acu against the resolving batch", fr.acu.read(np.float32), want["acu"]) is None
        assert np.array_equal(fr.seeds.read(np.int32), ref.seeds.read(np.int32))
    finally:
        for b in (nh, ad):
            b.release()
        fr.release()
        ref.release()


def test_forced_two_call_path_gives_the_same_bits(ctx):
    os.environ["MIRT_GUIDED_PASS"] = "0"   # read per call
    try:
        diff, routed, _, _ = compare(ctx, packed("cornell_32x24_r4", 7, 5, 16), "MIRT_GUIDED_PASS=0", 3)
    finally:
        del os.environ["MIRT_GUIDED_PASS"]
    assert diff is None, diff
    assert routed == 0


@pytest.mark.parametrize("name,forced,n", [("cornell_32x24_r4", "0", 2), ("cornell_teapot3_32x24_r4", "1", 2), ("cornell_teapot3_32x24_r4", "1", 1),
                                              ("cornell_32x24_r4", "0", 1)],
                         ids=["no_grids_plain_loop", "grids_reuse", "grids_reuse_one_pass", "no_grids_plain_loop_one_pass"])
def test_fallback_when_the_reuse_pairing_is_forced_against_the_default(ctx, name, forced, n):
    ps = packed(name, 7, 5, 16)
    os.environ["MIRT_MULTIPASS_REUSE"] = forced   # read per launch
    try:
        diff, routed, _, _ = compare(ctx, ps, f"{name}, {n} passes, MIRT_MULTIPASS_REUSE={forced}", n)
        assert diff is None, diff
        # the guided multi-pass kernels exist for the default pairing only; one pass runs the one-pass kernel, which has no pairing
        assert routed == (1 if n == 1 else 0)
        os.environ["MIRT_MULTIPASS_REUSE"] = "1" if forced == "0" else "0"   # forcing what the default is changes nothing
        diff, routed, _, _ = compare(ctx, ps, f"{name}, {n} passes, MIRT_MULTIPASS_REUSE forcing the default", n)
        assert diff is None, diff
        assert routed == (0 if "teapot" in name and n > 1 else 1)   # (several passes of a grid scene: the guide launches whatever the pairing)
    finally:
        del os.environ["MIRT_MULTIPASS_REUSE"]


# ---- refusals: nothing at all is written ---------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_leave_the_context_working(ctx):
    from raytracing_amd.pyhost import mirt, render
    ps = packed("cornell_32x24_r4", 7, 5, 16)
    fr = render.FusedRenderer(ctx, ps, seed_base=5)
    npix, nrays, n = fr.npix, fr.nrays, 3
    nh, ad, small = ctx.buffer(npix * 16), ctx.buffer(npix * 16), ctx.buffer(npix * 16 - 1)
    pixels, radiances = ctx.buffer(n * npix * 4), ctx.buffer(n * npix * 16)   # n frames, for MIRT_PASSES_EVERY_FRAME
    in_last_frame = ctx.wrap(radiances.device_ptr + (n - 1) * npix * 16, npix * 16)   # the bytes of the batch's last radiance frame
    fills = [(fr.seeds, np.arange(nrays, dtype=np.int32) * 7 + 1), (fr.acu, np.full(4 * nrays, 3.25, np.float32)), (fr.pixel, np.full(4 * npix, 0x5A, np.uint8)),
             (fr.radiance, np.full(4 * npix, 2.5, np.float32)), (nh, np.full(4 * npix, PATTERN, np.float32)), (ad, np.full(4 * npix, PATTERN, np.float32)),
             (small, np.full(npix * 16 - 1, 0xA5, np.uint8)), (pixels, np.full(n * 4 * npix, 0x3C, np.uint8)), (radiances, np.full(n * 4 * npix, 1.5, np.float32))]

    def desc(rpp=None, frames=False):
        d = fr.dev.pass_desc(fr.seeds, fr.acu, pixels if frames else fr.pixel, radiances if frames else fr.radiance)
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

    def call(d, n_passes=n, flags=mirt.PASSES_FRESH, a=nh, b=ad):
        return lambda: ctx._chk(mirt.lib().mirt_render_passes_guided(ctx.h, ctypes.byref(d), n_passes, flags, a.h if a else None, b.h if b else None))

    try:
        before = ctx.guided_passes()
        every = mirt.PASSES_FRESH | mirt.PASSES_EVERY_FRAME
        refused(-1, call(desc(), a=None, b=None), "both NULL")
        refused(-1, call(desc(1)), "seeds[col]")
        refused(-5, call(desc(), a=small), "normal_hits")
        refused(-5, call(desc(), b=small), "albedo_depth")
        refused(-1, call(desc(), a=fr.radiance), "aliases")
        refused(-1, call(desc(), b=fr.seeds), "aliases")
        refused(-1, call(desc(), b=nh), "aliases")
        refused(-1, call(desc(frames=True), flags=every, a=in_last_frame), "aliases")
        refused(-1, call(desc(frames=True), flags=every, b=in_last_frame), "aliases")
        refused(-1, call(desc(), n_passes=0), "n_passes")
        refused(-1, call(desc(), n_passes=65), "n_passes")
        refused(-1, call(desc(), flags=4), "unknown flags")
        refused(-1, call(desc(), flags=every), "frames")   # pixel and radiance hold one frame, three are asked for
        d = desc()   # (made outside the recording: a new scene would be validated and prepared here)
        for b, f in fills:
            b.write(f)
        ctx.finish()
        ctx.capture_begin()
        try:
            with pytest.raises(mirt.MirtError) as e:
                call(d)()
            assert e.value.code == -1 and "capture" in str(e.value)
        finally:
            ctx.graph_release(ctx.capture_end())
        untouched("inside a recording")
        assert ctx.guided_passes() == before
    finally:
        for b in (in_last_frame, nh, ad, small, pixels, radiances):
            b.release()
        fr.release()
    diff, routed, _, _ = compare(ctx, ps, "after the refusals", 3, every=True)
    assert diff is None, diff
    assert routed == 1


# ---- the Python hosts ---------------------------------------------------------------------------------------------------------------------------------
def test_renderer_methods(ctx):
    from raytracing_amd.pyhost import render
    ps = packed("cornell_32x24_r4", 24, 16, 4)
    a, b = render.FusedRenderer(ctx, ps, seed_base=3), render.FusedRenderer(ctx, ps, seed_base=3)
    try:
        before = ctx.guided_passes()
        got = a.denoised_passes(3, iterations=2)
        assert ctx.guided_passes() == before + 1 and a.passes == 4
        b.execute_passes(3, fresh=True)
        want = b.denoised(iterations=2)
        assert np.array_equal(got[0], want[0]) and difference("filtered", got[1], want[1]) is None
        g = b.guides()
        assert difference("normal_hits", a.normal_hits.read(np.float32), g[0]) is None and difference("albedo_depth", a.albedo_depth.read(np.float32), g[1]) is None
        assert np.array_equal(a.pixel.read(np.uint8), b.pixel.read(np.uint8)) and np.array_equal(a.seeds.read(np.int32), b.seeds.read(np.int32))
        fa, fb = a.execute_passes_guided(2, every_frame=True), b.execute_passes(2, every_frame=True)   # passes 4 and 5, a frame after each
        assert ctx.guided_passes() == before + 2
        assert np.array_equal(fa[0], fb[0]) and difference("frames", fa[1], fb[1]) is None
        assert difference("normal_hits again", a.normal_hits.read(np.float32), g[0]) is None
    finally:
        a.release()
        b.release()


def test_upscaled_renderer_uses_the_guided_call_for_several_passes(ctx):
    from raytracing_amd.pyhost import render
    ps = packed("cornell_32x24_r4", 28, 20, 4)
    a, b = render.UpscaledRenderer(ctx, ps, 2, seed_base=3), render.UpscaledRenderer(ctx, ps, 2, seed_base=3)
    try:
        before = ctx.guided_passes()
        got = a.render(passes=2)
        assert ctx.guided_passes() == before + 1
        os.environ["MIRT_GUIDED_PASS"] = "0"
        try:
            want = b.render(passes=2)
        finally:
            del os.environ["MIRT_GUIDED_PASS"]
        assert ctx.guided_passes() == before + 1
        assert np.array_equal(got[0], want[0]) and difference("upsampled", got[1], want[1]) is None
    finally:
        a.release()
        b.release()


def test_upscaled_renderer_splits_more_passes_than_one_call_runs(ctx):
    """65 passes: one more than MIRT_MAX_PASSES_PER_CALL.  The expectation is the loop of single passes with the guides call behind it, which
    render(passes=0) then filters and upsamples."""
    from raytracing_amd.pyhost import mirt, render
    n = mirt.MAX_PASSES_PER_CALL + 1
    ps = packed("cornell_32x24_r4", 28, 20, 4)
    a, b = render.UpscaledRenderer(ctx, ps, 2, seed_base=3), render.UpscaledRenderer(ctx, ps, 2, seed_base=3)
    try:
        before = ctx.guided_passes()
        got = a.render(passes=n)
        assert ctx.guided_passes() == before + 1 and a.lo.passes == n + 1   # the first call of the two wrote the guides
        for i in range(n):
            b.lo.execute_render(fresh=(i == 0))
        want = b.render(passes=0)
        assert ctx.guided_passes() == before + 1
        assert a.tone == b.tone == np.float32(1.0 / (4 * n))
        assert np.array_equal(got[0], want[0]) and difference("upsampled", got[1], want[1]) is None
        assert difference("low radiance", a.lo.radiance.read(np.float32), b.lo.radiance.read(np.float32)) is None
        assert difference("low normal_hits", a.nh_lo.read(np.float32), b.nh_lo.read(np.float32)) is None
        assert difference("low albedo_depth", a.ad_lo.read(np.float32), b.ad_lo.read(np.float32)) is None
        assert np.array_equal(a.lo.seeds.read(np.int32), b.lo.seeds.read(np.int32))
    finally:
        a.release()
        b.release()
