"""GPU: mirt_filter_atrous -- the edge-avoiding a-trous filter guided by the first-hit guide buffers (include/mirt.h) -- through the C ABI,
tolerance 0 against the numpy restatement of the header's definition (tests/filter_common.py; every NaN equal to every NaN):

  1. synthetic inputs at 83x47 with planted cases (background scattered and in blocks, NaN / +inf / -0 radiance, zero and negative albedo
     channels, z == 0, a pixel whose taps all weigh 0), at 7x5 and at 1x1: iterations 0 .. 5, DEMODULATE on and off, each edge term on and off,
     normal_power_log2 0 / 3 / 7, filtered alone, pixel alone, both -- through each of the two kernel structures and the shipped choice;
  2. rendered inputs: cornell and cornell_teapot3 at 96x54 x 4, radiance from mirt_render_first_pass, guides from mirt_render_guides, also under
     mirt_ctx_set_exact_only;
  3. the anchor: iterations == 0 without DEMODULATE gives radiance back and the pass's own pixel buffer; two progressive passes;
  4. properties, refusals, the held command stream;
  5. quality: the filtered 4-ray frame is closer to the converged frame than the unfiltered one (profiles/filter/quality.json);
  6. libmirt_default.so gives the same bits (a child process)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import a10_pass as A
from conftest import ROOT, load_fixture
from filter_common import DEFAULTS, NAN_AT, SYN_H, SYN_TONE, SYN_W, atrous, difference, synthetic, tone_map

pytestmark = pytest.mark.gpu

DEFAULT_LIB = os.path.join(ROOT, "2015-raytracing_amd", "libmirt_default.so")
OFF = dict(iterations=0, normal_power_log2=0, sigma_depth=0.0, sigma_colour=0.0, demodulate=False)


@pytest.fixture(scope="module")
def ctx(pkg):
    from raytracing_amd.pyhost import mirt
    c = mirt.Context(0)
    yield c
    c.destroy()


class Filter:
    """three input buffers and two outputs of one image size, driven through mirt_filter_atrous"""

    def __init__(self, ctx, width, height, inputs=None):
        self.ctx, self.w, self.h = ctx, width, height
        n = width * height
        self.rad, self.nh, self.ad = (ctx.buffer(n * 16) for _ in range(3))
        self.out, self.pix = ctx.buffer(n * 16), ctx.buffer(n * 4)
        if inputs is not None:
            for b, a in zip((self.rad, self.nh, self.ad), inputs):
                b.write(np.ascontiguousarray(a, np.float32))

    def run(self, tone, filtered=True, pixel=True, structure=None, **p):
        n = self.w * self.h
        self.out.write(np.full(n * 4, 7.5, np.float32))
        self.pix.write(np.full(n * 4, 0x5A, np.uint8))
        self.ctx.filter_atrous(self.w, self.h, tone, self.rad, self.nh, self.ad, filtered=self.out if filtered else None,
                               pixel=self.pix if pixel else None, structure=structure, **p)
        return self.out.read(np.float32).reshape(-1, 4), self.pix.read(np.uint8).reshape(-1, 4)

    def release(self):
        for b in (self.rad, self.nh, self.ad, self.out, self.pix):
            b.release()


def check(tag, got, want, filtered=True, pixel=True):
    if filtered:
        d = difference(f"{tag} filtered", got[0], want[0])
        assert d is None, d
    if pixel:
        d = difference(f"{tag} pixel", got[1], want[1])
        assert d is None, d


# ---- 1. synthetic inputs ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def syn():
    return synthetic()


@pytest.fixture(scope="module")
def syn_filter(ctx, syn):
    f = Filter(ctx, SYN_W, SYN_H, syn)
    yield f
    f.release()


_want = {}


def expected(syn, **p):
    """the restatement on the synthetic inputs, computed once per parameter set"""
    key = tuple(sorted(p.items()))
    if key not in _want:
        _want[key] = atrous(*syn, SYN_W, SYN_H, SYN_TONE, **p)
    return _want[key]


@pytest.mark.parametrize("structure", [None, "direct", "tiled"])
@pytest.mark.parametrize("demodulate", [False, True])
@pytest.mark.parametrize("iterations", [0, 1, 2, 3, 4, 5])
def test_synthetic_iterations(syn, syn_filter, iterations, demodulate, structure):
    p = dict(DEFAULTS, iterations=iterations, demodulate=demodulate)
    check(f"{iterations} iterations demodulate={demodulate} {structure}", syn_filter.run(SYN_TONE, structure=structure, **p), expected(syn, **p))


@pytest.mark.parametrize("structure", ["direct", "tiled"])
@pytest.mark.parametrize("npow", [0, 3, 7])
@pytest.mark.parametrize("sigma_depth,sigma_colour", [(0.0, 0.0), (0.1, 0.0), (0.0, 2.0), (0.1, 2.0), (float("nan"), float("inf")), (-1.0, 0.25)])
def test_synthetic_edge_terms(syn, syn_filter, sigma_depth, sigma_colour, npow, structure):
    p = dict(iterations=3, normal_power_log2=npow, sigma_depth=sigma_depth, sigma_colour=sigma_colour, demodulate=True)
    check(f"depth {sigma_depth} colour {sigma_colour} power 2^{npow} {structure}", syn_filter.run(SYN_TONE, structure=structure, **p), expected(syn, **p))


@pytest.mark.parametrize("structure", ["direct", "tiled"])
def test_synthetic_every_tap_at_every_step(syn, syn_filter, structure):
    """the colour term off: the weights do not shrink with the step, so the steps 8 and 16 add taps to nearly every pixel"""
    p = dict(DEFAULTS, iterations=5, sigma_colour=0.0)
    check(f"5 iterations without the colour term {structure}", syn_filter.run(SYN_TONE, structure=structure, **p), expected(syn, **p))


@pytest.mark.parametrize("filtered,pixel", [(True, False), (False, True), (True, True)])
def test_either_output_alone(syn, syn_filter, filtered, pixel):
    p = dict(DEFAULTS, iterations=2)
    got = syn_filter.run(SYN_TONE, filtered=filtered, pixel=pixel, **p)
    check("outputs", got, expected(syn, **p), filtered, pixel)
    if not filtered:
        assert (got[0] == 7.5).all(), "filtered was written though it was not passed"
    if not pixel:
        assert (got[1] == 0x5A).all(), "pixel was written though it was not passed"


@pytest.mark.parametrize("structure", ["direct", "tiled"])
@pytest.mark.parametrize("w,h", [(7, 5), (1, 1)])
def test_images_smaller_than_the_kernel(ctx, w, h, structure):
    inputs = synthetic(w, h, seed=11)
    f = Filter(ctx, w, h, inputs)
    try:
        for it in (0, 1, 5):
            for demod in (False, True):
                p = dict(DEFAULTS, iterations=it, demodulate=demod)
                check(f"{w}x{h} {it} iterations demodulate={demod} {structure}", f.run(SYN_TONE, structure=structure, **p), atrous(*inputs, w, h, SYN_TONE, **p))
    finally:
        f.release()


# ---- 2. rendered inputs -----------------------------------------------------------------------------------------------------------------------
def resized(name, w, h, rpp):
    from raytracing_amd.pyhost import scene
    _, sc0 = load_fixture(name)
    return scene.PackedScene(dict(sc0.d)).resized(w, h, rpp)


class Rendered:
    """a 96x54 x 4 frame on the device: `passes` progressive passes (the first one fresh), its guides, and everything read back"""

    def __init__(self, ctx, name, passes=1, w=96, h=54, rpp=4):
        from raytracing_amd.pyhost import render
        self.ctx, self.ps = ctx, resized(name, w, h, rpp)
        self.fr = render.FusedRenderer(ctx, self.ps, seeds=A.make_seeds(self.ps.total_rays))
        n = w * h
        self.nh, self.ad = ctx.buffer(n * 16), ctx.buffer(n * 16)
        for p in range(passes):
            self.fr.execute_render(fresh=(p == 0))
        ctx.render_guides(self.fr.dev.pass_desc(None, None), self.nh, self.ad)
        self.tone = np.float32(1.0 / (rpp * passes))
        self.inputs = tuple(b.read(np.float32).reshape(-1, 4) for b in (self.fr.radiance, self.nh, self.ad))
        self.pass_pixel = self.fr.pixel.read(np.uint8).reshape(-1, 4)
        self.out, self.pix = ctx.buffer(n * 16), ctx.buffer(n * 4)

    def run(self, **p):
        self.ctx.filter_atrous(self.ps.width, self.ps.height, self.tone, self.fr.radiance, self.nh, self.ad, filtered=self.out, pixel=self.pix, **p)
        return self.out.read(np.float32).reshape(-1, 4), self.pix.read(np.uint8).reshape(-1, 4)

    def want(self, **p):
        return atrous(*self.inputs, self.ps.width, self.ps.height, self.tone, **p)

    def release(self):
        for b in (self.nh, self.ad, self.out, self.pix):
            b.release()
        self.fr.release()


@pytest.mark.parametrize("exact_only", [False, True])
@pytest.mark.parametrize("name", ["cornell_32x24_r4", "cornell_teapot3_32x24_r4"])
def test_rendered_frames(ctx, name, exact_only):
    ctx.set_exact_only(exact_only)
    try:
        r = Rendered(ctx, name)
        try:
            assert (r.inputs[1][:, 3] > 0).mean() > 0.5
            for it in (3, 5):
                p = dict(DEFAULTS, iterations=it)
                check(f"{name} exact_only={exact_only} {it} iterations", r.run(**p), r.want(**p))
        finally:
            r.release()
    finally:
        ctx.set_exact_only(False)


# ---- 3. the anchor ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_32x24_r4", "cornell_teapot3_32x24_r4"])
def test_zero_iterations_give_the_pass_its_own_frame_back(ctx, name):
    r = Rendered(ctx, name)
    try:
        filtered, pixel = r.run(**OFF)
        d = difference("filtered against radiance", filtered, r.inputs[0])
        assert d is None, d
        d = difference("pixel against the pass's pixel buffer", pixel, r.pass_pixel)
        assert d is None, d
    finally:
        r.release()


def test_two_progressive_passes_use_their_tone(ctx):
    r = Rendered(ctx, "cornell_32x24_r4", passes=2)
    try:
        assert r.tone == np.float32(1.0 / 8.0)
        d = difference("pixel against the second pass's pixel buffer", r.run(**OFF)[1], r.pass_pixel)
        assert d is None, d
        p = dict(DEFAULTS, iterations=3)
        check("two passes, 3 iterations", r.run(**p), r.want(**p))
        pix, out = r.fr.denoised(iterations=3)   # the renderer's own route: guides + filter of its current radiance
        check("FusedRenderer.denoised", (out, pix), r.want(**p))
    finally:
        r.release()


# ---- 4. properties, refusals, the held stream -------------------------------------------------------------------------------------------------
def test_properties(syn, syn_filter):
    R, NH, AD = syn
    p = dict(DEFAULTS, iterations=5)
    a = [x.copy() for x in syn_filter.run(SYN_TONE, **p)]
    b = syn_filter.run(SYN_TONE, **p)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), "two calls differ"
    for name, buf, want in (("radiance", syn_filter.rad, R), ("normal_hits", syn_filter.nh, NH), ("albedo_depth", syn_filter.ad, AD)):
        assert buf.read(np.float32).tobytes() == np.ascontiguousarray(want, np.float32).tobytes(), f"{name} changed"
    nan_in = np.isnan(R[:, :3]).any(axis=1)
    nan_out = np.isnan(a[0][:, :3]).any(axis=1)
    assert nan_in[NAN_AT[0] * SYN_W + NAN_AT[1]] and np.array_equal(nan_in, nan_out), "a NaN pixel stays NaN and no neighbour becomes NaN"
    bg = ~(NH[:, 3] > 0)
    d = difference("background pixels", a[0][bg], R[bg])
    assert bg.any() and d is None, d


def test_refusals_write_nothing_and_leave_the_context_working(ctx, syn, syn_filter):
    import ctypes as C
    from raytracing_amd.pyhost import mirt
    f = syn_filter
    n = SYN_W * SYN_H
    fill_out, fill_pix = np.full(n * 4, 7.5, np.float32), np.full(n * 4, 0x5A, np.uint8)
    small16, small4 = ctx.buffer(n * 16 - 1), ctx.buffer(n * 4 - 1)
    carved, wrapped = ctx.buffer(2 * n * 16), []

    def call(ctx_h=None, **over):
        d = mirt._FilterDesc()
        d.struct_size = C.sizeof(d)
        d.width, d.height, d.iterations, d.flags, d.normal_power_log2 = SYN_W, SYN_H, 2, mirt.FILTER_DEMODULATE, 3
        d.tone, d.sigma_depth, d.sigma_colour = 0.25, 0.1, 2.0
        d.radiance, d.normal_hits, d.albedo_depth, d.filtered, d.pixel = f.rad.h, f.nh.h, f.ad.h, f.out.h, f.pix.h
        for k, v in over.items():
            setattr(d, k, v.h if isinstance(v, mirt.Buffer) else v)
        return mirt.lib().mirt_filter_atrous(ctx.h if ctx_h is None else ctx_h, C.byref(d))

    def refused(code, **over):
        f.out.write(fill_out)
        f.pix.write(fill_pix)
        assert call(**over) == code, (over, ctx.last_error())
        assert f.out.read(np.float32).tobytes() == fill_out.tobytes() and f.pix.read(np.uint8).tobytes() == fill_pix.tobytes(), f"an output was written: {over}"

    before = Rendered(ctx, "cornell_32x24_r4", w=32, h=24)
    pass_before = before.pass_pixel
    before.release()
    try:
        E_ARG, E_HANDLE, E_RANGE = -1, -2, -5
        refused(E_ARG, struct_size=76)
        refused(E_ARG, width=0)
        refused(E_ARG, height=0)
        refused(E_ARG, iterations=6)
        refused(E_ARG, normal_power_log2=8)
        for tone in (0.0, -0.25, float("nan"), float("inf")):
            refused(E_ARG, tone=tone)
        refused(E_ARG, flags=8)
        refused(E_ARG, flags=mirt.FILTER_DIRECT | mirt.FILTER_TILED)
        refused(E_ARG, filtered=None, pixel=None)
        refused(E_ARG, filtered=f.rad, pixel=None)      # aliasing: an output that is an input
        refused(E_ARG, filtered=f.nh)
        refused(E_ARG, filtered=None, pixel=f.ad)
        for owner in (f.rad, f.out):                    # ... or wrapped memory that shares SOME bytes: a pixel image 16 bytes inside radiance, inside filtered
            view = ctx.wrap(owner.device_ptr + 16, n * 4)
            wrapped.append(view)
            refused(E_ARG, pixel=view)
        assert f.rad.read(np.float32).tobytes() == np.ascontiguousarray(syn[0], np.float32).tobytes(), "radiance was written"
        refused(E_RANGE, radiance=small16)
        refused(E_RANGE, normal_hits=small16)
        refused(E_RANGE, albedo_depth=small16)
        refused(E_RANGE, filtered=small16)
        refused(E_RANGE, pixel=small4)
        refused(E_RANGE, height=SYN_H + 1)
        not_a_context = C.create_string_buffer(64)
        refused(E_HANDLE, ctx_h=C.c_void_p(C.addressof(not_a_context)))
        refused(E_HANDLE, radiance=C.c_void_p(C.addressof(not_a_context)))
        f.out.write(fill_out)
        f.pix.write(fill_pix)
        ctx.finish()
        ctx.capture_begin()
        try:
            assert call() == E_ARG and "capture" in ctx.last_error()
        finally:
            ctx.graph_release(ctx.capture_end())
        assert f.out.read(np.float32).tobytes() == fill_out.tobytes() and f.pix.read(np.uint8).tobytes() == fill_pix.tobytes(), "written inside a recording"
        # touching is not aliasing: filtered ends exactly where radiance begins, both carved from one allocation
        out_view, rad_view = ctx.wrap(carved.device_ptr, n * 16), ctx.wrap(carved.device_ptr + n * 16, n * 16)
        wrapped += [out_view, rad_view]
        rad_view.write(np.ascontiguousarray(syn[0], np.float32))
        f.pix.write(fill_pix)
        assert call(radiance=rad_view, filtered=out_view) == 0, ctx.last_error()
        check("filtered ends where radiance begins", (out_view.read(np.float32).reshape(-1, 4), f.pix.read(np.uint8).reshape(-1, 4)),
              atrous(*syn, SYN_W, SYN_H, np.float32(0.25), iterations=2, normal_power_log2=3, sigma_depth=0.1, sigma_colour=2.0, demodulate=True))
        # the context works afterwards: the filter, and a pass
        p = dict(DEFAULTS, iterations=2, normal_power_log2=3)
        check("after the refusals", f.run(SYN_TONE, **p), atrous(*syn, SYN_W, SYN_H, SYN_TONE, **p))
        r = Rendered(ctx, "cornell_32x24_r4", w=32, h=24)
        try:
            assert r.pass_pixel.any() and np.array_equal(r.pass_pixel, pass_before), "a pass after the refusals"
        finally:
            r.release()
    finally:
        for b in wrapped + [carved, small16, small4]:
            b.release()


def test_a_held_enqueue_stream_is_flushed_before_the_filter_reads_radiance(pkg):
    """fusion level 2 holds the pass's enqueues back until its copyToPixel; a pass without one stays held.  The filter observes device state, so
    it runs the held pass first: the accumulators it then reads are the pass's."""
    from raytracing_amd.pyhost import mirt, render
    ps = resized("cornell_32x24_r4", 32, 24, 4)
    seeds = A.make_seeds(ps.total_rays)
    c = mirt.Context(0)
    try:
        want = None
        for level in (0, 2):
            c.set_fusion(level)
            gr = render.GranularRenderer(c, ps, seeds=seeds)
            n = ps.width * ps.height
            nh, ad, out = c.buffer(n * 16), c.buffer(n * 16), c.buffer(n * 16)
            rad = c.buffer(n * 16)
            try:
                c.render_guides(gr.dev.pass_desc(None, None), nh, ad)
                gr._enqueue_segments(5)          # executeRender's enqueues without the copyToPixel: at level 2 they are all still held
                # the per-ray accumulator at 1 ray ... 4 rays per pixel is not a radiance image; a wrapped view of it is: filter acu's first n float4
                acu_view = mirt.Buffer(c, gr.b["acu"].h, n * 16)
                c.filter_atrous(ps.width, ps.height, 0.25, acu_view, nh, ad, filtered=out, **dict(DEFAULTS, iterations=2))
                got = out.read(np.float32)
                assert np.isfinite(got).all() and got.any()
                if want is None:
                    want = got
                else:
                    d = difference("fusion level 2 against level 0", got, want)
                    assert d is None, d
            finally:
                for b in (nh, ad, out, rad):
                    b.release()
                gr.release()
    finally:
        c.destroy()


# ---- 5. quality -------------------------------------------------------------------------------------------------------------------------------
def test_the_filtered_frame_is_closer_to_the_converged_frame(ctx):
    """expected behaviour, not bits: cornell 96x54, 4 rays filtered with the shipped defaults against 256 rays x 4 passes of this library, mean
    squared error over the tone-mapped floats before quantisation.  The assertion is only `smaller`."""
    from raytracing_amd.pyhost import render
    conv = render.FusedRenderer(ctx, resized("cornell_32x24_r4", 96, 54, 256), seed_base=5)
    r = Rendered(ctx, "cornell_32x24_r4")
    try:
        for p in range(4):
            conv.execute_render(fresh=(p == 0))
        ref = tone_map(conv.radiance.read(np.float32).reshape(-1, 4)[:, :3], np.float32(1.0 / 1024.0)).astype(np.float64)
        noisy = tone_map(r.inputs[0][:, :3], r.tone).astype(np.float64)
        filtered, _ = r.run(**DEFAULTS)
        den = tone_map(filtered[:, :3], r.tone).astype(np.float64)
        mse_noisy, mse_filtered = float(((noisy - ref) ** 2).mean()), float(((den - ref) ** 2).mean())
        print(f"mse against 256 rays x 4 passes: unfiltered {mse_noisy:.3f}, filtered {mse_filtered:.3f}")
        if os.environ.get("MIRT_FILTER_QUALITY_JSON"):   # how profiles/filter/quality.json is made
            with open(os.environ["MIRT_FILTER_QUALITY_JSON"], "w") as fh:
                json.dump({"scene": "cornell", "width": 96, "height": 54, "rays_per_pixel": 4, "converged": "256 rays x 4 passes", "parameters": DEFAULTS,
                           "mse_unfiltered": round(mse_noisy, 4), "mse_filtered": round(mse_filtered, 4)}, fh, indent=1)
                fh.write("\n")
        assert mse_filtered < mse_noisy
    finally:
        r.release()
        conv.release()


# ---- 6. the default contract ------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(DEFAULT_LIB), reason="needs libmirt_default.so")
def test_the_default_contract_library_gives_the_same_bits():
    """libmirt_default.so against the restatement on the synthetic inputs, in a process of its own (a process loads one libmirt)"""
    env = dict(os.environ, MIRT_CONTRACT="default")
    env.pop("MIRT_LIB_PATH", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "filter_default_child.py")], env=env, capture_output=True, text=True, timeout=600)
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0, (lines[-1:] or r.stderr[-2000:])
    assert lines and all(l["ok"] for l in lines)
