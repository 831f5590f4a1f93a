"""GPU: every refusal of mirt_upsample_guided (include/mirt.h) returns its code and leaves both outputs as they were -- they are pre-filled with
a pattern -- and the context works afterwards; a held command stream is flushed before the call reads the low frame."""
import ctypes as C

import numpy as np
import pytest

import a10_pass as A
from conftest import load_fixture
from filter_common import difference
from upsample_common import DEFAULTS, SYN_HL, SYN_TONE, SYN_WL, synthetic, upsample

pytestmark = pytest.mark.gpu

F = 3
W, H = SYN_WL * F, SYN_HL * F
E_ARG, E_HANDLE, E_RANGE = -1, -2, -5


@pytest.fixture(scope="module")
def ctx(pkg):
    from raytracing_amd.pyhost import mirt
    c = mirt.Context(0)
    yield c
    c.destroy()


def test_refusals_write_nothing_and_leave_the_context_working(ctx):
    from raytracing_amd.pyhost import mirt
    inputs = synthetic(SYN_WL, SYN_HL, F)
    names = ("radiance_lo", "normal_hits_lo", "albedo_depth_lo", "normal_hits", "albedo_depth")
    n, nlo = W * H, SYN_WL * SYN_HL
    # every input buffer is as large as a high image (a buffer may be larger than its image): so an input passed as an output is refused for being
    # an input, not for its size
    ins = {k: ctx.buffer(n * 16).write(np.ascontiguousarray(a, np.float32)) for k, a in zip(names, inputs)}
    out, pix = ctx.buffer(n * 16), ctx.buffer(n * 4)
    fill_out, fill_pix = np.full(n * 4, 7.5, np.float32), np.full(n * 4, 0x5A, np.uint8)
    small_lo, small_hi, small_pix = ctx.buffer(nlo * 16 - 1), ctx.buffer(n * 16 - 1), ctx.buffer(n * 4 - 1)
    carved, wrapped = ctx.buffer(n * 16 + nlo * 16), []

    def call(ctx_h=None, **over):
        d = mirt._UpsampleDesc()
        d.struct_size = C.sizeof(d)
        d.width, d.height, d.factor, d.flags, d.normal_power_log2 = W, H, F, mirt.UPSAMPLE_DEMODULATE, 5
        d.tone, d.sigma_depth = float(SYN_TONE), 0.1
        for k, b in ins.items():
            setattr(d, k, b.h)
        d.upsampled, d.pixel = out.h, pix.h
        for k, v in over.items():
            setattr(d, k, v.h if isinstance(v, mirt.Buffer) else v)
        return mirt.lib().mirt_upsample_guided(ctx.h if ctx_h is None else ctx_h, C.byref(d))

    def untouched(what):
        assert out.read(np.float32).tobytes() == fill_out.tobytes() and pix.read(np.uint8).tobytes() == fill_pix.tobytes(), f"an output was written: {what}"

    def refused(code, **over):
        out.write(fill_out)
        pix.write(fill_pix)
        assert call(**over) == code, (over, ctx.last_error())
        untouched(over)

    try:
        refused(E_ARG, struct_size=C.sizeof(mirt._UpsampleDesc) - 4)
        refused(E_ARG, width=0)
        refused(E_ARG, height=0)
        refused(E_ARG, width=65536 * 1 + 2)           # above 65535 (and a multiple of nothing that matters: the size check comes first)
        refused(E_ARG, height=65538)
        for factor in (0, 1, 5, 29):
            refused(E_ARG, factor=factor)
        refused(E_ARG, width=W + 1)                   # not a multiple of the factor
        refused(E_ARG, height=H - 1)
        refused(E_ARG, factor=2)                      # 87 x 51 is no multiple of 2
        refused(E_ARG, normal_power_log2=8)
        for tone in (0.0, -0.25, float("nan"), float("inf")):
            refused(E_ARG, tone=tone)
        refused(E_ARG, flags=2)
        refused(E_ARG, flags=0x80000001)
        refused(E_ARG, upsampled=None, pixel=None)
        for k in names:                               # aliasing: an output that is an input
            refused(E_ARG, upsampled=ins[k], pixel=None)
        refused(E_ARG, upsampled=None, pixel=ins["albedo_depth"])
        refused(E_ARG, upsampled=out, pixel=out)      # ... or the other output
        for owner in (ins["normal_hits"], out):       # ... or wrapped memory that shares SOME bytes: a pixel image 16 bytes inside an input, inside upsampled
            view = ctx.wrap(owner.device_ptr + 16, n * 4)
            wrapped.append(view)
            refused(E_ARG, pixel=view)
        assert ins["normal_hits"].read(np.float32, n * 4).tobytes() == np.ascontiguousarray(inputs[3], np.float32).tobytes(), "normal_hits was written"
        for k in names[:3]:
            refused(E_RANGE, **{k: small_lo})
        for k in names[3:]:
            refused(E_RANGE, **{k: small_hi})
        refused(E_RANGE, upsampled=small_hi)
        refused(E_RANGE, pixel=small_pix)
        refused(E_RANGE, height=H + F)                # every high buffer is one low row too small, the low ones too
        not_a_context = C.create_string_buffer(64)
        refused(E_HANDLE, ctx_h=C.c_void_p(C.addressof(not_a_context)))
        refused(E_HANDLE, radiance_lo=C.c_void_p(C.addressof(not_a_context)))
        refused(E_HANDLE, normal_hits=C.c_void_p(C.addressof(not_a_context)))
        out.write(fill_out)
        pix.write(fill_pix)
        ctx.finish()
        ctx.capture_begin()
        try:
            assert call() == E_ARG and "capture" in ctx.last_error()
        finally:
            ctx.graph_release(ctx.capture_end())
        untouched("inside a recording")
        want = upsample(*inputs, W, H, F, SYN_TONE, **DEFAULTS)
        # touching is not aliasing: upsampled ends exactly where radiance_lo begins, both carved from one allocation
        out_view, lo_view = ctx.wrap(carved.device_ptr, n * 16), ctx.wrap(carved.device_ptr + n * 16, nlo * 16)
        wrapped += [out_view, lo_view]
        lo_view.write(np.ascontiguousarray(inputs[0], np.float32))
        pix.write(fill_pix)
        assert call(radiance_lo=lo_view, upsampled=out_view) == 0, ctx.last_error()
        for tag, got, w in (("upsampled", out_view.read(np.float32).reshape(-1, 4), want[0]), ("pixel", pix.read(np.uint8).reshape(-1, 4), want[1])):
            d = difference(f"upsampled ends where radiance_lo begins, {tag}", got, w)
            assert d is None, d
        # the context works afterwards
        out.write(fill_out)
        pix.write(fill_pix)
        assert call() == 0, ctx.last_error()
        for tag, got, w in (("upsampled", out.read(np.float32).reshape(-1, 4), want[0]), ("pixel", pix.read(np.uint8).reshape(-1, 4), want[1])):
            d = difference(f"after the refusals, {tag}", got, w)
            assert d is None, d
    finally:
        for b in wrapped + list(ins.values()) + [out, pix, carved, small_lo, small_hi, small_pix]:
            b.release()


def test_a_held_enqueue_stream_is_flushed_before_the_upsampler_reads_the_low_frame(pkg):
    """fusion level 2 holds the pass's enqueues back until its copyToPixel; a pass without one stays held.  The upsampler observes device state,
    so it runs the held pass first: the accumulators it then reads are the pass's (as tests/test_filter.py shows for the filter)."""
    from raytracing_amd.pyhost import mirt, render, scene
    _, sc0 = load_fixture("cornell_32x24_r4")
    ps = scene.PackedScene(dict(sc0.d)).resized(32, 24, 4)
    seeds = A.make_seeds(ps.total_rays)
    f, w, h = 2, 64, 48
    c = mirt.Context(0)
    try:
        want = None
        for level in (0, 2):
            c.set_fusion(level)
            gr = render.GranularRenderer(c, ps, seeds=seeds)
            nlo, n = ps.width * ps.height, w * h
            nh_lo, ad_lo, nh, ad, out = c.buffer(nlo * 16), c.buffer(nlo * 16), c.buffer(n * 16), c.buffer(n * 16), c.buffer(n * 16)
            try:
                d = gr.dev.pass_desc(None, None)
                c.render_guides(d, nh_lo, ad_lo)
                hi = ps.resized(w, h, 4)
                d.width, d.height, d.cam = w, h, mirt._f(hi.cam, 16)
                c.render_guides(d, nh, ad)
                gr._enqueue_segments(5)          # executeRender's enqueues without the copyToPixel: at level 2 they are all still held
                acu_view = mirt.Buffer(c, gr.b["acu"].h, nlo * 16)   # a view of the per-ray accumulator's first nlo float4 stands in for a radiance image
                c.upsample_guided(w, h, f, 0.25, acu_view, nh_lo, ad_lo, nh, ad, upsampled=out)
                got = out.read(np.float32)
                assert np.isfinite(got).all() and got.any()
                if want is None:
                    want = got
                else:
                    diff = difference("fusion level 2 against level 0", got, want)
                    assert diff is None, diff
            finally:
                for b in (nh_lo, ad_lo, nh, ad, out):
                    b.release()
                gr.release()
    finally:
        c.destroy()
