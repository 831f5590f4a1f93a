"""GPU: batched view cameras -- mirt_view_rays_batch, mirt_render_view_batch (include/mirt.h) -- through the C ABI, tolerance 0 (conftest.bits:
every NaN equal to every NaN).  The definition is by composition, so the yardstick is the single call:

  1. the rays against the numpy restatement, per camera and concatenated (tests/view_batch_common.py), for the three models at 5 x 3 k = 2,
     N = 3 (60 rays a frame: one wave holds two frames), 13 x 7 k = 1, N = 3 (91), 1 x 1 k = 1, N = 5 (five frames in five lanes) and 3 x 1
     k = 16, N = 2 (a pixel is a block); sentinel bytes behind the records stay untouched;
  2. the frames against this library's own N single mirt_render_view calls in seeds, radiance and pixel: both fixtures x three models at
     13 x 7 k = 2, N = 3, bounces 2, under the optimistic / exact pair and under set_exact_only(True); every k at 5 x 3, N = 3;
  3. the frames against the oracle: one fixture x three models at 5 x 3 k = 2, N = 2 (120 rays);
  4. a fresh batch call, then one with MIRT_VIEW_ACCUMULATE and tone 1 / (4 * 2), equal the per-frame chain; pixel only, radiance only; N = 1
     against mirt_render_view;
  5. mixed deferral: ORTHOGRAPHIC at 13 x 7 k = 2 where the middle camera of three looks along -z, so the ray-side guard refuses every ray
     of its frame (rays 364 .. 727: blocks 1 and 2) -- the frames equal the singles, mirt_view_deferred is a multiple of 256 and at least
     512, and 0 under exact_only;
  6. every refusal of the header's list, the buffers pre-filled and compared afterwards; then cornell_32x24_r4 still renders correctly.
"""
import ctypes as C

import numpy as np
import pytest

import a10_pass as A
import view_batch_common as VB
import view_common as V
from conftest import bits, load_fixture

pytestmark = pytest.mark.gpu

E_ARG, E_HANDLE, E_RANGE, E_DATA = -1, -2, -5, -8
FIXTURES = ("cornell_32x24_r4", "cornell_teapot3_32x24_r4")
MODELS = ("ortho", "equirect", "fisheye")
W, H, N, BOUNCES = 13, 7, 3, 2
CAP_RAYS, CAP_PIXELS = N * max(W * H * 4, 5 * 3 * 256), N * W * H

_SCENES = {}


def scene(name):
    if name not in _SCENES:
        _SCENES[name] = load_fixture(name)[1]
    return _SCENES[name]


@pytest.fixture(scope="module")
def ctx(pkg):
    from raytracing_amd.pyhost import mirt
    c = mirt.Context(0)
    yield c
    c.destroy()


@pytest.fixture(scope="module")
def renderers(ctx):
    made = {}

    def get(name):
        if name not in made:
            made[name] = VB.BatchRenderer(ctx, scene(name), CAP_RAYS, CAP_PIXELS)
        return made[name]
    yield get
    for r in made.values():
        r.release()


def same(tag, got, want):
    d = V.differ(tag, got, want)
    assert d is None, d
    assert got[3], f"{tag}: bytes behind the records, or a buffer that was not given, were written"


# ---- 1. the rays ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,height,k,n", [(5, 3, 2, 3), (13, 7, 1, 3), (1, 1, 1, 5), (3, 1, 16, 2)])
@pytest.mark.parametrize("model", MODELS)
def test_batch_rays_equal_the_restatement(ctx, model, width, height, k, n):
    sc = scene(FIXTURES[0])
    v = V.standard_view(sc, model, width=width, height=height, k=k, t_min=0.03125, t_max=1000.0)
    v = v.with_(eye=np.full(3, np.nan, np.float32), forward=np.full(3, np.inf, np.float32))   # the descriptor's own basis is not read
    cams = VB.cameras(sc, n)
    total, tail = n * v.n_rays, 96
    buf = ctx.buffer(total * 32 + tail)
    try:
        buf.write(np.full(buf.nbytes, V.SENTINEL, np.uint8))
        ctx.view_rays_batch(v.desc(), cams, buf)
        raw = buf.read(np.uint8)
        got, want = raw[:total * 32].view(np.float32).reshape(-1, 8), VB.batch_rays(v, cams)
        bad = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
        assert bad.size == 0, (f"{model} {width}x{height} k={k} N={n}: {bad.size} of {total} rays differ; first is ray {int(bad[0])} (frame {int(bad[0]) // v.n_rays}): "
                               f"got {got[bad[0]].tolist()}, want {want[bad[0]].tolist()}")
        assert (raw[total * 32:] == V.SENTINEL).all(), "bytes behind the records were written"
    finally:
        buf.release()


# ---- 2. the frames against this library's own single calls ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact_only", [False, True], ids=["pair", "exact_only"])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", FIXTURES)
def test_the_frames_equal_the_single_calls(ctx, renderers, name, model, exact_only):
    sc, r = scene(name), renderers(name)
    v = V.standard_view(sc, model, tone=0.25)
    cams = VB.cameras(sc, N)
    seeds = A.make_seeds(N * v.n_rays)
    ctx.set_exact_only(exact_only)
    try:
        want = r.singles(v, cams, seeds, bounces=BOUNCES)
        assert (want[1][:, 3] > 0).any(), "no pixel received light"
        assert (want[0] != seeds).any(), "no seed advanced"
        same(f"{name} {model} exact_only={exact_only}", r.run_batch(v, cams, seeds, bounces=BOUNCES), want)
        if not exact_only:
            print(f"{name} {model}: deferred {ctx.view_deferred()} of {N * v.n_rays} rays")
    finally:
        ctx.set_exact_only(False)


@pytest.mark.parametrize("k", V.KS)
def test_the_frames_equal_the_single_calls_at_every_k(renderers, k):
    name = FIXTURES[1]
    sc, r = scene(name), renderers(name)
    v = V.standard_view(sc, "equirect", width=5, height=3, k=k, tone=1.0 / (k * k))
    cams = VB.cameras(sc, N)
    seeds = A.make_seeds(N * v.n_rays)
    want = r.singles(v, cams, seeds, bounces=BOUNCES)
    assert (want[1][:, 3] > 0).any(), "no pixel received light"
    same(f"{name} equirect 5x3 k={k}", r.run_batch(v, cams, seeds, bounces=BOUNCES), want)


# ---- 3. the frames against the oracle -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_the_frames_equal_the_oracle(renderers, model):
    name = FIXTURES[1]
    sc, r = scene(name), renderers(name)
    v = V.standard_view(sc, model, width=5, height=3, k=2, tone=0.25)
    cams = VB.cameras(sc, 2)
    seeds = A.make_seeds(2 * v.n_rays)
    want = VB.expected_batch(sc, v, cams, seeds, BOUNCES)
    assert (want[1][:, 3] > 0).any(), "no pixel received light"
    same(f"{name} {model} against the oracle", r.run_batch(v, cams, seeds, bounces=BOUNCES), want)


# ---- 4. progressive, single outputs, one frame ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_accumulate_continues_every_frames_chain(renderers, model):
    name = FIXTURES[0]
    sc, r = scene(name), renderers(name)
    cams = VB.cameras(sc, N)
    v1, v2 = V.standard_view(sc, model, tone=0.25), V.standard_view(sc, model, tone=1.0 / (4 * 2))
    seeds = A.make_seeds(N * v1.n_rays)
    w1 = r.singles(v1, cams, seeds, bounces=BOUNCES)
    w2 = r.singles(v2, cams, w1[0], bounces=BOUNCES, carry=w1[1])
    pre = np.random.default_rng(5).uniform(0.0, 4.0, size=(N * v1.n_pixels, 4)).astype(np.float32)
    g1 = r.run_batch(v1, cams, seeds, bounces=BOUNCES, prefill=pre)   # a fresh call ignores what the radiance buffer held
    same(f"{model} fresh", g1, w1)
    g2 = r.run_batch(v2, cams, g1[0], bounces=BOUNCES, carry=g1[1])
    same(f"{model} accumulate", g2, w2)
    assert (bits(g2[1]) != bits(g1[1])).any() and (g2[1][:, 3] >= g1[1][:, 3]).all(), "the second call added to the first's sums"


@pytest.mark.parametrize("model", MODELS)
def test_one_output_alone_is_what_both_give(renderers, model):
    name = FIXTURES[1]
    sc, r = scene(name), renderers(name)
    v = V.standard_view(sc, model, tone=0.25)
    cams = VB.cameras(sc, N)
    seeds = A.make_seeds(N * v.n_rays)
    sd, sums, px = r.singles(v, cams, seeds, bounces=BOUNCES)
    same(f"{model} pixel only", r.run_batch(v, cams, seeds, bounces=BOUNCES, radiance=False), (sd, None, px))
    same(f"{model} radiance only", r.run_batch(v.with_(tone=float("nan")), cams, seeds, bounces=BOUNCES, pixel=False), (sd, sums, None))


@pytest.mark.parametrize("model", MODELS)
def test_one_frame_is_render_view(renderers, model):
    name = FIXTURES[0]
    sc, r = scene(name), renderers(name)
    v = V.standard_view(sc, model, tone=0.25)
    cams = VB.cameras(sc, 3)[1:2]
    seeds = A.make_seeds(v.n_rays)
    want = r.run(VB.frame_view(v, cams[0]), seeds, bounces=BOUNCES)
    assert want[3]
    same(f"{model} N=1", r.run_batch(v, cams, seeds, bounces=BOUNCES), want)


# ---- 5. mixed deferral --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_a_frame_the_guard_refuses_goes_to_the_exact_kernel_among_frames_that_do_not(ctx, renderers, name):
    sc, r = scene(name), renderers(name)
    v = V.standard_view(sc, "ortho", tone=0.25)
    cams = VB.cameras(sc, N)
    cams[1, 3:12] = (1, 0, 0, 0, 1, 0, 0, 0, -1)   # the middle frame, rays 364 .. 727: forward has zero components, outside the ray-side guard
    assert v.n_rays == 364
    seeds = A.make_seeds(N * v.n_rays)
    want = r.singles(v, cams, seeds, bounces=BOUNCES)
    assert (want[1][:, 3] > 0).any(), "no pixel received light"
    same(f"{name} mixed, pair", r.run_batch(v, cams, seeds, bounces=BOUNCES), want)
    deferred = ctx.view_deferred()
    print(f"{name}: deferred {deferred} of {N * v.n_rays} rays")
    assert deferred % 256 == 0 and deferred >= 512, deferred
    ctx.set_exact_only(True)
    try:
        same(f"{name} mixed, exact_only", r.run_batch(v, cams, seeds, bounces=BOUNCES), want)
        assert ctx.view_deferred() == 0, "the exact kernel alone defers nothing"
    finally:
        ctx.set_exact_only(False)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_leave_the_context_working(ctx, pkg):
    from raytracing_amd.pyhost import mirt, render
    L = mirt.lib()
    name = FIXTURES[0]
    sc = scene(name)
    view = V.standard_view(sc, "equirect", tone=0.25)
    good = VB.cameras(sc, N)
    n, npx = N * view.n_rays, N * view.n_pixels
    r = VB.BatchRenderer(ctx, sc, n, npx, tail=0)
    desc = r.scene_desc(BOUNCES)
    short_seeds, short_rad, short_pix, short_rays = ctx.buffer(n * 4 - 1), ctx.buffer(npx * 16 - 1), ctx.buffer(npx * 4 - 1), ctx.buffer(n * 32 - 1)
    rays_buf = ctx.buffer(n * 32)
    outputs = (r.seeds, r.radiance, r.pixel, short_seeds, short_rad, short_pix, rays_buf, short_rays)
    extra = []

    def h(b):
        return b.h if isinstance(b, mirt.Buffer) else b

    def vd(flags=0, **fields):
        d = view.desc(flags)
        for k, val in fields.items():
            setattr(d, k, (C.c_float * 3)(*val) if isinstance(val, tuple) else val)
        return d

    def cptr(cams):
        return None if cams is None else np.ascontiguousarray(cams, np.float32).ctypes.data_as(C.c_void_p)

    def call(c=None, desc=desc, vd=vd(), cams=good, nf=N, seeds=r.seeds, radiance=r.radiance, pixel=r.pixel):
        keep = None if cams is None else np.ascontiguousarray(cams, np.float32)
        return L.mirt_render_view_batch(c or ctx.h, C.byref(desc) if desc is not None else None, C.byref(vd) if vd is not None else None, cptr(keep), nf,
                                        h(seeds), h(radiance), h(pixel))

    def call_rays(c=None, vd=vd(), cams=good, nf=N, rays=rays_buf):
        keep = None if cams is None else np.ascontiguousarray(cams, np.float32)
        return L.mirt_view_rays_batch(c or ctx.h, C.byref(vd) if vd is not None else None, cptr(keep), nf, h(rays))

    def fill():
        for b in outputs:
            b.write(np.full(b.nbytes, V.SENTINEL, np.uint8))

    def clean(what):
        for b in outputs:
            assert (b.read(np.uint8) == V.SENTINEL).all(), f"{what}: a buffer was written"

    def refused(code, **over):
        fill()
        assert call(**over) == code, (list(over), ctx.last_error())
        clean(list(over))

    def refused_rays(code, **over):
        fill()
        assert call_rays(**over) == code, (list(over), ctx.last_error())
        clean(list(over))

    def changed(**fields):
        d = r.scene_desc(BOUNCES)
        for k, val in fields.items():
            setattr(d, k, val)
        return d

    nan, inf = float("nan"), float("inf")
    # everything the single calls refuse in the descriptor, except the basis ...
    bad_views = [dict(struct_size=100), dict(model=3), dict(flags=2), dict(flags=0x80000001), dict(k=0), dict(k=3), dict(k=32), dict(width=0), dict(height=0),
                 dict(width=65536), dict(height=65536),
                 dict(model=0, half_w=0.0), dict(model=0, half_h=-1.0), dict(model=0, half_w=inf), dict(model=0, half_h=nan),
                 dict(model=2, half_angle=0.0), dict(model=2, half_angle=-0.5), dict(model=2, half_angle=3.1415930), dict(model=2, half_angle=nan), dict(model=2, half_angle=inf),
                 dict(t_min=-1.0), dict(t_min=nan), dict(t_min=inf), dict(t_max=nan), dict(t_max=0.0), dict(t_min=2.0, t_max=2.0), dict(t_min=2.0, t_max=1.0),
                 # ... whole frames only, and the ray limit of the whole batch
                 dict(row0=1), dict(row0=H), dict(nrows=3), dict(nrows=H + 1), dict(row0=1, nrows=H - 1), dict(width=65535, height=65535, k=1)]
    not_a_handle = C.create_string_buffer(64)
    fake = C.c_void_p(C.addressof(not_a_handle))
    try:
        for fields in bad_views:
            refused(E_ARG, vd=vd(**fields))
            refused_rays(E_ARG, vd=vd(**fields))
        refused(E_ARG, vd=None)
        refused_rays(E_ARG, vd=None)
        refused(E_ARG, desc=None)
        refused(E_ARG, desc=changed(struct_size=desc.struct_size - 4))
        # the cameras: NULL with frames, a non-finite component (the message names the frame)
        refused(E_ARG, cams=None)
        refused_rays(E_ARG, cams=None)
        for frame, slot, val in ((0, 0, nan), (1, 4, inf), (2, 11, -inf), (2, 8, nan)):
            bad = good.copy()
            bad[frame, slot] = val
            refused(E_ARG, cams=bad)
            assert f"frame {frame}" in ctx.last_error(), ctx.last_error()
            refused_rays(E_ARG, cams=bad)
            assert f"frame {frame}" in ctx.last_error(), ctx.last_error()
        # too many rays in all: 16 x 16 x 1 = 256 rays a frame, 2^24 frames (the table is not read: the count is refused first)
        refused(E_ARG, vd=vd(width=16, height=16, k=1), nf=1 << 24)
        refused_rays(E_ARG, vd=vd(width=16, height=16, k=1), nf=1 << 24)
        for tone in (0.0, -1.0, nan, inf):
            refused(E_ARG, vd=vd(tone=tone))
        refused(E_ARG, seeds=None)
        refused(E_ARG, radiance=None, pixel=None)
        refused(E_ARG, vd=vd(flags=V.ACCUMULATE), radiance=None)
        refused(E_ARG, desc=changed(n_lights=9))                # MIRT_MAX_LIGHTS is 8
        refused(E_ARG, desc=changed(n_meshes=17))               # MIRT_MAX_MESHES is 16
        refused(E_ARG, desc=changed(lights=None))
        refused(E_ARG, desc=changed(n_meshes=1, meshes=None))
        # MIRT_E_RANGE: a buffer shorter than N frames (each holds N - 1 and more), a material table shorter than one entry
        refused(E_RANGE, seeds=short_seeds)
        refused(E_RANGE, radiance=short_rad)
        refused(E_RANGE, pixel=short_pix)
        refused(E_RANGE, vd=vd(k=4))                            # the buffers hold k = 2
        refused(E_RANGE, cams=VB.cameras(sc, N + 1), nf=N + 1)
        refused_rays(E_RANGE, rays=short_rays)
        refused_rays(E_RANGE, cams=VB.cameras(sc, N + 1), nf=N + 1)
        small = ctx.wrap(r.dev.material.device_ptr, 8)
        extra.append(small)
        refused(E_RANGE, desc=changed(material=small.h))
        # MIRT_E_HANDLE: a bad context or buffer
        refused(E_HANDLE, c=fake)
        refused_rays(E_HANDLE, c=fake)
        refused(E_HANDLE, seeds=fake)
        refused(E_HANDLE, radiance=fake)
        refused(E_HANDLE, pixel=fake)
        refused(E_HANDLE, desc=changed(material=None))
        refused_rays(E_HANDLE, rays=fake)
        refused_rays(E_HANDLE, rays=None)
        # aliasing, on the whole batch buffers: a pixel buffer inside the LAST frame's seeds meets them
        refused(E_ARG, seeds=r.radiance)
        refused(E_ARG, pixel=r.radiance)
        refused(E_ARG, radiance=r.seeds, pixel=None)
        view_in = ctx.wrap(r.seeds.device_ptr + (n * 4 - npx * 4) // 16 * 16, npx * 4)
        extra.append(view_in)
        refused(E_ARG, pixel=view_in)
        big = ctx.buffer(max(npx * 16, r.dev.material.nbytes))
        extra.append(big)
        fill()
        big.write(np.full(big.nbytes, V.SENTINEL, np.uint8))
        assert call(desc=changed(material=big.h), radiance=big) == E_ARG, ctx.last_error()
        clean("radiance is the material")
        assert (big.read(np.uint8) == V.SENTINEL).all()
        prims = r.dev.tri["prims"] if r.dev.tri else r.dev.sph["prims"]
        if prims.nbytes >= npx * 4:
            geo = ctx.wrap(prims.device_ptr, npx * 4)
            extra.append(geo)
            before = prims.read(np.uint8).tobytes()
            fill()
            assert call(pixel=geo) == E_ARG, ctx.last_error()
            clean("pixel is geometry")
            assert prims.read(np.uint8).tobytes() == before
        # MIRT_E_DATA: a cell table that fails validation -- the loose triangles' offsets decrease
        off = r.dev.tri["off"]
        good_off = off.read(np.uint32)
        off.write(np.array([good_off[-1], 0], np.uint32))
        try:
            refused(E_DATA)
        finally:
            off.write(good_off)
        # while capturing
        fill()
        ctx.finish()
        ctx.capture_begin()
        try:
            assert call() == E_ARG and "capture" in ctx.last_error()
            assert call_rays() == E_ARG and "capture" in ctx.last_error()
        finally:
            ctx.graph_release(ctx.capture_end())
        clean("inside a recording")
        # no frames: MIRT_OK, nothing queued, nothing written -- with and without a table
        fill()
        assert call(nf=0) == 0 and call(nf=0, cams=None) == 0 and call_rays(nf=0) == 0 and call_rays(nf=0, cams=None) == 0, ctx.last_error()
        clean("no frames")
        # the descriptor's own basis is neither read nor checked; the same context renders the batch afterwards ...
        seeds = A.make_seeds(n)
        want = r.singles(view, good, seeds, bounces=BOUNCES)
        r.seeds.write(seeds)
        assert call(vd=vd(eye=(nan, 0.0, 0.0), right=(0.0, inf, 0.0), up=(0.0, 0.0, -inf), forward=(nan, nan, nan))) == 0, ctx.last_error()
        got = (r.seeds.read(np.int32), r.radiance.read(np.float32).reshape(-1, 4), r.pixel.read(np.uint8).reshape(-1, 4))
        d = V.differ("after the refusals", got, want)
        assert d is None, d
        # ... and the fixture's own camera
        fseeds = A.make_seeds(sc.total_rays)
        st = A.PassState(sc, fseeds)
        A.run_pass(A.load_oracle(), sc, st)
        fr = render.FusedRenderer(ctx, sc, seeds=fseeds)
        try:
            fr.execute_render()
            assert np.array_equal(fr.pixel.read(np.uint8).reshape(-1, 4), st.pixel), "cornell_32x24_r4 after the refusals"
        finally:
            fr.release()
    finally:
        for b in extra + [short_seeds, short_rad, short_pix, short_rays, rays_buf]:
            b.release()
        r.release()
