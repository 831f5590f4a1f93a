"""GPU: panoramic, fisheye and orthographic cameras -- mirt_view_rays, mirt_render_view, mirt_view_deferred (include/mirt.h) -- through the C ABI,
tolerance 0 (conftest.bits: every NaN equal to every NaN):

  1. the rays against the numpy restatement (tests/view_common.py) for the three models at 13 x 7 with k = 1, 2, 4, 8, 16, at 1 x 1 with k = 1
     and at 65 x 1 with k = 2 -- one lane, a second wave of one pixel, 91 rays (64 + 27), ragged last blocks at 256, 64, 16, 4 and 1 pixels
     per block; sentinel bytes behind the records stay untouched;
  2. the frame against the oracle (view_common.expected_view) in seeds, radiance and pixel: both fixtures x three models at 13 x 7, k = 2,
     bounces 2, under the optimistic / exact pair and under set_exact_only(True);
  3. the frame against composition at every k: mirt_render_view equals this library's own mirt_view_rays, then mirt_trace_radiance, then the
     numpy fold and tone map (no oracle time at 23 k rays);
  4. tiles (0, 3), (3, 1), (4, 3) of the 13 x 7 frame with their slices of the seeds give the whole frame's rows;
  5. progressive: a fresh call and two with MIRT_VIEW_ACCUMULATE equal expected_view chained with `carry`, tone 1 / (4 * 3) for the third; a fresh
     call into a pre-filled radiance buffer ignores what it held;
  6. the exact route: ORTHOGRAPHIC along -z equals the oracle, mirt_view_deferred is the tile's rays rounded up to whole blocks under the pair
     and 0 under exact_only;
  7. pixel only and radiance only give what both together give; every refusal of the header's list, seeds and outputs pre-filled and compared
     afterwards; the context still renders cornell_32x24_r4 correctly after them.
"""
import ctypes as C

import numpy as np
import pytest

import a10_pass as A
import radiance_common as RC
import view_common as V
from conftest import bits, load_fixture

pytestmark = pytest.mark.gpu

E_ARG, E_HANDLE, E_RANGE, E_DATA = -1, -2, -5, -8
FIXTURES = ("cornell_32x24_r4", "cornell_teapot3_32x24_r4")
MODELS = ("ortho", "equirect", "fisheye")
W, H, BOUNCES = 13, 7, 2
CAP_RAYS, CAP_PIXELS = W * H * 256, W * H

_SCENES, _EXPECTED = {}, {}


def scene(name):
    if name not in _SCENES:
        _SCENES[name] = load_fixture(name)[1]
    return _SCENES[name]


def seeds_of(n):
    return A.make_seeds(n)


def expected(name, model):
    """the oracle's frame for the standard inputs, computed once and shared"""
    key = (name, model)
    if key not in _EXPECTED:
        v = V.standard_view(scene(name), model, tone=0.25)
        out = V.expected_view(scene(name), v, seeds_of(v.n_rays), BOUNCES)
        for a in out:
            a.setflags(write=False)
        _EXPECTED[key] = out
    return _EXPECTED[key]


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
            made[name] = V.Renderer(ctx, scene(name), CAP_RAYS, CAP_PIXELS)
        return made[name]
    yield get
    for r in made.values():
        r.release()


def check(tag, r, view, seeds, want, **kw):
    got = r.run(view, seeds, **kw)
    d = V.differ(tag, got, want)
    assert d is None, d
    assert got[3], f"{tag}: bytes behind the records, or a buffer that was not given, were written"
    return got


# ---- 1. the rays ---------------------------------------------------------------------------------------------------------------------------------
SIZES = [(W, H, k) for k in V.KS] + [(1, 1, 1), (65, 1, 2)]


@pytest.mark.parametrize("width,height,k", SIZES)
@pytest.mark.parametrize("model", MODELS)
def test_view_rays_equal_the_restatement(ctx, model, width, height, k):
    v = V.standard_view(scene(FIXTURES[0]), model, width=width, height=height, k=k, t_min=0.03125, t_max=1000.0)
    n, tail = v.n_rays, 96
    buf = ctx.buffer(n * 32 + tail)
    try:
        buf.write(np.full(buf.nbytes, V.SENTINEL, np.uint8))
        ctx.view_rays(v.desc(), buf)
        raw = buf.read(np.uint8)
        got, want = raw[:n * 32].view(np.float32).reshape(-1, 8), V.view_rays(v)
        bad = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
        assert bad.size == 0, f"{model} {width}x{height} k={k}: {bad.size} of {n} rays differ; first is ray {int(bad[0])}: got {got[bad[0]].tolist()}, want {want[bad[0]].tolist()}"
        assert (raw[n * 32:] == V.SENTINEL).all(), "bytes behind the records were written"
    finally:
        buf.release()


# ---- 2. the frame against the oracle ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact_only", [False, True], ids=["pair", "exact_only"])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", FIXTURES)
def test_the_frame_equals_the_oracle(ctx, renderers, name, model, exact_only):
    v = V.standard_view(scene(name), model, tone=0.25)
    ctx.set_exact_only(exact_only)
    try:
        check(f"{name} {model} exact_only={exact_only}", renderers(name), v, seeds_of(v.n_rays), expected(name, model), bounces=BOUNCES)
        if not exact_only:
            print(f"{name} {model}: deferred {ctx.view_deferred()} of {v.n_rays} rays")
    finally:
        ctx.set_exact_only(False)


# ---- 3. the frame against composition, at every k --------------------------------------------------------------------------------------------------
def composition(ctx, r, v, seeds, bounces):
    """this library's own three steps: mirt_view_rays, mirt_trace_radiance at one sample, then the fold and the tone map in numpy"""
    n = v.n_rays
    rays, sd, acc = ctx.buffer(n * 32), ctx.buffer(n * 4), ctx.buffer(n * 16)
    try:
        sd.write(np.ascontiguousarray(seeds, np.int32))
        ctx.view_rays(v.desc(), rays)
        ctx.trace_radiance(r.scene_desc(bounces), rays, n, sd, acc, samples=1, flags=0)
        sums = V.fold(acc.read(np.float32).reshape(-1, 4), v.rpp)
        return sd.read(np.int32), sums, V.tone_rgba8(sums, v.tone)
    finally:
        for b in (rays, sd, acc):
            b.release()


@pytest.mark.parametrize("k", V.KS)
def test_the_frame_equals_rays_then_radiance_then_the_fold(ctx, renderers, k):
    name = FIXTURES[0]
    v = V.standard_view(scene(name), "equirect", k=k, tone=1.0 / (k * k))
    seeds = seeds_of(v.n_rays)
    r = renderers(name)
    want = composition(ctx, r, v, seeds, BOUNCES)
    assert (want[1][:, 3] > 0).any(), "no pixel received light"
    check(f"{name} equirect k={k}", r, v, seeds, want, bounces=BOUNCES)


# ---- 4. tiles ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", FIXTURES)
def test_tiles_give_the_frames_rows(renderers, name, model):
    v = V.standard_view(scene(name), model, tone=0.25)
    sd, sums, px = expected(name, model)
    seeds = seeds_of(v.n_rays)
    per_row = W * v.rpp
    for row0, nrows in ((0, 3), (3, 1), (4, 3)):
        rays, pix = slice(row0 * per_row, (row0 + nrows) * per_row), slice(row0 * W, (row0 + nrows) * W)
        check(f"{name} {model} rows [{row0}, +{nrows})", renderers(name), v.tile(row0, nrows), seeds[rays], (sd[rays], sums[pix], px[pix]), bounces=BOUNCES)


# ---- 5. progressive ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", FIXTURES)
def test_progressive_frames_continue_the_chain(renderers, name, model):
    sc, r = scene(name), renderers(name)
    seeds, carry = None, None
    for p in (1, 2, 3):
        v = V.standard_view(sc, model, tone=1.0 / (4 * p))
        seeds = seeds_of(v.n_rays) if seeds is None else seeds
        want = V.expected_view(sc, v, seeds, BOUNCES, carry=carry)
        got = check(f"{name} {model} frame {p}", r, v, seeds, want, bounces=BOUNCES, carry=carry)
        seeds, carry = got[0], got[1]
    assert (carry[:, 3] > 0).any()
    # a fresh call into a pre-filled radiance buffer ignores what it held
    v = V.standard_view(sc, model, tone=0.25)
    pre = np.random.default_rng(11).uniform(0.0, 4.0, size=(v.n_pixels, 4)).astype(np.float32)
    check(f"{name} {model} fresh over a pre-filled buffer", r, v, seeds_of(v.n_rays), expected(name, model), bounces=BOUNCES, prefill=pre)


# ---- 6. the exact route -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_an_axis_parallel_orthographic_camera_runs_in_the_exact_kernel(ctx, renderers, name):
    sc, r = scene(name), renderers(name)
    std = V.standard_view(sc, "ortho", tone=0.25)
    v = V.View("ortho", W, H, 2, std.eye, (1, 0, 0), (0, 1, 0), (0, 0, -1), half_w=std.half_w, half_h=std.half_h, tone=0.25)
    seeds = seeds_of(v.n_rays)
    want = V.expected_view(sc, v, seeds, BOUNCES)
    assert (want[1][:, 3] > 0).any(), "no pixel received light"
    check(f"{name} axis-parallel, pair", r, v, seeds, want, bounces=BOUNCES)
    assert ctx.view_deferred() == -(-v.n_rays // 256) * 256, "every block of the frame is the exact kernel's"
    ctx.set_exact_only(True)
    try:
        check(f"{name} axis-parallel, exact_only", r, v, seeds, want, bounces=BOUNCES)
        assert ctx.view_deferred() == 0, "the exact kernel alone defers nothing"
    finally:
        ctx.set_exact_only(False)


# ---- 7. outputs and refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_one_output_alone_is_what_both_give(renderers, model):
    name = FIXTURES[1]
    v = V.standard_view(scene(name), model, tone=0.25)
    sd, sums, px = expected(name, model)
    seeds = seeds_of(v.n_rays)
    check(f"{model} pixel only", renderers(name), v, seeds, (sd, None, px), bounces=BOUNCES, radiance=False)
    check(f"{model} radiance only", renderers(name), v.with_(tone=float("nan")), seeds, (sd, sums, None), bounces=BOUNCES, pixel=False)


def test_refusals_write_nothing_and_leave_the_context_working(ctx, pkg):
    from raytracing_amd.pyhost import mirt, render
    L = mirt.lib()
    name = FIXTURES[0]
    sc = scene(name)
    view = V.standard_view(sc, "equirect", tone=0.25)
    n, npx = view.n_rays, view.n_pixels
    r = V.Renderer(ctx, sc, n, npx, tail=0)
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

    def call(c=None, desc=desc, vd=vd(), seeds=r.seeds, radiance=r.radiance, pixel=r.pixel):
        return L.mirt_render_view(c or ctx.h, C.byref(desc) if desc is not None else None, C.byref(vd) if vd is not None else None, h(seeds), h(radiance), h(pixel))

    def call_rays(c=None, vd=vd(), rays=rays_buf):
        return L.mirt_view_rays(c or ctx.h, C.byref(vd) if vd is not None else None, h(rays))

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
    bad_views = [dict(struct_size=100), dict(model=3), dict(flags=2), dict(flags=0x80000001), dict(k=0), dict(k=3), dict(k=32), dict(width=0), dict(height=0),
                 dict(width=65536), dict(height=65536), dict(row0=H), dict(row0=5, nrows=3), dict(nrows=H + 1), dict(width=65535, height=65535),
                 dict(eye=(nan, 0.0, 0.0)), dict(right=(0.0, inf, 0.0)), dict(up=(0.0, 0.0, -inf)), dict(forward=(nan, nan, nan)),
                 dict(model=0, half_w=0.0), dict(model=0, half_h=-1.0), dict(model=0, half_w=inf), dict(model=0, half_h=nan),
                 dict(model=2, half_angle=0.0), dict(model=2, half_angle=-0.5), dict(model=2, half_angle=3.1415930), dict(model=2, half_angle=nan), dict(model=2, half_angle=inf),
                 dict(t_min=-1.0), dict(t_min=nan), dict(t_min=inf), dict(t_max=nan), dict(t_max=0.0), dict(t_min=2.0, t_max=2.0), dict(t_min=2.0, t_max=1.0)]
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
        for tone in (0.0, -1.0, nan, inf):
            refused(E_ARG, vd=vd(tone=tone))
        refused(E_ARG, seeds=None)
        refused(E_ARG, radiance=None, pixel=None)
        refused(E_ARG, vd=vd(flags=V.ACCUMULATE), radiance=None)
        refused(E_ARG, desc=changed(n_lights=9))                # MIRT_MAX_LIGHTS is 8
        refused(E_ARG, desc=changed(n_meshes=17))               # MIRT_MAX_MESHES is 16
        refused(E_ARG, desc=changed(lights=None))
        refused(E_ARG, desc=changed(n_meshes=1, meshes=None))
        # MIRT_E_RANGE: a buffer shorter than the tile's rays or pixels, a material table shorter than one entry
        refused(E_RANGE, seeds=short_seeds)
        refused(E_RANGE, radiance=short_rad)
        refused(E_RANGE, pixel=short_pix)
        refused(E_RANGE, vd=vd(k=4))                            # the buffers hold k = 2
        refused_rays(E_RANGE, rays=short_rays)
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
        # aliasing: all three are written -- none may meet another, a geometry buffer or the material
        refused(E_ARG, seeds=r.radiance)
        refused(E_ARG, pixel=r.radiance)
        refused(E_ARG, radiance=r.seeds, pixel=None)
        view_in = ctx.wrap(r.seeds.device_ptr + (n * 4 - npx * 4) // 16 * 16, npx * 4)      # a pixel buffer's worth of bytes near the end of the seeds
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
        good = off.read(np.uint32)
        off.write(np.array([good[-1], 0], np.uint32))
        try:
            refused(E_DATA)
        finally:
            off.write(good)
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
        # the same context renders the same view afterwards ...
        got = r.run(view, seeds_of(n), bounces=BOUNCES)
        d = V.differ("after the refusals", got, expected(name, "equirect"))
        assert d is None, d
        # ... and the fixture's own camera
        fsc = sc
        fseeds = A.make_seeds(fsc.total_rays)
        st = A.PassState(fsc, fseeds)
        A.run_pass(A.load_oracle(), fsc, st)
        fr = render.FusedRenderer(ctx, fsc, seeds=fseeds)
        try:
            fr.execute_render()
            assert np.array_equal(fr.pixel.read(np.uint8).reshape(-1, 4), st.pixel), "cornell_32x24_r4 after the refusals"
        finally:
            fr.release()
    finally:
        for b in extra + [short_seeds, short_rad, short_pix, short_rays, rays_buf]:
            b.release()
        r.release()
