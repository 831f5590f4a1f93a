"""GPU: first-hit guides of the view cameras -- mirt_view_guides, mirt_render_view_guided, mirt_ctx_guided_views (include/mirt.h) -- through the
C ABI, tolerance 0 (guides_common.difference / conftest.bits: every NaN equal to every NaN):

  1. against the oracle (view_guides_common.expected): both fixtures x three models at 13 x 7, k = 2, under the optimistic / exact pair and under
     set_exact_only(True); rim_17x40_pi, clipped_ortho, on_face and oblique_fisheye of the camera catalogue (37 x 21 = 777 pixels: four blocks,
     the last of 9 lanes);
  2. against composition -- this library's mirt_view_rays + mirt_trace_closest + numpy reduce_guides -- at every k at 13 x 7, at 1 x 1 with
     k = 1 and 65 x 1 with k = 2; sentinel bytes behind the records untouched, each output alone what both together give;
  3. tiles (0, 3), (3, 1), (4, 3) of the 13 x 7 frame equal the frame's rows;
  4. the exact route: ORTHOGRAPHIC along -z, all_refused and the mixed_k2 / k4 / k16 cameras under the pair equal the oracle;
  5. a material buffer cut short: samples with an id past it are not hits;
  6. mirt_render_view_guided equals mirt_render_view then mirt_view_guides in seeds, radiance, pixel and both guides at every k on both
     fixtures, fresh and with ACCUMULATE, under the pair, under exact_only and on the mixed_* cameras; mirt_ctx_guided_views goes up by one
     exactly where the route rule says, never at k = 16; MIRT_GUIDED_VIEW=0 (a child process): same bytes, counter unchanged;
  7. every refusal of both calls, all buffers pre-filled and compared afterwards; the context renders cornell_32x24_r4 correctly after them.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import a10_pass as A
import rays_common as R
import view_cameras_common as VC
import view_common as V
import view_guides_common as VG
from conftest import ROOT, load_fixture

pytestmark = pytest.mark.gpu

E_ARG, E_HANDLE, E_RANGE, E_DATA = -1, -2, -5, -8
MODELS = ("ortho", "equirect", "fisheye")
W, H, BOUNCES = 13, 7, 2
CAP_RAYS, CAP_PIXELS = W * H * 256, 2000   # 13 x 7 at k = 16; the 1000 x 2 tile of mixed_k2

_SCENES = {}


def scene(name):
    if name not in _SCENES:
        _SCENES[name] = load_fixture(name)[1] if name in VG.FIXTURES else R.scene(name)
    return _SCENES[name]


def expected_standard(name, model):
    return VG.cached(("standard", name, model), lambda: VG.expected(scene(name), V.standard_view(scene(name), model)))


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
            made[name] = VG.Renderer(ctx, scene(name), CAP_RAYS, CAP_PIXELS)
        return made[name]
    yield get
    for r in made.values():
        r.release()


def check(tag, r, view, want, **kw):
    got = r.guides(view, **kw)
    d = VG.differ(tag, got, want)
    assert d is None, d
    assert got[2], f"{tag}: bytes behind the records, or a buffer that was not given, were written"
    return got


# ---- 1. against the oracle ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact_only", [False, True], ids=["pair", "exact_only"])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", VG.FIXTURES)
def test_the_guides_equal_the_oracle(ctx, renderers, name, model, exact_only):
    v = V.standard_view(scene(name), model)
    ctx.set_exact_only(exact_only)
    try:
        got = check(f"{name} {model} exact_only={exact_only}", renderers(name), v, expected_standard(name, model))
        print(f"{name} {model}: (no hit, every sample, partly) = {VG.kinds(got[0], v.rpp)}")
    finally:
        ctx.set_exact_only(False)


@pytest.mark.parametrize("stratum,camera", VG.CATALOGUE)
def test_catalogue_cameras_equal_the_oracle(renderers, stratum, camera):
    v = VC.view(stratum, camera)
    got = check(f"{stratum} {camera}", renderers(stratum), v, VG.expected_catalogue(stratum, camera))
    assert (got[0][:, 3] > 0).any() and (got[0][:, 3] == 0).any()


# ---- 2. against composition -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,height,k", VG.SIZES)
@pytest.mark.parametrize("model", ("equirect", "fisheye"))
def test_the_guides_equal_rays_then_closest_then_the_reduction(ctx, renderers, model, width, height, k):
    name = VG.FIXTURES[1]
    v = V.standard_view(scene(name), model, width=width, height=height, k=k)
    d, want = VG.composition_difference(ctx, renderers(name), scene(name), v, f"{name} {model} {width}x{height} k={k}")
    assert d is None, d
    assert (want[0][:, 3] > 0).any(), "no pixel was hit"


# ---- 3. tiles ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", VG.FIXTURES)
def test_tiles_give_the_frames_rows(renderers, name, model):
    v = V.standard_view(scene(name), model)
    nh, ad = expected_standard(name, model)
    for row0, nrows in ((0, 3), (3, 1), (4, 3)):
        pix = slice(row0 * W, (row0 + nrows) * W)
        check(f"{name} {model} rows [{row0}, +{nrows})", renderers(name), v.tile(row0, nrows), (nh[pix], ad[pix]))


# ---- 4. the exact route -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", VG.FIXTURES)
def test_an_axis_parallel_orthographic_camera_equals_the_oracle(renderers, name):
    sc = scene(name)
    std = V.standard_view(sc, "ortho")
    v = V.View("ortho", W, H, 2, std.eye, (1, 0, 0), (0, 1, 0), (0, 0, -1), half_w=std.half_w, half_h=std.half_h)
    want = VG.expected(sc, v)
    assert (want[0][:, 3] > 0).any()
    check(f"{name} axis-parallel, pair", renderers(name), v, want)


@pytest.mark.parametrize("stratum,camera", VG.EXACT)
def test_refused_and_mixed_cameras_equal_the_oracle(renderers, stratum, camera):
    v = VC.view(stratum, camera)
    got = check(f"{stratum} {camera}", renderers(stratum), v, VG.expected_catalogue(stratum, camera))
    assert (got[0][:, 3] > 0).any()


# ---- 5. a material table cut short -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", VG.FIXTURES)
def test_ids_past_a_cut_material_table_are_not_hits(ctx, renderers, name):
    sc, r = scene(name), renderers(name)
    mats = np.asarray(sc.materials, np.float32).reshape(-1, 4)
    v = V.standard_view(sc, "equirect")
    full = expected_standard(name, "equirect")
    cut = ctx.wrap(r.dev.material.device_ptr, 2 * 16)
    try:
        desc = r.scene_desc(0)
        desc.material = cut.h
        hits, _ = R.expected_closest(sc, V.view_rays(v))
        want = VG.reduce_hits(hits, mats[:2], v.rpp)
        assert len(mats) > 2 and (want[0][:, 3] < full[0][:, 3]).any() and (want[0][:, 3] > 0).any(), "the cut changes nothing, or everything"
        check(f"{name} two material entries", r, v, want, scene_desc=desc)
    finally:
        cut.release()


# ---- 6. the guided frame ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact_only", [False, True], ids=["pair", "exact_only"])
@pytest.mark.parametrize("k", V.KS)
@pytest.mark.parametrize("name", VG.FIXTURES)
def test_the_guided_frame_equals_the_two_calls(ctx, renderers, name, k, exact_only):
    sc, r = scene(name), renderers(name)
    v = V.standard_view(sc, "equirect", k=k, tone=1.0 / (k * k))
    ctx.set_exact_only(exact_only)
    try:
        tag = f"{name} k={k} exact_only={exact_only}"
        d, got = VG.guided_difference(ctx, r, v, A.make_seeds(v.n_rays), tag, BOUNCES)
        assert d is None, d
        assert (got[0][1][:, 3] > 0).any() and (got[1][0][:, 3] > 0).any(), "nothing lit, or nothing hit"
        # the second progressive frame: the sums go on, the guides are the same
        d, acc = VG.guided_difference(ctx, r, v.with_(tone=1.0 / (2 * k * k)), got[0][0], tag + " accumulate", BOUNCES, carry=got[0][1])
        assert d is None, d
        assert VG.differ(tag + ": the guides of the second frame", acc[1], got[1]) is None
        assert not np.array_equal(acc[0][1], got[0][1])
    finally:
        ctx.set_exact_only(False)


@pytest.mark.parametrize("fisheye_k", (1, 2))
def test_the_guided_frame_with_dead_samples_and_one_output(ctx, renderers, fisheye_k):
    name = VG.FIXTURES[1]
    sc, r = scene(name), renderers(name)
    v = V.standard_view(sc, "fisheye", k=fisheye_k, tone=1.0 / (fisheye_k * fisheye_k))
    seeds = A.make_seeds(v.n_rays)
    d, got = VG.guided_difference(ctx, r, v, seeds, f"{name} fisheye k={fisheye_k}", BOUNCES)
    assert d is None, d
    # one guide alone, and no radiance: the others are what the full call gave
    r._load(v, seeds, None)
    ctx.render_view_guided(r.scene_desc(BOUNCES), v.desc(), r.seeds, None, r.pixel, None, r.ad)
    frame, guides = r._frame(v), r._read_guides(v.n_pixels, False, True)
    assert np.array_equal(frame[0], got[0][0]) and np.array_equal(frame[2], got[0][2]) and VG.differ("albedo_depth alone", guides, (None, got[1][1])) is None
    assert guides[2] and (r.radiance.read(np.uint8) == V.SENTINEL).all()


@pytest.mark.parametrize("stratum,camera", [e for e in VG.EXACT if e[1].startswith("mixed_")])
def test_the_guided_frame_on_cameras_whose_blocks_defer(ctx, renderers, stratum, camera):
    v = VC.view(stratum, camera)
    d, _ = VG.guided_difference(ctx, renderers(stratum), v, VC.seeds_of(v.n_rays), f"{stratum} {camera}", VC.BOUNCES)
    assert d is None, d
    deferred = ctx.view_deferred()
    assert 0 < deferred < VC.n_blocks(v) * 256, f"{camera}: {deferred} rays deferred -- the exact kernel's rewrite of a block's guides is not exercised beside blocks that stay"


def test_the_switch_forces_the_two_launches():
    env = dict(os.environ, MIRT_GUIDED_VIEW="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "view_guides_child.py"), "switch_off"], env=env, capture_output=True, text=True, timeout=600)
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0, (lines[-1:] or r.stderr[-2000:])
    assert len(lines) == len(V.KS) and all(l["ok"] and l["hit_pixels"] > 0 for l in lines), lines


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_leave_the_context_working(ctx, pkg):
    from raytracing_amd.pyhost import mirt, render
    L = mirt.lib()
    name = VG.FIXTURES[0]
    sc = scene(name)
    view = V.standard_view(sc, "equirect", tone=0.25)
    n, npx = view.n_rays, view.n_pixels
    r = VG.Renderer(ctx, sc, n, npx, tail=0)
    desc = r.scene_desc(BOUNCES)
    short_nh, short_ad = ctx.buffer(npx * 16 - 1), ctx.buffer(npx * 16 - 1)
    outputs = (r.seeds, r.radiance, r.pixel, r.nh, r.ad, short_nh, short_ad)
    extra = []

    def h(b):
        return b.h if isinstance(b, mirt.Buffer) else b

    def vd(flags=0, **fields):
        d = view.desc(flags)
        for k, val in fields.items():
            setattr(d, k, (C.c_float * 3)(*val) if isinstance(val, tuple) else val)
        return d

    def ref(x):
        return C.byref(x) if x is not None else None

    def call_guides(c=None, desc=desc, vd=vd(), nh=r.nh, ad=r.ad, **_frame_only):
        return L.mirt_view_guides(c or ctx.h, ref(desc), ref(vd), h(nh), h(ad))

    def call_guided(c=None, desc=desc, vd=vd(), seeds=r.seeds, radiance=r.radiance, pixel=r.pixel, nh=r.nh, ad=r.ad):
        return L.mirt_render_view_guided(c or ctx.h, ref(desc), ref(vd), h(seeds), h(radiance), h(pixel), h(nh), h(ad))

    def fill():
        for b in outputs:
            b.write(np.full(b.nbytes, V.SENTINEL, np.uint8))

    def clean(what):
        for b in outputs:
            assert (b.read(np.uint8) == V.SENTINEL).all(), f"{what}: a buffer was written"

    def refused(code, calls=(call_guides, call_guided), **over):
        for call in calls:
            fill()
            assert call(**over) == code, (call.__name__, list(over), ctx.last_error())
            clean((call.__name__, list(over)))

    def changed(**fields):
        d = r.scene_desc(BOUNCES)
        for k, val in fields.items():
            setattr(d, k, val)
        return d

    nan, inf = float("nan"), float("inf")
    bad_views = [dict(struct_size=100), dict(model=3), dict(flags=2), dict(flags=0x80000001), dict(k=0), dict(k=3), dict(k=32), dict(width=0), dict(height=0),
                 dict(width=65536), dict(height=65536), dict(row0=H), dict(row0=5, nrows=3), dict(nrows=H + 1), dict(width=65535, height=65535),
                 dict(eye=(nan, 0.0, 0.0)), dict(right=(0.0, inf, 0.0)), dict(up=(0.0, 0.0, -inf)), dict(forward=(nan, nan, nan)),
                 dict(model=0, half_w=0.0), dict(model=0, half_h=nan), dict(model=2, half_angle=0.0), dict(model=2, half_angle=3.1415930), dict(model=2, half_angle=nan),
                 dict(t_min=-1.0), dict(t_min=nan), dict(t_max=nan), dict(t_max=0.0), dict(t_min=2.0, t_max=2.0)]
    not_a_handle = C.create_string_buffer(64)
    fake = C.c_void_p(C.addressof(not_a_handle))
    try:
        # MIRT_E_ARG: the descriptor checks of mirt_view_rays, both descriptors' sizes, both outputs NULL, the mesh count rule
        for fields in bad_views:
            refused(E_ARG, vd=vd(**fields))
        refused(E_ARG, vd=None)
        refused(E_ARG, desc=None)
        refused(E_ARG, desc=changed(struct_size=desc.struct_size - 4))
        refused(E_ARG, nh=None, ad=None)
        refused(E_ARG, desc=changed(n_meshes=17))               # MIRT_MAX_MESHES is 16
        refused(E_ARG, desc=changed(n_meshes=1, meshes=None))
        # ... and the frame's own on top, for the guided call alone: the guides read neither tone, the lights nor the frame's buffers
        guided = (call_guided,)
        for tone in (0.0, nan):
            refused(E_ARG, guided, vd=vd(tone=tone))
        refused(E_ARG, guided, seeds=None)
        refused(E_ARG, guided, radiance=None, pixel=None)
        refused(E_ARG, guided, vd=vd(flags=V.ACCUMULATE), radiance=None)
        refused(E_ARG, guided, desc=changed(n_lights=9))
        refused(E_ARG, guided, desc=changed(lights=None))
        # MIRT_E_RANGE: an output shorter than the tile's pixels x 16 B, a material table shorter than one entry
        refused(E_RANGE, nh=short_nh)
        refused(E_RANGE, ad=short_ad)
        refused(E_RANGE, nh=short_nh, ad=None)
        small = ctx.wrap(r.dev.material.device_ptr, 8)
        extra.append(small)
        refused(E_RANGE, desc=changed(material=small.h))
        refused(E_RANGE, desc=changed(material=small.h), ad=None)   # needed even when only normal_hits is asked for
        # MIRT_E_HANDLE: a bad context or buffer
        refused(E_HANDLE, c=fake)
        refused(E_HANDLE, nh=fake)
        refused(E_HANDLE, ad=fake)
        refused(E_HANDLE, desc=changed(material=None))
        # aliasing: an output meets the other, a geometry buffer or the material; for the guided call, seeds, radiance or pixel as well
        refused(E_ARG, ad=r.nh)
        last = ctx.wrap(r.nh.device_ptr + 38 * 16, 39 * 16)   # a tile of 3 rows is 39 pixels: these bytes begin with its last pixel's
        extra.append(last)
        refused(E_ARG, nh=r.nh, ad=last, vd=vd(nrows=3))
        refused(E_ARG, guided, nh=r.radiance, radiance=r.radiance)
        refused(E_ARG, guided, ad=r.radiance)
        # (mirt_render_view, which has no guides, keeps its own words for the same refusals)
        assert L.mirt_render_view(ctx.h, ref(desc), ref(vd()), h(r.radiance), h(r.radiance), h(r.pixel)) == E_ARG and "guide" not in ctx.last_error()
        assert call_guided(ad=r.radiance) == E_ARG and "guides" in ctx.last_error()
        big_seeds = ctx.wrap(r.seeds.device_ptr, npx * 16)
        extra.append(big_seeds)
        refused(E_ARG, guided, nh=big_seeds)
        pix_tile = ctx.wrap(r.pixel.device_ptr, 16)
        extra.append(pix_tile)
        refused(E_ARG, guided, vd=vd(width=1, height=1, k=1), ad=pix_tile)
        big = ctx.buffer(max(npx * 16, r.dev.material.nbytes))
        extra.append(big)
        for call in (call_guides, call_guided):
            fill()
            big.write(np.full(big.nbytes, V.SENTINEL, np.uint8))
            assert call(desc=changed(material=big.h), nh=big) == E_ARG, ctx.last_error()
            clean("normal_hits is the material")
            assert (big.read(np.uint8) == V.SENTINEL).all()
        prims = r.dev.tri["prims"] if r.dev.tri else r.dev.sph["prims"]
        assert prims.nbytes >= W * 16
        geo = ctx.wrap(prims.device_ptr, W * 16)
        extra.append(geo)
        before = prims.read(np.uint8).tobytes()
        refused(E_ARG, ad=geo, vd=vd(nrows=1))
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
            assert call_guides() == E_ARG and "capture" in ctx.last_error()
            assert call_guided() == E_ARG and "capture" in ctx.last_error()
        finally:
            ctx.graph_release(ctx.capture_end())
        clean("inside a recording")
        assert L.mirt_ctx_guided_views(ctx.h, None) == E_ARG and L.mirt_ctx_guided_views(fake, C.byref(C.c_uint64())) == E_HANDLE
        # the same context gives the same view's guides afterwards ...
        got = r.guides(view)
        d = VG.differ("after the refusals", got, expected_standard(name, "equirect"))
        assert d is None, d
        d, _ = VG.guided_difference(ctx, r, view, A.make_seeds(n), "after the refusals, guided", BOUNCES)
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
        for b in extra + [short_nh, short_ad]:
            b.release()
        r.release()
