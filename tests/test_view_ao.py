"""GPU: mirt_view_ao -- ambient occlusion of the view cameras, {open, cast} per pixel in one launch (include/mirt.h) -- through the C ABI,
tolerance 0 (integers), against the restatement of tests/view_ao_common.py.  3 AO rays and bias 0.001 unless said otherwise.

  1. against the oracle, fixtures: both fixtures x three models at 13 x 7, k = 2, radius 1.0, under the optimistic / exact pair and under
     set_exact_only(True); one model each with radius inf and with bias 0; the 64 sentinel bytes behind ao_out untouched;
  2. against the oracle, strata: every stratum of random_scenes_common.STRATA x the models at 37 x 21, k = 2 (777 pixels: four blocks, the last of
     9 lanes; together the three GRIDS variants of k_viewAo), the four catalogue cameras, the exact-route cameras all_refused and mixed_k2 / k4 /
     k16; mirt_view_ao_deferred is the pixel count on all_refused and strictly between 0 and it on a mixed camera;
  3. against composition on the device: mirt_view_rays + mirt_trace_closest, the AO rays rebuilt in numpy from the hits (the hemisphere rays
     from the oracle's bouncePaths on those hits), mirt_trace_occluded -- at every k at 13 x 7 (5 x 3 at k = 16), 1 x 1 with k = 1, 65 x 1 with k = 2;
  4. tiles (0, 3), (3, 1), (4, 3) of the 13 x 7 frame equal the frame's rows, their seeds filled from the global first id;
  5. properties: repeatability, the seeds byte-identical afterwards, cast / samples is mirt_view_guides' hit count where the material table covers
     every id, and with the table cut short AO still casts where the guides count no hit;
  6. every refusal, all buffers pre-filled and compared afterwards; the context renders cornell_32x24_r4 correctly after them.

Every case asserts first, on the oracle's result alone, that it is not vacuous (view_ao_common.not_vacuous; tests/test_view_ao_expectation.py
checks the same on a machine without a GPU)."""
import ctypes as C

import numpy as np
import pytest

import a10_pass as A
import random_scenes_common as S
import rays_common as R
import view_ao_common as VA
import view_cameras_common as VC
import view_common as V

pytestmark = pytest.mark.gpu

E_ARG, E_HANDLE, E_RANGE, E_DATA = -1, -2, -5, -8
W, H = 13, 7
CAP_RAYS, CAP_PIXELS = 16384, 2000   # rim_17x40_pi at k = 4 is 10880 rays; the 1000 x 2 tile of mixed_k2


@pytest.fixture(scope="module")
def ctx(pkg):
    from raytracing_amd.pyhost import mirt
    c = mirt.Context(0)
    yield c
    c.destroy()


@pytest.fixture(scope="module")
def aos(ctx):
    made = {}

    def get(name):
        if name not in made:
            made[name] = VA.Ao(ctx, VA.scene(name), CAP_RAYS, CAP_PIXELS)
        return made[name]
    yield get
    for a in made.values():
        a.release()


def check(tag, ao, v, want, **kw):
    got, clean = ao.run(v, **kw)
    d = VA.difference(tag, got, want)
    assert d is None, d
    assert clean, f"{tag}: the bytes behind ao_out, or the seeds, were written"
    return got


def vacuity(tag, want, rpp, need_empty=False):
    d = VA.not_vacuous(tag, want, VA.SAMPLES, rpp, need_empty)
    assert d is None, d


# ---- 1. against the oracle, fixtures ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact_only", [False, True], ids=["pair", "exact_only"])
@pytest.mark.parametrize("model", VA.MODELS)
@pytest.mark.parametrize("name", VA.FIXTURES)
def test_fixtures_equal_the_oracle(ctx, aos, name, model, exact_only):
    want = VA.expected_standard(name, model)
    tag = f"{name} {model} exact_only={exact_only}"
    vacuity(tag, want, 4, need_empty=VA.FIXTURE_EMPTY[(name, model)] > 0)
    ctx.set_exact_only(exact_only)
    try:
        check(tag, aos(name), V.standard_view(VA.scene(name), model), want)
        if exact_only:
            assert ctx.view_ao_deferred() == 0
    finally:
        ctx.set_exact_only(False)


@pytest.mark.parametrize("name,model,radius,bias", VA.FIXTURE_VARIANTS)
def test_an_infinite_radius_and_no_bias_equal_the_oracle(aos, name, model, radius, bias):
    """radius = inf: the AO ray is bouncePaths' own; bias = 0: its origin is Poi.p bit for bit, ON the surface it leaves"""
    want = VA.expected_standard(name, model, radius, bias)
    tag = f"{name} {model} radius {radius} bias {bias}"
    vacuity(tag, want, 4)
    check(tag, aos(name), V.standard_view(VA.scene(name), model), want, radius=radius, bias=bias)


# ---- 2. against the oracle, strata -----------------------------------------------------------------------------------------------------------------
def test_the_strata_cases_cover_every_stratum():
    assert {s for s, _m in VA.STRATA_CASES} == set(S.STRATA) and len(VA.STRATA_CASES) == 3 * len(S.STRATA) - 1


@pytest.mark.parametrize("stratum,model", VA.STRATA_CASES)
def test_strata_equal_the_oracle(ctx, aos, stratum, model):
    sc = R.scene(stratum)
    v = V.standard_view(sc, model, width=37, height=21, k=2)
    want = VA.expected_standard(stratum, model, VA.RADIUS[stratum], VA.BIAS, 37, 21, 2)
    tag = f"{stratum} {model} 37x21 k=2"
    vacuity(tag, want, 4, need_empty=(stratum, model) == ("open", "ortho"))
    check(tag, aos(stratum), v, want, radius=VA.RADIUS[stratum])
    ctx.set_exact_only(True)
    try:
        check(tag + ", exact kernel only", aos(stratum), v, want, radius=VA.RADIUS[stratum])
    finally:
        ctx.set_exact_only(False)


@pytest.mark.parametrize("stratum,camera", VA.CATALOGUE)
def test_catalogue_cameras_equal_the_oracle(aos, stratum, camera):
    v = VC.view(stratum, camera)
    want = VA.expected_catalogue(stratum, camera)
    vacuity(f"{stratum} {camera}", want, v.rpp, need_empty=True)
    check(f"{stratum} {camera}", aos(stratum), v, want)


@pytest.mark.parametrize("stratum,camera", VA.EXACT)
def test_refused_and_mixed_cameras_equal_the_oracle_and_are_counted(ctx, aos, stratum, camera):
    v = VC.view(stratum, camera)
    want = VA.expected_catalogue(stratum, camera)
    vacuity(f"{stratum} {camera}", want, v.rpp)
    check(f"{stratum} {camera}", aos(stratum), v, want)
    deferred = ctx.view_ao_deferred()
    print(f"{camera}: mirt_view_ao_deferred {deferred} of {v.n_pixels} pixels")
    if camera == "all_refused":
        assert deferred == v.n_pixels
    else:
        assert 0 < deferred < v.n_pixels, f"{camera}: {deferred} pixels deferred -- the pair is not exercised on both sides"


# ---- 3. against composition on the device ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,height,k", VA.SIZES)
@pytest.mark.parametrize("model", ("equirect", "fisheye"))
def test_ao_equals_rays_then_closest_then_occluded(ctx, aos, model, width, height, k):
    name = VA.FIXTURES[1]
    sc = VA.scene(name)
    v = V.standard_view(sc, model, width=width, height=height, k=k)
    want = VA.composition(ctx, aos(name), sc, v, VA.SAMPLES, 1.0, VA.BIAS)
    assert want[:, 1].sum() > 0 and 0 < want[:, 0].sum() < want[:, 1].sum(), "nothing casts, or every AO ray has the same fate"
    assert want[:, 1].max() <= v.rpp * VA.SAMPLES
    check(f"{name} {model} {width}x{height} k={k}", aos(name), v, want)


# ---- 4. tiles --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", VA.MODELS)
@pytest.mark.parametrize("name", VA.FIXTURES)
def test_tiles_give_the_frames_rows(aos, name, model):
    v = V.standard_view(VA.scene(name), model)
    whole = VA.expected_standard(name, model)
    vacuity(f"{name} {model}", whole, 4)
    for row0, nrows in ((0, 3), (3, 1), (4, 3)):
        want = whole[row0 * W:(row0 + nrows) * W]
        assert want[:, 1].any()
        check(f"{name} {model} rows [{row0}, +{nrows})", aos(name), v.tile(row0, nrows), want)


# ---- 5. properties ---------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bytes_and_the_seeds_stay(ctx, aos):
    name = VA.FIXTURES[1]
    ao, v = aos(name), V.standard_view(VA.scene(name), "equirect")
    a, clean_a = ao.run(v)
    seeds = ao.seeds.read(np.int32)[:v.n_rays]
    assert np.array_equal(seeds, A.make_seeds(v.n_rays)), "mirt_seed_fill and a10_pass.make_seeds disagree, or the seeds were written"
    b, clean_b = ao.run(v)
    assert a.tobytes() == b.tobytes() and clean_a and clean_b
    # seeds of the caller's own are taken as they are, and are still there afterwards
    own = (A.make_seeds(v.n_rays, first=12345) ^ 0x2A).astype(np.int32)
    c, clean_c = ao.run(v, seeds=own)
    assert clean_c and np.array_equal(ao.seeds.read(np.int32)[:v.n_rays], own)
    assert np.array_equal(c, VA.expected(VA.scene(name), v, seeds=own)) and np.array_equal(c[:, 1], a[:, 1]) and not np.array_equal(c, a)


@pytest.mark.parametrize("samples", [1, 5, 64])
@pytest.mark.parametrize("model", ("equirect", "fisheye"))
def test_cast_is_the_guides_hit_count(ctx, aos, model, samples):
    """cornell_teapot3's material ids are all in range, so a sample casts exactly when the guides count it as a hit"""
    name = VA.FIXTURES[1]
    ao, v = aos(name), V.standard_view(VA.scene(name), model)
    nh = ctx.buffer(v.n_pixels * 16)
    try:
        got, clean = ao.run(v, samples=samples)
        open_, cast = got[:, 0], got[:, 1]
        assert clean and (cast % samples == 0).all() and cast.max() <= v.rpp * samples and (open_ <= cast).all()
        assert 0 < int(open_.sum()) < int(cast.sum())
        ctx.view_guides(ao.dev.pass_desc(None, None), v.desc(), nh, None)
        hits = nh.read(np.float32).reshape(-1, 4)[:, 3]
        assert np.array_equal(cast // samples, hits.astype(np.uint32))
        assert (cast == 0).any() and not got[cast == 0].any(), "a pixel with no hit is {0, 0}"
    finally:
        nh.release()


@pytest.mark.parametrize("name", VA.FIXTURES)
def test_ao_casts_where_a_cut_material_table_hides_the_hit_from_the_guides(ctx, aos, name):
    """no material is read: with two material entries the guides stop counting the samples with larger ids, AO gives what it gave, and a
    descriptor without any material does too"""
    sc, ao = VA.scene(name), aos(name)
    v = V.standard_view(sc, "equirect")
    want = VA.expected_standard(name, "equirect")
    cut = ctx.wrap(ao.dev.material.device_ptr, 2 * 16)
    nh = ctx.buffer(v.n_pixels * 16)
    try:
        desc = ao.scene_desc()
        desc.material = cut.h
        check(f"{name} two material entries", ao, v, want, scene_desc=desc)
        ctx.view_guides(desc, v.desc(), nh, None)
        hits = nh.read(np.float32).reshape(-1, 4)[:, 3].astype(np.uint32)
        assert (want[:, 1] // VA.SAMPLES >= hits).all() and (want[:, 1] // VA.SAMPLES > hits).any(), "the cut hides no hit from the guides"
        desc = ao.scene_desc()
        desc.material = None
        check(f"{name} no material", ao, v, want, scene_desc=desc)
    finally:
        nh.release()
        cut.release()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_leave_the_context_working(ctx, pkg):
    from raytracing_amd.pyhost import mirt, render
    L = mirt.lib()
    name = VA.FIXTURES[0]
    sc = VA.scene(name)
    view = V.standard_view(sc, "equirect")
    n, npx = view.n_rays, view.n_pixels
    dev = mirt.DeviceScene(ctx, sc)
    desc = dev.pass_desc(None, None)
    seeds, out = ctx.buffer(n * 4), ctx.buffer(npx * 8)
    short_seeds, short_out = ctx.buffer(n * 4 - 1), ctx.buffer(npx * 8 - 1)
    buffers = (seeds, out, short_seeds, short_out)
    extra = []

    def h(b):
        return b.h if isinstance(b, mirt.Buffer) else b

    def vd(**fields):
        d = view.desc(fields.pop("flags", 0))
        for k, val in fields.items():
            setattr(d, k, (C.c_float * 3)(*val) if isinstance(val, tuple) else val)
        return d

    def aod(samples=VA.SAMPLES, radius=1.0, bias=VA.BIAS, size=None):
        return mirt._AoDesc(C.sizeof(mirt._AoDesc) if size is None else size, samples, radius, bias)

    def ref(x):
        return C.byref(x) if x is not None else None

    def call(c=None, desc=desc, vd=vd(), ao=aod(), seeds=seeds, out=out):
        return L.mirt_view_ao(c or ctx.h, ref(desc), ref(vd), ref(ao), h(seeds), h(out))

    def fill():
        for b in buffers:
            b.write(np.full(b.nbytes, VA.SENTINEL, np.uint8))

    def clean(what):
        for b in buffers:
            assert (b.read(np.uint8) == VA.SENTINEL).all(), f"{what}: a buffer was written"

    def refused(code, **over):
        fill()
        assert call(**over) == code, (list(over), ctx.last_error())
        clean(list(over))

    def changed(**fields):
        d = dev.pass_desc(None, None)
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
        # MIRT_E_ARG: the descriptor checks of mirt_view_rays, the three descriptors' sizes, the AO descriptor's rules, NULL buffers, the mesh count rule
        for fields in bad_views:
            refused(E_ARG, vd=vd(**fields))
        refused(E_ARG, vd=None)
        refused(E_ARG, desc=None)
        refused(E_ARG, desc=changed(struct_size=desc.struct_size - 4))
        refused(E_ARG, ao=None)
        refused(E_ARG, ao=aod(size=12))
        for samples in (0, 65, 0xFFFFFFFF):
            refused(E_ARG, ao=aod(samples=samples))
        for radius in (0.0, -1.0, nan, -inf):
            refused(E_ARG, ao=aod(radius=radius))
        for bias in (-1e-9, nan, inf, -inf):
            refused(E_ARG, ao=aod(bias=bias))
        refused(E_ARG, seeds=None)
        refused(E_ARG, out=None)
        refused(E_ARG, desc=changed(n_meshes=17))               # MIRT_MAX_MESHES is 16
        refused(E_ARG, desc=changed(n_meshes=1, meshes=None))
        # MIRT_E_RANGE: seeds shorter than the tile's rays x 4 B, ao_out shorter than the tile's pixels x 8 B
        refused(E_RANGE, seeds=short_seeds)
        refused(E_RANGE, out=short_out)
        # MIRT_E_HANDLE: a bad context or buffer
        refused(E_HANDLE, c=fake)
        refused(E_HANDLE, seeds=fake)
        refused(E_HANDLE, out=fake)
        # aliasing: ao_out meets the seeds or a geometry buffer
        refused(E_ARG, out=seeds)
        last = ctx.wrap(seeds.device_ptr + (39 * 4 * 4 - 16), 39 * 8)   # a tile of 3 rows reads 39 * 4 seeds: these bytes begin with its last four
        extra.append(last)
        refused(E_ARG, out=last, vd=vd(nrows=3))
        prims = dev.tri["prims"] if dev.tri else dev.sph["prims"]
        assert prims.nbytes >= W * 8
        geo = ctx.wrap(prims.device_ptr, W * 8)
        extra.append(geo)
        before = prims.read(np.uint8).tobytes()
        refused(E_ARG, out=geo, vd=vd(nrows=1))
        assert prims.read(np.uint8).tobytes() == before
        # MIRT_E_DATA: a cell table that fails validation -- the loose triangles' offsets decrease
        off = dev.tri["off"]
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
            assert L.mirt_view_ao_deferred(ctx.h, C.byref(C.c_uint64())) == E_ARG
        finally:
            ctx.graph_release(ctx.capture_end())
        clean("inside a recording")
        assert L.mirt_view_ao_deferred(ctx.h, None) == E_ARG and L.mirt_view_ao_deferred(fake, C.byref(C.c_uint64())) == E_HANDLE
        # the accepted edges: k = 1, radius +inf, bias 0, the largest sample count, a set ACCUMULATE flag and a tone nobody reads
        ctx.seed_fill(seeds, 0, n)
        assert call(vd=vd(k=1, flags=V.ACCUMULATE, tone=nan), ao=aod(samples=64, radius=inf, bias=0.0)) == 0, ctx.last_error()
        # the same context gives the same view's AO afterwards ...
        assert call() == 0, ctx.last_error()
        d = VA.difference("after the refusals", out.read(np.uint32).reshape(-1, 2), VA.expected_standard(name, "equirect"))
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
        for b in extra + list(buffers):
            b.release()
        dev.release()
