"""GPU: the first-hit guides of the batched view cameras -- mirt_view_guides_batch (include/mirt.h) -- through the C ABI, tolerance 0
(conftest.bits).  The definition is by composition, so the yardstick is the single call:

  1. the batch against this library's own N mirt_view_guides calls: both fixtures x three models at 13 x 7, k = 2, N = 3 (273 pixels: a block
     border inside frame 2, a ragged last block of 17), under the optimistic / exact pair and under set_exact_only(True); every k at 5 x 3,
     N = 3 (45 pixels: one wave holds three frames); 16 x 16 k = 1 N = 2, 1 x 1 k = 1 N = 5 and 3 x 1 k = 16 N = 2, equirect;
  2. the batch against the oracle (view_guides_common.expected per frame, concatenated), with the non-vacuity conditions asserted on the
     oracle's result: over the batch a pixel with hits == rpp, one with 0 < hits < rpp, one all-zero, and frame 0's normal_hits unlike every
     other frame's;
  3. normal_hits alone and albedo_depth alone are what both give; N = 1 is mirt_view_guides;
  4. mixed deferral: ORTHOGRAPHIC where the middle camera of three looks along -z, so the ray-side guard refuses every ray of its frame --
     the guides equal the singles under the pair and under exact_only, and the middle frame has 66 full pixels by the oracle;
  5. every refusal of the header's list, the buffers pre-filled and compared afterwards; then the same context runs the batch correctly and
     cornell_32x24_r4 still renders equal to the oracle.
"""
import ctypes as C

import numpy as np
import pytest

import a10_pass as A
import view_batch_aov_common as BA
import view_batch_common as VB
import view_common as V
import view_guides_common as VG
from conftest import bits

pytestmark = pytest.mark.gpu

E_ARG, E_HANDLE, E_RANGE, E_DATA = -1, -2, -5, -8
FIXTURES, MODELS, N = BA.FIXTURES, BA.MODELS, BA.N


@pytest.fixture(scope="module")
def ctx(pkg):
    from raytracing_amd.pyhost import mirt
    c = mirt.Context(0)
    yield c
    c.destroy()


@pytest.fixture(scope="module")
def aov(ctx):
    made = {}

    def get(name):
        if name not in made:
            made[name] = BA.Aov(ctx, BA.scene(name))
        return made[name]
    yield get
    for r in made.values():
        r.release()


# ---- 1. against this library's own single calls ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact_only", [False, True], ids=["pair", "exact_only"])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", FIXTURES)
def test_the_guides_equal_the_single_calls(ctx, aov, name, model, exact_only):
    sc, r = BA.scene(name), aov(name)
    v = V.standard_view(sc, model)
    cams = VB.cameras(sc, N)
    ctx.set_exact_only(exact_only)
    try:
        want = r.guides_singles(v, cams)
        assert (want[0][:, 3] > 0).any(), "nothing was hit"
        BA.same_guides(f"{name} {model} exact_only={exact_only}", r.guides_batch(v, cams), want)
    finally:
        ctx.set_exact_only(False)


@pytest.mark.parametrize("k", V.KS)
def test_the_guides_equal_the_single_calls_at_every_k(aov, k):
    name = FIXTURES[1]
    sc, r = BA.scene(name), aov(name)
    v = V.standard_view(sc, "equirect", width=5, height=3, k=k)
    cams = VB.cameras(sc, N)
    want = r.guides_singles(v, cams)
    assert (want[0][:, 3] == k * k).any(), "no pixel every sample of which hit"
    BA.same_guides(f"{name} equirect 5x3 k={k}", r.guides_batch(v, cams), want)


@pytest.mark.parametrize("width,height,k,n", [s for s in BA.OTHER_SHAPES if s != (5, 3, 2, 3)])
@pytest.mark.parametrize("name", FIXTURES)
def test_the_guides_equal_the_single_calls_at_the_other_shapes(aov, name, width, height, k, n):
    sc, r = BA.scene(name), aov(name)
    v = V.standard_view(sc, "equirect", width=width, height=height, k=k)
    cams = VB.cameras(sc, n)
    want = r.guides_singles(v, cams)
    assert (want[0][:, 3] > 0).any(), "nothing was hit"
    BA.same_guides(f"{name} equirect {width}x{height} k={k} N={n}", r.guides_batch(v, cams), want)


# ---- 2. against the oracle ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", FIXTURES)
def test_the_guides_equal_the_oracle(aov, name, model):
    sc, r = BA.scene(name), aov(name)
    v = V.standard_view(sc, model)
    cams = VB.cameras(sc, N)
    want = BA.expected_guides(name, model)
    P = v.n_pixels
    per_frame = [BA.guide_kinds(want[0][f * P:(f + 1) * P], v.rpp) for f in range(N)]
    print(f"{name} {model}: oracle full / partial / empty per frame {per_frame}")
    full, part, empty = (sum(k[i] for k in per_frame) for i in range(3))
    assert full > 0 and part > 0 and empty > 0, f"the case is vacuous: full {full}, partial {part}, empty {empty}"
    for f in range(1, N):
        assert (bits(want[0][0:P]) != bits(want[0][f * P:(f + 1) * P])).any(), f"frame {f} has frame 0's normal_hits"
    BA.same_guides(f"{name} {model} against the oracle", r.guides_batch(v, cams), want)


# ---- 3. one output alone, one frame --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_one_output_alone_is_what_both_give(aov, model):
    name = FIXTURES[1]
    sc, r = BA.scene(name), aov(name)
    v = V.standard_view(sc, model)
    cams = VB.cameras(sc, N)
    both = r.guides_batch(v, cams)
    assert both[2] and (both[0][:, 3] > 0).any()
    BA.same_guides(f"{model} normal_hits alone", r.guides_batch(v, cams, ad=False), (both[0], None))
    BA.same_guides(f"{model} albedo_depth alone", r.guides_batch(v, cams, nh=False), (None, both[1]))


@pytest.mark.parametrize("model", MODELS)
def test_one_frame_is_view_guides(aov, model):
    name = FIXTURES[0]
    sc, r = BA.scene(name), aov(name)
    v = V.standard_view(sc, model)
    cams = VB.cameras(sc, 3)[1:2]
    want = r.guides_singles(v, cams)
    assert (want[0][:, 3] > 0).any()
    BA.same_guides(f"{model} N=1", r.guides_batch(v, cams), want)


# ---- 4. mixed deferral ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_a_frame_the_guard_refuses_goes_to_the_exact_kernel_among_frames_that_do_not(ctx, aov, name):
    sc, r = BA.scene(name), aov(name)
    v = V.standard_view(sc, "ortho")
    cams = BA.mixed_cameras(sc)
    P = v.n_pixels
    oracle = BA.expected_guides(name, "ortho", mixed=True)
    middle = BA.guide_kinds(oracle[0][P:2 * P], v.rpp)
    print(f"{name}: oracle full / partial / empty of the middle frame {middle}")
    assert middle[0] == 66, middle
    want = r.guides_singles(v, cams)
    d = VG.differ(f"{name} mixed: the singles against the oracle", want, oracle)
    assert d is None, d
    BA.same_guides(f"{name} mixed, pair", r.guides_batch(v, cams), want)
    ctx.set_exact_only(True)
    try:
        BA.same_guides(f"{name} mixed, exact_only", r.guides_batch(v, cams), want)
    finally:
        ctx.set_exact_only(False)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_leave_the_context_working(ctx, pkg):
    from raytracing_amd.pyhost import mirt, render
    L = mirt.lib()
    name = FIXTURES[0]
    sc = BA.scene(name)
    view = V.standard_view(sc, "equirect")
    good = VB.cameras(sc, N)
    npx = N * view.n_pixels
    r = BA.Aov(ctx, sc, N * view.n_rays, npx, tail=0)
    desc = r.scene_desc()
    short_nh, short_ad = ctx.buffer(npx * 16 - 1), ctx.buffer(npx * 16 - 1)
    outputs = (r.nh, r.ad, short_nh, short_ad)
    extra = []

    def h(b):
        return b.h if isinstance(b, mirt.Buffer) else b

    def vd(flags=0, **fields):
        d = view.desc(flags)
        for k, val in fields.items():
            setattr(d, k, (C.c_float * 3)(*val) if isinstance(val, tuple) else val)
        return d

    def call(c=None, desc=desc, vd=vd(), cams=good, nf=N, nh=r.nh, ad=r.ad):
        keep = None if cams is None else np.ascontiguousarray(cams, np.float32)
        return L.mirt_view_guides_batch(c or ctx.h, C.byref(desc) if desc is not None else None, C.byref(vd) if vd is not None else None,
                                        None if keep is None else keep.ctypes.data_as(C.c_void_p), nf, h(nh), h(ad))

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

    def changed(**fields):
        d = r.scene_desc()
        for k, val in fields.items():
            setattr(d, k, val)
        return d

    nan, inf = float("nan"), float("inf")
    bad_views = [dict(struct_size=100), dict(model=3), dict(flags=2), dict(k=0), dict(k=3), dict(k=32), dict(width=0), dict(height=0), dict(width=65536),
                 dict(height=65536), dict(model=0, half_w=0.0), dict(model=0, half_h=nan), dict(model=2, half_angle=0.0), dict(model=2, half_angle=3.1415930),
                 dict(t_min=-1.0), dict(t_min=nan), dict(t_max=nan), dict(t_max=0.0), dict(t_min=2.0, t_max=1.0),
                 dict(row0=1), dict(row0=BA.H), dict(nrows=3), dict(nrows=BA.H + 1), dict(row0=1, nrows=BA.H - 1), dict(width=65535, height=65535, k=1)]
    not_a_handle = C.create_string_buffer(64)
    fake = C.c_void_p(C.addressof(not_a_handle))
    try:
        for fields in bad_views:
            refused(E_ARG, vd=vd(**fields))
        refused(E_ARG, vd=None)
        refused(E_ARG, desc=None)
        refused(E_ARG, desc=changed(struct_size=desc.struct_size - 4))
        refused(E_ARG, cams=None)
        for frame, slot, val in ((0, 0, nan), (1, 4, inf), (2, 11, -inf), (2, 8, nan)):
            bad = good.copy()
            bad[frame, slot] = val
            refused(E_ARG, cams=bad)
            assert f"frame {frame}" in ctx.last_error(), ctx.last_error()
        refused(E_ARG, vd=vd(width=16, height=16, k=1), nf=1 << 24)
        # the batch's rules come first: a NULL table with both guides missing is the table's refusal
        refused(E_ARG, cams=None, nh=None, ad=None)
        assert "cameras" in ctx.last_error(), ctx.last_error()
        # mirt_view_guides' own
        refused(E_ARG, nh=None, ad=None)
        assert "normal_hits" in ctx.last_error(), ctx.last_error()
        refused(E_ARG, desc=changed(n_meshes=17))
        refused(E_ARG, desc=changed(n_meshes=1, meshes=None))
        refused(E_ARG, ad=r.nh)                                 # one buffer for both
        # MIRT_E_RANGE: a buffer shorter than N frames, a material table shorter than one entry
        refused(E_RANGE, nh=short_nh)
        refused(E_RANGE, ad=short_ad)
        refused(E_RANGE, cams=VB.cameras(sc, N + 1), nf=N + 1)
        small = ctx.wrap(r.dev.material.device_ptr, 8)
        extra.append(small)
        refused(E_RANGE, desc=changed(material=small.h))
        refused(E_HANDLE, c=fake)
        refused(E_HANDLE, nh=fake)
        refused(E_HANDLE, ad=fake)
        refused(E_HANDLE, desc=changed(material=None))
        # overlap, on the whole batch buffers: albedo_depth inside the LAST frame's slice of normal_hits
        pool = ctx.buffer(2 * npx * 16)
        pool.write(np.full(pool.nbytes, V.SENTINEL, np.uint8))
        first, last = ctx.wrap(pool.device_ptr, npx * 16), ctx.wrap(pool.device_ptr + (npx - view.n_pixels) * 16, npx * 16)
        extra += [first, last, pool]
        refused(E_ARG, nh=first, ad=last)
        assert (pool.read(np.uint8) == V.SENTINEL).all()
        big = ctx.buffer(max(npx * 16, r.dev.material.nbytes))
        extra.append(big)
        fill()
        big.write(np.full(big.nbytes, V.SENTINEL, np.uint8))
        assert call(desc=changed(material=big.h), nh=big) == E_ARG, ctx.last_error()
        clean("normal_hits is the material")
        assert (big.read(np.uint8) == V.SENTINEL).all()
        off = r.dev.tri["off"]
        good_off = off.read(np.uint32)
        off.write(np.array([good_off[-1], 0], np.uint32))
        try:
            refused(E_DATA)
        finally:
            off.write(good_off)
        fill()
        ctx.finish()
        ctx.capture_begin()
        try:
            assert call() == E_ARG and "capture" in ctx.last_error()
        finally:
            ctx.graph_release(ctx.capture_end())
        clean("inside a recording")
        fill()
        assert call(nf=0) == 0 and call(nf=0, cams=None) == 0, ctx.last_error()
        clean("no frames")
        # the descriptor's own basis is neither read nor checked; the same context runs the batch afterwards ...
        want = r.guides_singles(view, good)
        fill()
        assert call(vd=vd(eye=(nan, 0.0, 0.0), right=(0.0, inf, 0.0), up=(0.0, 0.0, -inf), forward=(nan, nan, nan))) == 0, ctx.last_error()
        got = (r.nh.read(np.float32).reshape(-1, 4), r.ad.read(np.float32).reshape(-1, 4))
        d = VG.differ("after the refusals", got, want)
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
