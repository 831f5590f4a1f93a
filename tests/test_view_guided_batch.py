"""GPU: the frames of the batched view cameras and their guides in one call -- mirt_render_view_guided_batch (include/mirt.h) -- through the C ABI,
tolerance 0 (conftest.bits), all five buffers:

  1. against this library's own N mirt_render_view_guided calls, and against mirt_render_view_batch followed by mirt_view_guides_batch: both
     fixtures x three models at 13 x 7, k = 2, N = 3 (364 rays a frame: block 1 holds pixels of frames 0 and 1), bounces 2, under the
     optimistic / exact pair and under set_exact_only(True);
  2. the route: mirt_ctx_guided_views rises by exactly 1 per call for k in 1, 2, 4, 8, by 0 at k = 16 (3 x 1, N = 2: the two-launch route) and
     by 0 in a child process with MIRT_GUIDED_VIEW=0 (tests/view_batch_aov_switch_child.py), with the same bytes;
  3. a fresh call, then one with MIRT_VIEW_ACCUMULATE and tone 1 / (4 * 2), equal the per-frame chain, and the second call leaves the guides
     as they were; pixel only, radiance only;
  4. mixed deferral: ORTHOGRAPHIC where the middle camera of three looks along -z -- the buffers equal the singles, mirt_view_deferred is a
     multiple of 256 and at least 512, and 0 under exact_only; the middle frame has 66 full pixels by the oracle;
  5. every refusal of the header's list, the buffers pre-filled and compared afterwards; then the same context runs the batch correctly and
     cornell_32x24_r4 still renders equal to the oracle.
"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import a10_pass as A
import view_batch_aov_common as BA
import view_batch_common as VB
import view_common as V
import view_guides_common as VG
from conftest import ROOT, bits

pytestmark = pytest.mark.gpu

E_ARG, E_HANDLE, E_RANGE, E_DATA = -1, -2, -5, -8
FIXTURES, MODELS, N, BOUNCES = BA.FIXTURES, BA.MODELS, BA.N, BA.BOUNCES


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


def digest(got):
    """one hash over the five buffers of a guided result"""
    h = hashlib.sha256()
    for a in got[0][:3] + got[1][:2]:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


# ---- 1. against the single calls and against the two batch calls -----------------------------------------------------------------------------------
@pytest.mark.parametrize("exact_only", [False, True], ids=["pair", "exact_only"])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", FIXTURES)
def test_the_five_buffers_equal_the_single_calls_and_the_two_batch_calls(ctx, aov, name, model, exact_only):
    sc, r = BA.scene(name), aov(name)
    v = V.standard_view(sc, model, tone=0.25)
    cams = VB.cameras(sc, N)
    seeds = A.make_seeds(N * v.n_rays)
    ctx.set_exact_only(exact_only)
    try:
        singles = r.guided_singles(v, cams, seeds)
        assert (singles[0][1][:, 3] > 0).any(), "no pixel received light"
        assert (singles[0][0] != seeds).any(), "no seed advanced"
        assert (singles[1][0][:, 3] > 0).any(), "nothing was hit"
        two = r.two_batch_calls(v, cams, seeds)
        before = ctx.guided_views()
        got = r.guided_batch(v, cams, seeds)
        assert ctx.guided_views() - before == 1, "k = 2 takes the one-launch route, counted once for the batch"
        BA.same_guided(f"{name} {model} exact_only={exact_only} against the singles", got, singles)
        BA.same_guided(f"{name} {model} exact_only={exact_only} against the two batch calls", got, two)
    finally:
        ctx.set_exact_only(False)


# ---- 2. the route ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", V.KS)
def test_the_route_follows_k(ctx, aov, k):
    name = FIXTURES[1]
    sc, r = BA.scene(name), aov(name)
    width, height, n = (3, 1, 2) if k == 16 else (5, 3, 3)
    v = V.standard_view(sc, "equirect", width=width, height=height, k=k, tone=1.0 / (k * k))
    cams = VB.cameras(sc, n)
    seeds = A.make_seeds(n * v.n_rays)
    want = r.guided_singles(v, cams, seeds)
    assert (want[1][0][:, 3] > 0).any(), "nothing was hit"
    before = ctx.guided_views()
    got = r.guided_batch(v, cams, seeds)
    assert ctx.guided_views() - before == (0 if k == 16 else 1), f"k = {k}"
    BA.same_guided(f"{name} equirect {width}x{height} k={k}", got, want)
    BA.same_guided(f"{name} equirect {width}x{height} k={k} against the two batch calls", got, r.two_batch_calls(v, cams, seeds))


def test_the_switch_forces_the_two_launches_with_the_same_bytes(aov):
    name = FIXTURES[1]
    sc, r = BA.scene(name), aov(name)
    v = V.standard_view(sc, "fisheye", tone=0.25)
    here = digest(r.guided_batch(v, VB.cameras(sc, N), A.make_seeds(N * v.n_rays)))
    env = dict(os.environ, MIRT_GUIDED_VIEW="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "view_batch_aov_switch_child.py"), name], env=env, capture_output=True, text=True,
                       timeout=600)
    lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert p.returncode == 0 and lines, (lines[-1:] or p.stderr[-2000:])
    assert lines[-1]["routed"] == 0, lines[-1]
    assert lines[-1]["digest"] == here, "the two-launch route leaves other bytes"


# ---- 3. progressive, single outputs --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_accumulate_continues_every_frames_chain_and_keeps_the_guides(aov, model):
    name = FIXTURES[0]
    sc, r = BA.scene(name), aov(name)
    cams = VB.cameras(sc, N)
    v1, v2 = V.standard_view(sc, model, tone=0.25), V.standard_view(sc, model, tone=1.0 / (4 * 2))
    seeds = A.make_seeds(N * v1.n_rays)
    w1 = r.guided_singles(v1, cams, seeds)
    w2 = r.guided_singles(v2, cams, w1[0][0], carry=w1[0][1])
    g1 = r.guided_batch(v1, cams, seeds)
    BA.same_guided(f"{model} fresh", g1, w1)
    g2 = r.guided_batch(v2, cams, g1[0][0], carry=g1[0][1])
    BA.same_guided(f"{model} accumulate", g2, w2)
    assert (bits(g2[0][1]) != bits(g1[0][1])).any() and (g2[0][1][:, 3] >= g1[0][1][:, 3]).all(), "the second call added to the first's sums"
    d = VG.differ(f"{model}: the guides of the second call", g2[1], g1[1])
    assert d is None, d


@pytest.mark.parametrize("model", MODELS)
def test_one_output_alone_is_what_both_give(aov, model):
    name = FIXTURES[1]
    sc, r = BA.scene(name), aov(name)
    v = V.standard_view(sc, model, tone=0.25)
    cams = VB.cameras(sc, N)
    seeds = A.make_seeds(N * v.n_rays)
    (sd, sums, px, _), guides = r.guided_singles(v, cams, seeds)
    BA.same_guided(f"{model} pixel only", r.guided_batch(v, cams, seeds, radiance=False), ((sd, None, px, True), guides))
    BA.same_guided(f"{model} radiance only", r.guided_batch(v.with_(tone=float("nan")), cams, seeds, pixel=False), ((sd, sums, None, True), guides))


# ---- 4. mixed deferral ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_a_frame_the_guard_refuses_goes_to_the_exact_kernel_among_frames_that_do_not(ctx, aov, name):
    sc, r = BA.scene(name), aov(name)
    v = V.standard_view(sc, "ortho", tone=0.25)
    cams = BA.mixed_cameras(sc)
    seeds = A.make_seeds(N * v.n_rays)
    P = v.n_pixels
    oracle = BA.expected_guides(name, "ortho", mixed=True)
    assert BA.guide_kinds(oracle[0][P:2 * P], v.rpp)[0] == 66
    want = r.guided_singles(v, cams, seeds)
    d = VG.differ(f"{name} mixed: the singles' guides against the oracle", want[1], oracle)
    assert d is None, d
    assert (want[0][1][:, 3] > 0).any(), "no pixel received light"
    BA.same_guided(f"{name} mixed, pair", r.guided_batch(v, cams, seeds), want)
    deferred = ctx.view_deferred()
    print(f"{name}: deferred {deferred} of {N * v.n_rays} rays")
    assert deferred % 256 == 0 and deferred >= 512, deferred
    ctx.set_exact_only(True)
    try:
        BA.same_guided(f"{name} mixed, exact_only", r.guided_batch(v, cams, seeds), want)
        assert ctx.view_deferred() == 0, "the exact kernel alone defers nothing"
    finally:
        ctx.set_exact_only(False)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_leave_the_context_working(ctx, pkg):
    from raytracing_amd.pyhost import mirt, render
    L = mirt.lib()
    name = FIXTURES[0]
    sc = BA.scene(name)
    view = V.standard_view(sc, "equirect", tone=0.25)
    good = VB.cameras(sc, N)
    n, npx, P, R = N * view.n_rays, N * view.n_pixels, view.n_pixels, view.n_rays
    r = BA.Aov(ctx, sc, n, npx, tail=0)
    desc = r.scene_desc(BOUNCES)
    short = {"seeds": ctx.buffer(n * 4 - 1), "radiance": ctx.buffer(npx * 16 - 1), "pixel": ctx.buffer(npx * 4 - 1), "nh": ctx.buffer(npx * 16 - 1),
             "ad": ctx.buffer(npx * 16 - 1)}
    outputs = (r.seeds, r.radiance, r.pixel, r.nh, r.ad) + tuple(short.values())
    extra = []

    def h(b):
        return b.h if isinstance(b, mirt.Buffer) else b

    def vd(flags=0, **fields):
        d = view.desc(flags)
        for k, val in fields.items():
            setattr(d, k, (C.c_float * 3)(*val) if isinstance(val, tuple) else val)
        return d

    def call(c=None, desc=desc, vd=vd(), cams=good, nf=N, seeds=r.seeds, radiance=r.radiance, pixel=r.pixel, nh=r.nh, ad=r.ad):
        keep = None if cams is None else np.ascontiguousarray(cams, np.float32)
        return L.mirt_render_view_guided_batch(c or ctx.h, C.byref(desc) if desc is not None else None, C.byref(vd) if vd is not None else None,
                                               None if keep is None else keep.ctypes.data_as(C.c_void_p), nf, h(seeds), h(radiance), h(pixel), h(nh), h(ad))

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
        d = r.scene_desc(BOUNCES)
        for k, val in fields.items():
            setattr(d, k, val)
        return d

    nan, inf = float("nan"), float("inf")
    bad_views = [dict(struct_size=100), dict(model=3), dict(flags=2), dict(flags=0x80000001), dict(k=0), dict(k=3), dict(k=32), dict(width=0), dict(height=0),
                 dict(width=65536), dict(height=65536), dict(model=0, half_w=0.0), dict(model=0, half_h=nan), dict(model=2, half_angle=0.0),
                 dict(model=2, half_angle=3.1415930), dict(t_min=-1.0), dict(t_min=nan), dict(t_max=nan), dict(t_max=0.0), dict(t_min=2.0, t_max=1.0),
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
        # the batch's rules first, then the frame's, then the guides'
        refused(E_ARG, cams=None, seeds=None, nh=None, ad=None)
        assert "cameras" in ctx.last_error(), ctx.last_error()
        for tone in (0.0, -1.0, nan, inf):
            refused(E_ARG, vd=vd(tone=tone))
        refused(E_ARG, seeds=None)
        refused(E_ARG, radiance=None, pixel=None)
        refused(E_ARG, vd=vd(flags=V.ACCUMULATE), radiance=None)
        refused(E_ARG, seeds=None, nh=None, ad=None)
        assert "seeds" in ctx.last_error(), ctx.last_error()
        refused(E_ARG, nh=None, ad=None)
        assert "normal_hits" in ctx.last_error(), ctx.last_error()
        refused(E_ARG, desc=changed(n_lights=9))
        refused(E_ARG, desc=changed(n_meshes=17))
        refused(E_ARG, desc=changed(lights=None))
        refused(E_ARG, desc=changed(n_meshes=1, meshes=None))
        # MIRT_E_RANGE: a buffer shorter than N frames, a material table shorter than one entry
        for key, name_ in (("seeds", "seeds"), ("radiance", "radiance"), ("pixel", "pixel"), ("nh", "nh"), ("ad", "ad")):
            refused(E_RANGE, **{name_: short[key]})
        refused(E_RANGE, vd=vd(k=4))
        refused(E_RANGE, cams=VB.cameras(sc, N + 1), nf=N + 1)
        small = ctx.wrap(r.dev.material.device_ptr, 8)
        extra.append(small)
        refused(E_RANGE, desc=changed(material=small.h))
        refused(E_HANDLE, c=fake)
        for key in ("seeds", "radiance", "pixel", "nh", "ad"):
            refused(E_HANDLE, **{key: fake})
        refused(E_HANDLE, desc=changed(material=None))
        # overlap, on the whole batch buffers
        refused(E_ARG, seeds=r.radiance)
        refused(E_ARG, pixel=r.radiance)
        refused(E_ARG, nh=r.radiance)
        refused(E_ARG, ad=r.nh)
        # ... a guide that begins inside the LAST frame's slice of the seeds, of the radiance, of the pixels
        pool = ctx.buffer(n * 4 + npx * 16 + npx * 16)
        pool.write(np.full(pool.nbytes, V.SENTINEL, np.uint8))
        extra.append(pool)
        for key, head, last_at in (("seeds", n * 4, (n - R) * 4), ("radiance", npx * 16, (npx - P) * 16), ("pixel", npx * 4, (npx - P) * 4)):
            first, guide = ctx.wrap(pool.device_ptr, head), ctx.wrap(pool.device_ptr + (last_at + 15) // 16 * 16, npx * 16)   # 16-byte aligned, inside the last frame
            extra[0:0] = [first, guide]
            for g in ("nh", "ad"):
                refused(E_ARG, **{key: first, g: guide})
            assert (pool.read(np.uint8) == V.SENTINEL).all()
        big = ctx.buffer(max(npx * 16, r.dev.material.nbytes))
        extra.append(big)
        fill()
        big.write(np.full(big.nbytes, V.SENTINEL, np.uint8))
        assert call(desc=changed(material=big.h), ad=big) == E_ARG, ctx.last_error()
        clean("albedo_depth is the material")
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
        seeds = A.make_seeds(n)
        want = r.guided_singles(view, good, seeds, bounces=BOUNCES)
        fill()
        r.seeds.write(seeds)
        assert call(vd=vd(eye=(nan, 0.0, 0.0), right=(0.0, inf, 0.0), up=(0.0, 0.0, -inf), forward=(nan, nan, nan))) == 0, ctx.last_error()
        got = ((r.seeds.read(np.int32), r.radiance.read(np.float32).reshape(-1, 4), r.pixel.read(np.uint8).reshape(-1, 4), True),
               (r.nh.read(np.float32).reshape(-1, 4), r.ad.read(np.float32).reshape(-1, 4), True))
        d = VG.same_frames("after the refusals", got, want)
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
        for b in extra + list(short.values()):
            b.release()
        r.release()
