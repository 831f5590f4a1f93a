"""GPU: mirt_render_guides -- the first-hit guide buffers (per pixel: sum of the hit samples' normals and their number, sum of their material
colours and of their hit distances; include/mirt.h) -- through the C ABI, tolerance 0 (every NaN equal to every NaN):

  1. against the CPU oracle: initTrace and the closest-hit kernels of oracle/liboracle.so, reduced with numpy in sample order, on all ten A10
     scenes at 240x135 with 4, 9 and 16 rays per pixel;
  2. against the reference binary on the device (oracle/ref_gpu.py), cornell and cornell_teapot3 at 480x270 x 16, and the same under the default
     contract (libmirt_default.so against the reference's default build) in a child process;
  3. against this library's own kernel-by-kernel path on the same device, at 25, 289 and 1024 rays per pixel;
  4. properties: tiles, repeatability, nothing else written, the hit count, empty pixels, independence of the passes;
  5. refusals: nothing is written and the context works afterwards.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import a10_pass as A
from conftest import ROOT, load_fixture
from guides_common import difference, expected_guides, reduce_guides

pytestmark = pytest.mark.gpu

# the ten scenes of the reference's Assign10 page, by the fixture that carries each one's packed inputs
A10_SCENES = ["basic_32x24_r4", "basic2_32x24_r4", "triangles_32x24_r4", "cornell_32x24_r4", "cornell_official_64x48_r1", "cornell_teapot_32x24_r4",
              "cornell_teapot2_32x24_r4", "cornell_teapot3_32x24_r4", "twoLights_32x24_r4", "threeLights_32x24_r1"]
HSACO = os.path.join(ROOT, "oracle", "_ref", "a10_gfx950.hsaco")
DEFAULT_HSACO = os.path.join(ROOT, "oracle", "_ref", "a10_gfx950_default.hsaco")
DEFAULT_LIB = os.path.join(ROOT, "2015-raytracing_amd", "libmirt_default.so")


@pytest.fixture(scope="module")
def ctx(pkg):
    from raytracing_amd.pyhost import mirt
    c = mirt.Context(0)
    yield c
    c.destroy()


@pytest.fixture(scope="module")
def oracle():
    return A.load_oracle()


def resized(name, w, h, rpp):
    from raytracing_amd.pyhost import scene
    _, sc0 = load_fixture(name)
    ps = scene.PackedScene(dict(sc0.d)).resized(w, h, rpp)
    return ps, A.Scene(ps.d)


class Guides:
    """the device scene of one packed scene and two output buffers, driven through mirt_render_guides"""

    def __init__(self, ctx, ps, npix=None):
        from raytracing_amd.pyhost import mirt
        self.ctx, self.ps = ctx, ps
        self.dev = mirt.DeviceScene(ctx, ps)
        self.npix = ps.width * ps.height if npix is None else npix
        self.nh, self.ad = ctx.buffer(self.npix * 16), ctx.buffer(self.npix * 16)

    def desc(self, row0=0, nrows=0, seeds=None, acu=None):
        return self.dev.pass_desc(seeds, acu, row0=row0, nrows=nrows)

    def run(self, row0=0, nrows=0, **kw):
        self.ctx.render_guides(self.desc(row0, nrows, **kw), self.nh, self.ad)
        n = (nrows or self.ps.height) * self.ps.width
        return self.nh.read(np.float32, count=4 * n).reshape(-1, 4), self.ad.read(np.float32, count=4 * n).reshape(-1, 4)

    def release(self):
        self.nh.release()
        self.ad.release()
        self.dev.release()


def check(tag, got, want):
    for name, g, w in (("normal_hits", got[0], want[0]), ("albedo_depth", got[1], want[1])):
        d = difference(f"{tag} {name}", g, w)
        assert d is None, d


# ---- 1. the CPU oracle ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rpp", [4, 9, 16])
@pytest.mark.parametrize("name", A10_SCENES)
def test_guides_equal_the_cpu_oracle(ctx, oracle, name, rpp):
    ps, sc = resized(name, 240, 135, rpp)
    want = expected_guides(oracle, sc)
    g = Guides(ctx, ps)
    try:
        check(f"{name} x{rpp}", g.run(), want)
        ctx.set_exact_only(True)    # the exact kernel alone gives the same bits as the optimistic pair
        try:
            check(f"{name} x{rpp} exact kernel only", g.run(), want)
        finally:
            ctx.set_exact_only(False)
    finally:
        g.release()


# ---- 2. the reference binary on the device ---------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HSACO), reason="oracle/_ref/a10_gfx950.hsaco not built (make -C oracle ref_gpu, build container)")
@pytest.mark.parametrize("name", ["cornell_32x24_r4", "cornell_teapot3_32x24_r4"])
def test_guides_equal_the_reference_binary(ctx, name):
    import ref_gpu as G
    ps, sc = resized(name, 480, 270, 16)
    k = G.GpuRefKernels()
    g = Guides(ctx, ps)
    try:
        check(f"{name} 480x270 x16", g.run(), expected_guides(k, sc))
    finally:
        k.release()
        g.release()


@pytest.mark.skipif(not (os.path.exists(DEFAULT_HSACO) and os.path.exists(DEFAULT_LIB)), reason="needs the default-build code object and libmirt_default.so")
def test_guides_equal_the_default_build_of_the_reference():
    """libmirt_default.so against the reference's code.cl as its own host builds it, in a process of its own (a process loads one libmirt)"""
    env = dict(os.environ, MIRT_CONTRACT="default")
    env.pop("MIRT_LIB_PATH", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "guides_default_child.py")], env=env, capture_output=True, text=True, timeout=600)
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0, (lines[-1:] or r.stderr[-2000:])
    assert len(lines) == 2 and all(l["ok"] for l in lines)


# ---- 3. this library's kernel-by-kernel path ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rpp", [25, 289, 1024])
@pytest.mark.parametrize("name,w,h", [("basic_32x24_r4", 24, 16), ("triangles_32x24_r4", 24, 16), ("cornell_teapot3_32x24_r4", 24, 16), ("cornell_16x12_r9", 16, 12)])
def test_guides_equal_the_kernel_by_kernel_path(pkg, name, w, h, rpp):
    """spheres only, loose triangles, two grid meshes, and the lens grid whose rays are NaN: initTrace and the trace kernels through
    mirt_kernel_get / mirt_enqueue, their Ray and Poi buffers read back and reduced"""
    from raytracing_amd.pyhost import mirt, render
    ps, sc = resized(name, w, h, rpp)
    c = mirt.Context(0)
    c.set_fusion(0)
    gr = render.GranularRenderer(c, ps)
    g = Guides(c, ps)
    try:
        gr.k["initTrace"].set_arg(4, ps.cam).enqueue(gr.gws["initTrace"], gr.lws["initTrace"])
        gr._closest()
        c.finish()
        rays, pois = gr.read("rays").view(A.RAY_DT), gr.read("pois").view(A.POI_DT)
        want = reduce_guides(rays["maxt"], pois["normal"], pois["matId"], ps.materials, rpp)
        check(f"{name} {w}x{h} x{rpp}", g.run(), want)
    finally:
        g.release()
        gr.release()
        c.destroy()


# ---- 4. properties ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_32x24_r4", "cornell_teapot3_32x24_r4"])
def test_uneven_row_tiles_equal_the_rows_of_the_full_frame(ctx, name):
    ps, _ = resized(name, 96, 54, 9)
    g = Guides(ctx, ps)
    try:
        full = [a.copy() for a in g.run()]
        row = 0
        for nrows in (1, 7, 13, 33):
            got = g.run(row0=row, nrows=nrows)
            lo, hi = row * ps.width, (row + nrows) * ps.width
            check(f"{name} rows [{row}, +{nrows})", got, (full[0][lo:hi], full[1][lo:hi]))
            row += nrows
        assert row == ps.height
    finally:
        g.release()


def test_two_calls_give_identical_bytes_and_nothing_else_is_written(ctx):
    ps, _ = resized("cornell_teapot3_32x24_r4", 96, 54, 16)
    n = ps.total_rays
    g = Guides(ctx, ps)
    seeds_in = A.make_seeds(n, seed_base=3)
    acu_in = np.arange(4 * n, dtype=np.float32)
    seeds, acu = ctx.buffer(n * 4), ctx.buffer(n * 16)
    seeds.write(seeds_in)
    acu.write(acu_in)
    try:
        a = [x.copy() for x in g.run(seeds=seeds, acu=acu)]
        b = g.run(seeds=seeds, acu=acu)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        assert np.array_equal(seeds.read(np.int32), seeds_in), "seeds changed"
        assert acu.read(np.float32).tobytes() == acu_in.tobytes(), "acu changed"
        check("without seeds and acu in the descriptor", g.run(), a)
    finally:
        for x in (seeds, acu):
            x.release()
        g.release()


@pytest.mark.parametrize("name,rpp", [("basic_32x24_r4", 16), ("cornell_teapot3_32x24_r4", 9), ("cornell_16x12_r9", 9)])
def test_hits_is_a_count_and_an_empty_pixel_is_all_plus_zero(ctx, name, rpp):
    ps, _ = resized(name, 96, 54, rpp)
    g = Guides(ctx, ps)
    try:
        nh, ad = g.run()
        hits = nh[:, 3]
        assert np.array_equal(hits, np.floor(hits)) and hits.min() >= 0 and hits.max() <= rpp
        empty = hits == 0
        assert not nh[empty].view(np.uint32).any() and not ad[empty].view(np.uint32).any(), "a pixel without a hit is (+0, +0, +0, +0) in both outputs"
        if name == "basic_32x24_r4":
            assert empty.any() and (~empty).any()   # spheres in front of nothing: both kinds of pixel occur
    finally:
        g.release()


def test_guides_are_the_same_before_and_after_the_first_pass(ctx):
    from raytracing_amd.pyhost import render
    ps, _ = resized("cornell_teapot3_32x24_r4", 96, 54, 4)
    fr = render.FusedRenderer(ctx, ps)
    try:
        before = fr.guides()
        fr.execute_render(fresh=True)
        after = fr.guides()
        check("after mirt_render_first_pass", after, before)
        check("rows (10, 20) of FusedRenderer.guides", fr.guides(rows=(10, 20)), (before[0][10 * 96:30 * 96], before[1][10 * 96:30 * 96]))
    finally:
        fr.release()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_leave_the_context_working(ctx):
    from raytracing_amd.pyhost import mirt
    ps, _ = resized("cornell_32x24_r4", 48, 27, 4)
    g = Guides(ctx, ps)
    npix = g.npix
    fill = np.full(4 * npix, 7.5, np.float32)
    small = ctx.buffer(npix * 16 - 1)
    sfill = np.full(npix * 16 - 1, 0x5A, np.uint8)

    def refused(code, call, word):
        g.nh.write(fill)
        g.ad.write(fill)
        small.write(sfill)
        with pytest.raises(mirt.MirtError) as e:
            call()
        assert e.value.code == code and word in str(e.value), str(e.value)
        assert g.nh.read(np.float32).tobytes() == fill.tobytes() and g.ad.read(np.float32).tobytes() == fill.tobytes(), "an output was written"
        assert small.read(np.uint8).tobytes() == sfill.tobytes(), "the short output was written"

    try:
        want = [a.copy() for a in g.run()]

        def with_rpp(rpp):
            d = g.desc()
            d.rays_per_pixel = rpp
            return d
        refused(-1, lambda: ctx.render_guides(with_rpp(1), g.nh, g.ad), "seeds[col]")
        refused(-1, lambda: ctx.render_guides(with_rpp(5), g.nh, g.ad), "not a square")
        refused(-1, lambda: ctx.render_guides(g.desc(), None, None), "both NULL")
        refused(-5, lambda: ctx.render_guides(g.desc(), small, g.ad), "normal_hits")
        refused(-5, lambda: ctx.render_guides(g.desc(), g.nh, small), "albedo_depth")
        refused(-1, lambda: ctx.render_guides(g.desc(row0=20, nrows=8), g.nh, g.ad), "outside the image")
        d = g.desc()   # (made outside the recording: a new scene would be validated and prepared here)
        g.nh.write(fill)
        g.ad.write(fill)
        ctx.finish()
        ctx.capture_begin()
        try:
            with pytest.raises(mirt.MirtError) as e:
                ctx.render_guides(d, g.nh, g.ad)
            assert e.value.code == -1 and "capture" in str(e.value)
        finally:
            ctx.graph_release(ctx.capture_end())
        assert g.nh.read(np.float32).tobytes() == fill.tobytes() and g.ad.read(np.float32).tobytes() == fill.tobytes(), "written inside a recording"
        check("after the refusals", g.run(), want)
        # one output alone
        g.ad.write(fill)
        ctx.render_guides(g.desc(), g.nh, None)
        assert g.ad.read(np.float32).tobytes() == fill.tobytes()
        assert difference("normal_hits alone", g.nh.read(np.float32), want[0]) is None
    finally:
        small.release()
        g.release()
