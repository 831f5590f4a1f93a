"""GPU: mirt_render_ao -- ambient occlusion of the first hit, {open, cast} per pixel in one launch (include/mirt.h) -- through the C ABI,
tolerance 0 (integers), against the restatement of tests/ao_common.py: initTrace, the closest-hit kernels, `samples` bouncePaths calls on a
scratch ray buffer, the casting samples' rays rewritten in numpy, the shadow kernels.

  a. against the CPU oracle (oracle/liboracle.so): every stratum of random_scenes_common.STRATA at 37x21 x 4 (rays_common.SCENE_SEEDS) with 3 AO
     rays -- together the three GRIDS variants of k_ao --, and cornell and cornell_teapot3 at 64x36 with 9 and 16 rays and 1 and 4 AO rays; each
     with the optimistic / exact pair and with the exact kernel alone; one case with radius = inf and one with bias = 0.
     The radii (RADIUS, FIXTURE_RADIUS) were found on the CPU with the oracle alone so that no case is vacuous: open / cast over the frame lies
     in [0.1, 0.9] (the oracle gives 0.67 .. 0.79 at these radii, 0.23 at inf on the enclosed scenes), and the `open` stratum has pixels that cast
     nothing (425 of 777).  Every case asserts that on the oracle's result before it compares.
  b. against the reference binary on the device (oracle/ref_gpu.py), cornell_teapot3 at 96x54 x 16 with 2 AO rays, and the same under the default
     contract in a child process (tests/ao_default_child.py);
  c. against this library's own kernel-by-kernel path on the device: initTrace, the closest-hit kernels and bouncePaths x samples through
     mirt_enqueue, then mirt_trace_occluded on the rewritten rays, at 25 rays per pixel, 20x12;
  d. properties: a row tile equals its rows of the frame, repeatability, seeds and the bytes behind ao_out untouched, the counts' ranges, the
     guides' hit count;
  e. mirt_ao_deferred on the `guard` stratum.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import a10_pass as A
import random_scenes_common as S
import rays_common as R
from ao_common import ROW_TILE, Ao, ao_rays, count_ao, difference, expected_ao
from conftest import ROOT, load_fixture

pytestmark = pytest.mark.gpu

HSACO = os.path.join(ROOT, "oracle", "_ref", "a10_gfx950.hsaco")
DEFAULT_HSACO = os.path.join(ROOT, "oracle", "_ref", "a10_gfx950_default.hsaco")
DEFAULT_LIB = os.path.join(ROOT, "2015-raytracing_amd", "libmirt_default.so")

SAMPLES, BIAS = 3, 0.001
# per stratum: about 0.28 of the scene box's diagonal (3.54; the guard stratum's geometry is scaled by 16).  Found with the oracle alone.
RADIUS = {"single_cell": 1.0, "staged": 1.0, "unstaged": 1.0, "many_sets": 1.0, "open": 1.0, "guard": 16.0}
FIXTURE_RADIUS = 1.0   # cornell's box has the diagonal 3.46, cornell_teapot3's 3.54
INF = float("inf")

_WANT = {}


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


def want_of(oracle, key, sc, samples, radius, bias):
    """the oracle's answer, computed once per case and left unchanged"""
    key = (key, samples, radius, bias)
    if key not in _WANT:
        w = expected_ao(oracle, sc, samples, radius, bias)
        w.setflags(write=False)
        _WANT[key] = w
    return _WANT[key]


def assert_not_vacuous(tag, want, samples, rpp, need_empty=False):
    """on the ORACLE's result alone: the frame's openness away from 0 and 1, hit pixels, and -- where asked -- pixels that cast nothing"""
    cast, open_ = int(want[:, 1].sum()), int(want[:, 0].sum())
    print(f"{tag}: oracle open {open_} / cast {cast} = {open_ / max(cast, 1):.4f}, {int((want[:, 1] == 0).sum())} of {len(want)} pixels cast nothing")
    assert cast > 0 and 0.1 <= open_ / cast <= 0.9, f"{tag}: the case is vacuous, open / cast = {open_} / {cast}"
    assert want[:, 1].max() <= rpp * samples
    if need_empty:
        assert (want[:, 1] == 0).any(), f"{tag}: no pixel without a hit"


def run_pair_and_exact(ctx, tag, ao, want, samples, radius, bias):
    got, tail = ao.run(samples, radius, bias)
    d = difference(tag, got, want)
    assert d is None, d
    assert (tail == Ao.SENTINEL).all(), f"{tag}: bytes behind ao_out were written"
    ctx.set_exact_only(True)    # the exact kernel alone gives the same pairs as the optimistic / exact pair
    try:
        got, tail = ao.run(samples, radius, bias)
    finally:
        ctx.set_exact_only(False)
    d = difference(f"{tag}, exact kernel only", got, want)
    assert d is None, d
    assert (tail == Ao.SENTINEL).all()


# ---- a. the CPU oracle -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stratum", S.STRATA)
def test_ao_of_every_stratum_equals_the_cpu_oracle(ctx, oracle, stratum):
    sc = R.scene(stratum)
    want = want_of(oracle, stratum, sc, SAMPLES, RADIUS[stratum], BIAS)
    assert_not_vacuous(stratum, want, SAMPLES, sc.rpp, need_empty=(stratum == "open"))
    ao = Ao(ctx, sc)
    try:
        run_pair_and_exact(ctx, f"{stratum} 37x21 x4, {SAMPLES} AO rays", ao, want, SAMPLES, RADIUS[stratum], BIAS)
    finally:
        ao.release()


@pytest.mark.parametrize("samples", [1, 4])
@pytest.mark.parametrize("rpp", [9, 16])
@pytest.mark.parametrize("name", ["cornell_32x24_r4", "cornell_teapot3_32x24_r4"])
def test_ao_of_the_a10_scenes_equals_the_cpu_oracle(ctx, oracle, name, rpp, samples):
    ps, sc = resized(name, 64, 36, rpp)
    want = want_of(oracle, (name, rpp), sc, samples, FIXTURE_RADIUS, BIAS)
    assert_not_vacuous(f"{name} x{rpp}", want, samples, rpp)
    ao = Ao(ctx, ps)
    try:
        run_pair_and_exact(ctx, f"{name} 64x36 x{rpp}, {samples} AO rays", ao, want, samples, FIXTURE_RADIUS, BIAS)
    finally:
        ao.release()


@pytest.mark.parametrize("stratum,radius,bias", [("single_cell", INF, BIAS), ("staged", 1.0, 0.0), ("many_sets", INF, 0.0)])
def test_ao_with_an_infinite_radius_and_without_bias_equals_the_cpu_oracle(ctx, oracle, stratum, radius, bias):
    """radius = inf: the AO ray is bouncePaths' own (maxt = inf); bias = 0: its origin is Poi.p bit for bit, ON the surface it leaves"""
    sc = R.scene(stratum)
    want = want_of(oracle, stratum, sc, SAMPLES, radius, bias)
    assert_not_vacuous(f"{stratum} radius {radius} bias {bias}", want, SAMPLES, sc.rpp)
    ao = Ao(ctx, sc)
    try:
        run_pair_and_exact(ctx, f"{stratum} radius {radius} bias {bias}", ao, want, SAMPLES, radius, bias)
    finally:
        ao.release()


# ---- b. the reference binary on the device -----------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HSACO), reason="oracle/_ref/a10_gfx950.hsaco not built (make -C oracle ref_gpu, build container)")
def test_ao_equals_the_reference_binary(ctx):
    import ref_gpu as G
    ps, sc = resized("cornell_teapot3_32x24_r4", 96, 54, 16)
    k = G.GpuRefKernels()
    ao = Ao(ctx, ps)
    try:
        want = expected_ao(k, sc, 2, FIXTURE_RADIUS, BIAS)
        assert_not_vacuous("cornell_teapot3 96x54 x16 by the reference binary", want, 2, 16)
        run_pair_and_exact(ctx, "cornell_teapot3 96x54 x16, 2 AO rays", ao, want, 2, FIXTURE_RADIUS, BIAS)
    finally:
        k.release()
        ao.release()


@pytest.mark.skipif(not (os.path.exists(DEFAULT_HSACO) and os.path.exists(DEFAULT_LIB)), reason="needs the default-build code object and libmirt_default.so")
def test_ao_equals_the_default_build_of_the_reference():
    """libmirt_default.so against the reference's code.cl as its own host builds it, in a process of its own (a process loads one libmirt)"""
    env = dict(os.environ, MIRT_CONTRACT="default")
    env.pop("MIRT_LIB_PATH", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ao_default_child.py")], env=env, capture_output=True, text=True, timeout=600)
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0, (lines[-1:] or r.stderr[-2000:])
    assert len(lines) == 1 and lines[0]["ok"] and 0.1 <= lines[0]["open"] / lines[0]["cast"] <= 0.9


# ---- c. this library's kernel-by-kernel path ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_32x24_r4", "cornell_teapot3_32x24_r4"])
def test_ao_equals_the_kernel_by_kernel_path(pkg, name):
    """initTrace, the closest-hit kernels and bouncePaths x samples through mirt_kernel_get / mirt_enqueue (the Poi buffer unchanged, the seeds
    advancing), the ray buffer read back after each and rewritten, mirt_trace_occluded on the casting samples' rays"""
    from raytracing_amd.pyhost import mirt, render
    samples, radius, rpp, w, h = 3, FIXTURE_RADIUS, 25, 20, 12
    ps, sc = resized(name, w, h, rpp)
    c = mirt.Context(0)
    c.set_fusion(0)
    gr = render.GranularRenderer(c, ps)
    ao = Ao(c, ps)
    tr = None
    try:
        gr.k["initTrace"].set_arg(4, ps.cam).enqueue(gr.gws["initTrace"], gr.lws["initTrace"])
        gr._closest()
        c.finish()
        pois = gr.read("pois").view(A.POI_DT).copy()
        cast = pois["matId"] >= 0
        tr = R.Tracer(c, sc, cap=max(int(cast.sum()), 1))
        occ = []
        for _ in range(samples):
            gr.k["bouncePaths"].enqueue(gr.g1, [64])
            c.finish()
            rays = gr.read("rays").view(A.RAY_DT)
            occ.append(tr.occluded(ao_rays(rays, pois, cast, radius, BIAS))[0].copy())
        want = count_ao(cast, occ, rpp)
        assert_not_vacuous(f"{name} kernel by kernel", want, samples, rpp)
        run_pair_and_exact(c, f"{name} {w}x{h} x{rpp}, {samples} AO rays", ao, want, samples, radius, BIAS)
    finally:
        if tr:
            tr.release()
        ao.release()
        gr.release()
        c.destroy()


# ---- d. properties -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stratum", ["staged", "open"])
def test_a_row_tile_equals_its_rows_of_the_whole_frame(ctx, stratum):
    sc = R.scene(stratum)
    row0, nrows = ROW_TILE
    full, tile = Ao(ctx, sc), Ao(ctx, sc, row0=row0, nrows=nrows)
    try:
        whole, _ = full.run(SAMPLES, RADIUS[stratum], BIAS)
        got, tail = tile.run(SAMPLES, RADIUS[stratum], BIAS)
        d = difference(f"{stratum} rows [{row0}, +{nrows})", got, whole[row0 * sc.width:(row0 + nrows) * sc.width])
        assert d is None, d
        assert (tail == Ao.SENTINEL).all()
        assert got[:, 1].any()
    finally:
        full.release()
        tile.release()


def test_two_calls_give_the_same_bytes_and_only_ao_out_is_written(ctx):
    sc = R.scene("many_sets")
    ao = Ao(ctx, sc)
    try:
        seeds_in = ao.seeds.read(np.int32).copy()
        assert np.array_equal(seeds_in, A.make_seeds(ao.nrays)), "mirt_seed_fill and a10_pass.make_seeds disagree"
        a, tail_a = ao.run(SAMPLES, RADIUS["many_sets"], BIAS)
        b, tail_b = ao.run(SAMPLES, RADIUS["many_sets"], BIAS)
        assert a.tobytes() == b.tobytes()
        assert (tail_a == Ao.SENTINEL).all() and (tail_b == Ao.SENTINEL).all(), "bytes behind ao_out were written"
        assert ao.seeds.read(np.int32).tobytes() == seeds_in.tobytes(), "the seeds were written"
    finally:
        ao.release()


@pytest.mark.parametrize("samples", [1, 5, 64])
def test_counts_are_in_range_and_cast_is_the_guides_hit_count(ctx, samples):
    """cast is a multiple of `samples`, at most rpp * samples, open <= cast; cornell_teapot3's material ids are all in range, so a sample
    casts exactly when the guides count it as a hit"""
    ps, _ = resized("cornell_teapot3_32x24_r4", 48, 27, 9)
    ao = Ao(ctx, ps)
    nh = ctx.buffer(ao.npix * 16)
    try:
        got, _ = ao.run(samples, FIXTURE_RADIUS, BIAS)
        open_, cast = got[:, 0], got[:, 1]
        assert (cast % samples == 0).all() and cast.max() <= ps.rpp * samples and (open_ <= cast).all()
        assert 0 < int(open_.sum()) < int(cast.sum())
        ctx.render_guides(ao.dev.pass_desc(None, None), nh, None)
        hits = nh.read(np.float32).reshape(-1, 4)[:, 3]
        assert np.array_equal(cast // samples, hits.astype(np.uint32))
        assert (cast == 0).any() and not got[cast == 0].any(), "a pixel with no hit is {0, 0}"
    finally:
        nh.release()
        ao.release()


def test_fused_renderer_ao(ctx):
    """FusedRenderer.ao: the renderer's own seeds, whole tile and a row range of it"""
    from raytracing_amd.pyhost import render
    sc = R.scene("staged")
    fr = render.FusedRenderer(ctx, sc)
    ao = Ao(ctx, sc)
    try:
        want, _ = ao.run(SAMPLES, RADIUS["staged"], BIAS)
        got = fr.ao(samples=SAMPLES, radius=RADIUS["staged"], bias=BIAS)
        assert got.dtype == np.uint32 and difference("FusedRenderer.ao", got, want) is None
        row0, nrows = ROW_TILE
        assert difference("FusedRenderer.ao(rows)", fr.ao(SAMPLES, RADIUS["staged"], BIAS, rows=ROW_TILE), want[row0 * sc.width:(row0 + nrows) * sc.width]) is None
    finally:
        ao.release()
        fr.release()


# ---- e. mirt_ao_deferred -----------------------------------------------------------------------------------------------------------------------
GUARD_SEED = R.SCENE_SEEDS["guard"]   # 3022: its frame has pixels on both sides of the guard


def test_ao_deferred_counts_the_pixels_of_the_guard_stratum(ctx, oracle):
    """the guard stratum's rays leave the optimistic kernel's windows for SOME pixels: those are counted, the others are not, and an exact-only
    call counts none"""
    sc = S.scene("guard", GUARD_SEED, *R.SCENE_SIZE)
    ao = Ao(ctx, sc)
    try:
        got, _ = ao.run(SAMPLES, RADIUS["guard"], BIAS)
        deferred = ctx.ao_deferred()
        print(f"guard seed {GUARD_SEED}: mirt_ao_deferred {deferred} of {ao.npix} pixels")
        assert 0 < deferred < ao.npix, deferred
        d = difference("guard", got, want_of(oracle, "guard", sc, SAMPLES, RADIUS["guard"], BIAS))
        assert d is None, d
        ctx.set_exact_only(True)
        try:
            ao.run(SAMPLES, RADIUS["guard"], BIAS)
            assert ctx.ao_deferred() == 0
        finally:
            ctx.set_exact_only(False)
    finally:
        ao.release()
