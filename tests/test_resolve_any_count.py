"""GPU: in-pass resolve at every ray count above 256 (pt_launch.hpp fused_segment: the segment plan; pt_kernels_fused.hip seg_ray).

A pixel's rays are cut, in ray order, into power-of-two segments of at most 256 -- floor(rpp / 256) of 256, then one per set bit of rpp % 256,
largest first (289 = 256 + 32 + 1).  One launch (optimistic + redo) covers one segment of every pixel, a block holding 256 / len pixels'
segments, and goes on from the sums the launch before it left -- the reference's single chain of additions (A10 code.cl:1377-1380), cut only at
segment boundaries.  So a frame's first pass needs no per-ray accumulator at any count above 256.  Everything is compared, tolerance 0, with the
separate copyToPixel of the same library over a kept accumulator (a context made with MIRT_INPASS_RESOLVE=0), and with the CPU oracle."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import a10_pass as A
from conftest import HOST, PAGE, ROOT, bits, load_fixture

pytestmark = pytest.mark.gpu

E_ARG = -1   # MIRT_E_ARG (include/mirt.h)
SCENES = ["cornell_32x24_r4", "cornell_teapot3_32x24_r4", "own_flat_32x24_r4"]
# small odd frames, so that the short segments leave partial blocks (7 x 5 pixels of one ray each are 35 lanes of a 256-lane block)
COUNTS = [(289, (7, 5)), (324, (7, 5)), (400, (7, 5)), (576, (7, 5)), (961, (3, 2)), (2304, (3, 2))]
node = shutil.which("node")


@pytest.fixture(scope="module")
def ctx(pkg):
    from raytracing_amd.pyhost import mirt
    c = mirt.Context(0)
    yield c
    c.destroy()


@pytest.fixture(scope="module")
def ctx_sep(pkg):
    """a context that never resolves in the pass (MIRT_INPASS_RESOLVE=0, read when a context is created): the separate copyToPixel"""
    from raytracing_amd.pyhost import mirt
    os.environ["MIRT_INPASS_RESOLVE"] = "0"
    try:
        c = mirt.Context(0)
    finally:
        del os.environ["MIRT_INPASS_RESOLVE"]
    yield c
    c.destroy()


def resized(name, rpp, size):
    from raytracing_amd.pyhost import scene
    fx, sc0 = load_fixture(name)
    ps = scene.PackedScene(dict(sc0.d)).resized(size[0], size[1], rpp)
    sc = A.Scene(ps.d)
    return ps, sc, A.make_seeds(sc.total_rays, seed_base=rpp + size[0])


def same(a, b, tag, radiance=True, acu=False):
    assert np.array_equal(a.pixel.read(np.uint8), b.pixel.read(np.uint8)), tag + ": pixel"
    if radiance:
        assert np.array_equal(bits(a.radiance.read(np.float32)), bits(b.radiance.read(np.float32))), tag + ": radiance"
    assert np.array_equal(a.seeds.read(np.int32), b.seeds.read(np.int32)), tag + ": seeds"
    if acu:
        assert np.array_equal(bits(a.acu.read(np.float32)), bits(b.acu.read(np.float32))), tag + ": acu"


@pytest.mark.parametrize("exact_only", [False, True], ids=["optimistic", "exact_only"])
@pytest.mark.parametrize("rpp,size", COUNTS, ids=[str(r) for r, _ in COUNTS])
@pytest.mark.parametrize("name", SCENES)
def test_first_pass_without_acu_at_any_count(ctx, ctx_sep, pkg, name, rpp, size, exact_only):
    """the acu-free first pass against the separate copyToPixel over a kept accumulator: pixel, radiance and seeds bit for bit, with and
    without a radiance buffer of the caller's; with acu kept (poisoned with NaN) every per-ray value too; two progressive passes with acu
    against two of the separate kernel.  own_flat defers samples: the blocks the exact kernel re-runs are whole."""
    from raytracing_amd.pyhost import render
    ps, sc, seeds = resized(name, rpp, size)
    ctx.set_exact_only(exact_only)
    ctx_sep.set_exact_only(exact_only)
    try:
        b = render.FusedRenderer(ctx_sep, ps, seeds=seeds)
        b.acu.write(np.full(sc.total_rays * 4, np.nan, np.float32))
        b.execute_render(fresh=True)                                   # accumulator + the separate copyToPixel
        deferred_samples = ctx_sep.pass_deferred()
        for want_radiance in (True, False):
            a = render.FusedRenderer(ctx, ps, seeds=seeds, keep_acu=False, want_radiance=want_radiance)
            a.pixel.write(np.full(sc.width * sc.height * 4, 7, np.uint8))
            a.execute_render(fresh=True)
            deferred_blocks = ctx.pass_deferred()
            same(a, b, f"{name} {rpp} radiance={want_radiance}", radiance=want_radiance)
            assert deferred_blocks % 256 == 0 and deferred_samples <= deferred_blocks <= 256 * deferred_samples, (deferred_samples, deferred_blocks)
            a.release()
        if name == "own_flat_32x24_r4" and not exact_only:
            assert deferred_samples > 0 and deferred_blocks > 0, "own_flat no longer defers: the redo launches between the segments are not exercised"
        a = render.FusedRenderer(ctx, ps, seeds=seeds, keep_acu=True)
        a.acu.write(np.full(sc.total_rays * 4, np.nan, np.float32))
        a.execute_render(fresh=True)
        same(a, b, f"{name} {rpp}, acu kept", acu=True)
        a.execute_render(fresh=False)                                  # a second progressive pass, the accumulator read and written
        b.execute_render(fresh=False)
        same(a, b, f"{name} {rpp}, two passes", acu=True)
        a.release()
        b.release()
    finally:
        ctx.set_exact_only(False)
        ctx_sep.set_exact_only(False)


@pytest.mark.parametrize("rpp", [289, 400])
def test_against_the_cpu_oracle(ctx, pkg, rpp):
    from raytracing_amd.pyhost import render
    ps, sc, seeds = resized("cornell_32x24_r4", rpp, (7, 5))
    a = render.FusedRenderer(ctx, ps, seeds=seeds, keep_acu=False)
    a.execute_render(fresh=True)
    st = A.PassState(sc, seeds)
    A.run_pass(A.load_oracle(), sc, st)
    assert np.array_equal(a.pixel.read(np.uint8).reshape(-1, 4), st.pixel)
    assert np.array_equal(a.seeds.read(np.int32), st.seeds)
    a.release()


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("name,rpp", [("cornell_32x24_r4", 289), ("cornell_teapot3_32x24_r4", 400), ("own_flat_32x24_r4", 324)])
def test_passes_in_one_launch_without_acu(ctx, pkg, name, rpp, n):
    """execute_passes(n, fresh=True) with no accumulator (mirt_render_passes, the MULTI kernels on each segment) against n ordinary passes"""
    from raytracing_amd.pyhost import render
    ps, sc, seeds = resized(name, rpp, (7, 5))
    b = render.FusedRenderer(ctx, ps, seeds=seeds)
    for p in range(n):
        b.execute_render(fresh=(p == 0))
    a = render.FusedRenderer(ctx, ps, seeds=seeds, keep_acu=False)
    a.pixel.write(np.full(sc.width * sc.height * 4, 7, np.uint8))
    a.execute_passes(n, fresh=True)
    same(a, b, f"{name} {rpp}, {n} passes in one launch")
    a.release()
    b.release()


@pytest.mark.parametrize("rpp", [289, 961])
def test_row_tiles(ctx, ctx_sep, pkg, rpp):
    """row tiles of the segment-by-segment resolve: their pixels are the whole frame's, nothing is written past the tile's pixel or radiance"""
    from raytracing_amd.pyhost import render
    ps, sc, seeds = resized("cornell_teapot3_32x24_r4", rpp, (5, 6))
    whole = render.FusedRenderer(ctx_sep, ps, seeds=seeds)
    whole.execute_render(fresh=True)
    want = whole.pixel.read(np.uint8).reshape(-1, 4)
    want_rad = bits(whole.radiance.read(np.float32).reshape(-1, 4))
    for row0, nrows in [(0, 1), (2, 3), (sc.height - 1, 1)]:
        fr = render.FusedRenderer(ctx, ps, seeds=seeds, row0=row0, nrows=nrows, keep_acu=False)
        npx = nrows * sc.width
        guard = np.full(npx * 4 + 256, 0xAB, np.uint8)
        fr.pixel.release()
        fr.pixel = ctx.buffer(guard.size)
        fr.pixel.write(guard)
        rguard = np.full(npx * 4 + 64, np.float32(-3.5), np.float32)
        fr.radiance.release()
        fr.radiance = ctx.buffer(rguard.nbytes)
        fr.radiance.write(rguard)
        fr.execute_render(fresh=True)
        got = fr.pixel.read(np.uint8)
        assert np.array_equal(got[:npx * 4].reshape(-1, 4), want[row0 * sc.width:(row0 + nrows) * sc.width]), (row0, nrows)
        assert np.all(got[npx * 4:] == 0xAB), "wrote past the tile's last pixel"
        rad = fr.radiance.read(np.float32)
        assert np.array_equal(bits(rad[:npx * 4].reshape(-1, 4)), want_rad[row0 * sc.width:(row0 + nrows) * sc.width])
        assert np.all(rad[npx * 4:] == np.float32(-3.5)), "wrote past the tile's last radiance sum"
        fr.release()
    whole.release()


def test_still_refused(ctx, pkg):
    """counts of at most 256 that do not divide it keep needing acu; a tile over the 32-bit ray limit is refused at any count"""
    from raytracing_amd.pyhost import mirt, render, scene
    fx, sc = load_fixture("cornell_16x12_r9")
    fr = render.FusedRenderer(ctx, sc, seeds=fx["seeds_in"], keep_acu=False)
    with pytest.raises(mirt.MirtError) as e:
        fr.execute_render(fresh=True)
    assert e.value.code == E_ARG and "acu" in str(e.value)
    fr.release()
    ps, sc, seeds = resized("cornell_32x24_r4", 289, (7, 5))
    fr = render.FusedRenderer(ctx, ps, seeds=seeds, keep_acu=False)
    with pytest.raises(mirt.MirtError) as e:
        fr.execute_render(fresh=False)                  # not a first pass: there is an accumulator to read
    assert e.value.code == E_ARG and "acu" in str(e.value)
    fr.release()
    _, sc0 = load_fixture("cornell_32x24_r4")
    big = scene.PackedScene(dict(sc0.d)).resized(4096, 4096, 289)   # 4.8e9 rays in one tile
    dev = mirt.DeviceScene(ctx, big)
    bufs = [ctx.buffer(16) for _ in range(3)]
    with pytest.raises(mirt.MirtError) as e:
        ctx.render_pass(dev.pass_desc(bufs[0], None, bufs[1], bufs[2]), fresh=True)
    assert e.value.code == E_ARG and "32 bits" in str(e.value)
    for b in bufs:
        b.release()
    dev.release()


DEFAULT_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
sys.path.insert(0, sys.argv[1] + "/oracle")
import __graft_entry__ as g
g.load_package()
from raytracing_amd.pyhost import mirt, render, scene
from conftest import load_fixture
import a10_pass as A
assert mirt.LIB_PATH.endswith("libmirt_default.so"), mirt.LIB_PATH
ctx = mirt.Context(0)
fx, sc0 = load_fixture("cornell_teapot3_32x24_r4")
ps = scene.PackedScene(dict(sc0.d)).resized(7, 5, 400)
seeds = A.make_seeds(7 * 5 * 400, seed_base=11)
b = render.FusedRenderer(ctx, ps, seeds=seeds)
b.execute_render(fresh=True)
a = render.FusedRenderer(ctx, ps, seeds=seeds, keep_acu=False)
a.execute_render(fresh=True)
ok = all(np.array_equal(x.read(np.uint8), y.read(np.uint8)) for x, y in ((a.pixel, b.pixel), (a.radiance, b.radiance), (a.seeds, b.seeds)))
print(json.dumps({"ok": bool(ok)}))
"""


@pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "2015-raytracing_amd", "libmirt_default.so")), reason="libmirt_default.so not built")
def test_default_contract_library(pkg):
    """libmirt_default.so gets the segment plan from the same sources: its acu-free first pass at 400 rays per pixel equals its own pass with
    the accumulator and the separate copyToPixel (a process of its own: a process loads one libmirt)"""
    env = dict(os.environ, MIRT_CONTRACT="default")
    env.pop("MIRT_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-c", DEFAULT_CHILD, ROOT], env=env, capture_output=True, text=True, timeout=600)
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and lines and lines[-1]["ok"], r.stderr[-2000:]


@pytest.mark.skipif(node is None, reason="node is not installed")
def test_node_cli_without_acu(tmp_path):
    """`cli.js render ... 289 1 ... --no-acu` (a 17 x 17 lens grid): the frame and radiance equal the same render with the accumulator"""
    scene_file = os.path.join(PAGE, "scenes", "gems.xml")
    outs = {}
    for tag, flags in (("acu", []), ("no_acu", ["--no-acu"])):
        out = str(tmp_path / (tag + ".rgba"))
        r = subprocess.run([node, os.path.join(HOST, "cli.js"), "render", scene_file, "9", "7", "289", "1", out, *flags], capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr.decode()
        outs[tag] = (open(out, "rb").read(), open(out + ".radiance.f32", "rb").read())
    assert outs["no_acu"][0] == outs["acu"][0], "frame"
    assert outs["no_acu"][1] == outs["acu"][1], "radiance"
