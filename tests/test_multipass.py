"""Several progressive passes in one call (mirt_render_passes; FusedRenderer.execute_passes; queue.renderPasses).

The contract (include/mirt.h): the call leaves every buffer the caller passes -- seeds, acu if given, pixel, radiance -- bit for bit as the
sequence of ordinary calls would (mirt_render_first_pass or mirt_render_pass at pass_index, then mirt_render_pass at each later index), with
the frame of the last pass.  One launch runs every sample through all the passes, so a frame of any pass count needs no per-ray
accumulator where a first pass can do without one.  Everything is compared with tolerance 0 against ordinary passes of the same library,
and against the CPU oracle."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import a10_pass as A
from conftest import FULL_CASES, HOST, PAGE, ROOT, bits, load_fixture

E_ARG = -1   # MIRT_E_ARG (include/mirt.h)
RESOLVABLE = [n for n in FULL_CASES if int(n.rsplit("_r", 1)[1]) > 1 and 256 % int(n.rsplit("_r", 1)[1]) == 0]
node = shutil.which("node")


@pytest.fixture(params=["default", "reuse", "plain"])
def loop(request, monkeypatch):
    """the two MULTI kernels, as the runtime picks them (primary-hit reuse for scenes without grids, else the plain pass loop) and each forced on
    every scene (MIRT_MULTIPASS_REUSE=1 / 0, read per launch)"""
    if request.param == "default":
        monkeypatch.delenv("MIRT_MULTIPASS_REUSE", raising=False)
    else:
        monkeypatch.setenv("MIRT_MULTIPASS_REUSE", "1" if request.param == "reuse" else "0")
    return request.param


@pytest.fixture(scope="module")
def ctx(pkg):
    from raytracing_amd.pyhost import mirt
    c = mirt.Context(0)
    yield c
    c.destroy()


def ordinary(ctx, sc, seeds, n, bounces=5, **kw):
    """the baseline: n ordinary passes (the first with initAcu folded in) into a kept accumulator"""
    from raytracing_amd.pyhost import render
    fr = render.FusedRenderer(ctx, sc, seeds=seeds, **kw)
    for p in range(n):
        fr.execute_render(bounces=bounces, fresh=(p == 0))
    return fr


def same_frame(a, b, tag, acu=True):
    assert np.array_equal(a.pixel.read(np.uint8), b.pixel.read(np.uint8)), tag + ": pixel"
    assert np.array_equal(bits(a.radiance.read(np.float32)), bits(b.radiance.read(np.float32))), tag + ": radiance"
    assert np.array_equal(a.seeds.read(np.int32), b.seeds.read(np.int32)), tag + ": seeds"
    if acu:
        assert np.array_equal(bits(a.acu.read(np.float32)), bits(b.acu.read(np.float32))), tag + ": acu"


def test_binding_declares_the_entry_point(pkg):
    """CPU: the header, the binding and the library agree on mirt_render_passes and its flag"""
    from raytracing_amd.pyhost import mirt
    text = open(os.path.join(ROOT, "include", "mirt.h")).read()
    assert "mirt_render_passes" in mirt.SYMBOLS and hasattr(mirt.lib(), "mirt_render_passes")
    assert f"#define MIRT_PASSES_FRESH {mirt.PASSES_FRESH}u" in text


@pytest.mark.gpu
@pytest.mark.parametrize("exact_only", [False, True], ids=["optimistic", "exact_only"])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("name", RESOLVABLE)
def test_passes_in_one_call_equal_ordinary_passes(ctx, pkg, name, n, exact_only, loop):
    from raytracing_amd.pyhost import render
    fx, sc = load_fixture(name)
    seeds = fx["seeds_in"]
    ctx.set_exact_only(exact_only)
    try:
        b = ordinary(ctx, sc, seeds, n)
        a = render.FusedRenderer(ctx, sc, seeds=seeds, keep_acu=False)   # no per-ray accumulator at all
        a.pixel.write(np.full(sc.width * sc.height * 4, 7, np.uint8))
        a.execute_passes(n, fresh=True)
        same_frame(a, b, f"{name} x{n}, no acu", acu=False)
        a.release()
        a = render.FusedRenderer(ctx, sc, seeds=seeds)                   # the accumulator kept: poisoned, not read, all of it written
        a.acu.write(np.full(sc.total_rays * 4, np.nan, np.float32))
        a.execute_passes(n, fresh=True)
        same_frame(a, b, f"{name} x{n}, acu")
        a.release()
        b.release()
    finally:
        ctx.set_exact_only(False)


@pytest.mark.gpu
@pytest.mark.parametrize("exact_only", [False, True], ids=["optimistic", "exact_only"])
def test_depth_8(ctx, pkg, exact_only, loop):
    from raytracing_amd.pyhost import render
    fx, sc = load_fixture("cornell_teapot3_32x24_r4")
    ctx.set_exact_only(exact_only)
    try:
        b = ordinary(ctx, sc, fx["seeds_in"], 3, bounces=8)
        a = render.FusedRenderer(ctx, sc, seeds=fx["seeds_in"], keep_acu=False)
        a.execute_passes(3, bounces=8, fresh=True)
        same_frame(a, b, "depth 8", acu=False)
        a.release()
        b.release()
    finally:
        ctx.set_exact_only(False)


@pytest.mark.gpu
def test_three_passes_match_the_oracle(ctx, pkg, loop):
    """as test_progressive_passes_match_oracle, with the three passes in one call"""
    from raytracing_amd.pyhost import render
    fx, sc = load_fixture("twoLights_32x24_r4")
    orc = A.load_oracle()
    for bounces in (5, 8):
        st = A.PassState(sc, fx["seeds_in"])
        for p in range(3):
            A.run_pass(orc, sc, st, bounces=bounces, init_acu=(p == 0))
        fr = render.FusedRenderer(ctx, sc, seeds=fx["seeds_in"])
        fr.execute_passes(3, bounces=bounces, fresh=True)
        assert np.array_equal(bits(fr.acu.read(np.float32).reshape(-1, 4)), bits(st.acu)), bounces
        assert np.array_equal(fr.pixel.read(np.uint8).reshape(-1, 4), st.pixel), bounces
        assert np.array_equal(fr.seeds.read(np.int32), st.seeds), bounces
        fr.release()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_32x24_r4", "cornell_teapot3_32x24_r4"])
def test_continuation(ctx, pkg, name):
    """2 ordinary passes, then 3 in one call from pass index 3: the 5-pass frame"""
    fx, sc = load_fixture(name)
    b = ordinary(ctx, sc, fx["seeds_in"], 5)
    a = ordinary(ctx, sc, fx["seeds_in"], 2)
    a.execute_passes(3)
    assert a.passes == 6
    same_frame(a, b, name)
    a.release()
    b.release()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_16x12_r9", "cornell_64x48_r1"])
def test_counts_that_need_the_accumulator(ctx, pkg, name, loop):
    """nine rays per pixel straddle blocks (the passes cannot resolve their pixels); one ray per pixel couples rows through seeds[col] (the call
    queues ordinary passes): with acu the results are the ordinary passes', without it MIRT_E_ARG naming the rule -- and the context works on"""
    from raytracing_amd.pyhost import mirt, render
    fx, sc = load_fixture(name)
    b = ordinary(ctx, sc, fx["seeds_in"], 3)
    a = render.FusedRenderer(ctx, sc, seeds=fx["seeds_in"], keep_acu=False)
    with pytest.raises(mirt.MirtError) as e:
        a.execute_passes(3, fresh=True)
    assert e.value.code == E_ARG and "acu" in str(e.value)
    a.release()
    a = render.FusedRenderer(ctx, sc, seeds=fx["seeds_in"])
    a.execute_passes(3, fresh=True)
    same_frame(a, b, name)
    a.release()
    b.release()


@pytest.mark.gpu
def test_argument_rules(ctx, pkg):
    from raytracing_amd.pyhost import mirt, render
    fx, sc = load_fixture("cornell_32x24_r4")
    fr = render.FusedRenderer(ctx, sc, seeds=fx["seeds_in"], keep_acu=False)
    d = fr.dev.pass_desc(fr.seeds, None, fr.pixel, fr.radiance)
    for n in (0, 65):
        with pytest.raises(mirt.MirtError) as e:
            ctx.render_passes(d, n, fresh=True)
        assert e.value.code == E_ARG, n
    with pytest.raises(mirt.MirtError) as e:    # not the frame's start: there is an accumulator to read
        ctx.render_passes(d, 2, fresh=False)
    assert e.value.code == E_ARG and "acu" in str(e.value)
    with pytest.raises(mirt.MirtError) as e:    # nowhere to put the frame
        ctx.render_passes(fr.dev.pass_desc(fr.seeds, None, None, None), 2, fresh=True)
    assert e.value.code == E_ARG
    assert np.array_equal(fr.seeds.read(np.int32), fx["seeds_in"]), "a refused call touched the seeds"
    fr.execute_passes(1, fresh=True)            # one pass in one call is the first pass (and the fixture's frame)
    assert np.array_equal(fr.pixel.read(np.uint8).reshape(-1, 4), fx["pixel"])
    assert np.array_equal(bits(fr.radiance.read(np.float32).reshape(-1, 4)), bits(fx["radiance"]))
    assert np.array_equal(fr.seeds.read(np.int32), fx["f_seeds"])
    fr.release()


@pytest.mark.gpu
@pytest.mark.parametrize("rpp,size", [(1024, (7, 5)), (4096, (3, 2))])
@pytest.mark.parametrize("name", ["cornell_32x24_r4", "cornell_teapot3_32x24_r4", "own_flat_32x24_r4"])
def test_pixels_of_more_than_256_rays(ctx, pkg, name, rpp, size, loop):
    """a pixel over 4 (16) blocks: launch c runs block c of every pixel through both passes and carries the radiance chain on; own_flat defers
    blocks to the exact kernel, which re-runs both passes of them"""
    from raytracing_amd.pyhost import render, scene
    fx, sc0 = load_fixture(name)
    ps = scene.PackedScene(dict(sc0.d)).resized(size[0], size[1], rpp)
    sc = A.Scene(ps.d)
    seeds = A.make_seeds(sc.total_rays, seed_base=rpp + size[0])
    b = ordinary(ctx, ps, seeds, 2)
    for want_radiance in (True, False):
        a = render.FusedRenderer(ctx, ps, seeds=seeds, keep_acu=False, want_radiance=want_radiance)
        a.execute_passes(2, fresh=True)
        deferred = ctx.pass_deferred()
        assert np.array_equal(a.pixel.read(np.uint8), b.pixel.read(np.uint8)), want_radiance
        assert np.array_equal(a.seeds.read(np.int32), b.seeds.read(np.int32)), want_radiance
        if want_radiance:
            assert np.array_equal(bits(a.radiance.read(np.float32)), bits(b.radiance.read(np.float32)))
        if name == "own_flat_32x24_r4":
            assert deferred > 0, "own_flat no longer defers: the exact kernel's re-run of both passes is not exercised"
        a.release()
    a = render.FusedRenderer(ctx, ps, seeds=seeds)
    a.execute_passes(2, fresh=True)
    same_frame(a, b, "with acu")
    a.release()
    b.release()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_teapot3_32x24_r4", "cornell_32x24_r4", "own_flat_32x24_r4"])
def test_row_tiles_with_partial_blocks(ctx, pkg, name, loop):
    from raytracing_amd.pyhost import render
    fx, sc = load_fixture(name)
    whole = ordinary(ctx, sc, fx["seeds_in"], 2)
    want_pix = whole.pixel.read(np.uint8).reshape(-1, 4)
    want_rad = bits(whole.radiance.read(np.float32).reshape(-1, 4))
    for row0, nrows in [(3, 7), (0, 1), (sc.height - 5, 5)]:
        fr = render.FusedRenderer(ctx, sc, seeds=fx["seeds_in"], row0=row0, nrows=nrows, keep_acu=False)
        guard = np.full(nrows * sc.width * 4 + 64, 0xAB, np.uint8)
        fr.pixel.release()
        fr.pixel = ctx.buffer(guard.size)
        fr.pixel.write(guard)
        fr.execute_passes(2, fresh=True)
        got = fr.pixel.read(np.uint8)
        lo, hi = row0 * sc.width, (row0 + nrows) * sc.width
        assert np.array_equal(got[:nrows * sc.width * 4].reshape(-1, 4), want_pix[lo:hi]), (name, row0, nrows)
        assert np.all(got[nrows * sc.width * 4:] == 0xAB), "wrote past the tile's last pixel"
        assert np.array_equal(bits(fr.radiance.read(np.float32).reshape(-1, 4)), want_rad[lo:hi])
        fr.release()
    whole.release()


@pytest.mark.gpu
def test_deferred_samples_rerun_all_passes_without_in_pass_resolve(ctx, pkg, loop):
    """the per-sample path: no in-pass resolve, so a sample that leaves the guard windows in any pass is re-run through all of them by the
    exact kernel, and the separate copyToPixel follows.  own_flat defers; at 9 rays per pixel (pixels straddle blocks), and at 4 on a context
    created with MIRT_INPASS_RESOLVE=0."""
    from raytracing_amd.pyhost import mirt, render, scene
    fx, sc0 = load_fixture("own_flat_32x24_r4")
    ps = scene.PackedScene(dict(sc0.d)).resized(32, 24, 9)
    seeds9 = A.make_seeds(ps.width * ps.height * 9, seed_base=9)
    os.environ["MIRT_INPASS_RESOLVE"] = "0"
    try:
        sep = mirt.Context(0)
    finally:
        del os.environ["MIRT_INPASS_RESOLVE"]
    try:
        for c, s, seeds, tag in ((ctx, ps, seeds9, "9 rays per pixel"), (sep, sc0, fx["seeds_in"], "MIRT_INPASS_RESOLVE=0")):
            b = ordinary(c, s, seeds, 3)
            a = render.FusedRenderer(c, s, seeds=seeds)
            a.acu.write(np.full(a.nrays * 4, np.nan, np.float32))
            a.execute_passes(3, fresh=True)
            deferred = c.pass_deferred()
            assert 0 < deferred < a.nrays, "own_flat no longer defers on the per-sample path: the exact kernel's re-run of all passes is not exercised"
            same_frame(a, b, f"own_flat, {tag}, {loop}")
            a.release()
            b.release()
    finally:
        sep.destroy()


DEFAULT_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
sys.path.insert(0, sys.argv[1] + "/oracle")
import __graft_entry__ as g
g.load_package()
from raytracing_amd.pyhost import mirt, render
from conftest import load_fixture
assert mirt.LIB_PATH.endswith("libmirt_default.so"), mirt.LIB_PATH
ctx = mirt.Context(0)
fx, sc = load_fixture("cornell_teapot3_32x24_r4")
b = render.FusedRenderer(ctx, sc, seeds=fx["seeds_in"])
for p in range(3):
    b.execute_render(fresh=(p == 0))
a = render.FusedRenderer(ctx, sc, seeds=fx["seeds_in"], keep_acu=False)
a.execute_passes(3, fresh=True)
ok = all(np.array_equal(x.read(np.uint8), y.read(np.uint8)) for x, y in ((a.pixel, b.pixel), (a.radiance, b.radiance), (a.seeds, b.seeds)))
print(json.dumps({"ok": bool(ok)}))
"""


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "2015-raytracing_amd", "libmirt_default.so")), reason="libmirt_default.so not built")
def test_default_contract_library(pkg):
    """libmirt_default.so (the reference's own build options) gets the feature from the same sources: its passes in one call equal its own
    ordinary passes (a process of its own: a process loads one libmirt)"""
    env = dict(os.environ, MIRT_CONTRACT="default")
    env.pop("MIRT_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-c", DEFAULT_CHILD, ROOT], env=env, capture_output=True, text=True, timeout=600)
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and lines and lines[-1]["ok"], r.stderr[-2000:]


@pytest.mark.gpu
@pytest.mark.skipif(node is None, reason="node is not installed")
@pytest.mark.parametrize("gpus", [None, 2])
def test_node_cli_passes_in_one_launch(tmp_path, gpus):
    """`cli.js render ... 3 --passes-in-one-launch --no-acu`: the frame and radiance of three passes without a per-ray accumulator, equal to the
    plain three-pass run; with --gpus 2 every row tile makes one call before the gather"""
    scene_file = os.path.join(PAGE, "scenes", "gems.xml")
    extra = ["--gpus", str(gpus)] if gpus else []
    env = dict(os.environ, MIRT_GROUP_ALLOW_REPEATED_DEVICES="1")
    outs = {}
    for tag, flags in (("plain", []), ("one", ["--passes-in-one-launch", "--no-acu"])):
        out = str(tmp_path / (tag + ".rgba"))
        r = subprocess.run([node, os.path.join(HOST, "cli.js"), "render", scene_file, "48", "36", "4", "3", out, *flags, *extra],
                           capture_output=True, env=env, timeout=600)
        assert r.returncode == 0, r.stderr.decode()
        outs[tag] = (open(out, "rb").read(), open(out + ".radiance.f32", "rb").read())
    assert outs["one"][0] == outs["plain"][0], "frame"
    assert outs["one"][1] == outs["plain"][1], "radiance"


@pytest.mark.gpu
@pytest.mark.skipif(node is None, reason="node is not installed")
def test_node_cli_more_passes_than_one_call_takes(tmp_path):
    """65 passes: with the accumulator kept the host splits them over calls of at most 64 (the frame of 65 ordinary passes); without it the
    CLI stops before rendering anything, naming the cap"""
    scene_file = os.path.join(PAGE, "scenes", "gems.xml")
    outs = {}
    for tag, flags in (("plain", []), ("one", ["--passes-in-one-launch"])):
        out = str(tmp_path / (tag + ".rgba"))
        r = subprocess.run([node, os.path.join(HOST, "cli.js"), "render", scene_file, "16", "12", "4", "65", out, *flags], capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr.decode()
        outs[tag] = (open(out, "rb").read(), open(out + ".radiance.f32", "rb").read())
    assert outs["one"] == outs["plain"]
    out = str(tmp_path / "noacu.rgba")
    r = subprocess.run([node, os.path.join(HOST, "cli.js"), "render", scene_file, "16", "12", "4", "65", out, "--passes-in-one-launch", "--no-acu"],
                       capture_output=True, timeout=600)
    assert r.returncode != 0 and b"at most 64" in r.stderr and not os.path.exists(out)
