"""The frame after every pass of one multi-pass call (mirt_render_passes with MIRT_PASSES_EVERY_FRAME; FusedRenderer.execute_passes(every_frame=True);
Node renderer.executePasses(n, bounces, {everyPass}); cli.js render ... --passes-in-one-launch --every-pass).

Frame p of the call is what pixel / radiance hold after the (p+1)-th call of the ordinary sequence (mirt_render_first_pass or mirt_render_pass at
pass_index, then mirt_render_pass at each later index), bit for bit, and seeds and acu end as that sequence leaves them.  Where the passes resolve in
the kernel every frame comes from the same launch(es) as the last-frame-only call; elsewhere the call queues ordinary passes, one frame slot each.
Everything is compared with tolerance 0 against ordinary passes of the same library, and one case against the CPU oracle."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import a10_pass as A
from conftest import HOST, ROOT, bits, load_fixture

E_ARG = -1   # MIRT_E_ARG (include/mirt.h)
SCENES = ["cornell_32x24_r4", "cornell_teapot3_32x24_r4", "own_gems_48x36_r4", "own_flat_32x24_r4"]
node = shutil.which("node")


def resized(name, rpp, size):
    from raytracing_amd.pyhost import scene
    fx, sc0 = load_fixture(name)
    ps = scene.PackedScene(dict(sc0.d)).resized(size[0], size[1], rpp)
    sc = A.Scene(ps.d)
    return ps, sc, A.make_seeds(sc.total_rays, seed_base=rpp + size[0])


@pytest.fixture(scope="module")
def ctx(pkg):
    from raytracing_amd.pyhost import mirt
    c = mirt.Context(0)
    yield c
    c.destroy()


@pytest.fixture(params=["reuse", "plain"])
def loop(request, monkeypatch):
    """both MULTI kernels: primary-hit reuse and the plain pass loop (MIRT_MULTIPASS_REUSE=1 / 0, read per launch)"""
    monkeypatch.setenv("MIRT_MULTIPASS_REUSE", "1" if request.param == "reuse" else "0")
    return request.param


def ordinary_frames(ctx, sc, seeds, n, first=0, **kw):
    """the baseline: `first` ordinary passes, then n more, into a kept accumulator; pixel and radiance after each of the n"""
    from raytracing_amd.pyhost import render
    fr = render.FusedRenderer(ctx, sc, seeds=seeds, **kw)
    for p in range(first):
        fr.execute_render(fresh=(p == 0))
    pix, rad = [], []
    for p in range(n):
        fr.execute_render(fresh=(first + p == 0))
        pix.append(fr.pixel.read(np.uint8).reshape(-1, 4))
        rad.append(bits(fr.radiance.read(np.float32).reshape(-1, 4)) if fr.radiance is not None else None)
    return fr, np.stack(pix), (np.stack(rad) if fr.radiance is not None else None)


def same_frames(a, frames, b, pix, rad, tag, acu):
    got_pix, got_rad = frames
    assert got_pix.shape == pix.shape and np.array_equal(got_pix, pix), tag + ": pixel frames"
    if rad is not None:
        assert np.array_equal(bits(got_rad), rad), tag + ": radiance frames"
        assert np.array_equal(bits(a.radiance.read(np.float32).reshape(-1, 4)), rad[-1]), tag + ": radiance buffer holds the last frame"
    assert np.array_equal(a.pixel.read(np.uint8).reshape(-1, 4), pix[-1]), tag + ": pixel buffer holds the last frame"
    assert np.array_equal(a.seeds.read(np.int32), b.seeds.read(np.int32)), tag + ": seeds"
    if acu:
        assert np.array_equal(bits(a.acu.read(np.float32)), bits(b.acu.read(np.float32))), tag + ": acu"


def test_flag_is_declared(pkg):
    """CPU: the header and the binding agree on the flag"""
    from raytracing_amd.pyhost import mirt
    text = open(os.path.join(ROOT, "include", "mirt.h")).read()
    assert "#define MIRT_PASSES_EVERY_FRAME 2u" in text
    assert mirt.PASSES_EVERY_FRAME == 2


@pytest.mark.gpu
@pytest.mark.parametrize("exact_only", [False, True], ids=["optimistic", "exact_only"])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("name", SCENES)
def test_frames_equal_ordinary_passes(ctx, pkg, name, n, exact_only, loop):
    """fresh and acu-free; then with acu kept, two ordinary passes and n more in one call from pass index 3"""
    from raytracing_amd.pyhost import render
    fx, sc = load_fixture(name)
    seeds = fx["seeds_in"]
    ctx.set_exact_only(exact_only)
    try:
        b, pix, rad = ordinary_frames(ctx, sc, seeds, n)
        a = render.FusedRenderer(ctx, sc, seeds=seeds, keep_acu=False)
        frames = a.execute_passes(n, fresh=True, every_frame=True)
        deferred = ctx.pass_deferred()
        same_frames(a, frames, b, pix, rad, f"{name} x{n}, no acu", acu=False)
        if name == "own_flat_32x24_r4" and not exact_only:
            assert deferred > 0, "own_flat no longer defers: the exact kernel's re-run of every frame is not exercised"
        a.release()
        b.release()
        b, pix, rad = ordinary_frames(ctx, sc, seeds, n, first=2)
        a = render.FusedRenderer(ctx, sc, seeds=seeds)
        for p in range(2):
            a.execute_render(fresh=(p == 0))
        frames = a.execute_passes(n, every_frame=True)
        same_frames(a, frames, b, pix, rad, f"{name} x{n}, acu continued", acu=True)
        a.release()
        b.release()
    finally:
        ctx.set_exact_only(False)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_teapot3_32x24_r4", "own_flat_32x24_r4"])
def test_row_tile_leaves_guard_bytes(ctx, pkg, name, loop):
    """a row tile's frames are the whole frame's rows; nothing is written after the last frame"""
    from raytracing_amd.pyhost import render
    fx, sc = load_fixture(name)
    n = 3
    whole, pix, rad = ordinary_frames(ctx, sc, fx["seeds_in"], n)
    for row0, nrows in [(3, 7), (sc.height - 5, 5)]:
        fr = render.FusedRenderer(ctx, sc, seeds=fx["seeds_in"], row0=row0, nrows=nrows, keep_acu=False)
        npx = nrows * sc.width
        fp = ctx.buffer(n * npx * 4 + 64)
        fp.write(np.full(n * npx * 4 + 64, 0xAB, np.uint8))
        frd = ctx.buffer(n * npx * 16 + 64)
        frd.write(np.full(n * npx * 4 + 16, np.float32(-3.5), np.float32))
        ctx.render_passes(fr.dev.pass_desc(fr.seeds, None, fp, frd, row0=row0, nrows=nrows), n, fresh=True, every_frame=True)
        got = fp.read(np.uint8)
        lo, hi = row0 * sc.width, (row0 + nrows) * sc.width
        assert np.array_equal(got[:n * npx * 4].reshape(n, npx, 4), pix[:, lo:hi]), (name, row0, nrows)
        assert np.all(got[n * npx * 4:] == 0xAB), "wrote past the last pixel frame"
        r = frd.read(np.float32)
        assert np.array_equal(bits(r[:n * npx * 4].reshape(n, npx, 4)), rad[:, lo:hi]), (name, row0, nrows)
        assert np.all(r[n * npx * 4:] == np.float32(-3.5)), "wrote past the last radiance frame"
        fp.release()
        frd.release()
        fr.release()
    whole.release()


COUNTS = [(64, (9, 7)), (256, (5, 4)), (289, (7, 5)), (1024, (7, 5))]


@pytest.mark.gpu
@pytest.mark.parametrize("rpp,size", COUNTS, ids=[str(r) for r, _ in COUNTS])
@pytest.mark.parametrize("name", ["cornell_32x24_r4", "own_flat_32x24_r4"])
def test_counts(ctx, pkg, name, rpp, size, loop):
    """64 and 256 in one segment; 289 and 1024 through the segment plan (the carry arrays alternate; own_flat defers segments), acu-free with and
    without a radiance buffer; then with acu kept (at 289 outside the counts that resolve beside acu: ordinary passes, one frame slot each)"""
    from raytracing_amd.pyhost import render
    ps, sc, seeds = resized(name, rpp, size)
    n = 3
    b, pix, rad = ordinary_frames(ctx, ps, seeds, n)
    for want_radiance in (True, False):
        a = render.FusedRenderer(ctx, ps, seeds=seeds, keep_acu=False, want_radiance=want_radiance)
        frames = a.execute_passes(n, fresh=True, every_frame=True)
        deferred = ctx.pass_deferred()
        same_frames(a, frames, b, pix, rad if want_radiance else None, f"{name} {rpp} radiance={want_radiance}", acu=False)
        if name == "own_flat_32x24_r4" and rpp > 256:
            assert deferred > 0, "own_flat no longer defers: the redo launches between the segments are not exercised"
        a.release()
    a = render.FusedRenderer(ctx, ps, seeds=seeds)
    a.acu.write(np.full(a.nrays * 4, np.nan, np.float32))
    frames = a.execute_passes(n, fresh=True, every_frame=True)
    same_frames(a, frames, b, pix, rad, f"{name} {rpp}, acu kept", acu=True)
    a.release()
    b.release()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_16x12_r9", "cornell_64x48_r1"])
def test_counts_through_ordinary_passes(ctx, pkg, name):
    """9 rays per pixel straddle blocks, 1 couples rows through seeds[col]: the call queues ordinary passes, each writing its frame slot"""
    from raytracing_amd.pyhost import render
    fx, sc = load_fixture(name)
    b, pix, rad = ordinary_frames(ctx, sc, fx["seeds_in"], 3)
    a = render.FusedRenderer(ctx, sc, seeds=fx["seeds_in"])
    a.acu.write(np.full(a.nrays * 4, np.nan, np.float32))
    frames = a.execute_passes(3, fresh=True, every_frame=True)
    same_frames(a, frames, b, pix, rad, name, acu=True)
    a.release()
    b.release()


@pytest.mark.gpu
def test_without_in_pass_resolve(pkg):
    """a context made with MIRT_INPASS_RESOLVE=0: ordinary passes and the separate copyToPixel into each frame slot"""
    from raytracing_amd.pyhost import mirt, render
    os.environ["MIRT_INPASS_RESOLVE"] = "0"
    try:
        sep = mirt.Context(0)
    finally:
        del os.environ["MIRT_INPASS_RESOLVE"]
    try:
        fx, sc = load_fixture("own_flat_32x24_r4")
        b, pix, rad = ordinary_frames(sep, sc, fx["seeds_in"], 3)
        a = render.FusedRenderer(sep, sc, seeds=fx["seeds_in"])
        frames = a.execute_passes(3, fresh=True, every_frame=True)
        same_frames(a, frames, b, pix, rad, "MIRT_INPASS_RESOLVE=0", acu=True)
        a.release()
        b.release()
    finally:
        sep.destroy()


@pytest.mark.gpu
def test_frames_match_the_oracle(ctx, pkg):
    """every frame against the CPU oracle's frame after that pass"""
    from raytracing_amd.pyhost import render
    fx, sc = load_fixture("twoLights_32x24_r4")
    orc = A.load_oracle()
    st = A.PassState(sc, fx["seeds_in"])
    want = []
    for p in range(3):
        A.run_pass(orc, sc, st, init_acu=(p == 0))
        want.append(st.pixel.copy())
    fr = render.FusedRenderer(ctx, sc, seeds=fx["seeds_in"], keep_acu=False)
    pix, _ = fr.execute_passes(3, fresh=True, every_frame=True)
    for p in range(3):
        assert np.array_equal(pix[p], want[p]), p
    assert np.array_equal(fr.seeds.read(np.int32), st.seeds)
    fr.release()


@pytest.mark.gpu
def test_refusals(ctx, pkg):
    """frame buffers too small for n, no frame buffer at all, an unknown flag bit, acu NULL at 9 rays: MIRT_E_ARG, nothing written"""
    from raytracing_amd.pyhost import mirt, render
    fx, sc = load_fixture("cornell_32x24_r4")
    fr = render.FusedRenderer(ctx, sc, seeds=fx["seeds_in"], keep_acu=False)
    npx = fr.npix
    small = ctx.buffer(2 * npx * 4)
    small.write(np.full(2 * npx * 4, 0x5A, np.uint8))
    rad3, rad2, pix3 = ctx.buffer(3 * npx * 16), ctx.buffer(2 * npx * 16), ctx.buffer(3 * npx * 4)
    for pixel, radiance in ((small, rad3), (pix3, rad2), (small, None), (None, rad2)):
        with pytest.raises(mirt.MirtError) as e:
            ctx.render_passes(fr.dev.pass_desc(fr.seeds, None, pixel, radiance), 3, fresh=True, every_frame=True)
        assert e.value.code == E_ARG, (pixel, radiance)
    with pytest.raises(mirt.MirtError) as e:
        ctx.render_passes(fr.dev.pass_desc(fr.seeds, None, None, None), 2, fresh=True, every_frame=True)
    assert e.value.code == E_ARG
    d = fr.dev.pass_desc(fr.seeds, None, pix3, rad3)
    assert mirt.lib().mirt_render_passes(ctx.h, C.byref(d), 2, mirt.PASSES_FRESH | 4) == E_ARG   # unknown flag bits stay refused
    assert np.array_equal(fr.seeds.read(np.int32), fx["seeds_in"]), "a refused call touched the seeds"
    assert np.all(small.read(np.uint8) == 0x5A), "a refused call wrote a frame"
    for b in (small, rad3, rad2, pix3):
        b.release()
    fr.release()
    fx9, sc9 = load_fixture("cornell_16x12_r9")
    fr = render.FusedRenderer(ctx, sc9, seeds=fx9["seeds_in"], keep_acu=False)
    with pytest.raises(mirt.MirtError) as e:
        fr.execute_passes(2, fresh=True, every_frame=True)
    assert e.value.code == E_ARG and "acu" in str(e.value)
    fr.release()


@pytest.mark.gpu
@pytest.mark.skipif(node is None, reason="node is not installed")
def test_node_cli_every_pass(tmp_path, ref_data):
    """`cli.js render cornell.xml 48 36 4 3 out --passes-in-one-launch --no-acu --every-pass` writes three frames, each equal to `cli.js render`
    with passes = 1, 2, 3; with --gpus 2 the CLI refuses --every-pass before rendering"""
    scene_file = os.path.join(ref_data, "a10", "scenes", "cornell.xml")
    cli = os.path.join(HOST, "cli.js")
    out = str(tmp_path / "every.rgba")
    r = subprocess.run([node, cli, "render", scene_file, "48", "36", "4", "3", out, "--passes-in-one-launch", "--no-acu", "--every-pass"],
                       capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    for k in (1, 2, 3):
        ref = str(tmp_path / f"plain{k}.rgba")
        r = subprocess.run([node, cli, "render", scene_file, "48", "36", "4", str(k), ref], capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr.decode()
        f = str(tmp_path / f"every.pass{k}.rgba")
        assert open(f, "rb").read() == open(ref, "rb").read(), k
        assert open(f + ".radiance.f32", "rb").read() == open(ref + ".radiance.f32", "rb").read(), k
    assert open(out, "rb").read() == open(str(tmp_path / "plain3.rgba"), "rb").read()
    env = dict(os.environ, MIRT_GROUP_ALLOW_REPEATED_DEVICES="1")
    bad = str(tmp_path / "gpus.rgba")
    r = subprocess.run([node, cli, "render", scene_file, "48", "36", "4", "3", bad, "--passes-in-one-launch", "--no-acu", "--every-pass", "--gpus", "2"],
                       capture_output=True, env=env, timeout=600)
    assert r.returncode != 0 and b"--every-pass" in r.stderr and not os.path.exists(bad)
