"""GPU: an Assign04 / Assign07 frame in ONE launch (mirt_render_frame, pt_kernels_frame.hip k_frame_fused) and the command-stream fusion of the
frame dialects (mirt_ctx_set_frame_fusion).  Every comparison is bit for bit: against the fixtures (the reference's own host + compiled code.cl),
against the kernel-by-kernel path on the same context (initTrace, then molTrace and / or meshTrace -- each pinned to the reference binaries by
tests/test_frames.py), and between fusion on and off."""
import ctypes as C
import glob
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import a10_pass as A
from conftest import GOLDEN, HOST, PAGE, ROOT, bits
from test_frames import fixture, resized

CASES = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, "frame_a0[47]_*.npz")))
FULL = [("frame_a04_parliament_96x64", (1024, 1024)), ("frame_a04_teapot_160x120", (1024, 1024)),            # test_full_size_frames_equal_the_reference_binaries'
        ("frame_a07_parliament_n16_160x120", (1920, 1080)), ("frame_a07_teapot_n2_160x120", (1920, 1080)),   # sizes (Assign01 is one launch already)
        ("frame_a07_mol_3IZ4_n16_96x64", (1920, 1080)), ("frame_a07_mol_c60_n4_160x120", (1920, 1080)),
        ("frame_a07_own_terrain_n5_96x64", (1920, 1080)),
        ("frame_a04_house_160x120", (1024, 1024)), ("frame_a07_house_n2_160x120", (1920, 1080)), ("frame_a07_house_n8_160x120", (1920, 1080))]
STREAM_CASES = ["frame_a04_own_icosphere_96x64", "frame_a07_own_terrain_n5_96x64", "frame_a07_teapot_n2_160x120", "frame_a07_own_mol_lattice_n6_96x64"]
SENTINEL = 0xA5
E_ARG, E_RANGE = -1, -5
node = shutil.which("node")
CHILD = os.path.join(ROOT, "tests", "frame_one_launch_child.py")
PROFILE_DIR = os.path.join(ROOT, "profiles", "frame_one_launch")


def test_the_new_entry_points_exist(pkg):
    """CPU: new symbols only, the ABI version stays.  (mirt_render_frame and mirt_ctx_set_frame_fusion do not exist before this feature.)"""
    from raytracing_amd.pyhost import mirt
    lib = mirt.lib()
    for name in ("mirt_render_frame", "mirt_ctx_set_frame_fusion", "mirt_ctx_fused_frames"):
        assert hasattr(lib, name), name
    assert lib.mirt_abi_version() == 4
    header = open(os.path.join(ROOT, "include", "mirt.h")).read()
    assert "#define MIRT_ABI_VERSION 4" in header and "mirt_frame_desc" in header
    assert C.sizeof(mirt._FrameDesc) == 4 * 4 + 64 + 32 + 2 * 4 + 7 * 8 + 2 * 4 + 4 * 8


@pytest.fixture(scope="module")
def ctx(pkg):
    from raytracing_amd.pyhost import mirt
    c = mirt.Context(0)
    yield c
    c.destroy()


@pytest.fixture(scope="module")
def fctx(pkg):
    """a context with frame fusion on"""
    from raytracing_amd.pyhost import mirt
    c = mirt.Context(0)
    c.set_frame_fusion(True)
    yield c
    c.destroy()


def rays40(raw):
    """the 40 bytes per ray the kernels write (o + pad, d + pad, mint, maxt), and the 8 they never touch"""
    r = np.ascontiguousarray(raw).reshape(-1, 48)
    return r[:, :40], r[:, 40:]


def packed(d):
    from raytracing_amd.pyhost import render
    return render.FramePacked(d)


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_one_launch_frame_equals_the_fixture(ctx, name):
    from raytracing_amd.pyhost import render
    fx, d = fixture(name)
    p = packed(d)
    px, none = render.render_frame_one_launch(ctx, p)
    assert none is None and np.array_equal(px, fx["pixel"])
    px2, rays = render.render_frame_one_launch(ctx, p, keep_rays=True)
    assert np.array_equal(px2, fx["pixel"])
    r = rays.view(A.RAY_DT)
    assert np.array_equal(bits(r["maxt"]), bits(fx["rays_maxt"])) and np.array_equal(bits(r["mint"]), bits(fx["rays_mint"]))
    _, want = render.render_frame_stream(ctx, p, rays_fill=0)
    assert np.array_equal(rays40(rays)[0], rays40(want)[0]), "the 40 written bytes of every ray equal the two launches'"


# ---- full size ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,size", FULL)
def test_full_size_one_launch_equals_two_launches(ctx, name, size):
    from raytracing_amd.pyhost import render
    _, d = fixture(name)
    p = packed(resized(d, *size))
    want_px, want_rays = render.render_frame_stream(ctx, p, rays_fill=0)
    px, rays = render.render_frame_one_launch(ctx, p, keep_rays=True)
    assert np.array_equal(px, want_px)
    assert np.array_equal(rays.view(A.RAY_DT)["maxt"].view(np.uint32), want_rays.view(A.RAY_DT)["maxt"].view(np.uint32))
    assert np.array_equal(rays40(rays)[0], rays40(want_rays)[0])
    px0, _ = render.render_frame_one_launch(ctx, p)
    assert np.array_equal(px0, want_px) and (px[:, :3].max(axis=1) > 0).mean() > 0.02


# ---- no ray buffer ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_without_a_ray_buffer_nothing_per_ray_is_written(ctx):
    from raytracing_amd.pyhost import render
    fx, d = fixture("frame_a07_house_n8_160x120")
    p = packed(d)
    spare = ctx.buffer(p.width * p.height * 48)
    spare.write(np.full(p.width * p.height * 48, SENTINEL, np.uint8))
    px, _ = render.render_frame_one_launch(ctx, p)
    assert np.array_equal(px, fx["pixel"]) and (spare.read(np.uint8) == SENTINEL).all()
    spare.release()
    f = render.FrameOneLaunch(ctx, p, keep_rays=True)   # and with one: 40 bytes per ray, the 8 of padding keep what they held
    f.rays.write(np.full(p.width * p.height * 48, SENTINEL, np.uint8))
    f.render()
    assert (rays40(f.rays.read(np.uint8))[1] == SENTINEL).all()
    f.release()


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("rocprofv3") is None, reason="rocprofv3 is not installed")
def test_a_kernel_trace_shows_one_kernel_per_frame(tmp_path):
    """rocprofv3 --kernel-trace --stats over a process of its own that renders five frames and nothing else"""
    out = str(tmp_path / "trace")
    r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, CHILD, "frames", "frame_a07_house_n8_160x120", "5"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    stats = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    assert stats, os.listdir(out)
    import csv
    rows = list(csv.DictReader(open(stats[0])))
    calls = {row["Name"]: int(row["Calls"]) for row in rows}
    print(calls)
    fused = {k: v for k, v in calls.items() if "k_frame_fused" in k}
    assert sum(fused.values()) == 5 and len(fused) == 1
    assert not [k for k in calls if "initTrace" in k or "k_a07_meshTrace" in k or "k_a07_molTrace" in k]
    if os.environ.get("MIRT_KEEP_PROFILE"):   # a path: how profiles/frame_one_launch/kernel_stats.csv was recorded
        shutil.copy(stats[0], os.environ["MIRT_KEEP_PROFILE"])


# ---- both models ------------------------------------------------------------------------------------------------------------------------------
def both_job(ctx, mesh_name, mol_name, where=(0.5, 0.5, 0.5), size=0.6):
    """A both-models job from a mesh fixture and a molecule fixture: the mesh job as it is, and the molecule's atoms scaled to `size` of the mesh's box,
    centred at the fraction `where` of it (clamped so that every atom stays inside) and binned there on the device (mirt_grid_build + gather = splitMolData) with the mesh's n_slabs -- one box, one camera, two packings."""
    _, dm = fixture(mesh_name)
    _, ds = fixture(mol_name)
    atoms = np.unique(np.asarray(ds["atoms"], np.float64).reshape(-1, 4), axis=0)
    b = np.asarray(dm["bounds"], np.float64)
    lo, hi = b[:3], b[4:7]
    c, r = atoms[:, :3], np.sqrt(atoms[:, 3])
    span = (c.max(axis=0) + r.max()) - (c.min(axis=0) - r.max())
    k = size * float(np.min((hi - lo) / span))
    half = span * k / 2
    c = (c - (c.max(axis=0) + c.min(axis=0)) / 2) * k + np.clip(lo + np.asarray(where) * (hi - lo), lo + half, hi - half)
    sph = np.concatenate([c, (r * k)[:, None]], axis=1)
    n = int(dm["n_slabs"])
    off, order, total = ctx.grid_build(0, sph, [lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]], n)
    slots = ctx.grid_gather_spheres(order, total, sph)
    mol = dict(s_size=len(sph), atoms=slots.read(np.float32, total * 4).tolist(), mindex=[0] * total, mcolor=[1.0, 1.0, 1.0, 1.0], slab_size=off.read(np.uint32).tolist())
    for buf in (off, order, slots):
        buf.release()
    return dict(dm, mol=mol)


@pytest.mark.gpu
@pytest.mark.parametrize("mesh_name,mol_name", [("frame_a07_teapot_n8_160x120", "frame_a07_mol_dna_n8_160x120"),
                                                ("frame_a07_own_octahedra_n3_96x64", "frame_a07_own_mol_helix_n3_96x64")])
def test_both_models_equal_the_three_kernel_stream(ctx, mesh_name, mol_name):
    """Molecule then mesh on the same ray (the page's computeBoth), against initTrace, molTrace, meshTrace enqueued one by one on this runtime: pixels,
    every ray's maxt, all 40 written bytes.  There is no reference fixture for this mode (generating one means touching oracle/); the three kernels it is
    compared against are each pinned to the reference binaries already (tests/test_frames.py test_full_size_frames_equal_the_reference_binaries)."""
    from raytracing_amd.pyhost import render
    only = lambda d: render.render_frame_one_launch(ctx, packed(d))[0]   # noqa: E731
    for where in ((0.5, 0.5, 0.5), (0.1, 0.9, 0.5), (0.9, 0.9, 0.5), (0.1, 0.1, 0.5), (0.5, 0.9, 0.9)):   # the first placement where both models show
        d = resized(both_job(ctx, mesh_name, mol_name, where, 0.35), 640, 400)
        mesh_only = only({k: v for k, v in d.items() if k != "mol"})
        mol_only = only(dict({k: v for k, v in d.items() if k not in ("mol", "pos", "normal", "t_size")}, **d["mol"]))
        lit_a, lit_b = mesh_only[:, :3].max(axis=1) > 0, mol_only[:, :3].max(axis=1) > 0
        if (lit_a & ~lit_b).any() and (lit_b & ~lit_a).any() and (lit_a & lit_b).any():
            break
    else:
        pytest.fail("no placement shows both models")
    p = packed(d)
    assert p.both is not None and not p.mol
    want_px, want_rays = render.render_frame_stream(ctx, p, rays_fill=0)
    px, rays = render.render_frame_one_launch(ctx, p, keep_rays=True)
    assert np.array_equal(px, want_px)
    assert np.array_equal(rays.view(A.RAY_DT)["maxt"].view(np.uint32), want_rays.view(A.RAY_DT)["maxt"].view(np.uint32))
    assert np.array_equal(rays40(rays)[0], rays40(want_rays)[0])
    px0, _ = render.render_frame_one_launch(ctx, p)
    assert np.array_equal(px0, want_px)
    assert (px != mesh_only).any() and (px != mol_only).any()   # both stages show in the frame


# ---- fusion on / off --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", STREAM_CASES)
def test_the_mirrors_stream_is_fused_when_asked(ctx, fctx, name):
    from raytracing_amd.pyhost import render
    fx, d = fixture(name)
    p = packed(d)
    n0 = fctx.fused_frames()
    px, _ = render.render_frame(fctx, p)   # the Python mirror of the pages' frame, unmodified
    assert np.array_equal(px, fx["pixel"]) and fctx.fused_frames() == n0 + 1
    px_on, rays_on = render.render_frame_stream(fctx, p, rays_fill=SENTINEL)
    assert np.array_equal(px_on, fx["pixel"]) and fctx.fused_frames() == n0 + 2
    assert (rays_on == SENTINEL).all(), "a fused frame does not write the ray buffer"
    # default: off -- the same stream writes the rays as ever, nothing is counted
    px_off, rays_off = render.render_frame_stream(ctx, p, rays_fill=SENTINEL)
    assert np.array_equal(px_off, fx["pixel"]) and ctx.fused_frames() == 0
    r = rays_off.view(A.RAY_DT)
    assert np.array_equal(bits(r["maxt"]), bits(fx["rays_maxt"])) and (rays40(rays_off)[1] == SENTINEL).all()


@pytest.mark.gpu
def test_the_both_models_stream_is_fused_when_asked(ctx, fctx):
    from raytracing_amd.pyhost import render
    p = packed(both_job(ctx, "frame_a07_own_octahedra_n3_96x64", "frame_a07_own_mol_helix_n3_96x64"))
    n0 = fctx.fused_frames()
    px_off, _ = render.render_frame_stream(ctx, p, rays_fill=SENTINEL)
    px_on, rays_on = render.render_frame_stream(fctx, p, rays_fill=SENTINEL)
    assert np.array_equal(px_on, px_off) and fctx.fused_frames() == n0 + 1 and (rays_on == SENTINEL).all() and ctx.fused_frames() == 0


def test_the_environment_switch(pkg):
    """MIRT_FRAME_FUSION=1 is read by mirt_ctx_create: checked on the GPU through frame.js below; here only that the header documents it"""
    assert "MIRT_FRAME_FUSION=1" in open(os.path.join(ROOT, "include", "mirt.h")).read()


def issue(c, p, mutant):
    """The both-models stream, or one of the streams the recogniser refuses, issued for real.  Returns every buffer it could have written."""
    from raytracing_amd.pyhost import mirt
    w, h = p.width, p.height
    g, l = [-(-w // 8) * 8, -(-h // 8) * 8], [8, 8]
    u32 = lambda v: np.array([v], np.uint32)   # noqa: E731
    bufs = {k: c.buffer(w * h * n) for k, n in (("pixels", 4), ("pixels2", 4), ("rays", 48), ("rays2", 48))}
    for k, b in bufs.items():
        b.write(np.full(b.nbytes, SENTINEL, np.uint8))
    acu = c.buffer(64 * 16)
    geo = [c.buffer_from(a) for a in (p.both["atoms"], p.both["mindex"], p.both["mcolor"], p.both["slab_size"], p.pos, p.normal, p.mindex, p.mcolor, p.slab_size)]
    cam2 = p.cam.copy()
    cam2[0] += 0.25
    pick = lambda what, stage, a, b: b if mutant == (what, stage) else a   # noqa: E731
    it = c.kernel("A07:initTrace").set_args(bufs["pixels"], p.cam, bufs["rays"], p.bounds)
    mol = c.kernel("A07:molTrace").set_args(pick("pixels", 1, bufs["pixels"], bufs["pixels2"]), pick("cam", 1, p.cam, cam2), pick("rays", 1, bufs["rays"], bufs["rays2"]),
                                            u32(p.both["s_size"]), geo[0], geo[1], geo[2], p.bounds, u32(p.n_slabs), geo[3])
    mesh = c.kernel("A07:meshTrace").set_args(pick("pixels", 2, bufs["pixels"], bufs["pixels2"]), pick("cam", 2, p.cam, cam2), pick("rays", 2, bufs["rays"], bufs["rays2"]),
                                              u32(p.t_size), geo[4], geo[5], geo[6], geo[7], p.bounds, u32(p.n_slabs), geo[8])
    ia = c.kernel("initAcu").set_args(acu, u32(64))
    small = [g[0] - 16, g[1] - 8]
    order = {"mesh before molecule": [(it, g), (mesh, g), (mol, g)],
             "a second initTrace": [(it, g), (mol, g), (it, g), (mesh, g)],
             "an Assign10 kernel in between": [(it, g), (mol, g), (ia, [64]), (mesh, g)],
             ("global", 1): [(it, g), (mol, small), (mesh, g)], ("global", 2): [(it, g), (mol, g), (mesh, small)]}.get(mutant, [(it, g), (mol, g), (mesh, g)])
    for k, gws in order:
        k.enqueue(gws, l if len(gws) == 2 else [64])
    c.finish()
    out = {k: b.read(np.uint8) for k, b in bufs.items()}
    for k in (it, mol, mesh, ia):
        k.release()
    for b in list(bufs.values()) + geo + [acu]:
        b.release()
    return out


MUTANTS = [("pixels", 1), ("pixels", 2), ("rays", 1), ("rays", 2), ("cam", 1), ("cam", 2), "mesh before molecule", "a second initTrace", ("global", 1), ("global", 2),
           "an Assign10 kernel in between"]


@pytest.mark.gpu
@pytest.mark.parametrize("mutant", MUTANTS, ids=[m if isinstance(m, str) else f"{m[0]} differs in stage {m[1]}" for m in MUTANTS])
def test_rejected_streams_run_as_issued(ctx, fctx, mutant):
    p = packed(resized(both_job(ctx, "frame_a07_own_octahedra_n3_96x64", "frame_a07_own_mol_helix_n3_96x64"), 200, 120))
    n0 = fctx.fused_frames()
    off, on = issue(ctx, p, mutant), issue(fctx, p, mutant)
    assert fctx.fused_frames() == n0, "a refused stream is not counted"
    for k in off:
        assert np.array_equal(on[k], off[k]), k
    assert (off["rays"] != SENTINEL).any() and (off["pixels"] != SENTINEL).any()


@pytest.mark.gpu
def test_the_well_formed_stream_of_the_mutants_is_fused(ctx, fctx):
    """the control of test_rejected_streams_run_as_issued: the same helper, no mutation"""
    p = packed(resized(both_job(ctx, "frame_a07_own_octahedra_n3_96x64", "frame_a07_own_mol_helix_n3_96x64"), 200, 120))
    n0 = fctx.fused_frames()
    off, on = issue(ctx, p, None), issue(fctx, p, None)
    assert fctx.fused_frames() == n0 + 1 and np.array_equal(on["pixels"], off["pixels"]) and (on["rays"] == SENTINEL).all()
    assert (on["pixels2"] == SENTINEL).all() and (on["rays2"] == SENTINEL).all()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_write_nothing(ctx):
    from raytracing_amd.pyhost import mirt, render
    _, d = fixture("frame_a07_house_n8_160x120")
    p = packed(d)
    f = render.FrameOneLaunch(ctx, p, keep_rays=True)
    for b in (f.pixels, f.rays):
        b.write(np.full(b.nbytes, SENTINEL, np.uint8))
    small = ctx.buffer(p.width * p.height * 4 - 4)
    small.write(np.full(small.nbytes, SENTINEL, np.uint8))
    short = ctx.buffer_from(p.slab_size[:-1])   # n^3 entries: one short of n^3 + 1
    args = dict(bounds=p.bounds, n_slabs=p.n_slabs, mesh=f.mesh, rays=f.rays)

    def refused(code, assign=7, pixel=f.pixels, **kw):
        with pytest.raises(mirt.MirtError) as e:
            ctx.render_frame(assign, p.width, p.height, p.cam, pixel, **dict(args, **kw))
        assert e.value.code == code, str(e.value)
    refused(E_RANGE, pixel=small)
    refused(E_RANGE, mesh=dict(f.mesh, slab_size=short))
    refused(E_RANGE, rays=small)
    refused(E_ARG, assign=1)
    refused(E_ARG, assign=10)
    refused(E_ARG, mesh=None)
    refused(E_ARG, assign=4, mesh=None, mol=dict(s_size=1, atoms=f.mesh["pos"], slab_size=f.mesh["slab_size"]))
    ctx.finish()
    for b in (f.pixels, f.rays, small):
        assert (b.read(np.uint8) == SENTINEL).all()
    f.render()   # and the same descriptor, whole, renders
    assert (f.pixels.read(np.uint8) != SENTINEL).any()
    small.release(); short.release(); f.release()


@pytest.mark.gpu
def test_a_frame_can_be_recorded(ctx):
    """inside mirt_capture_begin / _end under mirt_render_pass's rule: after one ordinary run the call records, and the replay renders the frame"""
    from raytracing_amd.pyhost import render
    fx, d = fixture("frame_a07_own_terrain_n5_96x64")
    f = render.FrameOneLaunch(ctx, packed(d))
    f.render()
    ctx.finish()
    ctx.capture_begin()
    f.render()
    g = ctx.capture_end()
    f.pixels.write(np.zeros(f.pixels.nbytes, np.uint8))
    ctx.graph_launch(g)
    ctx.finish()
    assert np.array_equal(f.pixels.read(np.uint8).reshape(-1, 4), fx["pixel"])
    ctx.graph_release(g)
    f.release()


# ---- the default contract ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.skipif(not (os.path.exists(os.path.join(ROOT, "oracle", "_ref", "a07_gfx950_default.hsaco")) and os.path.exists(os.path.join(ROOT, "2015-raytracing_amd", "libmirt_default.so"))),
                    reason="needs the default builds of Assign04 / 07 (make -C oracle ref_gpu) and libmirt_default.so")
def test_one_launch_frames_equal_the_default_builds_of_the_reference():
    """libmirt_default.so in a process of its own (a process loads one libmirt): every Assign04 / Assign07 fixture job through mirt_render_frame against
    the reference's code.cl built with its own defaults, on the device: every pixel and every ray's maxt"""
    env = dict(os.environ, MIRT_CONTRACT="default")
    env.pop("MIRT_LIB_PATH", None)
    r = subprocess.run([sys.executable, CHILD, "default"], env=env, capture_output=True, text=True, timeout=900)
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0, (lines[-1:] or r.stderr[-2000:])
    assert len(lines) == len(CASES) and all(l["ok"] for l in lines)


# ---- Node -------------------------------------------------------------------------------------------------------------------------------------
def cli(args, env=None):
    r = subprocess.run([node, os.path.join(HOST, "cli.js")] + [str(a) for a in args], capture_output=True, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr.decode()
    return r


OWN = [("tri/terrain.json", 5), ("tri/octahedra.json", 3), ("mol/helix.pdb", 3), ("mol/lattice.pdb", 6)]


@pytest.mark.gpu
@pytest.mark.skipif(node is None, reason="node is not installed")
@pytest.mark.parametrize("model,n", OWN)
def test_node_one_launch_writes_the_same_file(tmp_path, model, n):
    a, b, c = (str(tmp_path / f) for f in ("two.rgba", "one.rgba", "fused.rgba"))
    two = cli(["frame", 7, os.path.join(PAGE, model), 200, 120, n, a])
    one = cli(["frame", 7, os.path.join(PAGE, model), 200, 120, n, b, "--one-launch"])
    fused = cli(["frame", 7, os.path.join(PAGE, model), 200, 120, n, c], env={"MIRT_FRAME_FUSION": "1"})   # frame.js, unmodified stream, fused by the runtime
    want = np.fromfile(a, np.uint8)
    assert np.array_equal(np.fromfile(b, np.uint8), want) and np.array_equal(np.fromfile(c, np.uint8), want) and (want.reshape(-1, 4)[:, :3] > 0).any()
    assert b"fused from enqueues: 0" in two.stderr and b"fused from enqueues: 0" in one.stderr and b"fused from enqueues: 1" in fused.stderr


@pytest.mark.gpu
@pytest.mark.skipif(node is None, reason="node is not installed")
def test_node_assign04_one_launch_writes_the_same_file(tmp_path):
    a, b = str(tmp_path / "two.rgba"), str(tmp_path / "one.rgba")
    cli(["frame", 4, os.path.join(PAGE, "tri", "icosphere.json"), 200, 120, 0, a])
    cli(["frame", 4, os.path.join(PAGE, "tri", "icosphere.json"), 200, 120, 0, b, "--one-launch"])
    assert np.array_equal(np.fromfile(a, np.uint8), np.fromfile(b, np.uint8))


@pytest.mark.gpu
@pytest.mark.skipif(node is None, reason="node is not installed")
def test_node_both_models_equal_the_python_result(ctx, tmp_path):
    from raytracing_amd.pyhost import render
    mesh, mol = os.path.join(PAGE, "tri", "octahedra.json"), os.path.join(PAGE, "mol", "helix.pdb")
    job = json.loads(cli(["pack-frame", 7, mesh, mol, 200, 120, 3]).stdout)
    p = packed(job)
    assert p.both is not None
    want, _ = render.render_frame_stream(ctx, p)
    px, _ = render.render_frame_one_launch(ctx, p)
    assert np.array_equal(px, want)
    a, b, c = (str(tmp_path / f) for f in ("two.rgba", "one.rgba", "fused.rgba"))
    cli(["frame", 7, mesh, mol, 200, 120, 3, a])
    cli(["frame", 7, mesh, mol, 200, 120, 3, b, "--one-launch"])
    fused = cli(["frame", 7, mesh, mol, 200, 120, 3, c], env={"MIRT_FRAME_FUSION": "1"})
    for f in (a, b, c):
        assert np.array_equal(np.fromfile(f, np.uint8).reshape(-1, 4), want), f
    assert b"fused from enqueues: 1" in fused.stderr
    mesh_only, _ = render.render_frame_one_launch(ctx, packed({k: v for k, v in job.items() if k != "mol"}))
    assert (want != mesh_only).any() and (want[:, :3] > 0).any()
