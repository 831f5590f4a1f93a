"""The anti-aliased Assign04 / Assign07 frame: aa x aa samples a pixel in ONE launch (mirt_render_frame_aa, pt_kernels_frame.hip k_frame_aa_pixel /
k_frame_aa_lanes).  The frame is DEFINED as the integer box average of a fine frame mirt_render_frame already renders (include/mirt.h), so every GPU
comparison here is bit for bit: against the reference's own fixtures (each IS a fine frame), against this library's fine frames, against the CPU
oracle's.  tests/frame_aa_common.py restates the definition in numpy."""
import ctypes as C
import glob
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import frame_pass as F
from conftest import GOLDEN, HOST, PAGE, ROOT
from frame_aa_common import AAS, SIZES, box, coarse_job, coverage, fine_job
from test_frame_one_launch import both_job, rays40
from test_frames import fixture, resized

CASES = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, "frame_a0[47]_*.npz")))
JOBS = ["frame_a04_own_icosphere_96x64", "frame_a07_own_terrain_n5_96x64", "frame_a07_teapot_n2_160x120", "frame_a07_own_mol_lattice_n6_96x64", "both"]
SENTINEL = 0xA5
TAIL = 256
E_ARG, E_HANDLE, E_RANGE = -1, -2, -5
node = shutil.which("node")
ADDON = os.path.join(ROOT, "2015-raytracing_amd", "mirt.node")
CHILD = os.path.join(ROOT, "tests", "frame_aa_child.py")
TIMING = os.path.join(ROOT, "profiles", "frame_aa", "timing.json")


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------------
def test_the_new_entry_point_exists(pkg):
    from raytracing_amd.pyhost import mirt
    lib = mirt.lib()
    assert hasattr(lib, "mirt_render_frame_aa") and "mirt_render_frame_aa" in mirt.SYMBOLS
    assert lib.mirt_abi_version() == 4
    header = open(os.path.join(ROOT, "include", "mirt.h")).read()
    assert "#define MIRT_ABI_VERSION 4" in header
    assert "MIRT_API int mirt_render_frame_aa(mirt_ctx* ctx, const mirt_frame_desc* desc, uint32_t aa);" in header
    assert C.sizeof(mirt._FrameDesc) == 4 * 4 + 64 + 32 + 2 * 4 + 7 * 8 + 2 * 4 + 4 * 8


def test_box_of_one_sample_is_the_identity():
    px = np.random.default_rng(1).integers(0, 256, (7 * 5, 4), dtype=np.uint8)
    px[:, 3] = 255
    assert np.array_equal(box(px, 7, 5, 1), px)


@pytest.mark.parametrize("aa", AAS)
def test_box_of_a_constant_block_is_that_colour(aa):
    colours = np.array([[0, 0, 0, 255], [255, 255, 255, 255], [1, 127, 254, 255], [200, 3, 77, 255], [255, 0, 128, 255], [9, 9, 9, 255]], np.uint8)   # 3 x 2 pixels
    fine = np.repeat(np.repeat(colours.reshape(2, 3, 4), aa, axis=0), aa, axis=1)
    assert np.array_equal(box(fine, 3, 2, aa), colours)


@pytest.mark.parametrize("aa,total,want", [(2, 2, 1), (2, 1, 0), (3, 4, 0), (3, 5, 1), (4, 8, 1), (4, 7, 0), (4, 16 * 255 - 8, 255), (3, 9 * 255 - 5, 254)])
def test_box_rounds_half_up(aa, total, want):
    """a sum of `total` over aa*aa samples: exactly half (2 of 4, 8 of 16) goes up, 4 of 9 is below half and 5 of 9 above"""
    fine = np.zeros((aa * aa, 4), np.uint8)
    fine[:, 3] = 255
    left = total
    for i in range(aa * aa):   # spread over the samples, a different spread per channel
        fine[i, 0] = min(left, 255)
        left -= int(fine[i, 0])
    fine[:, 1] = fine[::-1, 0]
    fine[:, 2] = np.roll(fine[:, 0], 1)
    assert left == 0 and box(fine, 1, 1, aa).tolist() == [[want, want, want, 255]]


@pytest.mark.parametrize("name", ["frame_a04_own_icosphere_96x64", "frame_a07_own_terrain_n5_96x64", "frame_a07_own_mol_lattice_n6_96x64"])
def test_box_of_an_oracle_fine_frame_is_well_formed(name):
    """one small case per dialect (Assign04 mesh, Assign07 mesh, Assign07 molecule): the CPU oracle's fine frame of a 12 x 8 job, averaged"""
    _, d = fixture(name)
    for aa in AAS:
        fd = fine_job(d, 12, 8, aa)
        assert fd["width"] == 12 * aa and fd["cam"][14] == 12.0 * aa and fd["cam"][15] == 8.0 * aa and fd["cam"][:14] == list(d["cam"])[:14]
        assert {k: v for k, v in fd.items() if k not in ("width", "height", "cam")} == {k: v for k, v in d.items() if k not in ("width", "height", "cam")}
        fine, _ = F.run_frame("oracle", F.Frame(fd))
        out = box(fine, 12, 8, aa)
        assert out.shape == (96, 4) and out.dtype == np.uint8 and (out[:, 3] == 255).all()
        lit = (fine.reshape(8, aa, 12, aa, 4)[..., :3].max(axis=(1, 3, 4)) > 0).ravel()
        assert lit.any() and not out[~lit, :3].any()          # something shows, and a pixel none of whose samples hit is black
        lo, hi = (fine.reshape(8, aa, 12, aa, 4).min(axis=(1, 3)).reshape(-1, 4), fine.reshape(8, aa, 12, aa, 4).max(axis=(1, 3)).reshape(-1, 4))
        assert (out >= lo).all() and (out <= hi).all()         # an average lies between its samples


def test_timing_file_is_well_formed():
    """profiles/frame_aa/timing.json (profiles/frame_aa_bench.py), where present: three variants per configuration and aa, and the structure that
    ships per aa.  Nothing is timed here."""
    if not os.path.exists(TIMING):
        pytest.skip("profiles/frame_aa/timing.json is not there")
    t = json.load(open(TIMING))
    assert set(t["shipped"]) == {"2", "3", "4"} and all(v in ("pixel", "lanes") for v in t["shipped"].values())
    assert len(t["runs"]) >= 4 * 3
    for r in t["runs"]:
        assert r["aa"] in (2, 3, 4) and r["fine"][0] == r["aa"] * r["output"][0] and r["fine"][1] == r["aa"] * r["output"][1]
        for v in ("fine_frame", "pixel", "lanes"):
            m = r["ms"][v]
            assert 0 < m["min"] <= m["median"] <= m["max"] and m["calls"] == 20
        assert r["shipped"] == t["shipped"][str(r["aa"])] and isinstance(r["within_spread"], bool)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(pkg):
    from raytracing_amd.pyhost import mirt
    c = mirt.Context(0)
    yield c
    c.destroy()


def packed(d):
    from raytracing_amd.pyhost import render
    return render.FramePacked(d)


def aa_frame(ctx, d, W, H, aa):
    """mirt_render_frame_aa of coarse_job(d, W, H) into a pixel buffer with a sentinel tail: the W*H pixels, after checking the tail"""
    from raytracing_amd.pyhost import render
    f = render.FrameOneLaunch(ctx, packed(coarse_job(d, W, H)), aa=aa)
    try:
        big = ctx.buffer(W * H * 4 + TAIL)
        f.bufs.append(big)
        big.write(np.full(big.nbytes, SENTINEL, np.uint8))
        f.pixels = big
        f.render()
        raw = big.read(np.uint8)
        assert (raw[W * H * 4:] == SENTINEL).all(), "nothing past W*H*4 bytes is written"
        return raw[:W * H * 4].reshape(-1, 4)
    finally:
        f.release()


def lib_fine(ctx, d, W, H, aa):
    from raytracing_amd.pyhost import render
    return render.render_frame_one_launch(ctx, packed(fine_job(d, W, H, aa)))[0]


@pytest.mark.gpu
@pytest.mark.parametrize("aa", [2, 4])
@pytest.mark.parametrize("name", CASES)
def test_against_the_references_fixtures(ctx, name, aa):
    """every committed Assign04 / Assign07 fixture's `pixel` IS a fine frame (of the reference's own host and compiled kernels): the frame at 1 / aa
    of its size equals its box average"""
    fx, d = fixture(name)
    W, H = d["width"] // aa, d["height"] // aa
    assert (W, H) in ((160 // aa, 120 // aa), (96 // aa, 64 // aa)) and fine_job(d, W, H, aa) == coarse_job(d, d["width"], d["height"])
    mixed, undivided = coverage(fx["pixel"], W, H, aa)
    print(f"{name} aa {aa}: {100 * mixed:.1f} % of the pixels have samples that differ, {undivided} pixels have a sum {aa * aa} does not divide")
    assert mixed >= 0.01 and undivided >= 20
    assert np.array_equal(aa_frame(ctx, d, W, H, aa), box(fx["pixel"], W, H, aa))


@pytest.fixture(scope="module")
def jobs(ctx):
    def job(name):
        return both_job(ctx, "frame_a07_own_octahedra_n3_96x64", "frame_a07_own_mol_helix_n3_96x64") if name == "both" else fixture(name)[1]
    return {name: job(name) for name in JOBS}


@pytest.mark.gpu
@pytest.mark.parametrize("aa", AAS)
@pytest.mark.parametrize("name", JOBS)
def test_odd_sizes_equal_the_box_of_the_librarys_fine_frame(ctx, jobs, name, aa):
    """aa 3 as well, at outputs no tile of the kernel divides (one pixel, one row, one column, 37 x 23: several blocks with ragged edges)"""
    d = jobs[name]
    for W, H in SIZES:
        fine = lib_fine(ctx, d, W, H, aa)
        got = aa_frame(ctx, d, W, H, aa)
        assert np.array_equal(got, box(fine, W, H, aa)), (W, H)
        if (W, H) == (37, 23):
            assert (fine[:, :3].max(axis=1) > 0).any() and coverage(fine, W, H, aa)[0] > 0, "the model shows, and edges cross pixels"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["frame_a07_own_terrain_n5_96x64", "frame_a07_own_mol_lattice_n6_96x64"])
def test_37x23_at_three_samples_equals_the_box_of_the_oracles_fine_frame(ctx, name):
    _, d = fixture(name)
    fine, _ = F.run_frame("oracle", F.Frame(fine_job(d, 37, 23, 3)))
    assert np.array_equal(aa_frame(ctx, d, 37, 23, 3), box(fine, 37, 23, 3))


@pytest.mark.gpu
def test_many_blocks(ctx):
    """BASELINE config 3 at 480 x 270, 16 samples a pixel: the box of the library's 1920 x 1080 frame"""
    _, d = fixture("frame_a07_parliament_n16_160x120")
    d = coarse_job(resized(d, 1920, 1080), 480, 270)
    assert fine_job(d, 480, 270, 4) == resized(fixture("frame_a07_parliament_n16_160x120")[1], 1920, 1080)
    fine = lib_fine(ctx, d, 480, 270, 4)
    got = aa_frame(ctx, d, 480, 270, 4)
    assert np.array_equal(got, box(fine, 480, 270, 4))
    assert (got[:, :3].max(axis=1) > 0).mean() > 0.02


@pytest.mark.gpu
@pytest.mark.parametrize("name", JOBS)
def test_one_sample_is_mirt_render_frame(ctx, jobs, name):
    """aa = 1 through the new entry point itself: the pixels and the 40 written bytes of every ray"""
    from raytracing_amd.pyhost import mirt, render
    p = packed(jobs[name])
    want_px, want_rays = render.render_frame_one_launch(ctx, p, keep_rays=True)
    f = render.FrameOneLaunch(ctx, p, keep_rays=True)
    try:
        for b in (f.pixels, f.rays):
            b.write(np.full(b.nbytes, SENTINEL, np.uint8))
        d = ctx.frame_desc(p.assign, p.width, p.height, p.cam, f.pixels, bounds=getattr(p, "bounds", None), n_slabs=getattr(p, "n_slabs", 0), mesh=f.mesh, mol=f.mol,
                           rays=f.rays)
        assert mirt.lib().mirt_render_frame_aa(ctx.h, C.byref(d), 1) == 0
        assert np.array_equal(f.pixels.read(np.uint8).reshape(-1, 4), want_px)
        got, pad = rays40(f.rays.read(np.uint8))
        assert np.array_equal(got, rays40(want_rays)[0]) and (pad == SENTINEL).all()
    finally:
        f.release()


@pytest.mark.gpu
def test_refusals_write_nothing(ctx):
    from raytracing_amd.pyhost import mirt, render
    fx, d = fixture("frame_a07_house_n8_160x120")
    W, H = 80, 60
    p = packed(coarse_job(d, W, H))
    f = render.FrameOneLaunch(ctx, p, aa=2)
    rays = ctx.buffer(W * H * 48)
    small = ctx.buffer(W * H * 4 - 1)
    for b in (f.pixels, rays, small):
        b.write(np.full(b.nbytes, SENTINEL, np.uint8))
    args = dict(bounds=p.bounds, n_slabs=p.n_slabs, mesh=f.mesh)

    def refused(code, aa=2, width=W, height=H, pixel=f.pixels, cam=p.cam, **kw):
        with pytest.raises(mirt.MirtError) as e:
            ctx.render_frame(7, width, height, cam, pixel, aa=aa, **dict(args, **kw))
        assert e.value.code == code, str(e.value)
    refused(E_ARG, aa=0)
    refused(E_ARG, aa=5)
    refused(E_ARG, rays=rays)
    wide = p.cam.copy()
    wide[14] = 32768.0
    refused(E_ARG, width=32768, cam=wide)          # 2 x 32768 = 65536 samples per row
    refused(E_RANGE, pixel=small)
    desc = ctx.frame_desc(7, W, H, p.cam, f.pixels, **args)
    ghost = C.create_string_buffer(4096)           # not a context of this library
    assert mirt.lib().mirt_render_frame_aa(C.cast(ghost, C.c_void_p), C.byref(desc), 2) == E_HANDLE
    ctx.finish()
    for b in (f.pixels, rays, small):
        assert (b.read(np.uint8) == SENTINEL).all()
    f.render()   # and the same descriptor, whole, renders
    assert np.array_equal(f.pixels.read(np.uint8).reshape(-1, 4), box(fx["pixel"], W, H, 2))
    for b in (rays, small):
        b.release()
    f.release()


@pytest.mark.gpu
def test_an_anti_aliased_frame_can_be_recorded(ctx):
    """capture follows mirt_render_frame's rule: after one ordinary run the call records, and the replay renders the frame"""
    from raytracing_amd.pyhost import render
    fx, d = fixture("frame_a07_own_terrain_n5_96x64")
    f = render.FrameOneLaunch(ctx, packed(coarse_job(d, 48, 32)), aa=2)
    f.render()
    ctx.finish()
    ctx.capture_begin()
    f.render()
    g = ctx.capture_end()
    f.pixels.write(np.zeros(f.pixels.nbytes, np.uint8))
    ctx.graph_launch(g)
    ctx.finish()
    assert np.array_equal(f.pixels.read(np.uint8).reshape(-1, 4), box(fx["pixel"], 48, 32, 2))
    ctx.graph_release(g)
    f.release()


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "2015-raytracing_amd", "libmirt_default.so")), reason="needs libmirt_default.so")
def test_the_default_contract_library():
    """libmirt_default.so in a process of its own (a process loads one libmirt): the 37 x 23 outputs of every job at 2, 3 and 4 samples per axis against
    the box of THAT library's fine frames"""
    env = dict(os.environ, MIRT_CONTRACT="default")
    env.pop("MIRT_LIB_PATH", None)
    r = subprocess.run([sys.executable, CHILD], env=env, capture_output=True, text=True, timeout=600)
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0, (lines[-1:] or r.stderr[-2000:])
    assert len(lines) == len(JOBS) * len(AAS) and all(l["ok"] and l["lit"] > 0 for l in lines)
    assert all("libmirt_default.so" in l["library"] for l in lines)


# ---- Node -----------------------------------------------------------------------------------------------------------------------------------
def cli(args, env=None):
    r = subprocess.run([node, os.path.join(HOST, "cli.js")] + [str(a) for a in args], capture_output=True, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr.decode()
    return r


OWN = [("tri/terrain.json", 5), ("tri/octahedra.json", 3), ("mol/helix.pdb", 3), ("mol/lattice.pdb", 6)]


@pytest.mark.gpu
@pytest.mark.skipif(node is None or not os.path.exists(ADDON), reason="node or the addon is not there")
@pytest.mark.parametrize("model,n", OWN)
def test_node_writes_the_python_hosts_frame(ctx, tmp_path, model, n):
    from raytracing_amd.pyhost import render
    path = os.path.join(PAGE, model)
    job = json.loads(cli(["pack-frame", 7, path, 100, 60, n]).stdout)
    for aa in (2, 3):
        out = str(tmp_path / f"aa{aa}.rgba")
        r = cli(["frame", 7, path, 100, 60, n, out, "--aa", aa])
        want, _ = render.render_frame_one_launch(ctx, packed(job), aa=aa)
        assert np.array_equal(np.fromfile(out, np.uint8).reshape(-1, 4), want) and (want[:, :3] > 0).any()
        assert f"aa {aa}".encode() in r.stderr


@pytest.mark.gpu
@pytest.mark.skipif(node is None or not os.path.exists(ADDON), reason="node or the addon is not there")
def test_node_refuses_aa_with_assign01(tmp_path):
    r = subprocess.run([node, os.path.join(HOST, "cli.js"), "frame", "1", "-", "80", "60", "0", str(tmp_path / "x.rgba"), "--aa", "2"], capture_output=True)
    assert r.returncode != 0 and b"--aa" in r.stderr
