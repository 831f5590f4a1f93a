"""Generated cameras through every Assign01 / 04 / 07 frame path (csrc/pt_kernels_frame.hip): k_a01_raytrace, k_frame_initTrace, k_a04_meshTrace,
k_a07_meshTrace (with and without group spheres), k_a07_molTrace, k_frame_fused (rays kept or not; the enqueue stream with frame fusion on) and
k_frame_aa_lanes.  The cameras, the jobs and why the degenerate cameras may run on the device: tests/frame_cameras_common.py.

Every device comparison is bit for bit against the CPU oracle -- every pixel, and every ray's mint and maxt wherever a ray buffer exists.  The
oracle itself is compared with the reference's code.cl compiled for the host under every camera (skipped without oracle/_ref), with the reference's
own binaries on the device under three of them, and with four frames of the reference's own host code in its Rotate mode
(tests/golden/frame_rot_*.npz).  The guards (CPU, the oracle alone) say what the frames reach -- lit shares, rays that start inside the box, the
direction signs a whole wave shares, the page's near-zero direction components -- so that no comparison passes on an empty frame; run with -s to
see the figures."""
import glob
import os

import numpy as np
import pytest

import a10_pass as A
import frame_aa_common as AA
import frame_cameras_common as K
import frame_pass as F
from conftest import GOLDEN, ROOT, bits
from test_frames import fixture, resized
from test_random_molecules import every_path, same, uses_group_spheres

REF = {n: os.path.join(ROOT, "oracle", "_ref", f"libref_a{n:02d}.so") for n in (1, 4, 7)}
REF_GPU = {n: os.path.join(ROOT, "oracle", "_ref", f"a{n:02d}_gfx950.hsaco") for n in (1, 4, 7)}
ROT = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, "frame_rot_*.npz")))
A07_JOBS = [n for n in K.JOBS if n not in ("frame_a04_teapot_160x120", "soup_n0")]
MESH_JOBS = [n for n in K.JOBS if "mol" not in n]
AA_CAMERAS = ("orbit_90", "orbit_180", "inside", "from_below")
AA_JOBS = K.FIXTURE_JOBS + ("soup_n0", "soup_n2", "both_models")
REF_GPU_CAMERAS = ("orbit_90", "orbit_180", "inside")
REF_GPU_SIZE = (96, 64)                      # multiples of the reference's 8 x 8 work-group: its NDRange is the image
A01_SIZES = ((64, 48), (67, 45))
SENTINEL = 0xA5


def frames_of(name, cameras=None):
    """[(camera, size, job, oracle pixels, oracle rays)] of a named job: every camera it has, at both sizes"""
    out = []
    for camera in (cameras or K.cameras_of(name)):
        for size in K.SIZES:
            e = K.expected(name, camera, size)
            if e is not None:
                out.append((camera, size, *e))
    return out


# ---- CPU: the page's camera ------------------------------------------------------------------------------------------------------------------------
def rot_fixture(name):
    fx = np.load(os.path.join(GOLDEN, name + ".npz"))
    base = bytes(fx["base"]).decode()
    d = resized(fixture(base)[1], 96, 64)
    return fx, d, int(name.rsplit("_", 1)[1])


def test_the_rotated_fixtures_are_the_issued_ones():
    assert ROT == ["frame_rot_a04_teapot_135", "frame_rot_a07_mol_c60_n4_270", "frame_rot_a07_teapot_n2_180", "frame_rot_a07_teapot_n2_90"]
    for name in ROT:
        fx = np.load(os.path.join(GOLDEN, name + ".npz"))
        assert sorted(fx.files) == ["base", "cam", "pixel", "rays_maxt", "rays_mint"] and fx["pixel"].shape == (96 * 64, 4)
        assert (fx["pixel"][:, :3].max(axis=1) > 0).mean() > 0.02


@pytest.mark.parametrize("name", ROT)
def test_page_camera_is_the_pages_rotate(name):
    """Camera.set + Camera.rotate restated (frame_cameras_common.page_camera) against the reference's own host code run with its own rotate: the 16
    floats, bit for bit -- the near-zero components Math.cos / Math.sin leave at 90, 180 and 270 degrees included"""
    fx, d, angle = rot_fixture(name)
    cam = np.asarray(K.page_camera(d, angle), np.float32)
    assert np.array_equal(cam.view(np.uint32), np.asarray(fx["cam"], np.float32).view(np.uint32)), (cam.tolist(), fx["cam"].tolist())
    if angle in (90, 180, 270):
        tiny = np.abs(cam[3:12])
        assert ((tiny > 0) & (tiny < 2.0 ** -40)).any()
    # without an angle: Camera.set alone, the block the base fixture carries
    base = fixture(bytes(fx["base"]).decode())[1]
    assert np.array_equal(np.asarray(K.page_camera(base), np.float32), np.asarray(base["cam"], np.float32))


@pytest.mark.parametrize("name", ROT)
def test_oracle_reproduces_the_rotated_fixture(name):
    fx, d, _ = rot_fixture(name)
    px, rays = F.run_frame("oracle", F.Frame(dict(d, cam=fx["cam"].tolist())))
    assert np.array_equal(px, fx["pixel"])
    assert np.array_equal(bits(rays["maxt"]), bits(fx["rays_maxt"])) and np.array_equal(bits(rays["mint"]), bits(fx["rays_mint"]))


def test_orbit_0_is_camera_set():
    """rotate(0) computes what defaultInit + set leave: W = (0, 0, diag) / diag, U = V x W -- the fixtures' block, exactly"""
    for name in K.FIXTURE_JOBS:
        d = K.job_named(name)
        assert K.page_camera(d, 0) == K.page_camera(d)


# ---- CPU: the guards ---------------------------------------------------------------------------------------------------------------------------------
def test_the_jobs_reach_the_group_spheres_and_the_plain_loop():
    """launch_frame_stage / launch_frame_fused's rule n_slots >= n^3 * 4 * 16, and a partial last group in the brute-force list"""
    groups = {n: uses_group_spheres(K.job_named(n)) for n in K.JOBS if "n_slabs" in K.job_named(n) and "atoms" not in K.job_named(n)}
    assert groups["frame_a07_teapot_n2_160x120"] and groups["soup_n1"] and groups["soup_n2"]
    assert not groups["frame_a07_teapot_n8_160x120"] and not groups["frame_a07_own_octahedra_n3_96x64"]
    assert {True, False} == set(groups.values())
    assert K.job_named("soup_n0")["t_size"] % 16 and K.job_named("frame_a04_teapot_160x120")["t_size"] % 16 == 0
    for n in ("soup_n1", "soup_n2"):   # a cell whose list is no multiple of a group: the walk's `whole` ballot fails on its tail
        assert (np.diff(K.job_named(n)["slab_size"].astype(np.int64)) % 16).any()
    print("\ngroup spheres:", groups)


@pytest.mark.parametrize("name", K.JOBS)
def test_no_comparison_passes_on_an_empty_frame(name):
    """orbit, roll, shear, mirror, above, below, telephoto: at least 2 % of every frame lit; every far frame lights a pixel and (Assign07, whose
    initTrace clips) leaves a ray dead; inside / at a vertex: no ray dead"""
    shares = []
    for camera, size, d, px, rays in frames_of(name):
        share = float(K.lit(px).mean())
        if camera in K.LIT_2_PERCENT:
            assert share >= 0.02, (camera, size, share)
            shares.append(share)
        if camera.startswith("far_"):
            assert K.lit(px).any(), (camera, size)
            assert d["assign"] == 4 or (K.dead(rays).any() and not K.dead(rays).all()), (camera, size)
        if camera in K.NO_DEAD_RAY:
            assert not K.dead(rays).any(), (camera, size)
            if d["assign"] == 7:
                assert (rays["mint"] == 0).all(), "the walk starts in the eye's cell"
    print(f"\n{name}: lit share {min(shares):.3f} .. {max(shares):.3f} over {len(shares)} frames")


@pytest.mark.parametrize("name", MESH_JOBS)
def test_a_mesh_shows_from_inside(name):
    """single-sided triangles: from inside the teapot most are back faces; one of the inside cameras has to light a pixel"""
    if name == "frame_a07_parliament_n16_160x120":
        return   # three orbit angles only
    assert any(K.lit(px).any() for camera, _, _, px, _ in frames_of(name, K.NO_DEAD_RAY))


@pytest.mark.parametrize("name", A07_JOBS)
def test_both_directions_of_all_three_axes_are_walked_by_whole_waves(name):
    """Over the job's cameras each of d.x, d.y, d.z > 0 and < 0 is shared by all 64 pixels of a wave (32 x 2: frame_cameras_common's docstring) that
    holds a lit pixel: az.dslab = +1 / az.limit = n and the like as wave-uniform walks, in k_a07_meshTrace / k_a07_molTrace and k_frame_fused"""
    reached = {}
    for camera, size, d, px, rays in frames_of(name, [c for c in K.cameras_of(name) if c not in K.DEGENERATE]):
        for s in K.uniform_lit_tiles(px, rays, size):
            reached.setdefault(s, camera)
    print(f"\n{name}: " + ", ".join(f"d.{'xyz'[k]} {'>' if s > 0 else '<'} 0 by {reached[(k, s)]}" for k, s in sorted(reached)))
    assert set(reached) == {(k, s) for k in range(3) for s in (+1, -1)}


@pytest.mark.parametrize("name", AA_JOBS)
def test_the_anti_aliased_frames_walk_forwards_too(name):
    """k_frame_aa_lanes' waves are 8 x 8 (AA 2) and 21 x 3 (AA 3) tiles of the fine frame: under orbit_180 and from_below whole lit waves go
    forwards in z and in y"""
    for aa, tile in ((2, (8, 8)), (3, (21, 3))):
        for camera, sign in (("orbit_180", (2, +1)), ("from_below", (1, +1))):
            d = AA.fine_job(K.with_camera(K.job_named(name), camera, K.SIZES[0]), *K.SIZES[0], aa)
            fr = F.Frame(d)
            px, rays = F.run_frame_both("oracle", fr) if fr.both is not None else F.run_frame("oracle", fr)
            assert sign in K.uniform_lit_tiles(px, rays, (d["width"], d["height"]), tile), (aa, camera)


@pytest.mark.parametrize("angle", (90, 180, 270))
def test_the_pages_axis_parallel_frames_have_tiny_components(angle):
    """0 < |d_k| < 2^-40 in every job's orbit_90 / 180 / 270 frame at 67 x 45: the centre column (frame_cameras_common's docstring)"""
    for name in K.JOBS:
        if f"orbit_{angle}" in K.cameras_of(name):
            _, _, rays = K.expected(name, f"orbit_{angle}", (67, 45))
            n = K.tiny_components(rays)
            assert n >= 45, (name, n)
    print(f"\norbit_{angle}: {n} components of 0 < |d_k| < 2^-40 in a 67 x 45 frame")


# ---- CPU: the oracle against the compiled reference ---------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not (os.path.exists(REF[4]) and os.path.exists(REF[7])), reason="oracle/_ref/libref_a0N.so not built (the reference's own kernels for the host)")
@pytest.mark.parametrize("name", K.REF_JOBS)
def test_oracle_equals_the_compiled_reference_under_every_camera(name):
    for camera, _ in K.CAMERAS:
        d, px, rays = K.expected(name, camera, (67, 45))
        want_px, want_rays = F.run_frame("ref", F.Frame(d))
        assert np.array_equal(px, want_px), camera
        assert np.array_equal(bits(rays["maxt"]), bits(want_rays["maxt"])) and np.array_equal(bits(rays["mint"]), bits(want_rays["mint"])), camera


A01_CASES = [(r, a) for r in K.A01_RADII for a in K.A01_ANGLES]


def test_assign01_cameras_reach_the_second_root_and_the_wrap():
    """inside the sphere (radius 0.25) only the far root is positive: every pixel hits, at t in [0.25, 0.75]; from radius 6, t > 1 everywhere and
    (1 - t) * 255 < 0: the byte is the low byte of a negative int"""
    for angle in K.A01_ANGLES:
        px, _ = F.run_frame("oracle", F.Frame(K.a01_job(0.25, angle, (64, 48))))
        assert (px[:, 0] > 0).all() and px[:, 0].min() >= int(0.25 * 255) - 1 and px[:, 0].max() <= int(0.75 * 255) + 1
        px, _ = F.run_frame("oracle", F.Frame(K.a01_job(6.0, angle, (64, 48))))
        hit = px[:, 0] > 0
        assert hit.any() and not hit.all(), "a clamped shade would leave the frame black"
        px, _ = F.run_frame("oracle", F.Frame(K.a01_job(1.0, angle, (64, 48))))
        assert (px[:, 0] > 0).any()   # (A01's getRay aims normalize(cop - eye): from one radius every ray of this window meets the sphere)


@pytest.mark.skipif(not os.path.exists(REF[1]), reason="oracle/_ref/libref_a01.so not built (the reference's own kernel for the host)")
@pytest.mark.parametrize("radius,angle", A01_CASES)
def test_assign01_oracle_equals_the_compiled_reference(radius, angle):
    fr = F.Frame(K.a01_job(radius, angle, (64, 48)))
    assert np.array_equal(F.run_frame("oracle", fr)[0], F.run_frame("ref", fr)[0])


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------------
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


def all_paths(ctx, fctx, d, want_px, want_rays):
    """every_path (kernel by kernel, one launch with and without rays) and the enqueue stream on the context that fuses it"""
    from raytracing_amd.pyhost import render
    p = render.FramePacked(d)
    every_path(ctx, d, want_px, want_rays, stream=p.both is not None)
    n0 = fctx.fused_frames()
    px, rays = render.render_frame_stream(fctx, p, rays_fill=SENTINEL)
    assert fctx.fused_frames() == n0 + 1, "the stream was not fused"
    assert (rays == SENTINEL).all(), "a fused frame does not write the ray buffer"
    same("fused stream", px, None, want_px, want_rays)


@pytest.mark.gpu
@pytest.mark.parametrize("name", K.JOBS)
def test_every_path_matches_the_oracle_under_every_camera(ctx, fctx, name):
    """each camera of the job x both sizes x every path; all differing frames are reported, not the first"""
    wrong = []
    for camera, size, d, want_px, want_rays in frames_of(name):
        try:
            all_paths(ctx, fctx, d, want_px, want_rays)
        except AssertionError as e:
            wrong.append(f"{camera} {size[0]}x{size[1]}: {str(e).splitlines()[0]}")
    assert not wrong, "\n".join(wrong)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ROT)
def test_every_path_reproduces_the_rotated_fixture(ctx, fctx, name):
    fx, d, _ = rot_fixture(name)
    rays = np.zeros(96 * 64, A.RAY_DT)
    rays["maxt"], rays["mint"] = fx["rays_maxt"], fx["rays_mint"]
    all_paths(ctx, fctx, dict(d, cam=fx["cam"].tolist()), fx["pixel"], rays)


@pytest.mark.gpu
@pytest.mark.parametrize("name", AA_JOBS)
def test_anti_aliased_frames_match_the_oracles_box_average(ctx, name):
    """mirt_render_frame_aa at 67 x 45, aa = 2 and 3: the integer box average of the oracle's fine frame (tests/frame_aa_common.py)"""
    from raytracing_amd.pyhost import render
    W, H = K.SIZES[0]
    wrong = []
    for camera in AA_CAMERAS:
        d = K.with_camera(K.job_named(name), camera, (W, H))
        for aa in (2, 3):
            fr = F.Frame(AA.fine_job(d, W, H, aa))
            fine, _ = F.run_frame_both("oracle", fr) if fr.both is not None else F.run_frame("oracle", fr)
            assert K.lit(fine).any()
            got, _ = render.render_frame_one_launch(ctx, render.FramePacked(AA.coarse_job(d, W, H)), aa=aa)
            if not np.array_equal(got, AA.box(fine, W, H, aa)):
                wrong.append(f"{camera} aa {aa}: {int((got != AA.box(fine, W, H, aa)).any(axis=1).sum())} pixels differ")
    assert not wrong, "\n".join(wrong)


@pytest.mark.gpu
@pytest.mark.parametrize("size", A01_SIZES)
def test_assign01_raytrace_matches_the_oracle(ctx, size):
    """k_a01_raytrace under orbits about its sphere: both roots, the wrapped shade; 67 x 45 runs on a padded NDRange (the kernel's own range check)"""
    from raytracing_amd.pyhost import render
    for radius, angle in A01_CASES:
        d = K.a01_job(radius, angle, size)
        want, _ = F.run_frame("oracle", F.Frame(d))
        assert (want[:, 0] > 0).any()
        px, _ = render.render_frame(ctx, render.FramePacked(d))
        assert np.array_equal(px, want), (radius, angle)


@pytest.mark.gpu
@pytest.mark.skipif(not all(os.path.exists(p) for p in REF_GPU.values()), reason="oracle/_ref/*.hsaco not built (make -C oracle ref_gpu, build container)")
@pytest.mark.parametrize("name", ("assign01",) + K.REF_JOBS)
def test_frames_equal_the_reference_binaries_under_moved_cameras(ctx, name):
    """The reference's own kernels as AMD's OpenCL toolchain builds them for gfx950, on the device (oracle/frame_pass.run_frame_gpu), under
    orbit_90, orbit_180 and the eye inside: every pixel, and every ray's maxt"""
    from raytracing_amd.pyhost import render
    if name == "assign01":
        jobs = [K.a01_job(1.0, 90, (64, 48)), K.a01_job(1.0, 180, (64, 48)), K.a01_job(0.25, 0, (64, 48))]
    else:
        jobs = [K.with_camera(K.job_named(name), camera, REF_GPU_SIZE) for camera in REF_GPU_CAMERAS]
    for d in jobs:
        want_px, want_rays = F.run_frame_gpu(F.Frame(d))
        px, rays = render.render_frame(ctx, render.FramePacked(d))
        assert np.array_equal(px, want_px) and K.lit(px).any()
        if want_rays is not None:
            got = np.ascontiguousarray(rays).view(A.RAY_DT)
            assert np.array_equal(bits(got["maxt"]), bits(want_rays["maxt"]))
