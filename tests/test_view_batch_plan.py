"""CPU: what csrc/pt_view_plan.hpp decides for mirt_view_rays_batch and mirt_render_view_batch, dumped by tests/view_batch_plan_dump.cpp -- a
plain C++ program, no device: every verdict of view_check_batch in its order of precedence and mirt_render_view_batch's on top; the
descriptor's own basis being NaN is no refusal while a NaN or an infinity in any of a camera's twelve slots is, naming the frame; row tiles
are refused; the limit of 2^32 - 256 rays applies to the whole batch; and the plan against plain integer arithmetic, N * height above 65535
included."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "2015-raytracing_amd", "csrc")
E_ARG = -1
(OK, STRUCT_SIZE, MODEL, FLAGS, SAMPLES, EXTENT, TILE, TILE_RAYS, BASIS, ORTHO_WINDOW, FISHEYE_ANGLE, T_MIN, T_MAX, TONE, NO_SEEDS, NO_OUTPUT,
 ACCUMULATE_NEEDS_RADIANCE, NO_GUIDE, AO_STRUCT_SIZE, AO_SAMPLES, AO_RADIUS, AO_BIAS, AO_NO_SEEDS, AO_NO_OUTPUT, BATCH_TILE, BATCH_NO_CAMERAS,
 BATCH_CAMERA, BATCH_RAYS) = range(28)
MAX_RAYS = 2 ** 32 - 256


@pytest.fixture(scope="module")
def decide(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "no g++ to compile tests/view_batch_plan_dump.cpp with"
    exe = str(tmp_path_factory.mktemp("view_batch_plan") / "view_batch_plan_dump")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "view_batch_plan_dump.cpp"), "-o", exe], check=True)

    def run(cases):
        out = subprocess.run([exe], input="".join(c + "\n" for c in cases), stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
        assert len(out) == len(cases)
        return [tuple(int(t) for t in l.split()) for l in out]
    return run


def verdicts(decide, table):
    for (case, want_a, want_b), g in zip(table, decide([c for c, _a, _b in table])):
        assert (g[0], g[2]) == (want_a, want_b), f"{case!r}: verdicts {g[0]}, {g[2]}; want {want_a}, {want_b}"
        assert g[1] == (0 if want_a == OK else E_ARG) and g[3] == (0 if want_b == OK else E_ARG), (case, g)


def test_every_verdict(decide):
    verdicts(decide, [
        ("", OK, OK), ("n=1", OK, OK), ("n=0", OK, OK), ("n=0 cameras=0", OK, OK), ("nrows=7", OK, OK), ("k=16", OK, OK), ("model=0", OK, OK), ("model=2", OK, OK),
        ("struct_size=100", STRUCT_SIZE, STRUCT_SIZE), ("model=3", MODEL, MODEL), ("flags=2", FLAGS, FLAGS), ("k=3", SAMPLES, SAMPLES), ("k=32", SAMPLES, SAMPLES),
        ("width=0", EXTENT, EXTENT), ("height=65536", EXTENT, EXTENT),
        ("cameras=0", BATCH_NO_CAMERAS, BATCH_NO_CAMERAS), ("cam1.0=nan", BATCH_CAMERA, BATCH_CAMERA),
        ("model=0 half_w=0", ORTHO_WINDOW, ORTHO_WINDOW), ("model=2 half_angle=0", FISHEYE_ANGLE, FISHEYE_ANGLE), ("t_min=-1", T_MIN, T_MIN), ("t_max=0", T_MAX, T_MAX),
        # mirt_render_view_batch's own rules, behind the shared ones, in mirt_render_view's order
        ("tone=nan", OK, TONE), ("tone=0", OK, TONE), ("tone=nan pixel=0", OK, OK), ("seeds=0", OK, NO_SEEDS), ("radiance=0 pixel=0", OK, NO_OUTPUT),
        ("flags=1", OK, OK), ("flags=1 radiance=0", OK, ACCUMULATE_NEEDS_RADIANCE), ("tone=nan seeds=0", OK, TONE), ("seeds=0 radiance=0 pixel=0", OK, NO_SEEDS),
        ("t_max=0 seeds=0", T_MAX, T_MAX), ("cam0.3=inf tone=nan", BATCH_CAMERA, BATCH_CAMERA),
    ])


def test_order_of_precedence(decide):
    """each refusal with every later one present too: the earlier one is reported"""
    chain = [("struct_size=100", STRUCT_SIZE), ("model=3", MODEL), ("flags=2", FLAGS), ("k=3", SAMPLES), ("width=0", EXTENT), ("row0=1", BATCH_TILE),
             ("n=40000000", BATCH_RAYS), ("cameras=0", BATCH_NO_CAMERAS), ("cam2.5=nan", BATCH_CAMERA), ("t_min=-1", T_MIN), ("t_max=-2", T_MAX)]
    cases = [" ".join(c for c, _v in chain[i:]) for i in range(len(chain))]
    for (case, (_c, want)), g in zip(zip(cases, chain), decide(cases)):
        assert g[0] == want and g[2] == want, (case, g, want)
    # the window and the angle, each in its model, sit between the cameras and t_min
    got = decide(["model=0 cam0.0=nan half_w=0 t_min=-1", "model=0 half_w=0 t_min=-1", "model=2 cam0.0=nan half_angle=4 t_min=-1", "model=2 half_angle=4 t_min=-1",
                  "model=1 half_w=0 half_angle=0"])
    assert [g[0] for g in got] == [BATCH_CAMERA, ORTHO_WINDOW, BATCH_CAMERA, FISHEYE_ANGLE, OK]


def test_the_descriptors_own_basis_is_neither_read_nor_checked(decide):
    cases = [f"basis{s}={v}" for s in range(12) for v in ("nan", "inf", "-inf")]
    for case, g in zip(cases, decide(cases)):
        assert (g[0], g[2]) == (OK, OK), (case, g)


@pytest.mark.parametrize("value", ["nan", "inf", "-inf"])
def test_a_camera_with_a_non_finite_slot_is_refused_and_named(decide, value):
    cases = [f"n=5 cam{f}.{s}={value}" for f in (0, 3, 4) for s in range(12)]
    for case, g in zip(cases, decide(cases)):
        assert (g[0], g[2]) == (BATCH_CAMERA, BATCH_CAMERA) and g[4] == int(case.split("cam")[1].split(".")[0]), (case, g)
    (g,) = decide([f"n=5 cam3.2={value} cam1.7={value}"])
    assert g[0] == BATCH_CAMERA and g[4] == 1, "the first bad frame is the one named"
    (g,) = decide([f"n=3 cam3.2={value}"])
    assert g[0] == OK and g[4] == -1, "a camera past n_frames is not read"


def test_row_tiles_are_refused(decide):
    verdicts(decide, [("row0=1", BATCH_TILE, BATCH_TILE), ("row0=7", BATCH_TILE, BATCH_TILE), ("nrows=3", BATCH_TILE, BATCH_TILE), ("nrows=8", BATCH_TILE, BATCH_TILE),
                      ("row0=1 nrows=6", BATCH_TILE, BATCH_TILE), ("nrows=7", OK, OK), ("nrows=0", OK, OK), ("height=1 nrows=1", OK, OK)])


def test_the_ray_limit_is_the_whole_batchs(decide):
    # a frame of 4096 x 4096 x 1 = 2^24 rays: 255 frames fit, 256 are 2^32 > 2^32 - 256
    # a frame of 16 x 16 x 1 = 256 rays: 2^24 frames are 2^32 rays
    verdicts(decide, [("width=4096 height=4096 k=1 n=255", OK, OK), ("width=4096 height=4096 k=1 n=256", BATCH_RAYS, BATCH_RAYS),
                      ("width=16 height=16 k=1 n=16777216", BATCH_RAYS, BATCH_RAYS), ("width=65535 height=65535 k=1 n=1", OK, OK),
                      ("width=65535 height=65535 k=1 n=2", BATCH_RAYS, BATCH_RAYS), ("width=65535 height=65535 k=2 n=1", BATCH_RAYS, BATCH_RAYS),
                      ("width=65535 height=65535 k=16 n=4294967295", BATCH_RAYS, BATCH_RAYS), ("width=1 height=1 k=1 n=4294967295", BATCH_RAYS, BATCH_RAYS),
                      ("width=4096 height=4096 k=1 n=256 cameras=0", BATCH_RAYS, BATCH_RAYS)])
    for w, h, k, n in ((4096, 4096, 1, 255), (65535, 65535, 1, 1), (255, 257, 16, 255)):
        assert n * w * h * k * k <= MAX_RAYS
        (g,) = decide([f"width={w} height={h} k={k} n={n}"])
        assert g[0] == OK and g[10] == n * w * h * k * k, g


PLANS = [(13, 7, 2, 3), (13, 7, 1, 3), (5, 3, 2, 3), (1, 1, 1, 5), (3, 1, 16, 2), (1, 1, 1, 64), (32, 16, 2, 1024), (13, 7, 16, 1), (1, 65535, 1, 2), (2, 40000, 2, 3),
          (1, 1, 1, 4000), (7, 3, 4, 0), (65535, 1, 1, 4000), (3, 5, 8, 17)]


@pytest.mark.parametrize("w,h,k,n", PLANS)
def test_the_plan_is_plain_integer_arithmetic(decide, w, h, k, n):
    (g,) = decide([f"width={w} height={h} k={k} n={n}"])
    rpp = k * k
    pixels, rays = n * w * h, n * w * h * rpp
    blocks, ppb = -(-rays // 256), 256 // rpp
    last = pixels % ppb or ppb
    assert g[0] == OK
    assert g[5:] == (h, w * h, w * h * rpp, n * h, pixels, rays, blocks, ppb, last, -(-blocks // 32)), g
    assert (w * h * rpp) % rpp == 0 and 256 % rpp == 0, "a frame's rays are whole pixels and so are a block's"


def test_rows_of_the_stacked_image_may_pass_65535(decide):
    got = decide(["width=1 height=65535 k=1 n=2", "width=2 height=40000 k=2 n=3", "width=1 height=50 k=1 n=4000"])
    assert [g[8] for g in got] == [131070, 120000, 200000] and all(g[0] == OK for g in got)
