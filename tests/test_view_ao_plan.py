"""CPU: what csrc/pt_view_plan.hpp decides for mirt_view_ao, dumped by tests/view_ao_plan_dump.cpp -- a plain C++ program, no device:
view_check_ao's verdict for every argument rule (the descriptor checks of mirt_view_rays first, then mirt_render_ao's rules for the AO
descriptor, then the two buffers), and the one-lane-per-pixel grid and mask at 1 pixel, 256, 257, the 65535-wide tile and the 2^32 - 256 ray
limit, against plain integer arithmetic."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "2015-raytracing_amd", "csrc")
E_ARG = -1
(OK, STRUCT_SIZE, MODEL, FLAGS, SAMPLES, EXTENT, TILE, TILE_RAYS, BASIS, ORTHO_WINDOW, FISHEYE_ANGLE, T_MIN, T_MAX, TONE, NO_SEEDS, NO_OUTPUT,
 ACCUMULATE_NEEDS_RADIANCE, NO_GUIDE, AO_STRUCT_SIZE, AO_SAMPLES, AO_RADIUS, AO_BIAS, AO_NO_SEEDS, AO_NO_OUTPUT) = range(24)


@pytest.fixture(scope="module")
def decide(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "no g++ to compile tests/view_ao_plan_dump.cpp with"
    exe = str(tmp_path_factory.mktemp("view_ao_plan") / "view_ao_plan_dump")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "view_ao_plan_dump.cpp"), "-o", exe], check=True)

    def run(cases):
        out = subprocess.run([exe], input="".join(c + "\n" for c in cases), stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
        assert len(out) == len(cases)
        return [tuple(int(t) for t in l.split()) for l in out]
    return run


VERDICTS = [
    ("", OK), ("k=1", OK), ("k=16", OK), ("samples=1", OK), ("samples=64", OK), ("radius=inf", OK), ("radius=1e-30", OK), ("bias=0", OK), ("bias=3e38", OK),
    # tone and the meaning of flags are not read; an unknown flag is still refused
    ("tone=nan", OK), ("tone=0", OK), ("flags=1", OK), ("flags=2", FLAGS), ("flags=0x80000001", FLAGS),
    # the descriptor checks of mirt_view_rays
    ("struct_size=100", STRUCT_SIZE), ("model=3", MODEL), ("k=0", SAMPLES), ("k=3", SAMPLES), ("k=32", SAMPLES), ("width=0", EXTENT), ("height=0", EXTENT),
    ("width=65536", EXTENT), ("height=65536", EXTENT), ("row0=7", TILE), ("row0=5 nrows=3", TILE), ("nrows=8", TILE), ("width=65535 height=65535 k=2", TILE_RAYS),
    ("forward0=nan", BASIS), ("forward0=inf", BASIS), ("half_w=0", ORTHO_WINDOW), ("half_w=nan", ORTHO_WINDOW), ("model=2 half_angle=0", FISHEYE_ANGLE),
    ("model=2 half_angle=3.1415930", FISHEYE_ANGLE), ("model=2 half_angle=nan", FISHEYE_ANGLE), ("t_min=-1", T_MIN), ("t_min=nan", T_MIN), ("t_max=nan", T_MAX),
    ("t_max=0", T_MAX), ("t_min=2 t_max=2", T_MAX),
    # mirt_render_ao's rules for the AO descriptor
    ("ao_size=12", AO_STRUCT_SIZE), ("ao_size=0", AO_STRUCT_SIZE), ("samples=0", AO_SAMPLES), ("samples=65", AO_SAMPLES), ("samples=0xFFFFFFFF", AO_SAMPLES),
    ("radius=0", AO_RADIUS), ("radius=-1", AO_RADIUS), ("radius=nan", AO_RADIUS), ("radius=-inf", AO_RADIUS),
    ("bias=-1e-9", AO_BIAS), ("bias=nan", AO_BIAS), ("bias=inf", AO_BIAS), ("bias=-inf", AO_BIAS),
    # the buffers
    ("seeds=0", AO_NO_SEEDS), ("ao_out=0", AO_NO_OUTPUT), ("seeds=0 ao_out=0", AO_NO_SEEDS),
    # the order: the view, then the AO descriptor, then the buffers
    ("k=3 samples=0 seeds=0", SAMPLES), ("samples=0 seeds=0", AO_SAMPLES), ("ao_size=12 samples=0", AO_STRUCT_SIZE), ("radius=0 bias=-1", AO_RADIUS),
    ("bias=-1 ao_out=0", AO_BIAS),
]


def test_verdicts(decide):
    for (case, want), g in zip(VERDICTS, decide([c for c, _w in VERDICTS])):
        assert g[0] == want, f"{case!r}: verdict {g[0]}, want {want}"
        assert g[1] == (0 if want == OK else E_ARG), (case, g)


def test_grid_and_mask_of_one_lane_per_pixel(decide):
    """pixels -> ceil(pixels / 256) blocks and ceil(pixels / 32) mask words, whatever k; rays = pixels * k * k"""
    cases = {"width=1 height=1 k=1": (1, 1), "width=1 height=1 k=16": (1, 256), "width=256 height=1": (256, 1024), "width=257 height=1": (257, 1028),
             "width=16 height=16 k=1": (256, 256), "width=37 height=21": (777, 3108), "": (91, 364), "row0=3 nrows=1": (13, 52),
             "width=65535 height=1 k=1": (65535, 65535), "width=65535 height=1 k=16": (65535, 65535 * 256), "width=65535 height=65535 nrows=1 row0=65534 k=16": (65535, 65535 * 256),
             "width=65535 height=65535 k=1": (65535 * 65535, 65535 * 65535),   # the largest image there is: inside the ray limit at k = 1
             "width=65535 height=256 k=16 nrows=255": (65535 * 255, 65535 * 255 * 256)}
    for (case, (pixels, rays)), g in zip(cases.items(), decide(list(cases))):
        assert g[0] == OK and g[2:] == (pixels, rays, -(-pixels // 256), -(-pixels // 32)), (case, g)
    assert decide(["width=37 height=21"])[0][4:] == (4, 25)   # four blocks (the last of 9 lanes), 25 words of a bit per pixel


def test_the_ray_limit(decide):
    """a tile of 2^32 - 256 rays is the last one taken; one ray more is refused and plans nothing"""
    limit = 2 ** 32 - 256
    # 2^32 - 256 = 256 * (2^24 - 1) = 256 * 4095 * 4097: 4095 x 4097 pixels at k = 16 is exactly the limit
    assert 4095 * 4097 * 256 == limit
    at, over, wide = decide(["width=4095 height=4097 k=16", "width=4095 height=4098 k=16", "width=65535 height=65535 k=2 nrows=16385"])
    assert at[0] == OK and at[2:] == (2 ** 24 - 1, limit, 2 ** 16, 2 ** 19)
    assert over[0] == TILE_RAYS and over[1] == E_ARG
    assert 65535 * 16384 * 4 <= limit < 65535 * 16385 * 4 and wide[0] == TILE_RAYS
    assert decide(["width=65535 height=65535 k=2 nrows=16384"])[0][:4] == (OK, 0, 65535 * 16384, 65535 * 16384 * 4)
    assert decide(["k=3"])[0][2:] == (0, 0, 0, 0)
