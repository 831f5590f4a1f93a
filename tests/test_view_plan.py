"""CPU: the descriptor checks and the launch plan of the view cameras (csrc/pt_view_plan.hpp; mirt_view_rays, mirt_render_view), dumped by
tests/view_plan_dump.cpp -- a plain C++ program, no device.  Every refusal of include/mirt.h's list that needs no device, each accepted border
(k 16, width 65535, half_angle pi, t_max +inf), and the plan's blocks and ragged last block at 13 x 7 for every k and at 1 x 1, against plain
Python integer arithmetic."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "2015-raytracing_amd", "csrc")
HEADER = os.path.join(CSRC, "pt_view_plan.hpp")
E_ARG = -1
(OK, STRUCT_SIZE, MODEL, FLAGS, SAMPLES, EXTENT, TILE, TILE_RAYS, BASIS, ORTHO_WINDOW, FISHEYE_ANGLE, T_MIN, T_MAX, TONE, NO_SEEDS, NO_OUTPUT,
 ACCUMULATE_NEEDS_RADIANCE) = range(17)
PI_F32 = "0x1.921fb6p+1"
ABOVE_PI_F32 = "0x1.921fb8p+1"   # the next float


@pytest.fixture(scope="module")
def decide(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "no g++ to compile tests/view_plan_dump.cpp with"
    exe = str(tmp_path_factory.mktemp("view_plan") / "view_plan_dump")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "view_plan_dump.cpp"), "-o", exe], check=True)

    def run(cases):
        out = subprocess.run([exe], input="".join(c + "\n" for c in cases), stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
        assert len(out) == len(cases)
        return [tuple(int(t) for t in l.split()) for l in out]
    return run


def test_header_is_host_only():
    """it compiles alone with g++ (the fixture) and includes nothing of HIP"""
    text = open(HEADER).read()
    includes = [l.split()[1] for l in text.splitlines() if l.startswith("#include")]
    assert includes == ["<math.h>", "<stddef.h>", "<stdint.h>"], includes
    assert "hip" not in " ".join(includes).lower()
    assert "__device__" not in text and "__host__" not in text and "__global__" not in text


REFUSALS = [
    ("struct_size=100", STRUCT_SIZE), ("struct_size=108", STRUCT_SIZE), ("struct_size=0", STRUCT_SIZE),
    ("model=3", MODEL), ("model=0xFFFFFFFF", MODEL),
    ("flags=2", FLAGS), ("flags=3", FLAGS), ("flags=0x80000000", FLAGS),
    ("k=0", SAMPLES), ("k=3", SAMPLES), ("k=5", SAMPLES), ("k=12", SAMPLES), ("k=32", SAMPLES), ("k=17", SAMPLES),
    ("width=0", EXTENT), ("height=0", EXTENT), ("width=65536", EXTENT), ("height=65536", EXTENT),
    ("row0=7", TILE), ("row0=3", TILE), ("row0=6 nrows=2", TILE), ("nrows=8", TILE), ("row0=0xFFFFFFFF nrows=2", TILE),
    ("width=65535 height=65535 k=2", TILE_RAYS),            # 17 179 344 900 rays > 2^32 - 256
    ("width=65535 height=65535 k=16 nrows=257", TILE_RAYS),
    ("eye0=nan", BASIS), ("eye2=inf", BASIS), ("right1=-inf", BASIS), ("up0=nan", BASIS), ("forward2=inf", BASIS), ("forward0=nan", BASIS),
    ("half_w=0", ORTHO_WINDOW), ("half_h=0", ORTHO_WINDOW), ("half_w=-1", ORTHO_WINDOW), ("half_h=inf", ORTHO_WINDOW), ("half_w=nan", ORTHO_WINDOW),
    ("model=2 half_angle=0", FISHEYE_ANGLE), ("model=2 half_angle=-1", FISHEYE_ANGLE), ("model=2 half_angle=nan", FISHEYE_ANGLE),
    ("model=2 half_angle=inf", FISHEYE_ANGLE), (f"model=2 half_angle={ABOVE_PI_F32}", FISHEYE_ANGLE),
    ("t_min=-1", T_MIN), ("t_min=-0x1p-149", T_MIN), ("t_min=nan", T_MIN), ("t_min=inf", T_MIN),
    ("t_max=nan", T_MAX), ("t_max=0", T_MAX), ("t_min=2 t_max=2", T_MAX), ("t_min=2 t_max=1", T_MAX), ("t_max=-inf", T_MAX),
    ("tone=0", TONE), ("tone=-1", TONE), ("tone=nan", TONE), ("tone=inf", TONE),
    ("seeds=0", NO_SEEDS),
    ("radiance=0 pixel=0", NO_OUTPUT),
    ("flags=1 radiance=0", ACCUMULATE_NEEDS_RADIANCE),
]


def test_every_refusal_that_needs_no_device(decide):
    got = decide([c for c, _ in REFUSALS])
    for (case, want), g in zip(REFUSALS, got):
        assert g[0] == want and g[1] == E_ARG, f"{case}: verdict {g[0]}, status {g[1]}; want verdict {want}, status {E_ARG}"


ACCEPTED = [
    "", "k=1", "k=16", "width=65535", "height=65535 nrows=1", "width=65535 height=65535 k=1",   # 4 294 836 225 rays <= 2^32 - 256
    "width=65535 height=65535 k=16 nrows=256",              # 4 294 901 760 rays = 2^32 - 65536
    "model=1", "model=2", f"model=2 half_angle={PI_F32}", "model=2 half_angle=0x1p-149", "t_max=inf", "t_min=0x1p-149 t_max=0x1p-148",
    "model=1 half_w=0 half_h=nan half_angle=nan",            # read by their own models only
    "model=2 half_w=-1", "pixel=0 tone=nan",                 # tone is read only when pixel is given
    "radiance=0", "flags=1", "flags=1 pixel=0", "row0=6 nrows=1", "row0=3 nrows=4",
    "forward0=0 forward1=0",                                 # a zero component is the exact kernel's business, not a refusal
]


def test_accepted_borders(decide):
    for case, g in zip(ACCEPTED, decide(ACCEPTED)):
        assert g[0] == OK and g[1] == 0, f"{case!r}: verdict {g[0]}, status {g[1]}"


def test_view_rays_reads_neither_the_buffers_nor_tone(decide):
    cases = ["rays_call=1 seeds=0 radiance=0 pixel=0 tone=nan", "rays_call=1 flags=1 radiance=0", "rays_call=1 flags=2", "rays_call=1 k=3"]
    got = decide(cases)
    assert [g[0] for g in got] == [OK, OK, FLAGS, SAMPLES]


def plan_of(width, rows, k):
    rpp = k * k
    pixels = width * rows
    rays = pixels * rpp
    ppb = 256 // rpp
    blocks = -(-rays // 256)
    last = pixels % ppb or ppb
    return (rows, rpp, pixels, rays, blocks, ppb, last, -(-blocks // 32))


@pytest.mark.parametrize("k", [1, 2, 4, 8, 16])
def test_plan_of_13_by_7(decide, k):
    (g,) = decide([f"k={k}"])
    assert g[2:] == plan_of(13, 7, k), (k, g)
    assert {1: (1, 256, 91), 2: (2, 64, 27), 4: (6, 16, 11), 8: (23, 4, 3), 16: (91, 1, 1)}[k] == (g[6], g[7], g[8])


def test_plan_of_tiles_one_pixel_and_many_blocks(decide):
    cases = {"width=1 height=1 k=1": (1, 1, 1), "width=1 height=1 k=16": (1, 1, 16), "row0=3 nrows=1 k=2": (13, 1, 2), "row0=4 nrows=3 k=2": (13, 3, 2),
             "width=65 height=1 k=2": (65, 1, 2), "width=1920 height=1080 k=2": (1920, 1080, 2), "width=65535 height=65535 k=16 nrows=256": (65535, 256, 16),
             "width=256 height=32 k=1": (256, 32, 1), "width=256 height=33 k=1": (256, 33, 1)}
    for (case, (w, rows, k)), g in zip(cases.items(), decide(list(cases))):
        assert g[0] == OK and g[2:] == plan_of(w, rows, k), (case, g)
    assert plan_of(1, 1, 1)[4:] == (1, 256, 1, 1) and plan_of(65, 1, 2)[4:] == (2, 64, 1, 1) and plan_of(256, 33, 1)[7] == 2
