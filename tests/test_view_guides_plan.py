"""CPU: what csrc/pt_view_plan.hpp decides for mirt_view_guides and mirt_render_view_guided, dumped by tests/view_guides_plan_dump.cpp -- a plain
C++ program, no device: the two calls' verdicts (the descriptor checks of mirt_view_rays, then an output; the frame's rules first for the guided
call), the route rule over every k, grids on and off, the switch on and off, and the one-lane-per-pixel plan against plain integer arithmetic."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "2015-raytracing_amd", "csrc")
E_ARG = -1
(OK, STRUCT_SIZE, MODEL, FLAGS, SAMPLES, EXTENT, TILE, TILE_RAYS, BASIS, ORTHO_WINDOW, FISHEYE_ANGLE, T_MIN, T_MAX, TONE, NO_SEEDS, NO_OUTPUT,
 ACCUMULATE_NEEDS_RADIANCE, NO_GUIDE) = range(18)


@pytest.fixture(scope="module")
def decide(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "no g++ to compile tests/view_guides_plan_dump.cpp with"
    exe = str(tmp_path_factory.mktemp("view_guides_plan") / "view_guides_plan_dump")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "view_guides_plan_dump.cpp"), "-o", exe], check=True)

    def run(cases):
        out = subprocess.run([exe], input="".join(c + "\n" for c in cases), stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
        assert len(out) == len(cases)
        return [tuple(int(t) for t in l.split()) for l in out]
    return run


# case -> (mirt_view_guides's verdict, mirt_render_view_guided's)
VERDICTS = [
    ("", OK, OK), ("nh=0", OK, OK), ("ad=0", OK, OK), ("k=1", OK, OK), ("k=16", OK, OK),
    ("nh=0 ad=0", NO_GUIDE, NO_GUIDE),
    # the descriptor checks of mirt_view_rays come first in both
    ("struct_size=100", STRUCT_SIZE, STRUCT_SIZE), ("model=3", MODEL, MODEL), ("flags=2", FLAGS, FLAGS), ("k=3", SAMPLES, SAMPLES), ("k=32", SAMPLES, SAMPLES),
    ("width=0", EXTENT, EXTENT), ("row0=7", TILE, TILE), ("width=65535 height=65535 k=2", TILE_RAYS, TILE_RAYS), ("forward0=nan", BASIS, BASIS),
    ("half_w=0", ORTHO_WINDOW, ORTHO_WINDOW), ("model=2 half_angle=0", FISHEYE_ANGLE, FISHEYE_ANGLE), ("t_min=-1", T_MIN, T_MIN), ("t_max=0", T_MAX, T_MAX),
    ("k=3 nh=0 ad=0", SAMPLES, SAMPLES),
    # the guides read neither tone, the meaning of flags nor the frame's buffers; the guided frame does
    ("tone=nan", OK, TONE), ("tone=0", OK, TONE), ("tone=nan pixel=0", OK, OK), ("seeds=0", OK, NO_SEEDS), ("radiance=0 pixel=0", OK, NO_OUTPUT),
    ("flags=1", OK, OK), ("flags=1 radiance=0", OK, ACCUMULATE_NEEDS_RADIANCE),
    # ... and its rules come before the guides'
    ("seeds=0 nh=0 ad=0", NO_GUIDE, NO_SEEDS), ("tone=nan nh=0 ad=0", NO_GUIDE, TONE),
]


def test_verdicts_of_both_calls(decide):
    for (case, want_a, want_b), g in zip(VERDICTS, decide([c for c, _a, _b in VERDICTS])):
        assert (g[0], g[2]) == (want_a, want_b), f"{case!r}: verdicts {g[0]}, {g[2]}; want {want_a}, {want_b}"
        assert g[1] == (0 if want_a == OK else E_ARG) and g[3] == (0 if want_b == OK else E_ARG), (case, g)


@pytest.mark.parametrize("env", [1, 0])
@pytest.mark.parametrize("grids", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 4, 8, 16])
def test_route_rule(decide, k, grids, env):
    """one launch where a pixel's samples are consecutive lanes of one wave (rpp 1, 4, 16, 64) and the switch is on; never at k = 16"""
    (g,) = decide([f"k={k} grids={grids} env={env}"])
    assert g[4] == int(env == 1 and k in (1, 2, 4, 8)), (k, grids, env, g)


def test_route_rule_reads_nothing_but_its_arguments(decide):
    got = decide(["k=2", "k=2 model=1 width=1920 height=1080", "k=2 nh=0", "k=2 flags=1", "k=16 width=1 height=1"])
    assert [g[4] for g in got] == [1, 1, 1, 1, 0]


def test_plan_of_one_lane_per_pixel(decide):
    cases = {"": 91, "k=16": 91, "width=1 height=1 k=1": 1, "width=65 height=1": 65, "width=37 height=21": 777, "width=256 height=1": 256, "width=257 height=1": 257,
             "row0=3 nrows=1": 13, "width=1920 height=1080": 1920 * 1080, "width=32 height=1": 32, "width=33 height=1": 33}
    for (case, pixels), g in zip(cases.items(), decide(list(cases))):
        assert g[0] == OK and g[5:] == (-(-pixels // 256), -(-pixels // 32)), (case, g)
    assert decide(["width=37 height=21"])[0][5:] == (4, 25)   # four blocks (the last of 9 lanes), 25 words of a bit per pixel
    assert decide(["k=3"])[0][5:] == (0, 0)
