"""CPU: what csrc/pt_view_plan.hpp decides for mirt_view_guides_batch, mirt_view_ao_batch and mirt_render_view_guided_batch, dumped by
tests/view_batch_aov_plan_dump.cpp -- a plain C++ program, no device: every verdict of view_check_guides_batch, view_check_ao_batch and
view_check_render_guided_batch; the batch's rules come before each call's own, and those in the single call's order; the descriptor's own
basis being NaN is no refusal while a NaN in any of a camera's twelve slots is, naming the frame; and the per-pixel plan of the stacked image
against plain integer arithmetic."""
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


@pytest.fixture(scope="module")
def decide(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "no g++ to compile tests/view_batch_aov_plan_dump.cpp with"
    exe = str(tmp_path_factory.mktemp("view_batch_aov_plan") / "view_batch_aov_plan_dump")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "view_batch_aov_plan_dump.cpp"), "-o", exe], check=True)

    def run(cases):
        out = subprocess.run([exe], input="".join(c + "\n" for c in cases), stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
        assert len(out) == len(cases)
        return [tuple(int(t) for t in l.split()) for l in out]
    return run


def verdicts(decide, table):
    """table: (case, guides verdict, AO verdict, guided verdict)"""
    for (case, *want), g in zip(table, decide([row[0] for row in table])):
        assert [g[0], g[2], g[4]] == want, f"{case!r}: verdicts {g[0]}, {g[2]}, {g[4]}; want {want}"
        assert [g[1], g[3], g[5]] == [0 if w == OK else E_ARG for w in want], (case, g)


def same(case, v):
    return (case, v, v, v)


def test_every_verdict(decide):
    verdicts(decide, [
        same("", OK), same("n=1", OK), same("n=0", OK), same("n=0 cameras=0", OK), same("nrows=7", OK), same("k=16", OK), same("k=1", OK), same("model=0", OK),
        same("model=2", OK),
        # the batch's rules: view_check_batch's, for all three
        same("struct_size=100", STRUCT_SIZE), same("model=3", MODEL), same("flags=2", FLAGS), same("k=3", SAMPLES), same("width=0", EXTENT), same("height=65536", EXTENT),
        same("row0=1", BATCH_TILE), same("nrows=3", BATCH_TILE), same("width=4096 height=4096 k=1 n=256", BATCH_RAYS), same("cameras=0", BATCH_NO_CAMERAS),
        same("cam1.0=nan", BATCH_CAMERA), same("cam2.11=inf", BATCH_CAMERA), same("model=0 half_w=0", ORTHO_WINDOW), same("model=2 half_angle=0", FISHEYE_ANGLE),
        same("t_min=-1", T_MIN), same("t_max=0", T_MAX),
        # each call's own
        ("nh=0", OK, OK, OK), ("ad=0", OK, OK, OK), ("nh=0 ad=0", NO_GUIDE, OK, NO_GUIDE),
        ("ao_size=12", OK, AO_STRUCT_SIZE, OK), ("ao_samples=0", OK, AO_SAMPLES, OK), ("ao_samples=65", OK, AO_SAMPLES, OK), ("ao_samples=64", OK, OK, OK),
        ("ao_samples=1", OK, OK, OK), ("ao_radius=0", OK, AO_RADIUS, OK), ("ao_radius=nan", OK, AO_RADIUS, OK), ("ao_radius=inf", OK, OK, OK),
        ("ao_bias=-1", OK, AO_BIAS, OK), ("ao_bias=nan", OK, AO_BIAS, OK), ("ao_bias=inf", OK, AO_BIAS, OK), ("ao_bias=0", OK, OK, OK),
        ("ao_seeds=0", OK, AO_NO_SEEDS, OK), ("ao_out=0", OK, AO_NO_OUTPUT, OK),
        ("tone=nan", OK, OK, TONE), ("tone=0", OK, OK, TONE), ("tone=nan pixel=0", OK, OK, OK), ("seeds=0", OK, OK, NO_SEEDS), ("radiance=0 pixel=0", OK, OK, NO_OUTPUT),
        ("flags=1", OK, OK, OK), ("flags=1 radiance=0", OK, OK, ACCUMULATE_NEEDS_RADIANCE),
        # the guides and AO calls read neither tone nor the meaning of flags
        ("tone=nan flags=1 radiance=0 seeds=0", OK, OK, TONE),
    ])


def test_the_batchs_rules_come_before_each_calls_own(decide):
    own = "nh=0 ad=0 ao_size=12 ao_samples=0 ao_radius=0 ao_bias=-1 ao_seeds=0 ao_out=0 tone=nan seeds=0 radiance=0 pixel=0"
    chain = [("struct_size=100", STRUCT_SIZE), ("model=3", MODEL), ("flags=2", FLAGS), ("k=3", SAMPLES), ("width=0", EXTENT), ("row0=1", BATCH_TILE),
             ("n=40000000", BATCH_RAYS), ("cameras=0", BATCH_NO_CAMERAS), ("cam2.5=nan", BATCH_CAMERA), ("t_min=-1", T_MIN), ("t_max=-2", T_MAX)]
    cases = [" ".join(c for c, _v in chain[i:]) + " " + own for i in range(len(chain))]
    for (case, (_c, want)), g in zip(zip(cases, chain), decide(cases)):
        assert (g[0], g[2], g[4]) == (want, want, want), (case, g, want)
    got = decide(["model=0 cam0.0=nan half_w=0 " + own, "model=0 half_w=0 " + own, "model=2 half_angle=4 " + own])
    assert [(g[0], g[2], g[4]) for g in got] == [(BATCH_CAMERA,) * 3, (ORTHO_WINDOW,) * 3, (FISHEYE_ANGLE,) * 3]


def test_each_calls_own_rules_keep_the_single_calls_order(decide):
    # mirt_view_ao: descriptor size, samples, radius, bias, seeds, ao_out
    chain = [("ao_size=12", AO_STRUCT_SIZE), ("ao_samples=0", AO_SAMPLES), ("ao_radius=-1", AO_RADIUS), ("ao_bias=nan", AO_BIAS), ("ao_seeds=0", AO_NO_SEEDS),
             ("ao_out=0", AO_NO_OUTPUT)]
    cases = [" ".join(c for c, _v in chain[i:]) for i in range(len(chain))]
    for (case, (_c, want)), g in zip(zip(cases, chain), decide(cases)):
        assert g[2] == want and g[0] == OK and g[4] == OK, (case, g, want)
    # mirt_render_view_guided: the frame's rules (tone, seeds, an output, accumulate) and then the guides'
    # (tone is read only with a pixel buffer, so the chain with both outputs missing starts behind it)
    chain = [("seeds=0", NO_SEEDS), ("radiance=0 pixel=0", NO_OUTPUT), ("nh=0 ad=0", NO_GUIDE)]
    cases = [" ".join(c for c, _v in chain[i:]) for i in range(len(chain))]
    for (case, (_c, want)), g in zip(zip(cases, chain), decide(cases)):
        assert g[4] == want, (case, g, want)
    (g,) = decide(["tone=nan seeds=0 radiance=0 nh=0 ad=0"])
    assert g[4] == TONE
    (g,) = decide(["flags=1 radiance=0 nh=0 ad=0"])
    assert g[4] == ACCUMULATE_NEEDS_RADIANCE and g[0] == NO_GUIDE


def test_the_descriptors_own_basis_is_neither_read_nor_checked(decide):
    cases = [f"basis{s}={v}" for s in range(12) for v in ("nan", "inf")]
    for case, g in zip(cases, decide(cases)):
        assert (g[0], g[2], g[4]) == (OK, OK, OK), (case, g)


@pytest.mark.parametrize("value", ["nan", "inf", "-inf"])
def test_a_camera_with_a_non_finite_slot_is_refused_and_named(decide, value):
    cases = [f"n=5 cam{f}.{s}={value}" for f in (0, 3, 4) for s in range(12)]
    for case, g in zip(cases, decide(cases)):
        f = int(case.split("cam")[1].split(".")[0])
        assert (g[0], g[2], g[4]) == (BATCH_CAMERA,) * 3 and g[6:9] == (f, f, f), (case, g)
    (g,) = decide([f"n=5 cam3.2={value} cam1.7={value}"])
    assert g[6:9] == (1, 1, 1), "the first bad frame is the one named"
    (g,) = decide([f"n=3 cam3.2={value}"])
    assert (g[0], g[2], g[4]) == (OK, OK, OK) and g[6:9] == (-1, -1, -1), "a camera past n_frames is not read"


# N * P not a multiple of 256 or of 32 (273, 45, 5, 6), a multiple of both (512), N * height above 65535, no frames
PLANS = [(13, 7, 2, 3), (5, 3, 2, 3), (16, 16, 1, 2), (1, 1, 1, 5), (3, 1, 16, 2), (1, 1, 1, 64), (32, 16, 2, 1024), (1, 65535, 1, 2), (2, 40000, 2, 3),
         (1, 50, 1, 4000), (7, 3, 4, 0), (65535, 1, 1, 4000), (3, 5, 8, 17), (1, 1, 1, 257), (1, 1, 1, 33), (4096, 4096, 1, 255)]


@pytest.mark.parametrize("w,h,k,n", PLANS)
def test_the_pixel_plan_is_plain_integer_arithmetic(decide, w, h, k, n):
    (g,) = decide([f"width={w} height={h} k={k} n={n}"])
    pixels = n * w * h
    assert (g[0], g[2], g[4]) == (OK, OK, OK)
    assert g[9:13] == (n * h, pixels, -(-pixels // 256), -(-pixels // 32)), g


def test_no_frames_plan_nothing(decide):
    got = decide(["n=0", "n=0 cameras=0", "n=0 width=65535 height=65535 k=1"])
    assert all(g[9:13] == (0, 0, 0, 0) and (g[0], g[2], g[4]) == (OK, OK, OK) for g in got), got


def test_the_guided_batchs_route(decide):
    """one launch where a pixel's samples are lanes of one wave, in both scene families; two at k = 16 and with MIRT_GUIDED_VIEW=0"""
    cases = [f"k={k} grids={g} env={e}" for k in (1, 2, 4, 8, 16) for g in (0, 1) for e in (0, 1)]
    for case, got in zip(cases, decide(cases)):
        k, _g, e = (int(t.split("=")[1]) for t in case.split())
        assert got[13] == int(e == 1 and k != 16), (case, got)
