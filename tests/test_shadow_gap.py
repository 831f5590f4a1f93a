"""CPU: the shadow stage's plane-free gap (csrc/pt_shadow_gap.hpp: the host's constants; csrc/pt_direct.hpp gap_test: the kernel's test).  A wave
whose shadow segments all pass the gap test of a single-cell triangle set skips the set's box test and every axis entry of its plane list, so a
pass must imply what those would have said.  tests/shadow_gap_check.c -- a stand-alone C program compiled here with the host compiler, once plain
and once with -fsanitize=address,undefined -- includes the product's header, restates the kernel's test, the reference's box test, cell exit and
interTriangle and the sweep's verdict with fmaf, and counts, over rooms like cornell.xml's and random axis-plane soups (several planes per axis,
planes on box faces, sets without axis planes; forty octaves of scale; segment ends at 0.5, 1, 17/16 and 2 margins, one to four representable steps
and 1e-3 from a plane; |d_a| down to 2^-40; segments aimed at a record of the gap's own end), the passing segments for which

    * the box does not give v, tmin == 0, tmax >= maxt and an exit >= maxt                          (box violations)
    * an axis-plane triangle, in either winding, is accepted by the reference with t < maxt          (triangle violations)
    * the sweep's verdict on an axis entry, front or back, is not "drop"                              (sweep keeps)

All three are zero at the product's margins.  With the margins cut the third one is not: that is what the margin is for (the first two cannot
tell for axis planes -- the reference's numerator of t is sign-exact there; shadow_gap_check.c's header says why)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "2015-raytracing_amd", "csrc")
FIELDS = ("cases", "passes", "violations", "box_violations", "triangle_violations", "sweep_keeps", "interior", "interior_passes", "skipped")


def _compile(tmp, name, extra):
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler to build tests/shadow_gap_check.c with")
    exe = str(tmp / name)
    subprocess.run([cc, "-std=c11", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", *extra, "-I", CSRC, os.path.join(ROOT, "tests", "shadow_gap_check.c"),
                    "-o", exe, "-lm"], check=True)

    def run(seed, cases, shrink=0):
        r = subprocess.run([exe, str(seed), str(cases), str(shrink)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, r.stderr
        out = dict(zip(FIELDS, map(int, r.stdout.split())))
        print(out)
        return out
    return run


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("shadow_gap"), "shadow_gap_check", ["-O2"])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_a_passing_segment_meets_no_axis_plane_and_stays_in_the_box(check, seed):
    r = check(seed, 12_000_000)
    assert r["cases"] == 12_000_000 and r["passes"] > 1_500_000, r      # the test fires, also on the adversarial placements
    assert r["box_violations"] == 0 and r["triangle_violations"] == 0 and r["sweep_keeps"] == 0 and r["violations"] == 0, r


def test_the_gap_test_fires_on_interior_segments_of_the_room(check):
    """Origins 0.001 off a surface of the cornell-like room, end points on the light's disk, all forty octaves: at least nine in ten pass.  (The ones
    that do not are the smallest rooms, where the sweep margin's absolute floor 2^-56 / |n_a| is wider than a thousandth of the room.)"""
    r = check(11, 4_000_000)
    assert r["interior"] > 400_000, r
    assert r["interior_passes"] >= 0.90 * r["interior"], r


def test_the_check_sees_a_margin_that_is_too_small(check):
    """The margins cut by 2^-10 -- the sweep margin's 128 u to an eighth of a rounding unit, as tests/test_sweep_filter.py cuts the sweep's own: the
    early-out would then skip axis entries whose verdict is not "drop"."""
    r = check(7, 4_000_000, shrink=10)
    assert r["sweep_keeps"] > 0 and r["violations"] > 0, r


def test_under_the_sanitizers(tmp_path):
    run = _compile(tmp_path, "shadow_gap_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = run(5, 300_000)
    assert r["cases"] == 300_000 and r["violations"] == 0, r
