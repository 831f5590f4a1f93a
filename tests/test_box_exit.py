"""CPU: the one slab pass of a single-cell set whose exit planes are not the box's far faces (csrc/pt_trace.hpp box_exit1; the host's constant and the
derivation: csrc/pt_box_exit.hpp).  It gives the box verdict and the cell's exit t from six quotients where inter_aabb_t and cell1_exit form nine:
"meets the box" is read off tmin <= EXIT, and a lane whose window is shorter than the host's bound takes the box's own comparison on the axes whose
exit plane lies above hi.  tests/box_exit_check.c -- a stand-alone C program compiled here with the host compiler, once plain and once with
-fsanitize=address,undefined -- includes the product's header, restates both forms with fmaf and counts, over generated boxes (the exit plane below,
on and above hi on each axis: all 27 combinations) and several million rays per run (random ones, rays aimed within three representable steps of box
edges and corners, rays starting within three steps of a far face or exit plane, direction components down to 2^-40):

    * tmin or the exit differing from the two-function form as floats                                    (bit mismatches: zero)
    * final verdicts that differ where the reference's window [tmin, exit] is not empty                   (violations: zero)
    * the lanes that take the box's comparison, and those it drops                                         (stated; no lane defers)

With the host's bound cut to nothing the second count is not zero: that is what it is for."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "2015-raytracing_amd", "csrc")
FIELDS = ("cases", "skipped", "both_true", "differ", "overruled", "bit_mismatches", "violations", "close", "ordinary", "ordinary_overruled", "combos")


def _compile(tmp, name, extra):
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler to build tests/box_exit_check.c with")
    exe = str(tmp / name)
    subprocess.run([cc, "-std=c11", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", *extra, "-I", CSRC, os.path.join(ROOT, "tests", "box_exit_check.c"),
                    "-o", exe, "-lm"], check=True)

    def run(seed, cases, shrink=0):
        r = subprocess.run([exe, str(seed), str(cases), str(shrink)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, r.stderr
        out = dict(zip(FIELDS, map(int, r.stdout.split())))
        print(out, "share of lanes that take the box's comparison %.3g" % (out["close"] / max(out["cases"] - out["skipped"], 1)))
        return out
    return run


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("box_exit"), "box_exit_check", ["-O2"])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_one_pass_gives_the_two_functions_bits_and_the_boxes_verdict(check, seed):
    r = check(seed, 6_000_000)
    assert r["cases"] == 6_000_000 and r["skipped"] < 200_000 and r["combos"] == 27, r
    assert r["both_true"] > 1_500_000 and r["overruled"] > 10_000, r   # the adversarial placements reach the place where the verdicts part
    assert r["bit_mismatches"] == 0 and r["violations"] == 0, r
    assert r["ordinary"] > 10_000 and r["ordinary_overruled"] * 1000 < r["ordinary"], r


def test_the_check_sees_a_bound_that_is_too_small(check):
    """the bound times 2^-60: lanes between the box's far face and the exit plane keep tmin <= exit as their verdict, and some of those the reference drops"""
    r = check(3, 6_000_000, shrink=60)
    assert r["bit_mismatches"] == 0 and r["violations"] > 0, r


def test_under_the_sanitizers(tmp_path):
    run = _compile(tmp_path, "box_exit_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = run(5, 300_000)
    assert r["cases"] == 300_000 and r["bit_mismatches"] == 0 and r["violations"] == 0, r


def test_the_guard_and_the_constants_agree_on_the_axes(tmp_path):
    """pt_set_guard.hpp states the relation of the exit planes to hi (exit_above_axes), box_exit_consts makes the constants from the guard's exit planes:
    the same axes for n == 1, nothing for a grid.  cornell.xml's sphere box: above hi on x and y"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no C++ compiler")
    src = tmp_path / "dump.cpp"
    src.write_text('#include <stdio.h>\n#include <string.h>\n#include "pt_set_guard.hpp"\n#include "pt_box_exit.hpp"\n'
                   'static unsigned bits(float f) { unsigned u; memcpy(&u, &f, 4); return u; }\n'
                   'int main() { const float b[8] = {-0.4f, -1.0f, -0.4f, 1.0f, 0.7f, -0.4f, 0.5f, 1.0f};\n'
                   '  for (unsigned n = 1; n <= 2; ++n) { const pt::SetGuard g = pt::set_guard(b, n, true); const pt::BoxExit e = pt::box_exit_consts(b, g.exit_up);\n'
                   '    printf("%u %x %x %x %x %x %x\\n", g.fast_ok, g.exit_above_axes, e.above, bits(e.gap[0]), bits(e.gap[1]), bits(e.gap[2]), bits(e.gap_max)); }\n'
                   '  return 0; }\n')
    exe = str(tmp_path / "dump")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-O1", "-I", CSRC, str(src), "-o", exe], check=True)
    single, grid = (l.split() for l in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines())
    assert single[:3] == ["1", "3", "3"], single
    gx, gy, gz, gmax = (int(w, 16) for w in single[3:7])
    assert gx > 0 and gy > 0 and gz == 0 and gmax == max(gx, gy), single         # (positive floats order as their bits)
    assert grid[1:7] == ["0"] * 6, grid
