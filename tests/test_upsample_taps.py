"""CPU: where the taps of mirt_upsample_guided lie (csrc/pt_upsample_taps.hpp), dumped by tests/upsample_taps_dump.cpp and compared with the
rule as include/mirt.h states it, in Python's own floor division: e = 2x + 1 - f, X0 = e // 2f (-1 at the left edge: C++ `/` truncates, which
is where this goes wrong), m = e % 2f.  Also: the weights the four taps get inside the image are those of plain bilinear interpolation between
low pixel centres, clamped at the border.  No device: the header is plain integer arithmetic."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from upsample_common import tap_axis

CSRC = os.path.join(ROOT, "2015-raytracing_amd", "csrc")
HEADER = os.path.join(CSRC, "pt_upsample_taps.hpp")
FACTORS = (2, 3, 4)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++ to compile tests/upsample_taps_dump.cpp with")
    exe = str(tmp_path_factory.mktemp("upsample_taps") / "upsample_taps_dump")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "upsample_taps_dump.cpp"), "-o", exe],
                   check=True)
    return subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()


def test_header_is_host_only():
    """nothing beyond <stdint.h>: it compiles alone, without a HIP header"""
    text = open(HEADER).read()
    includes = [l.split()[1] for l in text.splitlines() if l.startswith("#include")]
    assert includes == ["<stdint.h>"], includes
    assert "__device__" not in text and "__host__" not in text


def test_taps_are_floor_division(dump):
    rows = np.array([l.split() for l in dump if l[0].isdigit()], dtype=np.int64)
    assert len(rows) == sum(f * wl for f in FACTORS for wl in range(1, 10))
    seen_left_edge = 0
    for f, width, x, q0, m, nearest in rows:
        e = 2 * x + 1 - f
        assert (q0, m) == (e // (2 * f), e % (2 * f)), f"factor {f} width {width} x {x}: header ({q0}, {m}), Python ({e // (2 * f)}, {e % (2 * f)})"
        assert 0 <= m < 2 * f and -1 <= q0 <= width // f - 1
        assert nearest == x // f
        seen_left_edge += q0 == -1
    assert seen_left_edge > 0, "no x left of the first low centre was dumped"


def test_the_restatement_uses_the_same_taps(dump):
    rows = np.array([l.split() for l in dump if l[0].isdigit()], dtype=np.int64)
    for f in FACTORS:
        for wl in range(1, 10):
            sel = rows[(rows[:, 0] == f) & (rows[:, 1] == wl * f)]
            q0, m = tap_axis(wl * f, f)
            assert np.array_equal(sel[:, 3], q0) and np.array_equal(sel[:, 4], m)


def test_sizes_and_factors(dump):
    low = {(int(a), int(b)): int(c) for _, a, b, c in (l.split() for l in dump if l.startswith("low "))}
    for f in FACTORS:
        for n in range(41):
            assert low[(f, n)] == (n // f if n % f == 0 else 0), (f, n)
    ok = {int(a): int(b) for _, a, b in (l.split() for l in dump if l.startswith("factor_ok "))}
    assert ok == {0: 0, 1: 0, 2: 1, 3: 1, 4: 1, 5: 0, 6: 0}


@pytest.mark.parametrize("f", FACTORS)
def test_inside_weights_are_bilinear_clamped_at_the_border(dump, f):
    """High pixel x has its centre at x + 1/2, low pixel X at f * (X + 1/2).  Bilinear interpolation between low centres weighs X0 with 1 - t and
    X0 + 1 with t, t = the distance past X0's centre over f; left of the first and right of the last centre it clamps: all the weight on the
    border pixel.  The taps inside the image, renormalised (what the division by sumw does), are exactly that."""
    rows = np.array([l.split() for l in dump if l[0].isdigit()], dtype=np.int64)
    for wl in range(1, 10):
        sel = rows[(rows[:, 0] == f) & (rows[:, 1] == wl * f)]
        for _, _, x, q0, m, _ in sel:
            t = m / (2.0 * f)
            got = np.zeros(wl)
            for X, w in ((q0, 1.0 - t), (q0 + 1, t)):
                if 0 <= X < wl:
                    got[X] += w
            got /= got.sum()
            u = (x + 0.5) / f - 0.5                        # x's centre in low pixel units, low centres at the integers
            uc = min(max(u, 0.0), wl - 1.0)                # clamped to the span of the low centres
            want = np.zeros(wl)
            X = min(int(np.floor(uc)), wl - 1)
            want[X] += 1.0 - (uc - X)
            if uc - X > 0:
                want[X + 1] += uc - X
            assert np.allclose(got, want, atol=1e-12), f"factor {f} low width {wl} x {x}: {got} against {want}"
