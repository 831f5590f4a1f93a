"""CPU: the geometry-side guard of the optimistic kernel (csrc/pt_set_guard.hpp: fast_ok, walk_ok, exit_is_far_face, exit_far_axes, exit_up, delta,
rdelta per primitive set) and the windows it shares with the device code (csrc/pt_windows.hpp), asked through tests/set_guard_dump.cpp.  The oracle is
the rules restated in numpy.float32 -- IEEE round-to-nearest, independent of the C++ -- and every field is compared bit for bit (NaNs as one pattern):
each window's edge and its neighbours in every bound slot, generated bounds, and the sets of the committed scenes.  No device."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, bits

CSRC = os.path.join(ROOT, "2015-raytracing_amd", "csrc")
F = np.float32
SLOTS = (0, 1, 2, 4, 5, 6)                # the bound components the guard reads: (min, 1, max, 1)
NS = (1, 2, 3, 7, 16, 1024)
FIELDS = ("fast_ok", "walk_ok", "exit_is_far_face", "set_exit_is_far_face", "exit_far_axes", "exit_up", "delta", "rdelta")


def P(p):
    return F(2.0) ** F(p)


def f32(u):
    return np.asarray(u, dtype=np.uint32).view(F)


def u32(v):
    return np.ascontiguousarray(v, dtype=F).view(np.uint32)


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++ to compile tests/set_guard_dump.cpp with")
    exe = str(tmp_path_factory.mktemp("set_guard") / "set_guard_dump")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "set_guard_dump.cpp"), "-o", exe], check=True)

    def run(lines):
        """one answer (a row of ints) per question"""
        r = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, text=True, check=True)
        rows = r.stdout.splitlines()
        assert len(rows) == len(lines)
        return np.array([int(x, 16) for x in r.stdout.split()], dtype=np.int64).reshape(len(rows), -1)
    return run


def guard(ask, b, n, sane):
    """the header's answer for bounds b (N x 8 float32), slab counts n and `sane` flags, as a dict of arrays"""
    ub = u32(b)
    got = ask(["guard " + " ".join(f"{x:x}" for x in row) + f" {int(k):x} {int(s):x}" for row, k, s in zip(ub.tolist(), n, sane)])
    assert got.shape[1] == 14
    out = {name: got[:, i] for i, name in enumerate(FIELDS[:5])}
    for i, name in enumerate(FIELDS[5:]):
        out[name] = bits(f32(got[:, 5 + 3 * i:8 + 3 * i]))
    return out


def oracle(b, n, sane):
    """the rules, in numpy.float32"""
    b, n, sane = np.asarray(b, dtype=F), np.asarray(n, dtype=np.uint32), np.asarray(sane, dtype=bool)
    one, zero = F(1.0), F(0.0)
    position = lambda v: (v == 0) | ((np.abs(v) >= P(-30)) & (np.abs(v) <= P(20)))
    with np.errstate(all="ignore"):
        lo, hi = b[:, 0:3], b[:, 4:7]
        single = n == 1
        # n == 1: the reference's two exit planes of the one cell, lo + (0 + (d >= 0)) * ((hi - lo) / 1)
        width1 = (hi - lo) / one
        up, dn = lo + one * width1, lo + zero * width1
        up_is_hi, dn_is_lo = up == hi, (dn == lo).all(axis=1)
        fast = sane & position(b[:, SLOTS]).all(axis=1) & (lo <= hi).all(axis=1) & (~single | (position(up).all(axis=1) & dn_is_lo))
        far = single & up_is_hi.all(axis=1) & dn_is_lo & ~np.isnan(up).any(axis=1)
        span = hi - lo
        delta = span / n.astype(F)[:, None]
        rdelta = one / delta
        span_in = (span == 0) | ((np.abs(span) >= P(-60)) & (np.abs(span) <= P(60)))
        delta_in = (np.abs(delta) >= P(-40)) & (np.abs(delta) <= P(40))
    assert up.dtype == F and delta.dtype == F and rdelta.dtype == F
    return {"fast_ok": fast.astype(np.int64), "walk_ok": (span_in & delta_in).all(axis=1).astype(np.int64),
            "exit_is_far_face": far.astype(np.int64), "set_exit_is_far_face": far.astype(np.int64),
            "exit_far_axes": np.where(single, (up_is_hi * np.array([1, 2, 4])).sum(axis=1), 7),
            "exit_up": bits(np.where(single[:, None], up, hi)), "delta": bits(delta), "rdelta": bits(rdelta)}


def check(ask, b, n, sane):
    b = np.asarray(b, dtype=F).reshape(-1, 8)
    got, want = guard(ask, b, n, sane), oracle(b, n, sane)
    for name in FIELDS:
        bad = np.flatnonzero((got[name] != want[name]).reshape(len(b), -1).any(axis=1))
        assert bad.size == 0, f"{name} differs in {bad.size} of {len(b)} cases; the first: bounds {[hex(x) for x in u32(b[bad[0]])]}, n {n[bad[0]]}, sane {sane[bad[0]]}"
    return want


def edge_values():
    """each window's bounds with their neighbours on either side, and the ends of the format; both signs of each"""
    v = []
    for p in (-60, -40, -30, 20, 40, 60):
        v += [np.nextafter(P(p), F(0.0)), P(p), np.nextafter(P(p), F(np.inf))]
    v += [F(0.0), f32(1), np.finfo(F).max, F(np.inf), F(np.nan)]
    v = np.array(v, dtype=F)
    return np.concatenate([v, -v])


ORDINARY = np.array([-1.5, -2.25, -0.75, 1.0, 3.0, 1.5, 2.5, 1.0], dtype=F)


# ---- the headers ------------------------------------------------------------------------------------------------------------------------------
def test_headers_are_host_only():
    """pt_windows.hpp: nothing beyond <stdint.h>; pt_set_guard.hpp: <stdint.h>, <math.h> and the windows.  No HIP header, no qualifier"""
    want = {"pt_windows.hpp": ["<stdint.h>"], "pt_set_guard.hpp": ["<stdint.h>", "<math.h>", '"pt_windows.hpp"']}
    for name, includes in want.items():
        text = open(os.path.join(CSRC, name)).read()
        assert [l.split()[1] for l in text.splitlines() if l.startswith("#include")] == includes, name
        assert "__device__" not in text and "__host__" not in text, name


def test_windows_are_the_powers_of_two(ask):
    (got,) = ask(["windows"])
    powers = [int(u32(P(p))[0]) for p in (-40, 40, -30, 20, -60, 60, 21)]
    assert list(got) == powers + powers[:4]       # the floats, then the bit patterns ray_guard's integer form compares with


# ---- edges ------------------------------------------------------------------------------------------------------------------------------------
def test_each_edge_value_in_each_bound_slot(ask):
    b, n, sane = [], [], []
    for v in edge_values():
        for slot in SLOTS:
            for k in NS:
                for s in (True, False):
                    box = ORDINARY.copy()
                    box[slot] = v
                    b.append(box), n.append(k), sane.append(s)
    want = check(ask, b, n, sane)
    assert len(b) == 2 * 23 * 6 * 6 * 2
    for name in ("fast_ok", "walk_ok"):
        assert 0 < want[name].sum() < len(b), name


def test_window_edges_decide_as_stated(ask):
    """the verdicts at the edges spelled out, so that the oracle above cannot be wrong in the same way as the header"""
    def verdict(slot, v, k=2):
        box = ORDINARY.copy()
        box[slot] = v
        w = check(ask, box, [k], [True])
        return int(w["fast_ok"][0]), int(w["walk_ok"][0])
    up, down = lambda v: np.nextafter(F(v), F(np.inf)), lambda v: np.nextafter(F(v), F(0.0))
    assert verdict(4, P(20)) == (1, 1) and verdict(4, up(P(20))) == (0, 1)               # a bound: at most 2^20 ...
    assert verdict(4, P(-30)) == (1, 1) and verdict(4, down(P(-30))) == (0, 1)           # ... at least 2^-30 ...
    assert verdict(4, F(0.0)) == (1, 1) and verdict(0, F(-0.0)) == (1, 1)                 # ... or zero
    assert verdict(0, -P(20)) == (1, 1) and verdict(0, -up(P(20))) == (0, 1)             # the windows are on the magnitude
    assert verdict(4, P(60), k=1024) == (0, 0)                                           # span 2^60 is in, delta 2^50 is out
    assert verdict(4, P(40), k=1) == (0, 1) and verdict(4, up(P(40)), k=1) == (0, 0)     # delta: at most 2^40
    assert verdict(4, F(np.nan)) == (0, 0) and verdict(0, F(-np.inf)) == (0, 0)
    # with n <= 1024 the width's window is the tighter one: a span at its own lower edge, over one slab, is refused through the width
    box = ORDINARY.copy()
    box[0], box[4] = F(0.0), P(-60)
    assert check(ask, box, [1], [True])["walk_ok"][0] == 0                               # span in [2^-60, 2^60], delta 2^-60 below 2^-40


def test_inverted_and_zero_width_axes(ask):
    b, n, sane, tag = [], [], [], []
    for axis in range(3):
        for k in NS:
            inv, flat = ORDINARY.copy(), ORDINARY.copy()
            inv[axis], inv[4 + axis] = ORDINARY[4 + axis], ORDINARY[axis]
            flat[4 + axis] = flat[axis]
            b += [inv, flat]
            n += [k, k]
            sane += [True, True]
            tag += ["inverted", "flat"]
    want = check(ask, b, n, sane)
    for i, t in enumerate(tag):
        # an inverted axis refuses the optimistic kernel; a zero-width one keeps it (lo <= hi holds) but its slab width of zero refuses the walk
        assert want["fast_ok"][i] == (0 if t == "inverted" else 1), (t, n[i])
        assert want["walk_ok"][i] == (1 if t == "inverted" else 0), (t, n[i])


# ---- generated bounds -------------------------------------------------------------------------------------------------------------------------
def generated(count, seed):
    """four families in equal parts: every slot an edge value; values spread over +-45 octaves; ordinary scene-sized boxes (half of them on a grid
    of eighths, whose exit planes are exact); ordinary boxes with one edge value.  n == 1 on two of seven draws, insane records on one of eight."""
    rng = np.random.default_rng(seed)
    edges = edge_values()
    quarter = count // 4
    b = np.ones((4 * quarter, 8), dtype=F)
    six = np.array(SLOTS)

    def ordinary(m):
        centre, half = rng.uniform(-8.0, 8.0, size=(m, 3)), rng.uniform(0.05, 6.0, size=(m, 3))
        box = np.concatenate([centre - half, centre + half], axis=1)
        round_ones = rng.random(m) < 0.5
        box[round_ones] = np.round(box[round_ones] * 8.0) / 8.0
        return box.astype(F)

    b[0 * quarter:1 * quarter, six] = edges[rng.integers(0, len(edges), size=(quarter, 6))]
    wide = np.exp2(rng.uniform(-45.0, 45.0, size=(quarter, 6))) * rng.choice([-1.0, 1.0], size=(quarter, 6))
    wide.sort(axis=1)          # lo <= hi on every axis: neighbours in the order make an axis
    b[1 * quarter:2 * quarter, six] = wide[:, [0, 2, 4, 1, 3, 5]].astype(F)
    b[2 * quarter:3 * quarter, six] = ordinary(quarter)
    one_edge = ordinary(quarter)
    one_edge[np.arange(quarter), rng.integers(0, 6, size=quarter)] = edges[rng.integers(0, len(edges), size=quarter)]
    b[3 * quarter:4 * quarter, six] = one_edge
    n = np.array((1, 1) + NS[1:], dtype=np.uint32)[rng.integers(0, 7, size=len(b))]
    sane = rng.random(len(b)) >= 0.125
    return b, n, sane


def test_generated_bounds(ask):
    b, n, sane = generated(200_000, 20261)
    assert len(b) >= 200_000
    want = check(ask, b, n, sane)
    for name in ("fast_ok", "walk_ok", "exit_is_far_face"):
        share = want[name].mean()
        assert 0.01 <= share <= 0.99, f"{name} is taken in {share:.1%} of the cases: the generator no longer reaches both branches"
    assert set(np.unique(want["exit_far_axes"])) == set(range(8))


# ---- the committed scenes ---------------------------------------------------------------------------------------------------------------------
ANCHORS = [   # (fixture, bounds, fast_ok, walk_ok, exit_is_far_face, exit_far_axes) with n_slabs = 1, computed with the code this header replaced
    ("cornell_32x24_r4", "sphere_bounds", 1, 1, 0, 0),        # misses hi by one ulp on all three
    ("cornell_32x24_r4", "triangle_bounds", 1, 1, 1, 7),
    ("cornell_teapot3_32x24_r4", "sphere_bounds", 1, 1, 0, 6),
    ("own_studio_48x36_r4", "sphere_bounds", 1, 1, 0, 3),
    ("own_gems_48x36_r4", "sphere_bounds", 1, 1, 0, 5),
    ("basic_32x24_r4", "sphere_bounds", 1, 1, 1, 7),
    ("triangles_32x24_r4", "triangle_bounds", 1, 1, 0, 6),
]


@pytest.mark.parametrize("fixture,which,fast,walk,far,axes", ANCHORS)
def test_sets_of_the_committed_scenes(ask, fixture, which, fast, walk, far, axes):
    scene = json.loads(bytes(np.load(os.path.join(GOLDEN, fixture + ".npz"))["scene_json"]).decode())
    want = check(ask, np.array(scene[which], dtype=F), [1], [True])
    assert (want["fast_ok"][0], want["walk_ok"][0], want["exit_is_far_face"][0], want["exit_far_axes"][0]) == (fast, walk, far, axes)
