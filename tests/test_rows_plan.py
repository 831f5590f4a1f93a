"""CPU: the row arithmetic of the post-process stage in row tiles (csrc/pt_rows_plan.hpp), asked through tests/rows_plan_dump.cpp and compared with
Python's own restatement, exhaustively over heights 1 .. 40, 1 .. 9 tiles of mirt_tile_rows's rule, iterations 0 .. 5 and factors 2 .. 4: the
halo, the filter's window and its shrinking bands, the upsampler's low window, the argument rules of the two _rows calls, and the exchange plan
-- windows over three and more owners, empty tiles, absent windows, windows clamped at both image edges -- with every refusal.  No device: the
header is plain integers."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "2015-raytracing_amd", "csrc")
HEADER = os.path.join(CSRC, "pt_rows_plan.hpp")
HEIGHTS, TILES, ITERATIONS, FACTORS = range(1, 41), range(1, 10), range(0, 6), (2, 3, 4)
OK, EMPTY, OUTSIDE, SHORT = 0, 1, 2, 3
PLAN_OK, OWNERS_OVERLAP, ROW_UNOWNED = 0, 1, 2


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++ to compile tests/rows_plan_dump.cpp with")
    exe = str(tmp_path_factory.mktemp("rows_plan") / "rows_plan_dump")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "rows_plan_dump.cpp"), "-o", exe], check=True)

    def run(lines):
        """one answer (a list of ints) per question"""
        r = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, text=True, check=True)
        out = [[int(x) for x in l.split()] for l in r.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return run


# ---- Python's own restatement -------------------------------------------------------------------------------------------------------------------
def tile_rows(height, n, i):
    """mirt_tile_rows's rule: the first height % n tiles take the extra row"""
    q, r = divmod(height, n)
    return i * q + min(i, r), q + (1 if i < r else 0)


def halo(iterations):
    return 2 * (2 ** iterations - 1)


def filter_window(height, row0, nrows, iterations):
    if nrows == 0 or iterations > 5 or row0 + nrows > height:
        return 0, 0
    lo, hi = max(0, row0 - halo(iterations)), min(height, row0 + nrows + halo(iterations))
    return lo, hi - lo


def filter_band(win0, wn, row0, nrows, iterations, i):
    reach = halo(iterations) if i >= iterations else 2 * (2 ** iterations - 2 ** (i + 1))
    lo, hi = max(win0, row0 - reach), min(win0 + wn, row0 + nrows + reach)
    return lo, hi - lo


def low_window(height, f, row0, nrows):
    if f not in FACTORS or nrows == 0 or height % f or height > 65535 or row0 + nrows > height:
        return 0, 0
    y0 = lambda y: (2 * y + 1 - f) // (2 * f)       # Python's // is floor division
    lo, hi = max(0, y0(row0)), min(height // f, y0(row0 + nrows - 1) + 2)
    return lo, hi - lo


def contains(row0, nrows, need):
    return row0 <= need[0] and need[0] + need[1] <= row0 + nrows


def filter_check(height, w0, wn, row0, nrows, iterations):
    if nrows == 0 or wn == 0:
        return EMPTY
    if row0 + nrows > height or w0 + wn > height:
        return OUTSIDE
    return OK if contains(w0, wn, filter_window(height, row0, nrows, iterations)) else SHORT


def upsample_check(height, f, row0, nrows, l0, ln):
    if nrows == 0 or ln == 0:
        return EMPTY
    hl = height // f if f and height % f == 0 else 0
    if row0 + nrows > height or l0 + ln > hl:
        return OUTSIDE
    return OK if contains(l0, ln, low_window(height, f, row0, nrows)) else SHORT


def plan(src, dst):
    """row by row: (verdict, at, copies) for owners src[i] = (row0, nrows) and windows dst[i] = (row0, nrows)"""
    owner = {}
    for i, (r0, n) in enumerate(src):
        for r in range(r0, r0 + n):
            if r in owner:
                return OWNERS_OVERLAP, i, []
            owner[r] = i
    copies = []
    for d, (r0, n) in enumerate(dst):
        for r in range(r0, r0 + n):
            if r not in owner:
                return ROW_UNOWNED, d, []
            s = owner[r]
            last = copies[-1] if copies else None
            if last and last[0] == s and last[2] == d and last[1] + last[4] == r - src[s][0]:
                last[4] += 1
            else:
                copies.append([s, r - src[s][0], d, r - r0, 1])
    return PLAN_OK, 0, copies


def plan_question(src, dst):
    return f"plan {len(src)} " + " ".join(f"{s[0]} {s[1]} {d[0]} {d[1]}" for s, d in zip(src, dst))


def plan_answer(got):
    return got[0], got[1], [got[3 + 5 * k:8 + 5 * k] for k in range(got[2])]


# ---- the tests ----------------------------------------------------------------------------------------------------------------------------------
def test_header_is_host_only():
    """<stddef.h>, <stdint.h>, <vector> and the tap header, itself host-only: it compiles alone, without a HIP header"""
    text = open(HEADER).read()
    includes = [l.split()[1] for l in text.splitlines() if l.startswith("#include")]
    assert includes == ["<stddef.h>", "<stdint.h>", "<vector>", '"pt_upsample_taps.hpp"'], includes
    assert "__device__" not in text and "__host__" not in text


def test_halo(ask):
    got = ask([f"halo {i}" for i in ITERATIONS])
    assert [g[0] for g in got] == [halo(i) for i in ITERATIONS] == [0, 2, 6, 14, 30, 62]


def test_filter_windows_and_bands_of_every_tiling(ask):
    cases, bands = [], []
    for h in HEIGHTS:
        for n in TILES:
            for t in range(n):
                r0, nr = tile_rows(h, n, t)
                for it in ITERATIONS:
                    cases.append((h, r0, nr, it))
                    w = filter_window(h, r0, nr, it)
                    if nr:
                        bands += [(w[0], w[1], r0, nr, it, i) for i in range(it + 1)]
                        bands.append((0, h, r0, nr, it, 0))        # a larger window: the whole image
    got = ask([f"fwin {h} {r0} {nr} {it}" for h, r0, nr, it in cases])
    clamped = set()
    for c, g in zip(cases, got):
        want = filter_window(*c)
        assert tuple(g) == want, c
        if c[2]:
            clamped.add((want[0] == 0 and c[1] < halo(c[3]), want[0] + want[1] == c[0] and c[1] + c[2] + halo(c[3]) > c[0]))
    assert clamped == {(False, False), (True, False), (False, True), (True, True)}
    got = ask([f"band {' '.join(map(str, b))}" for b in bands])
    for b, g in zip(bands, got):
        assert tuple(g) == filter_band(*b), b
        w0, wn, r0, nr, it, i = b
        lo, n = g
        assert w0 <= lo <= r0 and r0 + nr <= lo + n <= w0 + wn, b      # inside the window, around the own rows
        if i + 1 == it:
            assert (lo, n) == (r0, nr), b                                # the last iteration computes the own rows alone


def test_bad_rows_give_an_empty_window(ask):
    cases = [(10, 0, 0, 1), (10, 8, 3, 1), (10, 11, 1, 0), (10, 0, 10, 6), (0, 0, 0, 0), (2 ** 32 - 1, 2 ** 32 - 2, 2, 1)]
    got = ask([f"fwin {h} {r0} {n} {it}" for h, r0, n, it in cases])
    assert all(g == [0, 0] for g in got), got
    cases = [(12, 1, 0, 4), (12, 5, 0, 4), (12, 3, 0, 0), (12, 3, 10, 3), (13, 3, 0, 4), (65538, 2, 0, 4), (0, 2, 0, 0), (12, 0, 0, 4)]
    got = ask([f"uwin {h} {f} {r0} {n}" for h, f, r0, n in cases])
    assert all(g == [0, 0] for g in got), got
    assert ask(["fwin 4294967295 4294967290 5 5", "uwin 65535 3 65530 5"]) == [[4294967290 - 62, 67], list(low_window(65535, 3, 65530, 5))] == [[4294967228, 67], [21843, 2]]


def test_upsample_low_windows_of_every_tiling(ask):
    cases = [(h, f, *tile_rows(h, n, t)) for h in HEIGHTS for f in FACTORS for n in TILES for t in range(n)]
    got = ask([f"uwin {h} {f} {r0} {nr}" for h, f, r0, nr in cases])
    seen = set()
    for c, g in zip(cases, got):
        want = low_window(*c)
        assert tuple(g) == want, c
        h, f, r0, nr = c
        if want[1]:
            # the rows the definition reads: Y0, Y0 + 1 and y div f, inside the low image
            rows = {q for y in range(r0, r0 + nr) for q in ((2 * y + 1 - f) // (2 * f), (2 * y + 1 - f) // (2 * f) + 1, y // f) if 0 <= q < h // f}
            assert rows == set(range(want[0], want[0] + want[1])), c
            seen.add((r0 % f != 0, (r0 + nr) % f != 0))
    assert (True, True) in seen        # tile borders that are no multiple of the factor


def test_the_rules_of_the_rows_calls(ask):
    cases = [(h, w0, wn, r0, n, it) for h in (1, 4, 9) for it in (0, 1, 2) for w0 in range(h + 2) for wn in range(h + 2) for r0 in range(h + 2) for n in range(h + 2)]
    got = ask([f"fcheck {' '.join(map(str, c))}" for c in cases])
    seen = set()
    for c, (g,) in zip(cases, got):
        assert g == filter_check(*c), c
        seen.add(g)
    assert seen == {OK, EMPTY, OUTSIDE, SHORT}
    cases = [(12, f, r0, n, l0, ln) for f in (1, 2, 3, 4, 5) for r0 in range(14) for n in range(14) for l0 in range(8) for ln in range(8)]
    got = ask([f"ucheck {' '.join(map(str, c))}" for c in cases])
    seen = set()
    for c, (g,) in zip(cases, got):
        assert g == upsample_check(*c), c
        seen.add(g)
    assert seen == {OK, EMPTY, OUTSIDE, SHORT}
    # one row short at either end, and the exact window: the edge the GPU tests rely on
    assert ask(["fcheck 47 6 35 20 7 3", "fcheck 47 7 34 20 7 3", "fcheck 47 6 34 20 7 3", "fcheck 47 0 47 20 7 3"]) == [[OK], [SHORT], [SHORT], [OK]]


def test_exchange_plans_of_every_tiling(ask):
    """the tiles own, every tile's filter window is wanted (an empty tile wants nothing); also with every other window absent"""
    cases = []
    for h in HEIGHTS:
        for n in TILES:
            src = [tile_rows(h, n, t) for t in range(n)]
            for it in ITERATIONS:
                dst = [filter_window(h, *s, it) for s in src]
                cases.append((src, dst))
                if n > 1 and it in (1, 3):
                    cases.append((src, [d if t % 2 else (0, 0) for t, d in enumerate(dst)]))
    got = ask([plan_question(s, d) for s, d in cases])
    most_owners, empties = 0, 0
    for (src, dst), g in zip(cases, got):
        verdict, _, copies = plan_answer(g)
        assert (verdict, copies) == (PLAN_OK, plan(src, dst)[2]), (src, dst)
        # what the copies do to row-tagged buffers: every window row holds its own image row, once
        filled = [dict() for _ in dst]
        for s, sr, d, dr, nr in copies:
            assert nr > 0 and sr + nr <= src[s][1] and dr + nr <= dst[d][1], (src, dst)
            for k in range(nr):
                assert dr + k not in filled[d]
                filled[d][dr + k] = src[s][0] + sr + k
        for d, (r0, nr) in enumerate(dst):
            assert filled[d] == {k: r0 + k for k in range(nr)}, (src, dst)
            most_owners = max(most_owners, len({c[0] for c in copies if c[2] == d}))
        empties += any(s[1] == 0 for s in src)
    assert most_owners >= 9 and empties > 0


def test_the_window_of_the_gpu_test_spans_three_owners(ask):
    src = [tile_rows(12, 5, t) for t in range(5)]
    dst = [filter_window(12, *s, 2) for s in src]
    verdict, _, copies = plan_answer(ask([plan_question(src, dst)])[0])
    assert verdict == PLAN_OK and min(len([c for c in copies if c[2] == d]) for d in range(5)) >= 3


def test_exchange_refusals(ask):
    cases = [
        ([(0, 4), (3, 4)], [(0, 0), (0, 0)], OWNERS_OVERLAP, 1),               # one row shared
        ([(0, 4), (4, 4), (0, 8)], [(0, 0)] * 3, OWNERS_OVERLAP, 2),           # an owner over two others
        ([(2, 3), (2, 3)], [(0, 0)] * 2, OWNERS_OVERLAP, 1),                   # the same rows twice
        ([(0, 4), (5, 3)], [(0, 8), (0, 0)], ROW_UNOWNED, 0),                  # a gap between the tiles
        ([(0, 4), (4, 4)], [(0, 4), (4, 5)], ROW_UNOWNED, 1),                  # a window past the last row
        ([(2, 4), (6, 2)], [(0, 0), (1, 3)], ROW_UNOWNED, 1),                  # ... and before the first
        ([(0, 0), (0, 0)], [(0, 0), (3, 1)], ROW_UNOWNED, 1),                  # nobody owns anything
        ([(0, 4), (4, 0)], [(0, 4), (0, 4)], PLAN_OK, 0),                      # an empty tile owns nothing and overlaps nothing
        ([(4294967290, 5), (0, 4)], [(4294967292, 3), (0, 0)], PLAN_OK, 0),    # rows near 2^32
        ([(4294967290, 5), (4294967294, 1)], [(0, 0)] * 2, OWNERS_OVERLAP, 1),
    ]
    got = ask([plan_question(s, d) for s, d, _, _ in cases])
    for (src, dst, want, at), g in zip(cases, got):
        verdict, where, copies = plan_answer(g)
        assert verdict == want, (src, dst)
        if want != PLAN_OK:
            assert where == at and copies == [], (src, dst)
            assert plan(src, dst)[:2] == (want, at), "the test's own arithmetic"
        else:
            assert copies == plan(src, dst)[2], (src, dst)
    assert ask(["plan 0"]) == [[PLAN_OK, 0, 0]]
