"""Generated scenes of every stratum (tests/random_scenes_common.py: single_cell, staged, unstaged, many_sets, open, guard -- each named after the
k_fusedPass build it forces) through every route of the fused pass, each compared with the CPU ORACLE's state after every pass at tolerance 0, never
with another route of the library: ordinary passes, mirt_render_passes with and without a frame after every pass, the guides, the first pass with
guides, the guided multi-pass call, a row tile -- with the optimistic pair and under set_exact_only(True), with and without a kept accumulator, with
MIRT_MULTIPASS_REUSE unset, 0 and 1.  Frames are 37 x 21 (777 pixels: a partial last block at 4, 16 and 64 pixels a block); pixels of more than
256 rays use 9 x 5.

CPU (no mark): the conditions that keep a case from passing on emptiness (first hits, light gained at every bounce, measured on the oracle), the
kernel each stratum forces (the arithmetic of fused_lds_slots and launch_fused), the guard scenes' refused blocks, and the coverage table of the
parametrisation below.

The rotation: every scene (three seeds a stratum) gets the ordinary route and mirt_render_passes with n = 2 at its base ray count; every other
(route, ray count) pair of WANTED occurs once per stratum, dealt over the three seeds in turn, with n = 3 at THREE_PASSES, n = 1 at ONE_PASS and 8
bounces at EIGHT_BOUNCES.

The guard scenes (tests/random_scenes_common.py) hold rays the ray-side guard refuses in some of the units the optimistic kernel defers and not in
all, and units that are clean in pass 1 and hold their first refused ray in pass 2: test_guard_scenes_defer_in_some_units_and_some_first_in_pass_2
proves both on every ray of the oracle's passes, and the GPU cases of LATE assert that a launch of n passes defers more than the one-pass launch
does.  Their 289-ray cases run on the scene with a lens: under a pinhole no unit of a 289-ray launch is clean in pass 1."""
import json
import os
import subprocess
import sys

import pytest

import a10_pass as A
import random_scenes_common as C
from conftest import ROOT
from test_set_guard import ask   # noqa: F401  (the module-scoped fixture that compiles tests/set_guard_dump.cpp)

gpu = pytest.mark.gpu
W, H = 37, 21
BIG = (9, 5)        # the frame of the ray counts above 256

# (route, ray counts) every stratum must show
WANTED = {"ordinary": (1, 4, 16), "passes": (4, 16, 64, 9, 289, 1), "every": (4, 16, 64, 9, 289), "guides": (4, 16), "first_guided": (4, 16, 64, 289),
          "passes_guided": (4, 16, 64, 9), "row_tile": (4, 16)}
ALL_RPPS = (1, 4, 9, 16, 64, 289)
# where the rotation asks for n = 3 and for 8 bounces: at the small ray counts, so that the oracle's share of a case stays small
THREE_PASSES = {("passes", 1), ("passes", 9), ("every", 4), ("every", 9), ("passes_guided", 16)}
EIGHT_BOUNCES = {("ordinary", 16), ("passes", 16), ("every", 16), ("passes_guided", 4)}
ONE_PASS = {("passes_guided", 64)}      # mirt_render_passes_guided with n = 1: grid scenes write the guides in the launch too, every frame falls back
# guard scenes, multi-pass launches that resolve their pixels: (route, ray count) where some unit is clean in pass 1 and defers in a later pass
LATE = {("passes", 16), ("every", 16), ("passes", 64), ("every", 64), ("passes", 289), ("every", 289)}


def base_rpp(stratum):
    return 16 if stratum == "guard" else 4


def wanted(stratum):
    return [(route, rpp) for route, rpps in WANTED.items() for rpp in rpps]


def _cases():
    out = []
    for stratum in C.STRATA:
        base = base_rpp(stratum)
        for seed in C.SEEDS[stratum]:      # every scene: ordinary passes and n = 2
            out += [(stratum, seed, "ordinary", base, 3, 5), (stratum, seed, "passes", base, 2, 5)]
        k = 0
        for route, rpp in wanted(stratum):
            if route in ("ordinary", "passes") and rpp == base and (route, rpp) not in EIGHT_BOUNCES:
                continue      # (every scene has it already)
            seed = C.SEEDS[stratum][2 if stratum == "guard" and rpp == 289 else k % 3]      # (289 rays: the guard scene with a lens)
            n = 3 if route == "ordinary" or (route, rpp) in THREE_PASSES else 1 if route in ("guides", "first_guided") or (route, rpp) in ONE_PASS else 2
            out.append((stratum, seed, route, rpp, n, 8 if (route, rpp) in EIGHT_BOUNCES else 5))
            k += 1
    return out + [("guard", C.SEEDS["guard"][2], "every", 16, 3, 5)]      # the lens scene's every-frame launch at a count that divides 256


CASES = _cases()
IDS = [f"{s}-{seed}-{route}-r{rpp}-n{n}-b{b}" for s, seed, route, rpp, n, b in CASES]


def _scene(stratum, seed, rpp):
    w, h = BIG if rpp > 256 else (W, H)
    sc = C.scene(stratum, seed, w, h, rpp)
    return sc, A.make_seeds(sc.total_rays, seed_base=seed)


@pytest.fixture(scope="module")
def win(ask):   # noqa: F811
    import ray_edges_common as R
    return R.window_constants(ask)


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------------------------
def test_the_parametrisation_covers_every_stratum_route_and_ray_count():
    have = {}
    for s, seed, route, rpp, n, b in CASES:
        have.setdefault(s, set()).add((route, rpp))
    for s in C.STRATA:
        print(s, sorted(have[s]))
        assert have[s] == set(wanted(s)), s
        mine = [c for c in CASES if c[0] == s]
        assert len(C.SEEDS[s]) == 3 and len({seed % 3 for seed in C.SEEDS[s]}) == 3, "three seeds, one of each variant"
        for seed in C.SEEDS[s]:      # every scene has the ordinary and the n = 2 routes
            assert any(c[1] == seed and c[2] == "ordinary" for c in mine) and any(c[1] == seed and c[2] == "passes" and c[4] == 2 for c in mine), (s, seed)
            assert sum(c[1] == seed for c in mine) >= 5, "the rotation reaches every seed"
        for route in ("passes", "every", "passes_guided"):      # n = 2 and n = 3, 5 and 8 bounces, through each multi-pass call
            assert {c[4] for c in mine if c[2] == route} - {1} == {2, 3} and {c[5] for c in mine if c[2] == route} == {5, 8}, (s, route)
        assert any(c[2] == "passes_guided" and c[4] == 1 for c in mine), s
        assert {c[5] for c in mine if c[2] == "ordinary"} == {5, 8} and any(c[2] == "row_tile" for c in mine), s
    assert {rpp for v in WANTED.values() for rpp in v} == set(ALL_RPPS)
    # the frames: a partial last block at 4, 16 and 64 pixels per block, and in the row tile
    assert all((W * H) % k for k in (4, 16, 64)) and all((C.ROW_TILE[1] * W) % k for k in (4, 16, 64)) and C.ROW_TILE[0] > 0 and sum(C.ROW_TILE) < H
    # 289 rays: segments of 256 + 32 + 1 (csrc/pt_pass_plan.hpp fused_segment)
    assert 289 == 17 * 17 == 256 + 32 + 1


@pytest.mark.parametrize("stratum", C.ENCLOSED)
def test_conditions_hold(stratum):
    """no enclosed scene lets a case pass on emptiness: on the oracle, at the frame size and base ray count the GPU cases use, at least 25 % of the
    pixels have a first hit and at least 5 % of the samples gain colour with each further bounce 1..5 (run_pass at bounces = j against j - 1, same
    seeds).  `open` scenes are exempt: they are what tests/test_random_scenes.py runs, kept for the rays that miss everything."""
    for seed in C.SEEDS[stratum]:
        for rpp in (base_rpp(stratum), 289):      # both frame sizes the GPU cases use: 37 x 21, and 9 x 5 at 289 rays
            sc, seeds = _scene(stratum, seed, rpp)
            first, gain = C.shares(sc, seeds)
            print(f"{stratum} {seed} {sc.width}x{sc.height}x{rpp}: first hit {first:.3f}, gain at bounce 1..5 " + " ".join(f"{g:.3f}" for g in gain))
            assert first >= C.FLOOR_FIRST_HIT, (seed, rpp, first)
            assert min(gain) >= C.FLOOR_GAIN, (seed, rpp, gain)


def test_each_stratum_forces_its_kernel():
    """fused_lds_slots (csrc/pt_closest.hpp) and launch_fused (csrc/pt_kernels_fused.hip) in integers, on every scene"""
    choice = {(s, seed): C.kernel_choice(C.scene(s, seed, W, H, base_rpp(s))) for s in C.ENCLOSED for seed in C.SEEDS[s]}
    sets = {key: C.sets_of(C.scene(key[0], key[1], W, H, base_rpp(key[0]))) for key in choice}
    for key, c in choice.items():
        print(key, {k: v for k, v in c.items() if k != "tri_staged"}, [t[1:] for t in sets[key]], "staged records:", c["tri_staged"])
    for seed in C.SEEDS["single_cell"]:
        c = choice["single_cell", seed]
        assert c["GRIDS"] == 0 and not c["grids"] and all(n == 1 for _, n, _ in sets["single_cell", seed])
        assert C.kernel_choice(C.scene("single_cell", seed, W, H, 4), passes=2)["MULTI"] == 2      # default pairing: primary-hit reuse
    a, b, _ = C.SEEDS["single_cell"]
    assert [t[2] for t in sets["single_cell", a] if t[0]] == [60, 40, 7]
    assert [x for x, t in zip(choice["single_cell", a]["tri_staged"], sets["single_cell", a]) if t[0]] == [True, False, True]   # 60; 100 > 96; 67
    assert [t[2] for t in sets["single_cell", b] if t[0]] == [97, 96, 95]
    assert [x for x, t in zip(choice["single_cell", b]["tri_staged"], sets["single_cell", b]) if t[0]] == [False, True, False]  # 97 > 96; 96; 191 > 96
    for seed in C.SEEDS["staged"]:
        c = choice["staged", seed]
        assert c["GRIDS"] == 1 and 0 < c["words"] <= C.K_LDS_OFF_WORDS
        assert all(2 <= n <= 15 for _, n, _ in sets["staged", seed])
        assert C.kernel_choice(C.scene("staged", seed, W, H, 4), passes=2)["MULTI"] == 1            # grids: the plain pass loop
    assert choice["staged", C.SEEDS["staged"][0]]["words"] == 2 * (8 ** 3 + 1) + (12 ** 3 + 1) + (11 ** 3 + 1) + (2 ** 3 + 1) == 4096
    assert choice["staged", C.SEEDS["staged"][0]]["WAVES"] == 5 and choice["staged", C.SEEDS["staged"][2]]["WAVES"] == 0
    for seed in C.SEEDS["unstaged"]:
        c = choice["unstaged", seed]
        assert c["GRIDS"] == 2 and c["words"] > C.K_LDS_OFF_WORDS
    a, b, _ = C.SEEDS["unstaged"]
    assert choice["unstaged", a]["words"] == 16 ** 3 + 1 == 4097 and [n for _, n, _ in sets["unstaged", a] if n > 1] == [16]
    assert max(n ** 3 + 1 for _, n, _ in sets["unstaged", b]) <= 11 ** 3 + 1 < C.K_LDS_OFF_WORDS < choice["unstaged", b]["words"]
    for seed in C.SEEDS["many_sets"]:
        s = sets["many_sets", seed]
        assert len(s) == 2 + C.K_MAX_MESHES == 18 and not s[0][0] and all(1 <= t[2] for t in s)
        assert {n == 1 for _, n, _ in s[2:]} == {True, False}, "single cells and grids mixed"
    assert [choice["many_sets", seed]["GRIDS"] for seed in C.SEEDS["many_sets"]] == [1, 2, 1]
    assert [choice["guard", seed]["GRIDS"] for seed in C.SEEDS["guard"]] == [0, 1, 1]
    # The builds the multi-pass routes reach, so that the claimed reach cannot drift unnoticed: per scene GRIDS, then (WAVES, MULTI) of one pass and of
    # two passes with MIRT_MULTIPASS_REUSE unset, 0 and 1.  The numbers behind WAVES: a grid kernel's block asks for the four waves' exchange areas,
    # 4 * 1808 = 7232 B, beside 4 * (13 * 256 + 64) = 13 568 B of parked state and lens table; six blocks share a CU up to 21 granules of 1280 B, so
    # up to 1520 words of staged tables.  The reuse rows (8 * 256 words) take every grid kernel to 28 992 B = 23 granules and five blocks: with
    # MULTI 2 launch_fused picks the 5-wave grid builds for every scene, and the 6-wave ones only under MIRT_GRID_WAVES (the child's second mode).
    assert -(-(7232 + 13568) // 1280) == 17 and -(-(7232 + 13568 + 4 * 1520) // 1280) == 21 and -(-(7232 + 13568 + 8192) // 1280) == 23 and 128 // 23 == 5
    table = {
        ("single_cell", 0): (0, (0, 0), (0, 2), (0, 1), (0, 2)), ("single_cell", 1): (0, (0, 0), (0, 2), (0, 1), (0, 2)), ("single_cell", 2): (0, (0, 0), (0, 2), (0, 1), (0, 2)),
        ("staged", 0): (1, (5, 0), (5, 1), (5, 1), (5, 2)), ("staged", 1): (1, (5, 0), (5, 1), (5, 1), (5, 2)), ("staged", 2): (1, (0, 0), (0, 1), (0, 1), (5, 2)),
        ("unstaged", 0): (2, (0, 0), (0, 1), (0, 1), (5, 2)), ("unstaged", 1): (2, (0, 0), (0, 1), (0, 1), (5, 2)), ("unstaged", 2): (2, (0, 0), (0, 1), (0, 1), (5, 2)),
        ("many_sets", 0): (1, (5, 0), (5, 1), (5, 1), (5, 2)), ("many_sets", 1): (2, (0, 0), (0, 1), (0, 1), (5, 2)), ("many_sets", 2): (1, (5, 0), (5, 1), (5, 1), (5, 2)),
        ("guard", 0): (0, (0, 0), (0, 2), (0, 1), (0, 2)), ("guard", 1): (1, (5, 0), (5, 1), (5, 1), (5, 2)), ("guard", 2): (1, (5, 0), (5, 1), (5, 1), (5, 2))}
    for (s, i), want in table.items():
        sc = C.scene(s, C.SEEDS[s][i], W, H, base_rpp(s))
        rows = [C.kernel_choice(sc, 1)] + [C.kernel_choice(sc, 2, r) for r in (None, False, True)]
        assert (rows[0]["GRIDS"],) + tuple((r["WAVES"], r["MULTI"]) for r in rows) == want, (s, i)


def _late(sc, seeds, n, bounces, win):
    """(units of block_of clean in pass 1 whose first refused ray comes in passes 2..n, units refused in pass 1, all units), on the oracle"""
    import numpy as np
    by_pass, units = C.refused_blocks_by_pass(sc, seeds, n, win, bounces)
    later = np.setdiff1d(np.concatenate(by_pass[1:]), by_pass[0]) if n > 1 else by_pass[0][:0]
    return len(later), len(by_pass[0]), units


GUARD_CASES = [c for c in CASES if c[0] == "guard" and c[2] in ("passes", "every")]


@pytest.mark.parametrize("stratum,seed,route,rpp,n,bounces", GUARD_CASES, ids=[IDS[CASES.index(c)] for c in GUARD_CASES])
def test_guard_scenes_defer_in_some_units_and_some_first_in_pass_2(win, stratum, seed, route, rpp, n, bounces):
    """ray_edges_common.accepted over EVERY ray the oracle makes in the case's own passes (primary, bounce and shadow rays): more than 0 and fewer
    than all of the units the optimistic kernel defers -- blocks of 256 samples of a launch, or samples -- hold a refused ray in pass 1; and in the
    cases of LATE some unit is clean in pass 1 and holds its first refused ray in a later pass of the launch: it writes pass 1's sums (with a frame
    after every pass, pass 1's frame) and defers afterwards"""
    sc, seeds = _scene(stratum, seed, rpp)
    later, first, units = _late(sc, seeds, n, bounces, win)
    print(f"guard {seed} x{rpp}, {n} passes, {bounces} bounces: {first} of {units} units refused in pass 1, {later} more first in a later pass")
    assert 0 < first < units
    if (route, rpp) in LATE:
        assert later > 0


def test_guard_scenes_under_a_pinhole_have_no_clean_unit_at_289_rays(win):
    """why the 289-ray guard cases run on the scene with a lens: under a pinhole every block of every segment's launch holds a centre-column pixel
    (d.x == 0 in all of its samples) or the NaN centre sample"""
    for seed in C.SEEDS["guard"][:2]:
        sc, seeds = _scene("guard", seed, 289)
        _, first, units = _late(sc, seeds, 1, 5, win)
        assert first == units == 45 + 6 + 1      # 45 pixels: 256-ray blocks, 45 * 32 / 256 and 45 / 256 rounded up


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(pkg):
    from raytracing_amd.pyhost import mirt
    c = mirt.Context(0)
    yield c
    c.set_exact_only(False)
    c.destroy()


def run_case(ctx, stratum, seed, route, rpp, n, bounces):
    """-> (differences from the oracle, [mirt_pass_deferred after each multi-pass call: without an accumulator first, where that runs])"""
    sc, seeds = _scene(stratum, seed, rpp)
    deferred = []
    if route == "ordinary":
        return C.run_ordinary(ctx, sc, seeds, bounces, n), deferred
    if route in ("passes", "every"):
        return C.run_passes(ctx, sc, seeds, n, bounces, every=(route == "every"), deferred=deferred), deferred
    if route == "guides":
        return C.run_guides(ctx, sc, seeds), deferred
    if route == "first_guided":
        return C.run_first_guided(ctx, sc, seeds, bounces), deferred
    if route == "passes_guided":
        return C.run_passes_guided(ctx, sc, seeds, n, bounces), deferred
    assert route == "row_tile"
    return C.run_row_tile(ctx, sc, seeds, n, bounces), deferred


@gpu
@pytest.mark.parametrize("exact_only", [False, True], ids=["optimistic", "exact_only"])
@pytest.mark.parametrize("stratum,seed,route,rpp,n,bounces", CASES, ids=IDS)
def test_route_equals_the_oracle(ctx, pkg, stratum, seed, route, rpp, n, bounces, exact_only):
    ctx.set_exact_only(exact_only)
    try:
        diffs, deferred = run_case(ctx, stratum, seed, route, rpp, n, bounces)
    finally:
        ctx.set_exact_only(False)
    assert not diffs, diffs[:4]
    if stratum == "guard" and route in ("passes", "every"):
        # the redo kernel inside the multi-pass and every-frame launches: some block leaves the optimistic kernel, none exists without it
        print(f"deferred samples per call: {deferred}")
        assert deferred and all((d == 0) if exact_only else (d > 0) for d in deferred), deferred
        if (route, rpp) in LATE and not exact_only:
            # a unit that is clean in pass 1 and defers in a later pass of the launch (proved on the oracle by the CPU test of this case): the n-pass
            # launch defers more samples than the same launch with one pass, whose deferred units are those of pass 1
            sc, seeds = _scene(stratum, seed, rpp)
            one = []
            assert not C.run_passes(ctx, sc, seeds, 1, bounces, reuse=(None,), deferred=one)
            print(f"deferred by one pass: {one[0]}, by {n}: {deferred[0]}")
            assert deferred[0] > one[0] > 0


def _child(waves):
    import random_routes_child as child
    env = dict(os.environ, MIRT_GRID_WAVES=waves)
    env.pop("MIRT_LIB_PATH", None)
    env.pop("MIRT_MULTIPASS_REUSE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "random_routes_child.py"), waves], env=env, capture_output=True, text=True, timeout=600)
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0, (lines[-1:] or r.stderr[-2000:])
    assert len(lines) == 2 * len(child.cases(waves)) and all(l["ok"] for l in lines), lines


@gpu
def test_five_wave_build_of_the_grid_kernels():
    """MIRT_GRID_WAVES=5 is read once per process: tests/random_routes_child.py runs the staged and unstaged scenes through the routes ordinary,
    passes n = 2, every frame and first pass guided in a process of its own, against the oracle"""
    _child("5")


@gpu
def test_six_wave_build_of_the_grid_kernels_with_primary_hit_reuse():
    """the multi-pass cases among them under MIRT_GRID_WAVES=6: with MIRT_MULTIPASS_REUSE=1 the 6-wave grid kernels' MULTI 2 builds, which launch_fused's own LDS
    arithmetic never picks (tests/random_routes_child.py)"""
    _child("6")
