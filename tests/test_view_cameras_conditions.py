"""CPU: the view cameras of tests/view_cameras_common.py, on the oracle alone, meet the conditions that keep the GPU comparisons of
tests/test_view_cameras.py from passing on emptiness, and each edge camera can tell the definition from its nearest mistake.

  * every (stratum, camera) the GPU renders has w > 0 in at least 0.10 of its pixels, and in at least 0.25 outside `open` and clipped_*;
    outside those two, at least 0.05 of the pixels are not black after the tone map and at least 0.05 of the seeds advance;
  * axis_* and mixed_k*: the guard refuses a PRIMARY ray in 20 % to 80 % of the frame's blocks of 256 ray ids, and the frame has at least 8
    blocks, so the optimistic kernel's mask and grid hold a mix; the same holds for the row tile the GPU test takes, whose first block is clean;
  * all_refused: a primary ray in every block; oblique_*, scaled_up and every other edge camera: in none (what defers there is the bounces');
  * rim_*: the stated numbers of samples with r == 1.0f exactly (live) and r == nextafter(1.0f) (dead); axis_fisheye_601x3 has one r == 0;
  * clipped_*: t_max cuts some first hits and leaves others;
  * the three GRIDS values occur among the strata;
  * radiance_common.expected_radiance gives the same words with a `watch` as without;
  * DISCRIMINATION: view_rays_as(view, mistake) differs from view_common.view_rays in at least one word on the cameras made for that mistake,
    and the fold that ignores the carry or adds in pairwise order differs from the sequential one on the frames that use them.

These are conditions, not measurements: an input that misses one gets another seed or size, never another bound."""
import numpy as np
import pytest

import radiance_common as RC
import rays_common as R
import view_cameras_common as VC
import view_common as V
from conftest import bits
from random_scenes_common import ENCLOSED, STRATA, kernel_choice

f32 = np.float32
EXEMPT_CAMERAS = VC.CLIPPED


def words_differ(a, b):
    return bool((bits(np.ascontiguousarray(a, f32)) != bits(np.ascontiguousarray(b, f32))).any())


@pytest.mark.parametrize("stratum,name", VC.used_on_the_gpu())
def test_the_frame_is_not_empty(stratum, name):
    fr = VC.frame(stratum, name)
    lit, colour, advanced = VC.shares(fr)
    assert lit >= 0.10, (stratum, name, lit)
    if stratum != "open" and name not in EXEMPT_CAMERAS:
        assert lit >= 0.25 and colour >= 0.05 and advanced >= 0.05, (stratum, name, lit, colour, advanced)
    assert set(VC.blocks_of(fr.primary)) <= set(VC.blocks_of(fr.refused))


@pytest.mark.parametrize("name", VC.MIXED)
@pytest.mark.parametrize("stratum", ENCLOSED)
def test_mixed_frames_hold_refused_and_clean_blocks(stratum, name):
    v, fr = VC.view(stratum, name), VC.frame(stratum, name)
    blocks, refused = VC.n_blocks(v), len(VC.blocks_of(fr.primary))
    assert blocks >= 8 and 0.2 * blocks <= refused <= 0.8 * blocks, (stratum, name, refused, blocks)
    if name in VC.MIXED_K:
        assert v.k >= 2 and v.width * v.rpp > 3 * 256, "a row spans several blocks"
        assert v.rpp == 256 or (v.width * v.rpp) % 256, "... and, where a block holds several pixels, does not start one"
        per_row = np.array([len(VC.blocks_of(fr.primary[r * v.width * v.rpp:(r + 1) * v.width * v.rpp])) for r in range(v.rows)])
        assert (per_row > 0).all() and (per_row < -(-v.width * v.rpp // 256)).all(), "the refusal depends on the column"
    # the row tile the GPU test renders: its first block is clean, and it holds a mix as well
    row0, nrows = VC.clean_tile(fr)
    per = v.width * v.rpp
    tile = fr.refused[row0 * per:(row0 + nrows) * per]
    tb = VC.blocks_of(tile)
    assert row0 > 0 and 0 not in tb and 0 < len(tb) < -(-len(tile) // 256), (stratum, name, row0, tb)


@pytest.mark.parametrize("stratum", VC.EDGE_STRATA)
def test_which_edge_cameras_the_guard_refuses(stratum):
    for name in VC.EDGE:
        v, fr = VC.view(stratum, name), VC.frame(stratum, name)
        refused = len(VC.blocks_of(fr.primary))
        assert refused == (VC.n_blocks(v) if name == "all_refused" else 0), (stratum, name, refused)


@pytest.mark.parametrize("stratum", STRATA)
def test_no_primary_ray_of_the_oblique_cameras_is_refused(stratum):
    for name in VC.OBLIQUE:
        assert not VC.frame(stratum, name).primary.any(), (stratum, name)


@pytest.mark.parametrize("size", VC.RIMS)
def test_rim_samples_sit_exactly_on_the_circle(size):
    w, h, k = size
    one, nxt = f32(1.0), np.nextafter(f32(1.0), f32(2.0))
    for frame_size in ((w, h), (h, w)):
        v = VC.rim(R.scene("staged"), *frame_size, k, float(V.PI))
        a, b = VC.window(v)
        r = np.sqrt(a * a + b * b)
        assert r.dtype == f32
        assert (int((r == one).sum()), int((r == nxt).sum())) == VC.RIM_COUNTS[size], frame_size
        rays = V.view_rays(v)
        assert R.live(rays)[r == one].all() and not R.live(rays)[r == nxt].any()
        assert (r > one).any() and (r < one).any()


def test_the_axis_fisheye_frame_has_one_sample_at_the_centre():
    for h, want in ((3, 1), (4, 0)):
        a, b = VC.window(VC.axis(R.scene("staged"), "fisheye", h))
        assert int(((a == 0) & (b == 0)).sum()) == want
        assert int((a == 0).sum()) == h, "the centre column has a == 0 exactly"


@pytest.mark.parametrize("stratum", VC.EDGE_STRATA)
def test_clipping_cuts_some_first_hits_and_leaves_others(stratum):
    sc = R.scene(stratum)
    for name in ("clipped_equirect", "clipped_ortho"):
        rays = V.view_rays(VC.view(stratum, name))
        free = rays.copy()
        free[:, 7] = np.inf
        hit, hit_free = R.expected_closest(sc, rays)[1] != R.NO_SET, R.expected_closest(sc, free)[1] != R.NO_SET
        assert not (hit & ~hit_free).any()
        assert hit.mean() >= 0.10 and (hit_free & ~hit).mean() >= 0.10, (stratum, name, hit.mean(), hit_free.mean())
    thin = V.view_rays(VC.view(stratum, "clipped_thin"))
    live = R.live(thin)
    assert (thin[live, 7] == np.nextafter(thin[live, 3], f32(np.inf))).all() and live.any()


def test_the_strata_force_all_three_grid_variants():
    assert {kernel_choice(R.scene(s))["GRIDS"] for s in STRATA} == {0, 1, 2}


def test_a_watch_changes_no_result():
    sc, v = R.scene("guard"), VC.view("guard", "k4_equirect")
    rays, seeds = V.view_rays(v), VC.seeds_of(v.n_rays)
    seen = []
    plain = RC.expected_radiance(sc, rays, seeds, 1, VC.BOUNCES)
    watched = RC.expected_radiance(sc, rays, seeds, 1, VC.BOUNCES, watch=lambda kind, buf: seen.append((kind, len(buf))))
    assert RC.differ("with a watch", watched, plain) is None
    assert [k for k, _ in seen].count("rays") == 1 + VC.BOUNCES and [k for k, _ in seen].count("shadow") == (1 + VC.BOUNCES) * len(sc.lights)
    fr = VC.frame("guard", "k4_equirect")
    assert RC.differ("the cached frame", (fr.acc, fr.seeds), plain) is None
    assert np.array_equal(VC.refused_blocks(sc, v, seeds, VC.BOUNCES), VC.blocks_of(fr.refused))


# ---- discrimination ------------------------------------------------------------------------------------------------------------------------------------
TELLS = ([(n, "r_below_1") for n in VC.RIM] + [(n, "local_row") for n in ("extent_tall",) + VC.MIXED_K] + [("axis_fisheye_601x3", "q_unguarded")] +
         [(n, "normalised_basis") for n in ("all_refused", "scaled_up", "sheared_ortho", "sheared_equirect", "sheared_fisheye") + VC.MIXED_K] +
         [(n, "t_min_ignored") for n in VC.CLIPPED])


@pytest.mark.parametrize("name,mistake", TELLS)
def test_the_camera_tells_the_definition_from_the_mistake(name, mistake):
    v = VC.view("guard", name)
    right = V.view_rays(v)
    assert not words_differ(VC.view_rays_as(v), right)
    assert words_differ(VC.view_rays_as(v, mistake), right), (name, mistake)


def test_every_mistake_has_a_camera_and_every_edge_camera_a_mistake():
    assert {m for _, m in TELLS} == set(VC.MISTAKES)
    told = {n for n, _ in TELLS}
    assert set(VC.EDGE) - told <= {"outside", "on_face"}, "those two are inputs at the box's edge, not edges of the ray definition"


def test_q_at_r_0_matters_only_when_it_is_not_finite():
    """q = 1 at r == 0 in place of q = 0 is the same function: lx = a * q and ly = b * q with a == b == +0.  The mistake an input can show is the
    missing guard, q = 0 / 0."""
    v = VC.view("staged", "axis_fisheye_601x3")
    a, b = VC.window(v)
    at = np.flatnonzero(np.sqrt(a * a + b * b) == 0)
    assert len(at) == 1 and not np.signbit(a[at]).any() and not np.signbit(b[at]).any()
    for q in (f32(0.0), f32(1.0)):
        local = (a[at] * q, b[at] * q)
        assert all(x.view(np.uint32)[0] == 0 for x in local)
    assert np.isnan(VC.view_rays_as(v, "q_unguarded")[at, 4:7]).all() and not np.isnan(V.view_rays(v)).any()


@pytest.mark.parametrize("name", VC.MIXED)
def test_the_carry_matters_on_the_mixed_frames(name):
    fr = VC.frame("staged", name)
    carry = fr.sums
    assert words_differ(V.fold(fr.acc, fr.view.rpp, carry), V.fold(fr.acc, fr.view.rpp))
    _, sums, px = fr.triple(carry=carry, tone=fr.view.tone / 2)
    assert not words_differ(sums, V.fold(fr.acc, fr.view.rpp, carry))


@pytest.mark.parametrize("name", VC.MIXED_K + VC.RIM[:1] + VC.RIM[3:4] + ("k4_equirect", "k8_fisheye", "k16_equirect", "oblique_ortho"))
def test_the_order_of_the_fold_matters(name):
    fr = VC.frame("staged", name)
    assert fr.view.rpp >= 4
    assert words_differ(VC.fold_pairwise(fr.acc, fr.view.rpp), fr.sums), name
