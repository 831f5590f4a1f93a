"""CPU: the cases tests/test_view_guides.py renders exercise all three kinds of pixel -- without a hit, with every sample a hit, partly hit -- so a
kernel that skipped misses, or counted them, could not pass by accident.  The counts were computed with the CPU oracle
(view_guides_common.expected) when the cases were chosen; here they are asserted, with what the definition says about each kind."""
import numpy as np
import pytest

import rays_common as R
import view_cameras_common as VC
import view_common as V
import view_guides_common as VG
from conftest import load_fixture

STANDARD = [("cornell_32x24_r4", "equirect", (7, 78, 6)), ("cornell_32x24_r4", "fisheye", (12, 63, 16)), ("cornell_32x24_r4", "ortho", (0, 91, 0)),
            ("cornell_teapot3_32x24_r4", "equirect", (8, 78, 5)), ("cornell_teapot3_32x24_r4", "fisheye", (12, 63, 16))]
CATALOGUE = [("staged", "rim_17x40_pi", (116, 496, 68)), ("single_cell", "clipped_ortho", (415, 268, 94))]


def check_kinds(tag, sc, v, nh, ad, want):
    assert nh.dtype == np.float32 and ad.dtype == np.float32 and nh.shape == ad.shape == (v.n_pixels, 4)
    assert VG.kinds(nh, v.rpp) == want, f"{tag}: {VG.kinds(nh, v.rpp)} pixels (no hit, every sample, partly), want {want}"
    none = nh[:, 3] == 0
    assert (nh[none].view(np.uint32) == 0).all() and (ad[none].view(np.uint32) == 0).all(), f"{tag}: a pixel without a hit is all +0 in both"
    hit = ~none
    assert (ad[hit, 3] > 0).all(), f"{tag}: a hit pixel has a positive depth sum"
    assert (np.abs(nh[hit, 0:3]).sum(axis=1) > 0).all(), f"{tag}: a hit pixel has a normal"


@pytest.mark.parametrize("name,model,want", STANDARD)
def test_standard_views_hold_all_three_kinds(name, model, want):
    sc = load_fixture(name)[1]
    v = V.standard_view(sc, model)
    assert (v.width, v.height, v.k) == (13, 7, 2)
    nh, ad = VG.expected(sc, v)
    check_kinds(f"{name} {model}", sc, v, nh, ad, want)


@pytest.mark.parametrize("stratum,camera,want", CATALOGUE)
def test_catalogue_cameras_hold_all_three_kinds(stratum, camera, want):
    v = VC.view(stratum, camera)
    nh, ad = VG.expected_catalogue(stratum, camera)
    check_kinds(f"{stratum} {camera}", R.scene(stratum), v, nh, ad, want)
    assert min(want) > 0


def test_dead_fisheye_samples_are_never_hits():
    """a pixel wholly outside the circle is background; a pixel on the rim is partly hit at most by its live samples"""
    sc = load_fixture(STANDARD[1][0])[1]
    v = V.standard_view(sc, "fisheye")
    rays = V.view_rays(v)
    dead = (rays[:, 3] == rays[:, 7]).reshape(-1, v.rpp)
    nh, _ad = VG.expected(sc, v)
    assert dead.all(axis=1).any() and (dead.any(axis=1) & ~dead.all(axis=1)).any()
    assert (nh[dead.all(axis=1), 3] == 0).all()
    assert (nh[:, 3] <= (~dead).sum(axis=1)).all()


def test_a_cut_material_table_turns_hits_into_misses():
    sc = load_fixture(STANDARD[0][0])[1]
    v = V.standard_view(sc, "equirect")
    mats = np.asarray(sc.materials, np.float32).reshape(-1, 4)
    full, _ = VG.expected(sc, v)
    cut, _ = VG.expected(sc, v, materials=mats[:2])
    assert len(mats) > 2 and (cut[:, 3] <= full[:, 3]).all() and (cut[:, 3] < full[:, 3]).any() and (cut[:, 3] > 0).any()
