"""CPU: the generated rays of tests/rays_common.py, on the oracle alone, meet the conditions that keep the GPU comparisons of tests/test_rays.py
from passing on emptiness.  Per stratum:

  * every class of rays holds at least 5 % of the batch;
  * at least 25 % of the rays hit and at least 25 % miss;
  * every set of the scene wins at least one ray;
  * occlusion is 1 for at least 10 % and 0 for at least 10 % of the live rays;
  * the ray-side guard's rule, restated in numpy (include/mirt.h, mirt_debug_numerics op 28: every |d_k| in [2^-40, 2^40], every o_k zero or
    |o_k| in [2^-30, 2^20]), refuses at least 5 % and at most 60 % of the live rays.

These are conditions, not measurements: a stratum that misses one gets other seeds or shares in the generator, never another bound."""
import numpy as np
import pytest

import rays_common as R
from random_scenes_common import STRATA, kernel_choice


@pytest.mark.parametrize("stratum", STRATA)
def test_every_class_is_present(stratum):
    rays, cls = R.rays_of(stratum)
    assert rays.shape == (R.N_RAYS, 8) and rays.dtype == np.float32
    for k, name in enumerate(R.CLASSES):
        assert (cls == k).sum() >= 0.05 * R.N_RAYS, name
    live = R.live(rays)
    assert not live[cls == R.CLASSES.index("dead")].any() and live[cls != R.CLASSES.index("dead")].all()
    d = rays[cls == R.CLASSES.index("axis"), 4:7]
    assert ((d == 0).sum(axis=1) >= 1).all() and ((d == 0).sum(axis=1) <= 2).all()
    bad = rays[cls == R.CLASSES.index("nonfinite")][:, (0, 1, 2, 4, 5, 6)]
    assert (~np.isfinite(bad)).any(axis=1).all()
    ln = np.linalg.norm(rays[cls == R.CLASSES.index("scaled"), 4:7].astype(np.float64), axis=1)
    assert ln.min() >= 2.0 ** -3 * 0.999 and ln.max() <= 2.0 ** 3 * 1.001 and (np.abs(ln - 1.0) > 0.01).mean() > 0.9


@pytest.mark.parametrize("stratum", STRATA)
def test_face_origins_sit_exactly_on_a_face_of_a_set_box(stratum):
    rays, cls = R.rays_of(stratum)
    faces = np.concatenate([np.asarray(b, np.float32)[[0, 1, 2, 4, 5, 6]].reshape(2, 3) for _, _, b in R.set_list(R.scene(stratum))])
    for o in rays[cls == R.CLASSES.index("face"), 0:3]:
        assert (faces == o).any(), o


@pytest.mark.parametrize("stratum", STRATA)
def test_the_oracle_hits_and_misses_and_every_set_wins(stratum):
    sc = R.scene(stratum)
    hits, sets = R.closest_of(stratum)
    hit = hits[:, 7].view(np.int32) >= 0
    assert np.array_equal(hit, sets != R.NO_SET), "a winner changes Ray.maxt, and only a winner does"
    assert hit.mean() >= 0.25 and (~hit).mean() >= 0.25, (hit.mean(), stratum)
    n_sets = len(R.set_list(sc))
    won = np.unique(sets[hit])
    assert np.array_equal(won, np.arange(n_sets)), f"{stratum}: the sets that won a ray are {won.tolist()} of {n_sets}"
    rays, cls = R.rays_of(stratum)
    miss = hits[~hit]
    assert not miss[:, 0:3].view(np.uint32).any() and not miss[:, 4:7].view(np.uint32).any(), "a miss leaves normal and p at +0"
    assert np.array_equal(miss[:, 3].view(np.uint32), rays[~hit, 7].view(np.uint32)), "a miss keeps the input maxt"
    assert not hit[cls == R.CLASSES.index("dead")].any(), "a dead ray is a miss"


@pytest.mark.parametrize("stratum", STRATA)
def test_the_oracle_sees_both_occluded_and_free_rays(stratum):
    rays, cls = R.rays_of(stratum)
    occ = R.occluded_of(stratum)
    live = R.live(rays)
    assert occ[~live].all(), "a ray that enters dead is reported 1"
    assert occ[live].mean() >= 0.10 and (1 - occ[live]).mean() >= 0.10, (occ[live].mean(), stratum)


@pytest.mark.parametrize("stratum", STRATA)
def test_the_guard_refuses_some_live_rays_and_not_most(stratum):
    rays, _ = R.rays_of(stratum)
    live = R.live(rays)
    refused = (~R.guard_accepts(rays))[live].mean()
    assert 0.05 <= refused <= 0.60, (refused, stratum)


def test_the_strata_force_all_three_grid_variants():
    assert {kernel_choice(R.scene(s))["GRIDS"] for s in STRATA} == {0, 1, 2}
