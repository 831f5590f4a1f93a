"""CPU: the numpy restatement of the view cameras' ray definition (tests/view_common.py), on its own.

  * the standard inputs of the GPU tests exercise what they are meant to, through the oracle: at least half of the live rays hit, at least one
    ray sees an emitter, at least one equirect ray misses, the fisheye has a dead sample, and the ray-side guard accepts every live ray;
  * exact properties of the definition at odd width and height with k = 1: the centre sample of EQUIRECT and of FISHEYE has d == forward bit for
    bit, that of ORTHOGRAPHIC o == eye bit for bit;
  * a tile's rays equal the same rows of the whole frame's;
  * ray ids follow the (pixel, sy, sx) order."""
import numpy as np
import pytest

import radiance_common as RC
import rays_common as R
import view_common as V
from conftest import bits, load_fixture

FIXTURES = ("cornell_32x24_r4", "cornell_teapot3_32x24_r4")
MODELS = ("ortho", "equirect", "fisheye")


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", FIXTURES)
def test_the_standard_inputs_exercise_hits_misses_emitters_and_dead_samples(name, model):
    _, sc = load_fixture(name)
    rays = V.view_rays(V.standard_view(sc, model))
    assert len(rays) == 364
    live = R.live(rays)
    hits, _ = R.expected_closest(sc, rays)
    hit = live & (hits[:, 7].view(np.int32) >= 0)
    sees = RC.light_intercepts(sc, rays)
    print(f"{name} {model}: live {int(live.sum())}, hit {int(hit.sum())}, miss {int((live & ~hit).sum())}, dead {int((~live).sum())}, see an emitter {int(sees.sum())}")
    assert 2 * hit.sum() >= live.sum(), "fewer than half of the live rays hit"
    assert sees.any(), "no ray sees an emitter"
    assert R.guard_accepts(rays[live]).all(), "the ray-side guard refuses a live ray: the optimistic kernel is not exercised"
    if model == "equirect":
        assert (live & ~hit).any(), "no equirect ray misses"
    if model == "fisheye":
        assert (~live).any(), "the fisheye has no dead sample"
        dead = rays[~live]
        assert (dead[:, 3] == 0).all() and (dead[:, 7] == 0).all() and (bits(dead[:, 4:7]) == bits(V.standard_view(sc, model).forward)).all()
    else:
        assert live.all()


def _centre_view(model):
    right, up, fwd = V.standard_basis()
    return V.View(model, 13, 7, 1, (0.25, -1.5, 3.0), right, up, fwd, half_w=0.7, half_h=0.3, half_angle=1.1, t_min=0.125, t_max=50.0)


@pytest.mark.parametrize("model", ("equirect", "fisheye"))
def test_the_centre_sample_looks_along_forward_bit_for_bit(model):
    v = _centre_view(model)
    r = V.view_rays(v)[3 * 13 + 6]
    assert np.array_equal(bits(r[4:7]), bits(v.forward)), (r[4:7], v.forward)
    assert np.array_equal(bits(r[0:3]), bits(v.eye)) and r[3] == v.t_min and r[7] == v.t_max


def test_the_centre_sample_of_the_orthographic_camera_starts_at_the_eye():
    v = _centre_view("ortho")
    r = V.view_rays(v)[3 * 13 + 6]
    assert np.array_equal(bits(r[0:3]), bits(v.eye)), (r[0:3], v.eye)
    assert np.array_equal(bits(r[4:7]), bits(v.forward))


@pytest.mark.parametrize("k", V.KS)
@pytest.mark.parametrize("model", MODELS)
def test_a_tiles_rays_are_the_frames_rows(model, k):
    _, sc = load_fixture(FIXTURES[0])
    v = V.standard_view(sc, model, k=k)
    whole = V.view_rays(v)
    per_row = v.width * v.rpp
    for row0, nrows in ((0, 3), (3, 1), (4, 3)):
        tile = V.view_rays(v.tile(row0, nrows))
        assert len(tile) == nrows * per_row
        assert np.array_equal(bits(tile), bits(whole[row0 * per_row:(row0 + nrows) * per_row])), (model, k, row0, nrows)


@pytest.mark.parametrize("k", (2, 4))
def test_ray_ids_follow_pixel_then_sy_then_sx(k):
    """ORTHOGRAPHIC with an axis basis and unit window: o.x = a = 2 fx / W - 1 grows with x and sx, o.y = b = 1 - 2 fy / H falls with y and sy"""
    W, H = 5, 3
    v = V.View("ortho", W, H, k, (0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, -1))
    o = V.view_rays(v)[:, 0:3].reshape(H, W, k, k, 3)
    assert (np.diff(o[..., 0], axis=3) > 0).all() and (np.diff(o[..., 0], axis=1) > 0).all(), "x does not grow along sx and along the pixel column"
    assert (np.diff(o[..., 1], axis=2) < 0).all() and (np.diff(o[..., 1], axis=0) < 0).all(), "y does not fall along sy and along the pixel row"
    assert (np.diff(o[..., 0], axis=2) == 0).all() and (np.diff(o[..., 1], axis=3) == 0).all() and (o[..., 2] == 0).all()
    # the first sample of pixel (0, 0): fx = 0.5 / k, a = 2 fx / W - 1 in the definition's operations
    f32 = np.float32
    fx = f32(0) + (f32(0) + f32(0.5)) * (f32(1) / f32(k))
    u = fx / f32(W)
    assert o[0, 0, 0, 0, 0] == (u + u) - f32(1)
    # the sample positions of one pixel are k x k distinct points strictly inside it
    ax = (o[1, 2, :, :, 0].astype(np.float64) + 1) / 2 * W
    assert (ax > 2).all() and (ax < 3).all() and len(np.unique(o[1, 2, :, :, 0:2].reshape(-1, 2), axis=0)) == k * k
