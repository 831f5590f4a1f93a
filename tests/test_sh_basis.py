"""CPU: pyhost/rays.py sh9_basis / sh9_weights, the float64 matrices probe_sh projects with.

The weights sum to 4 pi.  The Gram matrix B^T diag(w) B is the identity up to the quadrature's error, and the bound on that error is computed
here, not guessed.  Along the longitude the rule is exact: a product of two harmonics of order <= 2 holds frequencies up to 4, and W >= 5
equispaced points integrate those exactly.  Along the latitude it is the composite midpoint rule on [-pi/2, pi/2] with h = pi / H, whose
error for an integrand g is at most (b - a) * h^2 / 24 * max |g''|.  For entry (i, j), g(t) = cos(t) * integral of Y_i Y_j over the longitude;
g and max |g''| are taken from ONE 1024 x 512 evaluation of sh9_basis itself (the longitude sum, then second differences over the 512
latitudes -- each is g'' at some point between its neighbours).  The weights are cos(latitude) NORMALISED to sum to 4 pi, which divides the
rule's by 1 + e / 2, e the same rule's error for the integral of cos, 2: |e| <= pi * h^2 / 24 (max |cos''| = 1).  Together
|G_ij - delta_ij| <= (b_cos / 2 * delta_ij + b_ij) / (1 - b_cos / 2)."""
import numpy as np
import pytest

FINE_W, FINE_H = 1024, 512
_FINE = {}


def rays_module(pkg):
    from raytracing_amd.pyhost import rays
    return rays


def second_derivative_bounds(rays):
    """-> M [9, 9]: max |g_ij''| over the latitude, from the fine evaluation"""
    if "M" not in _FINE:
        B = rays.sh9_basis(FINE_W, FINE_H).reshape(FINE_H, FINE_W, 9)
        lat = rays.sh9_directions(FINE_W, FINE_H)[1].reshape(FINE_H, FINE_W)[:, 0]
        h = np.pi / FINE_H
        assert np.allclose(np.diff(lat), -h, rtol=0, atol=1e-12), "rows run from the top: latitude falls by pi / H a row"
        g = np.einsum("hwi,hwj->hij", B, B) * (2.0 * np.pi / FINE_W) * np.cos(lat)[:, None, None]   # [H, 9, 9]
        _FINE["M"] = np.abs((g[:-2] - 2.0 * g[1:-1] + g[2:]) / (h * h)).max(axis=0)
    return _FINE["M"]


@pytest.mark.parametrize("w,h", [(32, 16), (8, 4)])
def test_weights_sum_to_four_pi(pkg, w, h):
    rays = rays_module(pkg)
    wt = rays.sh9_weights(w, h)
    assert wt.dtype == np.float64 and wt.shape == (h * w,) and (wt > 0).all()
    assert abs(wt.sum() - 4.0 * np.pi) <= 1e-12 * 4.0 * np.pi
    lat = rays.sh9_directions(w, h)[1]
    assert np.allclose(wt / wt[0], np.cos(lat) / np.cos(lat[0]), rtol=1e-13, atol=0), "the weights are cos(latitude) up to one factor"


@pytest.mark.parametrize("w,h", [(32, 16), (8, 4)])
def test_gram_matrix_is_the_identity_within_the_midpoint_rules_error(pkg, w, h):
    rays = rays_module(pkg)
    B, wt = rays.sh9_basis(w, h), rays.sh9_weights(w, h)
    assert B.dtype == np.float64 and B.shape == (h * w, 9) and w >= 5
    G = B.T @ (B * wt[:, None])
    step = np.pi / h
    b = np.pi * step * step / 24.0 * second_derivative_bounds(rays)
    b_cos = np.pi * step * step / 24.0
    bound = (b_cos / 2.0 * np.eye(9) + b) / (1.0 - b_cos / 2.0) + 1e-13   # (1e-13: float64 rounding of 512 terms of size <= 1)
    err = np.abs(G - np.eye(9))
    print(f"{w} x {h}: max |G - I| = {err.max():.3e}, bound there {bound[np.unravel_index(err.argmax(), err.shape)]:.3e}, largest bound {bound.max():.3e}")
    assert (err <= bound).all(), (err.max(), np.argwhere(err > bound).tolist())
    assert bound.max() < 1.0, "the bound says something"


def test_the_fine_evaluation_itself_is_nearly_orthonormal(pkg):
    rays = rays_module(pkg)
    B, wt = rays.sh9_basis(FINE_W, FINE_H), rays.sh9_weights(FINE_W, FINE_H)
    G = B.T @ (B * wt[:, None])
    step = np.pi / FINE_H
    b_cos = np.pi * step * step / 24.0
    bound = (b_cos / 2.0 * np.eye(9) + np.pi * step * step / 24.0 * second_derivative_bounds(rays)) / (1.0 - b_cos / 2.0) + 1e-12
    assert (np.abs(G - np.eye(9)) <= bound).all() and bound.max() < 1e-4


def test_directions_are_the_headers_equirect_formula(pkg):
    """pixel centres, right = +x, up = +y, forward = -z: d = (sin(phi) cos(th), sin(th), -cos(phi) cos(th)), phi = (2u - 1) pi, th = (1 - 2v) pi / 2"""
    rays = rays_module(pkg)
    w, h = 8, 4
    d, lat = rays.sh9_directions(w, h)
    assert d.shape == (h * w, 3) and np.allclose(np.linalg.norm(d, axis=1), 1.0, rtol=0, atol=1e-15)
    for (x, y) in ((0, 0), (3, 1), (7, 3), (4, 2)):
        phi, th = (2 * (x + 0.5) / w - 1) * np.pi, (1 - 2 * (y + 0.5) / h) * np.pi / 2
        want = (np.sin(phi) * np.cos(th), np.sin(th), -np.cos(phi) * np.cos(th))
        assert np.allclose(d[y * w + x], want, rtol=0, atol=1e-15) and abs(lat[y * w + x] - th) < 1e-15
    # the centre column looks along forward = -z, the top row up
    assert d[2 * w + 4][2] < 0 and abs(d[2 * w + 4][0]) < 0.5 and (d[:w, 1] > 0).all() and (d[-w:, 1] < 0).all()
