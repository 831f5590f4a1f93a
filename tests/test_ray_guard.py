"""GPU: the optimistic kernel's ray-side guard (csrc/pt_trace.hpp ray_guard, shipped in its integer form: unsigned bit patterns, `bits - 1` for
"zero or at least 2^-30", 3-way minima and maxima) against the plain rule it replaces, evaluated on the device by diagnostic op 28
(include/mirt.h) and stated here in numpy (tests/ray_edges_common.py accepted()): every |d_k| in [kDenLo, kDenHi] and every o_k a zero of either sign
or |o_k| in [kPosLo, kPosHi]; NaN and infinities fail.  The four constants are read from csrc/pt_windows.hpp through tests/set_guard_dump.cpp,
as tests/test_set_guard.py reads them.  Every element must agree: a catalogue of edge values in every slot, its cross product over every pair of
slots (a minimum or maximum taken over the wrong lanes), and two generated sets of 2^21 rays in which both verdicts are common."""
import itertools

import numpy as np
import pytest

from ray_edges_common import accepted, window_constants
from test_set_guard import ask   # noqa: F401  (the module-scoped fixture that compiles tests/set_guard_dump.cpp)

pytestmark = pytest.mark.gpu

F = np.float32
N = 1 << 21
ORDINARY = F(0.5)


@pytest.fixture(scope="module")
def ctx(pkg):
    from raytracing_amd.pyhost import mirt
    c = mirt.Context(0)
    yield c
    c.destroy()


@pytest.fixture(scope="module")
def win(ask):   # noqa: F811
    return window_constants(ask)


def f32(u):
    return np.asarray(u, dtype=np.uint32).view(F)


def catalogue(win):
    """+0, the smallest and the largest denormal, each window bound with its two float neighbours; both signs of all of these (-0 among them);
    +inf, -inf and a NaN"""
    v = [F(0.0), f32(1), f32(0x007FFFFF)]
    for b in win:
        v += [np.nextafter(b, F(0.0)), b, np.nextafter(b, F(np.inf))]
    v = np.array(v, dtype=F)
    return np.concatenate([v, -v, np.array([np.inf, -np.inf, np.nan], dtype=F)])


def verdicts(ctx, rays):
    """the device's answer for rays [n, 6] = (o, d): a bool per ray"""
    rays = np.ascontiguousarray(rays, dtype=F)
    got = ctx.debug_numerics(28, rays[:, :3].copy().ravel(), rays[:, 3:].copy().ravel())
    assert got.shape == (len(rays),) and np.isin(got, (0.0, 1.0)).all()
    return got == 1.0


def check(ctx, win, rays, tag):
    rays = np.ascontiguousarray(rays, dtype=F)
    want = accepted(rays[:, :3], rays[:, 3:], win)
    got = verdicts(ctx, rays)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"{tag}: the device's verdict differs from the rule on {bad.size} of {len(rays)} rays; the first: o, d bits "
                           f"{[hex(x) for x in rays[bad[0]].view(np.uint32)]}, device {bool(got[bad[0]])}, rule {bool(want[bad[0]])}")
    return want


def test_each_catalogue_value_in_each_slot(ctx, win):
    cat = catalogue(win)
    assert len(cat) == 2 * (3 + 3 * 4) + 3
    rays = np.full((len(cat) * 6, 6), ORDINARY, dtype=F)
    for i, (v, slot) in enumerate(itertools.product(cat, range(6))):
        rays[i, slot] = v
    want = check(ctx, win, rays, "one slot")
    assert 0 < want.sum() < len(want)


def test_catalogue_cross_product_over_two_slots(ctx, win):
    cat = catalogue(win)
    a, b = np.meshgrid(cat, cat, indexing="ij")
    blocks = []
    for s, t in itertools.combinations(range(6), 2):
        rays = np.full((a.size, 6), ORDINARY, dtype=F)
        rays[:, s], rays[:, t] = a.ravel(), b.ravel()
        blocks.append(rays)
    rays = np.concatenate(blocks)
    assert len(rays) == 15 * len(cat) ** 2
    want = check(ctx, win, rays, "two slots")
    assert 0 < want.sum() < len(want)


def in_window(rng, n, lo, hi):
    """ordinary accepted values: log-uniform magnitudes in [lo, hi] with random mantissas, either sign"""
    e = rng.uniform(np.log2(float(lo)), np.log2(float(hi)), size=n)
    v = np.clip(np.exp2(e), float(lo), float(hi)).astype(F)
    return v * rng.choice(np.array([-1.0, 1.0], dtype=F), size=n)


def ordinary_rays(rng, n, win):
    den_lo, den_hi, pos_lo, pos_hi = win
    rays = np.empty((n, 6), dtype=F)
    rays[:, :3] = in_window(rng, n * 3, pos_lo, pos_hi).reshape(n, 3)
    rays[:, 3:] = in_window(rng, n * 3, den_lo, den_hi).reshape(n, 3)
    return rays


def test_uniformly_random_bit_patterns(ctx, win):
    """2^21 rays.  Six slots of uniform bits would be accepted once in four thousand draws (a slot's exponent falls into a direction's window
    80 times in 256, into an origin's 50 times), so each slot holds uniform bits with probability 1/3 and an in-window value otherwise:
    (1 - 1/3 * 176/256)^3 * (1 - 1/3 * 206/256)^3 ~ 18 % of the rays pass.  The share is computed from the rule and required to lie in [5 %, 95 %]."""
    rng = np.random.default_rng(20281)
    rays = ordinary_rays(rng, N, win)
    noise = rng.integers(0, 1 << 32, size=(N, 6), dtype=np.uint64).astype(np.uint32).view(F)
    pick = rng.random((N, 6)) < 1.0 / 3.0
    rays[pick] = noise[pick]
    want = check(ctx, win, rays, "random bits")
    share = want.mean()
    print(f"random bit patterns: {share:.2%} of {N} rays accepted by the rule")
    assert 0.05 <= share <= 0.95, f"{share:.2%} accepted: the generator no longer reaches both verdicts"


def test_log_uniform_around_each_bound(ctx, win):
    """2^21 rays.  Each slot, with probability 1/4, holds a value drawn around one of its window's two bounds: bound * 2^(+-2^-r), r uniform in
    [0, 24] -- from an octave away down to the bound itself and its nearest neighbours -- of either sign; an origin slot instead holds a zero of
    either sign or a denormal one time in sixteen.  About half of the edge draws and two thirds of the small origins fail: some 40 % of the rays pass."""
    rng = np.random.default_rng(20282)
    den_lo, den_hi, pos_lo, pos_hi = (float(x) for x in win)
    rays = ordinary_rays(rng, N, win)
    which = rng.random((N, 6))
    r = rng.uniform(0.0, 24.0, size=(N, 6))
    factor = np.exp2(rng.choice([-1.0, 1.0], size=(N, 6)) * np.exp2(-r))
    low_side = rng.random((N, 6)) < 0.5
    bound = np.empty((N, 6))
    bound[:, :3] = np.where(low_side[:, :3], pos_lo, pos_hi)
    bound[:, 3:] = np.where(low_side[:, 3:], den_lo, den_hi)
    edge = (bound * factor).astype(F) * rng.choice(np.array([-1.0, 1.0], dtype=F), size=(N, 6))
    pick = which < 0.25
    rays[pick] = edge[pick]
    small = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1.1754942e-38], dtype=F)
    tiny = (which >= 0.25) & (which < 0.25 + 1.0 / 16.0)
    tiny[:, 3:] = False
    rays[tiny] = small[rng.integers(0, len(small), size=int(tiny.sum()))]
    want = check(ctx, win, rays, "around the bounds")
    share = want.mean()
    print(f"log-uniform around the bounds: {share:.2%} of {N} rays accepted by the rule")
    assert 0.05 <= share <= 0.95, f"{share:.2%} accepted: the generator no longer reaches both verdicts"
    exact = (np.abs(rays) == np.concatenate([np.full(3, win[2]), np.full(3, win[0])]).astype(F)).any(axis=1).sum()
    assert exact > 0      # some draws land on a bound itself


def test_the_op_list_ends_at_the_guard(ctx):
    """op 28 is the last diagnostic op: the next number is refused by name, and the guard needs both of its inputs"""
    from raytracing_amd.pyhost import mirt
    rays = np.full((4, 3), ORDINARY, dtype=F)
    with pytest.raises(mirt.MirtError) as e:
        ctx.debug_numerics(29, rays.ravel(), rays.ravel())
    assert e.value.code == -1 and "20..28" in str(e.value)
    with pytest.raises(mirt.MirtError) as e:
        ctx.debug_numerics(28, rays.ravel())
    assert e.value.code == -1 and "two inputs" in str(e.value)
    assert verdicts(ctx, np.full((4, 6), ORDINARY, dtype=F)).all()      # the context still works
