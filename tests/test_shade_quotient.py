"""The shading quotient (cosx cosy) / r^2 of sceneRender (csrc/pt_device.hpp shade_vertex) with its operands at and beyond the windows of the
optimistic kernel's cheap exact divisions (csrc/pt_windows.hpp: a denominator in [2^-40, 2^40], a numerator zero or in [2^-60, 2^60]).  It is
the one division of the segment loop that is still the compiler's; a cheaper form has to equal it on all of these (profiles/segment_audit has
the form that was measured and not kept).  The 32x24 r4 fixtures with their light records edited: a light within 2^-21 of the surfaces (the
scene shrunk around it), a light 2^20 and more away, emitter normals so short that the product of the cosines falls under 2^-60 or into the
denormals, and zero normals of either sign (cosines exactly +0 / -0).  Optimistic pair == exact kernel == CPU oracle, bit for bit; and the
quotient defers nothing: the scene hands no more samples to the exact kernel than its companion whose quotient stays inside the windows
(same paths, same shadow rays: shading reads the light's `scene` record and nothing else does)."""
import numpy as np
import pytest

import a10_pass as A
from conftest import bits, load_fixture
from test_gpu_parity import _variant

pytestmark = pytest.mark.gpu

FIXTURES = ("basic_32x24_r4", "twoLights_32x24_r4", "own_flat_32x24_r4")
# near: the scale that brings r^2 = |p - light|^2 down to 2^-40 and below (the scenes' distances to their lights: about 1 in flat.xml, 4 .. 12 in the others)
NEAR_SCALE = {"basic_32x24_r4": 2.0 ** -23, "twoLights_32x24_r4": 2.0 ** -23, "own_flat_32x24_r4": 2.0 ** -21}


@pytest.fixture()
def ctx(pkg):
    from raytracing_amd.pyhost import mirt
    c = mirt.Context(0)
    yield c
    c.destroy()


def _lights(d):
    return [{k: list(v) for k, v in l.items()} for l in d["lights"]]


def _shrunk(base, s):
    """the scene scaled by s about the origin -- geometry, bounds, camera, lens, the lights' `scene` and `light` records -- with the lights'
    `shadow` records left where they were: the shadow rays still leave the surfaces towards the old, far lights (cosines well above zero),
    while the distance the shading divides by is the shrunk one"""
    d = dict(base.d)
    out = {"bounds": [v * s if k % 4 != 3 else v for k, v in enumerate(d["bounds"])], "focal_length": d["focal_length"] * s, "lens_rad": d["lens_rad"] * s}
    cam = list(d["cam"])
    cam[0:3] = [v * s for v in cam[0:3]]
    out["cam"] = cam
    if d.get("n_spheres", 0):
        out["spheres"] = [v * (s * s if k % 4 == 3 else s) for k, v in enumerate(d["spheres"])]   # (centre, radius^2)
        out["sphere_bounds"] = [v * s if k % 4 != 3 else v for k, v in enumerate(d["sphere_bounds"])]
    if d.get("n_triangles", 0):
        out["t_pos"] = [v * s for v in d["t_pos"]]
        out["triangle_bounds"] = [v * s if k % 4 != 3 else v for k, v in enumerate(d["triangle_bounds"])]
    lights = _lights(d)
    for l in lights:
        for rec in ("scene", "light"):
            l[rec][0:3] = [v * s for v in l[rec][0:3]]
        l["scene"][9] *= s * s   # area
        l["light"][9] *= s       # radius
    out["lights"] = lights
    d.update(out)
    return A.Scene(d)


def _edit(base, f):
    """(scene, companion): the lights of `base` edited by f(light, inside) -- inside=True leaves the `scene` record's quotient within the windows"""
    def make(inside):
        lights = _lights(base.d)
        for l in lights:
            f(l, inside)
        return _variant(base, lights=lights)
    return make(False), make(True)


def _far(pos):
    def f(l, inside):
        for rec in ("shadow", "light"):
            l[rec][0:3] = pos
        if not inside:
            l["scene"][0:3] = pos
    return f


def _normal(scale=None, value=None):
    def f(l, inside):
        if not inside:
            l["scene"][3:6] = [v * scale for v in l["scene"][3:6]] if value is None else [value] * 3
    return f


def _near(base, name):
    s = NEAR_SCALE[name]
    sc = _shrunk(base, s)
    lights = _lights(sc.d)
    for l in lights:   # the companion: the same shrunk scene, the divisor's light a unit away
        l["scene"][0] += 1.0
    return sc, _variant(sc, lights=lights)


CASES = {
    "near": None,
    "far": _far([2.0 ** 19.5, 2.0 ** 19.7, 2.0 ** 19.6]),     # r^2 about 2^40.8, every component within the ray guard's 2^20
    "far_edge": _far([0.0, 2.0 ** 20, 0.0]),                  # r^2 on both sides of 2^40
    "grazing_edge": _normal(scale=2.0 ** -58),                # cosx cosy on both sides of 2^-60
    "grazing": _normal(scale=2.0 ** -70),                     # all under 2^-60
    "grazing_denormal": _normal(scale=2.0 ** -135),           # cosy itself a denormal
    "zero_plus": _normal(value=0.0),                          # cosy exactly zero
    "zero_minus": _normal(value=-0.0),
}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("name", FIXTURES)
def test_quotient_at_and_beyond_the_windows(ctx, pkg, name, case):
    from raytracing_amd.pyhost import render
    _, base = load_fixture(name)
    sc, companion = _near(base, name) if case == "near" else _edit(base, CASES[case])
    seeds = A.make_seeds(sc.total_rays, seed_base=7)
    st = A.PassState(sc, seeds)
    A.run_pass(A.load_oracle(), sc, st, bounces=8)
    assert (st.acu[:, 3] > 0).any()

    def run(scene, exact_only):
        ctx.set_exact_only(exact_only)
        fr = render.FusedRenderer(ctx, scene, seeds=seeds)
        fr.execute_render(bounces=8)
        out = (fr.acu.read(np.float32).reshape(-1, 4), fr.seeds.read(np.int32), ctx.pass_deferred())
        fr.release()
        return out

    try:
        for exact_only in (False, True):
            acu, seeds_out, deferred = run(sc, exact_only)
            assert np.array_equal(bits(acu), bits(st.acu)), f"radiance, exact_only={exact_only}"
            assert np.array_equal(seeds_out, st.seeds), f"seeds, exact_only={exact_only}"
            if not exact_only:
                _, _, deferred_inside = run(companion, False)
                print(f"{name} {case}: deferred {deferred}, companion {deferred_inside}, of {sc.total_rays}")
                assert deferred <= deferred_inside, "the quotient deferred samples"
    finally:
        ctx.set_exact_only(False)

