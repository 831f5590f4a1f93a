"""GPU: the shadow stage's plane-free gap (csrc/pt_direct.hpp gap_test, csrc/pt_shadow_gap.hpp) end to end.  Every frame -- 64 x 48 or smaller, 16
rays per pixel, depth 8 -- runs three ways: the optimistic pair (whose shadow stage takes the early-out wherever a whole wave passes the gap test),
the exact kernel alone, and the CPU oracle; seeds, per-ray radiance sums and RGBA8 pixels must be bit-identical across all three.

The scenes are chosen by what the early-out does on them (the hit rates are in DESIGN.md section 8; a -DPT_COUNT build reads them):
  cornell           nearly every wave passes: origins 0.001 off a surface, the light's disk inside the room
  cornell_x1024     the room scaled by 2^10: the 0.001 offset is inside the margin of the walls' planes, the early-out refuses, the box test runs
  light_beyond      the light outside the room's open side: every segment ends beyond the box face, outside the gap
  strip             a short wall at x = -0.7: floor points behind its plane lie in the strip between the plane and the box face -- waves that mix
                    passing and refusing lanes
  forty             cornell's twelve triangles and 28 more in quads: two chunks of the plane list, gaps narrowed by the quads' planes
  general_only      no axis plane at all: the gap is the box, the early-out skips the box test alone
  quad soups        tests/test_random_scenes.py's generator, imported: axis and general planes, back masks, chunk boundaries, 97 records (no list)"""
import numpy as np
import pytest

import a10_pass as A
from conftest import bits, load_fixture
from ray_edges_common import _variant
from test_random_scenes import quad_scene

pytestmark = pytest.mark.gpu

W, H, RPP, DEPTH = 64, 48, 16, 8


@pytest.fixture()
def ctx(pkg):
    from raytracing_amd.pyhost import mirt
    c = mirt.Context(0)
    yield c
    c.destroy()


def _f32(v):
    return [float(x) for x in np.asarray(v, np.float32).ravel()]


def _base():
    _, base = load_fixture("cornell_32x24_r4")
    return base


def _tris(base):
    d = base.d
    return (np.asarray(d["t_pos"], np.float32).reshape(-1, 3, 4).copy(), np.asarray(d["t_normal"], np.float32).reshape(-1, 3, 4).copy(),
            list(d["t_matid"]))


def _with_tris(base, pos, nor, matid, **kw):
    n = len(matid)
    return _variant(base, width=W, height=H, rays_per_pixel=RPP, n_triangles=n, t_pos=_f32(pos), t_normal=_f32(nor), t_matid=[int(m) for m in matid],
                    t_box=[0, n], **kw)


def cornell(base):
    return _variant(base, width=W, height=H, rays_per_pixel=RPP)


def cornell_scaled(base, s):
    """every length of the scene times s, a power of two (exact in fp32); the shadow ray's 0.001 offset stays what it is"""
    d = base.d
    s = np.float32(s)

    def b8(v):
        v = np.asarray(v, np.float32) * np.array([s, s, s, 1, s, s, s, 1], np.float32)
        return _f32(v)
    pos = np.asarray(d["t_pos"], np.float32).reshape(-1, 4) * np.array([s, s, s, 1], np.float32)
    sph = np.asarray(d["spheres"], np.float32).reshape(-1, 4) * np.array([s, s, s, s * s], np.float32)
    cam = list(d["cam"])
    cam[0:3] = _f32(np.asarray(cam[0:3], np.float32) * s)   # (the image plane's extent is given at unit distance: it stays)
    lights = []
    for L in d["lights"]:
        sh, sc, li = (np.asarray(L[k], np.float32).copy() for k in ("shadow", "scene", "light"))
        sh[0:3] *= s; sh[9] *= s           # position, radius
        sc[0:3] *= s; sc[9] *= s * s       # position, area
        li[0:3] *= s; li[9] *= s           # position, radius
        lights.append({"shadow": _f32(sh), "scene": _f32(sc), "light": _f32(li)})
    return _variant(base, width=W, height=H, rays_per_pixel=RPP, cam=cam, focal_length=float(np.float32(d["focal_length"]) * s),
                    lens_rad=float(np.float32(d["lens_rad"]) * s), bounds=b8(d["bounds"]), sphere_bounds=b8(d["sphere_bounds"]),
                    triangle_bounds=b8(d["triangle_bounds"]), t_pos=_f32(pos), spheres=_f32(sph), lights=lights)


def light_beyond(base):
    """the light's disk at z = 1.5, facing the room through its open side: beyond the box face z = 1"""
    L = base.d["lights"][0]
    sh, sc, li = (np.asarray(L[k], np.float32).copy() for k in ("shadow", "scene", "light"))
    sh[0:3] = (0, 0, 1.5); sh[3:6] = (1, 0, 0); sh[6:9] = (0, 1, 0)
    sc[0:3] = (0, 0, 1.5); sc[3:6] = (0, 0, -1)
    li[0:3] = (0, 0, 1.5); li[3:6] = (0, 0, -1)
    return _variant(base, width=W, height=H, rays_per_pixel=RPP, lights=[{"shadow": _f32(sh), "scene": _f32(sc), "light": _f32(li)}])


def strip(base):
    """the left wall moved to x = -0.7 and cut to z in [-1, 0]: the camera sees the floor, the ceiling and the back wall behind its plane"""
    pos, nor, matid = _tris(base)
    for t in range(len(matid)):
        if np.all(pos[t, :, 0] == np.float32(-0.99)):
            pos[t, :, 0] = np.float32(-0.7)
            pos[t, :, 2] = np.minimum(pos[t, :, 2], np.float32(0.0))
    return _with_tris(base, pos, nor, matid)


def _quads(rng, count, general):
    """count triangles in quads inside the room: axis-aligned on a 1/64 lattice, or (general) slanted"""
    pos, nor, k = np.zeros((count, 3, 4), np.float32), np.zeros((count, 3, 4), np.float32), 0
    while k < count:
        c = rng.uniform(-0.6, 0.6, size=3)
        if general:
            u, w = rng.normal(size=3) * 0.2, rng.normal(size=3) * 0.2
        else:
            ax = int(rng.integers(0, 3))
            u, w = np.zeros(3), np.zeros(3)
            u[(ax + 1) % 3] = float(rng.integers(2, 20)) / 64.0
            w[(ax + 2) % 3] = float(rng.integers(2, 20)) / 64.0
            c = np.round(c * 64.0) / 64.0
            if rng.random() < 0.5:
                u, w = w, u
        p = [c, c + u, c + u + w, c + w]
        n = np.cross(w, u)
        n = n / (np.linalg.norm(n) + 1e-30)
        for tri in ((p[0], p[1], p[2]), (p[0], p[2], p[3])):
            if k < count:
                pos[k, :, :3] = np.asarray(tri, np.float32)
                nor[k, :, :3] = n.astype(np.float32)
                k += 1
    return pos, nor


def forty(base):
    pos, nor, matid = _tris(base)
    rng = np.random.default_rng(40)
    p2, n2 = _quads(rng, 28, general=False)
    return _with_tris(base, np.concatenate([pos, p2]), np.concatenate([nor, n2]), matid + rng.integers(0, 6, size=28).tolist())


def general_only(base):
    pos, nor, matid = _tris(base)
    keep = [t for t in range(len(matid)) if len({float(x) for x in pos[t, :, 0]}) > 1 and len({float(x) for x in pos[t, :, 1]}) > 1 and len({float(x) for x in pos[t, :, 2]}) > 1]
    rng = np.random.default_rng(41)
    p2, n2 = _quads(rng, 10, general=True)
    return _with_tris(base, np.concatenate([pos[keep], p2]), np.concatenate([nor[keep], n2]), [matid[t] for t in keep] + rng.integers(0, 6, size=10).tolist())


SCENES = {
    "cornell": cornell,
    "cornell_x1024": lambda b: cornell_scaled(b, 1024.0),
    "light_beyond": light_beyond,
    "strip": strip,
    "forty": forty,
    "general_only": general_only,
    "quads_12": lambda b: _variant(quad_scene(b, 612, 12), rays_per_pixel=RPP),
    "quads_33_two_sided": lambda b: _variant(quad_scene(b, 633, 33, two_sided=0.4, shuffle=True), rays_per_pixel=RPP),
    "quads_96_two_sided": lambda b: _variant(quad_scene(b, 696, 96, two_sided=0.4, shuffle=True), rays_per_pixel=RPP),
    "quads_97_no_list": lambda b: _variant(quad_scene(b, 697, 97, two_sided=0.4, shuffle=True), rays_per_pixel=RPP),
}


@pytest.mark.parametrize("name", list(SCENES))
def test_optimistic_pair_exact_kernel_and_oracle_agree(ctx, pkg, name):
    from raytracing_amd.pyhost import render
    sc = SCENES[name](_base())
    assert sc.d["width"] <= W and sc.d["height"] <= H and sc.d["rays_per_pixel"] == RPP
    seeds = A.make_seeds(sc.total_rays, seed_base=len(name))
    st = A.PassState(sc, seeds)
    A.run_pass(A.load_oracle(), sc, st, bounces=DEPTH)
    for exact_only in (False, True):
        ctx.set_exact_only(exact_only)
        fr = render.FusedRenderer(ctx, sc, seeds=seeds)
        fr.execute_render(bounces=DEPTH)
        assert np.array_equal(fr.seeds.read(np.int32), st.seeds), f"seeds, exact_only={exact_only}"
        assert np.array_equal(bits(fr.acu.read(np.float32).reshape(-1, 4)), bits(st.acu)), f"radiance sums, exact_only={exact_only}"
        assert np.array_equal(fr.pixel.read(np.uint8).reshape(-1, 4), st.pixel), f"pixels, exact_only={exact_only}"
        fr.release()
    ctx.set_exact_only(False)
    if name != "quads_97_no_list":
        assert (st.acu[:, 3] > 0).any()       # something is lit: shadow queries ran
