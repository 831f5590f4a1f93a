"""Randomly generated scenes through every path: the fused pass (optimistic pair and exact-only), the kernel-by-kernel path and the CPU oracle
must agree bit for bit.  The generator varies what the fixtures do not: how many sets there are, their grid resolutions (1..7 cells per axis,
loose sets included), how full the cells are (hundreds of slots in one cell, whole grids nearly empty), overlapping meshes, tiny and huge
primitives, one to three lights.  Geometry is binned by the restatement of the reference host's split*Data (tests/test_grid_build.py).

What these scenes reach, measured on the CPU oracle (seeds 1000 + s, 48 x 27): a few primitives in front of nothing, so most paths end at their
first vertex.
  s                        0    1    2    3    4    5    6    7    8    9    10   11   12   13   14   15
  pixels with a first hit  .03  .03  .19  .03  .00  .48  .14  .45  .37  .00  .05  .02  .41  .35  .41  .02
  samples with any light   .025 .022 .051 .008 .003 .111 .075 .092 .113 .003 .036 .008 .097 .052 .101 .020
Eight of the sixteen hit something in at most 5 % of their pixels (1004 and 1009 practically nothing); 0.5 - 5 % of the samples gain light at a
given bounce.  They run one ordinary pass of k_fusedPass<*, 1, 0, 0> (staged grids, well under 4096 table words) and the kernel-by-kernel path.
Enclosed scenes that keep their paths alive, one stratum per kernel choice, through every multi-pass, every-frame and guided route against the
oracle: tests/test_random_scene_routes.py (generator: tests/random_scenes_common.py, whose `open` stratum is random_scene below)."""
import os

import numpy as np
import pytest

import a10_pass as A
from conftest import assert_state_equals_pass_state, bits, load_fixture
from test_grid_build import expected_grid
from test_gpu_parity import _variant, snapshot

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ctx(pkg):
    from raytracing_amd.pyhost import mirt
    c = mirt.Context(0)
    yield c
    c.destroy()


def _bbox8(lo, hi):
    lo, hi = np.float32(lo), np.float32(hi)
    return [float(lo[0]), float(lo[1]), float(lo[2]), 1.0, float(hi[0]), float(hi[1]), float(hi[2]), 1.0]


def _tri_soup(rng, count, centre, spread, size):
    c = centre + rng.uniform(-spread, spread, size=(count, 1, 3))
    v = (c + rng.uniform(-size, size, size=(count, 3, 3))).astype(np.float32)
    n = rng.normal(size=(count, 3, 3))
    n = (n / np.linalg.norm(n, axis=2, keepdims=True)).astype(np.float32)
    return v, n


def _pack_tris(v, n, order):
    pos = np.zeros((len(order), 3, 4), np.float32)
    nor = np.zeros((len(order), 3, 4), np.float32)
    pos[:, :, :3] = v[order]
    nor[:, :, :3] = n[order]
    return pos.ravel().tolist(), nor.ravel().tolist()


def random_scene(base, seed, rpp=None):
    """rpp: the rays per pixel instead of the scene's own draw (1 or 4) -- for checks against the reference binary ON the GPU, where initTrace at one ray
    per pixel races on seeds[column] (oracle/ref_gpu.py)"""
    rng = np.random.default_rng(seed)
    d = dict(base.d)
    nmat = len(d["materials"]) // 4
    n_loose = int(rng.integers(1, 4))
    out = {"n_slabs": n_loose, "n_spheres": 0, "n_triangles": 0, "spheres": [], "s_matid": [], "s_box": [0] * (n_loose ** 3 + 1),
           "t_pos": [], "t_normal": [], "t_matid": [], "t_box": [0] * (n_loose ** 3 + 1)}
    ks = int(rng.integers(0, 7))
    if ks:
        c = rng.uniform(-0.8, 0.8, size=(ks, 3))
        r = rng.uniform(0.04, 0.35, size=(ks, 1))
        lo, hi = (c - r).min(axis=0) - 0.01, (c + r).max(axis=0) + 0.01
        b8 = _bbox8(lo, hi)
        off, order = expected_grid(0, np.concatenate([c, r], axis=1), [b8[0], b8[1], b8[2], b8[4], b8[5], b8[6]], n_loose)
        sph = np.concatenate([c, r * r], axis=1).astype(np.float32)
        out.update(n_spheres=len(order), spheres=sph[order].ravel().tolist(), s_matid=rng.integers(0, nmat, size=ks)[order].tolist(),
                   s_box=off.tolist(), sphere_bounds=b8)
    kt = int(rng.integers(0, 40))
    if kt:
        v, n = _tri_soup(rng, kt, np.zeros(3), 0.8, float(rng.choice([0.05, 0.3, 1.2])))
        b8 = _bbox8(v.reshape(-1, 3).min(axis=0) - 0.01, v.reshape(-1, 3).max(axis=0) + 0.01)
        off, order = expected_grid(1, v.reshape(kt, 9).astype(np.float64), [b8[0], b8[1], b8[2], b8[4], b8[5], b8[6]], n_loose)
        pos, nor = _pack_tris(v, n, order)
        out.update(n_triangles=len(order), t_pos=pos, t_normal=nor, t_matid=rng.integers(0, nmat, size=kt)[order].tolist(), t_box=off.tolist(),
                   triangle_bounds=b8)
    meshes = []
    for _ in range(int(rng.integers(0, 4))):
        T = int(rng.choice([1, 7, 40, 150, 400]))
        n_m = int(rng.integers(1, 8))
        v, n = _tri_soup(rng, T, rng.uniform(-0.5, 0.5, size=3), float(rng.choice([0.05, 0.3])), float(rng.choice([0.02, 0.1, 0.4])))
        b8 = _bbox8(v.reshape(-1, 3).min(axis=0), v.reshape(-1, 3).max(axis=0))
        off, order = expected_grid(1, v.reshape(T, 9).astype(np.float64), [b8[0], b8[1], b8[2], b8[4], b8[5], b8[6]], n_m)
        pos, nor = _pack_tris(v, n, order)
        meshes.append({"pos": pos, "normal": nor, "box": off.tolist(), "matid": int(rng.integers(0, nmat)), "bounds": b8, "nslabs": n_m,
                       "ntriangles": len(order)})
    out["meshes"] = meshes
    out["lights"] = [d["lights"][i % len(d["lights"])] for i in range(int(rng.integers(1, 4)))]
    w = int(os.environ.get("MIRT_SOAK_W", "48"))
    own = int(rng.choice([1, 4]))
    return _variant(base, width=w, height=max(1, w * 9 // 16), rays_per_pixel=rpp or own, **out)


# MIRT_SOAK=N: N scenes instead of 16 (a longer hunt for a rare disagreement; not part of the default run)
@pytest.mark.parametrize("seed", range(int(os.environ.get("MIRT_SOAK", "16"))))
def test_random_scene_all_paths_agree(ctx, pkg, seed):
    from raytracing_amd.pyhost import render
    _, base = load_fixture("cornell_teapot3_32x24_r4")
    sc = random_scene(base, 1000 + seed)
    seeds = A.make_seeds(sc.total_rays, seed_base=seed)
    st = A.PassState(sc, seeds)
    A.run_pass(A.load_oracle(), sc, st)
    for exact_only in (False, True):
        ctx.set_exact_only(exact_only)
        fr = render.FusedRenderer(ctx, sc, seeds=seeds)
        fr.execute_render()
        assert np.array_equal(bits(fr.acu.read(np.float32).reshape(-1, 4)), bits(st.acu)), f"fused, exact_only={exact_only}"
        assert np.array_equal(fr.seeds.read(np.int32), st.seeds)
        assert np.array_equal(fr.pixel.read(np.uint8).reshape(-1, 4), st.pixel)
        fr.release()
        # the same frame from the pass that resolves its own pixels, without a per-ray accumulator (rays per pixel 1 or 4: whole pixels per block)
        fr = render.FusedRenderer(ctx, sc, seeds=seeds, keep_acu=False)
        fr.execute_render(fresh=True)
        assert np.array_equal(fr.seeds.read(np.int32), st.seeds), f"in-pass resolve, exact_only={exact_only}"
        assert np.array_equal(fr.pixel.read(np.uint8).reshape(-1, 4), st.pixel), f"in-pass resolve, exact_only={exact_only}"
        fr.release()
    ctx.set_exact_only(False)
    gr = render.GranularRenderer(ctx, sc, seeds=seeds)
    gr.execute_render()
    got = snapshot(gr)
    assert np.array_equal(bits(got["acu"]), bits(st.acu)) and np.array_equal(got["seeds"], st.seeds), "kernel by kernel"
    assert np.array_equal(got["pois"]["matId"], st.pois["matId"])
    assert_state_equals_pass_state("kernel by kernel", got, st)   # every Ray, shadow Ray (a blocked one's stored t included) and vertex
    gr.release()


def quad_scene(base, seed, n_tris, two_sided=0.0, shuffle=False):
    """Loose triangles that come in coplanar PAIRS (the halves of rectangles, same winding: bit-identical plane normals where the
    arithmetic is exact, nearly identical elsewhere), as scenes built from quads have them; an odd count leaves a single at the end.
    Sizes around the 32-record chunks of the candidate sweep, so a pair straddles a chunk boundary (records 31 | 32, 63 | 64)."""
    rng = np.random.default_rng(seed)
    d = dict(base.d)
    nmat = len(d["materials"]) // 4
    v = np.zeros((n_tris, 3, 3), np.float32)
    nrm = np.zeros((n_tris, 3, 3), np.float32)
    k = 0
    while k < n_tris:
        axis_aligned = rng.random() < 0.6
        c = rng.uniform(-0.8, 0.8, size=3)
        if axis_aligned:   # exact arithmetic: coordinates on a 1/64 lattice, edges along two axes
            ax = int(rng.integers(0, 3))
            u, w = np.zeros(3), np.zeros(3)
            u[(ax + 1) % 3] = float(rng.integers(2, 40)) / 64.0
            w[(ax + 2) % 3] = float(rng.integers(2, 40)) / 64.0
            c = np.round(c * 64.0) / 64.0
            if rng.random() < 0.5:
                u, w = w, u
        else:
            u, w = rng.normal(size=3) * 0.3, rng.normal(size=3) * 0.3
        p = [c, c + u, c + u + w, c + w]
        n = np.cross(w, u)
        n = n / (np.linalg.norm(n) + 1e-30)
        quad = [((p[0], p[1], p[2]), n), ((p[0], p[2], p[3]), n)]
        if rng.random() < two_sided:   # the same two triangles again with the winding reversed: the back faces (the plane list's back masks)
            quad += [((a, c2, b), -n) for (a, b, c2), _ in quad]
        for tri, nn in quad:
            if k < n_tris:
                v[k] = np.asarray(tri, np.float32)
                nrm[k] = nn.astype(np.float32)
                k += 1
    if shuffle:   # the halves of a quad and the twins anywhere in the list: merged through the entry masks, not through adjacency
        perm = rng.permutation(n_tris)
        v, nrm = v[perm], nrm[perm]
    b8 = _bbox8(v.reshape(-1, 3).min(axis=0) - 0.01, v.reshape(-1, 3).max(axis=0) + 0.01)
    off, order = expected_grid(1, v.reshape(n_tris, 9).astype(np.float64), [b8[0], b8[1], b8[2], b8[4], b8[5], b8[6]], 1)
    assert np.array_equal(order, np.arange(n_tris))      # one cell: upload order kept, pairs stay adjacent
    pos, nor = _pack_tris(v, nrm, order)
    out = {"n_slabs": 1, "n_spheres": 0, "spheres": [], "s_matid": [], "s_box": [0, 0], "n_triangles": n_tris, "t_pos": pos, "t_normal": nor,
           "t_matid": rng.integers(0, nmat, size=n_tris).tolist(), "t_box": off.tolist(), "triangle_bounds": b8, "meshes": [],
           "lights": [d["lights"][0]]}
    return _variant(base, width=64, height=36, rays_per_pixel=4, **out)


@pytest.mark.parametrize("variant", ["pairs", "two_sided_shuffled"])
@pytest.mark.parametrize("n_tris", [2, 12, 31, 33, 63, 65, 95, 96, 97])
def test_quad_soups_through_the_plane_list(ctx, pkg, n_tris, variant):
    """The candidate sweep's plane list (k_planeList): records merged per plane through masks (adjacent halves of a quad; with
    `two_sided_shuffled` the halves anywhere in the list and back faces in the back masks), axis planes and general ones, chunk boundaries
    inside a pair, the last staged size (96) and the first that falls back to the wave-uniform loop (97) -- optimistic pair == exact
    kernel == CPU oracle."""
    from raytracing_amd.pyhost import render
    _, base = load_fixture("cornell_32x24_r4")
    sc = quad_scene(base, 77 + n_tris, n_tris) if variant == "pairs" else quad_scene(base, 177 + n_tris, n_tris, two_sided=0.4, shuffle=True)
    seeds = A.make_seeds(sc.total_rays, seed_base=n_tris)
    st = A.PassState(sc, seeds)
    A.run_pass(A.load_oracle(), sc, st, bounces=8)
    for exact_only in (False, True):
        ctx.set_exact_only(exact_only)
        fr = render.FusedRenderer(ctx, sc, seeds=seeds)
        fr.execute_render(bounces=8)
        assert np.array_equal(bits(fr.acu.read(np.float32).reshape(-1, 4)), bits(st.acu)), f"fused, exact_only={exact_only}"
        assert np.array_equal(fr.seeds.read(np.int32), st.seeds)
        fr.release()
    ctx.set_exact_only(False)
    assert (st.acu[:, 3] > 0).any()       # the soup is hit


@pytest.mark.parametrize("n_tris", [1, 12, 32, 33, 64, 96])
def test_device_plane_list_equals_the_cpu_restatement(ctx, pkg, n_tris):
    """k_planeList on the device against oracle/sweep_check.c's word-for-word restatement, fed the device's own prepared records: header,
    classes, masks, back masks, padding, the chunks' largest margin constants -- byte for byte.  (The restatement's layout properties and the
    soundness of the sweep over it are CPU tests: tests/test_sweep_filter.py.)"""
    import ctypes as C
    import os
    from conftest import ROOT
    _, base = load_fixture("cornell_32x24_r4")
    sc = quad_scene(base, 500 + n_tris, n_tris, two_sided=0.4, shuffle=True)
    pos = ctx.buffer_from(np.asarray(sc.t_pos, np.float32))
    raw = ctx.prepared(pos, n_tris)
    pos.release()
    rec = raw[:48 * n_tris].view(np.float32).copy()
    off = (48 * n_tris + (n_tris + 15) // 16 * 16 + 63) & ~63          # pt_launch.hpp prepared_planes_offset
    dev = raw[off:].view(np.uint32)
    lib = C.CDLL(os.path.join(ROOT, "oracle", "liboracle.so"))
    lib.oracle_plane_list.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    lib.oracle_plane_list.restype = C.c_uint32
    cpu = np.zeros(16 + 4 * 320, np.uint32)
    used = lib.oracle_plane_list(rec.ctypes.data, n_tris, cpu.ctypes.data)
    assert used <= dev.size
    assert np.array_equal(dev[:used], cpu[:used])
