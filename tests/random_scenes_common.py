"""Shared by tests/test_random_scene_routes.py and tests/random_routes_child.py: a STRATIFIED generator of A10 scenes -- each stratum named after
the k_fusedPass build it forces -- and the CPU oracle's state after each progressive pass of such a scene, which every route of the library is
compared with at tolerance 0.

The pieces are those of tests/test_random_scenes.py (_tri_soup, _pack_tris, _bbox8, expected_grid, _variant) under the cornell_teapot3 fixture's
camera, materials and lights.  Every stratum except `open` is ENCLOSED: five walls of a box at +-0.98, just inside the scene bounds, open towards
the camera, normals inwards -- so that nearly every primary ray hits something and paths stay alive for all their bounces (the shares measured
on the oracle are in SHARES below; tests/test_random_scene_routes.py measures them again and holds them to the floors).

The strata, and the arithmetic of fused_lds_slots (csrc/pt_closest.hpp) and launch_fused (csrc/pt_kernels_fused.hip) behind each name, restated in
kernel_choice() below.  A set's cell table is n^3 + 1 words; sets with n > 1 make a scene a `grids` scene; the tables are staged in LDS when their
sum is at most kLdsOffWords = 4096; single-cell triangle sets of at most kLdsTriMax = 96 records are staged, in upload order, while the running
total stays within 96.

  single_cell  every set has n == 1: GRIDS 0 (with several passes the default pairing is primary-hit reuse, MULTI 2, and the guided multi-pass
               kernels run).  Loose triangles (the room among them) and 2 or 3 single-cell meshes.  seed % 3 == 0: 60, 40, 7 triangles -- 60
               staged, 60 + 40 > 96 skipped, 60 + 7 staged behind it.  seed % 3 == 1: 97, 96, 95 -- 97 can never be staged, 96 is, 96 + 95 is
               not.  seed % 3 == 2: sizes drawn around 96.
  staged       grids whose tables sum to at most 4096 words: GRIDS 1.  Resolutions 2..15; spheres and loose triangles share n_slabs.
               seed % 3 == 0: spheres and loose triangles at n_slabs 8, the room at 12, meshes at 11 and 2 (STAGED_EXACT):
               513 + 513 + 1729 + 1332 + 9 = 4096 EXACTLY, the largest sum that is staged (WAVES 5: so much LDS leaves five blocks a CU).
               seed % 3 == 1: a drawn sum of at most 4096.  seed % 3 == 2: a small one (the six-wave build).
  unstaged     the tables sum to more than 4096 words: GRIDS 2.  seed % 3 == 0: one mesh at n = 16 (16^3 + 1 = 4097, the smallest sum above the
               limit; every other set a single cell).  seed % 3 == 1: meshes at 11, 11, 9 and the room at 9 (1332 + 1332 + 730 + 730 = 4124
               and the loose sets' few words: no single table above 1332).  seed % 3 == 2: drawn, one mesh at 17 or more.
  many_sets    kMaxMeshes = 16 meshes of 1..40 triangles, single cells and grids mixed, spheres and loose triangles (the room) as well: 18 sets.
               seed % 3 == 0 and 2: GRIDS 1; seed % 3 == 1: two meshes at n = 13 take the sum past 4096, GRIDS 2.
  open         the generator of tests/test_random_scenes.py unchanged (random_scene): a few primitives in front of nothing.  Rays that miss
               everything, paths that die early, empty blocks riding along.  These are what the existing test runs; they are EXEMPT from the floors.
  guard        an enclosed scene of one of the strata above with a zero_patch in it -- a small square in the plane y == 0: a bounce ray that
               starts on it has an origin whose y is zero or the rounding's leftover, and a non-zero leftover below 2^-30 is outside the
               ray-side guard's window; which samples land so changes from pass to pass -- and edited with tests/ray_edges_common.py.
               seed % 3 == 0: a pinhole lens (PINHOLE) under the odd frame width, so that every sample of the centre column has d.x == 0
               exactly, in every pass.  seed % 3 == 1: the same, scaled by 16.  seed % 3 == 2: the fixture's lens, translated by 1 along z.
               In units of what the optimistic kernel defers (block_of), some hold a refused ray in pass 1 and some do not, and at 16 and
               64 rays per pixel some are clean in pass 1 and hold their first refused ray in pass 2: they write pass 1's frame and leave
               the launch afterwards.  At 289 rays on 9 x 5 every pixel's first 256 rays hold the NaN centre sample of the odd lens grid
               and every block of the 32-ray segment a centre-column pixel, so only the last segment's block (sample 288 of all 45 pixels)
               can be clean in pass 1: under the pinhole it is not, under the lens (seed % 3 == 2) it is and defers in pass 2 -- the case
               pass_segment's alternating carry arrays exist for.  The 289-ray cases of this stratum run on that seed.

SHARES, measured on the oracle when the seeds were chosen (37 x 21, 4 rays per pixel, the guard scenes 16; seeds make_seeds(seed_base=seed)):
the share of pixels with a first hit, then the share of samples that gain colour when the bounce count goes from j - 1 to j, j = 1..5.  Floors:
0.25 and 0.05.  (0.941 is what the room alone gives under this camera.)
  single_cell 3000  0.941   0.856 0.835 0.832 0.836 0.821        unstaged  3006  0.941   0.857 0.844 0.849 0.857 0.856
  single_cell 3001  0.941   0.524 0.483 0.467 0.446 0.420        unstaged  3007  0.941   0.684 0.664 0.650 0.629 0.623
  single_cell 3002  0.941   0.782 0.739 0.729 0.714 0.706        unstaged  3008  0.941   0.773 0.753 0.743 0.742 0.736
  staged      3003  0.941   0.727 0.695 0.695 0.695 0.688        many_sets 3009  0.941   0.614 0.561 0.546 0.516 0.503
  staged      3004  0.941   0.643 0.618 0.593 0.586 0.582        many_sets 3010  0.941   0.613 0.589 0.575 0.561 0.533
  staged      3005  0.941   0.815 0.797 0.798 0.788 0.781        many_sets 3011  0.941   0.496 0.485 0.481 0.452 0.431
  guard       3012  0.941   0.726 0.707 0.688 0.682 0.682        guard     3022  0.941   0.724 0.684 0.653 0.642 0.626
  guard       3026  0.941   0.572 0.518 0.491 0.474 0.451
At 9 x 5 x 289 rays every scene has a first hit in 0.956 of its pixels and gains within 0.02 of the row above (smallest: 0.422, single_cell 3001).
"""
import zlib

import numpy as np

import a10_pass as A
import ray_edges_common as R
from conftest import load_fixture
from guides_common import expected_guides
from pass_guided_common import PATTERN          # what a buffer holds where nobody wrote
from test_grid_build import expected_grid
from test_gpu_parity import _variant
from test_random_scenes import _bbox8, _pack_tris, _tri_soup, random_scene

BASE = "cornell_teapot3_32x24_r4"
ROOM = 0.98
K_LDS_OFF_WORDS, K_LDS_TRI_MAX, K_MAX_MESHES = 4096, 96, 16          # csrc/pt_launch.hpp
K_COOP_WORDS = 4 * (7 * 64 + 4)                                      # csrc/pt_trace_coop.hpp kCoopWordsPerBlock
STRATA = ("single_cell", "staged", "unstaged", "many_sets", "open", "guard")
ENCLOSED = tuple(s for s in STRATA if s != "open")
# three seeds per stratum, one of each residue mod 3 (the residue picks the variant), chosen on the CPU so that the oracle alone meets the floors
SEEDS = {"single_cell": (3000, 3001, 3002), "staged": (3003, 3004, 3005), "unstaged": (3006, 3007, 3008), "many_sets": (3009, 3010, 3011),
         "open": (1005, 1007, 1012), "guard": (3012, 3022, 3026)}
# the guard scenes' geometry: the stratum each is built as before the edit
GUARD_OF = {0: "single_cell", 1: "staged", 2: "many_sets"}
# Sigma (n^3 + 1) == 4096 exactly: spheres and loose triangles at n_slabs 8 (2 * 513), then the meshes, the room first (1729 + 1332 + 9)
STAGED_EXACT = (8, (12, 11, 2))
FLOOR_FIRST_HIT, FLOOR_GAIN = 0.25, 0.05
PATCH_HALF = 0.125      # half the side of the guard scenes' zero_patch


# ---- geometry ---------------------------------------------------------------------------------------------------------------------------------------
def room_tris():
    """the five walls as 10 triangles with inward vertex normals, wound as the fixture's own walls are (cross(p1 - p0, p2 - p0) along the normal: the
    reference's triangle test sees one side only, and a room wound the other way is hit by nothing)"""
    v, n = [], []
    r = ROOM
    for axis, side in ((0, -1), (0, 1), (1, -1), (1, 1), (2, -1)):
        nrm = np.zeros(3)
        nrm[axis] = -side
        a, b = (axis + 1) % 3, (axis + 2) % 3
        p = np.zeros((4, 3))
        p[:, axis] = side * r
        p[:, a] = [-r, r, r, -r]
        p[:, b] = [-r, -r, r, r]
        if np.dot(np.cross(p[1] - p[0], p[3] - p[0]), nrm) < 0:
            p = p[::-1].copy()
        for tri in ((p[0], p[1], p[2]), (p[0], p[2], p[3])):
            v.append(np.asarray(tri))
            n.append(np.tile(nrm, (3, 1)))
    return np.asarray(v, np.float32), np.asarray(n, np.float32)


def _soup(rng, count):
    """`count` triangles somewhere inside the room"""
    return _tri_soup(rng, count, rng.uniform(-0.4, 0.4, size=3), float(rng.choice([0.15, 0.4])), float(rng.choice([0.05, 0.15, 0.3])))


def _with_room(rng, count):
    """the room and count - 10 more triangles as one set"""
    rv, rn = room_tris()
    if count <= len(rv):
        return rv, rn
    v, n = _soup(rng, count - len(rv))
    return np.concatenate([rv, v]), np.concatenate([rn, n])


def zero_patch(half, centre=(0.1, -0.2)):
    """a small two-sided square in the plane y == 0 (four triangles, vertex normals +-y).  A path vertex on it has p.y = fma(t, d.y, o.y): a zero
    or the rounding's leftover, and where that is a non-zero magnitude below 2^-30 the bounce ray that starts there (its origin is p itself,
    A10 code.cl bouncePaths) is outside the ray-side guard's origin window.  Which samples land so changes from pass to pass with their seeds."""
    x, z = centre
    q = np.array([[x - half, 0, z - half], [x - half, 0, z + half], [x + half, 0, z + half], [x + half, 0, z - half]])
    up = [(q[0], q[1], q[2]), (q[0], q[2], q[3])]             # cross(p1 - p0, p2 - p0) along +y
    v = np.asarray(up + [(a, c, b) for a, b, c in up], np.float32)
    n = np.zeros((4, 3, 3), np.float32)
    n[:2, :, 1], n[2:, :, 1] = 1.0, -1.0
    return v, n


def _binned(v, n, nslabs, pad):
    b8 = _bbox8(v.reshape(-1, 3).min(axis=0) - pad, v.reshape(-1, 3).max(axis=0) + pad)
    off, order = expected_grid(1, v.reshape(len(v), 9).astype(np.float64), [b8[0], b8[1], b8[2], b8[4], b8[5], b8[6]], nslabs)
    pos, nor = _pack_tris(v, n, order)
    return b8, off, order, pos, nor


def _mesh(v, n, nslabs, matid, pad=0.0):
    """pad: 0 as tests/test_random_scenes.py has its meshes (triangles ON the faces of their box); the room as a mesh gets 0.01, since a wall in the
    far face of its own box is missed by the rays that should end on it"""
    b8, off, order, pos, nor = _binned(v, n, nslabs, pad)
    return {"pos": pos, "normal": nor, "box": off.tolist(), "matid": int(matid), "bounds": b8, "nslabs": int(nslabs), "ntriangles": len(order)}


def _loose(rng, nmat, n_slabs, tris, spheres, room=False):
    """the two loose sets at one n_slabs: `tris` = (v, n) or None, `spheres` = how many; room: the set starts with the room's 10 triangles"""
    cells = n_slabs ** 3 + 1
    out = {"n_slabs": int(n_slabs), "n_spheres": 0, "n_triangles": 0, "spheres": [], "s_matid": [], "s_box": [0] * cells, "t_pos": [], "t_normal": [],
           "t_matid": [], "t_box": [0] * cells}
    if spheres:
        c = rng.uniform(-0.6, 0.6, size=(spheres, 3))
        r = rng.uniform(0.05, 0.25, size=(spheres, 1))
        b8 = _bbox8((c - r).min(axis=0) - 0.01, (c + r).max(axis=0) + 0.01)
        off, order = expected_grid(0, np.concatenate([c, r], axis=1), [b8[0], b8[1], b8[2], b8[4], b8[5], b8[6]], n_slabs)
        sph = np.concatenate([c, r * r], axis=1).astype(np.float32)
        out.update(n_spheres=len(order), spheres=sph[order].ravel().tolist(), s_matid=rng.integers(0, nmat, size=spheres)[order].tolist(),
                   s_box=off.tolist(), sphere_bounds=b8)
    if tris is not None:
        v, n = tris
        b8, off, order, pos, nor = _binned(v, n, n_slabs, 0.01)
        mat = rng.integers(0, nmat, size=len(v))
        if room:
            mat[:10] = 4   # the room leads the set: white walls
        out.update(n_triangles=len(order), t_pos=pos, t_normal=nor, t_matid=mat[order].tolist(), t_box=off.tolist(), triangle_bounds=b8)
    return out


def _enclosed(stratum, seed, nmat, patch=None):
    """patch: (v, n) of more triangles for the loose set (the guard scenes' zero_patch)"""
    rng = np.random.default_rng(seed)

    def _more(tris):
        return tris if patch is None else (np.concatenate([tris[0], patch[0]]), np.concatenate([tris[1], patch[1]]))

    v3 = seed % 3
    white = 4
    if stratum == "single_cell":
        sizes = {0: (60, 40, 7), 1: (97, 96, 95)}.get(v3) or (int(rng.choice([40, 58, 90, 96])), int(rng.choice([30, 39, 97])), int(rng.choice([1, 6, 38])), int(rng.choice([2, 50])))
        out = _loose(rng, nmat, 1, _more(_with_room(rng, sizes[0])), int(rng.integers(0, 4)), room=True)
        out["meshes"] = [_mesh(*_soup(rng, t), 1, rng.integers(0, nmat)) for t in sizes[1:]]
    elif stratum == "staged":
        if v3 == 0:
            n_slabs, ns, spheres = STAGED_EXACT[0], STAGED_EXACT[1], int(rng.integers(1, 5))
        elif v3 == 1:
            n_slabs, ns, spheres = int(rng.integers(5, 10)), tuple(int(x) for x in rng.integers(2, 10, size=3)), int(rng.integers(1, 5))
        else:
            n_slabs, ns, spheres = int(rng.integers(2, 5)), tuple(int(x) for x in rng.integers(2, 8, size=2)), int(rng.integers(1, 5))
        out = _loose(rng, nmat, n_slabs, _more(_soup(rng, int(rng.integers(5, 40)))), spheres)
        out["meshes"] = [_mesh(*room_tris(), ns[0], white, 0.01)] + [_mesh(*_soup(rng, int(rng.choice([7, 40, 120]))), n, rng.integers(0, nmat)) for n in ns[1:]]
    elif stratum == "unstaged":
        if v3 == 0:      # one grid in the whole scene, at n = 16: the room and a soup in it
            out = _loose(rng, nmat, 1, None, int(rng.integers(1, 4)))
            out["meshes"] = [_mesh(*_with_room(rng, 130), 16, white, 0.01)]
        else:
            ns = (9, 11, 11, 9) if v3 == 1 else (int(rng.integers(2, 8)), int(rng.integers(17, 20)), int(rng.integers(2, 8)))
            out = _loose(rng, nmat, int(rng.integers(1, 4)), _soup(rng, int(rng.integers(5, 40))), int(rng.integers(0, 4)))
            out["meshes"] = [_mesh(*room_tris(), ns[0], white, 0.01)] + [_mesh(*_soup(rng, int(rng.choice([40, 150]))), n, rng.integers(0, nmat)) for n in ns[1:]]
    elif stratum == "many_sets":
        out = _loose(rng, nmat, int(rng.integers(1, 4)), _more(_with_room(rng, 10 + int(rng.integers(0, 30)))), int(rng.integers(1, 5)), room=True)
        ns = [int(x) for x in rng.choice([1, 1, 2, 3, 5], size=K_MAX_MESHES)]
        if v3 == 1:
            ns[3] = ns[11] = 13
        out["meshes"] = [_mesh(*_soup(rng, int(rng.integers(1, 41))), n, rng.integers(0, nmat)) for n in ns]
    else:
        raise KeyError(stratum)
    return out


def make_scene(stratum, seed, width, height, rpp):
    """-> a10_pass.Scene, with .key = (stratum, seed, width, height, rpp) for the caches below.  The geometry depends on (stratum, seed) alone."""
    _, base = load_fixture(BASE)
    nmat = len(base.d["materials"]) // 4
    if stratum == "open":
        sc = _variant(random_scene(base, seed, rpp), width=width, height=height)
    elif stratum == "guard":
        d = dict(_variant(base, width=width, height=height, rays_per_pixel=rpp, **_enclosed(GUARD_OF[seed % 3], seed, nmat, zero_patch(PATCH_HALF))).d)
        if seed % 3 == 0:
            d = dict(d, **R.PINHOLE)
        elif seed % 3 == 1:
            d = R.scaled(dict(d, **R.PINHOLE), 16.0)
        else:      # the fixture's lens
            d = R.translated(d, 2, 1.0)
        sc = A.Scene(d)
    else:
        sc = _variant(base, width=width, height=height, rays_per_pixel=rpp, **_enclosed(stratum, seed, nmat))
    sc.key = (stratum, int(seed), int(width), int(height), int(rpp))
    return sc


# ---- the kernel a scene forces -------------------------------------------------------------------------------------------------------------------------
def sets_of(sc):
    """(is a triangle set, n, slots) of every primitive set in upload order: spheres, loose triangles, the meshes (mirt_abi.cpp pass_setup)"""
    out = []
    if sc.has_spheres:
        out.append((False, sc.n_slabs, int(sc.s_box[-1])))
    if sc.has_triangles:
        out.append((True, sc.n_slabs, int(sc.t_box[-1])))
    return out + [(True, m["nslabs"], int(m["box"][-1])) for m in sc.meshes]


def kernel_choice(sc, passes=1, reuse=None):
    """fused_lds_slots and launch_fused in integers.  -> dict: grids; words (Sigma n^3 + 1 over the sets with n > 1); GRIDS 0 / 1 / 2; tri_staged:
    per set, whether its records get an LDS slot in the optimistic kernel; WAVES 0 / 5 of the optimistic grid kernels (reuse: MIRT_MULTIPASS_REUSE
    forced, None = the default pairing, which is reuse for scenes without grids); MULTI 0 / 1 / 2."""
    sets = sets_of(sc)
    grids = any(n != 1 for _, n, _ in sets)
    words = sum(n ** 3 + 1 for _, n, _ in sets if n > 1)
    staged = words <= K_LDS_OFF_WORDS
    tris, tri_staged = 0, []
    for tri, n, slots in sets:
        ok = tri and n == 1 and 0 < slots <= K_LDS_TRI_MAX and tris + slots <= K_LDS_TRI_MAX   # (pnorm is there up to kLdsTriMax records)
        tri_staged.append(bool(ok))
        tris += slots if ok else 0
    tri_base = K_COOP_WORDS + (words if staged else 0) if grids else 0
    lds_tri = ((-tri_base) % 4 + 28 * tris) * 4 if tris else 0
    use_reuse = (not grids) if reuse is None else bool(reuse)
    want = K_COOP_WORDS * 4 + (words * 4 if grids and staged else 0) + lds_tri
    fixed = 4 * (13 * 256 + 64 + (8 * 256 if passes > 1 and use_reuse else 0))
    granules = -(-(want + fixed) // 1280)
    return dict(grids=grids, words=words, GRIDS=0 if not grids else 1 if staged else 2, tri_staged=tri_staged,
                WAVES=5 if grids and 128 // granules < 6 else 0, MULTI=0 if passes == 1 else 2 if use_reuse else 1)


# ---- what the library's routes do with a request (csrc/pt_pass_plan.hpp, in integers) --------------------------------------------------------------------
def resolves(rpp, keep_acu, fresh=True):
    fused = rpp > 256 or 256 % rpp == 0
    if not keep_acu:
        return fresh and fused
    c = rpp // 256
    return fused and (rpp <= 256 or (rpp % 256 == 0 and c <= 32 and c & (c - 1) == 0))


def guides_in_launch(rpp, keep_acu, passes, every, default_pairing, grids, fresh=True):
    """fused_guides_in_pass / fused_guides_in_passes: whether a guided call writes the guides from the pass's own launch"""
    res = resolves(rpp, keep_acu, fresh)
    one_launch = rpp != 1 and (not every or (passes > 1 and res))
    return res and rpp in (4, 16, 64) and one_launch and (passes == 1 or (default_pairing and not grids))


# ---- the oracle's expectations, computed once -------------------------------------------------------------------------------------------------------------
_SCENES, _EXPECTED, _GUIDES = {}, {}, {}


def scene(stratum, seed, width, height, rpp):
    key = (stratum, seed, width, height, rpp)
    if key not in _SCENES:
        _SCENES[key] = make_scene(*key)
    return _SCENES[key]


class Pass:
    """the oracle's buffers after one progressive pass: acu [rays, 4], seeds, pixel [pixels, 4], radiance [pixels, 4]; read-only"""

    def __init__(self, st, rpp):
        self.acu, self.seeds, self.pixel = st.acu.copy(), st.seeds.copy(), st.pixel.copy()
        self.radiance = A.radiance_sums(self.acu, rpp)
        for a in (self.acu, self.seeds, self.pixel, self.radiance):
            a.setflags(write=False)


def expected(sc, seeds, passes, bounces=5):
    """-> [Pass after pass 1, ..., Pass after pass `passes`] of the CPU oracle from `seeds` (A.run_pass, init_acu on the first pass only), cached per
    (scene, seeds, bounces) and extended when more passes are asked for"""
    key = (sc.key, zlib.crc32(np.ascontiguousarray(seeds, np.int32).tobytes()), bounces)
    have = _EXPECTED.setdefault(key, {"st": None, "out": []})
    if have["st"] is None:
        have["st"] = A.PassState(sc, seeds)
    while len(have["out"]) < passes:
        A.run_pass(A.load_oracle(), sc, have["st"], bounces=bounces, init_acu=not have["out"])
        have["out"].append(Pass(have["st"], sc.rpp))
    return have["out"][:passes]


def guides(sc):
    """(normal_hits, albedo_depth) float32 [pixels, 4]: tests/guides_common.py expected_guides on the oracle's first-hit state"""
    if sc.key not in _GUIDES:
        _GUIDES[sc.key] = expected_guides(A.load_oracle(), sc)
    return _GUIDES[sc.key]


# ---- the conditions: what keeps a test from passing on emptiness --------------------------------------------------------------------------------------------
def shares(sc, seeds):
    """(share of pixels with a first hit, [share of samples that gain colour when the bounce count goes from j - 1 to j, j = 1..5]) on the oracle"""
    k = A.load_oracle()
    hits = guides(sc)[0][:, 3] > 0
    acu = []
    for j in range(6):
        st = A.PassState(sc, seeds)
        A.run_pass(k, sc, st, bounces=j)
        acu.append(st.acu[:, :3].copy())
    return float(hits.mean()), [float((acu[j] != acu[j - 1]).any(axis=1).mean()) for j in range(1, 6)]


# ---- the routes, each compared with expected(...) and never with another GPU route --------------------------------------------------------------------------
ROW_TILE = (5, 9)                  # rows 5..13 of 21: row0 > 0, and 9 * 37 pixels leave the tile's last block partial at every ray count
REUSE = (None, "0", "1")           # MIRT_MULTIPASS_REUSE unset, forced off, forced on (read per launch)


def words_differ(tag, got, want):
    """None when equal bit for bit (every NaN equal to every NaN: conftest.bits), else a sentence naming the first difference"""
    from conftest import bits
    g, w = bits(np.ascontiguousarray(got)).reshape(-1), bits(np.ascontiguousarray(want)).reshape(-1)
    if g.size != w.size:
        return f"{tag}: {g.size} words against {w.size}"
    bad = np.flatnonzero(g != w)
    return None if bad.size == 0 else f"{tag}: {bad.size} of {g.size} words differ, first at {int(bad[0])}: got {g[bad[0]]!r}, want {w[bad[0]]!r}"


class _Env:
    """MIRT_MULTIPASS_REUSE for the calls inside the block"""

    def __init__(self, reuse):
        self.reuse = reuse

    def __enter__(self):
        import os
        self.old = os.environ.pop("MIRT_MULTIPASS_REUSE", None)
        if self.reuse is not None:
            os.environ["MIRT_MULTIPASS_REUSE"] = self.reuse

    def __exit__(self, *exc):
        import os
        os.environ.pop("MIRT_MULTIPASS_REUSE", None)
        if self.old is not None:
            os.environ["MIRT_MULTIPASS_REUSE"] = self.old


def _renderer(ctx, sc, seeds, keep_acu, rows=None):
    """a FusedRenderer whose buffers hold patterns: acu NaN, pixel 0x5A, radiance PATTERN"""
    from raytracing_amd.pyhost import render
    fr = render.FusedRenderer(ctx, sc, seeds=seeds, keep_acu=keep_acu, **({} if rows is None else dict(row0=rows[0], nrows=rows[1])))
    if keep_acu:
        fr.acu.write(np.full(fr.nrays * 4, np.nan, np.float32))
    fr.pixel.write(np.full(fr.npix * 4, 0x5A, np.uint8))
    fr.radiance.write(np.full(fr.npix * 4, PATTERN, np.float32))
    return fr


def _frame_differs(tag, fr, want, rows=None, acu=True):
    """the renderer's seeds, pixel, radiance and (if kept) acu against one Pass of the oracle, or against its rows"""
    rpp, w = fr.s.rpp, fr.s.width
    px = slice(None) if rows is None else slice(rows[0] * w, (rows[0] + rows[1]) * w)
    ry = slice(None) if rows is None else slice(rows[0] * w * rpp, (rows[0] + rows[1]) * w * rpp)
    out = [None if np.array_equal(fr.seeds.read(np.int32), want.seeds[ry]) else f"{tag}: seeds differ",
           None if np.array_equal(fr.pixel.read(np.uint8, count=fr.npix * 4).reshape(-1, 4), want.pixel[px]) else f"{tag}: pixel differs",
           words_differ(f"{tag} radiance", fr.radiance.read(np.float32), want.radiance[px])]
    if acu and fr.acu is not None:
        out.append(words_differ(f"{tag} acu", fr.acu.read(np.float32), want.acu[ry]))
    return [x for x in out if x]


def _guides_differ(tag, got, sc, rows=None):
    want = guides(sc)
    px = slice(None) if rows is None else slice(rows[0] * sc.width, (rows[0] + rows[1]) * sc.width)
    return [x for x in (words_differ(f"{tag} normal_hits", got[0], want[0][px]), words_differ(f"{tag} albedo_depth", got[1], want[1][px])) if x]


def keeps(rpp):
    """the accumulator settings a fresh batch at this ray count can run with: without one only where the passes resolve their own pixels
    (and never at one ray per pixel, where mirt_render_passes queues ordinary passes)"""
    return (False, True) if rpp != 1 and resolves(rpp, False) else (True,)


def run_ordinary(ctx, sc, seeds, bounces=5, passes=3):
    """a fresh pass, then two more: acu, seeds, pixel and radiance after each"""
    want, out = expected(sc, seeds, passes, bounces), []
    fr = _renderer(ctx, sc, seeds, True)
    try:
        for p in range(passes):
            fr.execute_render(bounces=bounces, fresh=(p == 0))
            out += _frame_differs(f"ordinary pass {p + 1}", fr, want[p])
    finally:
        fr.release()
    return out


def run_passes(ctx, sc, seeds, n, bounces=5, every=False, rows=None, reuse=REUSE, deferred=None):
    """execute_passes(n, fresh=True) with and without a kept accumulator under every MIRT_MULTIPASS_REUSE setting; every: a frame after every
    pass, each compared with the oracle's after that pass.  deferred: a list that receives mirt_pass_deferred after each call."""
    want, out = expected(sc, seeds, n, bounces), []
    for keep_acu in keeps(sc.rpp):
        for r in reuse:
            tag = f"passes n={n} every={every} keep_acu={keep_acu} reuse={r}"
            fr = _renderer(ctx, sc, seeds, keep_acu, rows)
            try:
                if every:
                    fr._frames("_frame_pixel", n * fr.npix * 4).write(np.full(n * fr.npix * 4, 0x5A, np.uint8))
                    fr._frames("_frame_radiance", n * fr.npix * 16).write(np.full(n * fr.npix * 4, PATTERN, np.float32))
                with _Env(r):
                    frames = fr.execute_passes(n, bounces=bounces, fresh=True, every_frame=every)
                if deferred is not None:
                    deferred.append(ctx.pass_deferred())
                out += _frame_differs(tag, fr, want[n - 1], rows)
                if every:
                    w = sc.width
                    px = slice(None) if rows is None else slice(rows[0] * w, (rows[0] + rows[1]) * w)
                    for p in range(n):
                        if not np.array_equal(frames[0][p], want[p].pixel[px]):
                            out.append(f"{tag}: the pixel frame after pass {p + 1} differs")
                        out.append(words_differ(f"{tag} radiance frame after pass {p + 1}", frames[1][p], want[p].radiance[px]))
            finally:
                fr.release()
    return [x for x in out if x]


def run_guides(ctx, sc, seeds):
    fr = _renderer(ctx, sc, seeds, True)
    try:
        return _guides_differ("guides()", fr.guides(), sc)
    finally:
        fr.release()


def _pattern_guides(fr):
    for name in ("normal_hits", "albedo_depth"):
        fr._frames(name, fr.npix * 16).write(np.full(fr.npix * 4, PATTERN, np.float32))


def run_first_guided(ctx, sc, seeds, bounces=5):
    """execute_render_guided: the guides and the first pass's frame against the oracle; mirt_ctx_guided_passes moves where fused_guides_in_pass says"""
    want, out = expected(sc, seeds, 1, bounces), []
    grids = kernel_choice(sc)["grids"]
    for keep_acu in keeps(sc.rpp):
        tag = f"first pass guided keep_acu={keep_acu}"
        fr = _renderer(ctx, sc, seeds, keep_acu)
        try:
            _pattern_guides(fr)
            before = ctx.guided_passes()
            got = fr.execute_render_guided(bounces)
            routed, say = ctx.guided_passes() - before, int(guides_in_launch(sc.rpp, keep_acu, 1, False, True, grids))
            if routed != say:
                out.append(f"{tag}: mirt_ctx_guided_passes moved by {routed}, the plan says {say}")
            out += _guides_differ(tag, got, sc) + _frame_differs(tag, fr, want[0])
        finally:
            fr.release()
    return out


def run_passes_guided(ctx, sc, seeds, n, bounces=5, rows=None, reuse=REUSE, everies=(False, True)):
    """execute_passes_guided(n, fresh=True) with and without a frame after every pass: guides and frames against the oracle, and
    mirt_ctx_guided_passes against fused_guides_in_passes"""
    want, out = expected(sc, seeds, n, bounces), []
    grids = kernel_choice(sc)["grids"]
    w = sc.width
    px = slice(None) if rows is None else slice(rows[0] * w, (rows[0] + rows[1]) * w)
    for every in everies:
        for keep_acu in keeps(sc.rpp):
            for r in reuse:
                tag = f"passes guided n={n} every={every} keep_acu={keep_acu} reuse={r}"
                default_pairing = r is None or (r == "1") == (not grids)
                fr = _renderer(ctx, sc, seeds, keep_acu, rows)
                try:
                    _pattern_guides(fr)
                    before = ctx.guided_passes()
                    with _Env(r):
                        frames = fr.execute_passes_guided(n, bounces=bounces, fresh=True, every_frame=every)
                    routed, say = ctx.guided_passes() - before, int(guides_in_launch(sc.rpp, keep_acu, n, every, default_pairing, grids))
                    if routed != say:
                        out.append(f"{tag}: mirt_ctx_guided_passes moved by {routed}, the plan says {say}")
                    got = (fr.normal_hits.read(np.float32, count=4 * fr.npix).reshape(-1, 4), fr.albedo_depth.read(np.float32, count=4 * fr.npix).reshape(-1, 4))
                    out += _guides_differ(tag, got, sc, rows) + _frame_differs(tag, fr, want[n - 1], rows)
                    if every:
                        for p in range(n):
                            if not np.array_equal(frames[0][p], want[p].pixel[px]):
                                out.append(f"{tag}: the pixel frame after pass {p + 1} differs")
                            out.append(words_differ(f"{tag} radiance frame after pass {p + 1}", frames[1][p], want[p].radiance[px]))
                finally:
                    fr.release()
    return [x for x in out if x]


def run_row_tile(ctx, sc, seeds, n=2, bounces=5):
    """rows ROW_TILE of the frame through execute_passes and the guided call, against those rows of the whole frame's expectation"""
    return (run_passes(ctx, sc, seeds, n, bounces, rows=ROW_TILE, reuse=(None,)) +
            run_passes_guided(ctx, sc, seeds, n, bounces, rows=ROW_TILE, reuse=(None,), everies=(False,)))


def block_of(sc):
    """per ray id, the unit the optimistic kernel defers it in when the launch resolves its own pixels without an accumulator (csrc/pt_pass_plan.hpp):
    blocks of 256 consecutive ids where the ray count divides 256; above 256 one launch per segment of a pixel's rays (fused_segment: 289 = 256 + 32
    + 1), each in blocks of 256 / len pixels, numbered on from the segment before; at any other count the sample itself"""
    rpp, npix = sc.rpp, sc.width * sc.height
    ids = np.arange(npix * rpp)
    if rpp <= 256:
        return ids // 256 if 256 % rpp == 0 else ids
    pix, smp, out, off, first = ids // rpp, ids % rpp, np.zeros(npix * rpp, np.int64), 0, 0
    while off < rpp:
        left = rpp - off
        ln = 256 if left >= 256 else 1 << (left.bit_length() - 1)
        m = (smp >= off) & (smp < off + ln)
        out[m] = first + (pix[m] * ln + (smp[m] - off)) // 256
        first += -(-npix * ln // 256)
        off += ln
    return out


def refused_blocks_by_pass(sc, seeds, passes, win, bounces=5):
    """([per pass: the units of block_of that hold a ray the ray-side guard refuses], units in all), over EVERY ray the oracle's passes make that is
    not dead (mint == maxt) when it is made -- the primary rays (the NaN centre sample of an odd lens grid among them), every bounce ray and every
    shadow ray (a10_pass.run_pass's `watch`)"""
    st, out, unit = A.PassState(sc, seeds), [], block_of(sc)
    for p in range(passes):
        bad = np.zeros(sc.total_rays, bool)

        def watch(kind, rays, bad=bad):
            with np.errstate(invalid="ignore"):
                alive = ~(rays["mint"] == rays["maxt"])
            bad |= alive & ~R.accepted(rays["o"], rays["d"], win)
        A.run_pass(A.load_oracle(), sc, st, bounces=bounces, init_acu=(p == 0), watch=watch)
        out.append(np.unique(unit[bad]))
    return out, int(unit.max()) + 1
