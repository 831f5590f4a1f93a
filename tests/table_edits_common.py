"""Shared by tests/test_table_edits_cpu.py, tests/test_hand_made_tables.py and tests/test_table_rewrite.py: EDITS of a packed scene's cell tables.

include/mirt.h accepts any non-decreasing cell table (THE CELL TABLE at mirt_grid); every result is what the reference's kernels leave for
that table, read literally: cell c is slots [off[c], off[c + 1]) in list order.  Every other scene of the suite takes its tables from a grid
builder: off[0] == 0, no slack, every primitive in exactly the cells its box touches, lists in input order.  The edits below leave that shape.

An edit is a function (a10_pass.Scene, the index of ONE set in stage order: spheres, loose triangles, the meshes) -> Edited: the new Scene
(.key = the base key + the edit's name and the set), and the TARGETS of the edit -- the geometry a wrong reader of that table would treat
differently: the poison for lead / tail / empty, the primitives that left their cells for drop / hollow, the copies for dup / fat, the set
itself for shuffle.  The ray batch of an edited scene is rays_common.make_rays of the BASE scene plus AIMED = 64 rays aimed at the targets,
built as rays_common._aimed builds them.

  lead(k)        k poison slots in front of the arrays, every offset + k: off[0] == k
  tail(k)        k poison slots behind slot off[n^3]; the table unchanged
  drop           every cell with two or more slots loses its last: a table that lies by omission
  shuffle(seed)  the slots permuted inside each cell (ties on t go to the first slot in list order; so does the shadow ray's stored t)
  dup            the first slot of every non-empty cell repeated at the end of its list
  fat(r)         every non-empty cell gets r more slots, copies of primitives of the same set drawn by a seeded generator, whether they touch
                 the cell or not (r = FAT_R = 70: every non-empty cell then holds more than 64 slots, so the shared-test walk's pool fills)
  empty          the table all zero, the arrays poison only: the set is present and holds nothing
  hollow         every cell's list emptied except those of one z-slab (cells z * n^2 .. (z + 1) * n^2 - 1); the arrays stay as they are, so the
                 records of the slabs in front become slack before off[0] and those behind slack after off[n^3] -- REAL geometry as slack.
                 With n == 1 the one slab is the whole table: hollow is the identity there, and says so (Edited.identity).

POISON is ordinary finite geometry with a material id of its own (loose sets: one more material appended to the scene's; a mesh has one id for
all its records), placed where a wrong reader would hit it: across the set's box for a single cell, inside cell 0 for a grid under lead,
inside the last cell under tail -- triangles in both windings in turn (the reference's triangle test sees one side).  lead(k, nonfinite=True)
uses records of NaN and infinities instead: slack must not reach a result (it may cost a deferral, which nobody asserts).

MUTANT tables stand for the wrong readers: the lead scene with off[0] set to 0, the tail scene with off[n^3] set to the array length.
"""
import numpy as np

import a10_pass as A
import random_scenes_common as S
import rays_common as R

AIMED = 64
FAT_R = 70
FAT_CELL_R = 30     # ... and a single cell 30 more: the 60-record set stays within kLdsTriMax = 96 and staged
FLOOR = 32          # rays of the batch an edit (drop, hollow) or a mutant table must change in the oracle
SIZE = (37, 21, 4)


# ---- one set of a scene dict as arrays of slots ---------------------------------------------------------------------------------------------
def set_ids(sc):
    """the sets in stage order: "spheres", "triangles", ("mesh", j)"""
    return (["spheres"] if sc.has_spheres else []) + (["triangles"] if sc.has_triangles else []) + [("mesh", j) for j in range(len(sc.meshes))]


def _get(d, sid):
    """-> dict(kind, n, off uint32 [n^3 + 1], bounds [8], arrs {name: float / uint array [slots, width]}) of one set of the scene dict"""
    if sid == "spheres":
        return dict(kind="spheres", n=int(d["n_slabs"]), off=np.asarray(d["s_box"], np.uint32), bounds=np.asarray(d["sphere_bounds"], np.float32),
                    arrs=dict(prims=np.asarray(d["spheres"], np.float32).reshape(-1, 4), matid=np.asarray(d["s_matid"], np.uint32).reshape(-1, 1)))
    if sid == "triangles":
        return dict(kind="triangles", n=int(d["n_slabs"]), off=np.asarray(d["t_box"], np.uint32), bounds=np.asarray(d["triangle_bounds"], np.float32),
                    arrs=dict(prims=np.asarray(d["t_pos"], np.float32).reshape(-1, 12), normals=np.asarray(d["t_normal"], np.float32).reshape(-1, 12),
                              matid=np.asarray(d["t_matid"], np.uint32).reshape(-1, 1)))
    m = d["meshes"][sid[1]]
    return dict(kind="triangles", n=int(m["nslabs"]), off=np.asarray(m["box"], np.uint32), bounds=np.asarray(m["bounds"], np.float32),
                arrs=dict(prims=np.asarray(m["pos"], np.float32).reshape(-1, 12), normals=np.asarray(m["normal"], np.float32).reshape(-1, 12)))


def _put(d, sid, off, arrs):
    """the scene dict with one set replaced (n_spheres / n_triangles / ntriangles stay > 0: they only say "present")"""
    d = dict(d)
    flat = {k: np.ascontiguousarray(v).ravel() for k, v in arrs.items()}
    off = np.asarray(off, np.uint32)
    if sid == "spheres":
        d.update(spheres=flat["prims"], s_matid=flat["matid"], s_box=off, n_spheres=max(1, len(arrs["prims"])))
    elif sid == "triangles":
        d.update(t_pos=flat["prims"], t_normal=flat["normals"], t_matid=flat["matid"], t_box=off, n_triangles=max(1, len(arrs["prims"])))
    else:
        ms = list(d["meshes"])
        ms[sid[1]] = dict(ms[sid[1]], pos=flat["prims"], normal=flat["normals"], box=off, ntriangles=max(1, len(arrs["prims"])))
        d["meshes"] = ms
    return d


# ---- poison ---------------------------------------------------------------------------------------------------------------------------------
# big triangles through the centre of a box, in the cube [-1, 1]^3: two per diagonal plane (x == y, x == -y, y == z, y == -z)
_POOL = np.array([[(-1, -1, -1), (1, 1, -1), (1, 1, 1)], [(-1, -1, -1), (1, 1, 1), (-1, -1, 1)],
                  [(-1, 1, -1), (1, -1, -1), (1, -1, 1)], [(-1, 1, -1), (1, -1, 1), (-1, 1, 1)],
                  [(-1, -1, -1), (-1, 1, 1), (1, 1, 1)], [(-1, -1, -1), (1, 1, 1), (1, -1, -1)],
                  [(-1, 1, -1), (1, 1, -1), (1, -1, 1)], [(-1, 1, -1), (1, -1, 1), (-1, -1, 1)]], np.float64)
_POOL_ORDER = (0, 4, 2, 6, 1, 5, 3, 7)     # the planes in turn, so that a few records already face every axis


def cell_box(bounds, n, cell):
    """(lo, hi) of cell (x, y, z) = cell of the n^3 grid over bounds8"""
    lo, hi = np.asarray(bounds, np.float64)[0:3], np.asarray(bounds, np.float64)[4:7]
    delta = (hi - lo) / n
    c = np.asarray(cell, np.float64)
    return lo + c * delta, lo + (c + 1) * delta


def poison(kind, k, lo, hi, poison_mat, nonfinite=False):
    """k poison records for a set of `kind` inside the box (lo, hi) -> {name: [k, width]} for prims / normals / matid (a mesh drops matid)"""
    c, h = 0.5 * (lo + hi), 0.5 * (hi - lo)
    out = {}
    if kind == "spheres":
        p = np.zeros((k, 4), np.float32)
        for j in range(k):
            r = (0.45 - 0.03 * (j % 5)) * h.min()
            p[j] = [*(c + 0.1 * h * [(j % 3) - 1, ((j // 3) % 3) - 1, 0]), r * r]
        out["prims"] = p
    else:
        p, nr = np.zeros((k, 3, 4), np.float32), np.zeros((k, 3, 4), np.float32)
        for j in range(k):
            t = c + 0.9 * h * _POOL[_POOL_ORDER[(j // 2) % len(_POOL)]]
            if j % 2:
                t = t[::-1]
            nrm = np.cross(t[1] - t[0], t[2] - t[0])
            p[j, :, :3], nr[j, :, :3] = t, nrm / np.linalg.norm(nrm)
        out["prims"], out["normals"] = p.reshape(k, 12), nr.reshape(k, 12)
    if nonfinite:
        bad = np.array([np.nan, np.inf, -np.inf], np.float32)
        out["prims"] = bad[np.arange(out["prims"].size) % 3].reshape(out["prims"].shape)
        if "normals" in out:
            out["normals"] = np.full_like(out["normals"], np.nan)
    out["matid"] = np.full((k, 1), poison_mat, np.uint32)
    return out


def _prims_of(kind, recs):
    """records [k, 4] / [k, 12] as rays_common.set_list holds primitives"""
    recs = np.asarray(recs, np.float64)
    return recs.reshape(-1, 4) if kind == "spheres" else recs.reshape(-1, 3, 4)[:, :, :3]


# ---- the edits ------------------------------------------------------------------------------------------------------------------------------
class Edited:
    """scene: the edited a10_pass.Scene; base; name; sid; targets: (kind, primitives, bounds8) as rays_common.set_list's entries, or None;
    sides: which side of a target triangle the aimed rays start on (0: both in turn -- the poison has both windings; -1: the side the
    reference's test sees); identity: the edit changed nothing (hollow on a single cell)"""

    def __init__(self, base, name, sid, d, targets, sides=0, identity=False):
        self.base, self.name, self.sid, self.sides, self.identity = base, name, sid, sides, identity
        self.scene = A.Scene(d)
        self.scene.key = tuple(base.key) + (name, str(sid))
        self.targets = targets
        self._rays = None

    def set(self):
        return _get(self.scene.d, self.sid)

    def rays(self):
        """float32 [N_RAYS + AIMED, 8]: the base scene's batch, then the aimed rays; read-only"""
        if self._rays is None:
            base = base_rays(self.base)
            r = np.concatenate([base, aimed_rays(self)]) if self.targets is not None else base
            r.setflags(write=False)
            self._rays = r
        return self._rays


def _with_poison_mat(d):
    """the scene dict with one more material, the poison's own (magenta): -> (dict, its id)"""
    mats = list(np.asarray(d["materials"], np.float32).ravel())
    return dict(d, materials=mats + [1.0, 0.0, 1.0, 0.0]), len(mats) // 4


def _gather(s, src, pz):
    """the set's arrays re-made from a slot list: src >= 0 names an old slot, src == -(j + 1) poison record j"""
    src = np.asarray(src, np.int64)
    out = {}
    for name, a in s["arrs"].items():
        new = np.zeros((len(src), a.shape[1]), a.dtype)
        new[src >= 0] = a[src[src >= 0]]
        if (src < 0).any():
            new[src < 0] = pz[name][-src[src < 0] - 1]
        out[name] = new
    return out


def _cells(off):
    return [np.arange(int(off[c]), int(off[c + 1])) for c in range(len(off) - 1)]


def _from_cells(cells):
    off = np.zeros(len(cells) + 1, np.uint32)
    off[1:] = np.cumsum([len(c) for c in cells])
    return off, (np.concatenate(cells) if cells else np.zeros(0, np.int64)).astype(np.int64)


def lead(k, nonfinite=False):
    def edit(base, sid):
        d, pm = _with_poison_mat(base.d)
        s = _get(d, sid)
        lo, hi = cell_box(s["bounds"], s["n"], (0, 0, 0))
        pz = poison(s["kind"], k, lo, hi, pm, nonfinite)
        n = int(s["off"][-1])
        arrs = _gather(s, list(range(-1, -k - 1, -1)) + list(range(n)), pz)
        fin = poison(s["kind"], k, lo, hi, pm)      # the aimed rays go where finite poison would sit, whatever the records hold
        return Edited(base, f"lead({k}{',nonfinite' if nonfinite else ''})", sid, _put(d, sid, s["off"] + np.uint32(k), arrs),
                      (s["kind"], _prims_of(s["kind"], fin["prims"]), s["bounds"]))
    return edit


def tail(k):
    def edit(base, sid):
        d, pm = _with_poison_mat(base.d)
        s = _get(d, sid)
        lo, hi = cell_box(s["bounds"], s["n"], (s["n"] - 1,) * 3)
        pz = poison(s["kind"], k, lo, hi, pm)
        n = int(s["off"][-1])
        arrs = _gather(s, list(range(n)) + list(range(-1, -k - 1, -1)), pz)
        return Edited(base, f"tail({k})", sid, _put(d, sid, s["off"], arrs), (s["kind"], _prims_of(s["kind"], pz["prims"]), s["bounds"]))
    return edit


def _recut(base, sid, name, cells_of, targets_of, sides=-1):
    s = _get(base.d, sid)
    old = _cells(s["off"])
    new = cells_of(s, old)
    off, src = _from_cells(new)
    t = targets_of(s, old, new)
    targets = None if t is None or len(t) == 0 else (s["kind"], _prims_of(s["kind"], s["arrs"]["prims"][np.asarray(t, np.int64)]), s["bounds"])
    return Edited(base, name, sid, _put(base.d, sid, off, _gather(s, src, None)), targets, sides)


def drop(base, sid):
    return _recut(base, sid, "drop", lambda s, old: [c[:-1] if len(c) >= 2 else c for c in old],
                  lambda s, old, new: np.unique([c[-1] for c in old if len(c) >= 2]))


def shuffle(seed):
    def edit(base, sid):
        rng = np.random.default_rng(seed)
        return _recut(base, sid, f"shuffle({seed})", lambda s, old: [rng.permutation(c) for c in old],
                      lambda s, old, new: np.arange(int(s["off"][-1])))
    return edit


def dup(base, sid):
    return _recut(base, sid, "dup", lambda s, old: [np.concatenate([c, c[:1]]) for c in old],
                  lambda s, old, new: np.unique([c[0] for c in old if len(c)]))


def fat(r=FAT_R, seed=7):
    def edit(base, sid):
        rng = np.random.default_rng(seed)
        rr = r if _get(base.d, sid)["n"] > 1 else min(r, FAT_CELL_R)
        return _recut(base, sid, f"fat({rr})",
                      lambda s, old: [np.concatenate([c, rng.integers(0, int(s["off"][-1]), size=rr)]) if len(c) else c for c in old],
                      lambda s, old, new: np.arange(int(s["off"][-1])))
    return edit


def empty(base, sid, k=4):
    d, pm = _with_poison_mat(base.d)
    s = _get(d, sid)
    lo, hi = np.asarray(s["bounds"], np.float64)[0:3], np.asarray(s["bounds"], np.float64)[4:7]
    pz = poison(s["kind"], k, lo, hi, pm)
    arrs = _gather(s, list(range(-1, -k - 1, -1)), pz)
    return Edited(base, "empty", sid, _put(d, sid, np.zeros_like(s["off"]), arrs), (s["kind"], _prims_of(s["kind"], pz["prims"]), s["bounds"]))


def hollow_slab(s):
    """the z-slab hollow keeps: the one of 1 .. n - 1 that holds the most slots (so that off[0] != 0), 0 for a single cell"""
    n, off = s["n"], s["off"].astype(np.int64)
    if n == 1:
        return 0
    return 1 + int(np.argmax([off[(z + 1) * n * n] - off[z * n * n] for z in range(1, n)]))


def hollow(base, sid):
    s = _get(base.d, sid)
    n, off = s["n"], s["off"].astype(np.int64)
    z = hollow_slab(s)
    first, last = z * n * n, (z + 1) * n * n
    new = np.clip(off, off[first], off[last]).astype(np.uint32)     # the cells in front are empty at off[first], those behind at off[last]
    gone = np.concatenate([np.arange(0, off[first]), np.arange(off[last], off[-1])])
    targets = None if gone.size == 0 else (s["kind"], _prims_of(s["kind"], s["arrs"]["prims"][gone]), s["bounds"])
    return Edited(base, "hollow", sid, _put(base.d, sid, new, s["arrs"]), targets, -1, identity=(n == 1))


def without_set(base, sid):
    """the scene without that set: what `empty` must equal"""
    d = dict(base.d)
    if sid == "spheres":
        d["n_spheres"] = 0
    elif sid == "triangles":
        d["n_triangles"] = 0
    else:
        d["meshes"] = [m for j, m in enumerate(d["meshes"]) if j != sid[1]]
    sc = A.Scene(d)
    sc.key = tuple(base.key) + ("without", str(sid))
    return sc


def mutant(ed):
    """the wrong reader of a lead / tail scene as a table: off[0] = 0, or off[n^3] = the array length"""
    s = ed.set()
    off = s["off"].copy()
    if ed.name.startswith("lead"):
        off[0] = 0
    else:
        off[-1] = len(s["arrs"]["prims"])
    sc = A.Scene(_put(ed.scene.d, ed.sid, off, s["arrs"]))
    sc.key = tuple(ed.scene.key) + ("mutant",)
    return sc


# ---- rays -----------------------------------------------------------------------------------------------------------------------------------
_BASE_RAYS, _EXPECTED = {}, {}


def base_rays(sc):
    if sc.key not in _BASE_RAYS:
        _BASE_RAYS[sc.key] = R.make_rays(sc)[0]
    return _BASE_RAYS[sc.key]


def aimed_rays(ed, seed=77):
    """AIMED rays towards points of the targets from about 0.05 away, as rays_common._aimed makes them (sides 0); sides -1: every ray starts
    on the side the reference's one-sided triangle test sees: that of cross(p1 - p0, p2 - p0), as random_scenes_common.room_tris winds its walls"""
    rng = np.random.default_rng(seed)
    if ed.sides == 0 or ed.targets[0] == "spheres":
        o, d, _ = R._aimed(rng, [ed.targets], AIMED)
    else:
        o, d = np.zeros((AIMED, 3)), np.zeros((AIMED, 3))
        for k in range(AIMED):     # _aimed starts its first ray of a set on the +normal side
            oo, dd, _ = R._aimed(rng, [ed.targets], 1)
            o[k], d[k] = oo[0], dd[0]
    r = np.zeros((AIMED, 8), np.float32)
    r[:, 0:3], r[:, 4:7], r[:, 7] = o, d, np.inf
    return r


def expected(sc, rays, batch=None):
    """(hits, sets, occluded) of the oracle for `rays` in `sc`, cached by the scene's key and the batch's name (None: the scene's own batch)"""
    key = (sc.key, batch)
    if key not in _EXPECTED:
        h, s = R.expected_closest(sc, rays)
        o = R.expected_occluded(sc, rays)
        for a in (h, s, o):
            a.setflags(write=False)
        _EXPECTED[key] = (h, s, o)
    return _EXPECTED[key]


def expected_shadow(sc, rays):
    """(mint, maxt) float32 [n] of the rays after the shadow kernels of a10_pass.run_pass's direct(): the any-hit loop stores the t of the
    FIRST slot in list order that blocks the ray, so a shuffle moves it where the flag stays"""
    k = A.load_oracle()
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    n = len(rays)
    rb, g1 = R._ray_buffer(rays)
    B = k.buf
    if sc.has_spheres:
        k.sphereShadowTrace(n, B(rb), B(sc.spheres), B(sc.s_box), A._f(sc.sphere_bounds)[0], sc.n_slabs, g1)
    if sc.has_triangles:
        k.triangleShadowTrace(n, B(rb), B(sc.t_pos), B(sc.t_box), A._f(sc.triangle_bounds)[0], sc.n_slabs, g1)
    for m in sc.meshes:
        k.triangleShadowTrace(n, B(rb), B(m["pos"]), B(m["box"]), A._f(m["bounds"])[0], m["nslabs"], g1)
    k.flush()
    return rb["mint"][:n].copy(), rb["maxt"][:n].copy()


def changed(a, b):
    """per ray: the closest record, the winning set or the occlusion flag differs (bit for bit, every NaN equal to every NaN)"""
    from conftest import bits
    (h0, s0, o0), (h1, s1, o1) = a, b
    return (bits(h0.copy()) != bits(h1.copy())).any(axis=1) | (s0 != s1) | (o0 != o1)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
# the table SHAPES: (name, stratum, seed, set).  single_cell 3000: loose 60 triangles (staged), meshes of 40 (60 + 40 > 96: not staged) and 7
# (staged behind the 60).  single_cell 3001: loose 97 (can never be staged), meshes 96 (staged), 95.
SHAPES = (
    ("staged_cell", "single_cell", 3000, "triangles"),
    ("unstaged_cell", "single_cell", 3001, "triangles"),
    ("spheres", "staged", 3003, "spheres"),
    ("staged_grid", "staged", 3003, ("mesh", 0)),
    ("memory_grid", "unstaged", 3006, ("mesh", 0)),
    ("many_sets_mesh", "many_sets", 3010, ("mesh", 3)),
)
EDITS = (("lead", lead(5)), ("tail", tail(5)), ("drop", drop), ("shuffle", shuffle(11)), ("dup", dup), ("fat", fat()), ("empty", empty),
         ("hollow", hollow))
# the edges of lead on staged single-cell sets (nslots counts the slack), 60 / 40 / 7: 36 + 60 == 96 stays staged; 37 + 60 == 97 leaves LDS and
# the 40 and the 7 behind it enter.  97 / 96 / 95: tail must leave the 96-record mesh staged.  One nonfinite lead per scene.
EXTRA = (
    ("lead96", "single_cell", 3000, "triangles", lead(36)),
    ("lead97", "single_cell", 3000, "triangles", lead(37)),
    ("lead_mesh7", "single_cell", 3000, ("mesh", 1), lead(29)),        # 60 + 29 + 7 == 96
    ("tail_mesh96", "single_cell", 3001, ("mesh", 0), tail(5)),
    ("lead_mesh96", "single_cell", 3001, ("mesh", 0), lead(1)),        # 97 slots: leaves LDS, the 95 enters
    ("shuffle_mesh96", "single_cell", 3001, ("mesh", 0), shuffle(12)),
    ("drop_mesh40", "single_cell", 3000, ("mesh", 0), drop),           # unstaged before (60 + 40 > 96) and after (60 + 39)
    ("nonfinite_cell", "single_cell", 3000, "triangles", lead(5, True)),
    ("nonfinite_grid", "staged", 3003, ("mesh", 0), lead(5, True)),
    ("nonfinite_memory", "unstaged", 3006, ("mesh", 0), lead(5, True)),
    ("nonfinite_many", "many_sets", 3010, ("mesh", 3), lead(5, True)),
    ("nonfinite_spheres", "staged", 3003, "spheres", lead(5, True)),
)

_CASES = {}


def base_scene(stratum, seed):
    return S.scene(stratum, seed, *SIZE)


def case_ids():
    return [f"{shape}-{ename}" for shape, *_ in SHAPES for ename, _ in EDITS] + [name for name, *_ in EXTRA]


def case(cid):
    """-> Edited, made once"""
    if cid not in _CASES:
        table = {f"{shape}-{ename}": (stratum, seed, sid, fn) for shape, stratum, seed, sid in SHAPES for ename, fn in EDITS}
        table.update({name: (stratum, seed, sid, fn) for name, stratum, seed, sid, fn in EXTRA})
        stratum, seed, sid, fn = table[cid]
        _CASES[cid] = fn(base_scene(stratum, seed), sid)
    return _CASES[cid]


def shape_of(sc, sid):
    """what the table of set `sid` of `sc` IS, from the kernel the scene forces (random_scenes_common.kernel_choice) -> (shape name, choice)"""
    ch = S.kernel_choice(sc)
    i = set_ids(sc).index(sid)
    is_tri, n, slots = S.sets_of(sc)[i]
    if not is_tri:
        return "spheres", ch
    if n == 1:
        return ("staged_cell" if ch["tri_staged"][i] else "unstaged_cell"), ch
    if len(sc.meshes) == S.K_MAX_MESHES:
        return "many_sets_mesh", ch
    return ("staged_grid" if ch["GRIDS"] == 1 else "memory_grid"), ch


# ---- Assign07 frame jobs: the same edits on s_slab_size / t_slab_size and their arrays --------------------------------------------------------
FRAME_SIZE = (37, 21)
FRAME_JOBS = ("frame_a07_mol_c60_n4_160x120", "frame_a07_teapot_n8_160x120")     # one molecule job, one mesh job (tests/frame_cameras_common.py)
FRAME_EDITS = ("lead", "drop", "hollow")
FRAME_FLOOR = 8     # pixels of the 777 an edit (drop, hollow) or the lead mutant must change in the A07 oracle


def frame_camera(job, name):
    """The page's orbit leaves these objects a dozen pixels wide at 37 x 21, so the cameras come closer (Camera.set's basis: every d.z < 0).
    lead: the eye two cells behind the centre of cell 0, looking through it -- where a reader that starts the first cell at slot 0 meets the
    poison; drop, hollow: the eye at 0.45 of the box's diagonal from the centre, the object filling the frame"""
    import frame_cameras_common as K
    if name == "lead":
        lo, hi = cell_box(job["bounds"], int(job["n_slabs"]), (0, 0, 0))
        return K.block(job, [0.5 * (lo[0] + hi[0]), 0.5 * (lo[1] + hi[1]), lo[2] + 2.0 * (hi[2] - lo[2])])
    c, diag = K.centre_diag(job)
    return K.block(job, [c[0], c[1], c[2] + 0.45 * diag])


def _frame_get(d):
    """the one set of an Assign07 job (molecule: atoms + mindex; mesh: pos + normal + mindex) as _get gives a scene's"""
    n, off, bounds = int(d["n_slabs"]), np.asarray(d["slab_size"], np.uint32), np.asarray(d["bounds"], np.float32)
    if "atoms" in d:
        return dict(kind="spheres", n=n, off=off, bounds=bounds,
                    arrs=dict(prims=np.asarray(d["atoms"], np.float32).reshape(-1, 4), matid=np.asarray(d["mindex"], np.uint32).reshape(-1, 1)))
    return dict(kind="triangles", n=n, off=off, bounds=bounds,
                arrs=dict(prims=np.asarray(d["pos"], np.float32).reshape(-1, 12), normals=np.asarray(d["normal"], np.float32).reshape(-1, 12),
                          matid=np.asarray(d["mindex"], np.uint32).reshape(-1, 1)))


def _frame_put(d, off, arrs):
    flat = {k: np.ascontiguousarray(v).ravel() for k, v in arrs.items()}
    if "atoms" in d:
        return dict(d, slab_size=np.asarray(off, np.uint32), atoms=flat["prims"], mindex=flat["matid"])
    return dict(d, slab_size=np.asarray(off, np.uint32), pos=flat["prims"], normal=flat["normals"], mindex=flat["matid"])


def frame_edit(d, name, k=5):
    """-> (the edited job, the mutant job or None): lead puts k poison records inside cell 0 (an atom's float4 is (centre, radius): the poison
    takes cell-sized radii), drop and hollow as for a scene's sets.  The mutant of lead reads the first cell from slot 0."""
    s = _frame_get(d)
    if name == "lead":
        lo, hi = cell_box(s["bounds"], s["n"], (0, 0, 0))
        pz = poison(s["kind"], k, lo, hi, 0)
        if s["kind"] == "spheres":
            pz["prims"][:, 3] = np.sqrt(pz["prims"][:, 3])
        arrs = _gather(s, list(range(-1, -k - 1, -1)) + list(range(int(s["off"][-1]))), pz)
        off = s["off"] + np.uint32(k)
        wrong = off.copy()
        wrong[0] = 0
        return _frame_put(d, off, arrs), _frame_put(d, wrong, arrs)
    if name == "drop":
        off, src = _from_cells([c[:-1] if len(c) >= 2 else c for c in _cells(s["off"])])
        return _frame_put(d, off, _gather(s, src, None)), None
    if name == "hollow":
        n, o = s["n"], s["off"].astype(np.int64)
        z = hollow_slab(s)
        return _frame_put(d, np.clip(o, o[z * n * n], o[(z + 1) * n * n]).astype(np.uint32), s["arrs"]), None
    raise KeyError(name)


_FRAMES = {}


def frame_case(job, name):
    """-> dict(base=(job dict, oracle pixels, oracle rays), edited=..., mutant=... or None), the A07 oracle of tests/frame_cameras_common.py's
    jobs (oracle/frame_pass.py) run once"""
    import frame_cameras_common as K
    import frame_pass as F
    key = (job, name)
    if key not in _FRAMES:
        def run(d):
            px, rays = F.run_frame("oracle", F.Frame(d))
            px.flags.writeable = False
            rays.flags.writeable = False
            return d, px, rays
        base = K.resized(K.job_named(job), *FRAME_SIZE)
        base = dict(base, cam=frame_camera(base, name))
        ed, wrong = frame_edit(base, name)
        _FRAMES[key] = dict(base=run(base), edited=run(ed), mutant=None if wrong is None else run(wrong))
    return _FRAMES[key]
