"""Random and adversarial atom sets through every Assign07 frame path: the kernel-by-kernel initTrace + molTrace (k_a07_molTrace), the one-launch
frame with and without a ray buffer (k_frame_fused, the MOL instantiation of frame_stage_grid), the both-models frame (molecule, then mesh, on one
ray) and, for generated meshes, the one-launch frame's FS_A04 / FS_MESH modes.  Every comparison is bit for bit -- every pixel, every ray's mint and
maxt -- against the CPU oracle (oracle/frame_pass.py run_frame / run_frame_both on liboracle.so).  Kernel and oracle consume the same packed arrays:
these tests are about the walk, not about the binning.

The packing (pack_atoms) is test_grid_build.expected_grid(0, ...) + {c, r*r} with r*r formed in fp64 and narrowed, as k_gatherSpheres does.  The
reference's splitMolData (A07 code.js:889-978) differs from splitSphereData in no quirk: fed the molecule reader's own record that the fixtures carry
(`pdb`: atoms in file order, radii per element, bounds in doubles), pack_atoms rebuilds every molecule fixture exactly
(test_packing_reproduces_the_reference_hosts_molecule_grids).  The atom list cannot be recovered from the slot array alone: cells are emitted z-major,
so the order of first occurrences in slot order is not the input order, and the order inside a cell is the input order.

Notes on what the atom walk can and cannot show (pt_kernels_frame.hip against A07 code.cl:110-150, 337-473):
  * the sphere test of Assign07 is Assign10's: roots (-b -+ sqrt(dis)) * (1 / (2a)) and the CLOSED window [cmin, cmax];
  * a tie on t between two atoms of one cell goes to the first in list order (strict <).  Exact copies tie on every ray but give the same colour and
    the same maxt, so the `coincident` kind also carries a constructed pair (tied_pair): two different spheres that the central ray of an odd-sized
    image meets at bit-identical t with different normals -- the one pixel where the order shows;
  * once a cell has produced a champion no later cell can replace it -- a later cell's window starts where this one's ends, so its t is never below
    the champion's -- hence walking on after a hit changes the time a frame takes and nothing else.
"""
import os

import numpy as np
import pytest

import a10_pass as A
import frame_pass as F
from conftest import ROOT, bits
from test_frame_one_launch import rays40
from test_frames import _random_mesh_job, fixture, resized
from test_grid_build import expected_grid

BASE = "frame_a07_own_mol_lattice_n6_96x64"      # a small molecule fixture: its camera looks down -z at the middle of its box
KINDS = ("soup", "coincident", "lattice", "poking", "degenerate")
NS = (1, 2, 5, 16)
SEEDS = (0, 1)
SIZES = ((160, 100), (67, 45))                    # the second: no multiple of 8 or 32 either way, odd both ways (the central ray is the view axis)
RADII = (0.003, 0.02, 0.15, 0.6)                  # of the box's shortest edge
DEGENERATE = ("empty", "single", "flat", "crowded")
BOTH_SEEDS = (8, 9, 14, 7)                        # n = 2 | 5 by seed % 2, soup | poking by seed // 2 % 2; chosen on the CPU: both models show in the oracle's frame
BOTH_SIZE = (200, 120)
MOL_KEYS = ("s_size", "atoms", "mindex", "mcolor", "slab_size")
REF_A07 = os.path.join(ROOT, "oracle", "_ref", "libref_a07.so")


# ---- packing ------------------------------------------------------------------------------------------------------------------------------------
def pack_atoms(sph, mindex, bounds6, n):
    """splitMolData: atoms {c, r} in doubles -> (slab_size [n^3 + 1], slots {c, r*r} float32 [total, 4], the slots' mindex)"""
    sph = np.asarray(sph, np.float64).reshape(-1, 4)
    off, order = expected_grid(0, sph, bounds6, n)
    order = order.astype(np.int64)
    slots = np.concatenate([sph[order, :3], (sph[order, 3] * sph[order, 3])[:, None]], axis=1).astype(np.float32)
    return off, slots, np.asarray(mindex, np.uint32)[order]


def box_of(job):
    b = np.asarray(job["bounds"], np.float32).astype(np.float64)
    return b[:3], b[4:7]


def mol_job(base, sph, mindex, n):
    """the Assign07 molecule job of atoms {c, r} in base's box, under base's camera and material table"""
    sph = np.asarray(sph, np.float64).reshape(-1, 4).astype(np.float32).astype(np.float64)   # what is binned is what is traced
    lo, hi = box_of(base)
    off, slots, mi = pack_atoms(sph, mindex, [*lo, *hi], n)
    job = {k: v for k, v in base.items() if k not in ("mol", "pdb", "mesh", "pos", "normal", "t_size")}
    job.update(n_slabs=int(n), s_size=len(sph), atoms=slots.ravel(), mindex=mi, slab_size=off)
    return job


# ---- the kinds ----------------------------------------------------------------------------------------------------------------------------------
def _soup(rng, lo, hi, count, weights=(0.3, 0.3, 0.25, 0.15)):
    c = lo + rng.uniform(0.0, 1.0, (count, 3)) * (hi - lo)
    r = float(np.min(hi - lo)) * rng.choice(RADII, size=count, p=weights)
    return np.concatenate([c, r[:, None]], axis=1)


def tied_pair(base):
    """Two spheres A, B and the t at which the ray from the eye along -W = (0, 0, -1) meets both, bit for bit: A on the axis, radius s; B 1.5 s off
    the axis, radius 2.5 s, its centre s below A's (a 3-4-5 triangle through the hit point).  s is a power of two and every operand of both
    quadratics a small multiple of it, so every operation is exact in fp32 in whatever order it is done: with o - c = (0, 0, K + s) | (1.5 s, 0, K + 2 s)
    and d = (0, 0, -1), sqrt(dis) = 2 s | 4 s and t0 = K for both.  Normals at the hit: A's is W (shade 1), B's has W-component 0.8.
    test_the_tied_pair_ties checks all of this on the oracle."""
    cam = np.asarray(base["cam"], np.float32)
    assert cam[3:12].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1], "needs an axis-aligned camera"
    eye = cam[:3].astype(np.float64)
    lo, hi = box_of(base)
    assert lo[0] < eye[0] < hi[0] and lo[1] < eye[1] < hi[1] and eye[2] > hi[2]
    s = 2.0 ** np.floor(np.log2(np.min(hi - lo) / 16))
    K = s * (np.floor((eye[2] - hi[2]) / s) + 2)            # the hit lies between s and 2 s under the near face
    zh = eye[2] - K
    a = [eye[0], eye[1], zh - s, s]
    b = [eye[0] - 1.5 * s, eye[1], zh - 2 * s, 2.5 * s]
    pair = np.asarray([a, b])
    assert np.array_equal(pair.astype(np.float32).astype(np.float64), pair), "the centres are not fp32 numbers"
    return pair, float(K), s


def _coincident(rng, base, lo, hi, count):
    pair, K, s = tied_pair(base)
    eye = np.asarray(base["cam"], np.float64)[:3]
    edge = float(np.min(hi - lo))
    sph = _soup(rng, lo, hi, count, (0.3, 0.3, 0.4, 0.0))
    k = np.arange(7, count, 7)                               # exact copies of their predecessors (another mindex)
    k2 = np.arange(3, count, 7)                              # the predecessor's centre, another radius
    sph[k[::2] - 1, 3] = RADII[2] * edge                     # every other original is large enough to be seen at the small size
    # nothing (nor the 1.5 x copy, below) may reach the pair or the central ray's way to it: such an atom is drawn again
    for j in range(count):
        for _ in range(200):
            reach = 1.5 * sph[j, 3] + 5 * s
            if not (np.hypot(sph[j, 0] - eye[0], sph[j, 1] - eye[1]) < reach and sph[j, 2] + reach > eye[2] - K):
                break
            sph[j, :3] = lo + rng.uniform(0.0, 1.0, 3) * (hi - lo)
        else:
            raise AssertionError("no place for an atom beside the tied pair")
    sph[k] = sph[k - 1]
    sph[k2, :3] = sph[k2 - 1, :3]
    sph[k2, 3] = sph[k2 - 1, 3] * np.where(k2 % 2, 1.5, 0.5)
    dup = np.zeros(count + 2, bool)
    dup[k] = dup[k - 1] = True
    return np.concatenate([sph, pair]), dup


def _lattice(rng, lo, hi, n, count=48):
    w = (hi - lo) / n
    nint = rng.integers(1, 4, count)                         # 1: the middle of a cell face, 2: of a cell edge, 3: a cell corner
    axes = rng.permuted(np.tile(np.arange(3), (count, 1)), axis=1)
    on = np.zeros((count, 3), bool)
    for j in range(count):
        on[j, axes[j, :nint[j]]] = True
    k = np.where(on, rng.integers(0, n + 1, (count, 3)), rng.integers(0, n, (count, 3)) + 0.5)
    r = float(np.min(w)) * rng.choice([0.5, 1.0, 1e-3], size=count)
    return np.concatenate([lo + k * w, r[:, None]], axis=1)


def _poking(rng, base, lo, hi, n):
    edge = hi - lo
    out = []
    for a in range(3):                                       # through each of the six faces, the centre inside
        for side in (0, 1):
            r = float(np.min(edge)) * float(rng.choice([0.08, 0.2]))
            c = lo + rng.uniform(0.2, 0.8, 3) * edge
            c[a] = (hi[a] - 0.4 * r) if side else (lo[a] + 0.4 * r)
            out.append([*c, r])
    eye = np.asarray(base["cam"], np.float64)[:3]
    outside = np.maximum(eye - hi, lo - eye) / edge          # the face the camera looks at: the axis along which the eye is farthest outside
    a = int(np.argmax(outside))
    near = eye[a] > hi[a]
    c = (lo + hi) / 2
    c[a] = (hi[a] - 0.05 * edge[a]) if near else (lo[a] + 0.05 * edge[a])
    others = [i for i in range(3) if i != a]
    r = 1.1 * float(np.sqrt((edge[others[0]] / 2) ** 2 + (edge[others[1]] / 2) ** 2 + (0.05 * edge[a]) ** 2))
    assert 0.05 * edge[a] + r < edge[a], "the enclosing atom has to end inside the box"
    out.append([*c, r])                                      # encloses the whole near face: every ray enters the box inside it and leaves it inside the box
    r = 0.05 * float(np.min(edge))
    c = (lo + hi) / 2
    c[0] = hi[0] + 1.01 * r                                  # touches the max face from outside: lo index == n, hi index clamped to n - 1 -> in no cell
    out.append([*c, r])
    dropped = np.asarray(out[-1], np.float64).astype(np.float32).astype(np.float64)
    assert np.floor((dropped[0] - dropped[3] - lo[0]) / (edge[0] / n)) == n
    return np.concatenate([np.asarray(out), _soup(rng, lo, hi, 12, (0.2, 0.5, 0.3, 0.0))])


def degenerate_variant(n, seed):
    return DEGENERATE[((NS.index(n) if n in NS else n) + 2 * seed) % 4]


def _degenerate(rng, lo, hi, n, variant):
    edge = float(np.min(hi - lo))
    if variant == "empty":
        return np.zeros((0, 4))
    if variant == "single":
        return np.asarray([[*(lo + rng.uniform(0.3, 0.7, 3) * (hi - lo)), 0.1 * edge]])
    if variant == "flat":                                    # r = 0, one r whose square is a denormal float, and a few ordinary atoms to be seen
        sph = _soup(rng, lo, hi, 20, (0.0, 0.0, 1.0, 0.0))
        sph[:12, 3] = 0.0
        sph[12, 3] = 1e-20
        return sph
    w = (hi - lo) / n                                        # crowded: 300 atoms wholly inside the middle cell, every other cell empty
    cell = np.asarray([n // 2] * 3)
    c = lo + (cell + rng.uniform(0.2, 0.8, (300, 3))) * w
    return np.concatenate([c, np.full((300, 1), 0.1 * float(np.min(w)))], axis=1)


def random_mol_job(base, seed, n, kind, info=None):
    """An Assign07 molecule job, in the packed format oracle/frame_pass.Frame and render.FramePacked both accept, of generated atoms in base's box under
    base's camera.  info: a dict that receives what the guards need ("dup": which atoms are exact copies or their originals; "variant")."""
    rng = np.random.default_rng([seed, n, KINDS.index(kind)])
    lo, hi = box_of(base)
    count = (5, 60, 400)[(seed + n) % 3]
    info = {} if info is None else info
    if kind == "soup":
        sph = _soup(rng, lo, hi, count)
    elif kind == "coincident":
        sph, info["dup"] = _coincident(rng, base, lo, hi, max(count, 30))   # 5 atoms have no seventh
    elif kind == "lattice":
        sph = _lattice(rng, lo, hi, n)
    elif kind == "poking":
        sph = _poking(rng, base, lo, hi, n)
    else:
        info["variant"] = degenerate_variant(n, seed)
        sph = _degenerate(rng, lo, hi, n, info["variant"])
    ncol = len(base["mcolor"]) // 4
    job = mol_job(base, sph, (np.arange(len(sph)) * 7 + seed) % ncol, n)
    info["sph"] = np.asarray(sph, np.float64).reshape(-1, 4).astype(np.float32).astype(np.float64)
    off = job["slab_size"]
    if kind == "degenerate":
        counts = np.diff(off.astype(np.int64))
        if info["variant"] == "empty":
            assert not off.any() and job["s_size"] == 0
        elif info["variant"] == "crowded":
            assert counts.max() == 300 and np.count_nonzero(counts) == 1
        elif info["variant"] == "flat":
            rr = job["atoms"].reshape(-1, 4)[:, 3]
            assert (rr == 0).any() and ((rr > 0) & (rr < np.float32(1.1754944e-38))).any()
    if kind == "poking":
        assert int(off[-1]) and not (job["atoms"].reshape(-1, 4)[:, 0] > hi[0]).any(), "the atom on the max face is in no cell"
    return job


# ---- guards (on the oracle's frame; not the check itself) -----------------------------------------------------------------------------------------
def lit(px):
    return px[:, :3].max(axis=1) > 0


def hits_on(rays, sph):
    """pixels whose ray ends on the surface of one of the spheres {c, r} (fp64, 1e-4 of r): whose colour comes from one of them"""
    o, d, t = rays["o"].astype(np.float64)[:, :3], rays["d"].astype(np.float64)[:, :3], rays["maxt"].astype(np.float64)
    ok = np.isfinite(t)
    p = o[ok] + t[ok, None] * d[ok]
    near = np.zeros(len(p), bool)
    for c in sph:
        if c[3] > 0:
            near |= np.abs(np.linalg.norm(p - c[:3], axis=1) - c[3]) < 1e-4 * c[3]
    out = np.zeros(len(t), bool)
    out[ok] = near
    return out


def guard(kind, info, size, px, rays, base):
    if not (kind == "degenerate" and info["variant"] == "empty"):
        assert lit(px).any(), "nothing to see"
    else:
        assert not lit(px).any()
    if kind == "coincident":
        assert (hits_on(rays, info["sph"][info["dup"]]) & lit(px)).any(), "no pixel shows a duplicated atom"
        if size[0] % 2 and size[1] % 2:                      # the tied pair on the central ray: the first in list order (shade 1) wins
            mid = (size[1] // 2) * size[0] + size[0] // 2
            assert rays["maxt"][mid] == np.float32(tied_pair(base)[1]) and set(px[mid, :3].tolist()) <= {127, 254}


# ---- CPU: the packing convention, the constructed tie, the seeds of the both-models test --------------------------------------------------------------
@pytest.mark.parametrize("name", ["frame_a07_mol_benzene_n2_96x64", "frame_a07_mol_c60_n4_160x120", "frame_a07_own_mol_lattice_n6_96x64"])
def test_packing_reproduces_the_reference_hosts_molecule_grids(name):
    """pack_atoms, fed the molecule reader's record the fixture carries (atoms in file order, radius per element, bounds in doubles), rebuilds what
    the reference's splitMolData produced: slab_size, the slots {c, r*r} (z-major cells, input order inside a cell) and their mindex, exactly."""
    _, d = fixture(name)
    pdb = d["pdb"]
    rec = np.asarray(pdb["atomData"], np.float64).reshape(-1, 4)             # {element, x, y, z}
    ids = rec[:, 0].astype(int)
    sph = np.concatenate([rec[:, 1:], np.asarray(pdb["radiusData"], np.float64)[ids][:, None]], axis=1)
    off, slots, mi = pack_atoms(sph, ids, list(pdb["min"]) + list(pdb["max"]), d["n_slabs"])
    want = np.asarray(d["atoms"], np.float32).reshape(-1, 4)
    assert np.array_equal(off, np.asarray(d["slab_size"], np.uint32))
    assert np.array_equal(slots.view(np.uint32), want.view(np.uint32)) and np.array_equal(mi, np.asarray(d["mindex"], np.uint32))
    # the slots alone give the atoms back as a set (first occurrence of each distinct slot), r through the fp64 square root of the fp32 r*r ...
    key = np.concatenate([want.view(np.uint32), np.asarray(d["mindex"], np.uint32)[:, None]], axis=1)
    _, first = np.unique(key, axis=0, return_index=True)
    r = np.sqrt(want[first, 3].astype(np.float64))
    assert np.array_equal((r * r).astype(np.float32).view(np.uint32), want[first, 3].view(np.uint32)), "r*r does not survive sqrt and squaring in fp64"
    mine = np.concatenate([sph[:, :3], (sph[:, 3] ** 2)[:, None]], axis=1).astype(np.float32)
    assert {tuple(x) for x in want[first].view(np.uint32).tolist()} == {tuple(x) for x in mine.view(np.uint32).tolist()}
    # ... but not their order: the first occurrences in slot order are not in input order wherever a later atom reaches an earlier cell
    assert len(first) == len(sph)


@pytest.fixture(scope="module")
def base():
    return fixture(BASE)[1]


def test_the_tied_pair_ties(base):
    """CPU, the oracle alone: the central ray of a 67x45 frame meets both spheres of tied_pair at the same t; whichever is first in the list wins, and the
    two give different colours -- the pixel that tells `<` from `<=` in the champion update."""
    pair, K, _ = tied_pair(base)
    mid = (45 // 2) * 67 + 67 // 2
    seen = []
    for order in ([0, 1], [1, 0]):
        d = resized(mol_job(base, pair[order], [0, 1], 2), 67, 45)
        px, rays = F.run_frame("oracle", F.Frame(d))
        assert rays["maxt"][mid] == np.float32(K)
        seen.append(px[mid, :3].tolist())
    for order in ([0], [1]):                                  # each alone: the same t
        _, rays = F.run_frame("oracle", F.Frame(resized(mol_job(base, pair[order], [0], 2), 67, 45)))
        assert rays["maxt"][mid] == np.float32(K)
    assert set(seen[0]) <= {127, 254} and set(seen[1]) <= {101, 203} and seen[0] != seen[1]


def both_models_job(seed):
    """A random mesh (test_frames._random_mesh_job) and a random soup / poking atom set in the same box at the same n_slabs, packed as
    test_frame_one_launch.both_job packs them; and the mesh-only and molecule-only jobs of the same frame."""
    _, a04 = fixture("frame_a04_parliament_96x64")
    _, a07 = fixture("frame_a07_parliament_n16_160x120")
    n = (2, 5)[seed % 2]
    mesh = _random_mesh_job(a04, a07, 300 + seed, n)
    mol = random_mol_job(mesh, seed, n, ("soup", "poking")[(seed // 2) % 2])
    both = dict(mesh, mol={k: mol[k] for k in MOL_KEYS})
    return tuple(resized(d, *BOTH_SIZE) for d in (both, mesh, mol))


def uses_group_spheres(d):
    """launch_frame_fused's rule (pt_kernels_frame.hip): group spheres where cells hold 4 groups of 16 slots on average"""
    return len(d["mindex"]) >= int(d["n_slabs"]) ** 3 * 4 * 16


_both = {}


def both_expected(seed):
    """(job, oracle pixels, oracle rays) of the both-models frame, computed once; the oracle alone says that both models show"""
    if seed not in _both:
        d, mesh, mol = both_models_job(seed)
        px, rays = F.run_frame_both("oracle", F.Frame(d))
        mesh_px, _ = F.run_frame("oracle", F.Frame(mesh))
        mol_px, _ = F.run_frame("oracle", F.Frame(mol))
        assert (px != mesh_px).any() and (px != mol_px).any(), "both models have to show"
        px.flags.writeable = False
        rays.flags.writeable = False
        _both[seed] = (d, px, rays)
    return _both[seed]


def test_the_both_models_seeds_show_both_models():
    """CPU: for every seed of test_both_models_match_the_oracle the oracle's frame differs from the mesh-only and from the molecule-only frame, and the
    seeds cover the one-launch kernel's two FS_MOL | FS_MESH instantiations (with and without group spheres)"""
    groups = {uses_group_spheres(both_expected(seed)[0]) for seed in BOTH_SEEDS}
    assert groups == {False, True}


@pytest.mark.skipif(not os.path.exists(REF_A07), reason="oracle/_ref/libref_a07.so not built (the reference's own kernels for the host)")
@pytest.mark.parametrize("kind", KINDS)
def test_oracle_equals_the_compiled_reference_on_generated_jobs(base, kind):
    """CPU: the oracle is a restatement; on one generated job per kind it computes what the reference's own molTrace, compiled for the host, computes"""
    for n, seed in ((5, 0), (2, 1)):
        fr = F.Frame(resized(random_mol_job(base, seed, n, kind), 67, 45))
        px, rays = F.run_frame("oracle", fr)
        want_px, want_rays = F.run_frame("ref", fr)
        assert np.array_equal(px, want_px)
        assert np.array_equal(bits(rays["maxt"]), bits(want_rays["maxt"])) and np.array_equal(bits(rays["mint"]), bits(want_rays["mint"]))


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(pkg):
    from raytracing_amd.pyhost import mirt
    c = mirt.Context(0)
    yield c
    c.destroy()


def same(tag, px, raw, want_px, want_rays):
    """every pixel, and every ray's mint and maxt, bit for bit"""
    assert np.array_equal(px, want_px), f"{tag}: {int((px != want_px).any(axis=1).sum())} pixels differ"
    if raw is not None:
        r = np.ascontiguousarray(raw).view(A.RAY_DT)
        assert np.array_equal(bits(r["maxt"]), bits(want_rays["maxt"])), f"{tag}: maxt"
        assert np.array_equal(bits(r["mint"]), bits(want_rays["mint"])), f"{tag}: mint"


def every_path(ctx, d, want_px, want_rays, stream=False):
    """(a) kernel by kernel, (b) one launch with a ray buffer -- and its 40 written bytes per ray against (a)'s --, (c) one launch without"""
    from raytracing_amd.pyhost import render
    p = render.FramePacked(d)
    px, rays = render.render_frame_stream(ctx, p, rays_fill=0) if stream else render.render_frame(ctx, p)
    same("kernel by kernel", px, rays, want_px, want_rays)
    px1, rays1 = render.render_frame_one_launch(ctx, p, keep_rays=True)
    same("one launch, rays kept", px1, rays1, want_px, want_rays)
    assert np.array_equal(rays40(rays1)[0], rays40(rays)[0]), "the 40 written bytes of every ray"
    px0, none = render.render_frame_one_launch(ctx, p)
    assert none is None
    same("one launch", px0, None, want_px, want_rays)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("kind", KINDS)
def test_random_molecule_frames_match_oracle(ctx, base, kind, n, seed):
    info = {}
    job = random_mol_job(base, seed, n, kind, info)
    for size in SIZES:
        d = resized(job, *size)
        want_px, want_rays = F.run_frame("oracle", F.Frame(d))
        guard(kind, info, size, want_px, want_rays, base)
        every_path(ctx, d, want_px, want_rays)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", BOTH_SEEDS)
def test_both_models_match_the_oracle(ctx, seed):
    """The both-models frame against an independent reference: the oracle's initTrace, molTrace, meshTrace in the page's computeBoth order on one pixel
    and one ray array -- the three-kernel stream, and the one-launch frame's FS_MOL | FS_MESH path with and without group spheres."""
    from raytracing_amd.pyhost import render
    d, want_px, want_rays = both_expected(seed)
    p = render.FramePacked(d)
    assert p.both is not None and not p.mol
    every_path(ctx, d, want_px, want_rays, stream=True)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,n", [(s, n) for s in range(3) for n in (0, 1, 5)])
def test_random_meshes_one_launch_match_oracle(ctx, seed, n):
    """test_frames.test_random_meshes_frames_match_oracle's jobs through the one-launch frame's FS_A04 (n = 0) and FS_MESH modes, with and without rays"""
    from raytracing_amd.pyhost import render
    _, a04 = fixture("frame_a04_parliament_96x64")
    _, a07 = fixture("frame_a07_parliament_n16_160x120")
    d = resized(_random_mesh_job(a04, a07, 100 + seed, n), 320, 200)
    want_px, want_rays = F.run_frame("oracle", F.Frame(d))
    assert lit(want_px).mean() > 0.004
    p = render.FramePacked(d)
    px1, rays1 = render.render_frame_one_launch(ctx, p, keep_rays=True)
    same("one launch, rays kept", px1, rays1, want_px, want_rays)
    px0, _ = render.render_frame_one_launch(ctx, p)
    same("one launch", px0, None, want_px, want_rays)
