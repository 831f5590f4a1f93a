"""Shared by the view-camera AO tests (mirt_view_ao): what the AO pairs are checked against, and the library side.

The pair {open, cast} of a pixel is defined by composition (include/mirt.h), restated here with any checker `k` (a10_pass.load_oracle(), or
ref_gpu.GpuRefKernels() for the reference binary on the device) from pieces the other tests already have:

  view_common.view_rays(v)            the tile's rays (or `rays`, when the caller has them from elsewhere)
  rays_common._closest_stages         sphereTrace, triangleTrace and every meshTrace in upload order on a Poi buffer with matId = -1
  a10_pass.make_seeds(n, first)       the seeds of the tile: global ray ids, first = row0 * width * rpp
  `samples` times k.bouncePaths       on a SCRATCH ray buffer with the advancing copy of the seeds: the Poi buffer is unchanged, so call j stores
                                      getHemisphereRay's j-th ray of every casting sample (Poi.matId >= 0)
  ao_common.ao_rays, rays_common.expected_occluded, ao_common.count_ao

Nothing here is tuned to the library: integers, tolerance 0."""
import numpy as np

import a10_pass as A
import rays_common as R
import view_cameras_common as VC
import view_common as V
from ao_common import ao_rays, count_ao, difference  # noqa: F401  (difference: re-exported for the tests)

SENTINEL, TAIL = 0xA7, 64
SAMPLES, BIAS, INF = 3, 0.001, float("inf")
FIXTURES = ("cornell_32x24_r4", "cornell_teapot3_32x24_r4")
MODELS = ("ortho", "equirect", "fisheye")
# per stratum: the radius of tests/test_ao.py (the guard stratum's geometry is scaled by 16)
RADIUS = {"single_cell": 1.0, "staged": 1.0, "unstaged": 1.0, "many_sets": 1.0, "open": 1.0, "guard": 16.0}
# `open` x fisheye sits at open / cast = 0.09998, just under the non-vacuity bound: left out
STRATA_CASES = tuple((s, m) for s in RADIUS for m in MODELS if (s, m) != ("open", "fisheye"))
# the fixtures' standard views at 13 x 7, k = 2, radius 1.0: the pixels that cast nothing (0: the table shows none)
FIXTURE_EMPTY = {("cornell_32x24_r4", "ortho"): 0, ("cornell_32x24_r4", "equirect"): 7, ("cornell_32x24_r4", "fisheye"): 12,
                 ("cornell_teapot3_32x24_r4", "ortho"): 0, ("cornell_teapot3_32x24_r4", "equirect"): 8, ("cornell_teapot3_32x24_r4", "fisheye"): 12}
# one model each with radius inf and with bias 0
FIXTURE_VARIANTS = (("cornell_32x24_r4", "ortho", INF, BIAS), ("cornell_teapot3_32x24_r4", "equirect", INF, BIAS), ("cornell_32x24_r4", "fisheye", 1.0, 0.0),
                    ("cornell_teapot3_32x24_r4", "ortho", 1.0, 0.0))
CATALOGUE = (("staged", "rim_17x40_pi"), ("single_cell", "clipped_ortho"), ("staged", "on_face"), ("single_cell", "oblique_fisheye"))
EXACT = (("staged", "all_refused"),) + tuple(("staged", n) for n in VC.MIXED_K)
# catalogue cameras the table shows pixels casting nothing for
CATALOGUE_EMPTY = {"rim_17x40_pi", "clipped_ortho", "on_face", "oblique_fisheye"}
SIZES = [(13, 7, k) for k in V.KS if k < 16] + [(5, 3, 16), (1, 1, 1), (65, 1, 2)]

_CACHE = {}
_SCENES = {}


def scene(name):
    if name not in _SCENES:
        from conftest import load_fixture
        _SCENES[name] = load_fixture(name)[1] if name in FIXTURES else R.scene(name)
    return _SCENES[name]


def tile_seeds(v):
    """the seeds of a view's tile: global ray ids, as mirt_seed_fill(first = row0 * width * rpp) fills them"""
    return A.make_seeds(v.n_rays, first=v.row0 * v.width * v.rpp)


def first_hits(sc, rays, k):
    """-> (Poi buffer, launch size): the rays through the closest-hit stages on a Poi buffer with matId = -1"""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    n = len(rays)
    rb, g1 = R._ray_buffer(rays)
    pb = np.zeros(g1, A.POI_DT)
    pb["matId"] = -1
    for call in R._closest_stages(k, sc, n, rb, pb, g1):
        call()
        k.flush()
    return pb, g1


def expected_from_pois(sc, pois, n, seeds, rpp, samples, radius, bias, k):
    """the AO pairs of n samples whose first-hit state is `pois` (a Poi buffer of a whole launch size), by the checker k"""
    g1 = len(pois)
    B = k.buf
    sd = np.zeros(g1, np.int32)
    sd[:n] = seeds
    scratch = np.zeros(g1, A.RAY_DT)
    cast = pois["matId"][:n] >= 0
    occ = []
    for _ in range(samples):
        k.bouncePaths(B(pois), B(scratch), B(sd), n, g1)
        k.flush()
        occ.append(R.expected_occluded(sc, ao_rays(scratch[:n], pois[:n], cast, radius, bias), k))
    return count_ao(cast, occ, rpp)


def expected(sc, v, samples=SAMPLES, radius=1.0, bias=BIAS, k=None, rays=None, seeds=None):
    """uint32 [n_pixels, 2], {open, cast} per pixel of the view's tile as mirt_view_ao defines them"""
    k = k or A.load_oracle()
    rays = V.view_rays(v) if rays is None else rays
    pois, _g1 = first_hits(sc, rays, k)
    return expected_from_pois(sc, pois, v.n_rays, tile_seeds(v) if seeds is None else seeds, v.rpp, samples, radius, bias, k)


def cached(key, make):
    if key not in _CACHE:
        out = make()
        out.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def expected_standard(name, model, radius=1.0, bias=BIAS, width=13, height=7, k=2):
    """a fixture's or a stratum's standard view; strata run at 37 x 21"""
    return cached(("standard", name, model, radius, bias, width, height, k),
                  lambda: expected(scene(name), V.standard_view(scene(name), model, width=width, height=height, k=k), SAMPLES, radius, bias))


def expected_catalogue(stratum, camera, radius=1.0):
    return cached(("catalogue", stratum, camera, radius), lambda: expected(R.scene(stratum), VC.view(stratum, camera), SAMPLES, radius, BIAS))


def not_vacuous(tag, want, samples, rpp, need_empty=False):
    """on the ORACLE's result alone -> None, or a sentence: the frame's openness away from 0 and 1, the counts' range, and -- where asked --
    pixels that cast nothing"""
    want = np.asarray(want)
    cast, open_ = int(want[:, 1].sum()), int(want[:, 0].sum())
    print(f"{tag}: oracle open {open_} / cast {cast} = {open_ / max(cast, 1):.4f}, {int((want[:, 1] == 0).sum())} of {len(want)} pixels cast nothing")
    if not cast > 0:
        return f"{tag}: nothing casts"
    if not 0.1 <= open_ / cast <= 0.9:
        return f"{tag}: the case is vacuous, open / cast = {open_} / {cast}"
    if not want[:, 1].max() <= rpp * samples:
        return f"{tag}: a pixel casts {int(want[:, 1].max())} rays, more than rpp * samples = {rpp * samples}"
    if need_empty and not (want[:, 1] == 0).any():
        return f"{tag}: no pixel without a hit"
    return None


# ---- the library ------------------------------------------------------------------------------------------------------------------------------
class Ao:
    """one scene on one context: seeds of `cap_rays` int32 and an ao_out of `cap_pixels` pairs followed by TAIL sentinel bytes"""

    def __init__(self, ctx, sc, cap_rays, cap_pixels):
        from raytracing_amd.pyhost import mirt
        self.ctx = ctx
        self.dev = mirt.DeviceScene(ctx, sc)
        self.cap_rays, self.cap_pixels = cap_rays, cap_pixels
        self.seeds = ctx.buffer(cap_rays * 4)
        self.out = ctx.buffer(cap_pixels * 8 + TAIL)

    def scene_desc(self):
        return self.dev.pass_desc(None, None)

    def run(self, v, samples=SAMPLES, radius=1.0, bias=BIAS, seeds=None, scene_desc=None):
        """mirt_view_ao with the tile's global seeds (mirt_seed_fill), or `seeds` -> (uint32 [n_pixels, 2], untouched: the bytes behind the pairs
        still hold the sentinel, and the seeds are byte for byte what they were)"""
        n, npx = v.n_rays, v.n_pixels
        assert n <= self.cap_rays and npx <= self.cap_pixels
        if seeds is None:
            self.ctx.seed_fill(self.seeds, v.row0 * v.width * v.rpp, n)
        else:
            self.seeds.write(np.ascontiguousarray(seeds, np.int32))
        before = self.seeds.read(np.uint8).tobytes()
        self.out.write(np.full(self.out.nbytes, SENTINEL, np.uint8))
        self.ctx.view_ao(scene_desc or self.scene_desc(), v.desc(), self.seeds, self.out, samples, radius, bias)
        raw = self.out.read(np.uint8)
        clean = bool((raw[npx * 8:] == SENTINEL).all()) and self.seeds.read(np.uint8).tobytes() == before
        return raw[:npx * 8].view(np.uint32).reshape(-1, 2).copy(), clean

    def release(self):
        self.seeds.release()
        self.out.release()
        self.dev.release()


def composition(ctx, ao, sc, v, samples, radius, bias, k=None):
    """this library's own steps on the device -- mirt_view_rays, mirt_trace_closest, then per AO sample mirt_trace_occluded on rays rebuilt in numpy
    from the hits -- with the hemisphere directions from the checker's bouncePaths on those hits"""
    k = k or A.load_oracle()
    n = v.n_rays
    g1 = A._ceil(max(n, 1), A.WAVE)
    rays, hits = ctx.buffer(n * 32), ctx.buffer(n * 32)
    try:
        ctx.view_rays(v.desc(), rays)
        ctx.trace_closest(ao.scene_desc(), rays, n, hits, None)
        h = hits.read(np.float32).reshape(-1, 8)
    finally:
        rays.release()
        hits.release()
    pois = np.zeros(g1, A.POI_DT)
    pois["matId"] = -1
    pois["normal"][:n, 0:3], pois["p"][:n, 0:3] = h[:, 0:3], h[:, 4:7]
    pois["matId"][:n] = np.ascontiguousarray(h[:, 7]).view(np.int32)
    cast = pois["matId"][:n] >= 0
    B = k.buf
    sd = np.zeros(g1, np.int32)
    sd[:n] = tile_seeds(v)
    scratch = np.zeros(g1, A.RAY_DT)
    tr = R.Tracer(ctx, sc, cap=max(int(cast.sum()), 1), tail=0)
    try:
        occ = []
        for _ in range(samples):
            k.bouncePaths(B(pois), B(scratch), B(sd), n, g1)
            k.flush()
            occ.append(tr.occluded(ao_rays(scratch[:n], pois[:n], cast, radius, bias))[0].copy())
    finally:
        tr.release()
    return count_ao(cast, occ, v.rpp)
