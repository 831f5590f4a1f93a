"""GPU: the query kernels at the edges of their work-item prologue and their deferred hand-over -- a last wave and a last mask word that are partly
filled, a wave holding deferred and accepted units side by side, the exact kernel with a redo mask (behind the optimistic one) and without one
(set_exact_only).  The existing batches are 4096 + 37 rays and 37 x 21 tiles; here the SAME inputs are cut at the sizes the kernels' lane, wave
and mask-word arithmetic turns on, and every cut must give the bytes the whole gives.  Nothing is compared with the oracle: the existing tests
pin the whole batch and the whole image to it (tests/test_rays.py, test_radiance.py, test_guides.py, test_ao.py, test_view_guides.py,
test_view_ao.py), so a prefix or a row tile that equals the whole's records bit for bit is the oracle's too.

Ray kinds (trace_closest with hits + sets, trace_occluded, trace_radiance), strata single_cell (no grids: a lane without work leaves) and guard
(grids: it rides along dead; the guard refuses part of every wave), the first n rays of rays_common.rays_of(stratum) for n in PREFIXES:
  - the n records equal the first n of the full batch, and the sentinel bytes behind record n are untouched;
  - under set_exact_only(True) the same bytes come back and the kind's counter reads 0;
  - without it the counter is at most n and at least the number of live prefix rays that rays_common.guard_accepts refuses.
Pixel kinds (render_guides, render_ao on the guard scene, 37 x 21 x 4; view_guides, view_ao with the camera mixed_k2 of
tests/view_cameras_common.py, 1000 x 8 at k = 2): row tiles of 1 row and of 7 rows -- 37 and 259 pixels of the scene's image (one partial wave
that straddles a mask word; one block plus three pixels), 1000 and 7000 of the view's (3 blocks + 232 and 27 blocks + 88: a partial wave and a
partial mask word each) -- equal the same rows of the whole-image call; seeds are filled from the tile's first ray, as
tests/test_deferred_counters.py fills them; the sentinels are untouched; the same bytes come back under exact-only."""
import numpy as np
import pytest

import a10_pass as A
import ao_common as AO
import radiance_common as RC
import rays_common as R
import view_cameras_common as VC

pytestmark = pytest.mark.gpu

STRATA = ("single_cell", "guard")
PREFIXES = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257)
RAY_KINDS = ("closest", "occluded", "radiance")
PIXEL_KINDS = ("guides", "ao", "view_guides", "view_ao")
SCENE_TILES = {1: (5, 1), 7: (5, 7)}     # rows -> (row0, nrows) of the guard scene's 21 rows
VIEW_TILES = {1: (2, 1), 7: (1, 7)}      # ... of mixed_k2's 8 rows (rows 1 and 2 are the band where deferral depends on the column)
SAMPLES, RADIUS, BIAS = 3, 16.0, 0.001   # the AO parameters of tests/test_ao.py on this stratum
BOUNCES = 2
SENTINEL, TAIL = 0xA7, 64


@pytest.fixture(scope="module")
def ctx(pkg):
    from raytracing_amd.pyhost import mirt
    c = mirt.Context(0)
    yield c
    c.destroy()


# ---- ray kinds --------------------------------------------------------------------------------------------------------------------------------
class RayRig:
    """a stratum's tracers; run(kind, n) -> (the output records as byte arrays, the sentinel tails) of the batch's first n rays"""

    def __init__(self, ctx, stratum):
        self.ctx = ctx
        self.rays = R.rays_of(stratum)[0]
        self.seeds = A.make_seeds(len(self.rays))
        self.tracer = R.Tracer(ctx, R.scene(stratum))
        self.radiance = RC.RadianceTracer(ctx, R.scene(stratum))
        self.full = {}

    def run(self, kind, n):
        rays = self.rays[:n]
        if kind == "closest":
            hits, sets, tails = self.tracer.closest(rays)
            return (hits.view(np.uint8).reshape(-1).copy(), sets.view(np.uint8).copy()), tails
        if kind == "occluded":
            occ, tail = self.tracer.occluded(rays)
            return (occ.copy(),), (tail,)
        acc, seeds, tails = self.radiance.run(rays, self.seeds[:n], bounces=BOUNCES)
        return (acc.view(np.uint8).reshape(-1), seeds.view(np.uint8)), tails

    def counter(self, kind):
        return self.ctx.radiance_deferred() if kind == "radiance" else self.ctx.trace_deferred()

    def whole(self, kind):
        """the full batch's records, computed once and shared"""
        if kind not in self.full:
            out, _ = self.run(kind, len(self.rays))
            for a in out:
                a.setflags(write=False)
            self.full[kind] = out
        return self.full[kind]

    def release(self):
        self.tracer.release()
        self.radiance.release()


@pytest.fixture(scope="module")
def ray_rigs(ctx):
    rigs = {s: RayRig(ctx, s) for s in STRATA}
    yield rigs
    for r in rigs.values():
        r.release()


@pytest.mark.parametrize("n", PREFIXES)
@pytest.mark.parametrize("kind", RAY_KINDS)
@pytest.mark.parametrize("stratum", STRATA)
def test_a_prefix_of_the_batch_gives_the_batch_s_first_records(ray_rigs, stratum, kind, n):
    rig = ray_rigs[stratum]
    whole = rig.whole(kind)
    got, tails = rig.run(kind, n)
    deferred = rig.counter(kind)
    refused = int((R.live(rig.rays[:n]) & ~R.guard_accepts(rig.rays[:n])).sum())
    print(f"{stratum} {kind} n={n}: deferred {deferred}, live rays the guard refuses {refused}")
    for g, w in zip(got, whole):
        per = len(w) // len(rig.rays)
        assert np.array_equal(g, w[:n * per]), f"{stratum} {kind}: the first {n} rays alone differ from the first {n} records of the full batch"
    assert all(R.untouched(t) for t in tails), f"{stratum} {kind}: bytes behind record {n} were written"
    assert refused <= deferred <= n, f"{stratum} {kind}: {deferred} deferred of {n} rays, {refused} of them live and refused by the guard"
    rig.ctx.set_exact_only(True)
    try:
        exact, exact_tails = rig.run(kind, n)
        exact_deferred = rig.counter(kind)
    finally:
        rig.ctx.set_exact_only(False)
    for g, e in zip(got, exact):
        assert np.array_equal(g, e), f"{stratum} {kind}: the exact kernel alone gives other bytes for the first {n} rays"
    assert all(R.untouched(t) for t in exact_tails), f"{stratum} {kind}, exact only: bytes behind record {n} were written"
    assert exact_deferred == 0, f"{stratum} {kind}, exact only: the counter reads {exact_deferred}"


# ---- pixel kinds ------------------------------------------------------------------------------------------------------------------------------
class PixelRig:
    """the guard scene and the camera mixed_k2; run(kind, tile) -> (the output records as byte arrays, the sentinel tails), tile = (row0, nrows)
    or None for the whole image"""

    def __init__(self, ctx):
        from raytracing_amd.pyhost import mirt
        self.ctx = ctx
        self.sc = R.scene("guard")
        self.dev = mirt.DeviceScene(ctx, self.sc)
        self.view = VC.view("guard", "mixed_k2").tile(0, 0)   # the camera's whole frame: 8 rows
        self.full = {}

    def _filled(self, nbytes):
        return self.ctx.buffer(nbytes + TAIL).write(np.full(nbytes + TAIL, SENTINEL, np.uint8))

    def _guides(self, call, npix):
        nh, ad = self._filled(npix * 16), self._filled(npix * 16)
        try:
            call(nh, ad)
            a, b = nh.read(np.uint8), ad.read(np.uint8)
        finally:
            nh.release()
            ad.release()
        return (a[:npix * 16].copy(), b[:npix * 16].copy()), (a[npix * 16:], b[npix * 16:])

    def run(self, kind, tile):
        c, sc = self.ctx, self.sc
        if kind == "guides":
            row0, nrows = tile or (0, sc.height)
            desc = self.dev.pass_desc(None, None, row0=row0, nrows=nrows if tile else 0)
            return self._guides(lambda nh, ad: c.render_guides(desc, nh, ad), sc.width * nrows)
        if kind == "ao":
            ao = AO.Ao(c, sc, *(tile or (0, None)))   # seeds filled from the tile's first ray
            try:
                out, tail = ao.run(SAMPLES, RADIUS, BIAS)
            finally:
                ao.release()
            return (out.view(np.uint8).reshape(-1),), (tail,)
        v = self.view.tile(*tile) if tile else self.view
        scene_desc, vdesc = self.dev.pass_desc(None, None), v.desc()
        if kind == "view_guides":
            return self._guides(lambda nh, ad: c.view_guides(scene_desc, vdesc, nh, ad), v.n_pixels)
        seeds, out = c.buffer(v.n_rays * 4), self._filled(v.n_pixels * 8)
        try:
            c.seed_fill(seeds, v.row0 * v.width * v.rpp, v.n_rays)
            c.view_ao(scene_desc, vdesc, seeds, out, SAMPLES, RADIUS, BIAS)
            raw = out.read(np.uint8)
        finally:
            seeds.release()
            out.release()
        return (raw[:v.n_pixels * 8].copy(),), (raw[v.n_pixels * 8:],)

    def whole(self, kind):
        if kind not in self.full:
            out, tails = self.run(kind, None)
            assert all(R.untouched(t) for t in tails), kind
            for a in out:
                a.setflags(write=False)
            self.full[kind] = out
        return self.full[kind]

    def release(self):
        self.dev.release()


@pytest.fixture(scope="module")
def pixel_rig(ctx):
    r = PixelRig(ctx)
    yield r
    r.release()


@pytest.mark.parametrize("rows", (1, 7))
@pytest.mark.parametrize("kind", PIXEL_KINDS)
def test_a_row_tile_gives_the_whole_image_s_rows(pixel_rig, kind, rows):
    rig = pixel_rig
    view_kind = kind.startswith("view_")
    row0, nrows = (VIEW_TILES if view_kind else SCENE_TILES)[rows]
    width = rig.view.width if view_kind else rig.sc.width
    whole = rig.whole(kind)
    got, tails = rig.run(kind, (row0, nrows))
    if kind == "ao":
        print(f"{kind} rows [{row0}, +{nrows}): {rig.ctx.ao_deferred()} of {width * nrows} pixels deferred")
    if kind == "view_ao":
        print(f"{kind} rows [{row0}, +{nrows}): {rig.ctx.view_ao_deferred()} of {width * nrows} pixels deferred")
    for g, w in zip(got, whole):
        per = len(g) // (width * nrows)
        assert np.array_equal(g, w[row0 * width * per:(row0 + nrows) * width * per]), f"{kind}: rows [{row0}, +{nrows}) alone differ from the same rows of the whole image"
    assert all(R.untouched(t) for t in tails), f"{kind}: bytes behind the tile's last pixel were written"
    rig.ctx.set_exact_only(True)
    try:
        exact, exact_tails = rig.run(kind, (row0, nrows))
    finally:
        rig.ctx.set_exact_only(False)
    for g, e in zip(got, exact):
        assert np.array_equal(g, e), f"{kind}: the exact kernel alone gives other bytes for rows [{row0}, +{nrows})"
    assert all(R.untouched(t) for t in exact_tails), f"{kind}, exact only: bytes behind the tile's last pixel were written"
