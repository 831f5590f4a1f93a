"""Shared by the view-camera guide tests (mirt_view_guides, mirt_render_view_guided): what the guides are checked against, and the library side.

The guides are defined by composition (include/mirt.h): the rays of view_common.view_rays, each through rays_common.expected_closest (the CPU
oracle's sphereTrace, triangleTrace and every meshTrace on a Poi reset as initTrace resets it), reduced per pixel in sample order by
guides_common.reduce_guides -- one np.float32 addition at a time, over the samples with 0 <= matId < the number of material entries."""
import numpy as np

import guides_common as G
import rays_common as R
import view_cameras_common as VC
import view_common as V

f32 = np.float32
SENTINEL = V.SENTINEL
FIXTURES = ("cornell_32x24_r4", "cornell_teapot3_32x24_r4")
# (stratum, camera) of view_cameras_common the GPU tests render beside the fixtures' standard views
CATALOGUE = (("staged", "rim_17x40_pi"), ("single_cell", "clipped_ortho"), ("staged", "on_face"), ("single_cell", "oblique_fisheye"))
EXACT = (("staged", "all_refused"),) + tuple(("staged", n) for n in VC.MIXED_K)

_CACHE = {}


def mat_ids(hits):
    return np.ascontiguousarray(hits[:, 7]).view(np.int32)


def reduce_hits(hits, materials, rpp):
    """hit records [n, 8] (normal.xyz, t, p.xyz, matId's bits) -> (normal_hits, albedo_depth)"""
    hits = np.asarray(hits, f32).reshape(-1, 8)
    return G.reduce_guides(hits[:, 3], hits[:, 0:3], mat_ids(hits), materials, rpp)


def expected(sc, v, materials=None):
    """-> (normal_hits, albedo_depth), float32 [n_pixels, 4] each, as mirt_view_guides defines them; materials: a table other than the scene's"""
    hits, _sets = R.expected_closest(sc, V.view_rays(v))
    return reduce_hits(hits, sc.materials if materials is None else materials, v.rpp)


def cached(key, make):
    if key not in _CACHE:
        out = make()
        for a in out:
            a.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def expected_catalogue(stratum, name):
    return cached(("catalogue", stratum, name), lambda: expected(R.scene(stratum), VC.view(stratum, name)))


def kinds(nh, rpp):
    """(pixels without a hit, pixels every sample of which hit, pixels partly hit)"""
    hits = np.asarray(nh, f32)[:, 3]
    none, every = int((hits == 0).sum()), int((hits == rpp).sum())
    return none, every, len(hits) - none - every


def differ(tag, got, want):
    """(normal_hits, albedo_depth) pairs: None when equal bit for bit (every NaN equal to every NaN; a None member is not compared)"""
    for label, g, w in zip(("normal_hits", "albedo_depth"), got[:2], want[:2]):
        if g is None or w is None:
            continue
        d = G.difference(f"{tag} {label}", g, w)
        if d:
            return d
    return None


# ---- the library ------------------------------------------------------------------------------------------------------------------------------
class Renderer(V.Renderer):
    """view_common.Renderer with the two guide buffers of `cap_pixels` float4 each, followed by `tail` sentinel bytes like the others"""

    def __init__(self, ctx, sc, cap_rays, cap_pixels, tail=64):
        super().__init__(ctx, sc, cap_rays, cap_pixels, tail)
        self.nh, self.ad = ctx.buffer(cap_pixels * 16 + tail), ctx.buffer(cap_pixels * 16 + tail)

    def _fill_guides(self):
        for b in (self.nh, self.ad):
            b.write(np.full(b.nbytes, SENTINEL, np.uint8))

    def _read_guides(self, npx, nh, ad):
        a, b = self.nh.read(np.uint8), self.ad.read(np.uint8)
        clean = bool((a[npx * 16 if nh else 0:] == SENTINEL).all() and (b[npx * 16 if ad else 0:] == SENTINEL).all())
        return (a[:npx * 16].view(f32).reshape(-1, 4).copy() if nh else None, b[:npx * 16].view(f32).reshape(-1, 4).copy() if ad else None, clean)

    def guides(self, view, nh=True, ad=True, scene_desc=None):
        """mirt_view_guides -> (normal_hits or None, albedo_depth or None, untouched: the bytes behind the records, and a buffer not given, still
        hold the sentinel)"""
        self._fill_guides()
        self.ctx.view_guides(scene_desc or self.scene_desc(0), view.desc(), self.nh if nh else None, self.ad if ad else None)
        return self._read_guides(view.n_pixels, nh, ad)

    def _load(self, view, seeds, carry):
        n, npx = view.n_rays, view.n_pixels
        s = np.full(self.seeds.nbytes, SENTINEL, np.uint8)
        s[:n * 4] = np.ascontiguousarray(seeds, np.int32).view(np.uint8)
        r = np.full(self.radiance.nbytes, SENTINEL, np.uint8)
        if carry is not None:
            r[:npx * 16] = np.ascontiguousarray(carry, f32).reshape(-1).view(np.uint8)
        self.seeds.write(s)
        self.radiance.write(r)
        self.pixel.write(np.full(self.pixel.nbytes, SENTINEL, np.uint8))
        self._fill_guides()

    def _frame(self, view):
        n, npx = view.n_rays, view.n_pixels
        s, r, p = self.seeds.read(np.uint8), self.radiance.read(np.uint8), self.pixel.read(np.uint8)
        clean = bool((s[n * 4:] == SENTINEL).all() and (r[npx * 16:] == SENTINEL).all() and (p[npx * 4:] == SENTINEL).all())
        return s[:n * 4].view(np.int32).copy(), r[:npx * 16].view(f32).reshape(-1, 4).copy(), p[:npx * 4].reshape(-1, 4).copy(), clean

    def guided(self, view, seeds, bounces=2, carry=None):
        """mirt_render_view_guided -> ((seeds, radiance, pixel, untouched), (normal_hits, albedo_depth, untouched))"""
        self._load(view, seeds, carry)
        self.ctx.render_view_guided(self.scene_desc(bounces), view.desc(V.ACCUMULATE if carry is not None else 0), self.seeds, self.radiance, self.pixel,
                                    self.nh, self.ad)
        return self._frame(view), self._read_guides(view.n_pixels, True, True)

    def two_calls(self, view, seeds, bounces=2, carry=None):
        """mirt_render_view, then mirt_view_guides: the same shape of result"""
        self._load(view, seeds, carry)
        self.ctx.render_view(self.scene_desc(bounces), view.desc(V.ACCUMULATE if carry is not None else 0), self.seeds, self.radiance, self.pixel)
        self.ctx.view_guides(self.scene_desc(bounces), view.desc(), self.nh, self.ad)
        return self._frame(view), self._read_guides(view.n_pixels, True, True)

    def release(self):
        for b in (self.nh, self.ad):
            b.release()
        super().release()


def composition(ctx, r, v, materials):
    """this library's own steps: mirt_view_rays, mirt_trace_closest, then reduce_guides in numpy"""
    n = v.n_rays
    rays, hits = ctx.buffer(n * 32), ctx.buffer(n * 32)
    try:
        ctx.view_rays(v.desc(), rays)
        ctx.trace_closest(r.scene_desc(0), rays, n, hits, None)
        return reduce_hits(hits.read(f32).reshape(-1, 8), materials, v.rpp)
    finally:
        rays.release()
        hits.release()


def same_frames(tag, got, want):
    """results of Renderer.guided / two_calls: None when every buffer is equal bit for bit"""
    return V.differ(tag, got[0], want[0]) or differ(tag, got[1], want[1])


# ---- the checks the GPU tests and their child processes share ---------------------------------------------------------------------------------------
SIZES = [(13, 7, k) for k in V.KS] + [(1, 1, 1), (65, 1, 2)]
ONE_LAUNCH_KS = (1, 2, 4, 8)   # where a pixel's samples are consecutive lanes of one wave: pt_view_plan.hpp view_guides_in_pass


def composition_difference(ctx, r, sc, v, tag):
    """mirt_view_guides against this library's mirt_view_rays + mirt_trace_closest + numpy reduce_guides, both outputs together and each alone,
    the sentinel bytes behind the records untouched -> (a sentence or None, the composition's guides)"""
    want = composition(ctx, r, v, sc.materials)
    for nh, ad in ((True, True), (True, False), (False, True)):
        got = r.guides(v, nh=nh, ad=ad)
        d = differ(f"{tag} nh={nh} ad={ad}", got, want)
        if d is None and not got[2]:
            d = f"{tag} nh={nh} ad={ad}: bytes behind the records, or a buffer that was not given, were written"
        if d:
            return d, want
    return None, want


def guided_difference(ctx, r, v, seeds, tag, bounces=2, carry=None, one_launch=None):
    """mirt_render_view_guided against mirt_render_view then mirt_view_guides in all five buffers, and mirt_ctx_guided_views against the route
    rule (one_launch: whether the call is to take it; None: by k) -> (a sentence or None, the guided call's result)"""
    want = r.two_calls(v, seeds, bounces, carry)
    before = ctx.guided_views()
    got = r.guided(v, seeds, bounces, carry)
    routed = ctx.guided_views() - before
    d = same_frames(tag, got, want)
    if d is None and not (got[0][3] and got[1][2] and want[0][3] and want[1][2]):
        d = f"{tag}: bytes behind the records were written"
    expect = (v.k in ONE_LAUNCH_KS) if one_launch is None else one_launch
    if d is None and routed != int(expect):
        d = f"{tag}: mirt_ctx_guided_views went up by {routed}, the route rule says {int(expect)}"
    return d, got
