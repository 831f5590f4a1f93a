"""Pass drivers over the C ABI, in Python, for tests and bench.py.

`GranularRenderer` is a line-by-line functional mirror of the reference host's kernel
plumbing -- preRender() / executeRender() of A10 code.js:1784-1854 with its prepare*/execute*
helpers (:1078-1528) -- written against pyhost.mirt instead of WebCL: same kernels, same
argument indices, same enqueue order, same NDRange padding.  It exists so that the parity
tests read like the reference's own call sequence.  `FusedRenderer` is the one-launch path
(mirt_render_pass).  The JavaScript host in ../host/ has the same two drivers; that is the
product, this is tooling.
"""
import math

import numpy as np

from . import mirt

RAY_BYTES, POI_BYTES = 48, 64


def _u32(v):
    return np.array([v], np.uint32)


def _f32(v):
    return np.array([v], np.float32)


def get_local_ws(dim, multiple):
    """getLocalWS (A10 code.js:645-672)."""
    if dim == 1:
        return [multiple]
    x = int(math.floor(math.sqrt(multiple)))
    if x & (x - 1):
        x = 1 << (x - 1).bit_length()
    return [x, multiple // x]


class GranularRenderer:
    def __init__(self, ctx, scene, seeds=None, seed_base=0):
        self.ctx, self.s = ctx, scene
        self.dev = mirt.DeviceScene(ctx, scene)
        self.k, self.b, self.gws, self.lws = {}, {}, {}, {}
        self.passes = 1
        self._pre_render(seeds, seed_base)

    # -- preRender (code.js:1784-1804)
    def _pre_render(self, seeds, seed_base):
        ctx, s = self.ctx, self.s
        n = s.total_rays
        self.total_rays = n
        # getStructSize (code.js:1064-1076)
        sizes = {}
        for name in ("Ray", "Poi"):
            k = ctx.kernel("sizeof" + name)
            tmp = ctx.buffer(4, mirt.MEM_WRITE_ONLY)
            k.set_arg(0, tmp)
            k.enqueue([1], [1])
            sizes[name] = int(tmp.read(np.uint32, 1)[0])
            tmp.release()
            k.release()
        self.ray_size, self.poi_size = sizes["Ray"], sizes["Poi"]

        # prepareInitAcu (code.js:1078-1099)
        self.b["acu"] = ctx.buffer(n * 16)
        k = ctx.kernel("initAcu").set_args(self.b["acu"], _u32(n))
        l = get_local_ws(1, 64)
        k.enqueue([-(-n // l[0]) * l[0]], l)
        ctx.finish()
        k.release()
        # prepareInitSeeds (code.js:1140-1154)
        self.b["seeds"] = ctx.buffer(n * 4)
        if seeds is not None:
            self.b["seeds"].write(np.asarray(seeds, np.int32))
        else:
            ctx.seed_fill(self.b["seeds"], 0, n, seed_base)
        # prepareInitTrace (code.js:1101-1138)
        self.b["rays"] = ctx.buffer(n * self.ray_size)
        self.b["pois"] = ctx.buffer(n * self.poi_size)
        self.k["initTrace"] = ctx.kernel("initTrace").set_args(
            self.b["seeds"], self.b["rays"], self.b["pois"], s.bounds, None, _f32(s.focal_length), _f32(s.lens_rad), _u32(s.rpp))
        l = get_local_ws(2, 64)
        self.lws["initTrace"] = l
        self.gws["initTrace"] = [-(-s.width // l[0]) * l[0], -(-s.height // l[1]) * l[1]]
        g1 = [-(-n // 64) * 64]
        d = self.dev
        if s.has_spheres:  # prepareSphereTrace (code.js:1156-1202)
            self.k["sphereTrace"] = ctx.kernel("sphereTrace").set_args(
                _u32(n), self.b["pois"], self.b["rays"], d.sph["prims"], d.sph["matid"], d.sph["off"], s.sphere_bounds, _u32(s.n_slabs))
        if s.has_triangles:  # prepareTriangleTrace (code.js:1204-1252)
            self.k["triangleTrace"] = ctx.kernel("triangleTrace").set_args(
                _u32(n), self.b["pois"], self.b["rays"], d.tri["prims"], d.tri["normals"], d.tri["matid"], d.tri["off"],
                s.triangle_bounds, _u32(s.n_slabs))
        if s.meshes:  # prepareMeshTrace (code.js:1254-1291)
            self.k["meshTrace"] = ctx.kernel("meshTrace").set_args(_u32(n), self.b["pois"], self.b["rays"])
        # prepareInitShadowTrace (code.js:1417-1442)
        self.b["shadow"] = ctx.buffer(n * self.ray_size)
        self.k["initShadowTrace"] = ctx.kernel("initShadowTrace").set_args(self.b["shadow"], self.b["pois"], _u32(n), None, self.b["seeds"])
        if s.has_spheres:  # prepareSphereShadowTrace (code.js:1461-1479)
            self.k["sphereShadowTrace"] = ctx.kernel("sphereShadowTrace").set_args(
                _u32(n), self.b["shadow"], d.sph["prims"], d.sph["off"], s.sphere_bounds, _u32(s.n_slabs))
        if s.has_triangles or s.meshes:  # prepareTriangleShadowTrace (code.js:1481-1499)
            self.k["triangleShadowTrace"] = ctx.kernel("triangleShadowTrace").set_args(_u32(n), self.b["shadow"])
        # prepareSceneRender (code.js:1364-1395)
        self.k["sceneRender"] = ctx.kernel("sceneRender").set_args(self.b["acu"], self.b["pois"], self.b["shadow"], d.material, None, _u32(n))
        # prepareCopyToPixel (code.js:1305-1326)
        npix = s.width * s.height
        self.b["pixel"] = ctx.buffer(npix * 4, mirt.MEM_WRITE_ONLY)
        self.k["copyToPixel"] = ctx.kernel("copyToPixel").set_args(self.b["pixel"], self.b["acu"], None, _u32(npix), _u32(s.rpp))
        self.gws["copyToPixel"] = [-(-npix // 64) * 64]
        # prepareBouncePaths (code.js:1444-1459), prepareLightRender (code.js:1346-1362)
        self.k["bouncePaths"] = ctx.kernel("bouncePaths").set_args(self.b["pois"], self.b["rays"], self.b["seeds"], _u32(n))
        self.k["lightRender"] = ctx.kernel("lightRender").set_args(self.b["pois"], self.b["rays"], self.b["acu"], None, _u32(n))
        self.g1 = g1

    def _closest(self):
        s, k, d = self.s, self.k, self.dev
        if s.has_spheres:
            k["sphereTrace"].enqueue(self.g1, [64])
        if s.has_triangles:
            k["triangleTrace"].enqueue(self.g1, [64])
        for m in d.meshes:  # executeMeshTrace (code.js:1293-1303)
            k["meshTrace"].set_arg(3, m["prims"]).set_arg(4, m["normals"]).set_arg(5, m["off"]).set_arg(6, _u32(m["matid"]))
            k["meshTrace"].set_arg(7, m["bounds"]).set_arg(8, _u32(m["n"]))
            k["meshTrace"].enqueue(self.g1, [64])

    def _direct(self):
        s, k, d = self.s, self.k, self.dev
        for l in s.lights:
            k["initShadowTrace"].set_arg(3, l["shadow"]).enqueue(self.g1, [64])
            if s.has_spheres:
                k["sphereShadowTrace"].enqueue(self.g1, [64])
            if s.has_triangles:  # executeTriangleShadowTrace (code.js:1514-1520)
                k["triangleShadowTrace"].set_arg(2, d.tri["prims"]).set_arg(3, d.tri["off"]).set_arg(4, s.triangle_bounds).set_arg(5, _u32(s.n_slabs))
                k["triangleShadowTrace"].enqueue(self.g1, [64])
            for m in d.meshes:  # executeMeshShadowTrace (code.js:1522-1528)
                k["triangleShadowTrace"].set_arg(2, m["prims"]).set_arg(3, m["off"]).set_arg(4, m["bounds"]).set_arg(5, _u32(m["n"]))
                k["triangleShadowTrace"].enqueue(self.g1, [64])
            k["sceneRender"].set_arg(4, l["scene"]).enqueue(self.g1, [64])  # executeSceneRender (code.js:1402-1408)
            if not getattr(self, "_recording", False):   # the reference finishes the queue here (code.js:1406); a recording cannot wait
                self.ctx.finish()

    # -- executeRender (code.js:1806-1854)
    def _enqueue_segments(self, bounces, on_primary=None):
        s, k = self.s, self.k
        k["initTrace"].set_arg(4, s.cam).enqueue(self.gws["initTrace"], self.lws["initTrace"])
        self._closest()
        for l in s.lights:
            k["lightRender"].set_arg(3, l["light"]).enqueue(self.g1, [64])
        self._direct()
        if on_primary:
            on_primary(self)
        for _ in range(bounces):
            k["bouncePaths"].enqueue(self.g1, [64])
            self._closest()
            self._direct()

    def execute_render(self, bounces=5, on_primary=None, use_graph=False):
        """One executeRender() (code.js:1806-1854).  use_graph: the 40-odd enqueues of the pass body are recorded once (on the second
        pass; the first one runs normally and fills the runtime's caches) and replayed as one HIP graph afterwards; copyToPixel stays
        outside because its scale argument changes every pass (code.js:1412)."""
        s, k = self.s, self.k
        if use_graph and on_primary is None and self.passes > 1:
            if getattr(self, "_graph", None) is None or self._graph_bounces != bounces:
                if getattr(self, "_graph", None) is not None:
                    self.ctx.graph_release(self._graph)
                self.ctx.capture_begin()
                self._recording = True
                try:
                    self._enqueue_segments(bounces)
                finally:
                    self._recording = False
                    self._graph = self.ctx.capture_end()
                self._graph_bounces = bounces
            self.ctx.graph_launch(self._graph)
        else:
            self._enqueue_segments(bounces, on_primary)
        div = np.float32(1.0 / (s.rpp * self.passes))  # executeCopyToPixel (code.js:1410-1415)
        k["copyToPixel"].set_arg(2, _f32(div)).enqueue(self.gws["copyToPixel"], [64])
        self.ctx.finish()
        self.passes += 1

    def read(self, name):
        from_dt = {"seeds": np.int32, "acu": np.float32, "pixel": np.uint8, "rays": np.uint8, "pois": np.uint8, "shadow": np.uint8}
        return self.b[name].read(from_dt[name])

    def release(self):
        if getattr(self, "_graph", None) is not None:
            self.ctx.graph_release(self._graph)
            self._graph = None
        for k in self.k.values():
            k.release()
        for b in self.b.values():
            b.release()
        self.dev.release()
        self.k, self.b = {}, {}


class FusedRenderer:
    """One mirt_render_pass per progressive pass over rows [row0, row0+nrows)."""

    def __init__(self, ctx, scene, seeds=None, seed_base=0, row0=0, nrows=None, want_radiance=True, keep_acu=True):
        """nrows None: the whole image from row0 = 0.  nrows == 0 is an EMPTY tile (more ranks than rows): it owns minimal buffers and
        its passes do nothing -- it is not the whole frame.
        keep_acu False: no per-ray accumulator at all (16 B per ray never allocated); only a frame's first pass (or first execute_passes) can then run, with
        rays_per_pixel dividing 256, or any count above 256 (289, 1024, ...: one launch per segment of a pixel's rays): the pass resolves its
        pixels itself (mirt_render_first_pass with acu == NULL)."""
        self.ctx, self.s = ctx, scene
        self.dev = mirt.DeviceScene(ctx, scene)
        self.row0 = row0
        self.nrows = scene.height if nrows is None else nrows
        self.npix = self.nrows * scene.width
        self.nrays = self.npix * scene.rpp
        self.first_ray = row0 * scene.width * scene.rpp
        self.seeds = ctx.buffer(self.nrays * 4 or 16)
        if self.nrays:
            if seeds is not None:
                self.seeds.write(np.asarray(seeds, np.int32)[self.first_ray:self.first_ray + self.nrays])
            else:
                ctx.seed_fill(self.seeds, self.first_ray, self.nrays, seed_base)
        self.acu = None
        if keep_acu:
            self.acu = ctx.buffer(self.nrays * 16 or 16)
            ctx.zero(self.acu)
        self.pixel = ctx.buffer(self.npix * 4 or 16)
        self.radiance = ctx.buffer(self.npix * 16 or 16) if want_radiance else None
        self.passes = 1
        self._desc = None

    def execute_render(self, bounces=5, fresh=False):
        """fresh: first pass of a frame, accumulator initialised by the pass itself (no ctx.zero needed)."""
        if not self.nrays:
            self.passes += 1
            return
        d = self.dev.pass_desc(self.seeds, self.acu, self.pixel, self.radiance, pass_index=self.passes, bounces=bounces,
                               row0=self.row0, nrows=self.nrows)
        self.ctx.render_pass(d, fresh=fresh)
        self.passes += 1

    def execute_passes(self, n, bounces=5, fresh=False, every_frame=False):
        """n progressive passes in one call (mirt_render_passes): the frame after the last of them, as n execute_render calls would leave it.
        fresh: the first of them starts the frame; then keep_acu False is enough where the passes resolve their own pixels.
        every_frame: the frame after EVERY pass as well (MIRT_PASSES_EVERY_FRAME), into n-frame buffers this renderer owns; returns them as
        (n, npix, 4) uint8 pixels and float32 radiance sums (None without want_radiance).  self.pixel / self.radiance hold the last frame."""
        if not self.nrays:
            self.passes += n
            return (np.zeros((n, 0, 4), np.uint8), None if self.radiance is None else np.zeros((n, 0, 4), np.float32)) if every_frame else None
        return self._passes(n, bounces, every_frame, lambda d: self.ctx.render_passes(d, n, fresh=fresh, every_frame=every_frame))

    def _passes(self, n, bounces, every_frame, call):
        """the body of execute_passes and execute_passes_guided: call(desc) runs the n passes, into n-frame buffers with every_frame"""
        pixel, radiance = self.pixel, self.radiance
        if every_frame:
            pixel = self._frames("_frame_pixel", n * self.npix * 4)
            radiance = None if self.radiance is None else self._frames("_frame_radiance", n * self.npix * 16)
        call(self.dev.pass_desc(self.seeds, self.acu, pixel, radiance, pass_index=self.passes, bounces=bounces, row0=self.row0, nrows=self.nrows))
        self.passes += n
        if not every_frame:
            return None
        pix = pixel.read(np.uint8, count=n * self.npix * 4).reshape(n, self.npix, 4)
        self.pixel.write(pix[-1])
        rad = None
        if radiance is not None:
            rad = radiance.read(np.float32, count=n * self.npix * 4).reshape(n, self.npix, 4)
            self.radiance.write(rad[-1])
        return pix, rad

    def guides(self, rows=None):
        """First-hit guide buffers (mirt_render_guides) of this renderer's tile, or of rows = (row0, nrows) of the image: two float32 arrays
        [pixels, 4], normal_hits = (sum of the hit samples' normals, hits) and albedo_depth = (sum of their material colours, sum of their hit
        distances).  Seeds, accumulator and frame are not touched."""
        row0, nrows = (self.row0, self.nrows) if rows is None else rows
        npix = nrows * self.s.width
        if not npix:
            return np.zeros((0, 4), np.float32), np.zeros((0, 4), np.float32)
        nh, ad = self.ctx.buffer(npix * 16), self.ctx.buffer(npix * 16)
        try:
            d = self.dev.pass_desc(None, None, row0=row0, nrows=nrows)
            self.ctx.render_guides(d, nh, ad)
            return nh.read(np.float32).reshape(-1, 4), ad.read(np.float32).reshape(-1, 4)
        finally:
            nh.release()
            ad.release()

    def ao(self, samples=4, radius=float("inf"), bias=0.001, rows=None):
        """Ambient occlusion of the first hit (mirt_render_ao) of this renderer's tile, or of rows = (row0, nrows) of the image inside that
        tile: a uint32 array [pixels, 2] of {open, cast} -- per hit primary sample `samples` hemisphere rays of length `radius`, cast counts
        them and open those nothing blocks, so open / cast is the pixel's openness.  The AO rays draw from the renderer's seeds as they stand
        and do not advance them; accumulator and frame are not touched."""
        row0, nrows = (self.row0, self.nrows) if rows is None else rows
        npix = nrows * self.s.width
        if not npix:
            return np.zeros((0, 2), np.uint32)
        if row0 < self.row0 or row0 + nrows > self.row0 + self.nrows:
            raise mirt.MirtError(-1, f"FusedRenderer.ao: rows [{row0}, +{nrows}) lie outside the renderer's tile [{self.row0}, +{self.nrows}): it holds no seeds for them")
        out = self.ctx.buffer(npix * 8)
        seeds = self.seeds
        try:
            if (row0, nrows) != (self.row0, self.nrows):   # a tile's seeds are its own buffer from element 0 on: the rows' slice of the renderer's
                per_row = self.s.width * self.s.rpp
                seeds = self.ctx.buffer(nrows * per_row * 4)
                seeds.write(self.seeds.read(np.int32, count=nrows * per_row, offset=(row0 - self.row0) * per_row * 4))
            d = self.dev.pass_desc(seeds, None, row0=row0, nrows=nrows)
            self.ctx.render_ao(d, out, samples, radius, bias)
            return out.read(np.uint32).reshape(-1, 2)
        finally:
            out.release()
            if seeds is not self.seeds:
                seeds.release()

    def denoised(self, **params):
        """The a-trous-filtered frame (mirt_filter_atrous) of this renderer's current radiance: the guides of its tile (mirt_render_guides, as
        guides() renders them), then the filter, all on the device.  tone is 1 / (rays_per_pixel * passes rendered so far).  params:
        iterations, normal_power_log2, sigma_depth, sigma_colour, demodulate, structure (mirt.FILTER_DEFAULTS where left out).  Returns
        (pixel [pixels, 4] uint8, filtered [pixels, 4] float32, un-scaled like radiance).  A renderer of a row tile filters its tile alone: a
        tiled frame is gathered first and filtered whole (include/mirt.h)."""
        if self.radiance is None or self.passes < 2:
            raise mirt.MirtError(-1, "FusedRenderer.denoised: needs want_radiance and at least one rendered pass")
        if not self.npix:
            return np.zeros((0, 4), np.uint8), np.zeros((0, 4), np.float32)
        nh, ad = self.ctx.buffer(self.npix * 16), self.ctx.buffer(self.npix * 16)
        out, pix = self.ctx.buffer(self.npix * 16), self.ctx.buffer(self.npix * 4)
        try:
            self.ctx.render_guides(self.dev.pass_desc(None, None, row0=self.row0, nrows=self.nrows), nh, ad)
            tone = np.float32(1.0 / (self.s.rpp * (self.passes - 1)))
            self.ctx.filter_atrous(self.s.width, self.nrows, tone, self.radiance, nh, ad, filtered=out, pixel=pix, **params)
            return pix.read(np.uint8).reshape(-1, 4), out.read(np.float32).reshape(-1, 4)
        finally:
            for b in (nh, ad, out, pix):
                b.release()

    def execute_render_guided(self, bounces=5):
        """The frame's first pass and its first-hit guides in one call (mirt_render_first_pass_guided): execute_render(fresh=True) and guides()
        at once, into guide buffers this renderer then owns -- self.normal_hits, self.albedo_depth, float4 per pixel of the tile, on the
        device until release().  Returns them as two float32 arrays [pixels, 4]."""
        if self.passes != 1:
            raise mirt.MirtError(-1, "FusedRenderer.execute_render_guided: the frame's first pass only")
        if not self.nrays:
            self.passes += 1
            return np.zeros((0, 4), np.float32), np.zeros((0, 4), np.float32)
        self.normal_hits, self.albedo_depth = self._frames("normal_hits", self.npix * 16), self._frames("albedo_depth", self.npix * 16)
        d = self.dev.pass_desc(self.seeds, self.acu, self.pixel, self.radiance, pass_index=1, bounces=bounces, row0=self.row0, nrows=self.nrows)
        self.ctx.render_first_pass_guided(d, self.normal_hits, self.albedo_depth)
        self.passes += 1
        return (self.normal_hits.read(np.float32, count=4 * self.npix).reshape(-1, 4), self.albedo_depth.read(np.float32, count=4 * self.npix).reshape(-1, 4))

    def denoised_first_pass(self, bounces=5, **params):
        """execute_render_guided, then the a-trous filter of that one-pass frame (mirt_filter_atrous) guided by the buffers it wrote: what
        execute_render(fresh=True) and denoised() give, without the second trace of the primary rays.  params and the result as denoised()."""
        if self.radiance is None:
            raise mirt.MirtError(-1, "FusedRenderer.denoised_first_pass: needs want_radiance")
        self.execute_render_guided(bounces)
        if not self.npix:
            return np.zeros((0, 4), np.uint8), np.zeros((0, 4), np.float32)
        out, pix = self.ctx.buffer(self.npix * 16), self.ctx.buffer(self.npix * 4)
        try:
            tone = np.float32(1.0 / self.s.rpp)
            self.ctx.filter_atrous(self.s.width, self.nrows, tone, self.radiance, self.normal_hits, self.albedo_depth, filtered=out, pixel=pix, **params)
            return pix.read(np.uint8).reshape(-1, 4), out.read(np.float32).reshape(-1, 4)
        finally:
            out.release()
            pix.release()

    def execute_passes_guided(self, n, bounces=5, fresh=False, every_frame=False):
        """execute_passes(n, bounces, fresh, every_frame) and guides() in one call (mirt_render_passes_guided): the guides go into
        self.normal_hits / self.albedo_depth as in execute_render_guided, the frames where execute_passes puts them.  Returns what execute_passes
        returns (None, or with every_frame the n frames)."""
        if not self.nrays:
            return self.execute_passes(n, bounces, fresh, every_frame)
        self.normal_hits, self.albedo_depth = self._frames("normal_hits", self.npix * 16), self._frames("albedo_depth", self.npix * 16)
        return self._passes(n, bounces, every_frame, lambda d: self.ctx.render_passes_guided(d, n, fresh=fresh, every_frame=every_frame,
                                                                                               normal_hits=self.normal_hits, albedo_depth=self.albedo_depth))

    def denoised_passes(self, n, bounces=5, **params):
        """The frame's first n passes with their guides (execute_passes_guided, fresh), then the a-trous filter of that frame guided by the buffers
        the call wrote: what execute_passes(n, fresh=True) and denoised() give, without the second trace of the primary rays.  params and the
        result as denoised()."""
        if self.radiance is None:
            raise mirt.MirtError(-1, "FusedRenderer.denoised_passes: needs want_radiance")
        if self.passes != 1:
            raise mirt.MirtError(-1, "FusedRenderer.denoised_passes: the frame's first passes only")
        self.execute_passes_guided(n, bounces, fresh=True)
        if not self.npix:
            return np.zeros((0, 4), np.uint8), np.zeros((0, 4), np.float32)
        out, pix = self.ctx.buffer(self.npix * 16), self.ctx.buffer(self.npix * 4)
        try:
            tone = np.float32(1.0 / (self.s.rpp * (self.passes - 1)))
            self.ctx.filter_atrous(self.s.width, self.nrows, tone, self.radiance, self.normal_hits, self.albedo_depth, filtered=out, pixel=pix, **params)
            return pix.read(np.uint8).reshape(-1, 4), out.read(np.float32).reshape(-1, 4)
        finally:
            out.release()
            pix.release()

    def _frames(self, name, nbytes):
        """a frame buffer of at least nbytes, kept for the next call"""
        b = getattr(self, name, None)
        if b is None or b.nbytes < nbytes:
            if b is not None:
                b.release()
            b = self.ctx.buffer(nbytes)
            setattr(self, name, b)
        return b

    def release(self):
        for b in (self.seeds, self.acu, self.pixel, self.radiance, getattr(self, "_frame_pixel", None), getattr(self, "_frame_radiance", None),
                  getattr(self, "normal_hits", None), getattr(self, "albedo_depth", None)):
            if b:
                b.release()
        self.dev.release()


class UpscaledRenderer:
    """Shade at 1/factor resolution, output at full (mirt_upsample_guided): `scene` (a pyhost.scene.PackedScene) names the OUTPUT size W x H and
    the rays per LOW pixel.  A FusedRenderer traces the same camera at (W / factor) x (H / factor) -- the camera's window is given in scene space,
    so the frustum is the same -- and render() runs, all on the device: the passes, the low guides, optionally the a-trous filter of the low
    frame, the guides at W x H, the upsampler.  The buffers of the last render() stay on the device for a caller that wants to read them:
    lo.radiance, filtered (None without denoise), nh_lo / ad_lo, nh / ad, upsampled, pixel.  Whole frames only: no row tiles."""

    def __init__(self, ctx, scene, factor, seeds=None, seed_base=0):
        factor = int(factor)
        if factor < 2 or factor > 4 or scene.width % factor or scene.height % factor:
            raise mirt.MirtError(-1, f"UpscaledRenderer: {scene.width}x{scene.height} is not a multiple of a factor {factor} in 2 .. 4")
        self.ctx, self.s, self.factor = ctx, scene, factor
        self.wl, self.hl = scene.width // factor, scene.height // factor
        self.lo = FusedRenderer(ctx, scene.resized(self.wl, self.hl, scene.rpp), seeds=seeds, seed_base=seed_base)
        nlo, n = self.wl * self.hl, scene.width * scene.height
        self.nh_lo, self.ad_lo, self.filtered = ctx.buffer(nlo * 16), ctx.buffer(nlo * 16), None
        self.nh, self.ad = ctx.buffer(n * 16), ctx.buffer(n * 16)
        self.upsampled, self.pixel = ctx.buffer(n * 16), ctx.buffer(n * 4)
        self.tone = None

    def guides_desc(self):
        """the low renderer's scene on the device, seen through the camera pack of the output size: what mirt_render_guides reads"""
        d = self.lo.dev.pass_desc(None, None)
        d.width, d.height = self.s.width, self.s.height
        d.cam = mirt._f(self.s.cam, 16)
        return d

    def render(self, passes=1, bounces=5, denoise=True, filter_params=None, **params):
        """-> (pixel [W * H, 4] uint8, upsampled [W * H, 4] float32, un-scaled like radiance).  passes: progressive passes of the low frame, added
        to those already rendered; denoise: filter the low frame first (filter_params: mirt.FILTER_DEFAULTS where left out); params:
        normal_power_log2, sigma_depth, demodulate of the upsampler (mirt.UPSAMPLE_DEFAULTS where left out)."""
        ctx, lo = self.ctx, self.lo
        if int(passes) == 1 and lo.passes == 1:   # exactly the frame's first pass: it writes the low guides itself (mirt_render_first_pass_guided)
            ctx.render_first_pass_guided(lo.dev.pass_desc(lo.seeds, lo.acu, lo.pixel, lo.radiance, pass_index=1, bounces=bounces), self.nh_lo, self.ad_lo)
            lo.passes += 1
            self.tone = np.float32(1.0 / lo.s.rpp)
        elif int(passes) > 1:   # several passes: one call runs them and writes the low guides (mirt_render_passes_guided)
            # a call runs at most mirt.MAX_PASSES_PER_CALL passes: more are split into calls of that many on the accumulator the low renderer keeps
            # (the frame is the same), and the first call writes the guides -- they are the same for every pass of a frame
            left, guides = int(passes), dict(normal_hits=self.nh_lo, albedo_depth=self.ad_lo)
            while left:
                k = min(left, mirt.MAX_PASSES_PER_CALL)
                d = lo.dev.pass_desc(lo.seeds, lo.acu, lo.pixel, lo.radiance, pass_index=lo.passes, bounces=bounces)
                if guides:
                    ctx.render_passes_guided(d, k, fresh=(lo.passes == 1), **guides)
                else:
                    ctx.render_passes(d, k)
                lo.passes += k
                left -= k
                guides = None
            self.tone = np.float32(1.0 / (lo.s.rpp * (lo.passes - 1)))
        else:
            for _ in range(int(passes)):
                lo.execute_render(bounces, fresh=(lo.passes == 1))
            self.tone = np.float32(1.0 / (lo.s.rpp * (lo.passes - 1)))
            ctx.render_guides(lo.dev.pass_desc(None, None), self.nh_lo, self.ad_lo)
        radiance = lo.radiance
        if denoise:
            if self.filtered is None:
                self.filtered = ctx.buffer(self.wl * self.hl * 16)
            ctx.filter_atrous(self.wl, self.hl, self.tone, lo.radiance, self.nh_lo, self.ad_lo, filtered=self.filtered, **(filter_params or {}))
            radiance = self.filtered
        ctx.render_guides(self.guides_desc(), self.nh, self.ad)
        ctx.upsample_guided(self.s.width, self.s.height, self.factor, self.tone, radiance, self.nh_lo, self.ad_lo, self.nh, self.ad,
                            upsampled=self.upsampled, pixel=self.pixel, **params)
        return self.pixel.read(np.uint8).reshape(-1, 4), self.upsampled.read(np.float32).reshape(-1, 4)

    def release(self):
        for b in (self.nh_lo, self.ad_lo, self.filtered, self.nh, self.ad, self.upsampled, self.pixel):
            if b:
                b.release()
        self.lo.release()


def _tile_passes_guided(fr, passes, bounces):
    """The first `passes` passes of a tile renderer's frame with the tile's guides (fr.normal_hits / fr.albedo_depth), all queued on the tile's
    context and nothing read back: mirt_render_first_pass_guided for one pass, mirt_render_passes_guided for several."""
    passes = int(passes)
    if not fr.nrays:
        fr.passes += passes
        return
    fr.normal_hits, fr.albedo_depth = fr._frames("normal_hits", fr.npix * 16), fr._frames("albedo_depth", fr.npix * 16)
    desc = lambda: fr.dev.pass_desc(fr.seeds, fr.acu, fr.pixel, fr.radiance, pass_index=fr.passes, bounces=bounces, row0=fr.row0, nrows=fr.nrows)
    if passes == 1:
        fr.ctx.render_first_pass_guided(desc(), fr.normal_hits, fr.albedo_depth)
        fr.passes += 1
        return
    left, guides = passes, dict(normal_hits=fr.normal_hits, albedo_depth=fr.albedo_depth)
    while left:   # a call runs at most mirt.MAX_PASSES_PER_CALL passes; the first call writes the guides, the same for every pass of a frame
        k = min(left, mirt.MAX_PASSES_PER_CALL)
        if guides:
            fr.ctx.render_passes_guided(desc(), k, fresh=True, **guides)
        else:
            fr.ctx.render_passes(desc(), k)
        fr.passes += k
        left -= k
        guides = None


class TiledPostRenderer:
    """The post-process chain in row tiles over the contexts of a mirt.DeviceGroup: every context renders its rows, exchanges halo rows with its
    neighbours (mirt_exchange_rows) and filters / upsamples where it is (mirt_filter_atrous_rows, mirt_upsample_guided_rows); only the finished
    rows are gathered.  The frames are, bit for bit, those of FusedRenderer.denoised_first_pass / denoised_passes and UpscaledRenderer.render on
    one context.  `scene` (a pyhost.scene.PackedScene) names the output size; seeds as FusedRenderer takes them (the array of the frame that is
    traced -- the LOW frame for upscaled -- or a seed_base for mirt_seed_fill at each tile's first global ray)."""

    def __init__(self, group, scene, seeds=None, seed_base=0, root=0):
        self.g, self.s, self.seeds, self.seed_base, self.root = group, scene, seeds, seed_base, root
        self.n = len(group.contexts)

    def _tiles(self, scene):
        return [FusedRenderer(c, scene, seeds=self.seeds, seed_base=self.seed_base, row0=r0, nrows=nr)
                for c, (r0, nr) in zip(self.g.contexts, (self.g.tile_rows(scene.height, i) for i in range(self.n)))]

    def _exchange(self, bufs, src, own, want, row_bytes):
        """one exchange per source buffer list in src: -> per list, the window buffers (None where a context wants nothing)"""
        out = []
        for tiles in src:
            dst = [c.buffer(nr * row_bytes) if nr else None for c, (_, nr) in zip(self.g.contexts, want)]
            bufs += [b for b in dst if b]
            self.g.exchange_rows([t if nr else None for t, (_, nr) in zip(tiles, own)], own, dst, want, row_bytes)
            out.append(dst)
        return out

    def _filter(self, bufs, trs, tone, want_pixel, params):
        """the tiles' frames filtered in place: -> (pixel tiles or None, filtered tiles), 16-byte stand-ins where a tile is empty"""
        s = trs[0].s
        iterations = mirt.FILTER_DEFAULTS["iterations"] if params.get("iterations") is None else params["iterations"]
        own = [(t.row0, t.nrows) for t in trs]
        want = [mirt.filter_window_rows(s.height, r0, nr, iterations) if nr else (0, 0) for r0, nr in own]
        rad, nh, ad = self._exchange(bufs, ([t.radiance for t in trs], [getattr(t, "normal_hits", None) for t in trs], [getattr(t, "albedo_depth", None) for t in trs]),
                                     own, want, s.width * 16)
        pix = [t.ctx.buffer(t.npix * 4 or 16) for t in trs] if want_pixel else None
        out = [t.ctx.buffer(t.npix * 16 or 16) for t in trs]
        bufs += out + (pix or [])
        for i, t in enumerate(trs):
            if t.nrows:
                t.ctx.filter_atrous_rows(s.width, s.height, want[i][0], want[i][1], t.row0, t.nrows, tone, rad[i], nh[i], ad[i], filtered=out[i],
                                         pixel=pix[i] if pix else None, **params)
        return pix, out

    def _gather(self, bufs, tiles, nbytes, dtype):
        ctx = self.g.contexts[self.root]
        out = ctx.buffer(sum(nbytes) or 16)
        bufs.append(out)
        self.g.gather(tiles, nbytes, out, root=self.root)
        ctx.finish()
        return out.read(dtype, count=sum(nbytes) // np.dtype(dtype).itemsize).reshape(-1, 4)

    def denoised(self, passes=1, bounces=5, want_filtered=True, **params):
        """-> (pixel [W * H, 4] uint8, filtered [W * H, 4] float32 or None): the a-trous-filtered frame after `passes` passes, params as
        Context.filter_atrous.  Into the root go 4 B per pixel (20 with want_filtered), not radiance and both guides."""
        trs, bufs = self._tiles(self.s), []
        try:
            for t in trs:
                _tile_passes_guided(t, passes, bounces)
            tone = np.float32(1.0 / (self.s.rpp * int(passes)))
            pix, out = self._filter(bufs, trs, tone, True, params)
            pixel = self._gather(bufs, pix, [t.npix * 4 for t in trs], np.uint8)
            filtered = self._gather(bufs, out, [t.npix * 16 for t in trs], np.float32) if want_filtered else None
            return pixel, filtered
        finally:
            self.g.finish()
            for b in bufs:
                b.release()
            for t in trs:
                t.release()

    def upscaled(self, factor, passes=1, bounces=5, denoise=True, filter_params=None, want_upsampled=True, **params):
        """-> (pixel [W * H, 4] uint8, upsampled [W * H, 4] float32 or None): the frame traced at (W / factor) x (H / factor) in row tiles of the LOW
        image, optionally filtered there, and rebuilt in row tiles of the output; arguments as UpscaledRenderer.render."""
        s, f = self.s, int(factor)
        if f < 2 or f > 4 or s.width % f or s.height % f:
            raise mirt.MirtError(-1, f"TiledPostRenderer: {s.width}x{s.height} is not a multiple of a factor {factor} in 2 .. 4")
        wl, hl = s.width // f, s.height // f
        trs, bufs = self._tiles(s.resized(wl, hl, s.rpp)), []
        try:
            for t in trs:
                _tile_passes_guided(t, passes, bounces)
            tone = np.float32(1.0 / (s.rpp * int(passes)))
            radiance = [t.radiance for t in trs]
            if denoise:
                radiance = self._filter(bufs, trs, tone, False, filter_params or {})[1]
            own = [(t.row0, t.nrows) for t in trs]
            high = [self.g.tile_rows(s.height, i) for i in range(self.n)]
            want = [mirt.upsample_low_rows(s.height, f, r0, nr) if nr else (0, 0) for r0, nr in high]
            rad, nhl, adl = self._exchange(bufs, (radiance, [getattr(t, "normal_hits", None) for t in trs], [getattr(t, "albedo_depth", None) for t in trs]),
                                           own, want, wl * 16)
            pix, ups = [], []
            for i, (t, (r0, nr)) in enumerate(zip(trs, high)):
                c = t.ctx
                pix.append(c.buffer(nr * s.width * 4 or 16))
                ups.append(c.buffer(nr * s.width * 16 or 16))
                if not nr:
                    continue
                nh, ad = c.buffer(nr * s.width * 16), c.buffer(nr * s.width * 16)
                bufs += [nh, ad]
                d = t.dev.pass_desc(None, None, row0=r0, nrows=nr)   # the tile's scene seen through the camera pack of the output size
                d.width, d.height = s.width, s.height
                d.cam = mirt._f(s.cam, 16)
                c.render_guides(d, nh, ad)
                c.upsample_guided_rows(s.width, s.height, f, r0, nr, want[i][0], want[i][1], tone, rad[i], nhl[i], adl[i], nh, ad,
                                       upsampled=ups[i], pixel=pix[i], **params)
            bufs += pix + ups
            pixel = self._gather(bufs, pix, [nr * s.width * 4 for _, nr in high], np.uint8)
            upsampled = self._gather(bufs, ups, [nr * s.width * 16 for _, nr in high], np.float32) if want_upsampled else None
            return pixel, upsampled
        finally:
            self.g.finish()
            for b in bufs:
                b.release()
            for t in trs:
                t.release()


class FramePacked:
    """Packed inputs of an Assign01 / 04 / 07 frame job (what `node host/cli.js pack-frame` emits)."""

    def __init__(self, d):
        self.assign, self.width, self.height = int(d["assign"]), int(d["width"]), int(d["height"])
        self.cam = np.asarray(d["cam"], np.float32)
        self.mol = "atoms" in d       # A07 molecule mode: parsePDB + splitMolData + molTrace (A07 code.js:569-600)
        self.both = None              # both models (`cli.js pack-frame 7 <mesh.json> <mol.pdb>`): the mesh job's fields, the molecule's packing under "mol"
        if isinstance(d.get("mol"), dict):
            m = d["mol"]
            self.both = dict(s_size=int(m["s_size"]), atoms=np.asarray(m["atoms"], np.float32), mindex=np.asarray(m["mindex"], np.uint32),
                             mcolor=np.asarray(m["mcolor"], np.float32), slab_size=np.asarray(m["slab_size"], np.uint32))
        if self.mol:
            self.bounds = np.asarray(d["bounds"], np.float32)
            self.s_size = int(d["s_size"])
            self.atoms = np.asarray(d["atoms"], np.float32)
            self.mindex, self.mcolor = np.asarray(d["mindex"], np.uint32), np.asarray(d["mcolor"], np.float32)
        elif self.assign != 1:
            self.bounds = np.asarray(d["bounds"], np.float32)
            self.t_size = int(d["t_size"])
            self.pos, self.normal = np.asarray(d["pos"], np.float32), np.asarray(d["normal"], np.float32)
            self.mindex, self.mcolor = np.asarray(d["mindex"], np.uint32), np.asarray(d["mcolor"], np.float32)
        if self.assign == 7:
            self.n_slabs, self.slab_size = int(d["n_slabs"]), np.asarray(d["slab_size"], np.uint32)


def render_frame(ctx, p, timing=None):
    """compute() of A01 (code.js:166-269) / computeTri() of A04 (code.js:553-577) and A07 (code.js:603-628) over the C ABI:
    same kernels, argument indices and NDRange.  Returns (pixels [H*W,4] uint8, rays bytes or None).
    timing: a dict that receives "trace_ms", the HIP-event time of the frame's trace kernel alone (raytrace / meshTrace / molTrace)."""
    def timed(k, gws, l):
        if timing is None:
            return k.enqueue(gws, l)
        ctx.finish()
        ctx.timer_start()
        k.enqueue(gws, l)
        timing["trace_ms"] = ctx.timer_stop_ms()

    pre = {1: "A01:", 4: "A04:", 7: "A07:"}[p.assign]
    w, h = p.width, p.height
    l = get_local_ws(2, 64)
    gws = [-(-w // l[0]) * l[0], -(-h // l[1]) * l[1]]
    pixels = ctx.buffer(w * h * 4, mirt.MEM_WRITE_ONLY)
    keep = [pixels]
    try:
        if p.assign == 1:
            k = ctx.kernel(pre + "raytrace").set_args(pixels, p.cam)
            timed(k, gws, l)
            k.release()
            return pixels.read(np.uint8).reshape(-1, 4), None
        k = ctx.kernel(pre + "sizeofRay")
        tmp = ctx.buffer(4)
        k.set_arg(0, tmp).enqueue([1], [1])
        ray_size = int(tmp.read(np.uint32, 1)[0])
        tmp.release(); k.release()
        rays = ctx.buffer(w * h * ray_size)
        up = lambda a: keep.append(ctx.buffer_from(a)) or keep[-1]
        keep.append(rays)
        it = ctx.kernel(pre + "initTrace").set_args(pixels, p.cam, rays)
        if p.assign == 7:
            it.set_arg(3, p.bounds)
        if p.mol:   # prepareMolTrace / executeMolTrace (A07 code.js:434-470, 549-552): ten arguments, s_mindex / m_color bound but unread
            mt = ctx.kernel(pre + "molTrace").set_args(pixels, p.cam, rays, _u32(p.s_size), up(p.atoms), up(p.mindex), up(p.mcolor), p.bounds,
                                                       _u32(p.n_slabs), up(p.slab_size))
            it.enqueue(gws, l)
            timed(mt, gws, l)
            ctx.finish()
            it.release(); mt.release()
            return pixels.read(np.uint8).reshape(-1, 4), rays.read(np.uint8)
        mt = ctx.kernel(pre + "meshTrace").set_args(pixels, p.cam, rays, _u32(p.t_size), up(p.pos), up(p.normal), up(p.mindex), up(p.mcolor))
        if p.assign == 7:
            mt.set_arg(8, p.bounds).set_arg(9, _u32(p.n_slabs)).set_arg(10, up(p.slab_size))
        it.enqueue(gws, l)
        timed(mt, gws, l)
        ctx.finish()
        it.release(); mt.release()
        return pixels.read(np.uint8).reshape(-1, 4), rays.read(np.uint8)
    finally:
        for b in keep:
            b.release()


def render_frame_stream(ctx, p, rays_fill=None):
    """render_frame's enqueue stream for every Assign04 / Assign07 job, the both-models one included -- initTrace, molTrace (a molecule, or
    p.both), meshTrace (a mesh) -- with nothing between the enqueues, as the pages issue a frame (A07 code.js:659-661).  rays_fill: a byte the ray
    buffer is filled with first.  Returns (pixels [H*W,4] uint8, rays bytes)."""
    pre = {4: "A04:", 7: "A07:"}[p.assign]
    w, h = p.width, p.height
    l = get_local_ws(2, 64)
    gws = [-(-w // l[0]) * l[0], -(-h // l[1]) * l[1]]
    keep, ks = [], []
    up = lambda a: keep.append(ctx.buffer_from(a)) or keep[-1]
    try:
        pixels = ctx.buffer(w * h * 4, mirt.MEM_WRITE_ONLY)
        keep.append(pixels)
        rays = ctx.buffer(w * h * RAY_BYTES)
        keep.append(rays)
        if rays_fill is not None:
            rays.write(np.full(w * h * RAY_BYTES, rays_fill, np.uint8))
        it = ctx.kernel(pre + "initTrace").set_args(pixels, p.cam, rays)
        ks.append(it)
        if p.assign == 7:
            it.set_arg(3, p.bounds)
        stages = []
        mol = dict(s_size=p.s_size, atoms=p.atoms, mindex=p.mindex, mcolor=p.mcolor, slab_size=p.slab_size) if p.mol else p.both
        if mol:
            stages.append(ctx.kernel(pre + "molTrace").set_args(pixels, p.cam, rays, _u32(mol["s_size"]), up(mol["atoms"]), up(mol["mindex"]), up(mol["mcolor"]),
                                                                 p.bounds, _u32(p.n_slabs), up(mol["slab_size"])))
        if not p.mol:
            mt = ctx.kernel(pre + "meshTrace").set_args(pixels, p.cam, rays, _u32(p.t_size), up(p.pos), up(p.normal), up(p.mindex), up(p.mcolor))
            if p.assign == 7:
                mt.set_arg(8, p.bounds).set_arg(9, _u32(p.n_slabs)).set_arg(10, up(p.slab_size))
            stages.append(mt)
        ks += stages
        it.enqueue(gws, l)
        for k in stages:
            k.enqueue(gws, l)
        ctx.finish()
        return pixels.read(np.uint8).reshape(-1, 4), rays.read(np.uint8)
    finally:
        for k in ks:
            k.release()
        for b in keep:
            b.release()


class FrameOneLaunch:
    """An Assign04 / Assign07 frame job uploaded once, rendered by mirt_render_frame: one launch per frame, no ray buffer unless keep_rays.
    aa > 1: by mirt_render_frame_aa, aa x aa samples a pixel averaged in that launch; the job and the pixel buffer stay p.width x p.height."""

    def __init__(self, ctx, p, keep_rays=False, aa=1):
        self.ctx, self.p, self.bufs, self.aa = ctx, p, [], aa
        up = lambda a: self.bufs.append(ctx.buffer_from(a)) or self.bufs[-1]
        self.pixels = ctx.buffer(p.width * p.height * 4, mirt.MEM_WRITE_ONLY)
        self.rays = ctx.buffer(p.width * p.height * RAY_BYTES) if keep_rays else None
        self.bufs += [b for b in (self.pixels, self.rays) if b]
        self.mesh = self.mol = None
        mol = dict(s_size=p.s_size, atoms=p.atoms, mindex=p.mindex, mcolor=p.mcolor, slab_size=p.slab_size) if p.mol else p.both
        if mol:
            self.mol = dict(s_size=mol["s_size"], atoms=up(mol["atoms"]), mindex=up(mol["mindex"]), mcolor=up(mol["mcolor"]), slab_size=up(mol["slab_size"]))
        if not p.mol:
            self.mesh = dict(t_size=p.t_size, pos=up(p.pos), normal=up(p.normal), mindex=up(p.mindex), mcolor=up(p.mcolor))
            if p.assign == 7:
                self.mesh["slab_size"] = up(p.slab_size)

    def render(self):
        p = self.p
        self.ctx.render_frame(p.assign, p.width, p.height, p.cam, self.pixels, bounds=getattr(p, "bounds", None), n_slabs=getattr(p, "n_slabs", 0),
                              mesh=self.mesh, mol=self.mol, rays=self.rays, aa=self.aa)

    def release(self):
        for b in self.bufs:
            b.release()
        self.bufs = []


def render_frame_one_launch(ctx, p, keep_rays=False, timing=None, aa=1):
    """The frame of render_frame (Assign04 / Assign07, the both-models job included) through mirt_render_frame: initTrace and the trace kernel(s) in
    one launch.  Returns (pixels [H*W,4] uint8, rays bytes or None); keep_rays: the kernel also stores every finished ray.
    timing: a dict that receives "frame_ms", the HIP-event time of the one launch.  aa: samples per axis and pixel (mirt_render_frame_aa)."""
    f = FrameOneLaunch(ctx, p, keep_rays, aa)
    try:
        if timing is None:
            f.render()
        else:
            ctx.finish()
            ctx.timer_start()
            f.render()
            timing["frame_ms"] = ctx.timer_stop_ms()
        return f.pixels.read(np.uint8).reshape(-1, 4), (f.rays.read(np.uint8) if keep_rays else None)
    finally:
        f.release()


def frame_resized(d, w, h):
    """The same frame job at another size: Camera.set (A07 code.js:55-71) makes width = height * cols / rows; cols, rows ride in .sE / .sF."""
    d = dict(d, width=w, height=h)
    cam = list(d["cam"])
    cam[12] = float(np.float32(cam[13] * (w / h)))
    cam[14], cam[15] = float(w), float(h)
    d["cam"] = cam
    return d


def frame_regrid(ctx, a07_job, a04_job, n):
    """The Assign07 job of a mesh at another n_slabs, binned ON THE DEVICE (mirt_grid_build + gathers = splitMeshData, A07 code.js:631-767):
    the mesh's triangles in input order come from its Assign04 job (one slot per triangle), the bounds from the Assign07 job."""
    tri = np.asarray(a04_job["pos"], np.float32).reshape(-1, 3, 4)[:, :, :3].reshape(-1, 9).astype(np.float64)
    nor = np.asarray(a04_job["normal"], np.float32).reshape(-1, 3, 4)[:, :, :3].reshape(-1, 9).astype(np.float64)
    b = np.asarray(a07_job["bounds"], np.float64)
    off, order, total = ctx.grid_build(1, tri, [b[0], b[1], b[2], b[4], b[5], b[6]], n)
    pos, nrm = ctx.grid_gather_triangles(order, total, tri, nor, pad_w=0.0)
    mi = ctx.grid_gather_u32(order, total, np.asarray(a04_job["mindex"], np.uint32))
    out = dict(a07_job, n_slabs=n, slab_size=off.read(np.uint32).tolist(), pos=pos.read(np.float32, total * 12).tolist(),
               normal=nrm.read(np.float32, total * 12).tolist(), mindex=mi.read(np.uint32, total).tolist())
    for buf in (off, order, pos, nrm, mi):
        buf.release()
    return out
