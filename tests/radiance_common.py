"""Shared by the radiance tests (mirt_trace_radiance): the definition of include/mirt.h restated with any checker `k` -- the CPU oracle, or through
mirt_enqueue the library's own kernel-by-kernel path -- and the buffers of one scene on one context.

The definition is executeRender (a10_pass.run_pass) without initTrace and copyToPixel.  Per sample: a Ray buffer filled from the caller's rays
(rays_common._ray_buffer), a Poi buffer with matId = -1 and atte = 1 (as initTrace resets it), then the kernel calls of run_pass's closest(), its
lightRender loop (not with MIRT_RADIANCE_NO_EMITTERS), its direct(), and `bounces` times bouncePaths, closest(), direct().  The seeds and the
accumulators are carried from one sample to the next.

Rays and scenes are the ray queries': rays_common.rays_of(stratum), 4133 rays in eight classes, on rays_common.scene(stratum); seeds:
a10_pass.make_seeds(n)."""
import numpy as np

import a10_pass as A
import rays_common as R

ACCUMULATE, NO_EMITTERS, MAX_SAMPLES = 1, 2, 64   # MIRT_RADIANCE_* (include/mirt.h)
SENTINEL = 0xA7

_EXPECTED = {}


def expected_radiance(sc, rays, seeds, samples, bounces, acu=None, emitters=True, k=None, watch=None):
    """-> (radiance float32 [n, 4], seeds int32 [n]): the accumulators and seeds the kernel sequence leaves.  acu: the accumulators to go on from.
    watch: optional callable, called as watch("rays", ray buffer) with the caller's rays before the first closest() of a sample and after every
    bouncePaths, and as watch("shadow", shadow buffer) after every initShadowTrace (a10_pass.run_pass's `watch`: every ray the sequence makes,
    before anything traces it; the buffers are a10_pass.RAY_DT records, the first n of them the caller's).  It changes no result."""
    k = k or A.load_oracle()
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    n = len(rays)
    rb0, g1 = R._ray_buffer(rays)
    B = k.buf
    acc = np.zeros((g1, 4), np.float32)
    if acu is not None:
        acc[:n] = acu
    sd = np.zeros(g1, np.int32)
    sd[:n] = seeds
    shadow = np.zeros(g1, A.RAY_DT)

    def seen(kind, buf):
        if watch is not None:
            k.flush()
            watch(kind, buf)

    for _ in range(samples):
        rb = rb0.copy()
        pb = np.zeros(g1, A.POI_DT)
        pb["matId"] = -1
        pb["atte"] = 1.0

        def closest():
            for call in R._closest_stages(k, sc, n, rb, pb, g1):
                call()

        def direct():
            for l in sc.lights:
                p, _k = A._f(l["shadow"])
                k.initShadowTrace(B(shadow), B(pb), n, p, B(sd), g1)
                seen("shadow", shadow)
                if sc.has_spheres:
                    p, _k = A._f(sc.sphere_bounds)
                    k.sphereShadowTrace(n, B(shadow), B(sc.spheres), B(sc.s_box), p, sc.n_slabs, g1)
                if sc.has_triangles:
                    p, _k = A._f(sc.triangle_bounds)
                    k.triangleShadowTrace(n, B(shadow), B(sc.t_pos), B(sc.t_box), p, sc.n_slabs, g1)
                for m in sc.meshes:
                    p, _k = A._f(m["bounds"])
                    k.triangleShadowTrace(n, B(shadow), B(m["pos"]), B(m["box"]), p, m["nslabs"], g1)
                p, _k = A._f(l["scene"])
                k.sceneRender(B(acc), B(pb), B(shadow), B(sc.materials), p, n, g1)

        seen("rays", rb)
        closest()
        if emitters:
            for l in sc.lights:
                p, _k = A._f(l["light"])
                k.lightRender(B(pb), B(rb), B(acc), p, n, g1)
        direct()
        for _j in range(bounces):
            k.bouncePaths(B(pb), B(rb), B(sd), n, g1)
            seen("rays", rb)
            closest()
            direct()
        k.flush()
    return acc[:n].copy(), sd[:n].copy()


def seeds_of(stratum):
    return A.make_seeds(len(R.rays_of(stratum)[0]))


def radiance_of(stratum, samples, bounces):
    """the oracle's answer for the stratum's rays with make_seeds' seeds, computed once and shared"""
    key = (stratum, samples, bounces)
    if key not in _EXPECTED:
        out = expected_radiance(R.scene(stratum), R.rays_of(stratum)[0], seeds_of(stratum), samples, bounces)
        for a in out:
            a.setflags(write=False)
        _EXPECTED[key] = out
    return _EXPECTED[key]


def camera_rays(sc, seeds, bounces=5, k=None):
    """-> (rays float32 [n, 8] as initTrace stores them, the PassState a10_pass.run_pass leaves): the camera's own rays of a fixture scene"""
    k = k or A.load_oracle()
    st = A.PassState(sc, seeds)
    got = {}

    def watch(kind, rays):
        if kind == "rays" and "r" not in got:
            got["r"] = rays.copy()
    A.run_pass(k, sc, st, bounces=bounces, watch=watch)
    return pack_rays(got["r"], sc.total_rays), st


def pack_rays(ray_buffer, n):
    """48-byte Ray records (a10_pass.RAY_DT) -> the 32-byte records of the ABI"""
    r = ray_buffer
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = r["o"][:n], r["mint"][:n], r["d"][:n], r["maxt"][:n]
    return rays


def light_intercepts(sc, rays, k=None):
    """bool [n]: lightRender of some light fires on the ray after the closest-hit stage (the accumulator's w goes up)"""
    k = k or A.load_oracle()
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    n = len(rays)
    rb, g1 = R._ray_buffer(rays)
    pb = np.zeros(g1, A.POI_DT)
    pb["matId"] = -1
    pb["atte"] = 1.0
    acc = np.zeros((g1, 4), np.float32)
    for call in R._closest_stages(k, sc, n, rb, pb, g1):
        call()
    for l in sc.lights:
        p, _k = A._f(l["light"])
        k.lightRender(k.buf(pb), k.buf(rb), k.buf(acc), p, n, g1)
    k.flush()
    return acc[:n, 3] > 0


# ---- the library ----------------------------------------------------------------------------------------------------------------------------
class RadianceTracer:
    """one scene on one context, with a ray buffer and seeds / radiance buffers of `cap` rays each followed by `tail` sentinel bytes"""

    def __init__(self, ctx, sc, cap=R.N_RAYS, tail=64):
        from raytracing_amd.pyhost import mirt
        self.ctx, self.cap, self.tail = ctx, cap, tail
        self.dev = mirt.DeviceScene(ctx, sc)
        self.rays = ctx.buffer(max(cap * 32, 16))
        self.seeds, self.radiance = ctx.buffer(cap * 4 + tail), ctx.buffer(cap * 16 + tail)

    def desc(self, bounces):
        return self.dev.pass_desc(None, None, bounces=bounces)

    def run(self, rays, seeds, samples=1, bounces=5, flags=0, acu=None):
        """-> (radiance [n, 4], seeds [n], (the bytes behind the n seeds, those behind the n accumulators))"""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        n = len(rays)
        s = np.full(self.seeds.nbytes, SENTINEL, np.uint8)
        s[:n * 4] = np.ascontiguousarray(seeds, np.int32).view(np.uint8)
        a = np.full(self.radiance.nbytes, SENTINEL, np.uint8)
        if acu is not None:
            a[:n * 16] = np.ascontiguousarray(acu, np.float32).reshape(-1).view(np.uint8)
        self.seeds.write(s)
        self.radiance.write(a)
        if n:
            self.rays.write(rays)
        self.ctx.trace_radiance(self.desc(bounces), self.rays, n, self.seeds, self.radiance, samples=samples, flags=flags)
        s, a = self.seeds.read(np.uint8), self.radiance.read(np.uint8)
        return a[:n * 16].view(np.float32).reshape(-1, 4).copy(), s[:n * 4].view(np.int32).copy(), (s[n * 4:], a[n * 16:])

    def release(self):
        for b in (self.rays, self.seeds, self.radiance):
            b.release()
        self.dev.release()


def untouched(tail):
    return bool((np.asarray(tail) == SENTINEL).all())


def differ(tag, got, want):
    """(radiance, seeds) pairs: None when equal bit for bit (every NaN equal to every NaN), else a sentence"""
    from conftest import bits
    (ga, gs), (wa, ws) = got, want
    ga, wa = np.ascontiguousarray(ga, np.float32).reshape(-1, 4), np.ascontiguousarray(wa, np.float32).reshape(-1, 4)
    if ga.shape != wa.shape or len(gs) != len(ws):
        return f"{tag}: {len(ga)} accumulators and {len(gs)} seeds against {len(wa)} and {len(ws)}"
    bad = np.flatnonzero((bits(ga) != bits(wa)).any(axis=1))
    if bad.size:
        i = int(bad[0])
        return f"{tag}: {bad.size} of {len(ga)} accumulators differ; first is ray {i}: got {ga[i].tolist()}, want {wa[i].tolist()}"
    bad = np.flatnonzero(np.asarray(gs) != np.asarray(ws))
    if bad.size:
        i = int(bad[0])
        return f"{tag}: {bad.size} of {len(gs)} seeds differ; first is ray {i}: got {int(gs[i])}, want {int(ws[i])}"
    return None


def kernel_by_kernel(ctx, dev, sc, rays, seeds, samples, bounces, acu=None, emitters=True):
    """The library's own kernel-by-kernel path on the same rays, extending rays_common.kernel_by_kernel: 48-byte Ray / 64-byte Poi buffers filled
    here per sample, then the mirt_enqueue sequence GranularRenderer._closest, its lightRender loop, ._direct and bouncePaths issue.  dev: a
    mirt.DeviceScene of `ctx`.  -> (radiance [n, 4], seeds [n])"""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    n = len(rays)
    rb, g1 = R._ray_buffer(rays)
    pb = np.zeros(g1, A.POI_DT)
    pb["matId"] = -1
    pb["atte"] = 1.0
    acc = np.zeros((g1, 4), np.float32)
    if acu is not None:
        acc[:n] = acu
    sd = np.zeros(g1, np.int32)
    sd[:n] = seeds
    u32 = lambda v: np.array([v], np.uint32)
    rbuf, pbuf, sbuf = ctx.buffer(rb.nbytes), ctx.buffer(pb.nbytes), ctx.buffer(rb.nbytes).write(np.zeros(g1, A.RAY_DT))
    abuf, dbuf = ctx.buffer(acc.nbytes).write(acc), ctx.buffer(sd.nbytes).write(sd)
    ks = []

    def kernel(name, *args):
        k = ctx.kernel(name).set_args(*args)
        ks.append(k)
        return k
    try:
        closest, shadows = [], []
        if sc.has_spheres:
            closest.append(kernel("sphereTrace", u32(n), pbuf, rbuf, dev.sph["prims"], dev.sph["matid"], dev.sph["off"], sc.sphere_bounds, u32(sc.n_slabs)))
            shadows.append(kernel("sphereShadowTrace", u32(n), sbuf, dev.sph["prims"], dev.sph["off"], sc.sphere_bounds, u32(sc.n_slabs)))
        if sc.has_triangles:
            closest.append(kernel("triangleTrace", u32(n), pbuf, rbuf, dev.tri["prims"], dev.tri["normals"], dev.tri["matid"], dev.tri["off"],
                                  sc.triangle_bounds, u32(sc.n_slabs)))
            shadows.append(kernel("triangleShadowTrace", u32(n), sbuf, dev.tri["prims"], dev.tri["off"], sc.triangle_bounds, u32(sc.n_slabs)))
        for m in dev.meshes:
            closest.append(kernel("meshTrace", u32(n), pbuf, rbuf, m["prims"], m["normals"], m["off"], u32(m["matid"]), m["bounds"], u32(m["n"])))
            shadows.append(kernel("triangleShadowTrace", u32(n), sbuf, m["prims"], m["off"], m["bounds"], u32(m["n"])))
        init_shadow = [kernel("initShadowTrace", sbuf, pbuf, u32(n), l["shadow"], dbuf) for l in sc.lights]
        scene_render = [kernel("sceneRender", abuf, pbuf, sbuf, dev.material, l["scene"], u32(n)) for l in sc.lights]
        light_render = [kernel("lightRender", pbuf, rbuf, abuf, l["light"], u32(n)) for l in sc.lights]
        bounce = kernel("bouncePaths", pbuf, rbuf, dbuf, u32(n))

        def go(k):
            k.enqueue([g1], [64])

        def direct():
            for i in range(len(sc.lights)):
                go(init_shadow[i])
                for k in shadows:
                    go(k)
                go(scene_render[i])

        for _ in range(samples):
            rbuf.write(rb)
            pbuf.write(pb)
            for k in closest:
                go(k)
            if emitters:
                for k in light_render:
                    go(k)
            direct()
            for _j in range(bounces):
                go(bounce)
                for k in closest:
                    go(k)
                direct()
        ctx.finish()
        return abuf.read(np.float32).reshape(-1, 4)[:n].copy(), dbuf.read(np.int32)[:n].copy()
    finally:
        for k in ks:
            k.release()
        for b in (rbuf, pbuf, sbuf, abuf, dbuf):
            b.release()
