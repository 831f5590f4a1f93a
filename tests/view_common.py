"""Shared by the view-camera tests (mirt_view_rays, mirt_render_view): the ray definition of include/mirt.h restated in numpy, and the frame it
defines through the CPU oracle.

The restatement is fp32 arrays all the way: numpy's `+ - *` on float32 are single IEEE operations, its `/` and sqrt on float32 are correctly
rounded (what div_cr and sqrt_cr are), and sin / cos come element-wise from the oracle's oracle_bi_sin / oracle_bi_cos, the contract's own
(tests/test_gpu_numerics.py binds them the same way).  Nothing is fused: every operation below is one numpy call on float32 operands.

expected_view: the restated rays, then radiance_common.expected_radiance at one sample per ray, then the sequential fp32 fold over a pixel's
samples (copyToPixel's order) from +0 or from `carry`, then copyToPixel's tone map."""
import ctypes as C

import numpy as np

import a10_pass as A
import radiance_common as RC

f32 = np.float32
ORTHOGRAPHIC, EQUIRECT, FISHEYE = 0, 1, 2   # MIRT_VIEW_* (include/mirt.h)
ACCUMULATE = 1
MODELS = {"ortho": ORTHOGRAPHIC, "equirect": EQUIRECT, "fisheye": FISHEYE}
KS = (1, 2, 4, 8, 16)
PI = f32(float.fromhex("0x1.921fb6p+1"))
HALF_PI = f32(float.fromhex("0x1.921fb6p+0"))
SENTINEL = 0xA7

_SINCOS = {}


def _trig():
    if "lib" not in _SINCOS:
        lib = A.load_oracle().lib
        for fn in (lib.oracle_bi_sin, lib.oracle_bi_cos):
            fn.restype = C.c_float
            fn.argtypes = [C.c_float]
        _SINCOS["lib"] = lib
    return _SINCOS["lib"]


def sincos(x):
    """element-wise (sin, cos) of a float32 array by the oracle's contract functions; equal arguments are computed once"""
    lib = _trig()
    x = np.ascontiguousarray(x, f32)
    u, inv = np.unique(x.view(np.uint32), return_inverse=True)
    s = np.array([lib.oracle_bi_sin(float(v)) for v in u.view(f32)], f32)
    c = np.array([lib.oracle_bi_cos(float(v)) for v in u.view(f32)], f32)
    return s[inv].reshape(x.shape), c[inv].reshape(x.shape)


class View:
    """the fields of a mirt_view_desc the definition reads, fp32"""

    def __init__(self, model, width, height, k, eye, right, up, forward, half_w=1.0, half_h=1.0, half_angle=float(HALF_PI), t_min=0.0,
                 t_max=float("inf"), tone=1.0, row0=0, nrows=0):
        self.model = MODELS[model] if isinstance(model, str) else int(model)
        self.width, self.height, self.k, self.row0, self.nrows = int(width), int(height), int(k), int(row0), int(nrows)
        self.eye, self.right, self.up, self.forward = (np.asarray(v, np.float64).astype(f32).reshape(3) for v in (eye, right, up, forward))
        self.half_w, self.half_h, self.half_angle, self.t_min, self.t_max, self.tone = (f32(v) for v in (half_w, half_h, half_angle, t_min, t_max, tone))

    @property
    def rows(self):
        return self.nrows or self.height

    @property
    def rpp(self):
        return self.k * self.k

    @property
    def n_pixels(self):
        return self.rows * self.width

    @property
    def n_rays(self):
        return self.n_pixels * self.rpp

    def tile(self, row0, nrows):
        v = View.__new__(View)
        v.__dict__.update(self.__dict__)
        v.row0, v.nrows = int(row0), int(nrows)
        return v

    def with_(self, **fields):
        v = View.__new__(View)
        v.__dict__.update(self.__dict__)
        for name, val in fields.items():
            setattr(v, name, f32(val) if isinstance(getattr(self, name), np.floating) else val)
        return v

    def desc(self, flags=0):
        """the ctypes mirt_view_desc"""
        from raytracing_amd.pyhost import mirt
        d = mirt._ViewDesc()
        d.struct_size = C.sizeof(mirt._ViewDesc)
        d.model, d.width, d.height, d.k, d.row0, d.nrows, d.flags = self.model, self.width, self.height, self.k, self.row0, self.nrows, int(flags)
        for name in ("eye", "right", "up", "forward"):
            setattr(d, name, (C.c_float * 3)(*(float(c) for c in getattr(self, name))))
        d.half_w, d.half_h, d.half_angle, d.t_min, d.t_max, d.tone = (float(x) for x in (self.half_w, self.half_h, self.half_angle, self.t_min, self.t_max, self.tone))
        return d


def standard_basis():
    """forward = normalize(0.3, -0.2, -1), right = normalize(forward x (0, 1, 0)), up = right x forward -- in double, narrowed once"""
    fwd = np.array([0.3, -0.2, -1.0])
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    return right, up, fwd


def standard_view(sc, model, width=13, height=7, k=2, **kw):
    """the standard inputs of the tests: eye at the centre of sc.bounds, the oblique basis, ORTHOGRAPHIC half extents 0.8 x the box's, FISHEYE pi / 2"""
    b = np.asarray(sc.bounds, np.float64)
    lo, hi = b[0:3], b[4:7]
    right, up, fwd = standard_basis()
    half = 0.8 * (hi - lo) / 2
    return View(model, width, height, k, (lo + hi) / 2, right, up, fwd, half_w=half[0], half_h=half[1], half_angle=float(HALF_PI), **kw)


def view_rays(v):
    """-> float32 [n_rays, 8]: the tile's rays (o.xyz, mint, d.xyz, maxt) in ray id order, ((y - row0) * width + x) * rpp + sy * k + sx"""
    k, W = v.k, v.width
    ys, xs, sy, sx = np.meshgrid(np.arange(v.row0, v.row0 + v.rows), np.arange(W), np.arange(k), np.arange(k), indexing="ij")
    ys, xs, sy, sx = (a.reshape(-1) for a in (ys, xs, sy, sx))
    ik = f32(1.0) / f32(k)
    fx = xs.astype(f32) + (sx.astype(f32) + f32(0.5)) * ik
    fy = ys.astype(f32) + (sy.astype(f32) + f32(0.5)) * ik
    u, w = fx / f32(W), fy / f32(v.height)
    a = (u + u) - f32(1.0)
    b = f32(1.0) - (w + w)
    n = len(a)
    rays = np.zeros((n, 8), f32)
    rays[:, 0:3] = v.eye
    rays[:, 3], rays[:, 7] = v.t_min, v.t_max

    def direction(lx, ly, lz):
        return np.stack([(v.right[c] * lx + v.up[c] * ly) + v.forward[c] * lz for c in range(3)], axis=1)

    if v.model == ORTHOGRAPHIC:
        ta, tb = a * v.half_w, b * v.half_h
        rays[:, 0:3] = np.stack([(v.eye[c] + v.right[c] * ta) + v.up[c] * tb for c in range(3)], axis=1)
        rays[:, 4:7] = v.forward
    elif v.model == EQUIRECT:
        sp, cp = sincos(a * PI)
        st, ct = sincos(b * HALF_PI)
        rays[:, 4:7] = direction(sp * ct, st, cp * ct)
    else:
        r = np.sqrt(a * a + b * b)
        assert r.dtype == f32
        livem = r <= f32(1.0)
        sa, ca = sincos(r * v.half_angle)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(r > 0, sa / r, f32(0.0)).astype(f32)
        rays[:, 4:7] = direction(a * q, b * q, ca)
        rays[~livem, 4:7] = v.forward
        rays[~livem, 3] = 0.0
        rays[~livem, 7] = 0.0
    assert rays.dtype == f32
    return rays


def fold(acc, rpp, carry=None):
    """per pixel, the sequential fp32 sum of its rpp accumulators, all four channels, from +0 or from carry"""
    a = np.ascontiguousarray(acc, f32).reshape(-1, rpp, 4)
    s = np.zeros((a.shape[0], 4), f32) if carry is None else np.array(carry, f32).reshape(-1, 4)
    for i in range(rpp):
        s = (s + a[:, i, :]).astype(f32)
    return s


def tone_rgba8(sums, tone):
    """copyToPixel's tone map (A10 code.cl:1381-1385): (c * (255 * m)) * 1.8 clamped to 0 .. 255, truncated, NaN -> 0; alpha 255"""
    sc = f32(255.0) * f32(tone)
    with np.errstate(invalid="ignore", over="ignore"):
        val = (np.asarray(sums, f32)[:, 0:3] * sc) * f32(1.8)
    val = np.where(np.isnan(val), f32(0), np.clip(val, f32(0), f32(255)))
    px = np.full((len(val), 4), 255, np.uint8)
    px[:, 0:3] = val.astype(np.uint8)
    return px


def expected_view(sc, view, seeds, bounces, carry=None):
    """-> (seeds int32 [n_rays], radiance float32 [n_pixels, 4], pixel uint8 [n_pixels, 4]) as mirt_render_view defines them"""
    acc, sd = RC.expected_radiance(sc, view_rays(view), seeds, 1, bounces)
    sums = fold(acc, view.rpp, carry)
    return sd, sums, tone_rgba8(sums, view.tone)


# ---- the library ------------------------------------------------------------------------------------------------------------------------------
class Renderer:
    """one scene on one context with seeds / radiance / pixel buffers of `cap_rays` / `cap_pixels` records, each followed by `tail` sentinel bytes"""

    def __init__(self, ctx, sc, cap_rays, cap_pixels, tail=64):
        from raytracing_amd.pyhost import mirt
        self.ctx, self.tail = ctx, tail
        self.dev = mirt.DeviceScene(ctx, sc)
        self.seeds = ctx.buffer(cap_rays * 4 + tail)
        self.radiance, self.pixel = ctx.buffer(cap_pixels * 16 + tail), ctx.buffer(cap_pixels * 4 + tail)

    def scene_desc(self, bounces):
        return self.dev.pass_desc(None, None, bounces=bounces)

    def run(self, view, seeds, bounces=2, carry=None, prefill=None, radiance=True, pixel=True):
        """-> (seeds, radiance or None, pixel or None, untouched: the bytes behind every record still hold the sentinel).  carry: the sums to go on
        from (sets MIRT_VIEW_ACCUMULATE); prefill: what radiance holds before a call WITHOUT the flag."""
        n, npx = view.n_rays, view.n_pixels
        s = np.full(self.seeds.nbytes, SENTINEL, np.uint8)
        s[:n * 4] = np.ascontiguousarray(seeds, np.int32).view(np.uint8)
        r = np.full(self.radiance.nbytes, SENTINEL, np.uint8)
        for pre in (carry, prefill):
            if pre is not None:
                r[:npx * 16] = np.ascontiguousarray(pre, f32).reshape(-1).view(np.uint8)
        self.seeds.write(s)
        self.radiance.write(r)
        self.pixel.write(np.full(self.pixel.nbytes, SENTINEL, np.uint8))
        self.ctx.render_view(self.scene_desc(bounces), view.desc(ACCUMULATE if carry is not None else 0), self.seeds,
                             self.radiance if radiance else None, self.pixel if pixel else None)
        s2, r2, p2 = self.seeds.read(np.uint8), self.radiance.read(np.uint8), self.pixel.read(np.uint8)
        clean = bool((s2[n * 4:] == SENTINEL).all() and (r2[npx * 16:] == SENTINEL).all() and (p2[npx * 4:] == SENTINEL).all())
        if not radiance:
            clean = clean and bool((r2 == r).all())
        if not pixel:
            clean = clean and bool((p2 == SENTINEL).all())
        return (s2[:n * 4].view(np.int32).copy(), r2[:npx * 16].view(f32).reshape(-1, 4).copy() if radiance else None,
                p2[:npx * 4].reshape(-1, 4).copy() if pixel else None, clean)

    def release(self):
        for b in (self.seeds, self.radiance, self.pixel):
            b.release()
        self.dev.release()


def differ(tag, got, want):
    """(seeds, radiance, pixel) triples: None when equal bit for bit (every NaN equal to every NaN; a None member is not compared), else a sentence"""
    from conftest import bits
    (gs, gr, gp), (ws, wr, wp) = got[:3], want[:3]
    if len(gs) != len(ws):
        return f"{tag}: {len(gs)} seeds against {len(ws)}"
    bad = np.flatnonzero(np.asarray(gs) != np.asarray(ws))
    if bad.size:
        i = int(bad[0])
        return f"{tag}: {bad.size} of {len(gs)} seeds differ; first is ray {i}: got {int(gs[i])}, want {int(ws[i])}"
    if gr is not None and wr is not None:
        bad = np.flatnonzero((bits(gr) != bits(wr)).any(axis=1))
        if bad.size:
            i = int(bad[0])
            return f"{tag}: {bad.size} of {len(gr)} radiance sums differ; first is pixel {i}: got {gr[i].tolist()}, want {wr[i].tolist()}"
    if gp is not None and wp is not None:
        bad = np.flatnonzero((np.asarray(gp) != np.asarray(wp)).any(axis=1))
        if bad.size:
            i = int(bad[0])
            return f"{tag}: {bad.size} of {len(gp)} pixels differ; first is pixel {i}: got {gp[i].tolist()}, want {wp[i].tolist()}"
    return None
