"""Shared by the tests of the batch's guides and ambient occlusion (mirt_view_guides_batch, mirt_render_view_guided_batch, mirt_view_ao_batch):
the definition by composition on the single-camera helpers, and the library side.

  expected_guides / expected_ao   the oracle's (view_guides_common.expected, view_ao_common.expected) per frame, concatenated -- computed once
                                  per input and shared read-only
  Aov                             one scene on one context: seeds / radiance / pixel / normal_hits / albedo_depth / ao_out for N frames, each
                                  followed by sentinel bytes; the batch calls on them, and the same library's N single calls on each slice
  mixed_cameras                   the three standard cameras with the middle one looking along -z: the ray-side guard refuses its every ray
  SHAPES                          the smallest shapes at which a per-pixel batch kernel can still go wrong (width, height, k, N)

Tolerance 0 throughout (conftest.bits)."""
import numpy as np

import a10_pass as A
import view_ao_common as VA
import view_batch_common as VB
import view_common as V
import view_guides_common as VG

f32 = np.float32
SENTINEL, TAIL = V.SENTINEL, 64
FIXTURES = VG.FIXTURES
MODELS = ("ortho", "equirect", "fisheye")
W, H, K, N, BOUNCES = 13, 7, 2, 3, 2
AO_SAMPLES, AO_RADIUS = 4, 1.0
# 45 pixels: one wave holds three frames | 273: a block border inside frame 2, a ragged last block of 17 | a frame is exactly one block |
# five frames in five lanes | a pixel is 256 samples
SHAPES = [(5, 3, 2, 3), (13, 7, 2, 3), (16, 16, 1, 2), (1, 1, 1, 5), (3, 1, 16, 2)]
OTHER_SHAPES = [s for s in SHAPES if s != (13, 7, 2, 3)]
CAP_PIXELS = max(w * h * n for w, h, _k, n in SHAPES)
CAP_RAYS = max([w * h * k * k * n for w, h, k, n in SHAPES] + [5 * 3 * 256 * 3])

_SCENES, _CACHE = {}, {}


def scene(name):
    if name not in _SCENES:
        from conftest import load_fixture
        _SCENES[name] = load_fixture(name)[1]
    return _SCENES[name]


def mixed_cameras(sc):
    cams = VB.cameras(sc, N)
    cams[1, 3:12] = (1, 0, 0, 0, 1, 0, 0, 0, -1)
    return cams


def _cached(key, make):
    if key not in _CACHE:
        out = make()
        for a in (out if isinstance(out, tuple) else (out,)):
            a.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def expected_guides(name, model, mixed=False):
    """the oracle's guides of the N frames at 13 x 7, k = 2: (normal_hits, albedo_depth), float32 [N * P, 4] each"""
    def make():
        sc = scene(name)
        v = V.standard_view(sc, model)
        parts = [VG.expected(sc, VB.frame_view(v, c)) for c in (mixed_cameras(sc) if mixed else VB.cameras(sc, N))]
        return tuple(np.concatenate([p[i] for p in parts], axis=0) for i in range(2))
    return _cached(("guides", name, model, mixed), make)


def expected_ao(name, model, mixed=False):
    """the oracle's AO pairs of the N frames at 13 x 7, k = 2, seeds make_seeds(N * R) sliced, with view_ao_common.expected's own parameters:
    view_ao_common.SAMPLES = 3 samples, radius 1, view_ao_common.BIAS -- at which every frame of every model has fully open pixels (at 4 samples
    frame 0 of the teapot fixture's ORTHOGRAPHIC batch has none)"""
    def make():
        sc = scene(name)
        v = V.standard_view(sc, model)
        seeds = A.make_seeds(N * v.n_rays)
        cams = mixed_cameras(sc) if mixed else VB.cameras(sc, N)
        return np.concatenate([VA.expected(sc, VB.frame_view(v, c), VA.SAMPLES, AO_RADIUS, VA.BIAS, seeds=seeds[f * v.n_rays:(f + 1) * v.n_rays])
                               for f, c in enumerate(cams)], axis=0)
    return _cached(("ao", name, model, mixed), make)


def guide_kinds(nh, rpp):
    """(full, partial, empty) pixel counts of a normal_hits array"""
    none, every, part = VG.kinds(nh, rpp)
    return every, part, none


def ao_kinds(ao):
    """(cast > 0, open < cast, open == cast > 0, {0, 0}) pixel counts of an AO array"""
    ao = np.asarray(ao)
    o, c = ao[:, 0], ao[:, 1]
    return int((c > 0).sum()), int((o < c).sum()), int(((o == c) & (c > 0)).sum()), int(((o == 0) & (c == 0)).sum())


class Aov:
    def __init__(self, ctx, sc, cap_rays=CAP_RAYS, cap_pixels=CAP_PIXELS, tail=TAIL):
        from raytracing_amd.pyhost import mirt
        self.ctx, self.sc = ctx, sc
        self.dev = mirt.DeviceScene(ctx, sc)
        self.seeds = ctx.buffer(cap_rays * 4 + tail)
        self.radiance, self.pixel = ctx.buffer(cap_pixels * 16 + tail), ctx.buffer(cap_pixels * 4 + tail)
        self.nh, self.ad = ctx.buffer(cap_pixels * 16 + tail), ctx.buffer(cap_pixels * 16 + tail)
        self.ao = ctx.buffer(cap_pixels * 8 + tail)

    def buffers(self):
        return (self.seeds, self.radiance, self.pixel, self.nh, self.ad, self.ao)

    def scene_desc(self, bounces=0):
        return self.dev.pass_desc(None, None, bounces=bounces)

    def release(self):
        for b in self.buffers():
            b.release()
        self.dev.release()

    # -- filling and reading: every buffer is the sentinel but the given records; `clean`: everything behind the records still is
    def _fill(self, seeds=None, carry=None):
        for b in self.buffers():
            raw = np.full(b.nbytes, SENTINEL, np.uint8)
            if b is self.seeds and seeds is not None:
                raw[:len(seeds) * 4] = np.ascontiguousarray(seeds, np.int32).view(np.uint8)
            if b is self.radiance and carry is not None:
                raw[:len(carry) * 16] = np.ascontiguousarray(carry, f32).reshape(-1).view(np.uint8)
            b.write(raw)

    def _read(self, buf, n, size, dtype, cols, given=True):
        raw = buf.read(np.uint8)
        if not given:
            return None, bool((raw == SENTINEL).all())
        return raw[:n * size].view(dtype).reshape(-1, cols).copy() if cols else raw[:n * size].view(dtype).copy(), bool((raw[n * size:] == SENTINEL).all())

    def _guides(self, npx, nh, ad):
        a, ca = self._read(self.nh, npx, 16, f32, 4, nh)
        b, cb = self._read(self.ad, npx, 16, f32, 4, ad)
        return a, b, ca and cb

    def _frame(self, n, npx, radiance=True, pixel=True):
        s, cs = self._read(self.seeds, n, 4, np.int32, 0)
        r, cr = self._read(self.radiance, npx, 16, f32, 4) if radiance else (None, True)
        p, cp = self._read(self.pixel, npx, 4, np.uint8, 4, pixel)
        return s, r, p, cs and cr and cp

    # -- mirt_view_guides_batch and the N single calls: -> (normal_hits or None, albedo_depth or None, clean)
    def guides_batch(self, view, cams, nh=True, ad=True):
        self._fill()
        self.ctx.view_guides_batch(self.scene_desc(), view.desc(), cams, self.nh if nh else None, self.ad if ad else None)
        return self._guides(len(cams) * view.n_pixels, nh, ad)

    def guides_singles(self, view, cams):
        parts = []
        for f, c in enumerate(cams):
            self._fill()
            self.ctx.view_guides(self.scene_desc(), VB.frame_view(view, c).desc(), self.nh, self.ad)
            got = self._guides(view.n_pixels, True, True)
            assert got[2], f"single call of frame {f}: bytes behind the records were written"
            parts.append(got)
        return tuple(np.concatenate([p[i] for p in parts], axis=0) for i in range(2))

    # -- mirt_view_ao_batch and the N single calls: -> (uint32 [N * P, 2], clean: the tail untouched and the seeds byte for byte what they were)
    def ao_batch(self, view, cams, seeds, samples=AO_SAMPLES, radius=AO_RADIUS, bias=VA.BIAS):
        self._fill(seeds=seeds)
        before = self.seeds.read(np.uint8).tobytes()
        self.ctx.view_ao_batch(self.scene_desc(), view.desc(), cams, self.seeds, self.ao, samples, radius, bias)
        out, clean = self._read(self.ao, len(cams) * view.n_pixels, 8, np.uint32, 2)
        return out, clean and self.seeds.read(np.uint8).tobytes() == before

    def ao_singles(self, view, cams, seeds, samples=AO_SAMPLES, radius=AO_RADIUS, bias=VA.BIAS):
        R, parts = view.n_rays, []
        for f, c in enumerate(cams):
            self._fill(seeds=seeds[f * R:(f + 1) * R])
            self.ctx.view_ao(self.scene_desc(), VB.frame_view(view, c).desc(), self.seeds, self.ao, samples, radius, bias)
            out, clean = self._read(self.ao, view.n_pixels, 8, np.uint32, 2)
            assert clean, f"single call of frame {f}: bytes behind the pairs were written"
            parts.append(out)
        return np.concatenate(parts, axis=0)

    # -- mirt_render_view_guided_batch, the N single calls and the two batch calls: -> ((seeds, radiance, pixel, clean), (nh, ad, clean))
    def guided_batch(self, view, cams, seeds, bounces=BOUNCES, carry=None, radiance=True, pixel=True):
        nf = len(cams)
        self._fill(seeds=seeds, carry=carry)
        self.ctx.render_view_guided_batch(self.scene_desc(bounces), view.desc(V.ACCUMULATE if carry is not None else 0), cams, self.seeds,
                                          self.radiance if radiance else None, self.pixel if pixel else None, self.nh, self.ad)
        return self._frame(nf * view.n_rays, nf * view.n_pixels, radiance, pixel), self._guides(nf * view.n_pixels, True, True)

    def two_batch_calls(self, view, cams, seeds, bounces=BOUNCES, carry=None):
        nf = len(cams)
        self._fill(seeds=seeds, carry=carry)
        self.ctx.render_view_batch(self.scene_desc(bounces), view.desc(V.ACCUMULATE if carry is not None else 0), cams, self.seeds, self.radiance, self.pixel)
        self.ctx.view_guides_batch(self.scene_desc(bounces), view.desc(), cams, self.nh, self.ad)
        return self._frame(nf * view.n_rays, nf * view.n_pixels), self._guides(nf * view.n_pixels, True, True)

    def guided_singles(self, view, cams, seeds, bounces=BOUNCES, carry=None):
        R, P, parts = view.n_rays, view.n_pixels, []
        for f, c in enumerate(cams):
            self._fill(seeds=seeds[f * R:(f + 1) * R], carry=None if carry is None else carry[f * P:(f + 1) * P])
            self.ctx.render_view_guided(self.scene_desc(bounces), VB.frame_view(view, c).desc(V.ACCUMULATE if carry is not None else 0), self.seeds, self.radiance,
                                        self.pixel, self.nh, self.ad)
            fr, gd = self._frame(R, P), self._guides(P, True, True)
            assert fr[3] and gd[2], f"single call of frame {f}: bytes behind the records were written"
            parts.append(fr[:3] + gd[:2])
        cat = [np.concatenate([p[i] for p in parts], axis=0) for i in range(5)]
        return (cat[0], cat[1], cat[2], True), (cat[3], cat[4], True)


def same_guides(tag, got, want):
    d = VG.differ(tag, got, want)
    assert d is None, d
    assert got[2], f"{tag}: bytes behind the records, or a buffer that was not given, were written"


def same_ao(tag, got, want):
    out, clean = got
    d = VA.difference(tag, out, want)
    assert d is None, d
    assert clean, f"{tag}: bytes behind the pairs were written, or the seeds changed"


def same_guided(tag, got, want):
    d = VG.same_frames(tag, got, want)
    assert d is None, d
    assert got[0][3] and got[1][2], f"{tag}: bytes behind the records, or a buffer that was not given, were written"


# ---- the three comparisons a child process on the other library runs too (tests/view_batch_aov_default_child.py) -------------------------------
def batch_equals_singles(ctx, name, model="equirect"):
    """the three batch calls against this library's own single calls at 13 x 7, k = 2, N = 3 -> a list of sentences, empty when all agree"""
    sc = scene(name)
    r = Aov(ctx, sc)
    bad = []
    try:
        v = V.standard_view(sc, model, tone=0.25)
        cams = VB.cameras(sc, N)
        seeds = A.make_seeds(N * v.n_rays)
        got, want = r.guides_batch(v, cams), r.guides_singles(v, cams)
        d = VG.differ(f"{name} {model} guides", got, want) or (None if got[2] else f"{name} {model} guides: tail written")
        if d is None and not (want[0][:, 3] > 0).any():
            d = f"{name} {model} guides: nothing was hit"
        bad += [d] if d else []
        got, want = r.ao_batch(v, cams, seeds), r.ao_singles(v, cams, seeds)
        d = VA.difference(f"{name} {model} ao", got[0], want) or (None if got[1] else f"{name} {model} ao: tail or seeds written")
        if d is None and not (want[:, 1] > 0).any():
            d = f"{name} {model} ao: nothing casts"
        bad += [d] if d else []
        got, want = r.guided_batch(v, cams, seeds), r.guided_singles(v, cams, seeds)
        d = VG.same_frames(f"{name} {model} guided", got, want) or (None if got[0][3] and got[1][2] else f"{name} {model} guided: tail written")
        if d is None and not (want[0][1][:, 3] > 0).any():
            d = f"{name} {model} guided: no pixel received light"
        bad += [d] if d else []
    finally:
        r.release()
    return bad
