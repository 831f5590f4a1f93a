"""Shared by tests/test_upsample.py, tests/test_upsample_abi.py, tests/test_upsample_js.py, tests/test_upsample_taps.py and
tests/upsample_default_child.py: what mirt_upsample_guided is checked against.

upsample() restates the definition in include/mirt.h (the comment of mirt_upsample_guided) with numpy: one np.float32 operation at a time in the
order the header writes them, np.fmax (a NaN loses) for max, every quotient through float64 (53 >= 2 * 24 + 2 bits: the rounded-back quotient is
the correctly rounded fp32 one).  Vectorised over the high image: four gathered taps.  The tap geometry is Python's own // (floor division).
The counterpart of tests/filter_common.py::atrous; synthetic() makes the planted inputs the GPU tests and the default-contract child share."""
import numpy as np

from filter_common import div, term_on, tone_map

f32 = np.float32
DEFAULTS = {"normal_power_log2": 5, "sigma_depth": 0.1, "demodulate": True}   # MIRT_UPSAMPLE_DEFAULT_* (include/mirt.h)


def tap_axis(n_high, f):
    """per high coordinate x of an axis: (X0, m), e = 2x + 1 - f, X0 = floor(e / 2f), m = e - 2f * X0"""
    e = 2 * np.arange(n_high, dtype=np.int64) + 1 - f
    q0 = e // (2 * f)
    return q0, e - 2 * f * q0


def _normalised(NH, AD):
    one = f32(1)
    hits = NH[..., 3]
    live = hits > 0
    r = np.where(live, div(one, np.where(live, hits, one)), one).astype(f32)
    return live, (NH[..., :3] * r[..., None]).astype(f32), (AD[..., 3] * r).astype(f32), (AD[..., :3] * r[..., None]).astype(f32)


def upsample(radiance_lo, normal_hits_lo, albedo_depth_lo, normal_hits, albedo_depth, width, height, factor, tone, normal_power_log2=0,
             sigma_depth=0.0, demodulate=False):
    """-> (upsampled float32 [high pixels, 4], pixel uint8 [high pixels, 4])"""
    W, H, f = int(width), int(height), int(factor)
    assert W % f == 0 and H % f == 0
    wl, hl = W // f, H // f
    Rl = np.asarray(radiance_lo, f32).reshape(hl, wl, 4)
    NHl = np.asarray(normal_hits_lo, f32).reshape(hl, wl, 4)
    ADl = np.asarray(albedo_depth_lo, f32).reshape(hl, wl, 4)
    NH = np.asarray(normal_hits, f32).reshape(H, W, 4)
    AD = np.asarray(albedo_depth, f32).reshape(H, W, 4)
    one = f32(1)
    with np.errstate(all="ignore"):
        live_lo, n_lo, z_lo, a_lo = _normalised(NHl, ADl)
        dem_lo = (live_lo[..., None] & (a_lo > 0)) if demodulate else np.zeros((hl, wl, 3), bool)
        J = np.where(dem_lo, div(Rl[..., :3], np.where(dem_lo, a_lo, one)), Rl[..., :3]).astype(f32)
        live, n, z, a = _normalised(NH, AD)
        depth_on = term_on(sigma_depth)
        izp = div(one, f32(sigma_depth) * z) if depth_on else None
        X0, mx = tap_axis(W, f)
        Y0, my = tap_axis(H, f)
        tx, ty = div(mx.astype(f32), f32(2 * f)), div(my.astype(f32), f32(2 * f))
        bx, by = ((one - tx).astype(f32), tx), ((one - ty).astype(f32), ty)
        sumw = np.zeros((H, W), f32)
        sumc = np.zeros((H, W, 3), f32)
        for j in range(2):
            for i in range(2):
                qx, qy = X0 + i, Y0 + j
                inside = ((qy >= 0) & (qy < hl))[:, None] & ((qx >= 0) & (qx < wl))[None, :]
                Q = (np.clip(qy, 0, hl - 1)[:, None], np.clip(qx, 0, wl - 1)[None, :])
                b = (by[j][:, None] * bx[i][None, :]).astype(f32)
                nq = n_lo[Q]
                wn = np.fmax(f32(0), (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2])
                for _ in range(int(normal_power_log2)):
                    wn = wn * wn
                w = b * wn
                if depth_on:
                    w = w * np.fmax(f32(0), one - np.abs(z - z_lo[Q]) * izp)
                w = np.where(live, w, b).astype(f32)                     # a background pixel: w = b ...
                val = np.where(live[..., None], J[Q], Rl[Q][..., :3])     # ... and the raw radiance of its background taps
                take = inside & (live_lo[Q] == live) & (w > 0)
                sumw = np.where(take, sumw + w, sumw).astype(f32)
                sumc = np.where(take[..., None], sumc + val * w[..., None], sumc).astype(f32)
        ok = sumw > 0
        Q0 = ((np.arange(H) // f)[:, None], (np.arange(W) // f)[None, :])
        both = live & live_lo[Q0]
        fallback = np.where(both[..., None], J[Q0], Rl[Q0][..., :3])
        I = np.where(ok[..., None], div(sumc, np.where(ok, sumw, one)[..., None]), fallback).astype(f32)
        raw = ~ok & ~both
        back = (live & ~raw)[..., None] & (a > 0) & bool(demodulate)
        out = np.where(back, I * a, I).astype(f32)
    upsampled = np.concatenate([out, Rl[Q0][..., 3:4]], axis=2).astype(f32).reshape(-1, 4)
    pixel = np.concatenate([tone_map(out, tone).astype(np.uint8), np.full((H, W, 1), 255, np.uint8)], axis=2).reshape(-1, 4)
    return upsampled, pixel


SYN_WL, SYN_HL, SYN_TONE = 29, 17, f32(0.25)
# low (row, column) of the planted cases of synthetic() at sizes of at least 24 x 16 low pixels
NAN_AT, INF_AT, NEGZERO_AT = (8, 5), (12, 20), (2, 25)
AWAY_LOW = (5, 22)      # the high pixel (f * 5 + 1, f * 22 + 1) faces away from all four of its taps: the fallback
LOW_ONLY_BG = (slice(3, 7), slice(14, 16))      # background in the low image, surface in the high one
HIGH_ONLY_BG = (slice(10, 12), slice(20, 23))   # (in low pixels) surface in the low image, background in the high one


def _guides(g, h, w, nrm, z):
    hits = g.integers(1, 5, (h, w)).astype(f32)
    alb = g.uniform(0.2, 1.0, (h, w, 3)).astype(f32)
    NH = np.concatenate([nrm * hits[..., None], hits[..., None]], axis=2).astype(f32)
    AD = np.concatenate([alb * hits[..., None], (z * hits)[..., None]], axis=2).astype(f32)
    return NH, AD


def synthetic(wl=SYN_WL, hl=SYN_HL, f=3, seed=7):
    """Planted inputs (float32 [pixels, 4] each: radiance_lo, normal_hits_lo, albedo_depth_lo, normal_hits, albedo_depth).  The low image:
    random radiance, normals of the +z hemisphere, depths with a step, albedos, hits 1 .. 4; the high guides: the low ones replicated f x f and
    perturbed, with hit counts of their own.  Planted (at 24 x 16 low pixels and more): background pixels scattered and in blocks, in the low
    image, in the high image, in both and in one only; NaN / +inf / -0 radiance; zero and negative albedo channels in both resolutions; z == 0
    in both; a live high pixel facing away from all four taps.  Smaller images get a background pixel in each resolution, a NaN and a pixel
    facing away, as far as they have room."""
    g = np.random.default_rng(seed)
    W, H = wl * f, hl * f
    nrm = g.normal(size=(hl, wl, 3)).astype(f32)
    nrm[..., 2] = np.abs(nrm[..., 2]) + f32(0.3)
    nrm = (nrm / np.linalg.norm(nrm, axis=2, keepdims=True)).astype(f32)
    yy, xx = np.mgrid[0:hl, 0:wl]
    z = (f32(5) + f32(0.09) * xx + f32(0.15) * yy + g.uniform(0, 0.2, (hl, wl)) + 3.0 * (xx > (2 * wl) // 3)).astype(f32)
    NHl, ADl = _guides(g, hl, wl, nrm, z)
    rad = (g.uniform(0.0, 1.0, (hl, wl, 3)) * (1.0 + (yy[..., None] > hl // 2))).astype(f32)
    Rl = np.concatenate([rad, g.uniform(0, 4, (hl, wl, 1)).astype(f32)], axis=2)
    rep = lambda a: np.repeat(np.repeat(a, f, axis=0), f, axis=1)
    nrm_h = rep(nrm) + f32(0.25) * g.normal(size=(H, W, 3)).astype(f32)
    nrm_h = (nrm_h / np.linalg.norm(nrm_h, axis=2, keepdims=True)).astype(f32)
    z_h = (rep(z) * g.uniform(0.97, 1.03, (H, W))).astype(f32)
    NH, AD = _guides(g, H, W, nrm_h, z_h)
    hi = lambda s: slice(s.start * f, s.stop * f)
    if wl >= 24 and hl >= 16:
        bg_lo = g.uniform(size=(hl, wl)) < 0.05                 # background: scattered ...
        bg_hi = rep(bg_lo) ^ (g.uniform(size=(H, W)) < 0.03)    # ... mostly the same pixels in both, some in one only
        bg_lo[3:7, 10:16] = True                                # ... and in blocks: both resolutions,
        bg_hi[hi(slice(3, 7)), hi(slice(10, 16))] = True
        bg_hi[hi(LOW_ONLY_BG[0]), hi(LOW_ONLY_BG[1])] = False   # the low image only (high pixels over background low pixels),
        bg_lo[HIGH_ONLY_BG] = False
        bg_hi[hi(HIGH_ONLY_BG[0]), hi(HIGH_ONLY_BG[1])] = True  # the high image only
        for r, c in (NAN_AT, INF_AT, NEGZERO_AT):
            bg_lo[r, c] = False
        bg_lo[AWAY_LOW[0] - 1:AWAY_LOW[0] + 2, AWAY_LOW[1] - 1:AWAY_LOW[1] + 2] = False
        ay, ax = AWAY_LOW[0] * f + 1, AWAY_LOW[1] * f + 1
        bg_hi[ay, ax] = False
        NHl[bg_lo] = 0
        ADl[bg_lo] = 0
        NH[bg_hi] = 0
        AD[bg_hi] = 0
        Rl[NAN_AT][0] = np.nan
        Rl[INF_AT][1] = np.inf
        Rl[NEGZERO_AT][:3] = f32(-0.0)
        ADl[9, 3:6, 0] = 0                                      # zero and negative albedo channels, low ...
        ADl[10, 3:6, 1] = -ADl[10, 3:6, 1]
        ADl[11, 4, :3] = 0
        AD[9 * f + 1, 3 * f:6 * f, 0] = 0                       # ... and high
        AD[10 * f, 3 * f:6 * f, 1] = -AD[10 * f, 3 * f:6 * f, 1]
        AD[5, 7, :3] = 0
        ADl[13, 8:10, 3] = 0                                    # z == 0, low and high
        AD[14 * f, 8 * f:10 * f, 3] = 0
        NH[ay, ax, :3] = (0, 0, -NH[ay, ax, 3])                 # dn = 0 for each of its taps
    else:
        if wl * hl > 1:
            NHl[0, 0] = 0                                       # a background low pixel under live high pixels
            ADl[0, 0] = 0
            Rl[hl - 1, wl - 1, 2] = np.nan
        NH[0, 0] = 0                                            # a background high pixel
        AD[0, 0] = 0
        NH[H - 1, W - 1, :3] = (0, 0, -NH[H - 1, W - 1, 3])     # faces away from its taps
        AD[H - 1, 0, 1] = 0
    return tuple(a.reshape(-1, 4) for a in (Rl, NHl, ADl, NH, AD))
