"""Shared by tests/test_filter.py, tests/test_filter_abi.py, tests/test_filter_js.py and tests/filter_default_child.py: what mirt_filter_atrous is
checked against.

atrous() restates the definition in include/mirt.h (the comment of mirt_filter_atrous) with numpy: one np.float32 operation at a time in the order
the header writes them, np.fmax (a NaN loses) for max, every quotient through float64 (53 >= 2 * 24 + 2 bits: the rounded-back quotient is the
correctly rounded fp32 one).  Vectorised over the image: 24 shifted slices per iteration.  synthetic() makes the planted inputs the GPU tests and
the default-contract child share; difference() reports the first bit that differs."""
import numpy as np

f32 = np.float32
H3 = (f32(0.375), f32(0.25), f32(0.0625))   # the B3 spline by |offset|: 3/8, 1/4, 1/16
DEFAULTS = {"iterations": 3, "normal_power_log2": 5, "sigma_depth": 0.1, "sigma_colour": 1.0, "demodulate": True}   # MIRT_FILTER_DEFAULT_* (include/mirt.h)


def div(n, d):
    """the correctly rounded fp32 quotient"""
    return (np.asarray(n, f32).astype(np.float64) / np.asarray(d, f32).astype(np.float64)).astype(f32)


def term_on(sigma):
    s = f32(sigma)
    return bool(np.isfinite(s) and s > 0)


def tone_map(out, tone):
    """copyToPixel's tone map (A10 code.cl:1381-1385) up to the clamp: the float the pixel is converted from"""
    sc = f32(255.0) * f32(tone)
    v = (out * sc) * f32(1.8)
    return np.where(np.isnan(v), f32(0), np.clip(v, f32(0), f32(255))).astype(f32)


def atrous(radiance, normal_hits, albedo_depth, width, height, tone, iterations=0, normal_power_log2=0, sigma_depth=0.0, sigma_colour=0.0,
           demodulate=False):
    """-> (filtered float32 [pixels, 4], pixel uint8 [pixels, 4])"""
    W, H = int(width), int(height)
    R = np.asarray(radiance, f32).reshape(H, W, 4)
    NH = np.asarray(normal_hits, f32).reshape(H, W, 4)
    AD = np.asarray(albedo_depth, f32).reshape(H, W, 4)
    tone = f32(tone)
    one = f32(1)
    with np.errstate(all="ignore"):
        hits = NH[..., 3]
        live = hits > 0
        r = np.where(live, div(one, np.where(live, hits, one)), one).astype(f32)
        n = (NH[..., :3] * r[..., None]).astype(f32)
        z = (AD[..., 3] * r).astype(f32)
        a = (AD[..., :3] * r[..., None]).astype(f32)
        demod = np.zeros((H, W, 3), bool)
        if demodulate:
            demod = live[..., None] & (a > 0)
        I = np.where(demod, div(R[..., :3], np.where(demod, a, one)), R[..., :3]).astype(f32)
        depth_on, colour_on = term_on(sigma_depth), term_on(sigma_colour)
        izp = div(one, f32(sigma_depth) * z) if depth_on else None
        for i in range(int(iterations)):
            s = 1 << i
            inv = None
            if colour_on:
                k_i = f32(sigma_colour) * f32(2.0 ** -i)
                inv = one / (k_i * k_i)
            sumw = np.full((H, W), f32(0.140625), f32)
            sumc = (I * f32(0.140625)).astype(f32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    if dx == 0 and dy == 0:
                        continue
                    oy, ox = dy * s, dx * s
                    py0, py1 = max(0, -oy), H - max(0, oy)
                    px0, px1 = max(0, -ox), W - max(0, ox)
                    if py0 >= py1 or px0 >= px1:
                        continue   # every such tap is outside the image
                    P = (slice(py0, py1), slice(px0, px1))
                    Q = (slice(py0 + oy, py1 + oy), slice(px0 + ox, px1 + ox))
                    k = H3[abs(dy)] * H3[abs(dx)]
                    np_, nq = n[P], n[Q]
                    wn = np.fmax(f32(0), (np_[..., 0] * nq[..., 0] + np_[..., 1] * nq[..., 1]) + np_[..., 2] * nq[..., 2])
                    for _ in range(int(normal_power_log2)):
                        wn = wn * wn
                    w = k * wn
                    if depth_on:
                        w = w * np.fmax(f32(0), one - np.abs(z[P] - z[Q]) * izp[P])
                    if colour_on:
                        e = (I[P] - I[Q]) * tone
                        c = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
                        w = w * np.fmax(f32(0), one - c * inv)
                    take = live[P] & live[Q] & (w > 0)
                    sumw[P] = np.where(take, sumw[P] + w, sumw[P])
                    sumc[P] = np.where(take[..., None], sumc[P] + I[Q] * w[..., None], sumc[P])
            I = np.where(live[..., None], div(sumc, sumw[..., None]), I).astype(f32)
        out = np.where(demod, I * a, I).astype(f32)
    filtered = np.concatenate([out, R[..., 3:4]], axis=2).astype(f32).reshape(-1, 4)
    pixel = np.concatenate([tone_map(out, tone).astype(np.uint8), np.full((H, W, 1), 255, np.uint8)], axis=2).reshape(-1, 4)
    return filtered, pixel


SYN_W, SYN_H, SYN_TONE = 83, 47, f32(0.25)
LONELY = (20, 40)     # (row, column): the pixel of synthetic() whose every tap gets weight 0
NAN_AT, INF_AT, NEGZERO_AT = (10, 12), (30, 60), (25, 5)


def synthetic(width=SYN_W, height=SYN_H, seed=7):
    """Planted inputs (float32 [pixels, 4] each): random radiance, normals of the +z hemisphere, depths and albedos, hits 1 .. 4, with background
    pixels scattered and in blocks, NaN / +inf / -0 radiance, zero and negative albedo channels, z == 0, and (at the default size) one pixel
    facing away from all the others -- every one of its taps gets weight 0."""
    W, H = width, height
    g = np.random.default_rng(seed)
    hits = g.integers(1, 5, (H, W)).astype(f32)
    nrm = g.normal(size=(H, W, 3)).astype(f32)
    nrm[..., 2] = np.abs(nrm[..., 2]) + f32(0.3)
    nrm = (nrm / np.linalg.norm(nrm, axis=2, keepdims=True)).astype(f32)
    yy, xx = np.mgrid[0:H, 0:W]
    z = (f32(5) + f32(0.03) * xx + f32(0.05) * yy + g.uniform(0, 0.2, (H, W)) + 3.0 * (xx > (2 * W) // 3)).astype(f32)
    alb = g.uniform(0.2, 1.0, (H, W, 3)).astype(f32)
    rad = (g.uniform(0.0, 1.0, (H, W, 3)) * (1.0 + (yy[..., None] > H // 2))).astype(f32)   # (tone 0.25: colour distances around the hat's width)
    R = np.concatenate([rad, g.uniform(0, 4, (H, W, 1)).astype(f32)], axis=2)
    NH = np.concatenate([nrm * hits[..., None], hits[..., None]], axis=2).astype(f32)
    AD = np.concatenate([alb * hits[..., None], (z * hits)[..., None]], axis=2).astype(f32)
    if W > 70 and H > 40:
        bg = g.uniform(size=(H, W)) < 0.05                      # background: scattered ...
        bg[5:12, 30:45] = True                                  # ... and in blocks
        bg[H - 6:, :9] = True
        for at in (LONELY, NAN_AT, INF_AT, NEGZERO_AT):
            bg[at] = False
        NH[bg] = 0
        AD[bg] = 0
        R[NAN_AT][0] = np.nan
        R[INF_AT][1] = np.inf
        R[NEGZERO_AT][:3] = f32(-0.0)
        AD[15, 20:26, 0] = 0                                    # zero and negative albedo channels
        AD[16, 20:26, 1] = -AD[16, 20:26, 1]
        AD[17, 22, :3] = 0
        AD[33, 50:54, 3] = 0                                    # z == 0
        NH[LONELY][:3] = (0, 0, -NH[LONELY][3])                 # faces away from every other normal: dn = 0 for each of its taps
    elif W * H > 1:
        NH[0, 0] = 0                                            # one background pixel, one NaN
        AD[0, 0] = 0
        R[H - 1, W - 1, 2] = np.nan                             # (a 1x1 image keeps its one pixel live and finite: a centre all of whose taps are outside)
    return R.reshape(-1, 4), NH.reshape(-1, 4), AD.reshape(-1, 4)


def difference(tag, got, want):
    """None when equal bit for bit (every NaN equal to every NaN), else a sentence naming the first difference"""
    g = np.ascontiguousarray(got).reshape(-1)
    w = np.ascontiguousarray(want).reshape(-1)
    if g.dtype != w.dtype or g.size != w.size:
        return f"{tag}: {g.size} {g.dtype} against {w.size} {w.dtype}"
    per = 4
    if g.dtype == np.float32:
        g, w = g.view(np.uint32).copy(), w.view(np.uint32).copy()
        for u in (g, w):
            u[(u & 0x7FFFFFFF) > 0x7F800000] = 0x7FC00000
    bad = np.flatnonzero(g != w)
    if bad.size == 0:
        return None
    i = int(bad[0])
    return f"{tag}: {bad.size} of {g.size} words differ; first at pixel {i // per} channel {i % per}: got 0x{int(g[i]):08x}, want 0x{int(w[i]):08x}"
