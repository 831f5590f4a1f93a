"""GPU: mirt_upsample_guided -- shade at 1/f resolution, output at full, guided by the first-hit guide buffers of both resolutions
(include/mirt.h) -- through the C ABI, tolerance 0 against the numpy restatement of the header's definition (tests/upsample_common.py; every NaN
equal to every NaN):

  1. synthetic inputs with planted cases (background in either image, both and one only, NaN / +inf / -0 radiance, zero and negative albedo
     channels, z == 0, a pixel facing away from all four taps), low size -> factor: 1x1 -> 2, 2x1 -> 3, 1x3 -> 4, 29x17 -> 2, 3, 4 (high widths
     above one 64-wide block, partial blocks on both axes); each with the depth term on and off, DEMODULATE on and off, normal_power_log2 0 and
     5, and one output NULL in turn;
  2. libmirt_default.so gives the same bits (a child process);
  3. end to end on cornell: 96x54 from a 48x27 x 16 frame filtered with the shipped defaults, the Python driver against the restatement fed with
     the radiance and guides of the same device run;
  4. quality: the upsampled frame is closer to the converged frame than the same low frame replicated f x f (profiles/upsample/quality.json)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_fixture
from filter_common import DEFAULTS as FILTER_DEFAULTS
from filter_common import atrous, difference, tone_map
from upsample_common import DEFAULTS, SYN_HL, SYN_TONE, SYN_WL, synthetic, upsample

pytestmark = pytest.mark.gpu

DEFAULT_LIB = os.path.join(ROOT, "2015-raytracing_amd", "libmirt_default.so")
SHAPES = [(1, 1, 2), (2, 1, 3), (1, 3, 4), (SYN_WL, SYN_HL, 2), (SYN_WL, SYN_HL, 3), (SYN_WL, SYN_HL, 4)]   # low width, low height, factor


@pytest.fixture(scope="module")
def ctx(pkg):
    from raytracing_amd.pyhost import mirt
    c = mirt.Context(0)
    yield c
    c.destroy()


class Upsampler:
    """five input buffers and two outputs of one pair of image sizes, driven through mirt_upsample_guided"""

    def __init__(self, ctx, wl, hl, f, inputs):
        self.ctx, self.w, self.h, self.f = ctx, wl * f, hl * f, f
        self.ins = [ctx.buffer(np.ascontiguousarray(a, np.float32).nbytes).write(np.ascontiguousarray(a, np.float32)) for a in inputs]
        n = self.w * self.h
        self.out, self.pix = ctx.buffer(n * 16), ctx.buffer(n * 4)

    def run(self, tone, upsampled=True, pixel=True, **p):
        n = self.w * self.h
        self.out.write(np.full(n * 4, 7.5, np.float32))
        self.pix.write(np.full(n * 4, 0x5A, np.uint8))
        self.ctx.upsample_guided(self.w, self.h, self.f, tone, *self.ins, upsampled=self.out if upsampled else None, pixel=self.pix if pixel else None, **p)
        return self.out.read(np.float32).reshape(-1, 4), self.pix.read(np.uint8).reshape(-1, 4)

    def release(self):
        for b in self.ins + [self.out, self.pix]:
            b.release()


def check(tag, got, want, upsampled=True, pixel=True):
    if upsampled:
        d = difference(f"{tag} upsampled", got[0], want[0])
        assert d is None, d
    if pixel:
        d = difference(f"{tag} pixel", got[1], want[1])
        assert d is None, d


# ---- 1. synthetic inputs ----------------------------------------------------------------------------------------------------------------------
_shape = {}


def shape(ctx, wl, hl, f):
    """the planted inputs of a shape on the device, and the restatement per parameter set: made once, shared by the tests, never changed"""
    key = (wl, hl, f)
    if key not in _shape:
        inputs = synthetic(wl, hl, f)
        _shape[key] = (inputs, Upsampler(ctx, wl, hl, f, inputs), {})
    return _shape[key]


def expected(ctx, wl, hl, f, **p):
    inputs, _, want = shape(ctx, wl, hl, f)
    key = tuple(sorted(p.items()))
    if key not in want:
        want[key] = upsample(*inputs, wl * f, hl * f, f, SYN_TONE, **p)
    return want[key]


@pytest.fixture(scope="module", autouse=True)
def _release_shapes(ctx):
    yield
    for _, u, _ in _shape.values():
        u.release()
    _shape.clear()


@pytest.mark.parametrize("npow", [0, 5])
@pytest.mark.parametrize("demodulate", [False, True])
@pytest.mark.parametrize("sigma_depth", [0.0, 0.1])
@pytest.mark.parametrize("wl,hl,f", SHAPES)
def test_synthetic(ctx, wl, hl, f, sigma_depth, demodulate, npow):
    p = dict(normal_power_log2=npow, sigma_depth=sigma_depth, demodulate=demodulate)
    u = shape(ctx, wl, hl, f)[1]
    tag = f"{wl}x{hl} -> {f}, depth {sigma_depth} demodulate={demodulate} power 2^{npow}"
    want = expected(ctx, wl, hl, f, **p)
    check(tag, u.run(SYN_TONE, **p), want)
    for upsampled, pixel in ((True, False), (False, True)):   # one output NULL in turn: the other one is written alike, the missing one not at all
        got = u.run(SYN_TONE, upsampled=upsampled, pixel=pixel, **p)
        check(f"{tag}, {'upsampled' if upsampled else 'pixel'} alone", got, want, upsampled, pixel)
        if not upsampled:
            assert (got[0] == 7.5).all(), "upsampled was written though it was not passed"
        if not pixel:
            assert (got[1] == 0x5A).all(), "pixel was written though it was not passed"


@pytest.mark.parametrize("sigma_depth", [float("nan"), float("inf"), -1.0])
def test_a_sigma_that_is_no_width_turns_the_depth_term_off(ctx, sigma_depth):
    p = dict(DEFAULTS, sigma_depth=sigma_depth)
    u = shape(ctx, SYN_WL, SYN_HL, 3)[1]
    check(f"sigma_depth {sigma_depth}", u.run(SYN_TONE, **p), expected(ctx, SYN_WL, SYN_HL, 3, **dict(DEFAULTS, sigma_depth=0.0)))


def test_the_planted_cases_take_the_paths_they_were_planted_for(ctx):
    """what the restatement itself says of the planted inputs, so that the bit comparison above is known to cover them: the facing-away pixel
    falls back to its covering low pixel times its own albedo, a background high pixel over surface low pixels gets their raw radiance, the
    inputs are left alone"""
    from upsample_common import AWAY_LOW, HIGH_ONLY_BG
    f = 3
    inputs, u, _ = shape(ctx, SYN_WL, SYN_HL, f)
    Rl, NHl, ADl, NH, AD = inputs
    W = SYN_WL * f
    got, _ = u.run(SYN_TONE, **DEFAULTS)
    ay, ax = AWAY_LOW[0] * f + 1, AWAY_LOW[1] * f + 1
    q = AWAY_LOW[0] * SYN_WL + AWAY_LOW[1]
    a_lo, a_hi = ADl[q, :3] / NHl[q, 3], AD[ay * W + ax, :3] / NH[ay * W + ax, 3]
    assert np.allclose(got[ay * W + ax, :3], Rl[q, :3] / a_lo * a_hi, rtol=1e-5), "the pixel facing away from its taps"
    by, bx = HIGH_ONLY_BG[0].start * f + 1, HIGH_ONLY_BG[1].start * f + 1
    assert NH[by * W + bx, 3] == 0 and NHl[HIGH_ONLY_BG[0].start * SYN_WL + HIGH_ONLY_BG[1].start, 3] > 0
    d = difference("a background high pixel over a surface", got[by * W + bx], Rl[HIGH_ONLY_BG[0].start * SYN_WL + HIGH_ONLY_BG[1].start])
    assert d is None, d
    for name, buf, want in zip(("radiance_lo", "normal_hits_lo", "albedo_depth_lo", "normal_hits", "albedo_depth"), u.ins, inputs):
        assert buf.read(np.float32).tobytes() == np.ascontiguousarray(want, np.float32).tobytes(), f"{name} changed"


# ---- 2. the default contract ------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(DEFAULT_LIB), reason="needs libmirt_default.so")
def test_the_default_contract_library_gives_the_same_bits(ctx, tmp_path):
    """libmirt_default.so at 29x17 -> 3, in a process of its own (a process loads one libmirt): against the restatement there, and here its
    saved outputs against what libmirt.so writes for the same inputs and parameters, bit for bit (every NaN equal to every NaN)"""
    from upsample_default_child import CASES, F
    env = dict(os.environ, MIRT_CONTRACT="default")
    env.pop("MIRT_LIB_PATH", None)
    saved = str(tmp_path / "default.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "upsample_default_child.py"), saved], env=env, capture_output=True, text=True, timeout=600)
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0, (lines[-1:] or r.stderr[-2000:])
    assert len(lines) == len(CASES) and all(l["ok"] for l in lines)
    theirs = np.load(saved)
    u = shape(ctx, SYN_WL, SYN_HL, F)[1]
    for i, (npow, sigma_depth, demodulate) in enumerate(CASES):
        ours = u.run(SYN_TONE, normal_power_log2=npow, sigma_depth=sigma_depth, demodulate=demodulate)
        check(f"libmirt_default.so against libmirt.so, case {i}", (theirs[f"upsampled_{i}"], theirs[f"pixel_{i}"]), ours)


# ---- 3. end to end, 4. quality ----------------------------------------------------------------------------------------------------------------
W, H, F, RPP = 96, 54, 2, 16


def resized(w, h, rpp):
    from raytracing_amd.pyhost import scene
    _, sc0 = load_fixture("cornell_32x24_r4")
    return scene.PackedScene(dict(sc0.d)).resized(w, h, rpp)


@pytest.fixture(scope="module")
def cornell(ctx):
    """one device run of the driver: 96x54 from 48x27 x 16, one pass, filtered with the shipped defaults; everything read back once"""
    from raytracing_amd.pyhost import render
    u = render.UpscaledRenderer(ctx, resized(W, H, RPP), F, seed_base=3)
    try:
        pixel, upsampled = u.render(passes=1, denoise=True)
        rd = lambda b: b.read(np.float32).reshape(-1, 4)
        yield dict(pixel=pixel, upsampled=upsampled, tone=u.tone, radiance=rd(u.lo.radiance), filtered=rd(u.filtered), nh_lo=rd(u.nh_lo), ad_lo=rd(u.ad_lo),
                   nh=rd(u.nh), ad=rd(u.ad))
    finally:
        u.release()


def test_the_driver_equals_the_restatement_on_cornell(cornell):
    c = cornell
    assert c["tone"] == np.float32(1.0 / RPP) and (c["nh"][:, 3] > 0).mean() > 0.5 and (c["nh_lo"][:, 3] > 0).mean() > 0.5
    filtered, _ = atrous(c["radiance"], c["nh_lo"], c["ad_lo"], W // F, H // F, c["tone"], **FILTER_DEFAULTS)
    d = difference("the low frame the driver filtered", c["filtered"], filtered)
    assert d is None, d
    want = upsample(c["filtered"], c["nh_lo"], c["ad_lo"], c["nh"], c["ad"], W, H, F, c["tone"], **DEFAULTS)
    check("cornell 48x27 x 16 -> 96x54", (c["upsampled"], c["pixel"]), want)
    assert (c["upsampled"][:, :3] != np.repeat(np.repeat(c["filtered"].reshape(H // F, W // F, 4), F, 0), F, 1).reshape(-1, 4)[:, :3]).any()


def test_the_upsampled_frame_beats_pixel_replication(ctx, cornell):
    """expected behaviour, not bits.  The truth: 256 rays x 4 passes at 96x54 from this library.  Error: mean squared error over the tone-mapped
    floats before quantisation (as tests/test_filter.py).  ASSERTED: the upsampled frame is closer to the truth than the same filtered low frame
    replicated f x f by numpy -- a baseline independent of the code under test, without a margin: beating pixel replication is the least the
    feature must do.  RECORDED only: the equal-budget alternative, 96x54 x 4 rays filtered."""
    from raytracing_amd.pyhost import render
    c = cornell
    conv = render.FusedRenderer(ctx, resized(W, H, 256), seed_base=5)
    full = render.FusedRenderer(ctx, resized(W, H, 4), seed_base=3)
    try:
        for p in range(4):
            conv.execute_render(fresh=(p == 0))
        ref = tone_map(conv.radiance.read(np.float32).reshape(-1, 4)[:, :3], np.float32(1.0 / 1024.0)).astype(np.float64)
        full.execute_render(fresh=True)
        _, equal_budget = full.denoised(**FILTER_DEFAULTS)
        mse = lambda img, tone: float(((tone_map(img[:, :3], tone).astype(np.float64) - ref) ** 2).mean())
        replicated = np.repeat(np.repeat(c["filtered"].reshape(H // F, W // F, 4), F, axis=0), F, axis=1).reshape(-1, 4)
        mse_up, mse_rep, mse_equal = mse(c["upsampled"], c["tone"]), mse(replicated, c["tone"]), mse(equal_budget, np.float32(0.25))
        print(f"mse against 256 rays x 4 passes: upsampled {mse_up:.3f}, replicated {mse_rep:.3f}, 96x54 x 4 filtered {mse_equal:.3f}")
        if os.environ.get("MIRT_UPSAMPLE_QUALITY_JSON"):   # how profiles/upsample/quality.json is made
            with open(os.environ["MIRT_UPSAMPLE_QUALITY_JSON"], "w") as fh:
                json.dump({"scene": "cornell", "width": W, "height": H, "factor": F, "low_rays_per_pixel": RPP, "converged": "256 rays x 4 passes",
                           "filter_parameters": FILTER_DEFAULTS, "upsample_parameters": DEFAULTS, "mse_upsampled": round(mse_up, 4),
                           "mse_low_frame_replicated": round(mse_rep, 4), "mse_equal_budget_full_resolution_4_rays_filtered": round(mse_equal, 4)}, fh, indent=1)
                fh.write("\n")
        assert mse_up < mse_rep
    finally:
        conv.release()
        full.release()
