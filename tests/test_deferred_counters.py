"""GPU: which deferral counter belongs to which call.  Six kinds of call run an optimistic / exact pair and keep a counter of what the exact kernel
redid -- mirt_render_first_pass / mirt_pass_deferred, mirt_render_ao / mirt_ao_deferred, mirt_trace_closest / mirt_trace_deferred,
mirt_trace_radiance / mirt_radiance_deferred, mirt_render_view / mirt_view_deferred, mirt_view_ao / mirt_view_ao_deferred -- and the counter of
one kind survives calls of every other kind (mirt_render_guides and mirt_view_guides included: they share a mask of their own and have no
counter).  ONE context, the `guard` stratum scene of tests/rays_common.py (37 x 21 x 4, seed 3022), its ray batch, and the view camera mixed_k2
of tests/view_cameras_common.py for the three view calls: every kind defers something there.

Each kind runs once alone for its baseline (inputs refilled before every call, so a kind's count is the same each time); then
  a. a counter read twice in a row gives the same value;
  b. all six kinds in a fixed order with the two guide calls in between, the six counters read only at the end: each is its baseline;
  c. the same in the reverse order;
  d. after set_exact_only(True) and one call of kind X, counter X is 0 and the other five are their baselines;
  e. a mirt_trace_closest of zero rays queues nothing and touches no counter: mirt_trace_deferred stays what the last batch left, and so do
     the other five (the zero-ray call returns before the pair is reached);
  f. every baseline is above 0, and a multiple of 256 for the two block masks (the pass resolving its own pixels, the view pass).
"""
import numpy as np
import pytest

import rays_common as R
import view_cameras_common as VC

pytestmark = pytest.mark.gpu

KINDS = ("pass", "ao", "trace", "radiance", "view", "view_ao")
BLOCK_KINDS = ("pass", "view")   # a bit of their masks is a block of 256 samples
ORDER = ("pass", "guides", "ao", "trace", "view_guides", "radiance", "view", "guides", "view_ao", "view_guides")
SAMPLES, RADIUS, BIAS = 3, 16.0, 0.001   # the AO parameters of tests/test_ao.py on this stratum


class Rig:
    """the scene, the rays, the camera and every buffer of the eight calls, on one context"""

    def __init__(self, ctx):
        from raytracing_amd.pyhost import mirt
        self.ctx = ctx
        sc = R.scene("guard")
        assert (sc.width, sc.height, sc.rpp) == R.SCENE_SIZE
        self.dev = mirt.DeviceScene(ctx, sc)
        self.npix, self.nrays = sc.width * sc.height, sc.width * sc.height * sc.rpp
        self.view = VC.view("guard", "mixed_k2")
        self.vdesc = self.view.desc()
        rays, _ = R.rays_of("guard")
        self.n = len(rays)
        vr, vp = self.view.n_rays, self.view.n_pixels
        b = ctx.buffer
        self.bufs = dict(pass_seeds=b(self.nrays * 4), pixel=b(self.npix * 4), ao_seeds=b(self.nrays * 4), ao_out=b(self.npix * 8),
                         rays=b(self.n * 32), hits=b(self.n * 32), sets=b(self.n * 4), rad_seeds=b(self.n * 4), rad_out=b(self.n * 16),
                         view_seeds=b(vr * 4), view_rad=b(vp * 16), vao_seeds=b(vr * 4), vao_out=b(vp * 8),
                         nh=b(self.npix * 16), ad=b(self.npix * 16), vnh=b(vp * 16), vad=b(vp * 16))
        for name, buf in self.bufs.items():
            setattr(self, name, buf)
        self.rays.write(rays)
        self.scene_desc = self.dev.pass_desc(None, None)
        self.view_scene_desc = self.dev.pass_desc(None, None, bounces=VC.BOUNCES)
        self.pass_desc = self.dev.pass_desc(self.pass_seeds, None, pixel=self.pixel)   # no accumulator: the pass resolves its own pixels, a bit per block
        self.ao_desc = self.dev.pass_desc(self.ao_seeds, None)
        self.view_first = self.view.row0 * self.view.width * self.view.rpp

    def run(self, kind):
        c = self.ctx
        if kind == "pass":
            c.seed_fill(self.pass_seeds, 0, self.nrays)
            c.render_pass(self.pass_desc, fresh=True)
        elif kind == "ao":
            c.seed_fill(self.ao_seeds, 0, self.nrays)
            c.render_ao(self.ao_desc, self.ao_out, SAMPLES, RADIUS, BIAS)
        elif kind == "trace":
            c.trace_closest(self.scene_desc, self.rays, self.n, self.hits, self.sets)
        elif kind == "radiance":
            c.seed_fill(self.rad_seeds, 0, self.n)
            c.trace_radiance(self.scene_desc, self.rays, self.n, self.rad_seeds, self.rad_out)
        elif kind == "view":
            c.seed_fill(self.view_seeds, self.view_first, self.view.n_rays)
            c.render_view(self.view_scene_desc, self.vdesc, self.view_seeds, self.view_rad, None)
        elif kind == "view_ao":
            c.seed_fill(self.vao_seeds, self.view_first, self.view.n_rays)
            c.view_ao(self.scene_desc, self.vdesc, self.vao_seeds, self.vao_out, SAMPLES, RADIUS, BIAS)
        elif kind == "guides":
            c.render_guides(self.scene_desc, self.nh, self.ad)
        elif kind == "view_guides":
            c.view_guides(self.scene_desc, self.vdesc, self.vnh, self.vad)
        else:
            raise KeyError(kind)

    def counter(self, kind):
        c = self.ctx
        return {"pass": c.pass_deferred, "ao": c.ao_deferred, "trace": c.trace_deferred, "radiance": c.radiance_deferred, "view": c.view_deferred,
                "view_ao": c.view_ao_deferred}[kind]()

    def counters(self):
        return {k: self.counter(k) for k in KINDS}

    def release(self):
        for buf in self.bufs.values():
            buf.release()
        self.dev.release()


@pytest.fixture(scope="module")
def rig(pkg):
    from raytracing_amd.pyhost import mirt
    ctx = mirt.Context(0)
    r = Rig(ctx)
    yield r
    r.release()
    ctx.destroy()


@pytest.fixture(scope="module")
def baseline(rig):
    """each kind once, alone, its counter read right behind it"""
    out = {}
    for kind in KINDS:
        rig.run(kind)
        out[kind] = rig.counter(kind)
    print("baselines:", out)
    return out


def test_every_kind_defers_something_on_the_guard_scene(rig, baseline):
    sizes = {"pass": rig.nrays, "ao": rig.npix, "trace": rig.n, "radiance": rig.n, "view": rig.view.n_rays, "view_ao": rig.view.n_pixels}
    for kind in KINDS:
        unit = 256 if kind in BLOCK_KINDS else 1
        assert baseline[kind] > 0, f"{kind}: nothing deferred"
        assert baseline[kind] % unit == 0, f"{kind}: {baseline[kind]} is no multiple of {unit}"
        assert baseline[kind] <= -(-sizes[kind] // unit) * unit, f"{kind}: {baseline[kind]} deferred of {sizes[kind]}"


def test_a_counter_read_twice_is_the_same(rig, baseline):
    for kind in KINDS:
        rig.run(kind)
        assert rig.counter(kind) == rig.counter(kind) == baseline[kind], kind
    assert rig.counters() == rig.counters() == baseline


@pytest.mark.parametrize("order", [ORDER, ORDER[::-1]], ids=["forward", "reverse"])
def test_each_counter_survives_the_calls_of_every_other_kind(rig, baseline, order):
    for kind in order:
        rig.run(kind)
    got = rig.counters()
    print(got)
    assert got == baseline


@pytest.mark.parametrize("kind", KINDS)
def test_an_exact_only_call_zeroes_its_own_counter_alone(rig, baseline, kind):
    for k in KINDS:
        rig.run(k)
    rig.ctx.set_exact_only(True)
    try:
        rig.run(kind)
    finally:
        rig.ctx.set_exact_only(False)
    want = dict(baseline)
    want[kind] = 0
    assert rig.counters() == want
    rig.run(kind)
    assert rig.counters() == baseline


def test_a_trace_of_zero_rays_touches_no_counter(rig, baseline):
    for k in KINDS:
        rig.run(k)
    rig.ctx.trace_closest(rig.scene_desc, rig.rays, 0, rig.hits, rig.sets)
    assert rig.counters() == baseline
    # ... and behind an exact-only batch, whose count is 0, it is still 0
    rig.ctx.set_exact_only(True)
    try:
        rig.run("trace")
    finally:
        rig.ctx.set_exact_only(False)
    rig.ctx.trace_closest(rig.scene_desc, rig.rays, 0, rig.hits, rig.sets)
    want = dict(baseline)
    want["trace"] = 0
    assert rig.counters() == want
