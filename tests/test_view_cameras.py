"""GPU: mirt_view_rays and mirt_render_view on generated input -- the catalogue of tests/view_cameras_common.py on the stratified random scenes,
every frame against the CPU oracle (view_cameras_common.frame: view_common.view_rays, radiance_common.expected_radiance, the sequential fold, the
tone map), tolerance 0 (view_common.differ), sentinel bytes behind every record (view_common.Renderer).  What keeps these from passing on
emptiness is tests/test_view_cameras_conditions.py.

  1. mirt_view_rays against the numpy restatement for every camera of the catalogue, the 65535-wide and the 65535-high image included;
  2. every stratum x three models, oblique, bounces 2, under the optimistic / exact pair and under set_exact_only(True) -- GRIDS 0, 1 and 2, the
     staged single cells around 96 records, 18 sets; `staged` and `unstaged` at bounces 0 and 5 as well;
  3. k = 1, 4, 8, 16 (256, 16, 4, 1 pixels a block), EQUIRECT and FISHEYE, on single_cell, staged, unstaged and many_sets;
  4. every edge camera on staged, single_cell and guard; all_refused has mirt_view_deferred == every block, and 0 under exact_only;
  5. MIXED frames (axis_*, mixed_k*) on every enclosed stratum: the frame equals the oracle and mirt_view_deferred is at least 256 x the blocks
     that hold a ray the guard refuses (printed; a grid walk may defer more); then, on the same frames, three progressive calls with
     MIRT_VIEW_ACCUMULATE chained from the GPU's own seeds and sums, a row tile whose first block is clean (fresh and from a carry), pixel
     only, radiance only; and all_refused followed by oblique on the same context -- a mask left over from the call before.
"""
import numpy as np
import pytest

import rays_common as R
import view_cameras_common as VC
import view_common as V
from conftest import bits

pytestmark = pytest.mark.gpu

CAP_RAYS = max(VC.view("staged", n).n_rays for n in VC.CAMERAS)
CAP_PIXELS = max(VC.view("staged", n).n_pixels for n in VC.CAMERAS)


@pytest.fixture(scope="module")
def ctx(pkg):
    from raytracing_amd.pyhost import mirt
    c = mirt.Context(0)
    yield c
    c.destroy()


@pytest.fixture(scope="module")
def renderers(ctx):
    made = {}

    def get(stratum):
        if stratum not in made:
            made[stratum] = V.Renderer(ctx, R.scene(stratum), CAP_RAYS, CAP_PIXELS)
        return made[stratum]
    yield get
    for r in made.values():
        r.release()


def check(tag, r, view, seeds, want, **kw):
    got = r.run(view, seeds, **kw)
    d = V.differ(tag, got, want)
    assert d is None, d
    assert got[3], f"{tag}: bytes behind the records, or a buffer that was not given, were written"
    return got


def pair_and_exact(ctx, r, tag, view, seeds, want, bounces, refused=None):
    """the frame under the optimistic / exact pair, then under set_exact_only; -> the rays the pair deferred"""
    check(f"{tag}, pair", r, view, seeds, want, bounces=bounces)
    deferred = ctx.view_deferred()
    assert deferred % 256 == 0 and deferred <= VC.n_blocks(view) * 256
    if refused is not None:
        assert deferred >= 256 * len(refused), f"{tag}: {deferred} rays deferred, {len(refused)} blocks hold a ray the guard refuses"
    ctx.set_exact_only(True)
    try:
        check(f"{tag}, exact_only", r, view, seeds, want, bounces=bounces)
        assert ctx.view_deferred() == 0, "the exact kernel alone defers nothing"
    finally:
        ctx.set_exact_only(False)
    return deferred


# ---- 1. the rays ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(VC.CAMERAS) + list(VC.RAYS_ONLY))
def test_view_rays_equal_the_restatement(ctx, name):
    v = VC.view("guard", name)
    n, tail = v.n_rays, 96
    buf = ctx.buffer(n * 32 + tail)
    try:
        buf.write(np.full(buf.nbytes, V.SENTINEL, np.uint8))
        ctx.view_rays(v.desc(), buf)
        raw = buf.read(np.uint8)
        got, want = raw[:n * 32].view(np.float32).reshape(-1, 8), V.view_rays(v)
        bad = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
        assert bad.size == 0, f"{name}: {bad.size} of {n} rays differ; first is ray {int(bad[0])}: got {got[bad[0]].tolist()}, want {want[bad[0]].tolist()}"
        assert (raw[n * 32:] == V.SENTINEL).all(), "bytes behind the records were written"
    finally:
        buf.release()


# ---- 2. every stratum, the three models ------------------------------------------------------------------------------------------------------------
OBLIQUE_CASES = [(s, VC.BOUNCES) for s in VC.STRATA] + [(s, b) for s in ("staged", "unstaged") for b in (0, 5)]


@pytest.mark.parametrize("name", VC.OBLIQUE)
@pytest.mark.parametrize("stratum,bounces", OBLIQUE_CASES)
def test_oblique_frames_equal_the_oracle(ctx, renderers, stratum, bounces, name):
    fr = VC.frame(stratum, name, bounces)
    v = fr.view
    deferred = pair_and_exact(ctx, renderers(stratum), f"{stratum} {name} bounces {bounces}", v, VC.seeds_of(v.n_rays), fr.triple(), bounces,
                              refused=VC.blocks_of(fr.refused))
    print(f"view_deferred {stratum} {name} bounces {bounces}: {deferred} of {v.n_rays} rays")


# ---- 3. every k --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", VC.EVERY_K_NAMES)
@pytest.mark.parametrize("stratum", VC.EVERY_K_STRATA)
def test_every_k_equals_the_oracle(ctx, renderers, stratum, name):
    fr = VC.frame(stratum, name)
    v = fr.view
    pair_and_exact(ctx, renderers(stratum), f"{stratum} {name}", v, VC.seeds_of(v.n_rays), fr.triple(), VC.BOUNCES, refused=VC.blocks_of(fr.refused))


# ---- 4. the edge cameras -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", VC.EDGE)
@pytest.mark.parametrize("stratum", VC.EDGE_STRATA)
def test_edge_cameras_equal_the_oracle(ctx, renderers, stratum, name):
    fr = VC.frame(stratum, name)
    v = fr.view
    deferred = pair_and_exact(ctx, renderers(stratum), f"{stratum} {name}", v, VC.seeds_of(v.n_rays), fr.triple(), VC.BOUNCES,
                              refused=VC.blocks_of(fr.refused))
    if name == "all_refused":
        assert deferred == VC.n_blocks(v) * 256, "every block of the frame is the exact kernel's"
    print(f"view_deferred {stratum} {name}: {deferred} of {v.n_rays} rays")


# ---- 5. mixed frames -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", VC.MIXED)
@pytest.mark.parametrize("stratum", VC.ENCLOSED)
def test_mixed_frames_equal_the_oracle(ctx, renderers, stratum, name):
    fr = VC.frame(stratum, name)
    v, refused = fr.view, VC.blocks_of(fr.refused)
    assert 0 < len(refused) < VC.n_blocks(v)
    deferred = pair_and_exact(ctx, renderers(stratum), f"{stratum} {name}", v, VC.seeds_of(v.n_rays), fr.triple(), VC.BOUNCES, refused=refused)
    print(f"view_deferred {stratum} {name}: {deferred} of {v.n_rays} rays, {len(refused)} of {VC.n_blocks(v)} blocks hold a refused ray")


@pytest.mark.parametrize("name", VC.MIXED)
@pytest.mark.parametrize("stratum", VC.ENCLOSED)
def test_progressive_calls_continue_the_chain_over_mixed_frames(ctx, renderers, stratum, name):
    sc, r, base = R.scene(stratum), renderers(stratum), VC.view(stratum, name)
    seeds, carry = VC.seeds_of(base.n_rays), None
    for p in (1, 2, 3):
        v = base.with_(tone=1.0 / (base.rpp * p))
        fr = VC.frame(stratum, name) if p == 1 else VC.Frame(sc, v, seeds, VC.BOUNCES)
        refused = VC.blocks_of(fr.refused)
        assert 0 < len(refused) < VC.n_blocks(v), "the frame is partly deferred"
        got = check(f"{stratum} {name} frame {p}", r, v, seeds, fr.triple(carry=carry, tone=v.tone), bounces=VC.BOUNCES, carry=carry)
        assert ctx.view_deferred() >= 256 * len(refused)
        seeds, carry = got[0], got[1]
    assert (carry[:, 3] > 0).any()


@pytest.mark.parametrize("name", VC.MIXED)
@pytest.mark.parametrize("stratum", VC.ENCLOSED)
def test_tiles_and_single_outputs_of_mixed_frames(ctx, renderers, stratum, name):
    r, fr = renderers(stratum), VC.frame(stratum, name)
    v = fr.view
    seeds = VC.seeds_of(v.n_rays)
    sd, sums, px = fr.triple()
    # a row tile whose first block is clean: the blocks of the tile are not the frame's
    row0, nrows = VC.clean_tile(fr)
    per = v.width * v.rpp
    ry = slice(row0 * per, (row0 + nrows) * per)
    tile = v.tile(v.row0 + row0, nrows)
    tile_refused = VC.blocks_of(fr.refused[ry])
    assert 0 not in tile_refused and 0 < len(tile_refused) < VC.n_blocks(tile)
    check(f"{stratum} {name} rows [{row0}, +{nrows})", r, tile, seeds[ry], fr.rows(row0, nrows), bounces=VC.BOUNCES)
    assert ctx.view_deferred() >= 256 * len(tile_refused)
    # ... and from a carry
    carry = np.random.default_rng(12).uniform(0.0, 2.0, size=(tile.n_pixels, 4)).astype(np.float32)
    tsums = V.fold(fr.acc[ry], v.rpp, carry)
    check(f"{stratum} {name} rows [{row0}, +{nrows}) from a carry", r, tile, seeds[ry], (sd[ry], tsums, V.tone_rgba8(tsums, v.tone)), bounces=VC.BOUNCES, carry=carry)
    # one output alone
    check(f"{stratum} {name} pixel only", r, v, seeds, (sd, None, px), bounces=VC.BOUNCES, radiance=False)
    assert ctx.view_deferred() >= 256 * len(VC.blocks_of(fr.refused))
    check(f"{stratum} {name} radiance only", r, v.with_(tone=float("nan")), seeds, (sd, sums, None), bounces=VC.BOUNCES, pixel=False)
    # a fresh call over what an earlier one left in radiance ignores it, in the deferred blocks too
    pre = np.random.default_rng(13).uniform(0.0, 4.0, size=(v.n_pixels, 4)).astype(np.float32)
    check(f"{stratum} {name} fresh over a pre-filled buffer", r, v, seeds, (sd, sums, px), bounces=VC.BOUNCES, prefill=pre)


@pytest.mark.parametrize("stratum", VC.ENCLOSED)
def test_a_mask_left_over_from_the_call_before_is_not_read(ctx, renderers, stratum):
    """every bit of the mask is set by all_refused; the next call goes on from a carry, which a block run by BOTH kernels would add to twice"""
    r = renderers(stratum)
    full = VC.view(stratum, "all_refused")
    for name in VC.OBLIQUE + ("mixed_k2",):
        r.run(full, VC.seeds_of(full.n_rays), bounces=0)
        assert ctx.view_deferred() == VC.n_blocks(full) * 256
        fr = VC.frame(stratum, name)
        v = fr.view
        carry = np.random.default_rng(14).uniform(0.0, 2.0, size=(v.n_pixels, 4)).astype(np.float32)
        check(f"{stratum} {name} after a frame that was deferred whole", r, v, VC.seeds_of(v.n_rays), fr.triple(carry=carry), bounces=VC.BOUNCES, carry=carry)
        deferred = ctx.view_deferred()
        assert 256 * len(VC.blocks_of(fr.refused)) <= deferred <= VC.n_blocks(v) * 256
        print(f"view_deferred {stratum} {name} after all_refused: {deferred} of {v.n_rays} rays")
