"""Shared by tests/test_passes_guided.py and tests/passes_guided_child.py: mirt_render_passes_guided against the two calls it stands for.

Two renderers over the same scene, tile and seeds: one runs the guided call, the other mirt_render_passes and then mirt_render_guides.  Every
buffer the caller passes -- seeds, acu if kept, pixel and radiance (n frames each with MIRT_PASSES_EVERY_FRAME), normal_hits, albedo_depth -- is
compared as bits (every NaN equal to every NaN), the guide and frame buffers filled with a pattern first so that a pixel nobody wrote shows."""
import numpy as np

import a10_pass as A
from guides_common import difference
from pass_guided_common import PATTERN, packed  # noqa: F401  (packed: for the importers)

BUFFERS = ("normal_hits", "albedo_depth", "pixel", "radiance", "seeds", "acu")


def run(ctx, fr, n, guided, fresh=True, every=False, outputs=(True, True), bounces=5):
    """n passes from fr.passes on and the guides, into buffers of this call's own (pattern-filled): the guided call, or mirt_render_passes and then
    mirt_render_guides.  -> {buffer name: array}; an output not asked for comes back as the pattern."""
    npix, frames = fr.npix, (n if every else 1)
    nh, ad = ctx.buffer(npix * 16), ctx.buffer(npix * 16)
    pixel, radiance = ctx.buffer(frames * npix * 4), ctx.buffer(frames * npix * 16)
    try:
        fill = np.full(4 * npix, PATTERN, np.float32)
        nh.write(fill)
        ad.write(fill)
        pixel.write(np.full(frames * npix * 4, 0x5A, np.uint8))
        radiance.write(np.full(frames * npix * 4, PATTERN, np.float32))
        d = fr.dev.pass_desc(fr.seeds, fr.acu, pixel, radiance, pass_index=fr.passes, bounces=bounces, row0=fr.row0, nrows=fr.nrows)
        if guided:
            ctx.render_passes_guided(d, n, fresh=fresh, every_frame=every, normal_hits=nh if outputs[0] else None, albedo_depth=ad if outputs[1] else None)
        else:
            ctx.render_passes(d, n, fresh=fresh, every_frame=every)
            ctx.render_guides(d, nh, ad)
        fr.passes += n
        out = {"normal_hits": nh.read(np.float32).reshape(-1, 4), "albedo_depth": ad.read(np.float32).reshape(-1, 4),
               "pixel": pixel.read(np.uint8), "radiance": radiance.read(np.float32), "seeds": fr.seeds.read(np.int32)}
        if fr.acu is not None:
            out["acu"] = fr.acu.read(np.float32)
        return out
    finally:
        for b in (nh, ad, pixel, radiance):
            b.release()


def first_difference(tag, got, want):
    assert got.keys() == want.keys()
    for name in BUFFERS:
        if name not in got:
            continue
        g, w = got[name], want[name]
        if g.dtype == np.float32:
            d = difference(f"{tag} {name}", g, w)
        else:
            d = None if np.array_equal(g, w) else f"{tag}: {name} differs"
        if d:
            return d
    return None


def compare(ctx, ps, tag, n, every=False, keep_acu=True, first_pass=False, row0=0, nrows=None, seed_base=5, ref_ctx=None):
    """first_pass: an ordinary fresh pass on both renderers first, so that the batch is not fresh and starts at pass_index 2 (needs keep_acu).
    -> (first difference or None, calls that took the one-launch route, blocks or samples the guided call deferred, the guided call's buffers)"""
    from raytracing_amd.pyhost import render
    seeds = A.make_seeds(ps.total_rays, seed_base=seed_base)
    a = render.FusedRenderer(ctx, ps, seeds=seeds, row0=row0, nrows=nrows, keep_acu=keep_acu)
    b = render.FusedRenderer(ref_ctx or ctx, ps, seeds=seeds, row0=row0, nrows=nrows, keep_acu=keep_acu)
    try:
        if first_pass:
            a.execute_render(fresh=True)
            b.execute_render(fresh=True)
        before = ctx.guided_passes()
        got = run(ctx, a, n, True, fresh=not first_pass, every=every)
        routed = ctx.guided_passes() - before
        deferred = ctx.pass_deferred()
        want = run(ref_ctx or ctx, b, n, False, fresh=not first_pass, every=every)
        return first_difference(tag, got, want), routed, deferred, got
    finally:
        a.release()
        b.release()
