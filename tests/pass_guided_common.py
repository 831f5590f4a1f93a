"""Shared by tests/test_pass_guided.py and tests/pass_guided_child.py: mirt_render_first_pass_guided against the two calls it stands for.

Two renderers over the same scene, tile and seeds: one runs the guided call, the other mirt_render_first_pass and then mirt_render_guides.
Every buffer the caller passes -- seeds, acu if kept, pixel, radiance, normal_hits, albedo_depth -- is compared as bits (every NaN equal to
every NaN), the guide buffers filled with a pattern first so that a pixel nobody wrote shows."""
import numpy as np

import a10_pass as A
from guides_common import difference

PATTERN = np.float32(7.5)


def packed(name, w, h, rpp):
    from conftest import load_fixture
    from raytracing_amd.pyhost import scene
    _, sc0 = load_fixture(name)
    return scene.PackedScene(dict(sc0.d)).resized(w, h, rpp)


def two_calls(ctx, fr, bounces=5):
    """mirt_render_first_pass, then mirt_render_guides, on renderer `fr`: -> (normal_hits, albedo_depth) float32 [pixels, 4]"""
    nh, ad = ctx.buffer(fr.npix * 16), ctx.buffer(fr.npix * 16)
    try:
        fill = np.full(4 * fr.npix, PATTERN, np.float32)
        nh.write(fill)
        ad.write(fill)
        d = fr.dev.pass_desc(fr.seeds, fr.acu, fr.pixel, fr.radiance, pass_index=1, bounces=bounces, row0=fr.row0, nrows=fr.nrows)
        ctx.render_pass(d, fresh=True)
        ctx.render_guides(d, nh, ad)
        return nh.read(np.float32).reshape(-1, 4), ad.read(np.float32).reshape(-1, 4)
    finally:
        nh.release()
        ad.release()


def guided(ctx, fr, bounces=5, outputs=(True, True)):
    """mirt_render_first_pass_guided on renderer `fr`: -> (normal_hits, albedo_depth); an output not asked for comes back as the pattern"""
    nh, ad = ctx.buffer(fr.npix * 16), ctx.buffer(fr.npix * 16)
    try:
        fill = np.full(4 * fr.npix, PATTERN, np.float32)
        nh.write(fill)
        ad.write(fill)
        d = fr.dev.pass_desc(fr.seeds, fr.acu, fr.pixel, fr.radiance, pass_index=1, bounces=bounces, row0=fr.row0, nrows=fr.nrows)
        ctx.render_first_pass_guided(d, nh if outputs[0] else None, ad if outputs[1] else None)
        return nh.read(np.float32).reshape(-1, 4), ad.read(np.float32).reshape(-1, 4)
    finally:
        nh.release()
        ad.release()


def compare(ctx, ps, tag, keep_acu=True, row0=0, nrows=None, seed_base=5, ref_ctx=None, want_radiance=True):
    """-> (first difference or None, calls that took the one-launch route, blocks or samples the guided pass deferred, the guided call's guides)"""
    from raytracing_amd.pyhost import render
    seeds = A.make_seeds(ps.total_rays, seed_base=seed_base)
    a = render.FusedRenderer(ctx, ps, seeds=seeds, row0=row0, nrows=nrows, keep_acu=keep_acu, want_radiance=want_radiance)
    b = render.FusedRenderer(ref_ctx or ctx, ps, seeds=seeds, row0=row0, nrows=nrows, keep_acu=keep_acu, want_radiance=want_radiance)
    try:
        before = ctx.guided_passes()
        got = guided(ctx, a)
        routed = ctx.guided_passes() - before
        deferred = ctx.pass_deferred()
        want = two_calls(ref_ctx or ctx, b)
        diff = None
        for name, g, w in (("normal_hits", got[0], want[0]), ("albedo_depth", got[1], want[1])):
            diff = diff or difference(f"{tag} {name}", g, w)
        if not np.array_equal(a.seeds.read(np.int32), b.seeds.read(np.int32)):
            diff = diff or f"{tag}: seeds differ"
        if not np.array_equal(a.pixel.read(np.uint8), b.pixel.read(np.uint8)):
            diff = diff or f"{tag}: pixel differs"
        if want_radiance:
            diff = diff or difference(f"{tag} radiance", a.radiance.read(np.float32), b.radiance.read(np.float32))
        if keep_acu:
            diff = diff or difference(f"{tag} acu", a.acu.read(np.float32), b.acu.read(np.float32))
        return diff, routed, deferred, got
    finally:
        a.release()
        b.release()
