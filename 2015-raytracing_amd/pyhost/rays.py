"""Ray queries on torch tensors: the closest hit, occlusion, or the path radiance of rays the caller holds as a cuda tensor (mirt_trace_closest,
mirt_trace_occluded, mirt_trace_radiance; the definitions are include/mirt.h's) -- and, beside trace_radiance, render_view: a frame of a
panoramic, fisheye or orthographic camera into cuda tensors (mirt_render_view), view_guides: its first-hit guides (mirt_view_guides),
view_ao: its ambient occlusion (mirt_view_ao), and
denoised_view: progressive frames, the guides from the first (mirt_render_view_guided), and the a-trous filter behind the last.

The tensors are not copied: each is wrapped as a buffer of the context (Context.wrap) for the length of the call, and the launches are queued on
torch's CURRENT stream (Context.set_stream), so they are ordered after whatever produced `rays` there and before whatever reads the result there.

    rays  float32 [N, 8], contiguous, on the context's device: o.xyz, mint, d.xyz, maxt per row (d is not normalised: t is in units of |d|)
    hits  float32 [N, 8]: normal.xyz, t, p.xyz, and the material id in column 7 -- hits[:, 7].view(torch.int32); -1 is a miss
    sets  int32 [N] (uint32 bits: the index of the set whose primitive won, -1 = 0xFFFFFFFF for a miss)
    occluded  uint8 [N]: 1 iff something blocks the ray (a ray with mint == maxt is reported 1)
    seeds     int32 [N], contiguous: a ray's random sequence, advanced in place by trace_radiance
    radiance  float32 [N, 4]: a ray's accumulator -- rgb sums and, in column 3, the number of contributions
"""
import torch


def _check(ctx, rays):
    if not (isinstance(rays, torch.Tensor) and rays.is_cuda and rays.dtype == torch.float32 and rays.dim() == 2 and rays.shape[1] == 8 and rays.is_contiguous()):
        raise ValueError("rays: a contiguous float32 cuda tensor [N, 8] (o.xyz, mint, d.xyz, maxt)")
    if rays.device.index != ctx.device:
        raise ValueError(f"rays live on cuda:{rays.device.index}, the context on device {ctx.device}")


class _OnTorchStream:
    """the context's launches go to torch's current stream inside the block, and back to the context's own afterwards"""

    def __init__(self, ctx, device):
        self.ctx, self.device = ctx, device

    def __enter__(self):
        self.ctx.set_stream(torch.cuda.current_stream(self.device).cuda_stream)

    def __exit__(self, *exc):
        self.ctx.set_stream(None)   # (waits for the stream it leaves: the wrapped handles can be released)


def trace_closest(ctx, dev_scene, rays, want_sets=False):
    """-> hits [N, 8] float32, or (hits, sets) with want_sets.  dev_scene: a mirt.DeviceScene of `ctx`."""
    _check(ctx, rays)
    n = rays.shape[0]
    hits = torch.empty((n, 8), dtype=torch.float32, device=rays.device)
    sets = torch.empty((n,), dtype=torch.int32, device=rays.device) if want_sets else None
    if n:
        with _OnTorchStream(ctx, rays.device):
            wrapped = [ctx.wrap(rays.data_ptr(), n * 32), ctx.wrap(hits.data_ptr(), n * 32)] + ([ctx.wrap(sets.data_ptr(), n * 4)] if want_sets else [])
            try:
                ctx.trace_closest(dev_scene.pass_desc(None, None), wrapped[0], n, wrapped[1], wrapped[2] if want_sets else None)
            finally:
                for b in wrapped:
                    b.release()
    return (hits, sets) if want_sets else hits


def trace_occluded(ctx, dev_scene, rays):
    """-> occluded [N] uint8"""
    _check(ctx, rays)
    n = rays.shape[0]
    occluded = torch.empty((n,), dtype=torch.uint8, device=rays.device)
    if n:
        with _OnTorchStream(ctx, rays.device):
            wrapped = [ctx.wrap(rays.data_ptr(), n * 32), ctx.wrap(occluded.data_ptr(), n)]
            try:
                ctx.trace_occluded(dev_scene.pass_desc(None, None), wrapped[0], n, wrapped[1])
            finally:
                for b in wrapped:
                    b.release()
    return occluded


def trace_radiance(ctx, dev_scene, rays, seeds, samples=1, bounces=5, accumulate_into=None, emitters=True):
    """-> radiance [N, 4] float32: the pass's path from each ray on, `samples` times per ray (mirt_trace_radiance).  seeds: int32 cuda [N],
    advanced in place.  accumulate_into: a float32 cuda [N, 4] of accumulators to continue (written in place and returned).  emitters=False: the
    rays continue paths whose vertices already sampled the lights (MIRT_RADIANCE_NO_EMITTERS)."""
    from . import mirt
    _check(ctx, rays)
    n = rays.shape[0]
    if not (isinstance(seeds, torch.Tensor) and seeds.is_cuda and seeds.dtype == torch.int32 and seeds.shape == (n,) and seeds.is_contiguous() and seeds.device == rays.device):
        raise ValueError("seeds: a contiguous int32 cuda tensor [N] on the rays' device")
    out = accumulate_into
    if out is None:
        out = torch.empty((n, 4), dtype=torch.float32, device=rays.device)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.shape == (n, 4) and out.is_contiguous() and out.device == rays.device):
        raise ValueError("accumulate_into: a contiguous float32 cuda tensor [N, 4] on the rays' device")
    flags = (mirt.RADIANCE_ACCUMULATE if accumulate_into is not None else 0) | (0 if emitters else mirt.RADIANCE_NO_EMITTERS)
    if n:
        with _OnTorchStream(ctx, rays.device):
            wrapped = [ctx.wrap(rays.data_ptr(), n * 32), ctx.wrap(seeds.data_ptr(), n * 4), ctx.wrap(out.data_ptr(), n * 16)]
            try:
                ctx.trace_radiance(dev_scene.pass_desc(None, None, bounces=bounces), wrapped[0], n, wrapped[1], wrapped[2], samples=samples, flags=flags)
            finally:
                for b in wrapped:
                    b.release()
    return out


def view_guides(ctx, dev_scene, view):
    """-> (normal_hits, albedo_depth), float32 cuda [rows * width, 4] each on the context's device: the first-hit guides of a panoramic, fisheye
    or orthographic camera's frame (or row tile) in one launch (mirt_view_guides).  view: mirt.view_desc(...)."""
    npix = (view.nrows or view.height) * view.width
    device = torch.device("cuda", ctx.device)
    nh = torch.empty((npix, 4), dtype=torch.float32, device=device)
    ad = torch.empty((npix, 4), dtype=torch.float32, device=device)
    with _OnTorchStream(ctx, device):
        wrapped = [ctx.wrap(nh.data_ptr(), npix * 16), ctx.wrap(ad.data_ptr(), npix * 16)]
        try:
            ctx.view_guides(dev_scene.pass_desc(None, None), view, wrapped[0], wrapped[1])
        finally:
            for b in wrapped:
                b.release()
    return nh, ad


def view_ao(ctx, dev_scene, view, seeds, samples=None, radius=float("inf"), bias=None):
    """-> ao, uint32 cuda [rows * width, 2] on the context's device: {open, cast} per pixel of a panoramic, fisheye or orthographic camera's frame
    (or row tile) in one launch (mirt_view_ao).  view: mirt.view_desc(...).  seeds: int32 cuda [rows * width * k * k], read and not written.
    samples / bias left None are MIRT_AO_DEFAULT_*."""
    from . import mirt
    npix = (view.nrows or view.height) * view.width
    n = npix * view.k * view.k
    if not (isinstance(seeds, torch.Tensor) and seeds.is_cuda and seeds.dtype == torch.int32 and seeds.shape == (n,) and seeds.is_contiguous()):
        raise ValueError(f"seeds: a contiguous int32 cuda tensor [{n}]")
    if seeds.device.index != ctx.device:
        raise ValueError(f"seeds live on cuda:{seeds.device.index}, the context on device {ctx.device}")
    ao = torch.empty((npix, 2), dtype=torch.uint32, device=seeds.device)
    with _OnTorchStream(ctx, seeds.device):
        wrapped = [ctx.wrap(seeds.data_ptr(), n * 4), ctx.wrap(ao.data_ptr(), npix * 8)]
        try:
            ctx.view_ao(dev_scene.pass_desc(None, None), view, wrapped[0], wrapped[1], samples=mirt.AO_DEFAULT_SAMPLES if samples is None else samples, radius=radius,
                        bias=mirt.AO_DEFAULT_BIAS if bias is None else bias)
        finally:
            for b in wrapped:
                b.release()
    return ao


def render_view(ctx, dev_scene, view, seeds, bounces=5, accumulate_into=None, want_pixel=False, want_guides=False):
    """-> radiance [rows * width, 4] float32, or (radiance, pixel [rows * width, 4] uint8) with want_pixel: a frame (or row tile) of a panoramic,
    fisheye or orthographic camera in one launch (mirt_render_view).  view: mirt.view_desc(...); its ACCUMULATE flag is set here from
    accumulate_into, a float32 cuda [rows * width, 4] of sums to continue (written in place and returned).  seeds: int32 cuda [rows * width * k * k],
    advanced in place.  want_guides: the frame's first-hit guides too (mirt_render_view_guided) -- the result ends with normal_hits and
    albedo_depth, float32 [rows * width, 4] each."""
    from . import mirt
    rows = view.nrows or view.height
    npix = rows * view.width
    n = npix * view.k * view.k
    if not (isinstance(seeds, torch.Tensor) and seeds.is_cuda and seeds.dtype == torch.int32 and seeds.shape == (n,) and seeds.is_contiguous()):
        raise ValueError(f"seeds: a contiguous int32 cuda tensor [{n}]")
    if seeds.device.index != ctx.device:
        raise ValueError(f"seeds live on cuda:{seeds.device.index}, the context on device {ctx.device}")
    out = accumulate_into
    if out is None:
        out = torch.empty((npix, 4), dtype=torch.float32, device=seeds.device)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.shape == (npix, 4) and out.is_contiguous() and out.device == seeds.device):
        raise ValueError("accumulate_into: a contiguous float32 cuda tensor [rows * width, 4] on the seeds' device")
    pixel = torch.empty((npix, 4), dtype=torch.uint8, device=seeds.device) if want_pixel else None
    guides = [torch.empty((npix, 4), dtype=torch.float32, device=seeds.device) for _ in range(2)] if want_guides else []
    view.flags = mirt.VIEW_ACCUMULATE if accumulate_into is not None else 0
    with _OnTorchStream(ctx, seeds.device):
        wrapped = [ctx.wrap(seeds.data_ptr(), n * 4), ctx.wrap(out.data_ptr(), npix * 16)] + ([ctx.wrap(pixel.data_ptr(), npix * 4)] if want_pixel else [])
        gw = [ctx.wrap(g.data_ptr(), npix * 16) for g in guides]
        try:
            desc = dev_scene.pass_desc(None, None, bounces=bounces)
            if want_guides:
                ctx.render_view_guided(desc, view, wrapped[0], wrapped[1], wrapped[2] if want_pixel else None, gw[0], gw[1])
            else:
                ctx.render_view(desc, view, wrapped[0], wrapped[1], wrapped[2] if want_pixel else None)
        finally:
            for b in wrapped + gw:
                b.release()
    result = (out,) + ((pixel,) if want_pixel else ()) + tuple(guides)
    return result if len(result) > 1 else out


def denoised_view(ctx, dev_scene, view, seeds, passes=1, bounces=5, **filter_params):
    """-> (filtered [rows * width, 4] float32, pixel [rows * width, 4] uint8): `passes` progressive frames of a WHOLE view-camera image -- the
    first through mirt_render_view_guided, which leaves the guides too, the later ones plain with ACCUMULATE -- and then, once, the a-trous
    filter (mirt_filter_atrous) with the shipped defaults and tone = 1 / (rpp * passes); filter_params override the defaults.  Nothing leaves
    the device.  seeds: int32 cuda [height * width * k * k], advanced in place."""
    if view.row0 or (view.nrows and view.nrows != view.height):
        raise ValueError("denoised_view filters a whole image: view.row0 and view.nrows must be 0")
    if passes < 1:
        raise ValueError("passes >= 1")
    npix = view.height * view.width
    radiance, nh, ad = render_view(ctx, dev_scene, view, seeds, bounces=bounces, want_guides=True)
    for _ in range(1, passes):
        render_view(ctx, dev_scene, view, seeds, bounces=bounces, accumulate_into=radiance)
    filtered = torch.empty((npix, 4), dtype=torch.float32, device=seeds.device)
    pixel = torch.empty((npix, 4), dtype=torch.uint8, device=seeds.device)
    with _OnTorchStream(ctx, seeds.device):
        wrapped = [ctx.wrap(t.data_ptr(), t.numel() * t.element_size()) for t in (radiance, nh, ad, filtered, pixel)]
        try:
            ctx.filter_atrous(view.width, view.height, 1.0 / (view.k * view.k * passes), *wrapped, **filter_params)
        finally:
            for b in wrapped:
                b.release()
    return filtered, pixel
