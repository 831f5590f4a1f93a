"""Ray queries on torch tensors: the closest hit, occlusion, or the path radiance of rays the caller holds as a cuda tensor (mirt_trace_closest,
mirt_trace_occluded, mirt_trace_radiance; the definitions are include/mirt.h's) -- and, beside trace_radiance, render_view: a frame of a
panoramic, fisheye or orthographic camera into cuda tensors (mirt_render_view), view_guides: its first-hit guides (mirt_view_guides),
view_ao: its ambient occlusion (mirt_view_ao), and
denoised_view: progressive frames, the guides from the first (mirt_render_view_guided), and the a-trous filter behind the last;
render_views: the frames of N cameras in one launch (mirt_render_view_batch; with want_guides mirt_render_view_guided_batch),
view_guides_batch and view_ao_batch: their guides and ambient occlusion (mirt_view_guides_batch, mirt_view_ao_batch), probe_depth: the mean
distance to the first hit around N positions, and probe_sh: the order-2 spherical-harmonic coefficients of the
radiance arriving at N positions, from N small equirect frames and one matmul against sh9_basis.

The tensors are not copied: each is wrapped as a buffer of the context (Context.wrap) for the length of the call, and the launches are queued on
torch's CURRENT stream (Context.set_stream), so they are ordered after whatever produced `rays` there and before whatever reads the result there.

    rays  float32 [N, 8], contiguous, on the context's device: o.xyz, mint, d.xyz, maxt per row (d is not normalised: t is in units of |d|)
    hits  float32 [N, 8]: normal.xyz, t, p.xyz, and the material id in column 7 -- hits[:, 7].view(torch.int32); -1 is a miss
    sets  int32 [N] (uint32 bits: the index of the set whose primitive won, -1 = 0xFFFFFFFF for a miss)
    occluded  uint8 [N]: 1 iff something blocks the ray (a ray with mint == maxt is reported 1)
    seeds     int32 [N], contiguous: a ray's random sequence, advanced in place by trace_radiance
    radiance  float32 [N, 4]: a ray's accumulator -- rgb sums and, in column 3, the number of contributions
"""
import numpy as np
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


def _batch_cameras(view, cameras, who):
    """-> cameras as a contiguous float32 numpy [N, 12]; a cuda tensor is brought to the host (48 bytes a frame).  Whole frames only."""
    if isinstance(cameras, torch.Tensor):
        cameras = cameras.detach().cpu().numpy()
    cam = np.ascontiguousarray(np.asarray(cameras, np.float32))
    if cam.ndim != 2 or cam.shape[1] != 12:
        raise ValueError(f"cameras: expected [N, 12] floats (eye, right, up, forward per frame), got {cam.shape}")
    if view.row0 or (view.nrows and view.nrows != view.height):
        raise ValueError(f"{who} renders whole frames: view.row0 and view.nrows must be 0")
    return cam


def view_guides_batch(ctx, dev_scene, view, cameras):
    """-> (normal_hits, albedo_depth), float32 cuda [N, height, width, 4] each on the context's device: the first-hit guides of the whole frames
    of N cameras that share everything of `view` but the basis, in one launch (mirt_view_guides_batch).  cameras: as for render_views."""
    cam = _batch_cameras(view, cameras, "view_guides_batch")
    nf = cam.shape[0]
    npix = nf * view.height * view.width
    device = torch.device("cuda", ctx.device)
    nh = torch.empty((nf, view.height, view.width, 4), dtype=torch.float32, device=device)
    ad = torch.empty((nf, view.height, view.width, 4), dtype=torch.float32, device=device)
    if nf:
        with _OnTorchStream(ctx, device):
            wrapped = [ctx.wrap(nh.data_ptr(), npix * 16), ctx.wrap(ad.data_ptr(), npix * 16)]
            try:
                ctx.view_guides_batch(dev_scene.pass_desc(None, None), view, cam, wrapped[0], wrapped[1])
            finally:
                for b in wrapped:
                    b.release()
    return nh, ad


def view_ao_batch(ctx, dev_scene, view, cameras, seeds, samples=None, radius=float("inf"), bias=None):
    """-> ao, int32 cuda [N, height, width, 2] on the context's device: {open, cast} per pixel of the whole frames of N cameras, in one launch
    (mirt_view_ao_batch).  seeds: int32 cuda [N * height * width * k * k], frame after frame, read and not written.  samples / bias left None
    are MIRT_AO_DEFAULT_*."""
    from . import mirt
    cam = _batch_cameras(view, cameras, "view_ao_batch")
    nf = cam.shape[0]
    npix = nf * view.height * view.width
    n = npix * view.k * view.k
    if not (isinstance(seeds, torch.Tensor) and seeds.is_cuda and seeds.dtype == torch.int32 and seeds.shape == (n,) and seeds.is_contiguous()):
        raise ValueError(f"seeds: a contiguous int32 cuda tensor [{n}]")
    if seeds.device.index != ctx.device:
        raise ValueError(f"seeds live on cuda:{seeds.device.index}, the context on device {ctx.device}")
    ao = torch.empty((nf, view.height, view.width, 2), dtype=torch.int32, device=seeds.device)
    if nf:
        with _OnTorchStream(ctx, seeds.device):
            wrapped = [ctx.wrap(seeds.data_ptr(), n * 4), ctx.wrap(ao.data_ptr(), npix * 8)]
            try:
                ctx.view_ao_batch(dev_scene.pass_desc(None, None), view, cam, wrapped[0], wrapped[1], samples=mirt.AO_DEFAULT_SAMPLES if samples is None else samples,
                                  radius=radius, bias=mirt.AO_DEFAULT_BIAS if bias is None else bias)
            finally:
                for b in wrapped:
                    b.release()
    return ao


def render_views(ctx, dev_scene, view, cameras, seeds, bounces=5, accumulate_into=None, want_pixel=False, want_guides=False):
    """-> radiance [N, height, width, 4] float32 cuda, or (radiance, pixel [N, height, width, 4] uint8) with want_pixel: the whole frames of N
    cameras that share everything of `view` but the basis, in one launch (mirt_render_view_batch).  want_guides: the frames' first-hit guides
    too (mirt_render_view_guided_batch) -- the result ends with normal_hits and albedo_depth, float32 [N, height, width, 4] each.  cameras: anything np.asarray(..., float32)
    turns into [N, 12] -- eye, right, up, forward per frame; a cuda tensor is brought to the host (48 bytes a frame).  The call's ACCUMULATE flag
    comes from accumulate_into (view.flags is neither read nor changed), a float32 cuda [N, height, width, 4] of sums to continue (written in place and returned).  seeds: int32 cuda
    [N * height * width * k * k], frame after frame, advanced in place."""
    from . import mirt
    cam = _batch_cameras(view, cameras, "render_views")
    nf = cam.shape[0]
    npix = nf * view.height * view.width
    n = npix * view.k * view.k
    shape = (nf, view.height, view.width, 4)
    if not (isinstance(seeds, torch.Tensor) and seeds.is_cuda and seeds.dtype == torch.int32 and seeds.shape == (n,) and seeds.is_contiguous()):
        raise ValueError(f"seeds: a contiguous int32 cuda tensor [{n}]")
    if seeds.device.index != ctx.device:
        raise ValueError(f"seeds live on cuda:{seeds.device.index}, the context on device {ctx.device}")
    out = accumulate_into
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=seeds.device)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.shape == shape and out.is_contiguous() and out.device == seeds.device):
        raise ValueError("accumulate_into: a contiguous float32 cuda tensor [N, height, width, 4] on the seeds' device")
    pixel = torch.empty(shape, dtype=torch.uint8, device=seeds.device) if want_pixel else None
    guides = [torch.empty(shape, dtype=torch.float32, device=seeds.device) for _ in range(2)] if want_guides else []
    view = type(view).from_buffer_copy(view)   # the caller's descriptor keeps its flags
    view.flags = mirt.VIEW_ACCUMULATE if accumulate_into is not None else 0
    if nf:
        with _OnTorchStream(ctx, seeds.device):
            wrapped = [ctx.wrap(seeds.data_ptr(), n * 4), ctx.wrap(out.data_ptr(), npix * 16)] + ([ctx.wrap(pixel.data_ptr(), npix * 4)] if want_pixel else [])
            gw = [ctx.wrap(g.data_ptr(), npix * 16) for g in guides]
            try:
                desc = dev_scene.pass_desc(None, None, bounces=bounces)
                if want_guides:
                    ctx.render_view_guided_batch(desc, view, cam, wrapped[0], wrapped[1], wrapped[2] if want_pixel else None, gw[0], gw[1])
                else:
                    ctx.render_view_batch(desc, view, cam, wrapped[0], wrapped[1], wrapped[2] if want_pixel else None)
            finally:
                for b in wrapped + gw:
                    b.release()
    result = (out,) + ((pixel,) if want_pixel else ()) + tuple(guides)
    return result if len(result) > 1 else out


def sh9_directions(width, height):
    """-> (d [height * width, 3], latitude [height * width]) float64 numpy: the directions of the pixel CENTRES of a width x height EQUIRECT
    frame under include/mirt.h's formula with right = +x, up = +y, forward = -z, row-major like the frame."""
    x, y = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    a = 2.0 * (x + 0.5) / width - 1.0
    b = 1.0 - 2.0 * (y + 0.5) / height
    phi, th = (a * np.pi).ravel(), (b * (np.pi / 2)).ravel()
    lx, ly, lz = np.sin(phi) * np.cos(th), np.sin(th), np.cos(phi) * np.cos(th)
    return np.stack([lx, ly, -lz], axis=1), th


def sh9_weights(width, height):
    """-> w [height * width] float64 numpy: the solid-angle weights of those pixels, cos(latitude) scaled so that they sum to 4 pi"""
    w = np.cos(sh9_directions(width, height)[1])
    return w * (4.0 * np.pi / w.sum())


def sh9_basis(width, height):
    """-> B [height * width, 9] float64 numpy: the real orthonormal spherical harmonics of order 0..2 (index l * l + l + m) at those
    directions; integral of B_i * B_j over the sphere = delta_ij, which sum(w * B_i * B_j) with sh9_weights approaches at the midpoint rule's rate."""
    d = sh9_directions(width, height)[0]
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    c0, c1, c2, c3, c4 = 0.5 * np.sqrt(1.0 / np.pi), np.sqrt(3.0 / (4.0 * np.pi)), 0.5 * np.sqrt(15.0 / np.pi), 0.25 * np.sqrt(5.0 / np.pi), 0.25 * np.sqrt(15.0 / np.pi)
    return np.stack([np.full_like(x, c0), c1 * y, c1 * z, c1 * x, c2 * x * y, c2 * y * z, c3 * (3.0 * z * z - 1.0), c2 * x * z, c4 * (x * x - y * y)], axis=1)


def probe_sh(ctx, dev_scene, positions, width=32, height=16, k=2, passes=1, bounces=5, seeds=None):
    """-> [N, 9, 3] float32 cuda: the order-2 spherical-harmonic coefficients (sh9_basis's order) of the radiance arriving at each of the N
    positions ([N, 3]).  `passes` progressive batch calls of N width x height EQUIRECT frames at k x k samples with the basis right = +x, up =
    +y, forward = -z (render_views), then ONE matmul of the pixels' values -- sums.xyz / (k * k * passes) -- against sh9_weights * sh9_basis.
    seeds: int32 cuda [N * height * width * k * k], advanced in place; None draws them from mirt_seed_fill's sequence."""
    from . import mirt
    if isinstance(positions, torch.Tensor):
        positions = positions.detach().cpu().numpy()
    pos = np.asarray(positions, np.float32).reshape(-1, 3)
    if passes < 1:
        raise ValueError("passes >= 1")
    nf = pos.shape[0]
    cam = np.zeros((nf, 12), np.float32)
    cam[:, 0:3] = pos
    cam[:, 3], cam[:, 7], cam[:, 11] = 1.0, 1.0, -1.0
    device = torch.device("cuda", ctx.device)
    n = nf * height * width * k * k
    if seeds is None:
        seeds = torch.empty((n,), dtype=torch.int32, device=device)
        if n:
            with _OnTorchStream(ctx, device):
                w = ctx.wrap(seeds.data_ptr(), n * 4)
                try:
                    ctx.seed_fill(w, 0, n)
                finally:
                    w.release()
    view = mirt.view_desc(mirt.VIEW_EQUIRECT, width, height, k=k)
    sums = render_views(ctx, dev_scene, view, cam, seeds, bounces=bounces)
    for _ in range(1, passes):
        render_views(ctx, dev_scene, view, cam, seeds, bounces=bounces, accumulate_into=sums)
    m = (sh9_basis(width, height) * sh9_weights(width, height)[:, None] / (k * k * passes)).T   # [9, P], the pixel's scale folded in
    m = torch.from_numpy(np.ascontiguousarray(m.astype(np.float32))).to(device)
    return torch.matmul(m, sums.reshape(nf, height * width, 4)[:, :, :3])


def probe_depth(ctx, dev_scene, positions, width=32, height=16, k=1):
    """-> (mean_distance [N, height, width], hit_fraction [N, height, width]) float32 cuda: around each of the N positions ([N, 3]) the mean
    distance to the first hit of a pixel's k * k samples -- the visibility term of an irradiance volume -- and the fraction of the samples that
    hit.  N width x height EQUIRECT frames with probe_sh's unit basis (right = +x, up = +y, forward = -z), so depth is distance, in one launch
    (view_guides_batch); mean_distance = depth_sum / hits where hits > 0 and +inf elsewhere, hit_fraction = hits / (k * k)."""
    from . import mirt
    if isinstance(positions, torch.Tensor):
        positions = positions.detach().cpu().numpy()
    pos = np.asarray(positions, np.float32).reshape(-1, 3)
    cam = np.zeros((pos.shape[0], 12), np.float32)
    cam[:, 0:3] = pos
    cam[:, 3], cam[:, 7], cam[:, 11] = 1.0, 1.0, -1.0
    view = mirt.view_desc(mirt.VIEW_EQUIRECT, width, height, k=k)
    nh, ad = view_guides_batch(ctx, dev_scene, view, cam)
    hits, depth = nh[..., 3], ad[..., 3]
    mean = torch.where(hits > 0, depth / hits, torch.full_like(depth, float("inf")))
    return mean, hits / float(k * k)
