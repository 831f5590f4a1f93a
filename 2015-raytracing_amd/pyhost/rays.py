"""Ray queries on torch tensors: the closest hit, or occlusion, of rays the caller holds as a cuda tensor (mirt_trace_closest,
mirt_trace_occluded; the definition is include/mirt.h's).

The tensors are not copied: each is wrapped as a buffer of the context (Context.wrap) for the length of the call, and the launches are queued on
torch's CURRENT stream (Context.set_stream), so they are ordered after whatever produced `rays` there and before whatever reads the result there.

    rays  float32 [N, 8], contiguous, on the context's device: o.xyz, mint, d.xyz, maxt per row (d is not normalised: t is in units of |d|)
    hits  float32 [N, 8]: normal.xyz, t, p.xyz, and the material id in column 7 -- hits[:, 7].view(torch.int32); -1 is a miss
    sets  int32 [N] (uint32 bits: the index of the set whose primitive won, -1 = 0xFFFFFFFF for a miss)
    occluded  uint8 [N]: 1 iff something blocks the ray (a ray with mint == maxt is reported 1)
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
