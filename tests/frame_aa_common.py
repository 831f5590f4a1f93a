"""The anti-aliased frame of mirt_render_frame_aa (include/mirt.h) restated in numpy, for tests/test_frame_aa.py and tests/frame_aa_child.py.
The FINE frame of a W x H job at `aa` samples per axis is the same job with aa*W columns and aa*H rows and nothing else changed -- the camera window
(cam[12], cam[13]) is given in scene space, so the frustum stays -- and the anti-aliased frame is the integer box average of the fine frame's bytes."""
import numpy as np

SIZES = [(1, 1), (5, 1), (1, 7), (37, 23)]   # outputs no tile of either structure of the kernel divides
AAS = [2, 3, 4]


def _sized(d, w, h):
    cam = list(d["cam"])
    cam[14], cam[15] = float(w), float(h)
    return dict(d, width=int(w), height=int(h), cam=cam)


def coarse_job(d, W, H):
    """the job dict `d` at W x H pixels: width, height, cam[14] and cam[15] change, nothing else"""
    return _sized(d, W, H)


def fine_job(d, W, H, aa):
    """the job dict whose frame is the FINE frame of coarse_job(d, W, H) at aa samples per axis"""
    return _sized(d, aa * W, aa * H)


def box_sums(fine_pixels, W, H, aa):
    """[H, W, 3] integer sums of the R, G, B bytes of each output pixel's aa x aa fine pixels"""
    f = np.asarray(fine_pixels, np.uint8).reshape(H, aa, W, aa, 4).astype(np.uint32)
    return f[..., :3].sum(axis=(1, 3))


def box(fine_pixels, W, H, aa):
    """[W*H, 4] uint8: per channel (S + floor(aa*aa / 2)) div (aa*aa) of the sum S over the pixel's aa x aa fine bytes; alpha 255"""
    n = aa * aa
    out = np.full((H, W, 4), 255, np.uint8)
    out[..., :3] = ((box_sums(fine_pixels, W, H, aa) + n // 2) // n).astype(np.uint8)
    return out.reshape(-1, 4)


def coverage(fine_pixels, W, H, aa):
    """(share of output pixels whose samples differ among themselves, number of output pixels with a channel sum aa*aa does not divide)"""
    f = np.asarray(fine_pixels, np.uint8).reshape(H, aa, W, aa, 4)[..., :3]
    mixed = (f.max(axis=(1, 3)) != f.min(axis=(1, 3))).any(axis=-1)
    undivided = (box_sums(fine_pixels, W, H, aa) % (aa * aa) != 0).any(axis=-1)
    return float(mixed.mean()), int(undivided.sum())
