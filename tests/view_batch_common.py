"""Shared by the batched view-camera tests (mirt_view_rays_batch, mirt_render_view_batch): the definition by composition, restated on the
single-camera helpers of tests/view_common.py.

  batch_rays      the batch's rays are view_common.view_rays per camera, concatenated
  expected_batch  the expected frames are view_common.expected_view per frame, on that frame's slice of the seeds (and of the carry)
  cameras         the three standard cameras: the oblique standard basis at the box centre, a second eye with a rotated basis, and a third
                  with an un-normalised, non-orthogonal basis
  BatchRenderer   view_common.Renderer with run_batch: the batch call on sentinel-tailed buffers, and singles(): the same library's N single calls
"""
import numpy as np

import view_common as V

f32 = np.float32


def cameras(sc, n=3):
    """-> float32 [n, 12]: eye, right, up, forward per frame (n <= 3 takes the first n; more repeat them at shifted eyes)"""
    b = np.asarray(sc.bounds, np.float64)
    lo, hi = b[0:3], b[4:7]
    c, ext = (lo + hi) / 2, hi - lo
    right, up, fwd = V.standard_basis()
    a = 0.7   # a rotation about y by 0.7 rad, then a tilt: still orthonormal in double
    r2 = np.array([np.cos(a), 0.0, -np.sin(a)])
    f2 = np.array([-np.sin(a) * np.cos(0.3), -np.sin(0.3), -np.cos(a) * np.cos(0.3)])
    u2 = np.cross(r2, f2)
    base = [np.concatenate([c, right, up, fwd]),
            np.concatenate([c + ext * [0.2, -0.15, 0.1], r2, u2, f2]),
            np.concatenate([c + ext * [-0.25, 0.1, -0.2], [1.7, 0.2, 0.0], [0.3, 0.6, 0.1], [0.25, -0.4, -2.0]])]
    out = [base[i % 3].copy() for i in range(n)]
    for i in range(3, n):
        out[i][0:3] += ext * 0.03 * (i // 3) * np.array([1.0, -1.0, 0.5])
    return np.asarray(out, np.float64).astype(f32)


def frame_view(view, cam):
    """`view` with eye / right / up / forward replaced by one row of the camera table"""
    cam = np.asarray(cam, f32)
    return view.with_(eye=cam[0:3].copy(), right=cam[3:6].copy(), up=cam[6:9].copy(), forward=cam[9:12].copy())


def batch_rays(view, cams):
    return np.concatenate([V.view_rays(frame_view(view, c)) for c in cams], axis=0) if len(cams) else np.zeros((0, 8), f32)


def expected_batch(sc, view, cams, seeds, bounces, carry=None):
    """-> (seeds [N * R], radiance [N * P, 4], pixel [N * P, 4]) through the oracle, frame by frame"""
    R, P = view.n_rays, view.n_pixels
    parts = [V.expected_view(sc, frame_view(view, c), seeds[f * R:(f + 1) * R], bounces, carry=None if carry is None else carry[f * P:(f + 1) * P])
             for f, c in enumerate(cams)]
    return tuple(np.concatenate([p[i] for p in parts], axis=0) for i in range(3))


class BatchRenderer(V.Renderer):
    def run_batch(self, view, cams, seeds, bounces=2, carry=None, prefill=None, radiance=True, pixel=True):
        """as Renderer.run, of the N frames: -> (seeds, radiance or None, pixel or None, untouched)"""
        nf = len(cams)
        n, npx = nf * view.n_rays, nf * view.n_pixels
        s = np.full(self.seeds.nbytes, V.SENTINEL, np.uint8)
        s[:n * 4] = np.ascontiguousarray(seeds, np.int32).view(np.uint8)
        r = np.full(self.radiance.nbytes, V.SENTINEL, np.uint8)
        for pre in (carry, prefill):
            if pre is not None:
                r[:npx * 16] = np.ascontiguousarray(pre, f32).reshape(-1).view(np.uint8)
        self.seeds.write(s)
        self.radiance.write(r)
        self.pixel.write(np.full(self.pixel.nbytes, V.SENTINEL, np.uint8))
        self.ctx.render_view_batch(self.scene_desc(bounces), view.desc(V.ACCUMULATE if carry is not None else 0), cams, self.seeds,
                                   self.radiance if radiance else None, self.pixel if pixel else None)
        s2, r2, p2 = self.seeds.read(np.uint8), self.radiance.read(np.uint8), self.pixel.read(np.uint8)
        clean = bool((s2[n * 4:] == V.SENTINEL).all() and (r2[npx * 16:] == V.SENTINEL).all() and (p2[npx * 4:] == V.SENTINEL).all())
        if not radiance:
            clean = clean and bool((r2 == r).all())
        if not pixel:
            clean = clean and bool((p2 == V.SENTINEL).all())
        return (s2[:n * 4].view(np.int32).copy(), r2[:npx * 16].view(f32).reshape(-1, 4).copy() if radiance else None,
                p2[:npx * 4].reshape(-1, 4).copy() if pixel else None, clean)

    def singles(self, view, cams, seeds, bounces=2, carry=None, radiance=True, pixel=True):
        """this library's own N single calls (mirt_render_view), each on its slice: -> (seeds, radiance or None, pixel or None)"""
        R, P = view.n_rays, view.n_pixels
        parts = []
        for f, c in enumerate(cams):
            got = self.run(frame_view(view, c), seeds[f * R:(f + 1) * R], bounces=bounces, carry=None if carry is None else carry[f * P:(f + 1) * P],
                           radiance=radiance, pixel=pixel)
            assert got[3], f"single call of frame {f}: bytes behind the records were written"
            parts.append(got)
        return tuple(None if parts[0][i] is None else np.concatenate([p[i] for p in parts], axis=0) for i in range(3))
