"""Shared by tests/test_ao.py, tests/test_ao_abi.py, tests/test_ao_js.py and tests/ao_default_child.py: what mirt_render_ao is checked against.

The AO pair {open, cast} of a pixel is defined by composing kernels the reference already has (include/mirt.h), and this module restates it that
way with any checker `k` (a10_pass.load_oracle(), or ref_gpu.GpuRefKernels() for the reference binary on the device):

  guides_common.first_hit_state   initTrace and the closest-hit stage: the Poi buffer and the seeds (the k x k lens grid draws none)
  `samples` times                 k.bouncePaths on a SCRATCH ray buffer with the advancing copy of the seeds -- the Poi buffer is unchanged, so call j
                                  stores getHemisphereRay's j-th ray of every casting sample (Poi.matId >= 0) --, the casting samples' rays
                                  rewritten in numpy (bias: two np.float32 operations; mint 0; maxt radius), rays_common.expected_occluded, count.

Nothing here is tuned to the library: integers, tolerance 0."""
import numpy as np

import a10_pass as A
from guides_common import first_hit_state
from random_scenes_common import ROW_TILE   # rows 5..13 of 21
from rays_common import expected_occluded


def tile_seeds(sc, row0, nrows):
    """the seeds of a row tile: global ray ids, as mirt_seed_fill(first = row0 * width * rpp) fills them"""
    n = sc.width * nrows * sc.rpp
    return A.make_seeds(n, first=row0 * sc.width * sc.rpp)


def ao_rays(ray_buf, pois, cast, radius, bias):
    """The casting samples' AO rays [ncast, 8] {o, mint, d, maxt} from the rays bouncePaths stored: maxt = radius, and with a bias the origin
    p + (n * bias), each operation rounded to fp32 on its own"""
    r = np.zeros((int(cast.sum()), 8), np.float32)
    o = ray_buf["o"][cast].astype(np.float32)
    if bias != 0:
        with np.errstate(all="ignore"):
            step = (pois["normal"][cast].astype(np.float32) * np.float32(bias)).astype(np.float32)
            o = (pois["p"][cast].astype(np.float32) + step).astype(np.float32)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, np.float32(0.0), ray_buf["d"][cast], np.float32(radius)
    return r


def count_ao(cast, occluded_per_sample, rpp):
    """{open, cast} per pixel, uint32 [pixels, 2], from the casting mask [rays] and one occluded array [ncast] per AO sample"""
    samples = len(occluded_per_sample)
    open_ray = np.zeros(cast.shape[0], np.uint32)
    for occ in occluded_per_sample:
        open_ray[cast] += (np.asarray(occ) == 0).astype(np.uint32)
    out = np.zeros((cast.shape[0] // rpp, 2), np.uint32)
    out[:, 0] = open_ray.reshape(-1, rpp).sum(axis=1)
    out[:, 1] = cast.reshape(-1, rpp).sum(axis=1).astype(np.uint32) * np.uint32(samples)
    return out


def expected_ao(k, sc, samples, radius, bias, rows=None):
    """uint32 [pixels, 2] of the whole frame (rows: of its first `rows` rows), by the checker k"""
    st = first_hit_state(k, sc, rows)
    n = sc.width * (sc.height if rows is None else rows) * sc.rpp
    g1 = A._ceil(n, A.WAVE)
    B = k.buf
    seeds = st.seeds.copy()
    scratch = np.zeros(len(st.rays), A.RAY_DT)
    cast = st.pois["matId"][:n] >= 0
    occ = []
    for _ in range(samples):
        k.bouncePaths(B(st.pois), B(scratch), B(seeds), n, g1)
        k.flush()
        occ.append(expected_occluded(sc, ao_rays(scratch[:n], st.pois[:n], cast, radius, bias), k))
    return count_ao(cast, occ, sc.rpp)


class Ao:
    """the device scene of one packed scene, its seeds filled by mirt_seed_fill and an output buffer with sentinel bytes behind it"""
    SENTINEL, TAIL = 0xA7, 64

    def __init__(self, ctx, ps, row0=0, nrows=None):
        from raytracing_amd.pyhost import mirt
        self.ctx, self.ps = ctx, ps
        self.row0, self.nrows = row0, ps.height if nrows is None else nrows
        self.dev = mirt.DeviceScene(ctx, ps)
        self.npix = ps.width * self.nrows
        self.nrays = self.npix * ps.rpp
        self.seeds = ctx.buffer(self.nrays * 4)
        ctx.seed_fill(self.seeds, row0 * ps.width * ps.rpp, self.nrays)
        self.out = ctx.buffer(self.npix * 8 + self.TAIL)

    def desc(self, seeds="own"):
        return self.dev.pass_desc(self.seeds if isinstance(seeds, str) else seeds, None, row0=self.row0, nrows=self.nrows if (self.row0 or self.nrows != self.ps.height) else 0)

    def run(self, samples, radius, bias):
        """-> (uint32 [pixels, 2], the bytes behind them)"""
        self.out.write(np.full(self.out.nbytes, self.SENTINEL, np.uint8))
        self.ctx.render_ao(self.desc(), self.out, samples, radius, bias)
        raw = self.out.read(np.uint8)
        return raw[:self.npix * 8].view(np.uint32).reshape(-1, 2).copy(), raw[self.npix * 8:]

    def release(self):
        self.seeds.release()
        self.out.release()
        self.dev.release()


def difference(tag, got, want):
    """None when equal, else a sentence naming the first pixel that differs"""
    g, w = np.asarray(got, np.uint32).reshape(-1, 2), np.asarray(want, np.uint32).reshape(-1, 2)
    if g.shape != w.shape:
        return f"{tag}: {g.shape[0]} pixels against {w.shape[0]}"
    bad = np.flatnonzero((g != w).any(axis=1))
    if bad.size == 0:
        return None
    i = int(bad[0])
    return f"{tag}: {bad.size} of {len(g)} pixels differ; first is pixel {i}: got open {int(g[i, 0])} cast {int(g[i, 1])}, want open {int(w[i, 0])} cast {int(w[i, 1])}"
