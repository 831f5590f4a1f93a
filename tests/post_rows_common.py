"""Shared by tests/test_post_rows_restatement.py, tests/test_filter_rows.py, tests/test_upsample_rows.py and the child processes of the two GPU
tests: the row arithmetic of the post-process stage in tiles, restated in Python (include/mirt.h, the section on row tiles), and the two numpy
restatements (tests/filter_common.py, tests/upsample_common.py) applied to a WINDOW of their inputs."""
import numpy as np

from filter_common import atrous
from upsample_common import upsample

f32 = np.float32


def tile_rows(height, n, i):
    """mirt_tile_rows's rule"""
    q, r = divmod(height, n)
    return i * q + min(i, r), q + (1 if i < r else 0)


def halo(iterations):
    return 2 * (2 ** iterations - 1)


def filter_window(height, row0, nrows, iterations):
    lo, hi = max(0, row0 - halo(iterations)), min(height, row0 + nrows + halo(iterations))
    return lo, hi - lo


def low_window(height, f, row0, nrows):
    y0 = lambda y: (2 * y + 1 - f) // (2 * f)
    lo, hi = max(0, y0(row0)), min(height // f, y0(row0 + nrows - 1) + 2)
    return lo, hi - lo


def rows(a, width, row0, nrows):
    """rows [row0, row0 + nrows) of an image of [pixels, 4]"""
    return np.ascontiguousarray(np.asarray(a).reshape(-1, width, 4)[row0:row0 + nrows].reshape(-1, 4))


def atrous_window(inputs, width, win, own, tone, **p):
    """the filter's restatement run on the window win = (row0, nrows) of the inputs AS IF IT WERE AN IMAGE; -> its rows own = (row0, nrows)"""
    cut = [rows(a, width, *win) for a in inputs]
    filtered, pixel = atrous(*cut, width, win[1], tone, **p)
    return rows(filtered, width, own[0] - win[0], own[1]), rows(pixel, width, own[0] - win[0], own[1])


def upsample_window(inputs, width, height, f, own, low, tone, **p):
    """the upsampler's restatement with every low row outside low = (row0, nrows) and every high guide row outside own = (row0, nrows) replaced
    by NaN: what a band computes that holds these rows and no others; -> its rows `own`"""
    wl = width // f
    cut = []
    for a, w, keep in zip(inputs, (wl, wl, wl, width, width), (low, low, low, own, own)):
        b = np.full_like(np.asarray(a, f32).reshape(-1, w, 4), np.nan)
        b[keep[0]:keep[0] + keep[1]] = np.asarray(a, f32).reshape(-1, w, 4)[keep[0]:keep[0] + keep[1]]
        cut.append(b.reshape(-1, 4))
    upsampled, pixel = upsample(*cut, width, height, f, tone, **p)
    return rows(upsampled, width, *own), rows(pixel, width, *own)


# ---- the two _rows calls on a device (ctx: a pyhost.mirt.Context), for the GPU tests and their default-contract child ---------------------------
PATTERN_F, PATTERN_B = 7.5, 0x5A      # what the outputs hold before a call: a row the call must not write keeps it


class RowsFilter:
    """mirt_filter_atrous_rows on the planted inputs of a width x height image: buffers of the whole image's size; a call uploads the window's rows
    to their beginning, plants the pattern in the outputs, and returns the own rows -- after checking that nothing behind them was written"""

    def __init__(self, ctx, width, height, inputs):
        self.ctx, self.w, self.h = ctx, width, height
        self.inputs = [np.ascontiguousarray(a, f32) for a in inputs]
        n = width * height
        self.ins = [ctx.buffer(n * 16) for _ in range(3)]
        self.out, self.pix = ctx.buffer(n * 16), ctx.buffer(n * 4)

    def plant(self):
        n = self.w * self.h
        self.out.write(np.full(n * 4, PATTERN_F, f32))
        self.pix.write(np.full(n * 4, PATTERN_B, np.uint8))

    def outputs(self):
        return self.out.read(f32).reshape(-1, 4), self.pix.read(np.uint8).reshape(-1, 4)

    def run(self, win, own, tone, filtered=True, pixel=True, **p):
        for b, a in zip(self.ins, self.inputs):
            b.write(rows(a, self.w, *win))
        self.plant()
        self.ctx.filter_atrous_rows(self.w, self.h, win[0], win[1], own[0], own[1], tone, *self.ins, filtered=self.out if filtered else None,
                                    pixel=self.pix if pixel else None, **p)
        out, pix = self.outputs()
        k = own[1] * self.w
        assert (out[k:] == PATTERN_F).all() and (pix[k:] == PATTERN_B).all(), f"rows behind the {own[1]} own rows were written"
        return out[:k], pix[:k]

    def release(self):
        for b in self.ins + [self.out, self.pix]:
            b.release()


class RowsUpsampler:
    """mirt_upsample_guided_rows on the planted inputs of a (wl * f) x (hl * f) image, in the manner of RowsFilter"""

    def __init__(self, ctx, wl, hl, f, inputs):
        self.ctx, self.wl, self.hl, self.f, self.w, self.h = ctx, wl, hl, f, wl * f, hl * f
        self.inputs = [np.ascontiguousarray(a, f32) for a in inputs]
        self.ins = [ctx.buffer(a.nbytes) for a in self.inputs]
        n = self.w * self.h
        self.out, self.pix = ctx.buffer(n * 16), ctx.buffer(n * 4)

    def plant(self):
        n = self.w * self.h
        self.out.write(np.full(n * 4, PATTERN_F, f32))
        self.pix.write(np.full(n * 4, PATTERN_B, np.uint8))

    def outputs(self):
        return self.out.read(f32).reshape(-1, 4), self.pix.read(np.uint8).reshape(-1, 4)

    def upload(self, own, low):
        for b, a, w, keep in zip(self.ins, self.inputs, (self.wl,) * 3 + (self.w,) * 2, (low,) * 3 + (own,) * 2):
            b.write(rows(a, w, *keep))

    def run(self, own, low, tone, upsampled=True, pixel=True, **p):
        self.upload(own, low)
        self.plant()
        self.ctx.upsample_guided_rows(self.w, self.h, self.f, own[0], own[1], low[0], low[1], tone, *self.ins, upsampled=self.out if upsampled else None,
                                      pixel=self.pix if pixel else None, **p)
        out, pix = self.outputs()
        k = own[1] * self.w
        assert (out[k:] == PATTERN_F).all() and (pix[k:] == PATTERN_B).all(), f"rows behind the {own[1]} own rows were written"
        return out[:k], pix[:k]

    def release(self):
        for b in self.ins + [self.out, self.pix]:
            b.release()
