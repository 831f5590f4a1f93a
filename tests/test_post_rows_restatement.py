"""CPU, numpy only: the two facts the definition of the post-process stage in row tiles rests on (include/mirt.h), pinned on the restatements of
the filter (tests/filter_common.py) and the upsampler (tests/upsample_common.py) and their planted inputs.

  1. Filtering the window [row0 - H, row0 + nrows + H), H = 2 * (2^iterations - 1), clamped to the image, AS IF IT WERE AN IMAGE gives rows
     [row0, row0 + nrows) of the filtered frame bit for bit; so does any larger window.  A band of high rows of the upsampler that is given low rows
     max(0, Y0(row0)) .. min(hl, Y0(row0 + nrows - 1) + 2) and its own guide rows, and nothing else, gives those rows of the upsampled frame.
  2. A window one row short, at either end, does not: at least one planted case differs.  That keeps the "contains" rule of
     mirt_filter_atrous_rows and mirt_upsample_guided_rows from being loosened unnoticed."""
import pytest

import filter_common as F
import upsample_common as U
from filter_common import difference
from post_rows_common import atrous_window, filter_window, low_window, rows, tile_rows, upsample_window

OFF = dict(normal_power_log2=0, sigma_depth=0.0, sigma_colour=0.0, demodulate=False)


@pytest.fixture(scope="module")
def syn():
    return F.synthetic()


_whole = {}


def whole(syn, **p):
    key = tuple(sorted(p.items()))
    if key not in _whole:
        _whole[key] = F.atrous(*syn, F.SYN_W, F.SYN_H, F.SYN_TONE, **p)
    return _whole[key]


def same(tag, got, want):
    for name, g, w in zip(("filtered", "pixel"), got, want):
        d = difference(f"{tag} {name}", g, w)
        assert d is None, d


@pytest.mark.parametrize("terms", ["shipped", "off"])
@pytest.mark.parametrize("iterations", [0, 1, 2, 3])
def test_filter_window_as_image_gives_the_frames_rows(syn, iterations, terms):
    p = dict(F.DEFAULTS if terms == "shipped" else OFF, iterations=iterations)
    want = whole(syn, **p)
    shorter_than_halo = False
    for n in (1, 2, 3, 5, 12):
        for t in range(n):
            own = tile_rows(F.SYN_H, n, t)
            win = filter_window(F.SYN_H, *own, iterations)
            shorter_than_halo |= own[1] < 2 * (2 ** iterations - 1)
            same(f"{iterations} iterations, tile {t} of {n}", atrous_window(syn, F.SYN_W, win, own, F.SYN_TONE, **p), [rows(w, F.SYN_W, *own) for w in want])
    assert shorter_than_halo == (iterations >= 2)


def test_filter_larger_window_gives_the_same_rows(syn):
    p = dict(F.DEFAULTS, iterations=2)
    want = whole(syn, **p)
    own = tile_rows(F.SYN_H, 3, 1)
    for win in ((own[0] - 9, own[1] + 15), (0, F.SYN_H), (0, own[0] + own[1] + 6), (own[0] - 6, F.SYN_H - own[0] + 6)):
        same(f"window {win}", atrous_window(syn, F.SYN_W, win, own, F.SYN_TONE, **p), [rows(w, F.SYN_W, *own) for w in want])


@pytest.mark.parametrize("end", ["top", "bottom"])
def test_filter_window_one_row_short_differs(syn, end):
    """tile 1 of 3 at 2 iterations, shipped parameters: H - 1 rows at one end are not enough"""
    p = dict(F.DEFAULTS, iterations=2)
    want = [rows(w, F.SYN_W, *tile_rows(F.SYN_H, 3, 1)) for w in whole(syn, **p)]
    own = tile_rows(F.SYN_H, 3, 1)
    w0, wn = filter_window(F.SYN_H, *own, 2)
    assert w0 > 0 and w0 + wn < F.SYN_H, "a window clamped by the image would have no row to lose"
    short = (w0 + 1, wn - 1) if end == "top" else (w0, wn - 1)
    got = atrous_window(syn, F.SYN_W, short, own, F.SYN_TONE, **p)
    assert difference("filtered", got[0], want[0]) is not None


_up = {}


def up_inputs(f):
    if f not in _up:
        inputs = U.synthetic(f=f)
        _up[f] = inputs, U.upsample(*inputs, U.SYN_WL * f, U.SYN_HL * f, f, U.SYN_TONE, **U.DEFAULTS)
    return _up[f]


@pytest.mark.parametrize("f", [2, 3, 4])
def test_upsampler_band_with_its_low_window_gives_the_frames_rows(f):
    inputs, want = up_inputs(f)
    W, H = U.SYN_WL * f, U.SYN_HL * f
    unaligned = False
    for n in (2, 3, 7):
        for t in range(n):
            own = tile_rows(H, n, t)
            unaligned |= own[0] % f != 0
            low = low_window(H, f, *own)
            same(f"factor {f}, tile {t} of {n}", upsample_window(inputs, W, H, f, own, low, U.SYN_TONE, **U.DEFAULTS), [rows(w, W, *own) for w in want])
    assert unaligned


@pytest.mark.parametrize("end", ["top", "bottom"])
@pytest.mark.parametrize("f", [2, 3, 4])
def test_upsampler_low_window_one_row_short_differs(f, end):
    inputs, want = up_inputs(f)
    W, H = U.SYN_WL * f, U.SYN_HL * f
    own = tile_rows(H, 3, 1)
    l0, ln = low_window(H, f, *own)
    assert l0 > 0 and l0 + ln < H // f
    short = (l0 + 1, ln - 1) if end == "top" else (l0, ln - 1)
    got = upsample_window(inputs, W, H, f, own, short, U.SYN_TONE, **U.DEFAULTS)
    assert difference("upsampled", got[0], rows(want[0], W, *own)) is not None
