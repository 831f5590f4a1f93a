"""GPU: mirt_filter_atrous_rows -- the a-trous filter of rows [row0, row0 + nrows) from a window of the image (include/mirt.h) -- through the C ABI,
tolerance 0 against the rows of the numpy restatement of the WHOLE frame (tests/filter_common.py; every NaN equal to every NaN), on the planted
83 x 47 inputs (NaN / inf / -0 radiance, background blocks, zero albedo channels):

  1. 1, 2, 3 and 12 tiles of mirt_tile_rows's rule, each from exactly its window: iterations 0 .. 3, and 5 where the window is the whole image;
     shipped parameters and all terms off, demodulated and not, the shipped structure and both forced;
  2. a window larger than needed gives the same bits; window and rows both the whole image give mirt_filter_atrous's bytes; either output alone;
  3. refusals: a window one row short at the top or at the bottom is MIRT_E_ARG and the outputs keep their planted pattern; rows or windows outside
     the image, no rows, short buffers, aliasing, a call while capturing;
  4. libmirt_default.so gives the same bits (a child process)."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT
from filter_common import DEFAULTS, SYN_H, SYN_TONE, SYN_W, atrous, difference, synthetic
from post_rows_common import PATTERN_B, PATTERN_F, RowsFilter, filter_window, rows, tile_rows

pytestmark = pytest.mark.gpu

E_ARG, E_RANGE = -1, -5
OFF = dict(normal_power_log2=0, sigma_depth=0.0, sigma_colour=0.0)
TILINGS = (1, 2, 3, 12)


@pytest.fixture(scope="module")
def ctx(pkg):
    from raytracing_amd.pyhost import mirt
    c = mirt.Context(0)
    yield c
    c.destroy()


@pytest.fixture(scope="module")
def syn():
    return synthetic()


@pytest.fixture(scope="module")
def rf(ctx, syn):
    f = RowsFilter(ctx, SYN_W, SYN_H, syn)
    yield f
    f.release()


_want = {}


def expected(syn, **p):
    """the restatement of the whole frame, computed once per parameter set"""
    key = tuple(sorted(p.items()))
    if key not in _want:
        _want[key] = atrous(*syn, SYN_W, SYN_H, SYN_TONE, **p)
    return _want[key]


def check(tag, got, want, own):
    for name, g, w in zip(("filtered", "pixel"), got, want):
        d = difference(f"{tag} {name}", g, rows(w, SYN_W, *own))
        assert d is None, d


@pytest.mark.parametrize("structure", [None, "direct", "tiled"])
@pytest.mark.parametrize("iterations", [0, 1, 2, 3])
def test_every_tile_from_its_window(syn, rf, iterations, structure):
    for terms in (DEFAULTS, dict(DEFAULTS, **OFF)):
        for demodulate in (False, True):
            p = dict(terms, iterations=iterations, demodulate=demodulate)
            want = expected(syn, **p)
            for n in TILINGS:
                for t in range(n):
                    own = tile_rows(SYN_H, n, t)
                    win = filter_window(SYN_H, *own, iterations)
                    tag = f"{iterations} iterations {structure} colour {p['sigma_colour']} demodulate={demodulate}, tile {t} of {n}: rows {own} from {win}"
                    check(tag, rf.run(win, own, SYN_TONE, structure=structure, **p), want, own)


@pytest.mark.parametrize("structure", [None, "direct", "tiled"])
def test_five_iterations_where_the_window_is_the_whole_image(syn, rf, structure):
    p = dict(DEFAULTS, iterations=5)
    own = tile_rows(SYN_H, 3, 1)
    win = filter_window(SYN_H, *own, 5)
    assert win == (0, SYN_H)
    check(f"5 iterations {structure}", rf.run(win, own, SYN_TONE, structure=structure, **p), expected(syn, **p), own)


@pytest.mark.parametrize("structure", ["direct", "tiled"])
def test_a_larger_window_gives_the_same_bits(syn, rf, structure):
    p = dict(DEFAULTS, iterations=2)
    want = expected(syn, **p)
    own = tile_rows(SYN_H, 3, 1)
    w0, wn = filter_window(SYN_H, *own, 2)
    for win in ((w0 - 3, wn + 8), (0, SYN_H), (0, w0 + wn), (w0, SYN_H - w0)):
        check(f"window {win} {structure}", rf.run(win, own, SYN_TONE, structure=structure, **p), want, own)


@pytest.mark.parametrize("iterations", [0, 3])
def test_the_whole_image_as_one_tile_equals_mirt_filter_atrous(ctx, syn, rf, iterations):
    p = dict(DEFAULTS, iterations=iterations)
    got = rf.run((0, SYN_H), (0, SYN_H), SYN_TONE, **p)
    rf.plant()
    ctx.filter_atrous(SYN_W, SYN_H, SYN_TONE, *rf.ins, filtered=rf.out, pixel=rf.pix, **p)
    whole = rf.outputs()
    assert got[0].tobytes() == whole[0].tobytes() and got[1].tobytes() == whole[1].tobytes()


@pytest.mark.parametrize("filtered,pixel", [(True, False), (False, True)])
def test_either_output_alone(syn, rf, filtered, pixel):
    p = dict(DEFAULTS, iterations=2)
    own = tile_rows(SYN_H, 3, 2)
    got = rf.run(filter_window(SYN_H, *own, 2), own, SYN_TONE, filtered=filtered, pixel=pixel, **p)
    want = expected(syn, **p)
    which = 0 if filtered else 1
    d = difference("the output asked for", got[which], rows(want[which], SYN_W, *own))
    assert d is None, d
    assert (got[1 - which] == (PATTERN_B if filtered else PATTERN_F)).all(), "an output that was not passed was written"


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------------------
def refused(rf, code, call):
    from raytracing_amd.pyhost import mirt
    rf.plant()
    with pytest.raises(mirt.MirtError) as e:
        call()
    assert e.value.code == code, str(e.value)
    out, pix = rf.outputs()
    assert (out == PATTERN_F).all() and (pix == PATTERN_B).all(), "a refused call wrote to an output"
    return str(e.value)


def call_rows(rf, win, own, image_height=SYN_H, ins=None, filtered=None, pixel=None, **p):
    q = dict(DEFAULTS, iterations=2)
    q.update(p)
    ins = ins or rf.ins
    return lambda: rf.ctx.filter_atrous_rows(rf.w, image_height, win[0], win[1], own[0], own[1], SYN_TONE, *ins, filtered=filtered or rf.out,
                                             pixel=pixel or rf.pix, **q)


def test_a_window_one_row_short_is_refused(rf):
    own = tile_rows(SYN_H, 3, 1)
    w0, wn = filter_window(SYN_H, *own, 2)
    assert w0 > 0 and w0 + wn < SYN_H
    assert "does not contain" in refused(rf, E_ARG, call_rows(rf, (w0 + 1, wn - 1), own))
    assert "does not contain" in refused(rf, E_ARG, call_rows(rf, (w0, wn - 1), own))
    call_rows(rf, (w0, wn), own)()      # the window itself is accepted


def test_rows_and_windows_outside_the_image_are_refused(rf):
    own = tile_rows(SYN_H, 3, 1)
    win = filter_window(SYN_H, *own, 2)
    refused(rf, E_ARG, call_rows(rf, win, (own[0], 0)))
    refused(rf, E_ARG, call_rows(rf, (win[0], 0), own))
    refused(rf, E_ARG, call_rows(rf, (0, SYN_H + 1), own))
    refused(rf, E_ARG, call_rows(rf, (0, SYN_H), (SYN_H - 2, 3)))
    refused(rf, E_ARG, call_rows(rf, (0, SYN_H), (2 ** 32 - 1, 2)))
    refused(rf, E_ARG, call_rows(rf, (2 ** 32 - 2, 4), own))
    refused(rf, E_ARG, call_rows(rf, win, own, image_height=0))
    refused(rf, E_ARG, call_rows(rf, win, own, image_height=65536))
    refused(rf, E_ARG, call_rows(rf, (0, SYN_H), own, iterations=6))


def test_short_buffers_are_refused(ctx, rf):
    own = tile_rows(SYN_H, 3, 1)
    win = filter_window(SYN_H, *own, 2)
    short_in = ctx.buffer(win[1] * SYN_W * 16 - 16)
    short_out, short_pix = ctx.buffer(own[1] * SYN_W * 16 - 16), ctx.buffer(own[1] * SYN_W * 4 - 4)
    exact_out, exact_pix = ctx.buffer(own[1] * SYN_W * 16), ctx.buffer(own[1] * SYN_W * 4)
    try:
        for i in range(3):
            ins = list(rf.ins)
            ins[i] = short_in
            refused(rf, E_RANGE, call_rows(rf, win, own, ins=ins))
        refused(rf, E_RANGE, call_rows(rf, win, own, filtered=short_out))
        refused(rf, E_RANGE, call_rows(rf, win, own, pixel=short_pix))
        call_rows(rf, win, own, filtered=exact_out, pixel=exact_pix)()      # outputs of exactly nrows rows are enough
    finally:
        for b in (short_in, short_out, short_pix, exact_out, exact_pix):
            b.release()


def test_aliasing_and_capture_are_refused(ctx, rf):
    own = tile_rows(SYN_H, 3, 1)
    win = filter_window(SYN_H, *own, 2)
    assert "aliases" in refused(rf, E_ARG, call_rows(rf, win, own, filtered=rf.ins[0]))
    assert "aliases" in refused(rf, E_ARG, call_rows(rf, win, own, pixel=rf.ins[2]))
    assert "aliases" in refused(rf, E_ARG, call_rows(rf, win, own, filtered=rf.out, pixel=rf.out))
    ctx.finish()
    ctx.capture_begin()
    try:
        msg = refused_while_capturing(rf, call_rows(rf, win, own))
    finally:
        ctx.graph_release(ctx.capture_end())
    assert "capture" in msg
    out, pix = rf.outputs()
    assert (out == PATTERN_F).all() and (pix == PATTERN_B).all()


def refused_while_capturing(rf, call):
    """the outputs were planted before the recording began: nothing may read them back inside it"""
    from raytracing_amd.pyhost import mirt
    with pytest.raises(mirt.MirtError) as e:
        call()
    assert e.value.code == E_ARG
    return str(e.value)


# ---- 4. the second library --------------------------------------------------------------------------------------------------------------------
def test_the_default_contract_library_gives_the_same_bits():
    env = dict(os.environ, MIRT_CONTRACT="default")
    env.pop("MIRT_LIB_PATH", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "post_rows_default_child.py"), "filter"], env=env, capture_output=True, text=True, timeout=600)
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0, (lines[-1:] or r.stderr[-2000:])
    assert lines and all(l["ok"] for l in lines)
