"""GPU: mirt_exchange_rows -- the halo exchange between the contexts of a group (include/mirt.h) -- on rehearsal groups
(MIRT_GROUP_ALLOW_REPEATED_DEVICES=1: the contexts share the device at hand, each with a stream of its own) of 1, 2, 3 and 5 contexts.

  1. 12 rows over the group's tiles, every tile's filter window at halo 6 wanted -- over 5 tiles a window spans three owners and more, over more
     tiles than rows some are empty -- the buffers holding row-tagged patterns: every byte of every window is checked, and what lies behind a
     window keeps its pattern.  Some contexts want no window.  Each source is zeroed on its own stream right after the call, with no finish in
     between: the windows still hold the tags.
  2. Every refusal, and that a refused call queued nothing: the windows keep their pattern."""
import numpy as np
import pytest

from post_rows_common import filter_window, tile_rows

pytestmark = pytest.mark.gpu

E_ARG, E_HANDLE, E_RANGE = -1, -2, -5
ROWS, WORDS, ITERATIONS = 12, 6, 2          # 24-byte rows (a multiple of 4 and of nothing larger), halo 2 * (2^2 - 1) = 6
PATTERN = 0xA5A5A5A5


def tags(row0, nrows):
    """row r, word k -> r * 1000 + k + 1 (never 0, never the pattern)"""
    r = np.arange(row0, row0 + nrows, dtype=np.uint32)[:, None]
    return (r * 1000 + np.arange(WORDS, dtype=np.uint32)[None, :] + 1).astype(np.uint32)


@pytest.fixture()
def group(pkg, monkeypatch):
    from raytracing_amd.pyhost import mirt
    monkeypatch.setenv("MIRT_GROUP_ALLOW_REPEATED_DEVICES", "1")
    made = []

    def make(n):
        g = mirt.DeviceGroup([0] * n)
        made.append(g)
        return g
    yield make
    for g in made:
        g.destroy()


class Exchange:
    """per context a source buffer with the tagged rows of its tile, and a window buffer one row longer than the window, all pattern"""

    def __init__(self, g, src_rows, dst_rows):
        self.g, self.src_rows, self.dst_rows = g, src_rows, dst_rows
        self.src, self.dst = [], []
        for c, (s0, sn), (d0, dn) in zip(g.contexts, src_rows, dst_rows):
            self.src.append(c.buffer(sn * WORDS * 4).write(tags(s0, sn)) if sn else None)
            self.dst.append(c.buffer((dn + 1) * WORDS * 4).write(np.full((dn + 1) * WORDS, PATTERN, np.uint32)) if dn else None)
        g.finish()

    def run(self, **over):
        a = dict(src=self.src, src_rows=self.src_rows, dst=self.dst, dst_rows=self.dst_rows, row_bytes=WORDS * 4)
        a.update(over)
        self.g.exchange_rows(a["src"], a["src_rows"], a["dst"], a["dst_rows"], a["row_bytes"])

    def windows(self):
        return [None if b is None else b.read(np.uint32).reshape(-1, WORDS) for b in self.dst]

    def untouched(self):
        return all(w is None or (w == PATTERN).all() for w in self.windows())


@pytest.mark.parametrize("absent", [(), (0,), (1, 3)])
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_every_window_byte(group, n, absent):
    g = group(n)
    src_rows = [tile_rows(ROWS, n, t) for t in range(n)]
    dst_rows = [(0, 0) if t in absent else filter_window(ROWS, *src_rows[t], ITERATIONS) for t in range(n)]
    x = Exchange(g, src_rows, dst_rows)
    x.run()
    for c, b in zip(g.contexts, x.src):      # the source's next work, queued right behind the exchange on its own stream: no finish in between
        c.zero(b)
    g.finish()
    for t, (w, (d0, dn)) in enumerate(zip(x.windows(), dst_rows)):
        if w is None:
            continue
        assert np.array_equal(w[:dn], tags(d0, dn)), f"window {t} of {n}: rows [{d0}, +{dn})"
        assert (w[dn:] == PATTERN).all(), f"window {t} of {n}: the row behind the window was written"
    for b in x.src:
        assert not b.read(np.uint32).any(), "the zeroing of a source did not run"
    if n == 5 and not absent:
        owners = [sum(1 for s0, sn in src_rows if s0 < d0 + dn and d0 < s0 + sn) for d0, dn in dst_rows]
        assert min(owners) >= 3 and max(owners) == 5


def test_more_contexts_than_rows(group):
    """3 rows over 5 contexts: two tiles are empty -- NULL buffers with 0 rows -- and every window is the whole image"""
    g = group(5)
    src_rows = [tile_rows(3, 5, t) for t in range(5)]
    dst_rows = [filter_window(3, *s, ITERATIONS) if s[1] else (0, 0) for s in src_rows]
    assert [s[1] for s in src_rows] == [1, 1, 1, 0, 0]
    x = Exchange(g, src_rows, dst_rows)
    assert x.src[3] is None and x.dst[4] is None
    x.run()
    g.finish()
    for w, (d0, dn) in zip(x.windows(), dst_rows):
        if w is not None:
            assert (d0, dn) == (0, 3) and np.array_equal(w[:dn], tags(d0, dn)) and (w[dn:] == PATTERN).all()


def refused(x, code, **over):
    from raytracing_amd.pyhost import mirt
    with pytest.raises(mirt.MirtError) as e:
        x.run(**over)
    assert e.value.code == code, str(e.value)
    x.g.finish()
    assert x.untouched(), "a refused exchange copied something"
    return str(e.value)


def test_refusals(group):
    from raytracing_amd.pyhost import mirt
    g = group(3)
    src_rows = [tile_rows(ROWS, 3, t) for t in range(3)]
    dst_rows = [filter_window(ROWS, *s, 1) for s in src_rows]      # halo 2: windows (0, 6), (2, 8), (6, 6)
    x = Exchange(g, src_rows, dst_rows)
    # MIRT_E_ARG: the plan
    assert "owns rows" in refused(x, E_ARG, src_rows=[(0, 4), (3, 4), (8, 4)])
    assert "no source owns" in refused(x, E_ARG, src_rows=[(0, 4), (4, 3), (8, 4)])
    assert "no source owns" in refused(x, E_ARG, src_rows=[(1, 4), (5, 4), (9, 3)])
    # ... the sizes
    refused(x, E_ARG, src=x.src[:2], src_rows=src_rows[:2], dst=x.dst[:2], dst_rows=dst_rows[:2])
    refused(x, E_ARG, row_bytes=0)
    refused(x, E_ARG, row_bytes=WORDS * 4 - 2)
    # ... a destination whose bytes meet a source's: context 1's tile as its own window
    own = [(0, 0), src_rows[1], (0, 0)]
    assert "meet" in refused(x, E_ARG, dst=[None, x.src[1], None], dst_rows=own)
    # ... while a context is capturing
    g.finish()
    g.contexts[2].capture_begin()
    try:
        assert "capture" in refused_while_capturing(x)
    finally:
        g.contexts[2].graph_release(g.contexts[2].capture_end())
    g.finish()
    assert x.untouched()
    # MIRT_E_HANDLE: another context's buffer, NULL with rows, a released buffer
    refused(x, E_HANDLE, src=[x.src[1], x.src[0], x.src[2]])
    refused(x, E_HANDLE, dst=[x.dst[0], x.dst[2], x.dst[1]])
    refused(x, E_HANDLE, src=[x.src[0], None, x.src[2]])
    refused(x, E_HANDLE, dst=[None, x.dst[1], x.dst[2]])
    gone = g.contexts[0].buffer(64)
    stale = mirt.Buffer(g.contexts[0], gone.h, 64)
    gone.release()
    refused(x, E_HANDLE, src=[stale, x.src[1], x.src[2]])
    # MIRT_E_RANGE: a buffer shorter than its rows
    short = g.contexts[0].buffer(src_rows[0][1] * WORDS * 4 - 4)
    refused(x, E_RANGE, src=[short, x.src[1], x.src[2]])
    short_dst = g.contexts[1].buffer(dst_rows[1][1] * WORDS * 4 - 4)
    refused(x, E_RANGE, dst=[x.dst[0], short_dst, x.dst[2]])
    # and the call as it should be goes through
    x.run()
    g.finish()
    for w, (d0, dn) in zip(x.windows(), dst_rows):
        assert np.array_equal(w[:dn], tags(d0, dn))


def refused_while_capturing(x):
    """nothing may be read back inside a recording: the windows are looked at after it"""
    from raytracing_amd.pyhost import mirt
    with pytest.raises(mirt.MirtError) as e:
        x.run()
    assert e.value.code == E_ARG
    return str(e.value)
