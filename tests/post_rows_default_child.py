#!/usr/bin/env python3
"""tests/post_rows_default_child.py filter|upsample -- run by tests/test_filter_rows.py and tests/test_upsample_rows.py in a process of its own with
MIRT_CONTRACT=default, so that pyhost loads libmirt_default.so: mirt_filter_atrous_rows / mirt_upsample_guided_rows of the library built for the
reference's own build options against the rows of the numpy restatement of the whole frame, on the planted inputs.  There is one contract for the
post-process stage, so the bits are those libmirt.so gives.  Prints one JSON object per case; exits non-zero on the first difference, naming it."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402
import filter_common as F  # noqa: E402
import upsample_common as U  # noqa: E402
from post_rows_common import RowsFilter, RowsUpsampler, filter_window, low_window, rows, tile_rows  # noqa: E402


def differs(tag, got, want, width, own):
    for name, g, w in zip(("rows", "pixel"), got, want):
        d = F.difference(f"{tag} {name}", g, rows(w, width, *own))
        if d:
            print(json.dumps({"case": tag, "ok": False, "difference": d}), flush=True)
            return True
    return False


def filter_cases(ctx):
    inputs = F.synthetic()
    rf = RowsFilter(ctx, F.SYN_W, F.SYN_H, inputs)
    try:
        for iterations, demodulate in ((0, True), (1, False), (2, True), (3, True), (5, False)):
            p = dict(F.DEFAULTS, iterations=iterations, demodulate=demodulate)
            want = F.atrous(*inputs, F.SYN_W, F.SYN_H, F.SYN_TONE, **p)
            for structure in ("direct", "tiled"):
                for n in (1, 3, 12):
                    for t in range(n):
                        own = tile_rows(F.SYN_H, n, t)
                        got = rf.run(filter_window(F.SYN_H, *own, iterations), own, F.SYN_TONE, structure=structure, **p)
                        if differs(f"{iterations} iterations demodulate={demodulate} {structure} tile {t} of {n}", got, want, F.SYN_W, own):
                            return 1
            print(json.dumps({"iterations": iterations, "demodulate": demodulate, "ok": True}), flush=True)
    finally:
        rf.release()
    return 0


def upsample_cases(ctx):
    for f in (2, 3, 4):
        inputs = U.synthetic(f=f)
        W, H = U.SYN_WL * f, U.SYN_HL * f
        ru = RowsUpsampler(ctx, U.SYN_WL, U.SYN_HL, f, inputs)
        try:
            for demodulate in (False, True):
                p = dict(U.DEFAULTS, demodulate=demodulate)
                want = U.upsample(*inputs, W, H, f, U.SYN_TONE, **p)
                for n in (1, 3, 7):
                    for t in range(n):
                        own = tile_rows(H, n, t)
                        if differs(f"factor {f} demodulate={demodulate} tile {t} of {n}", ru.run(own, low_window(H, f, *own), U.SYN_TONE, **p), want, W, own):
                            return 1
                print(json.dumps({"factor": f, "demodulate": demodulate, "ok": True}), flush=True)
        finally:
            ru.release()
    return 0


def main():
    graft.load_package()
    from raytracing_amd.pyhost import mirt
    assert os.path.basename(mirt.LIB_PATH) == "libmirt_default.so", mirt.LIB_PATH
    ctx = mirt.Context(0)
    try:
        return {"filter": filter_cases, "upsample": upsample_cases}[sys.argv[1]](ctx)
    finally:
        ctx.destroy()


if __name__ == "__main__":
    sys.exit(main())
