#!/usr/bin/env python3
"""tests/filter_default_child.py -- run by tests/test_filter.py in a process of its own with MIRT_CONTRACT=default, so that pyhost loads
libmirt_default.so: mirt_filter_atrous of the library built for the reference's own build options (AMD's 2.5-ulp `/`) against the numpy
restatement of the header's definition, on the synthetic inputs of tests/filter_common.py.  The reference has no filter: there is one contract, so
the bits are those libmirt.so gives.  Prints one JSON object per case; exits non-zero on the first difference, naming it."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402
from filter_common import DEFAULTS, SYN_H, SYN_TONE, SYN_W, atrous, difference, synthetic  # noqa: E402


def main():
    graft.load_package()
    from raytracing_amd.pyhost import mirt
    assert os.path.basename(mirt.LIB_PATH) == "libmirt_default.so", mirt.LIB_PATH
    inputs = synthetic()
    n = SYN_W * SYN_H
    ctx = mirt.Context(0)
    rad, nh, ad, out, pix = ctx.buffer(n * 16), ctx.buffer(n * 16), ctx.buffer(n * 16), ctx.buffer(n * 16), ctx.buffer(n * 4)
    try:
        for b, a in zip((rad, nh, ad), inputs):
            b.write(np.ascontiguousarray(a, np.float32))
        for iterations, demodulate in ((0, False), (0, True), (1, True), (3, False), (5, True)):
            p = dict(DEFAULTS, iterations=iterations, demodulate=demodulate)
            want = atrous(*inputs, SYN_W, SYN_H, SYN_TONE, **p)
            for structure in ("direct", "tiled"):
                ctx.filter_atrous(SYN_W, SYN_H, SYN_TONE, rad, nh, ad, filtered=out, pixel=pix, structure=structure, **p)
                got = out.read(np.float32).reshape(-1, 4), pix.read(np.uint8).reshape(-1, 4)
                for tag, g, w in (("filtered", got[0], want[0]), ("pixel", got[1], want[1])):
                    d = difference(f"{iterations} iterations demodulate={demodulate} {structure} {tag}", g, w)
                    if d:
                        print(json.dumps({"iterations": iterations, "ok": False, "difference": d}), flush=True)
                        return 1
            print(json.dumps({"iterations": iterations, "demodulate": demodulate, "ok": True}), flush=True)
    finally:
        for b in (rad, nh, ad, out, pix):
            b.release()
        ctx.destroy()
    return 0


if __name__ == "__main__":
    sys.exit(main())
