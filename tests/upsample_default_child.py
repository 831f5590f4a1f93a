#!/usr/bin/env python3
"""tests/upsample_default_child.py -- run by tests/test_upsample.py in a process of its own with MIRT_CONTRACT=default, so that pyhost loads
libmirt_default.so: mirt_upsample_guided of the library built for the reference's own build options (AMD's 2.5-ulp `/`) against the numpy
restatement of the header's definition, on the planted inputs of tests/upsample_common.py at 29x17 -> 3.  The reference has no upsampler: there
is one contract, so the bits are those libmirt.so gives: with a path as its argument the child also saves what it got (an .npz, upsampled_<i> and
pixel_<i> per case of CASES), which the parent compares with libmirt.so's own outputs.  Prints one JSON object per case; exits non-zero on the
first difference, naming it."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402
from filter_common import difference  # noqa: E402
from upsample_common import SYN_HL, SYN_TONE, SYN_WL, synthetic, upsample  # noqa: E402

F = 3
CASES = ((0, 0.0, False), (5, 0.1, True), (5, 0.0, True), (0, 0.1, False))   # normal_power_log2, sigma_depth, demodulate


def main():
    graft.load_package()
    from raytracing_amd.pyhost import mirt
    assert os.path.basename(mirt.LIB_PATH) == "libmirt_default.so", mirt.LIB_PATH
    inputs = synthetic(SYN_WL, SYN_HL, F)
    W, H = SYN_WL * F, SYN_HL * F
    ctx = mirt.Context(0)
    bufs = [ctx.buffer(a.nbytes).write(np.ascontiguousarray(a, np.float32)) for a in inputs]
    out, pix = ctx.buffer(W * H * 16), ctx.buffer(W * H * 4)
    try:
        saved = {}
        for i, (npow, sigma_depth, demodulate) in enumerate(CASES):
            p = dict(normal_power_log2=npow, sigma_depth=sigma_depth, demodulate=demodulate)
            want = upsample(*inputs, W, H, F, SYN_TONE, **p)
            ctx.upsample_guided(W, H, F, SYN_TONE, *bufs, upsampled=out, pixel=pix, **p)
            got = out.read(np.float32).reshape(-1, 4), pix.read(np.uint8).reshape(-1, 4)
            saved[f"upsampled_{i}"], saved[f"pixel_{i}"] = got[0].copy(), got[1].copy()
            for tag, g, w in (("upsampled", got[0], want[0]), ("pixel", got[1], want[1])):
                d = difference(f"power 2^{npow} depth {sigma_depth} demodulate={demodulate} {tag}", g, w)
                if d:
                    print(json.dumps(dict(p, ok=False, difference=d)), flush=True)
                    return 1
            print(json.dumps(dict(p, ok=True)), flush=True)
        if len(sys.argv) > 1:
            np.savez(sys.argv[1], **saved)
    finally:
        for b in bufs + [out, pix]:
            b.release()
        ctx.destroy()
    return 0


if __name__ == "__main__":
    sys.exit(main())
