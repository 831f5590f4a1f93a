#!/usr/bin/env python3
"""tests/view_batch_aov_default_child.py -- run by tests/test_view_batch_aov_default.py in a process of its own with MIRT_CONTRACT=default, so
that pyhost loads libmirt_default.so.  The batch's guides, ambient occlusion and guided frames have the single calls' contract there too:
mirt_view_guides_batch, mirt_view_ao_batch and mirt_render_view_guided_batch equal that library's OWN N single calls at 13 x 7, k = 2, N = 3
-- both fixtures x three models.  Prints one JSON object per case; exits non-zero on the first difference, naming it."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as graft  # noqa: E402
import view_batch_aov_common as BA  # noqa: E402


def main():
    graft.load_package()
    from raytracing_amd.pyhost import mirt
    assert os.path.basename(mirt.LIB_PATH) == "libmirt_default.so", mirt.LIB_PATH
    ctx = mirt.Context(0)
    try:
        for name in BA.FIXTURES:
            for model in BA.MODELS:
                bad = BA.batch_equals_singles(ctx, name, model)
                print(json.dumps({"case": f"{name} {model}", "ok": not bad, "difference": bad[:1]}), flush=True)
                if bad:
                    return 1
    finally:
        ctx.destroy()
    return 0


if __name__ == "__main__":
    sys.exit(main())
