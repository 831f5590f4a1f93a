"""GPU: the edge cameras of tests/view_cameras_common.py under the DEFAULT contract (libmirt_default.so: the reference as its own host builds it) --
in a child process with MIRT_CONTRACT=default, as a process loads one libmirt (tests/view_cameras_default_child.py).  axis_*, rim_* and mixed_k2
on `staged` and `single_cell`: the rays equal the numpy restatement there too, and mirt_render_view equals that library's own kernel-by-kernel
path on the restated rays, then the numpy fold and tone map; the frames with refused primary rays are partly deferred."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_axis_rim_and_mixed_frames_under_the_default_contract():
    import view_cameras_common as VC
    env = dict(os.environ, MIRT_CONTRACT="default")
    env.pop("MIRT_LIB_PATH", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "view_cameras_default_child.py")], env=env, capture_output=True, text=True, timeout=600)
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0, (lines[-1:] or r.stderr[-2000:])
    names = VC.AXIS + VC.RIM + ("mixed_k2",)
    assert [l["case"] for l in lines] == [f"{s} {n}" for s in ("staged", "single_cell") for n in names] and all(l["ok"] for l in lines)
    assert all(l["lit"] > 0 and l["advanced"] > 0 for l in lines), lines
    for l in lines:
        mixed = l["case"].split()[1] in VC.MIXED
        assert (0 < l["refused_blocks"] < l["blocks"]) == mixed and 256 * l["refused_blocks"] <= l["deferred"] <= 256 * l["blocks"], l
    print("\n".join(f"view_deferred default {l['case']}: {l['deferred']} of {l['rays']} rays" for l in lines))
