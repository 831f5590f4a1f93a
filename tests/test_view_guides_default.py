"""GPU: the view cameras' guides under the DEFAULT contract (libmirt_default.so: the reference as its own host builds it) -- in a child process
with MIRT_CONTRACT=default, as a process loads one libmirt (tests/view_guides_child.py).  mirt_view_guides equals that library's own
mirt_view_rays, mirt_trace_closest and the numpy reduction at every size, and mirt_render_view_guided its own two calls at every k, fresh and with
ACCUMULATE, under the pair and under set_exact_only, with mirt_ctx_guided_views moving as the route rule says."""
import json
import os
import subprocess
import sys

import pytest

import view_common as V
import view_guides_common as VG
from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_guides_equal_their_composition_and_the_guided_frame_its_two_calls_under_the_default_contract():
    env = dict(os.environ, MIRT_CONTRACT="default")
    env.pop("MIRT_LIB_PATH", None)
    env.pop("MIRT_GUIDED_VIEW", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "view_guides_child.py"), "default"], env=env, capture_output=True, text=True, timeout=600)
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0, (lines[-1:] or r.stderr[-2000:])
    assert len(lines) == len(VG.FIXTURES) * (len(VG.SIZES) + 2 * len(V.KS)) and all(l["ok"] for l in lines), lines
    assert all(l["hit_pixels"] > 0 for l in lines), lines
