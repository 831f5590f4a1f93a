"""GPU: the view cameras under the DEFAULT contract (libmirt_default.so: the reference as its own host builds it) -- in a child process with
MIRT_CONTRACT=default, as a process loads one libmirt (tests/view_default_child.py).  The rays equal the numpy restatement there too (one
contract for both libraries), and mirt_render_view equals that library's own mirt_view_rays, mirt_trace_radiance, fold and tone map."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_rays_equal_the_restatement_and_the_frame_its_own_composition_under_the_default_contract():
    env = dict(os.environ, MIRT_CONTRACT="default")
    env.pop("MIRT_LIB_PATH", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "view_default_child.py")], env=env, capture_output=True, text=True, timeout=600)
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0, (lines[-1:] or r.stderr[-2000:])
    assert len(lines) == 3 * 7 + 5 and all(l["ok"] for l in lines)
    frames = [l for l in lines if l["case"].startswith("frame")]
    assert all(l["lit"] > 0 and l["advanced"] > 0 for l in frames), frames
