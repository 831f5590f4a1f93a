"""GPU: the batch's guides, ambient occlusion and guided frames under the DEFAULT contract (libmirt_default.so) -- in a child process with
MIRT_CONTRACT=default, as a process loads one libmirt (tests/view_batch_aov_default_child.py): mirt_view_guides_batch, mirt_view_ao_batch and
mirt_render_view_guided_batch equal that library's own N single calls at 13 x 7, k = 2, N = 3, both fixtures x three models."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_the_batch_equals_the_single_calls_under_the_default_contract():
    env = dict(os.environ, MIRT_CONTRACT="default")
    env.pop("MIRT_LIB_PATH", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "view_batch_aov_default_child.py")], env=env, capture_output=True, text=True, timeout=600)
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0, (lines[-1:] or r.stderr[-2000:])
    assert len(lines) == 2 * 3 and all(l["ok"] for l in lines), lines
