"""GPU: the batched view cameras under the DEFAULT contract (libmirt_default.so) -- in a child process with MIRT_CONTRACT=default, as a process
loads one libmirt (tests/view_batch_default_child.py).  The batch's rays equal the numpy restatement there too, and mirt_render_view_batch
equals that library's own N single mirt_render_view calls: both fixtures x three models at 13 x 7, k = 2, N = 3, pair and exact_only."""
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
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "view_batch_default_child.py")], env=env, capture_output=True, text=True, timeout=600)
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0, (lines[-1:] or r.stderr[-2000:])
    assert len(lines) == 2 * 3 * 3 and all(l["ok"] for l in lines)
    frames = [l for l in lines if l["case"].startswith("frames")]
    assert all(l["lit"] > 0 and l["advanced"] > 0 for l in frames), frames
