"""GPU: the view cameras' ambient occlusion under the DEFAULT contract (libmirt_default.so: the reference as its own host builds it) -- in a
child process with MIRT_CONTRACT=default, as a process loads one libmirt (tests/view_ao_child.py).  mirt_view_ao on both fixtures x three models
at 13 x 7, k = 2, equals the restatement of tests/view_ao_common.py with the reference's default build on the device as the checker
(oracle/ref_gpu.py), under the pair and under set_exact_only."""
import json
import os
import subprocess
import sys

import pytest

import view_ao_common as VA
from conftest import ROOT

pytestmark = pytest.mark.gpu

DEFAULT_HSACO = os.path.join(ROOT, "oracle", "_ref", "a10_gfx950_default.hsaco")
DEFAULT_LIB = os.path.join(ROOT, "2015-raytracing_amd", "libmirt_default.so")


@pytest.mark.skipif(not (os.path.exists(DEFAULT_HSACO) and os.path.exists(DEFAULT_LIB)), reason="needs the default-build code object and libmirt_default.so")
def test_view_ao_equals_the_default_build_of_the_reference():
    env = dict(os.environ, MIRT_CONTRACT="default")
    env.pop("MIRT_LIB_PATH", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "view_ao_child.py")], env=env, capture_output=True, text=True, timeout=600)
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0, (lines[-1:] or r.stderr[-2000:])
    assert len(lines) == len(VA.FIXTURES) * len(VA.MODELS) and all(l["ok"] for l in lines), lines
    assert all(0.1 <= l["open"] / l["cast"] <= 0.9 for l in lines), lines
