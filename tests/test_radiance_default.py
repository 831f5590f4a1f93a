"""GPU: mirt_trace_radiance under the DEFAULT contract (libmirt_default.so: the reference as its own host builds it) equals that library's own
kernel-by-kernel path on the same rays and seeds -- in a child process with MIRT_CONTRACT=default, as a process loads one libmirt
(tests/radiance_default_child.py)."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT
from random_scenes_common import STRATA

pytestmark = pytest.mark.gpu


def test_radiance_equals_the_kernel_by_kernel_path_under_the_default_contract():
    env = dict(os.environ, MIRT_CONTRACT="default")
    env.pop("MIRT_LIB_PATH", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "radiance_default_child.py")], env=env, capture_output=True, text=True, timeout=600)
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0, (lines[-1:] or r.stderr[-2000:])
    assert len(lines) == len(STRATA) and all(l["ok"] for l in lines)
    assert all(0 < l["lit"] < l["rays"] and 0 < l["advanced"] < l["rays"] for l in lines), lines
