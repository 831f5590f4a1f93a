"""CPU: the guide-driven upsampler is part of the C ABI -- include/mirt.h declares mirt_upsample_guided and mirt_upsample_desc, both libraries
export the symbol, and the Python binding lists it with a descriptor of the header's layout.  No device."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "2015-raytracing_amd")
HEADER = open(os.path.join(ROOT, "include", "mirt.h")).read()


def test_header_declares_the_entry_point_and_its_descriptor():
    assert re.search(r"MIRT_API\s+int\s+mirt_upsample_guided\s*\(\s*mirt_ctx\s*\*\s*\w*\s*,\s*const\s+mirt_upsample_desc\s*\*", HEADER)
    body = re.search(r"typedef struct mirt_upsample_desc \{(.*?)\} mirt_upsample_desc;", HEADER, re.S)
    assert body, "mirt_upsample_desc is not declared"
    fields = re.findall(r"(\w+)\s*(?:,\s*(\w+)\s*)?;", re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S))
    names = [n for pair in fields for n in pair if n]
    assert names == ["struct_size", "width", "height", "factor", "flags", "normal_power_log2", "tone", "sigma_depth", "radiance_lo", "normal_hits_lo",
                     "albedo_depth_lo", "normal_hits", "albedo_depth", "upsampled", "pixel"], names
    assert re.search(r"#define MIRT_UPSAMPLE_DEMODULATE 1u", HEADER)
    assert int(re.search(r"#define MIRT_ABI_VERSION (\d+)", HEADER).group(1)) == 4, "the entry point is detected by its symbol: the version stays"


@pytest.mark.parametrize("name", ["libmirt.so", "libmirt_default.so"])
def test_both_libraries_export_the_symbol(pkg, name):
    path = os.path.join(PKG, name)
    assert os.path.exists(path), f"{name} is not built"
    # in a process of its own: a process loads one libmirt
    r = subprocess.run([sys.executable, "-c", "import ctypes, sys; sys.exit(0 if hasattr(ctypes.CDLL(sys.argv[1]), 'mirt_upsample_guided') else 3)", path],
                       capture_output=True, text=True)
    assert r.returncode == 0, f"{name} does not export mirt_upsample_guided (exit {r.returncode}) {r.stderr[-500:]}"


def test_the_binding_lists_it(pkg):
    from raytracing_amd.pyhost import mirt
    assert "mirt_upsample_guided" in mirt.SYMBOLS
    d = mirt._UpsampleDesc
    assert [n for n, _ in d._fields_] == ["struct_size", "width", "height", "factor", "flags", "normal_power_log2", "tone", "sigma_depth", "radiance_lo",
                                           "normal_hits_lo", "albedo_depth_lo", "normal_hits", "albedo_depth", "upsampled", "pixel"]
    assert C.sizeof(d) == 8 * 4 + 7 * C.sizeof(C.c_void_p)
    defaults = {k: float(re.search(rf"#define MIRT_UPSAMPLE_DEFAULT_{k.upper()} ([\d.]+)", HEADER).group(1)) for k in ("normal_power_log2", "sigma_depth")}
    assert mirt.UPSAMPLE_DEFAULTS == dict(defaults, normal_power_log2=int(defaults["normal_power_log2"]), demodulate=True)
