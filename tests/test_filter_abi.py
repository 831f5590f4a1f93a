"""CPU: the a-trous filter's entry point exists in every layer -- include/mirt.h declares mirt_filter_atrous and lays mirt_filter_desc out as the
ctypes struct has it, pyhost binds it, both libraries export it, the addon and the JavaScript host carry it -- and the numpy restatement the GPU
tests compare against (tests/filter_common.py) has the properties the header derives from the definition."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import HOST, ROOT
from filter_common import DEFAULTS, INF_AT, LONELY, NAN_AT, SYN_H, SYN_TONE, SYN_W, atrous, difference, synthetic

PKG = os.path.join(ROOT, "2015-raytracing_amd")
HEADER = os.path.join(ROOT, "include", "mirt.h")


def header_struct_layout():
    """(offsets by field name, size) of mirt_filter_desc as a C compiler lays the header's declaration out on this ABI: 4-byte scalars, 8-byte pointers"""
    text = open(HEADER).read()
    body = re.search(r"typedef struct mirt_filter_desc \{(.*?)\} mirt_filter_desc;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    off, fields, align = 0, {}, 1
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(uint32_t|float|mirt_buf\s*\*)\s*(.*)$", decl)
        assert m, decl
        size = 8 if "*" in m.group(1) else 4
        for name in m.group(2).split(","):
            off = (off + size - 1) // size * size
            fields[name.strip()] = off
            off += size
            align = max(align, size)
    return fields, (off + align - 1) // align * align


def test_the_ctypes_struct_is_the_header_struct(pkg):
    from raytracing_amd.pyhost import mirt
    fields, size = header_struct_layout()
    assert C.sizeof(mirt._FilterDesc) == size == 80
    assert [n for n, _ in mirt._FilterDesc._fields_] == list(fields)
    for name, off in fields.items():
        assert getattr(mirt._FilterDesc, name).offset == off, name


def test_the_header_declares_the_entry_point_and_the_python_binding_carries_it(pkg):
    from raytracing_amd.pyhost import mirt, render
    text = open(HEADER).read()
    assert re.search(r"MIRT_API\s+int\s+mirt_filter_atrous\s*\(\s*mirt_ctx\s*\*\s*\w+,\s*const\s+mirt_filter_desc\s*\*\s*\w+\s*\)", text)
    assert int(re.search(r"#define MIRT_ABI_VERSION (\d+)", text).group(1)) == 4   # a host detects the feature by the symbol
    assert "mirt_filter_atrous" in mirt.SYMBOLS and hasattr(mirt.lib(), "mirt_filter_atrous")
    assert callable(mirt.Context.filter_atrous) and callable(render.FusedRenderer.denoised)
    # the shipped defaults are the header's, in the Python host and in the restatement's module
    for key, macro in (("iterations", "ITERATIONS"), ("normal_power_log2", "NORMAL_POWER_LOG2"), ("sigma_depth", "SIGMA_DEPTH"), ("sigma_colour", "SIGMA_COLOUR")):
        v = float(re.search(rf"#define MIRT_FILTER_DEFAULT_{macro} ([\d.]+)", text).group(1))
        assert mirt.FILTER_DEFAULTS[key] == v == DEFAULTS[key], key
    for name, bit in (("DEMODULATE", mirt.FILTER_DEMODULATE), ("DIRECT", mirt.FILTER_DIRECT), ("TILED", mirt.FILTER_TILED)):
        assert int(re.search(rf"#define MIRT_FILTER_{name} (\d+)u", text).group(1)) == bit


def test_without_a_gpu_the_wrapper_raises_mirt_error(pkg):
    """no device is touched: a handle that is no live context is MIRT_E_HANDLE before anything else, and the wrapper raises it"""
    from raytracing_amd.pyhost import mirt
    d = mirt._FilterDesc()
    d.struct_size = C.sizeof(d)
    assert mirt.lib().mirt_filter_atrous(None, C.byref(d)) == -2
    not_a_context = C.create_string_buffer(64)
    ctx = mirt.Context(0, _handle=C.addressof(not_a_context))
    with pytest.raises(mirt.MirtError) as e:
        ctx.filter_atrous(4, 4, 0.25, None, None, None, pixel=None)
    assert e.value.code == -2


@pytest.mark.parametrize("lib", ["libmirt.so", "libmirt_default.so"])
def test_both_libraries_export_it(pkg, lib):
    path = os.path.join(PKG, lib)
    assert os.path.exists(path), f"{lib} not built"
    names = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT mirt_filter_atrous$", names, re.M)
    strings = subprocess.run(["strings", "-a", path], capture_output=True, text=True, check=True).stdout
    for kernel in ("k_filterPrepare", "k_filterDirect", "k_filterTiled"):
        assert kernel in strings, f"{kernel} is not in the library"


def test_the_kernel_file_is_built_like_the_other_translation_units():
    sh = open(os.path.join(PKG, "csrc", "build.sh")).read()
    assert "pt_kernels_filter.hip" in re.search(r"^SRC=\((.*)\)$", sh, re.M).group(1)
    code = {name: re.sub(r"//.*", "", open(os.path.join(PKG, "csrc", name)).read()) for name in ("pt_kernels_filter.hip", "pt_kernels_upsample.hip", "pt_post.hpp")}
    for name, text in code.items():
        assert not re.search(r"\b(expf?|powf?|sqrtf?|fmaf?)\s*\(", text), f"no exp, pow, sqrt or fma in {name}"
    # one contract for both builds: every quotient goes through div_cr, the only `/` on floats -- defined once, in the shared header
    assert len(re.findall(r"\(double\)\s*n\s*/\s*\(double\)\s*d", code["pt_post.hpp"])) == 1
    assert code["pt_post.hpp"].count("/") == 1
    # ... so what the kernel files divide are the integers of the grid and tile arithmetic: a `/` there has an unsigned literal or one of these
    # integer names on its right, and no floating-point literal or cast on its left
    # (a whitelist by NAME: a float variable called `f` or `step` would slip through, and a new integer divisor has to be added here)
    integer = r"\d+u\b|(?:\(uint32_t\))?(?:step|kTileSide|kTileIn|f)\b"
    for name in ("pt_kernels_filter.hip", "pt_kernels_upsample.hip"):
        assert "(double)" not in code[name] and not re.search(r"\bdiv_cr\s*\([^()]*\)\s*\{", code[name]), f"{name} defines a quotient of its own"
        for m in re.finditer(r"/", code[name]):
            left, right = code[name][:m.start()].rstrip(), code[name][m.end():].lstrip()
            assert re.match(integer, right), f"{name}: `/` applied to {right[:30]!r}"
            assert not re.search(r"(\d\.\d*f?|\df|\(float\)\s*\w+)$", left), f"{name}: {left[-30:]!r} is divided"


def test_the_addon_and_the_javascript_host_export_it():
    node = shutil.which("node")
    addon = os.path.join(PKG, "mirt.node")
    if node is None or not os.path.exists(addon):
        pytest.skip("node or mirt.node not present")
    for name in ("mirt.node", "mirt_default.node"):
        r = subprocess.run([node, "-e", f"const a = require({os.path.join(PKG, name)!r}); process.stdout.write(typeof a.filterAtrous)"], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout == "function", r.stderr
    src = open(os.path.join(HOST, "webcl.js")).read()
    assert re.search(r"\n  filterFrame\(", src)
    usage = subprocess.run([node, os.path.join(HOST, "cli.js")], capture_output=True, text=True)
    assert "--denoise [iterations]" in usage.stderr


# ---- the restatement's own checks ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def syn():
    return synthetic()


def test_restatement_zero_iterations_is_the_identity(syn):
    R, NH, AD = syn
    filtered, pixel = atrous(R, NH, AD, SYN_W, SYN_H, SYN_TONE)
    assert difference("iterations == 0", filtered, R) is None
    v = (R[:, :3] * (np.float32(255) * SYN_TONE)) * np.float32(1.8)
    want = np.where(np.isnan(v), 0, np.clip(v, 0, 255)).astype(np.uint8)
    assert np.array_equal(pixel[:, :3], want) and (pixel[:, 3] == 255).all()


@pytest.mark.parametrize("demodulate", [False, True])
def test_restatement_contains_nan_and_inf_and_passes_background_through(syn, demodulate):
    R, NH, AD = syn
    p = dict(DEFAULTS, iterations=5, demodulate=demodulate)
    filtered, _ = atrous(R, NH, AD, SYN_W, SYN_H, SYN_TONE, **p)
    bad_in = ~np.isfinite(R[:, :3]).all(axis=1)
    bad_out = ~np.isfinite(filtered[:, :3]).all(axis=1)
    assert bad_in.sum() == 2 and np.array_equal(bad_in, bad_out), "a NaN or inf pixel stays where it is and does not spread"
    assert np.isnan(filtered[NAN_AT[0] * SYN_W + NAN_AT[1], 0]) and np.isinf(filtered[INF_AT[0] * SYN_W + INF_AT[1], 1])
    bg = ~(NH[:, 3] > 0)
    assert bg.sum() > 100 and difference("background", filtered[bg], R[bg]) is None
    if not demodulate:
        lonely = LONELY[0] * SYN_W + LONELY[1]   # every tap weighs 0: (I * h0^2) / h0^2 per iteration, I again up to the two roundings
        assert np.allclose(filtered[lonely], R[lonely], rtol=5 * 2.0 ** -23, atol=0)
    live = ~bg & ~bad_in
    assert (filtered[live, :3] != R[live, :3]).any(axis=1).mean() > 0.5, "the filter filters: most live pixels have a tap with a positive weight"
