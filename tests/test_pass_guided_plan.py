"""CPU: the route of mirt_render_first_pass_guided (csrc/pt_pass_plan.hpp fused_guides_in_pass), dumped by tests/pass_guided_plan_dump.cpp and
compared with the rule as include/mirt.h states it: the pass writes the guides itself where it resolves its pixels in the kernel, as one segment
and one pass, at 4, 16 or 64 rays per pixel; everywhere else the guide launches follow the pass.  And that the entry points exist: the header
declares them, the Python binding lists them, the built library exports them.  No device."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "2015-raytracing_amd", "csrc")
RPPS = [1, 4, 9, 16, 64, 100, 256, 289, 1024]      # the request grid of tests/test_pass_plan.py
TILES = [1, 7 * 5, 32 * 24, 1920 * 1080]
FIELDS = ("rpp", "npix", "passes", "fresh", "acu", "pixel", "radiance", "every", "inpass")
SYMBOLS = ("mirt_render_first_pass_guided", "mirt_ctx_guided_passes")


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++ to compile tests/pass_guided_plan_dump.cpp with")
    exe = str(tmp_path_factory.mktemp("pass_guided_plan") / "pass_guided_plan_dump")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "pass_guided_plan_dump.cpp"), "-o", exe],
                   check=True)

    def run(requests):
        text = "".join(" ".join(str(int(r[f])) for f in FIELDS) + "\n" for r in requests)
        out = subprocess.run([exe], input=text, stdout=subprocess.PIPE, text=True, check=True).stdout
        rows = [tuple(int(x) for x in l.split()) for l in out.splitlines()]
        assert len(rows) == len(requests)
        return rows
    return run


def requests_for(rpp):
    out = []
    for npix in TILES:
        for acu, fresh, pixel, radiance, inpass, passes, every in itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (1, 0), (1, 4), (0, 1)):
            out.append(dict(rpp=rpp, npix=npix, passes=passes, fresh=fresh, acu=acu, pixel=pixel, radiance=radiance, every=every, inpass=inpass))
    return out


def resolves_in_prose(r):
    """tests/test_pass_plan.py's statement: the switch is on, there is an output buffer, the count divides 256 or is above it; without `acu` the
    pass is a frame's first, with it above 256 only 256 x 2^k, k <= 5"""
    rpp = r["rpp"]
    if not r["inpass"] or not (r["pixel"] or r["radiance"]) or not (rpp > 256 or 256 % rpp == 0):
        return False
    if r["acu"]:
        return rpp <= 256 or rpp in [256 << k for k in range(6)]
    return bool(r["fresh"])


@pytest.mark.parametrize("rpp", RPPS)
def test_route(dump, rpp):
    reqs = requests_for(rpp)
    seen = set()
    for r, (resolves, n_segments, in_pass) in zip(reqs, dump(reqs)):
        assert resolves == resolves_in_prose(r), str(r)
        want = resolves_in_prose(r) and r["passes"] == 1 and rpp in (4, 16, 64)
        assert in_pass == want, str(r)
        if in_pass:
            assert n_segments == 1, str(r)
        seen.add(bool(in_pass))
    # the one-launch route exists at 4, 16 and 64 rays and nowhere else: not at 1 (refused), 256 (a pixel spans four waves), a count that does not
    # divide 256, a count above it
    assert seen == ({False, True} if rpp in (4, 16, 64) else {False})


def test_acu_without_an_output_buffer_and_the_switch_fall_back(dump):
    base = dict(rpp=16, npix=35, passes=1, fresh=1, acu=0, pixel=1, radiance=1, every=0, inpass=1)
    cases = [(base, 1), (dict(base, acu=1), 1), (dict(base, acu=1, pixel=0, radiance=0), 0), (dict(base, inpass=0, acu=1), 0), (dict(base, passes=4), 0)]
    got = dump([c for c, _ in cases])
    assert [g[2] for g in got] == [w for _, w in cases]


def test_header_is_still_host_only():
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-fsyntax-only", "-x", "c++", os.path.join(CSRC, "pt_pass_plan.hpp")], check=True)
    text = open(os.path.join(CSRC, "pt_pass_plan.hpp")).read()
    includes = [l.split()[1] for l in text.splitlines() if l.startswith("#include")]
    assert sorted(includes) == ["<stddef.h>", "<stdint.h>"]
    assert "fused_guides_in_pass" in text


def test_header_declares_and_binding_lists_the_entry_points(pkg):
    from raytracing_amd.pyhost import mirt
    header = open(os.path.join(ROOT, "include", "mirt.h")).read()
    assert re.search(r"MIRT_API int mirt_render_first_pass_guided\(mirt_ctx\* ctx, const mirt_pass_desc\* desc,\s*mirt_buf\* normal_hits, mirt_buf\* albedo_depth\);", header)
    assert re.search(r"MIRT_API int mirt_ctx_guided_passes\(mirt_ctx\* ctx, uint64_t\* count\);", header)
    for name in SYMBOLS:
        assert name in mirt.SYMBOLS
    assert callable(mirt.Context.render_first_pass_guided) and callable(mirt.Context.guided_passes)
    assert re.search(r"#define MIRT_ABI_VERSION 4\b", header), "the entry points are detected by their symbols: the ABI version stays"


@pytest.mark.parametrize("name", ["libmirt.so", "libmirt_default.so"])
def test_library_exports_the_entry_points(name):
    path = os.path.join(ROOT, "2015-raytracing_amd", name)
    if not os.path.exists(path):
        pytest.skip(f"{name} not built")
    nm = shutil.which("nm")
    if not nm:
        pytest.skip("no nm")
    out = subprocess.run([nm, "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for sym in SYMBOLS:
        assert sym in exported, f"{name} does not export {sym}"
