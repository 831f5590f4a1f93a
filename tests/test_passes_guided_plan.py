"""CPU: the route of mirt_render_passes_guided (csrc/pt_pass_plan.hpp fused_guides_in_passes), dumped by tests/passes_guided_plan_dump.cpp and
compared with the rule as include/mirt.h states it: the launch writes the guides itself where the plan resolves in the kernel, as one segment, at
4, 16 or 64 rays per pixel, on one of mirt_render_passes's one-launch routes, and for several passes with the default multi-pass pairing and -- the class
the measurement excluded -- not in a scene with grids; everywhere else the guide launches follow.  And that the entry point exists: the header declares it, the Python binding lists it, the built libraries export it.  No device."""
import itertools
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
from test_pass_guided_plan import RPPS, TILES, resolves_in_prose

CSRC = os.path.join(ROOT, "2015-raytracing_amd", "csrc")
FIELDS = ("rpp", "npix", "passes", "fresh", "acu", "pixel", "radiance", "every", "inpass", "pairing", "grids")
ONE_LAUNCH, ONE_LAUNCH_EVERY, ORDINARY = 0, 1, 2     # pt::PassRoute
SYMBOL = "mirt_render_passes_guided"


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++ to compile tests/passes_guided_plan_dump.cpp with")
    exe = str(tmp_path_factory.mktemp("passes_guided_plan") / "passes_guided_plan_dump")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "passes_guided_plan_dump.cpp"), "-o", exe],
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
        for acu, fresh, pixel, radiance, inpass, passes, every, pairing in itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (1, 0), (1, 2, 4), (0, 1), (1, 0)):
            for grids in (0, 1):
                out.append(dict(rpp=rpp, npix=npix, passes=passes, fresh=fresh, acu=acu, pixel=pixel, radiance=radiance, every=every, inpass=inpass, pairing=pairing,
                                grids=grids))
    return out


def route_in_prose(r):
    """include/mirt.h, mirt_render_passes: one ray per pixel runs as ordinary passes; without a frame after every pass one launch; with it one launch
    where there are several passes and they resolve in the kernel, ordinary passes elsewhere"""
    if r["rpp"] == 1:
        return ORDINARY
    if not r["every"]:
        return ONE_LAUNCH
    return ONE_LAUNCH_EVERY if r["passes"] > 1 and resolves_in_prose(r) else ORDINARY


@pytest.mark.parametrize("rpp", RPPS)
def test_route(dump, rpp):
    reqs = requests_for(rpp)
    seen = set()
    for r, (resolves, n_segments, route, first_pass_rule, in_launch) in zip(reqs, dump(reqs)):
        assert resolves == resolves_in_prose(r), str(r)
        assert route == route_in_prose(r), str(r)
        want = resolves_in_prose(r) and n_segments == 1 and rpp in (4, 16, 64) and route in (ONE_LAUNCH, ONE_LAUNCH_EVERY)
        # the pairing is a property of the multi-pass kernels: one pass has none.  Several passes of a grid scene: (b) > (a) in both runs of
        # profiles/passes_guided/
        want = want and (r["passes"] == 1 or (bool(r["pairing"]) and not r["grids"]))
        assert in_launch == want, str(r)
        # one pass and no frame after every pass is mirt_render_first_pass_guided's case, whatever the pairing and the grids (with the flag the batch
        # runs as an ordinary pass and the guide launches follow it)
        if r["passes"] == 1 and not r["every"]:
            assert in_launch == first_pass_rule, str(r)
        if r["passes"] == 4:
            assert not first_pass_rule, "fused_guides_in_pass stays a one-pass rule"
        seen.add((bool(in_launch), r["passes"], r["every"], r["grids"]))
    for passes, every, grids in itertools.product((1, 2, 4), (0, 1), (0, 1)):
        possible = rpp in (4, 16, 64) and not (every and passes == 1) and not (grids and passes > 1)
        assert ((True, passes, every, grids) in seen) == possible, (passes, every, grids)


def test_the_fallbacks_of_the_header(dump):
    base = dict(rpp=16, npix=35, passes=4, fresh=1, acu=0, pixel=1, radiance=1, every=0, inpass=1, pairing=1, grids=0)
    cases = [(base, 1), (dict(base, every=1), 1), (dict(base, acu=1, fresh=0), 1), (dict(base, passes=1), 1), (dict(base, passes=64), 1),
             (dict(base, passes=1, grids=1), 1), (dict(base, passes=1, pairing=0), 1), (dict(base, passes=1, grids=1, pairing=0), 1), (dict(base, grids=1), 0), (dict(base, grids=1, every=1), 0), (dict(base, pairing=0), 0), (dict(base, acu=1, pixel=0, radiance=0), 0), (dict(base, inpass=0, acu=1), 0),
             (dict(base, rpp=256), 0), (dict(base, rpp=9, acu=1), 0), (dict(base, rpp=289), 0), (dict(base, passes=1, every=1), 0),
             (dict(base, every=1, inpass=0, acu=1), 0)]
    got = dump([c for c, _ in cases])
    assert [g[4] for g in got] == [w for _, w in cases]


def test_header_is_still_host_only():
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-fsyntax-only", "-x", "c++", os.path.join(CSRC, "pt_pass_plan.hpp")], check=True)
    text = open(os.path.join(CSRC, "pt_pass_plan.hpp")).read()
    includes = [l.split()[1] for l in text.splitlines() if l.startswith("#include")]
    assert sorted(includes) == ["<stddef.h>", "<stdint.h>"]
    assert "getenv" not in text, "the pairing comes in as an argument"
    assert "fused_guides_in_passes" in text


def test_header_declares_and_binding_lists_the_entry_point(pkg):
    from raytracing_amd.pyhost import mirt, render
    header = open(os.path.join(ROOT, "include", "mirt.h")).read()
    assert re.search(r"MIRT_API int mirt_render_passes_guided\(mirt_ctx\* ctx, const mirt_pass_desc\* desc, uint32_t n_passes, uint32_t flags,\s*"
                     r"mirt_buf\* normal_hits,\s*mirt_buf\* albedo_depth\);", header)
    assert SYMBOL in mirt.SYMBOLS
    assert callable(mirt.Context.render_passes_guided)
    assert callable(render.FusedRenderer.execute_passes_guided) and callable(render.FusedRenderer.denoised_passes)
    assert re.search(r"#define MIRT_ABI_VERSION 4\b", header), "the entry point is detected by its symbol: the ABI version stays"


@pytest.mark.parametrize("name", ["libmirt.so", "libmirt_default.so"])
def test_library_exports_the_entry_point(name):
    path = os.path.join(ROOT, "2015-raytracing_amd", name)
    if not os.path.exists(path):
        pytest.skip(f"{name} not built")
    nm = shutil.which("nm")
    if not nm:
        pytest.skip("no nm")
    out = subprocess.run([nm, "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert SYMBOL in exported, f"{name} does not export {SYMBOL}"
