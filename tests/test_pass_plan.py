"""CPU: the launch plan of a fused pass (csrc/pt_pass_plan.hpp), dumped by tests/pass_plan_dump.cpp and compared with the rules as the
prose states them (pt_launch.hpp FusedArgs, DESIGN.md section 5, include/mirt.h): which passes resolve their pixels in the kernel and may do
without `acu`, the segments of a pixel's rays, every launch's region of the deferred-block mask, the alternating carry arrays, the scratch
buffer's one size, and the route mirt_render_passes takes.  The segment lengths come from profiles/resolve_counts_bench.py::segments, an
independent statement of the rule.  No device: the header is plain integer arithmetic."""
import importlib.util
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "2015-raytracing_amd", "csrc")
RPPS = [1, 4, 9, 16, 64, 100, 121, 256, 289, 400, 512, 768, 1024, 2304, 8192, 16384, 1 << 24]
TILES = [1, 7 * 5, 32 * 24, 1920 * 1080]   # 7 x 5: npix * len is no multiple of 256 for any segment shorter than 256
MAX_RAYS = 0xFFFFFF00                      # what one tile may hold (mirt_render_pass refuses more)
ONE_LAUNCH, ONE_LAUNCH_EVERY, ORDINARY_PASSES = 0, 1, 2
FIELDS = ("rpp", "npix", "passes", "fresh", "acu", "pixel", "radiance", "every", "inpass")


def _segments(rpp):
    spec = importlib.util.spec_from_file_location("resolve_counts_bench", os.path.join(ROOT, "profiles", "resolve_counts_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.segments(rpp)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++ to compile tests/pass_plan_dump.cpp with")
    exe = str(tmp_path_factory.mktemp("pass_plan") / "pass_plan_dump")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "pass_plan_dump.cpp"), "-o", exe],
                   check=True)

    def run(requests):
        text = "".join(" ".join(str(int(r[f])) for f in FIELDS) + "\n" for r in requests)
        out = subprocess.run([exe], input=text, stdout=subprocess.PIPE, text=True, check=True).stdout
        chunks = out.split("plan ")[1:]
        assert len(chunks) == len(requests)
        res = []
        for c in chunks:
            head, _, rest = c.partition("\n")
            plan = dict(kv.split("=") for kv in head.split())
            segs = np.array(rest.replace("seg", " ").split(), dtype=np.int64).reshape(-1, 8)
            res.append((plan, segs))
        return res
    return run


def test_header_is_host_only():
    """nothing but <stdint.h> / <stddef.h>: it compiles alone, without a HIP header"""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-fsyntax-only", "-x", "c++", os.path.join(CSRC, "pt_pass_plan.hpp")], check=True)
    text = open(os.path.join(CSRC, "pt_pass_plan.hpp")).read()
    includes = [l.split()[1] for l in text.splitlines() if l.startswith("#include")]
    assert sorted(includes) == ["<stddef.h>", "<stdint.h>"]


def requests_for(rpp):
    out = []
    for npix in TILES:
        if npix * rpp > MAX_RAYS:
            continue
        for acu, fresh, pixel, radiance, inpass, passes, every in itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (1, 0), (1, 4), (0, 1)):
            out.append(dict(rpp=rpp, npix=npix, passes=passes, fresh=fresh, acu=acu, pixel=pixel, radiance=radiance, every=every, inpass=inpass))
    return out


def resolves_in_prose(r):
    """The pass writes its own pixels: the switch is on, there is an output buffer, and the count divides 256 or is above 256.  A pass without
    `acu` must also be a frame's first; one that keeps `acu` resolves above 256 only at 256 x 2^k, k <= 5."""
    rpp = r["rpp"]
    if not r["inpass"] or not (r["pixel"] or r["radiance"]) or not (rpp > 256 or 256 % rpp == 0):
        return False
    if r["acu"]:
        return rpp <= 256 or rpp in [256 << k for k in range(6)]
    return bool(r["fresh"])


def ceil_div(a, b):
    return -(-a // b)


@pytest.mark.parametrize("rpp", RPPS)
def test_plan(dump, rpp):
    reqs = requests_for(rpp)
    assert len(reqs) >= 128 * 2, "at least the 1-pixel and the 7 x 5 tile fit at every count"
    cut = _segments(rpp)                        # the lengths when the pass resolves: power-of-two pieces of at most 256, or the whole pixel
    assert sum(cut) == rpp
    if rpp > 256:
        assert all(n <= 256 and n & (n - 1) == 0 for n in cut) and len(cut) == rpp // 256 + bin(rpp % 256).count("1")
    else:
        assert cut == [rpp]
    seen = set()
    for r, (plan, segs) in zip(reqs, dump(reqs)):
        tag = str(r)
        npix, passes = r["npix"], r["passes"]
        P = {k: int(v) for k, v in plan.items() if "+" not in v}
        assert P["rpp"] == rpp and P["npix"] == npix, tag

        # -- the verdicts
        resolves = resolves_in_prose(r)
        seen.add(resolves)
        assert P["resolves"] == resolves, tag
        assert P["null_acu_ok"] == (bool(r["acu"]) or resolves), tag                      # acu may be null only where the pass resolves (then it is fresh)
        assert P["null_acu_ok_passes"] == (bool(r["acu"]) or (resolves and rpp > 1)), tag   # mirt_render_passes: and rays_per_pixel > 1

        # -- the route of mirt_render_passes: 1 ray per pixel couples the rows -> ordinary passes; no frames in between -> one launch; every frame
        # from one launch where several passes resolve in the kernel, else ordinary passes
        if rpp == 1:
            route = ORDINARY_PASSES
        elif not r["every"]:
            route = ONE_LAUNCH
        else:
            route = ONE_LAUNCH_EVERY if passes > 1 and resolves else ORDINARY_PASSES
        assert P["route"] == route, tag

        # -- segments tile [0, rpp) in order
        lens = cut if resolves else [rpp]
        n = len(lens)
        assert P["n_segments"] == n == len(segs), tag
        off, length, pitch, first, words, writes_pixel, cw, cr = segs.T
        lens = np.array(lens, dtype=np.int64)
        assert np.array_equal(length, lens), tag
        assert np.array_equal(off, np.cumsum(lens) - lens) and off[-1] + length[-1] == rpp, tag
        assert np.array_equal(pitch, np.where((length == 256) & (rpp > 256), rpp, 256)), tag

        # -- the mask: one bit per block of 256 samples resolving in the pass, else per sample; the launches' regions back to back
        if resolves:
            want_words = (((npix * lens + 255) // 256) + 31) // 32
            assert P["mask_unit"] == 256, tag
        else:
            want_words = np.array([ceil_div(npix * rpp, 32)], dtype=np.int64)
            assert P["mask_unit"] == 1, tag
        assert np.array_equal(words, want_words), tag
        assert np.array_equal(first, np.cumsum(want_words) - want_words), tag            # adjacent and disjoint
        assert P["mask_words"] == int(want_words.sum()) < 1 << 32, tag

        # -- `pixel` goes to the last launch of a resolving pass only
        assert not writes_pixel[:-1].any() and writes_pixel[-1] == resolves, tag

        # -- every frame above 256 rays: the sums alternate between two arrays
        carries = bool(r["every"]) and resolves and rpp > 256
        assert P["carries"] == carries, tag
        if carries:
            assert cw[-1] == 0, tag                          # the last segment writes array 0: the caller's radiance, or scratch
            assert np.array_equal(cr[1:], cw[:-1]), tag      # each goes on from what the one before wrote
            assert (cr != cw).all() and set(cw) | set(cr) <= {0, 1}, tag   # the redo launch reads what the optimistic one read

        # -- scratch: one size, the named regions inside it
        region = {k: tuple(int(x) for x in plan[k].split("+")) for k in ("lens", "sums", "carry0", "carry1")}
        want = {"lens": 8 * npix if rpp == 1 else 0,
                "sums": 16 * npix if resolves and rpp > 256 and not r["every"] and not r["radiance"] else 0,
                "carry0": passes * npix * 16 if carries and not r["radiance"] else 0,
                "carry1": passes * npix * 16 if carries else 0}
        assert {k: v[1] for k, v in region.items()} == want, tag
        if rpp == 1:
            total = 8 * npix
        elif carries:
            total = passes * npix * 16 * (1 if r["radiance"] else 2)
        elif resolves and rpp > 256 and not r["radiance"]:
            total = 16 * npix
        else:
            total = 0
        assert P["scratch"] == total, tag
        used = sorted((o, o + b) for o, b in region.values() if b)
        assert all(e <= total for _, e in used) and all(a[1] <= b[0] for a, b in zip(used, used[1:])), tag
    assert seen == ({False, True} if rpp > 256 or 256 % rpp == 0 else {False}), "both verdicts occur at every count that can resolve"
