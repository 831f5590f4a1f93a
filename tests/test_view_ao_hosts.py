"""The hosts of mirt_view_ao / mirt_view_ao_deferred:

  * CPU: the Python wrappers' marshalling -- Context.view_ao hands the C entry the three descriptors by reference with their struct sizes and
    the two buffer handles, its defaults are MIRT_AO_DEFAULT_* of include/mirt.h, an _AoDesc goes through as given; the symbols are in the
    header, both libraries, pyhost's table, the addon and webcl.js; `cli.js --view-ao` without `--view` exits 2 and the thin lens's `--ao`
    beside `--view` still does (skipped without node, as the other JavaScript tests are);
  * GPU: pyhost/rays.py view_ao with cuda tensors equals the C-ABI call on buffers; Node's queue.viewAo through `cli.js render ... --view fisheye
    --view-ao PREFIX` writes the C ABI's pairs, the .pgm follows the rounding rule (floor(255 * open / cast + 0.5), 0 where cast is 0), and the
    flag combines with --view-guides and --view-denoise without changing them.
"""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import a10_pass as A
import view_ao_common as VA
import view_common as V
from conftest import HOST, PAGE, ROOT, load_fixture

PKG_DIR = os.path.join(ROOT, "2015-raytracing_amd")
SYMBOLS = ("mirt_view_ao", "mirt_view_ao_deferred")
node = shutil.which("node")
W, H, K = 13, 7, 2


def header_define(name):
    m = re.search(r"#define\s+" + name + r"\s+([0-9.]+)[uf]?", open(os.path.join(ROOT, "include", "mirt.h")).read())
    assert m, name
    return float(m.group(1))


class _Recorder:
    def __init__(self):
        self.calls = []

    def mirt_view_ao(self, *args):
        self.calls.append(args)
        return 0

    def mirt_view_ao_deferred(self, ctx, out):
        out._obj.value = 41
        return 0


def test_context_view_ao_marshals_the_descriptors_and_defaults(pkg, monkeypatch):
    from raytracing_amd.pyhost import mirt
    assert (mirt.AO_DEFAULT_SAMPLES, mirt.AO_MAX_SAMPLES) == (header_define("MIRT_AO_DEFAULT_SAMPLES"), header_define("MIRT_AO_MAX_SAMPLES"))
    assert np.float32(mirt.AO_DEFAULT_BIAS) == np.float32(header_define("MIRT_AO_DEFAULT_BIAS"))
    res, args = mirt.SYMBOLS["mirt_view_ao"]
    assert res is C.c_int and args == [C.c_void_p, C.POINTER(mirt._PassDesc), C.POINTER(mirt._ViewDesc), C.POINTER(mirt._AoDesc), C.c_void_p, C.c_void_p]
    assert mirt.SYMBOLS["mirt_view_ao_deferred"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)])
    assert C.sizeof(mirt._AoDesc) == 16 and [f[0] for f in mirt._AoDesc._fields_] == ["struct_size", "samples", "radius", "bias"]
    rec = _Recorder()
    monkeypatch.setattr(mirt, "lib", lambda: rec)
    ctx = mirt.Context(0, _handle=0x1234)
    seeds, out = mirt.Buffer(ctx, C.c_void_p(0x10), 64), mirt.Buffer(ctx, C.c_void_p(0x20), 64)
    scene_desc = mirt._PassDesc()
    scene_desc.struct_size = C.sizeof(mirt._PassDesc)
    view = mirt.view_desc("equirect", W, H, k=K, eye=(0, 0, 0), look_at=(0, 0, -1))
    ctx.view_ao(scene_desc, view, seeds, out)
    h, d, v, ao, s, o = rec.calls[-1]
    assert h.value == 0x1234 and d._obj is scene_desc and v._obj is view and s.value == 0x10 and o.value == 0x20
    assert v._obj.struct_size == C.sizeof(mirt._ViewDesc) and (v._obj.width, v._obj.height, v._obj.k) == (W, H, K)
    a = ao._obj
    assert (a.struct_size, a.samples, a.bias) == (16, mirt.AO_DEFAULT_SAMPLES, np.float32(mirt.AO_DEFAULT_BIAS)) and math.isinf(a.radius) and a.radius > 0
    ctx.view_ao(scene_desc, view, seeds, out, samples=7, radius=2.5, bias=0.0)
    a = rec.calls[-1][3]._obj
    assert (a.struct_size, a.samples, a.radius, a.bias) == (16, 7, 2.5, 0.0)
    given = mirt._AoDesc(12, 9, 1.0, 0.5)   # an _AoDesc goes through as it is, its size field included
    ctx.view_ao(scene_desc, view, seeds, out, given)
    assert rec.calls[-1][3]._obj is given
    ctx.view_ao(None, None, None, None)      # NULLs reach the library, which refuses them
    assert rec.calls[-1][1] is None and rec.calls[-1][2] is None and rec.calls[-1][4] is None and rec.calls[-1][5] is None
    assert ctx.view_ao_deferred() == 41


def test_the_symbols_are_in_the_header_the_libraries_the_binding_and_the_addon(pkg):
    from raytracing_amd.pyhost import mirt, rays as prays
    header = open(os.path.join(ROOT, "include", "mirt.h")).read()
    for lib in ("libmirt.so", "libmirt_default.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG_DIR, lib)], capture_output=True, text=True, check=True).stdout
        exported = set(re.findall(r"\bT (mirt_\w+)", out))
        for s in SYMBOLS:
            assert s in exported, (lib, s)
    for s in SYMBOLS:
        assert re.search(r"MIRT_API\s+int\s+" + s + r"\s*\(", header), s
        assert s in mirt.SYMBOLS and hasattr(mirt.lib(), s), s
    assert "MIRT_ABI_VERSION 4" in header and "NOT BUILT: ambient occlusion" not in header
    assert callable(mirt.Context.view_ao) and callable(mirt.Context.view_ao_deferred) and callable(prays.view_ao)
    napi = open(os.path.join(PKG_DIR, "csrc", "addon", "mirt_napi.cc")).read()
    for js, s in zip(("viewAo", "viewAoDeferred"), SYMBOLS):
        assert f'{{"{js}", ' in napi and s + "(" in napi, js
    webcl = open(os.path.join(HOST, "webcl.js")).read()
    for js in ("viewAo(", "viewAoDeferred()", "hasViewAo()"):
        assert js in webcl, js
    addon = os.path.join(PKG_DIR, "mirt.node")
    if os.path.exists(addon):   # built where the Node headers are (csrc/addon/build_addon.sh)
        out = subprocess.run(["nm", "-D", "--undefined-only", addon], capture_output=True, text=True, check=True).stdout
        for s in SYMBOLS:
            assert re.search(r"\bU " + s + r"\b", out), ("mirt.node", s)


@pytest.mark.skipif(node is None, reason="node is not installed")
def test_cli_refuses_view_ao_without_view_and_ao_beside_view(tmp_path):
    """both are decided from the arguments alone, before a device is opened"""
    xml = os.path.join(PAGE, "scenes", "gems.xml")
    base = [node, os.path.join(HOST, "cli.js"), "render", xml, str(W), str(H), str(K * K), "1", str(tmp_path / "f.ppm")]
    r = subprocess.run(base + ["--view-ao", str(tmp_path / "a")], capture_output=True)
    assert r.returncode == 2 and b"--view-ao needs --view" in r.stderr, r.stderr.decode()
    r = subprocess.run(base + ["--view", "fisheye", "--ao", str(tmp_path / "a")], capture_output=True)
    assert r.returncode == 2 and b"--view is not available with --ao" in r.stderr and b"--view-ao" in r.stderr, r.stderr.decode()
    r = subprocess.run(base + ["--view", "fisheye", "--view-ao"], capture_output=True)   # no prefix: the usage text
    assert r.returncode == 2 and b"--view-ao PREFIX" in r.stderr
    assert not list(tmp_path.iterdir()), "a refused command wrote a file"


@pytest.mark.gpu
def test_torch_tensors_equal_the_buffer_call(pkg):
    import torch
    from raytracing_amd.pyhost import mirt, rays as prays
    name = VA.FIXTURES[1]
    sc = VA.scene(name)
    v = V.standard_view(sc, "fisheye")
    want = VA.expected_standard(name, "fisheye")
    d = VA.not_vacuous(f"{name} fisheye", want, VA.SAMPLES, v.rpp, need_empty=True)
    assert d is None, d
    ctx = mirt.Context(0)
    ao = VA.Ao(ctx, sc, v.n_rays, v.n_pixels)
    try:
        got, clean = ao.run(v)
        assert clean and VA.difference("the buffer call", got, want) is None
        seeds = torch.from_numpy(A.make_seeds(v.n_rays)).to("cuda:0")
        before = seeds.clone()
        t = prays.view_ao(ctx, ao.dev, v.desc(), seeds, samples=VA.SAMPLES, radius=1.0, bias=VA.BIAS)
        assert t.shape == (v.n_pixels, 2) and t.dtype == torch.uint32 and t.is_cuda
        assert t.cpu().numpy().tobytes() == got.tobytes() and torch.equal(seeds, before)
        # the defaults are the header's: 4 AO rays, unbounded, bias 0.001
        t = prays.view_ao(ctx, ao.dev, v.desc(), seeds)
        dflt, _ = ao.run(v, samples=mirt.AO_DEFAULT_SAMPLES, radius=float("inf"), bias=mirt.AO_DEFAULT_BIAS)
        assert t.cpu().numpy().tobytes() == dflt.tobytes() and dflt[:, 1].max() == v.rpp * 4
        with pytest.raises(ValueError):
            prays.view_ao(ctx, ao.dev, v.desc(), seeds[:-1])
    finally:
        ao.release()
        ctx.destroy()


def box_centre(sc):
    b = np.asarray(sc.bounds, np.float64)
    return [(float(b[c]) + float(b[4 + c])) / 2 for c in range(3)]


@pytest.mark.gpu
@pytest.mark.skipif(node is None, reason="node is not installed")
def test_cli_view_ao_writes_the_bytes_the_c_abi_does(pkg, tmp_path):
    """cli.js reaches the library through the Node binding (queue.viewAo, before the first pass) and takes its seeds from mirt_seed_fill(0, count, 0)"""
    from raytracing_amd.pyhost import mirt
    _, sc = load_fixture("own_gems_48x36_r4")
    eye = box_centre(sc)
    look = [eye[0] + 0.3, eye[1] - 0.2, eye[2] - 1.0]
    n, npx = W * H * K * K, W * H
    samples, radius, bias = 3, 0.75, 0.002
    ctx = mirt.Context(0)
    dev = mirt.DeviceScene(ctx, sc)
    sb, ab, nb, db = (ctx.buffer(b) for b in (n * 4, npx * 8, npx * 16, npx * 16))
    try:
        ctx.seed_fill(sb, 0, n)
        view = mirt.view_desc("fisheye", W, H, k=K, eye=eye, look_at=look, half_angle=np.float32(100.0 / 2 * np.pi / 180), tone=1.0 / (K * K))
        ctx.view_ao(dev.pass_desc(None, None), view, sb, ab, samples, radius, bias)
        want = ab.read(np.uint32).reshape(-1, 2).copy()
        ctx.view_ao(dev.pass_desc(None, None), view, sb, ab)
        want_default = ab.read(np.uint32).reshape(-1, 2).copy()
        ctx.view_guides(dev.pass_desc(None, None), view, nb, db)
        want_nh = nb.read(np.float32).copy()
    finally:
        for b in (sb, ab, nb, db):
            b.release()
        dev.release()
        ctx.destroy()
    open_, cast = want[:, 0].astype(np.int64), want[:, 1].astype(np.int64)
    assert cast.sum() > 0 and 0 < open_.sum() < cast.sum() and (cast == 0).any(), "nothing casts, every AO ray has the same fate, or every pixel casts"
    gray = np.where(cast > 0, np.floor(255.0 * open_ / np.maximum(cast, 1) + 0.5), 0).astype(np.uint8)
    assert len(np.unique(gray)) > 2
    xml = os.path.join(PAGE, "scenes", "gems.xml")
    out, prefix = str(tmp_path / "fish.ppm"), str(tmp_path / "a")
    base = [node, os.path.join(HOST, "cli.js"), "render", xml, str(W), str(H), str(K * K), "1", out]
    cam = ["--view", "fisheye", "--fov", "100", "--look", ",".join(repr(c) for c in look)]
    r = subprocess.run(base + cam + ["--view-ao", prefix, "--ao-samples", str(samples), "--ao-radius", str(radius), "--ao-bias", str(bias)], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert b"ambient occlusion: " in r.stderr
    assert open(prefix + ".ao.u32", "rb").read() == want.tobytes(), "the pairs"
    header = f"P5\n{W} {H}\n255\n".encode()
    pgm = open(prefix + ".ao.pgm", "rb").read()
    assert pgm.startswith(header) and pgm[len(header):] == gray.tobytes(), "the grey picture"
    plain = open(out, "rb").read()
    # the defaults, beside the guides and the filter: the pairs are the defaults', the guides are mirt_view_guides'
    g = str(tmp_path / "g")
    r = subprocess.run(base + cam + ["--view-ao", prefix, "--view-guides", g, "--view-denoise"], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert open(prefix + ".ao.u32", "rb").read() == want_default.tobytes(), "the pairs with the default AO descriptor"
    assert open(g + ".normal_hits.f32", "rb").read() == want_nh.tobytes(), "normal_hits beside --view-ao"
    assert len(open(out + ".radiance.f32", "rb").read()) == npx * 16 and len(open(out, "rb").read()) == len(plain)
