"""The hosts of mirt_trace_radiance:

  * pyhost/rays.py trace_radiance with cuda tensors on a non-default torch stream equals the Buffer path byte for byte, seeds included;
  * the Node binding (queue.traceRadiance) and `cli.js trace --radiance` write the bytes the Python call does (skipped without node, as the other
    JavaScript tests are);
  * the symbols appear in `nm -D` of both libraries, in pyhost/mirt.py's table and in the addon.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import a10_pass as A
import radiance_common as RC
import rays_common as R
from conftest import HOST, PAGE, ROOT, load_fixture

PKG_DIR = os.path.join(ROOT, "2015-raytracing_amd")
SYMBOLS = ("mirt_trace_radiance", "mirt_radiance_deferred")
node = shutil.which("node")


@pytest.mark.gpu
def test_torch_tensors_on_a_side_stream_equal_the_buffer_path(pkg):
    import torch
    from raytracing_amd.pyhost import mirt, rays as prays
    stratum = "staged"
    sc = R.scene(stratum)
    rays, _ = R.rays_of(stratum)
    seeds = RC.seeds_of(stratum)
    ctx = mirt.Context(0)
    t = RC.RadianceTracer(ctx, sc)
    try:
        acu, sd, _ = t.run(rays, seeds, samples=2, bounces=3)
        d = RC.differ("the Buffer path against the oracle", (acu, sd), RC.radiance_of(stratum, 2, 3))
        assert d is None, d
        no_em = t.run(rays, seeds, samples=1, bounces=3, flags=RC.NO_EMITTERS)
        side = torch.cuda.Stream(device=0)
        with torch.cuda.stream(side):
            rt = torch.from_numpy(rays.copy()).to("cuda:0")
            st = torch.from_numpy(seeds.copy()).to("cuda:0")
            out = prays.trace_radiance(ctx, t.dev, rt, st, samples=2, bounces=3)
            got, got_seeds = out.cpu().numpy(), st.cpu().numpy()
            # one sample, then one more into the same tensor: the joint call's result
            st2 = torch.from_numpy(seeds.copy()).to("cuda:0")
            first = prays.trace_radiance(ctx, t.dev, rt, st2, samples=1, bounces=3)
            again = prays.trace_radiance(ctx, t.dev, rt, st2, samples=1, bounces=3, accumulate_into=first)
            assert again is first
            split, split_seeds = again.cpu().numpy(), st2.cpu().numpy()
            st3 = torch.from_numpy(seeds.copy()).to("cuda:0")
            dark = prays.trace_radiance(ctx, t.dev, rt, st3, samples=1, bounces=3, emitters=False).cpu().numpy()
            dark_seeds = st3.cpu().numpy()
        side.synchronize()
        assert got.shape == (len(rays), 4) and got.dtype == np.float32
        assert got.tobytes() == acu.tobytes() and got_seeds.tobytes() == sd.tobytes()
        assert split.tobytes() == acu.tobytes() and split_seeds.tobytes() == sd.tobytes()
        assert dark.tobytes() == no_em[0].tobytes() and dark_seeds.tobytes() == no_em[1].tobytes()
        # the context is back on its own stream and works as before
        assert t.run(rays, seeds, samples=2, bounces=3)[0].tobytes() == acu.tobytes()
        empty = prays.trace_radiance(ctx, t.dev, torch.zeros((0, 8), dtype=torch.float32, device="cuda:0"), torch.zeros((0,), dtype=torch.int32, device="cuda:0"))
        assert empty.shape == (0, 4) and empty.dtype == torch.float32
        with pytest.raises(ValueError):
            prays.trace_radiance(ctx, t.dev, rt, torch.zeros((4,), dtype=torch.int32, device="cuda:0"))
        with pytest.raises(ValueError):
            prays.trace_radiance(ctx, t.dev, rt, st.to(torch.int64))
    finally:
        t.release()
        ctx.destroy()


@pytest.mark.gpu
@pytest.mark.skipif(node is None, reason="node is not installed")
def test_cli_trace_radiance_writes_the_bytes_the_python_call_does(pkg, tmp_path):
    """the fixture's scene_json is what the JavaScript host packs from tests/scenes/page/scenes/gems.xml; cli.js reaches the library through the
    Node binding (queue.traceRadiance) and takes its seeds from mirt_seed_fill(0, count, X), which a10_pass.make_seeds restates"""
    from raytracing_amd.pyhost import mirt
    _, sc = load_fixture("own_gems_48x36_r4")
    rays, _ = R.make_rays(sc, seed=77)
    n = len(rays)
    ctx = mirt.Context(0)
    t = RC.RadianceTracer(ctx, sc)
    try:
        filled = ctx.buffer(n * 4)
        ctx.seed_fill(filled, 0, n, 5)
        seeds = filled.read(np.int32)
        filled.release()
        assert np.array_equal(seeds, A.make_seeds(n, seed_base=5))
        want, _, _ = t.run(rays, seeds, samples=2, bounces=3)
        want_dark, _, _ = t.run(rays, seeds, samples=1, bounces=5, flags=RC.NO_EMITTERS)
    finally:
        t.release()
        ctx.destroy()
    d = RC.differ("the Python call against the oracle", (want, seeds), (RC.expected_radiance(sc, rays, seeds, 2, 3)[0], seeds))
    assert d is None, d
    with np.errstate(invalid="ignore"):
        assert (want[:, 3] > 0).any() and (want[:, 3] == 0).any()
    rf, of = str(tmp_path / "rays.f32"), str(tmp_path / "radiance.f32")
    rays.tofile(rf)
    xml = os.path.join(PAGE, "scenes", "gems.xml")
    r = subprocess.run([node, os.path.join(HOST, "cli.js"), "trace", xml, rf, of, "--radiance", "--samples", "2", "--bounces", "3", "--seed-base", "5"], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert open(of, "rb").read() == want.tobytes(), "radiance"
    r = subprocess.run([node, os.path.join(HOST, "cli.js"), "trace", xml, rf, of, "--radiance", "--seed-base", "5", "--no-emitters"], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert open(of, "rb").read() == want_dark.tobytes(), "radiance with --no-emitters, the default samples and bounces"


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
    assert re.search(r"typedef struct mirt_radiance_desc \{[^}]*\} mirt_radiance_desc;", header)
    for name, value in (("MIRT_RADIANCE_ACCUMULATE", mirt.RADIANCE_ACCUMULATE), ("MIRT_RADIANCE_NO_EMITTERS", mirt.RADIANCE_NO_EMITTERS),
                        ("MIRT_RADIANCE_MAX_SAMPLES", mirt.RADIANCE_MAX_SAMPLES)):
        assert int(re.search(r"#define " + name + r" (\d+)u", header).group(1)) == value, name
    for method in ("trace_radiance", "radiance_deferred"):
        assert callable(getattr(mirt.Context, method))
    assert callable(prays.trace_radiance)
    napi = open(os.path.join(PKG_DIR, "csrc", "addon", "mirt_napi.cc")).read()
    for js, s in zip(("traceRadiance", "radianceDeferred"), SYMBOLS):
        assert f'{{"{js}", ' in napi and s + "(" in napi, js
    addon = os.path.join(PKG_DIR, "mirt.node")
    if os.path.exists(addon):   # built where the Node headers are (csrc/addon/build_addon.sh)
        out = subprocess.run(["nm", "-D", "--undefined-only", addon], capture_output=True, text=True, check=True).stdout
        for s in SYMBOLS:
            assert re.search(r"\bU " + s + r"\b", out), ("mirt.node", s)
