"""The hosts of the ray queries (mirt_trace_closest, mirt_trace_occluded):

  * pyhost/rays.py with cuda tensors on a non-default torch stream equals the Buffer path byte for byte;
  * `cli.js trace` writes the bytes the Python call does (skipped without node, as the other JavaScript tests are);
  * the symbols appear in include/mirt.h, in `nm -D` of both libraries, in pyhost/mirt.py's table and in the addon.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import rays_common as R
from conftest import HOST, PAGE, ROOT, load_fixture

PKG_DIR = os.path.join(ROOT, "2015-raytracing_amd")
SYMBOLS = ("mirt_trace_closest", "mirt_trace_occluded", "mirt_trace_deferred")
node = shutil.which("node")


@pytest.mark.gpu
@pytest.mark.parametrize("stratum", ["staged", "single_cell"])
def test_torch_tensors_on_a_side_stream_equal_the_buffer_path(pkg, stratum):
    import torch
    from raytracing_amd.pyhost import mirt, rays as prays
    sc = R.scene(stratum)
    rays, _ = R.rays_of(stratum)
    ctx = mirt.Context(0)
    t = R.Tracer(ctx, sc)
    try:
        hits, sets, _ = t.closest(rays)
        occ, _ = t.occluded(rays)
        side = torch.cuda.Stream(device=0)
        with torch.cuda.stream(side):
            rt = torch.from_numpy(rays.copy()).to("cuda:0")
            th, ts = prays.trace_closest(ctx, t.dev, rt, want_sets=True)
            only = prays.trace_closest(ctx, t.dev, rt)
            to = prays.trace_occluded(ctx, t.dev, rt)
            ids = th[:, 7].view(torch.int32).cpu().numpy()
            th, ts, only, to = th.cpu().numpy(), ts.cpu().numpy(), only.cpu().numpy(), to.cpu().numpy()
        side.synchronize()
        assert th.tobytes() == hits.tobytes() and only.tobytes() == hits.tobytes()
        assert ts.view(np.uint32).tobytes() == sets.tobytes() and to.tobytes() == occ.tobytes()
        assert np.array_equal(ids, hits[:, 7].view(np.int32)) and (ids >= 0).any() and (ids == -1).any()
        assert R.hits_differ("against the oracle", th, R.closest_of(stratum)[0]) is None
        # the context is back on its own stream and works as before
        again, _, _ = t.closest(rays)
        assert again.tobytes() == hits.tobytes()
        empty = prays.trace_occluded(ctx, t.dev, torch.zeros((0, 8), dtype=torch.float32, device="cuda:0"))
        assert empty.shape == (0,) and empty.dtype == torch.uint8
        with pytest.raises(ValueError):
            prays.trace_closest(ctx, t.dev, torch.zeros((4, 7), dtype=torch.float32, device="cuda:0"))
    finally:
        t.release()
        ctx.destroy()


@pytest.mark.gpu
@pytest.mark.skipif(node is None, reason="node is not installed")
def test_cli_trace_writes_the_bytes_the_python_call_does(pkg, tmp_path):
    """the fixture's scene_json is what the JavaScript host packs from tests/scenes/page/scenes/gems.xml"""
    from raytracing_amd.pyhost import mirt
    _, sc = load_fixture("own_gems_48x36_r4")
    rays, _ = R.make_rays(sc, seed=77)
    ctx = mirt.Context(0)
    t = R.Tracer(ctx, sc)
    try:
        hits, sets, _ = t.closest(rays)
        occ, _ = t.occluded(rays)
    finally:
        t.release()
        ctx.destroy()
    assert (sets != R.NO_SET).any() and (sets == R.NO_SET).any() and occ.any() and not occ.all()
    rf, hf, sf, of = (str(tmp_path / n) for n in ("rays.f32", "hits.f32", "sets.u32", "occ.u8"))
    rays.tofile(rf)
    xml = os.path.join(PAGE, "scenes", "gems.xml")
    r = subprocess.run([node, os.path.join(HOST, "cli.js"), "trace", xml, rf, hf, "--sets", sf], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert open(hf, "rb").read() == hits.tobytes(), "hits"
    assert open(sf, "rb").read() == sets.tobytes(), "sets"
    r = subprocess.run([node, os.path.join(HOST, "cli.js"), "trace", xml, rf, of, "--occluded"], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert open(of, "rb").read() == occ.tobytes(), "occluded"


def test_the_symbols_are_in_the_header_the_libraries_the_binding_and_the_addon(pkg):
    from raytracing_amd.pyhost import mirt
    header = open(os.path.join(ROOT, "include", "mirt.h")).read()
    for lib in ("libmirt.so", "libmirt_default.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG_DIR, lib)], capture_output=True, text=True, check=True).stdout
        exported = set(re.findall(r"\bT (mirt_\w+)", out))
        for s in SYMBOLS:
            assert s in exported, (lib, s)
    for s in SYMBOLS:
        assert re.search(r"MIRT_API\s+int\s+" + s + r"\s*\(", header), s
        assert s in mirt.SYMBOLS and hasattr(mirt.lib(), s), s
    for name in ("mirt_ray", "mirt_hit"):
        assert re.search(r"typedef struct " + name + r" \{[^}]*\} " + name + ";", header), name
    for method in ("trace_closest", "trace_occluded", "trace_deferred"):
        assert callable(getattr(mirt.Context, method))
    napi = open(os.path.join(PKG_DIR, "csrc", "addon", "mirt_napi.cc")).read()
    for js, s in zip(("traceClosest", "traceOccluded", "traceDeferred"), SYMBOLS):
        assert f'{{"{js}", ' in napi and s + "(" in napi, js
    addon = os.path.join(PKG_DIR, "mirt.node")
    if os.path.exists(addon):   # built where the Node headers are (csrc/addon/build_addon.sh)
        out = subprocess.run(["nm", "-D", "--undefined-only", addon], capture_output=True, text=True, check=True).stdout
        for s in SYMBOLS:
            assert re.search(r"\bU " + s + r"\b", out), ("mirt.node", s)
