"""The JavaScript host's guide buffers: `cli.js render ... --guides PREFIX` writes PREFIX.normal_hits.f32 and PREFIX.albedo_depth.f32 (raw
little-endian float4 rows, mirt_render_guides through the N-API addon: queue.renderGuides) beside the frame.  They equal the Python host's arrays
for the same scene -- the fixture's scene_json is what the JavaScript host packs from tests/scenes/page/ -- on one fused renderer and with
`--gpus 2` on the one device of the box, where each context renders its row tile's guides and the tiles are gathered like radiance."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import HOST, PAGE, load_fixture
from guides_common import difference

node = shutil.which("node")
pytestmark = pytest.mark.skipif(node is None, reason="node is not installed")


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [[], ["--gpus", "2"]])
def test_node_guides_equal_the_python_hosts(pkg, tmp_path, flags):
    from raytracing_amd.pyhost import mirt, render, scene
    fx, sc = load_fixture("own_gems_48x36_r4")
    out, prefix = str(tmp_path / "frame.rgba"), str(tmp_path / "g")
    r = subprocess.run([node, os.path.join(HOST, "cli.js"), "render", os.path.join(PAGE, "scenes", "gems.xml"), "48", "36", "4", "1", out, *flags, "--guides", prefix],
                       capture_output=True, env=dict(os.environ, MIRT_GROUP_ALLOW_REPEATED_DEVICES="1"))
    assert r.returncode == 0, r.stderr.decode()
    assert np.array_equal(np.fromfile(out, np.uint8).reshape(-1, 4), fx["pixel"]), "the frame beside the guides"
    ctx = mirt.Context(0)
    fr = render.FusedRenderer(ctx, scene.PackedScene(dict(sc.d)))
    try:
        nh, ad = fr.guides()
    finally:
        fr.release()
        ctx.destroy()
    assert nh[:, 3].max() > 0
    for name, want in (("normal_hits", nh), ("albedo_depth", ad)):
        got = np.fromfile(f"{prefix}.{name}.f32", np.float32)
        assert got.size == 48 * 36 * 4
        d = difference(f"{name} {' '.join(flags)}", got, want)
        assert d is None, d
