"""The JavaScript host's a-trous filter: `cli.js render cornell.xml 48 36 4 1 out.ppm --denoise 3` writes the filtered picture (mirt_filter_atrous
through the N-API addon: queue.filterFrame), on one fused renderer and with `--gpus 2` on the one device of the box, where the radiance and both
guides are gathered to the root and filtered there.  The picture equals the numpy restatement of the header's definition (tests/filter_common.py)
applied to the radiance and the guides the same command writes with `--guides`."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import HOST
from filter_common import DEFAULTS, atrous, difference

node = shutil.which("node")
pytestmark = pytest.mark.skipif(node is None, reason="node is not installed")

W, H, RPP = 48, 36, 4


@pytest.fixture(scope="module")
def cornell_xml(ref_data):
    return os.path.join(ref_data, "a10", "scenes", "cornell.xml")


def read_ppm(path):
    raw = open(path, "rb").read()
    head = f"P6\n{W} {H}\n255\n".encode()
    assert raw.startswith(head) and len(raw) == len(head) + W * H * 3
    return np.frombuffer(raw[len(head):], np.uint8).reshape(-1, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [[], ["--gpus", "2"]])
def test_cli_denoise_equals_the_restatement(pkg, tmp_path, cornell_xml, flags):
    out, prefix = str(tmp_path / "out.ppm"), str(tmp_path / "g")
    r = subprocess.run([node, os.path.join(HOST, "cli.js"), "render", cornell_xml, str(W), str(H), str(RPP), "1", out, *flags, "--denoise", "3", "--guides", prefix],
                       capture_output=True, env=dict(os.environ, MIRT_GROUP_ALLOW_REPEATED_DEVICES="1"))
    assert r.returncode == 0, r.stderr.decode()
    rad = np.fromfile(out + ".radiance.f32", np.float32).reshape(-1, 4)
    nh = np.fromfile(prefix + ".normal_hits.f32", np.float32).reshape(-1, 4)
    ad = np.fromfile(prefix + ".albedo_depth.f32", np.float32).reshape(-1, 4)
    assert rad.shape[0] == W * H and (nh[:, 3] > 0).mean() > 0.5
    want_f, want_p = atrous(rad, nh, ad, W, H, np.float32(1.0 / RPP), **dict(DEFAULTS, iterations=3))
    d = difference(f"filtered {' '.join(flags)}", np.fromfile(out + ".filtered.f32", np.float32), want_f)
    assert d is None, d
    got = read_ppm(out)
    assert np.array_equal(got, want_p[:, :3]), f"{int((got != want_p[:, :3]).any(axis=1).sum())} pixels of the picture differ from the restatement"
    assert (want_f[:, :3] != rad[:, :3]).any(), "the picture is filtered"


@pytest.mark.gpu
def test_the_tiled_picture_is_the_single_context_picture(pkg, tmp_path, cornell_xml):
    """--gpus 2 gathers, then filters: the same picture as one context, rows next to the tile border included"""
    outs = []
    for tag, flags in (("one", []), ("two", ["--gpus", "2"])):
        out = str(tmp_path / f"{tag}.ppm")
        r = subprocess.run([node, os.path.join(HOST, "cli.js"), "render", cornell_xml, str(W), str(H), str(RPP), "1", out, *flags, "--denoise"],
                           capture_output=True, env=dict(os.environ, MIRT_GROUP_ALLOW_REPEATED_DEVICES="1"))
        assert r.returncode == 0, r.stderr.decode()
        outs.append(read_ppm(out))
    assert np.array_equal(outs[0], outs[1])
