"""The JavaScript host's post-process chain in row tiles: `cli.js render ... --gpus N --post-in-tiles` on the one device of the box (a rehearsal
group) filters and upsamples every tile where it is, after a halo exchange (group.exchangeRows, queue.filterFrameRows, queue.upsampleFrameRows
through the N-API addon), and writes the bytes of the single-context command: --denoise over 2 and 3 contexts, --upscale 2 over 2, with and without
--denoise.  Without the flag nothing changes: tests/test_filter_js.py and tests/test_upsample_js.py hold that."""
import os
import shutil
import subprocess

import pytest

from conftest import HOST

node = shutil.which("node")
pytestmark = [pytest.mark.skipif(node is None, reason="node is not installed"), pytest.mark.gpu]

W, H, RPP = 48, 36, 4


@pytest.fixture(scope="module")
def cornell_xml(ref_data):
    return os.path.join(ref_data, "a10", "scenes", "cornell.xml")


def render(out, cornell_xml, *flags):
    r = subprocess.run([node, os.path.join(HOST, "cli.js"), "render", cornell_xml, str(W), str(H), str(RPP), "1", out, *flags],
                       capture_output=True, env=dict(os.environ, MIRT_GROUP_ALLOW_REPEATED_DEVICES="1"))
    assert r.returncode == 0, r.stderr.decode()
    return r.stderr.decode()


def same_file(a, b):
    x, y = open(a, "rb").read(), open(b, "rb").read()
    assert len(x) == len(y) and len(x) > 0
    assert x == y, f"{os.path.basename(a)}: {sum(p != q for p, q in zip(x, y))} bytes differ"


@pytest.fixture(scope="module")
def single_denoise(tmp_path_factory, pkg, cornell_xml):
    out = str(tmp_path_factory.mktemp("post_tiles_js") / "one.rgba")
    render(out, cornell_xml, "--denoise")
    return out


@pytest.mark.parametrize("n", [2, 3])
def test_denoise_in_tiles_writes_the_single_context_bytes(pkg, tmp_path, cornell_xml, single_denoise, n):
    out = str(tmp_path / "tiles.rgba")
    log = render(out, cornell_xml, "--gpus", str(n), "--denoise", "--post-in-tiles")
    assert "post-process in row tiles" in log
    same_file(out, single_denoise)
    same_file(out + ".filtered.f32", single_denoise + ".filtered.f32")
    assert not os.path.exists(out + ".radiance.f32"), "the unfiltered sums are not gathered"


@pytest.mark.parametrize("denoise", [[], ["--denoise"]])
def test_upscale_in_tiles_writes_the_single_context_bytes(pkg, tmp_path, cornell_xml, denoise):
    one, tiles = str(tmp_path / "one.rgba"), str(tmp_path / "tiles.rgba")
    render(one, cornell_xml, "--upscale", "2", *denoise)
    render(tiles, cornell_xml, "--upscale", "2", "--gpus", "2", "--post-in-tiles", *denoise)
    same_file(tiles, one)
    same_file(tiles + ".upsampled.f32", one + ".upsampled.f32")
