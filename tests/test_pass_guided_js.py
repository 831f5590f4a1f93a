"""The JavaScript host on mirt_render_first_pass_guided (queue.renderFirstPassGuided through the N-API addon): where one pass and its guides are
asked for -- `--guides`, `--denoise`, `--upscale` on one context -- the pass writes the guides itself, and every file the command writes is,
byte for byte, the file it writes on the two calls.  The comparison is made in the same test by the same command with MIRT_GUIDED_PASS=0, which
makes the library queue the pass and then the guide launches; the command reports the route (ctx.guidedPasses()) in its last line."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import HOST

node = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(node is None, reason="node is not installed")]


def render(scenes, tmp, tag, flags, env):
    d = tmp / tag
    d.mkdir()
    flags = [str(d / f[1:]) if f.startswith("@") else f for f in flags]
    r = subprocess.run([node, os.path.join(HOST, "cli.js"), "render", os.path.join(scenes, "cornell.xml"), "48", "36", "4", "1", str(d / "out.ppm"), *flags],
                       capture_output=True, text=True, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr
    m = re.search(r"first passes that wrote their guides: (\d+)", r.stderr)
    assert m, r.stderr
    return {f: open(d / f, "rb").read() for f in sorted(os.listdir(d))}, int(m.group(1))


@pytest.mark.parametrize("flags,files", [(["--denoise", "--guides", "@out"], 5), (["--guides", "@g"], 4), (["--denoise", "2"], 3),
                                         (["--upscale", "2", "--denoise", "--guides", "@g"], 8)],
                         ids=["denoise_guides", "guides", "denoise", "upscale"])
def test_files_equal_the_two_call_path(pkg, ref_data, tmp_path, flags, files):
    scenes = os.path.join(ref_data, "a10", "scenes")
    got, routed = render(scenes, tmp_path, "guided", flags, {})
    want, forced = render(scenes, tmp_path, "two_calls", flags, {"MIRT_GUIDED_PASS": "0"})
    assert routed == 1 and forced == 0, "the route the command reports"
    assert len(got) == files and sorted(got) == sorted(want), sorted(got)
    for name in got:
        assert got[name] == want[name], f"{name} differs"


def test_several_passes_stay_on_the_two_calls(pkg, ref_data, tmp_path):
    d = tmp_path / "three"
    d.mkdir()
    r = subprocess.run([node, os.path.join(HOST, "cli.js"), "render", os.path.join(ref_data, "a10", "scenes", "cornell.xml"), "48", "36", "4", "3", str(d / "out.ppm"),
                        "--guides", str(d / "g")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "first passes that wrote their guides: 0" in r.stderr
