"""The JavaScript host on mirt_render_passes_guided (queue.renderPassesGuided through the N-API addon): where passes in one launch and the frame's
guides are asked for -- `--passes-in-one-launch` with `--guides`, `--denoise` or `--upscale` on one context, with or without `--every-pass` -- the
multi-pass call writes the guides itself, and every file the command writes is, byte for byte, the file it writes on the two calls.  The
comparison is made in the same test by the same command with MIRT_GUIDED_PASS=0, which makes the library queue the passes and then the guide
launches; the command reports the route (ctx.guidedPasses()) in its last line."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import HOST

node = shutil.which("node")


def test_the_queue_and_the_renderer_have_the_call():
    webcl = open(os.path.join(HOST, "webcl.js")).read()
    renderer = open(os.path.join(HOST, "renderer.js")).read()
    addon = open(os.path.join(HOST, "..", "csrc", "addon", "mirt_napi.cc")).read()
    assert "renderPassesGuided(desc, n, normalHits, albedoDepth)" in webcl and "hasPassesGuided()" in webcl
    assert "executePassesGuided(n, bounces, opt)" in renderer
    assert '{"renderPassesGuided", RenderPassesGuided}' in addon and "mirt_render_passes_guided(" in addon


def render(scenes, tmp, tag, flags, env):
    d = tmp / tag
    d.mkdir()
    flags = [str(d / f[1:]) if f.startswith("@") else f for f in flags]
    r = subprocess.run([node, os.path.join(HOST, "cli.js"), "render", os.path.join(scenes, "cornell.xml"), "28", "20", "4", "3", str(d / "out.ppm"),
                        "--passes-in-one-launch", *flags], capture_output=True, text=True, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr
    m = re.search(r"first passes that wrote their guides: (\d+)", r.stderr)
    assert m, r.stderr
    return {f: open(d / f, "rb").read() for f in sorted(os.listdir(d))}, int(m.group(1))


@pytest.mark.gpu
@pytest.mark.skipif(node is None, reason="node is not installed")
@pytest.mark.parametrize("flags", [["--no-acu", "--guides", "@P", "--denoise"], ["--guides", "@P", "--every-pass"], ["--upscale", "2", "--denoise"]],
                         ids=["no_acu_guides_denoise", "every_pass_guides", "upscale"])
def test_files_equal_the_two_call_path(pkg, ref_data, tmp_path, flags):
    scenes = os.path.join(ref_data, "a10", "scenes")
    got, routed = render(scenes, tmp_path, "guided", flags, {})
    want, forced = render(scenes, tmp_path, "two_calls", flags, {"MIRT_GUIDED_PASS": "0"})
    assert routed == 1 and forced == 0, "the route the command reports"
    assert len(got) >= 3 and sorted(got) == sorted(want), sorted(got)
    for name in got:
        assert got[name] == want[name], f"{name} differs"
