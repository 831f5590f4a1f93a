"""The ray-side guard of the optimistic kernel at its edges, through whole renders of generated cameras and lights (tests/ray_edges_common.py: one
job per edge, each with a predicate over the CPU oracle's own rays that says on which side of the edge it sits).

CPU (no mark): the rule's own verdicts at the edges; every job's predicate and measured counts on the oracle's rays; something is lit, or where
all is dark by design something is accumulated; pt_set_guard.hpp's verdict on every set as the job's table says; and, where the compiled
reference is built, oracle == reference bit for bit on every job -- these inputs (NaN through min / max, 0 / 0, division by zero) are where a
restatement goes wrong.

GPU: every path on every job against the oracle on the same seeds, bit for bit (for the two light_nonfinite jobs a NaN equals a NaN): the
fused pass with the accumulator, the fused pass that resolves its own pixels, the kernel-by-kernel path, the guide buffers, and the one-launch
first pass with guides -- each with the optimistic pair and with the exact kernel alone.  Where single samples are deferred (a context that
leaves the pixels to copyToPixel; nine rays per pixel) their number is bounded from below by the samples the rule puts outside the window, is 0
where a set is refused, and stays below the number of alive primary rays where a value sits exactly ON a bound.  A pass that resolves its
pixels -- with or without the accumulator -- defers whole blocks of 256 ray ids: there the count is bounded from below by 256 times the number
of blocks that hold such a sample."""
import os

import numpy as np
import pytest

import a10_pass as A
import ray_edges_common as R
from conftest import ROOT, assert_state_equals_pass_state
from guides_common import difference, expected_guides
from test_set_guard import ask   # noqa: F401  (the module-scoped fixture that compiles tests/set_guard_dump.cpp)
from test_set_guard import oracle as guard_oracle

F = np.float32
ORDINARY = F(0.5)
REF_A10 = os.path.join(ROOT, "oracle", "_ref", "libref_a10.so")
gpu = pytest.mark.gpu

RPP = {name: R.JOBS[name].size.get("rays_per_pixel", 4) for name in R.NAMES}
WHOLE_PIXEL_BLOCKS = [n for n in R.NAMES if 256 % RPP[n] == 0]        # the pass resolves its own pixels where the ray count divides 256
GUIDES = [n for n in R.NAMES if RPP[n] != 1]                             # the guide kernel has no seeds[col] pre-pass: it refuses one ray per pixel
GUIDED = [n for n in R.NAMES if RPP[n] == 4]                             # the one-launch route of the jobs at 4 rays per pixel
MODES = pytest.mark.parametrize("exact_only", [False, True], ids=["optimistic", "exact_only"])


def f32(u):
    return np.asarray(u, dtype=np.uint32).view(F)


@pytest.fixture(scope="module")
def win(ask):   # noqa: F811
    return R.window_constants(ask)


@pytest.fixture(scope="module")
def ctx(pkg):
    from raytracing_amd.pyhost import mirt
    c = mirt.Context(0)
    yield c
    c.set_exact_only(False)
    c.destroy()


@pytest.fixture(scope="module")
def ctx_sep(pkg):
    """a context that never resolves in the pass (MIRT_INPASS_RESOLVE=0 is read when a context is created, tests/test_inpass_resolve.py)"""
    from raytracing_amd.pyhost import mirt
    os.environ["MIRT_INPASS_RESOLVE"] = "0"
    try:
        c = mirt.Context(0)
    finally:
        del os.environ["MIRT_INPASS_RESOLVE"]
    yield c
    c.set_exact_only(False)
    c.destroy()


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------------------
def test_the_rule_at_its_edges_as_stated(win):
    """the numpy rule's own verdicts spelled out, so that it cannot be wrong in the same way as the device code"""
    den_lo, den_hi, pos_lo, pos_hi = win
    assert [float(np.log2(x)) for x in win] == [-40.0, 40.0, -30.0, 20.0]
    up, down = lambda v: np.nextafter(F(v), F(np.inf)), lambda v: np.nextafter(F(v), F(0.0))

    def one(slot, v):
        r = np.full((1, 6), ORDINARY, dtype=F)
        r[0, slot] = v
        return bool(R.accepted(r[:, :3], r[:, 3:], win)[0])
    for s in range(3):      # an origin component: zero of either sign, or a magnitude in [2^-30, 2^20]
        assert one(s, F(0.0)) and one(s, F(-0.0)) and one(s, pos_lo) and one(s, -pos_lo) and one(s, pos_hi) and one(s, -pos_hi)
        assert not one(s, down(pos_lo)) and not one(s, -down(pos_lo)) and not one(s, up(pos_hi)) and not one(s, f32(1)) and not one(s, f32(0x007FFFFF))
        assert not one(s, F(np.inf)) and not one(s, F(-np.inf)) and not one(s, F(np.nan))
    for s in range(3, 6):   # a direction component: a magnitude in [2^-40, 2^40]; zero is refused
        assert one(s, den_lo) and one(s, -den_lo) and one(s, den_hi) and one(s, -den_hi)
        assert not one(s, down(den_lo)) and not one(s, up(den_hi)) and not one(s, -up(den_hi)) and not one(s, F(0.0)) and not one(s, F(-0.0))
        assert not one(s, F(np.inf)) and not one(s, F(np.nan)) and not one(s, f32(1))



@pytest.mark.parametrize("name", R.NAMES)
def test_job_sits_on_its_side_of_the_edge(win, name):
    """the job's predicate over the oracle's own rays, the rule's verdict on its alive primary rays, and the counts measured when it was written"""
    s = R.state(name, win)
    job, alive = s.job, int(s.alive.sum())
    print(f"{name}: {len(s.alive)} rays, {alive} alive, {s.n_out} of them outside the window, {s.lit} of {len(s.st.pixel)} pixels lit")
    if job.outside == "none":
        assert alive > 0 and s.n_out == 0
    elif job.outside == "all":
        assert alive > 0 and s.n_out == alive
    elif job.outside == "some":
        assert 0 < s.n_out < alive
    for key, got in (("alive", alive), ("outside", s.n_out), ("lit", s.lit)):
        if key in job.measured:
            assert got == job.measured[key], f"{key}: the oracle gives {got}, the job's table says {job.measured[key]}"
    if job.holds:
        job.holds(s)
    assert s.sc.width * s.sc.height * s.sc.rpp <= 33 * 25 * 9 and s.sc.width <= 48 and s.sc.height <= 36


@pytest.mark.parametrize("name", R.NAMES)
def test_job_shows_something(win, name):
    """a lit pixel; where everything is dark by design, an accumulator that counted a sample.  Two jobs show nothing at all, and that is what
    they are for: focal_zero_pinhole (every direction norm3(0)) and focal_zero from the fixture's eye (every ray runs in the lens plane, outside
    the scene box) -- focal_zero_eye_inside is the latter with rays that arrive."""
    s = R.state(name, win)
    if name in ("focal_zero_pinhole", "focal_zero"):
        assert not s.alive.any() and not s.st.acu.any() and s.lit == 0
    elif s.job.dark:
        assert s.lit == 0 and (s.st.acu[:, 3] > 0).any()
    else:
        assert s.lit > 0


@pytest.mark.parametrize("name", R.NAMES)
def test_set_guard_decides_as_the_jobs_table_says(win, name):
    s = R.state(name, win)
    sets = R.sets_of(s.sc)
    assert set(s.job.refused) <= {x[0] for x in sets}
    for key, b8, n, tri, pos in sets:
        sane = R.records_sane(pos, win) if tri else True
        got = int(guard_oracle(np.array(b8, dtype=F).reshape(1, 8), [n], [sane])["fast_ok"][0])
        assert got == (0 if key in s.job.refused else 1), key


def _same(tag, got, want, nan_rule):
    assert R.equal_words(got, want, nan_rule), f"{tag} differs"


@pytest.mark.skipif(not os.path.exists(REF_A10), reason="oracle/_ref/libref_a10.so not built (the reference's own kernels for the host)")
@pytest.mark.parametrize("name", R.NAMES)
def test_oracle_equals_the_compiled_reference(win, name):
    """the accumulator, the seeds, and every primary and shadow ray after the primary segment.  (A shadow ray of a path that ended has only its
    mint / maxt defined.)"""
    s = R.state(name, win)
    st, cp = A.PassState(s.sc, s.seeds), {}
    A.run_pass(A.load_ref(), s.sc, st, checkpoints=cp)
    nan = s.job.nan_rule
    _same("acu", st.acu, s.st.acu, nan)
    assert np.array_equal(st.seeds, s.st.seeds), "seeds"
    assert np.array_equal(st.pixel, s.st.pixel), "pixel"
    made = s.primary["pois"]["matId"] >= 0
    assert np.array_equal(cp["primary"]["pois"]["matId"], s.primary["pois"]["matId"])
    for k in ("rays", "shadow"):
        got, want = cp["primary"][k], s.primary[k]
        for f in ("mint", "maxt"):
            _same(f"primary {k}.{f}", got[f], want[f], nan)
        rows = slice(None) if k == "rays" else made
        for f in ("o", "d"):
            _same(f"primary {k}.{f}", got[f][rows], want[f][rows], nan)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------------
def _fused(ctx, s, exact_only, keep_acu):
    from raytracing_amd.pyhost import render
    ctx.set_exact_only(exact_only)
    try:
        fr = render.FusedRenderer(ctx, s.sc, seeds=s.seeds, keep_acu=keep_acu)
        try:
            fr.execute_render(fresh=not keep_acu)
            out = dict(deferred=ctx.pass_deferred(), seeds=fr.seeds.read(np.int32), pixel=fr.pixel.read(np.uint8).reshape(-1, 4))
            if keep_acu:
                out["acu"] = fr.acu.read(np.float32).reshape(-1, 4)
            return out
        finally:
            fr.release()
    finally:
        ctx.set_exact_only(False)


def _check_deferred(s, ctx_resolves, exact_only, deferred, tag):
    """the number of deferred samples against the rule.  A context that resolves in the pass defers whole blocks of 256 consecutive ray ids where
    the ray count divides 256 (csrc/pt_pass_plan.hpp mask_unit; tests/test_inpass_resolve.py): every block that holds a sample whose alive
    primary ray the rule puts outside the window is among them.  Otherwise single samples are deferred: at least those."""
    alive, total = int(s.alive.sum()), s.sc.total_rays
    unit = 256 if ctx_resolves and 256 % s.sc.rpp == 0 else 1
    need = unit * np.unique(np.flatnonzero(s.outside) // unit).size
    print(f"{tag}: {deferred} samples deferred in units of {unit}; the rule puts {s.n_out} of {alive} alive primary rays outside the window, which needs {need}")
    if exact_only or s.job.refused:
        assert deferred == 0                # the optimistic kernel did not run: nothing was deferred to the exact one
        return
    assert deferred % unit == 0 and need <= deferred <= -(-total // unit) * unit
    if s.job.at_edge and unit == 1:         # from the rule, not measured: a guard that refuses the edge value itself defers every alive primary ray
        assert alive > 0 and deferred < alive


@gpu
@MODES
@pytest.mark.parametrize("name", R.NAMES)
def test_fused_pass_with_the_accumulator(ctx, pkg, win, name, exact_only):
    s = R.state(name, win)
    got = _fused(ctx, s, exact_only, keep_acu=True)
    _same("acu", got["acu"], s.st.acu, s.job.nan_rule)
    assert np.array_equal(got["seeds"], s.st.seeds), "seeds"
    assert np.array_equal(got["pixel"], s.st.pixel), "pixel"
    _check_deferred(s, True, exact_only, got["deferred"], f"{name}, exact_only={exact_only}")


@gpu
@MODES
@pytest.mark.parametrize("name", R.NAMES)
def test_fused_pass_deferring_sample_by_sample(ctx_sep, pkg, win, name, exact_only):
    """the same pass in a context that leaves the pixels to the separate copyToPixel: the optimistic kernel defers single samples, and the
    count is bounded by the rule from both sides"""
    s = R.state(name, win)
    got = _fused(ctx_sep, s, exact_only, keep_acu=True)
    _same("acu", got["acu"], s.st.acu, s.job.nan_rule)
    assert np.array_equal(got["seeds"], s.st.seeds), "seeds"
    assert np.array_equal(got["pixel"], s.st.pixel), "pixel"
    _check_deferred(s, False, exact_only, got["deferred"], f"{name}, sample by sample, exact_only={exact_only}")


@gpu
@MODES
@pytest.mark.parametrize("name", WHOLE_PIXEL_BLOCKS)
def test_fused_pass_resolving_its_own_pixels(ctx, pkg, win, name, exact_only):
    s = R.state(name, win)
    got = _fused(ctx, s, exact_only, keep_acu=False)
    assert np.array_equal(got["seeds"], s.st.seeds), "seeds"
    assert np.array_equal(got["pixel"], s.st.pixel), "pixel"
    _check_deferred(s, True, exact_only, got["deferred"], f"{name}, no accumulator, exact_only={exact_only}")


@gpu
@pytest.mark.parametrize("name", R.NAMES)
def test_kernel_by_kernel(ctx, pkg, win, name):
    from raytracing_amd.pyhost import render
    from test_gpu_parity import snapshot
    s = R.state(name, win)
    gr = render.GranularRenderer(ctx, s.sc, seeds=s.seeds)
    try:
        gr.execute_render()
        got = snapshot(gr)
        _same("acu", got["acu"], s.st.acu, s.job.nan_rule)
        assert_state_equals_pass_state(name, got, s.st)      # every Ray, shadow Ray and vertex
        assert np.array_equal(gr.read("pixel").reshape(-1, 4), s.st.pixel), "pixel"
    finally:
        gr.release()


@pytest.fixture(scope="module")
def guides_of():
    """the CPU reduction of tests/guides_common.py over the oracle's first-hit state, once per job"""
    cache, k = {}, A.load_oracle()

    def get(s):
        if s.job.name not in cache:
            cache[s.job.name] = expected_guides(k, s.sc)
        return cache[s.job.name]
    return get


@gpu
@MODES
@pytest.mark.parametrize("name", GUIDES)
def test_guides(ctx, pkg, win, guides_of, name, exact_only):
    from raytracing_amd.pyhost import render
    s = R.state(name, win)
    want = guides_of(s)
    ctx.set_exact_only(exact_only)
    try:
        fr = render.FusedRenderer(ctx, s.sc, seeds=s.seeds)
        try:
            got = fr.guides()
        finally:
            fr.release()
    finally:
        ctx.set_exact_only(False)
    for tag, g, w in (("normal_hits", got[0], want[0]), ("albedo_depth", got[1], want[1])):
        d = difference(f"{name} {tag}", g, w)
        assert d is None, d


@gpu
@MODES
@pytest.mark.parametrize("keep_acu", [False, True], ids=["acu_null", "acu_given"])
@pytest.mark.parametrize("name", GUIDED)
def test_first_pass_with_guides_in_one_launch(ctx, pkg, win, guides_of, name, keep_acu, exact_only):
    """mirt_render_first_pass_guided against the pass followed by the guides call (tests/pass_guided_common.py), and its guides against the CPU"""
    from pass_guided_common import compare
    s = R.state(name, win)
    ctx.set_exact_only(exact_only)
    try:
        diff, routed, deferred, got = compare(ctx, s.sc, f"{name} exact_only={exact_only}", keep_acu=keep_acu, seed_base=0)
    finally:
        ctx.set_exact_only(False)
    assert diff is None, diff
    assert routed == 1, "the call did not take the one-launch route"
    want = guides_of(s)
    for tag, g, w in (("normal_hits", got[0], want[0]), ("albedo_depth", got[1], want[1])):
        d = difference(f"{name} {tag} against the CPU reduction", g, w)
        assert d is None, d
    if exact_only or s.job.refused:
        assert deferred == 0
