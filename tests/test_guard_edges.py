"""The host's geometry-side guard (csrc/pt_set_guard.hpp) at its edge, through whole renders: cornell.xml's sets with one bound AT the end of the
bounds' window [2^-30, 2^20] -- the optimistic kernel runs the set -- and one float BEYOND it, or an inverted axis -- the guard refuses the set and
only the exact kernel runs.  Either way the frame is the CPU oracle's, bit for bit, with the optimistic pair and with the exact kernel alone."""
import numpy as np
import pytest

import a10_pass as A
from conftest import bits, load_fixture
from test_gpu_parity import _variant
from test_set_guard import oracle as guard_oracle

pytestmark = pytest.mark.gpu

F = np.float32
TOP, BOTTOM = F(2.0) ** F(20), F(2.0) ** F(-30)


def _with(bounds, index, value):
    b = list(bounds)
    b[index] = float(value)
    return b


def _swapped(bounds, axis):
    b = list(bounds)
    b[axis], b[4 + axis] = b[4 + axis], b[axis]
    return b


VARIANTS = {   # name: (which bounds, how to change them, the guard accepts the set)
    "triangle_max_at_2p20": ("triangle_bounds", lambda b: _with(b, 4, TOP), True),
    "triangle_max_above_2p20": ("triangle_bounds", lambda b: _with(b, 4, np.nextafter(TOP, F(np.inf))), False),
    "sphere_min_at_2m30": ("sphere_bounds", lambda b: _with(b, 0, BOTTOM), True),
    "sphere_min_below_2m30": ("sphere_bounds", lambda b: _with(b, 0, np.nextafter(BOTTOM, F(0.0))), False),
    "sphere_axis_inverted": ("sphere_bounds", lambda b: _swapped(b, 0), False),
}


@pytest.fixture()
def ctx(pkg):
    from raytracing_amd.pyhost import mirt
    c = mirt.Context(0)
    yield c
    c.destroy()


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_bounds_at_the_guards_edge(ctx, pkg, name):
    from raytracing_amd.pyhost import render
    which, change, accepted = VARIANTS[name]
    _, base = load_fixture("cornell_32x24_r4")
    sc = _variant(base, **{which: change(base.d[which])})
    for key in ("sphere_bounds", "triangle_bounds"):   # the variant is on the side of the edge its name says, by the rules themselves
        want = guard_oracle(np.array(sc.d[key], dtype=F).reshape(1, 8), [sc.d["n_slabs"]], [True])["fast_ok"][0]
        assert want == (int(accepted) if key == which else 1), key
    seeds = A.make_seeds(sc.total_rays)
    st = A.PassState(sc, seeds)
    A.run_pass(A.load_oracle(), sc, st)
    for exact_only in (False, True):
        ctx.set_exact_only(exact_only)
        fr = render.FusedRenderer(ctx, sc, seeds=seeds)
        fr.execute_render()
        deferred = ctx.pass_deferred()
        assert np.array_equal(bits(fr.acu.read(np.float32).reshape(-1, 4)), bits(st.acu)), f"acu, exact_only={exact_only}"
        assert np.array_equal(fr.seeds.read(np.int32), st.seeds), f"seeds, exact_only={exact_only}"
        assert np.array_equal(fr.pixel.read(np.uint8).reshape(-1, 4), st.pixel), f"pixel, exact_only={exact_only}"
        fr.release()
        if not exact_only and not accepted:
            assert deferred == 0       # a refused set: the optimistic kernel did not run, nothing was deferred to the exact one
    ctx.set_exact_only(False)
    assert (st.acu[:, 3] > 0).any()
