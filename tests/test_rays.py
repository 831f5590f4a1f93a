"""GPU: ray queries on caller-supplied rays -- mirt_trace_closest, mirt_trace_occluded, mirt_trace_deferred (include/mirt.h) -- through the C ABI,
tolerance 0 (conftest.bits: every NaN equal to every NaN):

  1. against the CPU oracle (tests/rays_common.py): hits, sets and occluded per stratum of the random scenes, with the optimistic / exact pair
     and under set_exact_only(True); and on one grid scene and one single-cell scene at N = 1, 63, 64, 65, 255, 257 -- a lone lane in a walk all
     64 enter, a second wave of one lane, a second block;
  2. deferred rays: under the pair mirt_trace_deferred is at least the number of live rays the ray-side guard's rule refuses, and below N;
  3. order: the batch reversed, and the batch with a dead ray inserted after every ray, give the same record per ray (the shared-test walk pools
     a wave's tests: a ray's result must not depend on its wave-mates);
  4. only one output: hits alone and sets alone each equal the both-buffers call;
  5. sentinels: the bytes behind the `count` records of every output stay untouched (checked in every case above as well);
  6. refusals: every one include/mirt.h lists, with the outputs pre-filled and compared afterwards, and the context still renders
     cornell_32x24_r4 correctly after them.
"""
import ctypes as C

import numpy as np
import pytest

import a10_pass as A
import rays_common as R
from conftest import load_fixture
from random_scenes_common import STRATA

pytestmark = pytest.mark.gpu

E_ARG, E_HANDLE, E_RANGE, E_DATA = -1, -2, -5, -8
SMALL_N = (1, 63, 64, 65, 255, 257)


@pytest.fixture(scope="module")
def ctx(pkg):
    from raytracing_amd.pyhost import mirt
    c = mirt.Context(0)
    yield c
    c.destroy()


@pytest.fixture(scope="module")
def tracers(ctx):
    made = {}

    def get(stratum):
        if stratum not in made:
            made[stratum] = R.Tracer(ctx, R.scene(stratum), cap=2 * R.N_RAYS)
        return made[stratum]
    yield get
    for t in made.values():
        t.release()


def check_closest(tag, t, rays, want_hits, want_sets):
    hits, sets, tails = t.closest(rays)
    d = R.hits_differ(f"{tag} hits", hits, want_hits)
    assert d is None, d
    bad = np.flatnonzero(sets != want_sets)
    assert bad.size == 0, f"{tag} sets: {bad.size} differ, first ray {bad[0]}: got {sets[bad[0]]}, want {want_sets[bad[0]]}"
    assert R.untouched(tails[0]) and R.untouched(tails[1]), f"{tag}: bytes behind the records were written"


def check_occluded(tag, t, rays, want):
    occ, tail = t.occluded(rays)
    bad = np.flatnonzero(occ != want)
    assert bad.size == 0, f"{tag} occluded: {bad.size} differ, first ray {bad[0]}: got {occ[bad[0]]}, want {want[bad[0]]}"
    assert R.untouched(tail), f"{tag}: bytes behind the {len(want)} results were written"


# ---- 1. the oracle ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact_only", [False, True], ids=["pair", "exact_only"])
@pytest.mark.parametrize("stratum", STRATA)
def test_closest_and_occluded_equal_the_oracle(ctx, tracers, stratum, exact_only):
    rays, _ = R.rays_of(stratum)
    want_hits, want_sets = R.closest_of(stratum)
    t = tracers(stratum)
    ctx.set_exact_only(exact_only)
    try:
        check_closest(f"{stratum} exact_only={exact_only}", t, rays, want_hits, want_sets)
        check_occluded(f"{stratum} exact_only={exact_only}", t, rays, R.occluded_of(stratum))
    finally:
        ctx.set_exact_only(False)


@pytest.mark.parametrize("exact_only", [False, True], ids=["pair", "exact_only"])
@pytest.mark.parametrize("n", SMALL_N)
@pytest.mark.parametrize("stratum", ["staged", "single_cell"])
def test_small_batches_equal_the_oracle(ctx, tracers, stratum, n, exact_only):
    """rays are independent, so the first n rays of the batch have the first n answers of the oracle's"""
    rays, _ = R.rays_of(stratum)
    want_hits, want_sets = R.closest_of(stratum)
    t = tracers(stratum)
    ctx.set_exact_only(exact_only)
    try:
        check_closest(f"{stratum} n={n}", t, rays[:n], want_hits[:n], want_sets[:n])
        check_occluded(f"{stratum} n={n}", t, rays[:n], R.occluded_of(stratum)[:n])
    finally:
        ctx.set_exact_only(False)


def test_no_rays_is_ok_and_writes_nothing(ctx, tracers):
    t = tracers("staged")
    hits, sets, tails = t.closest(np.zeros((0, 8), np.float32))
    assert len(hits) == 0 and len(sets) == 0 and R.untouched(tails[0]) and R.untouched(tails[1])
    occ, tail = t.occluded(np.zeros((0, 8), np.float32))
    assert len(occ) == 0 and R.untouched(tail)
    assert ctx.trace_deferred() == 0


# ---- 2. deferred rays --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stratum", STRATA)
def test_the_exact_kernel_redoes_at_least_the_rays_the_guard_refuses(ctx, tracers, stratum):
    rays, _ = R.rays_of(stratum)
    refused = int((R.live(rays) & ~R.guard_accepts(rays)).sum())
    assert refused > 0
    t = tracers(stratum)
    t.closest(rays)
    closest = ctx.trace_deferred()
    t.occluded(rays)
    occluded = ctx.trace_deferred()
    print(f"{stratum}: guard refuses {refused} live rays of {len(rays)}; deferred: closest {closest}, occluded {occluded}")
    assert refused <= closest < len(rays)
    assert refused <= occluded < len(rays)
    ctx.set_exact_only(True)
    try:
        t.closest(rays)
        assert ctx.trace_deferred() == 0, "the exact kernel alone defers nothing"
    finally:
        ctx.set_exact_only(False)


# ---- 3. order ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stratum", ["staged", "unstaged", "many_sets", "single_cell"])
def test_a_rays_record_does_not_depend_on_its_wave_mates(ctx, tracers, stratum):
    rays, _ = R.rays_of(stratum)
    want_hits, want_sets = R.closest_of(stratum)
    want_occ = R.occluded_of(stratum)
    t = tracers(stratum)
    check_closest(f"{stratum} reversed", t, rays[::-1], want_hits[::-1], want_sets[::-1])
    check_occluded(f"{stratum} reversed", t, rays[::-1], want_occ[::-1])
    # a dead ray behind every ray: every wave is half dead lanes, and every ray has other wave-mates than before
    dead = np.array([0.1, -0.2, 0.3, 2.5, 0.0, 0.0, -1.0, 2.5], np.float32)
    both = np.empty((2 * len(rays), 8), np.float32)
    both[0::2], both[1::2] = rays, dead
    hits, sets, tails = t.closest(both)
    d = R.hits_differ(f"{stratum} interleaved", hits[0::2], want_hits)
    assert d is None, d
    assert np.array_equal(sets[0::2], want_sets)
    miss = np.array([0, 0, 0, 2.5, 0, 0, 0], np.float32)
    assert (hits[1::2, :7].view(np.uint32) == miss.view(np.uint32)).all() and (hits[1::2, 7].view(np.int32) == -1).all() and (sets[1::2] == R.NO_SET).all()
    assert R.untouched(tails[0]) and R.untouched(tails[1])
    occ, tail = t.occluded(both)
    assert np.array_equal(occ[0::2], want_occ) and (occ[1::2] == 1).all() and R.untouched(tail)


# ---- 4. only one output --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stratum", ["staged", "single_cell"])
def test_hits_alone_and_sets_alone_equal_the_call_with_both(ctx, tracers, stratum):
    rays, _ = R.rays_of(stratum)
    want_hits, want_sets = R.closest_of(stratum)
    t = tracers(stratum)
    hits, none, tails = t.closest(rays, sets=False)
    assert none is None and R.hits_differ("hits alone", hits, want_hits) is None
    assert R.untouched(tails[0]) and R.untouched(tails[1]), "the sets buffer, not given, was written"
    none, sets, tails = t.closest(rays, hits=False)
    assert none is None and np.array_equal(sets, want_sets)
    assert R.untouched(tails[0]) and R.untouched(tails[1]), "the hits buffer, not given, was written"


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_leave_the_context_working(ctx, pkg):
    from raytracing_amd.pyhost import mirt, render
    L = mirt.lib()
    sc = R.scene("single_cell")
    rays = R.rays_of("single_cell")[0][:300]
    n = len(rays)
    t = R.Tracer(ctx, sc, cap=n, tail=0)
    t.rays.write(rays)
    short32, short4, short1, short_rays = ctx.buffer(n * 32 - 1), ctx.buffer(n * 4 - 1), ctx.buffer(n - 1), ctx.buffer(n * 32 - 1)
    outputs = (t.hits, t.sets, t.occ, short32, short4, short1)
    wrapped = []

    def h(b):
        return b.h if isinstance(b, mirt.Buffer) else b

    def closest(c=None, desc=t.desc, rays=t.rays, count=n, hits=t.hits, sets=t.sets):
        return L.mirt_trace_closest(c or ctx.h, C.byref(desc) if desc is not None else None, h(rays), count, h(hits), h(sets))

    def occluded(c=None, desc=t.desc, rays=t.rays, count=n, occ=t.occ):
        return L.mirt_trace_occluded(c or ctx.h, C.byref(desc) if desc is not None else None, h(rays), count, h(occ))

    def refused(code, call, **over):
        for b in outputs:
            b.write(np.full(b.nbytes, R.Tracer.SENTINEL, np.uint8))
        assert call(**over) == code, (call.__name__, list(over), ctx.last_error())
        for b in outputs:
            assert R.untouched(b.read(np.uint8)), f"{call.__name__} {list(over)}: an output was written"
        assert t.rays.read(np.float32).tobytes() == rays.tobytes(), "the rays were written"

    def wrong_size():
        d = t.dev.pass_desc(None, None)
        d.struct_size -= 4
        return d

    try:
        for call in (closest, occluded):
            refused(E_ARG, call, desc=None)
            refused(E_ARG, call, desc=wrong_size())
            refused(E_ARG, call, count=2 ** 32 - 255)
            refused(E_RANGE, call, count=n + 1)                 # every buffer holds exactly n records
            refused(E_RANGE, call, rays=short_rays)
            not_a_handle = C.create_string_buffer(64)
            refused(E_HANDLE, call, c=C.c_void_p(C.addressof(not_a_handle)))
            refused(E_HANDLE, call, rays=C.c_void_p(C.addressof(not_a_handle)))
            refused(E_HANDLE, call, rays=None)
        refused(E_ARG, closest, hits=None, sets=None)
        refused(E_ARG, occluded, occ=None)
        refused(E_RANGE, closest, hits=short32)
        refused(E_RANGE, closest, sets=short4)
        refused(E_RANGE, occluded, occ=short1)
        refused(E_HANDLE, closest, hits=C.c_void_p(C.addressof(not_a_handle)))
        refused(E_HANDLE, occluded, occ=C.c_void_p(C.addressof(not_a_handle)))
        # aliasing: an output that is the rays, shares some of their bytes, or meets the other output
        refused(E_ARG, closest, hits=t.rays)
        refused(E_ARG, occluded, occ=t.rays)
        view = ctx.wrap(t.rays.device_ptr + 16, n * 4)
        wrapped.append(view)
        refused(E_ARG, closest, sets=view)
        refused(E_ARG, closest, sets=t.hits)
        view = ctx.wrap(t.hits.device_ptr + n * 32 - n * 4, n * 4)     # the last n words of hits
        wrapped.append(view)
        refused(E_ARG, closest, sets=view)
        # a cell table that fails validation: the loose triangles' offsets decrease
        off = t.dev.tri["off"]
        good = off.read(np.uint32)
        off.write(np.array([good[-1], 0], np.uint32))
        try:
            refused(E_DATA, closest)
            refused(E_DATA, occluded)
        finally:
            off.write(good)
        # while capturing
        for b in outputs:
            b.write(np.full(b.nbytes, R.Tracer.SENTINEL, np.uint8))
        ctx.finish()
        ctx.capture_begin()
        try:
            assert closest() == E_ARG and "capture" in ctx.last_error()
            assert occluded() == E_ARG and "capture" in ctx.last_error()
        finally:
            ctx.graph_release(ctx.capture_end())
        for b in outputs:
            assert R.untouched(b.read(np.uint8)), "written inside a recording"
        # the same context answers the same rays afterwards ...
        want_hits, want_sets = R.closest_of("single_cell")
        hits, sets, _ = t.closest(rays)
        assert R.hits_differ("after the refusals", hits, want_hits[:n]) is None and np.array_equal(sets, want_sets[:n])
        assert np.array_equal(t.occluded(rays)[0], R.occluded_of("single_cell")[:n])
        # ... and renders
        fx, fsc = load_fixture("cornell_32x24_r4")
        seeds = A.make_seeds(fsc.total_rays)
        st = A.PassState(fsc, seeds)
        A.run_pass(A.load_oracle(), fsc, st)
        fr = render.FusedRenderer(ctx, fsc, seeds=seeds)
        try:
            fr.execute_render()
            assert np.array_equal(fr.pixel.read(np.uint8).reshape(-1, 4), st.pixel), "cornell_32x24_r4 after the refusals"
        finally:
            fr.release()
    finally:
        for b in wrapped + [short32, short4, short1, short_rays]:
            b.release()
        t.release()
