"""CPU: the yardstick of the radiance tests itself -- tests/radiance_common.expected_radiance, the definition of mirt_trace_radiance restated on
the CPU oracle -- and the entry points' presence in both libraries (which load without a GPU):

  (a) split equals joint: samples = 2 equals 1 + 1 with the accumulators and seeds carried over, per stratum;
  (b) initTrace's own rays of cornell_32x24_r4 and cornell_teapot3_32x24_r4 reproduce a10_pass.run_pass's acu and seeds at 5 bounces;
  (c) MIRT_RADIANCE_NO_EMITTERS differs from the default on at least one ray of a fixture, and never on a ray whose primary ray no light intercepts;
  (d) the rays exercise the call: at samples = 2, bounces = 3 every stratum has more than 30 % of its rays with w > 0, a NaN accumulator (the
      non-finite class), a ray whose seed is unchanged and one whose seed is changed;
  (e) mirt_trace_radiance and mirt_radiance_deferred are exported by libmirt.so and libmirt_default.so, and the call on an unknown context is
      MIRT_E_HANDLE.
"""
import ctypes as C
import os

import numpy as np
import pytest

import a10_pass as A
import radiance_common as RC
import rays_common as R
from conftest import ROOT, bits, load_fixture
from random_scenes_common import STRATA

FIXTURES = ("cornell_32x24_r4", "cornell_teapot3_32x24_r4")


@pytest.mark.parametrize("stratum", STRATA)
def test_two_samples_equal_one_and_one_accumulated(stratum):
    sc, rays, seeds = R.scene(stratum), R.rays_of(stratum)[0], RC.seeds_of(stratum)
    joint = RC.radiance_of(stratum, 2, 3)
    a1, s1 = RC.expected_radiance(sc, rays, seeds, 1, 3)
    split = RC.expected_radiance(sc, rays, s1, 1, 3, acu=a1)
    d = RC.differ(f"{stratum} 1 + 1 against 2", split, joint)
    assert d is None, d


@pytest.mark.parametrize("name", FIXTURES)
def test_the_cameras_own_rays_give_the_pass(name):
    _, sc = load_fixture(name)
    seeds = A.make_seeds(sc.total_rays)
    rays, st = RC.camera_rays(sc, seeds, bounces=5)
    got = RC.expected_radiance(sc, rays, seeds, 1, 5)
    d = RC.differ(name, got, (st.acu[:sc.total_rays], st.seeds[:sc.total_rays]))
    assert d is None, d


def test_no_emitters_differs_only_where_a_light_is_seen():
    differing = 0
    for name in FIXTURES:
        _, sc = load_fixture(name)
        seeds = A.make_seeds(sc.total_rays)
        rays, _ = RC.camera_rays(sc, seeds, bounces=0)
        seen = RC.light_intercepts(sc, rays)
        with_lights = RC.expected_radiance(sc, rays, seeds, 1, 2)
        without = RC.expected_radiance(sc, rays, seeds, 1, 2, emitters=False)
        differs = (bits(with_lights[0]) != bits(without[0])).any(axis=1) | (with_lights[1] != without[1])
        assert not (differs & ~seen).any(), f"{name}: NO_EMITTERS changed a ray no light intercepts"
        differing += int(differs.sum())
    assert differing > 0, "no ray of the fixtures sees a light: the flag is not exercised"


@pytest.mark.parametrize("stratum", STRATA)
def test_the_rays_exercise_the_call(stratum):
    acu, sd = RC.radiance_of(stratum, 2, 3)
    seeds = RC.seeds_of(stratum)
    with np.errstate(invalid="ignore"):
        lit = float((acu[:, 3] > 0).mean())
    nan = int(np.isnan(acu).any(axis=1).sum())
    print(f"{stratum}: w > 0 on {lit:.3f} of the rays, {nan} NaN accumulators, seed advanced on {float((sd != seeds).mean()):.3f}")
    assert lit > 0.30
    assert nan >= 1
    assert (sd == seeds).any() and (sd != seeds).any()
    # a dead ray adds nothing and draws nothing
    dead = ~R.live(R.rays_of(stratum)[0])
    assert dead.any() and (acu[dead].view(np.uint32) == 0).all() and (sd[dead] == seeds[dead]).all()


@pytest.mark.parametrize("libname", ["libmirt.so", "libmirt_default.so"])
def test_both_libraries_export_the_entry_points(pkg, libname):
    lib = C.CDLL(os.path.join(ROOT, "2015-raytracing_amd", libname))
    for name in ("mirt_trace_radiance", "mirt_radiance_deferred"):
        assert hasattr(lib, name), f"{libname} lacks {name}"


def test_an_unknown_context_is_a_handle_error(pkg):
    from raytracing_amd.pyhost import mirt
    not_a_handle = C.create_string_buffer(64)
    rd = mirt._RadianceDesc(C.sizeof(mirt._RadianceDesc), 1, 0, 0)
    desc = mirt._PassDesc()
    desc.struct_size = C.sizeof(mirt._PassDesc)
    rc = mirt.lib().mirt_trace_radiance(C.c_void_p(C.addressof(not_a_handle)), C.byref(desc), C.byref(rd), None, 0, None, None)
    assert rc == -2   # MIRT_E_HANDLE
    n = C.c_uint64(7)
    assert mirt.lib().mirt_radiance_deferred(C.c_void_p(C.addressof(not_a_handle)), C.byref(n)) == -2
