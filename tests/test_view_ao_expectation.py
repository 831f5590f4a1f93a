"""CPU: the cases of tests/test_view_ao.py are not vacuous -- checked on the ORACLE's result alone (view_ao_common.expected: view_rays, the
closest-hit stages, bouncePaths x 3 on a scratch buffer, the rewritten rays, the shadow kernels), so the conditions hold on a machine without a
GPU too.  Every case: cast > 0, 0.1 <= open / cast <= 0.9 over the frame, cast <= rpp * samples per pixel, and a pixel that casts nothing where
the cameras leave some without a hit.  3 AO rays, bias 0.001 throughout; `open` x fisheye (0.09998) is left out."""
import numpy as np
import pytest

import view_ao_common as VA
import view_cameras_common as VC
import view_common as V


def check(tag, want, rpp, need_empty=False, share=None):
    d = VA.not_vacuous(tag, want, VA.SAMPLES, rpp, need_empty)
    assert d is None, d
    assert (want[:, 0] <= want[:, 1]).all() and (want[:, 1] % VA.SAMPLES == 0).all()
    if share is not None:
        assert share[0] <= want[:, 0].sum() / want[:, 1].sum() <= share[1], (tag, share)


@pytest.mark.parametrize("model", VA.MODELS)
@pytest.mark.parametrize("name", VA.FIXTURES)
def test_fixture_cases(name, model):
    want = VA.expected_standard(name, model)
    check(f"{name} {model} 13x7 k=2 radius 1.0", want, 4, need_empty=VA.FIXTURE_EMPTY[(name, model)] > 0)
    assert int((want[:, 1] == 0).sum()) == VA.FIXTURE_EMPTY[(name, model)]
    assert len(want) == 91


@pytest.mark.parametrize("name,model,radius,bias", VA.FIXTURE_VARIANTS)
def test_fixture_variants(name, model, radius, bias):
    check(f"{name} {model} radius {radius} bias {bias}", VA.expected_standard(name, model, radius, bias), 4)


@pytest.mark.parametrize("stratum,model", VA.STRATA_CASES)
def test_strata_cases(stratum, model):
    want = VA.expected_standard(stratum, model, VA.RADIUS[stratum], VA.BIAS, 37, 21, 2)
    check(f"{stratum} {model} 37x21 k=2", want, 4, need_empty=(stratum, model) == ("open", "ortho"))
    assert len(want) == 777


@pytest.mark.parametrize("stratum,camera", VA.CATALOGUE + VA.EXACT)
def test_catalogue_and_exact_route_cases(stratum, camera):
    v = VC.view(stratum, camera)
    check(f"{stratum} {camera}", VA.expected_catalogue(stratum, camera), v.rpp, need_empty=camera in VA.CATALOGUE_EMPTY)


def test_a_tile_of_the_expectation_is_the_frames_rows():
    """the restatement itself: global y and global seed ids make a tile's pairs the frame's rows"""
    name, model = VA.FIXTURES[1], "fisheye"
    v = V.standard_view(VA.scene(name), model)
    whole = VA.expected_standard(name, model)
    tile = VA.expected(VA.scene(name), v.tile(3, 2))
    assert np.array_equal(tile, whole[3 * 13:5 * 13])
