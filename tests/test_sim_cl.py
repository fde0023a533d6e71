"""The channels-last kernels (ganet_amd/csrc/cl_kernels.h: ganet_bn_apply_forward_cl, ganet_cost_volume_forward_cl) on the CPU
emulator build: the case table of tests/cl_cases.py (tests/test_gpu_cl.py runs the same table on the device), every buffer at a
guard page -- ENDING at one, resp. BEGINNING right behind one -- and every output pre-filled with NaN.  Equality of bits
throughout: against the planar entries of the same build on the permuted input, and against the numpy statement."""
import pytest

import cl_cases as cc
import parity_cases as pc


@pytest.fixture(scope="module")
def sim():
    from sim_util import sim_api
    return sim_api()


@pytest.fixture(params=["end", "start"])
def dev(request):
    return pc.NumpyDev(request.param)


@pytest.mark.parametrize("C", cc.BN_C)
@pytest.mark.parametrize("combo", list(cc.COMBOS))
def test_bn_apply_cl(sim, dev, combo, C):
    cc.check_bn_table(sim, dev, combo, C)


@pytest.mark.parametrize("combo", list(cc.COMBOS))
def test_bn_apply_cl_special_values(sim, dev, combo):
    cc.check_special(sim, dev, combo)


@pytest.mark.parametrize("combo", list(cc.COMBOS))
def test_bn_apply_cl_offset_bases(sim, dev, combo):
    cc.check_offsets(sim, dev, combo)


@pytest.mark.parametrize("combo", cc.INPLACE)
def test_bn_apply_cl_in_place(sim, dev, combo):
    cc.check_inplace(sim, dev, combo)


@pytest.mark.parametrize("combo", list(cc.SECOND_TRIP))
def test_bn_apply_cl_second_trip(sim, combo):
    cc.check_second_trip(sim, pc.NumpyDev(), combo)


@pytest.mark.parametrize("Dn", cc.CV_DN)
@pytest.mark.parametrize("C", cc.CV_C)
def test_cost_volume_cl(sim, dev, C, Dn):
    cc.check_cv_table(sim, dev, C, Dn)


def test_cost_volume_cl_blocks_and_bases(sim, dev):
    cc.check_cv_extra(sim, dev)


def test_bad_arguments(sim):
    cc.check_bad_arguments(sim, pc.NumpyDev())


def test_exports():
    from ganet_amd import _native
    assert _native.ABI_VERSION == 14
    assert sorted(_native._PROTOS_CL) == sorted(cc.ENTRIES)
    assert not set(_native._PROTOS_CL) & set(_native.EXPORTS)                # a table of its own: EXPORTS is include/ganet_hip.h's
