"""conv32x1 on a 16-bit x (ganet_amd/csrc/disp_conv_kernels.h on a 16-bit storage type: ganet_disp_conv_forward_16 / _backward_data_16 /
_backward_weight_16) on the CPU emulator build: the case table of tests/mixed_conv_cases.py (tests/test_gpu_mixed_conv.py runs the
same table on the device), in both formats and both guard modes -- each buffer ENDS at an inaccessible page, resp. BEGINS right
behind one -- with the workspace and every output pre-filled with NaN patterns.  Equality of bits throughout: against the fp32
entries of the same build on the up-cast x, and on the exact family against the float64 statement."""
import numpy as np
import pytest

import mixed_cases as mc
import mixed_conv_cases as mcc
import parity_cases as pc

fmt_id = mc.FMT_NAME.get


@pytest.fixture(scope="module")
def sim():
    from sim_util import sim_api
    return sim_api()


@pytest.fixture(params=["end", "start"])
def dev(request):
    return pc.NumpyDev(request.param)


def test_case_table_reaches_what_it_claims():
    mcc.check_table()


@pytest.mark.parametrize("fmt", mcc.FMTS, ids=fmt_id)
@pytest.mark.parametrize("case", mcc.CASES, ids=repr)
def test_case(sim, dev, case, fmt):
    mcc.check_case(sim, dev, case, fmt)


@pytest.mark.parametrize("fmt", mcc.FMTS, ids=fmt_id)
def test_weight_gradient_twice_gives_the_same_bits(sim, fmt):
    case = mcc.by_name("C33-W8-H3-D9-N2")
    a, b = (mcc.run(sim, pc.NumpyDev(), case, fmt, which=("16",))["16"]["grad_weight"] for _ in range(2))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_bad_arguments(sim):
    mcc.check_bad_arguments(sim, pc.NumpyDev())
