"""The streaming and fused kernels (ganet_amd/csrc/misc_kernels.h) on the gfx950 build at their edge shapes: the case table of
tests/misc_cases.py, which tests/test_sim_misc_edges.py runs on the emulator.  What the model's own shapes never reach on the
device: the scalar twins of the 16-byte forms (sizes that are no multiple of four, tensors 4 bytes behind a 16-byte
boundary), depths of 1 / below / equal to / one more than a chunk of the depth loops and Dn > W, negative, exact-zero and
clamped-norm inputs of the normalisations, softmin columns that make the running-max rescale matter, the second trip of the
grid-stride loops (more than 4096 x 256 lanes, more than 65535 slices), trilinear zooms that take the backward's slow loop,
down-sampling and one-voxel axes.  The device's expf, division and fma contraction are not the emulator's: same inputs,
same float64 references, same bars."""
import pytest

import misc_cases as mc
from test_gpu_parity import TorchDev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from ganet_amd import _native
    lib = _native.lib()
    assert not lib.is_simulator, "GPU tests must run the gfx950 build"
    assert lib.path.endswith("ganet_amd/libganet_hip.so")
    return lib


@pytest.fixture(scope="module")
def dev():
    return TorchDev()


@pytest.mark.parametrize("case", mc.CASES, ids=repr)
def test_edge_case(api, dev, case):
    mc.check(case.run(api, dev))


@pytest.mark.parametrize("case", mc.GRID_CASES, ids=repr)
def test_grid_stride_second_trip(api, dev, case):
    """more lanes than the 4096 x 256 of one launch: the loops' `o += stride` and the n / pixel split behind it; outputs are
    poisoned with NaN first, so a lane that never came round shows"""
    mc.check(case.run(api, dev))
