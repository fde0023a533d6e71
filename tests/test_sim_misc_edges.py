"""Kernel logic of the streaming and fused kernels (ganet_amd/csrc/misc_kernels.h) at their edge shapes, on the CPU emulator
build: the case table of tests/misc_cases.py (tests/test_gpu_misc_edges.py runs the same table on the device), every case in
both guard modes -- each buffer ENDS at an inaccessible page, resp. BEGINS right behind one (parity_cases.guarded_empty) --
so that the clamped-address loads of the depth loops (Dn-1, W-1, row[whi]) are shown to stay inside their tensors.  The
misaligned (`-offset1`) tensors are views into a guarded flat allocation whose last element is the tensor's last element.

The grid-stride cases (`-stride2`) take 1 - 3 s each here and run; the four `residual-gridy` cases (65538 slices: two launches
of 65535 blocks, 26 s each on the emulator, which pays per block) run on the device only."""
import pytest

import misc_cases as mc
import parity_cases as pc


@pytest.fixture(scope="module")
def sim():
    from sim_util import sim_api
    return sim_api()


@pytest.fixture(params=["end", "start"])
def dev(request):
    return pc.NumpyDev(request.param)


@pytest.mark.parametrize("case", [c for c in mc.CASES if not c.device_only], ids=repr)
def test_edge_case(sim, dev, case):
    mc.check(case.run(sim, dev))


@pytest.mark.parametrize("case", mc.GRID_CASES, ids=repr)
def test_grid_stride_second_trip(sim, dev, case):
    """more lanes than the 4096 x 256 of one launch: the loops' `o += stride` and the n / pixel split behind it"""
    mc.check(case.run(sim, dev))
