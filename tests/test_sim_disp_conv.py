"""DispConv's kernels (ganet_amd/csrc/disp_conv_kernels.h: ganet_disp_conv_forward / _backward_data / _backward_weight) on the CPU
emulator build: the case table of tests/disp_conv_cases.py (tests/test_gpu_disp_conv.py runs the same table on the device), every
case in both guard modes -- each buffer ENDS at an inaccessible page, resp. BEGINS right behind one -- with the workspace and
every output pre-filled with NaN, against the float64 statement of tests/disp_conv_ref64.py.  The first tests calibrate that
yardstick on the CPU: it agrees with ATen's conv3d and its autograd to within the bars (and how closely is printed), equals
them on the exact family, the comparison discriminates against six wrong definitions, and the table reaches what its ids name."""
import os
import re

import numpy as np
import pytest

import disp_conv_cases as dc
import disp_conv_ref64 as ref
import parity_cases as pc

F32 = np.float32
GENERAL = [c for c in dc.CASES if c.kind == "general" and c.offset == 0]
EXACT = [c for c in dc.CASES if c.kind == "exact" and c.offset == 0]


@pytest.fixture(scope="module")
def sim():
    from sim_util import sim_api
    return sim_api()


@pytest.fixture(params=["end", "start"])
def dev(request):
    return pc.NumpyDev(request.param)


# ---- the yardstick and the table ------------------------------------------------------------------------------------------

def _aten(case):
    """F.conv3d and autograd's backward, in fp32 on the CPU"""
    import torch
    import torch.nn.functional as F
    x = torch.from_numpy(np.array(case.x)).requires_grad_()
    w = torch.from_numpy(np.array(case.weight)).requires_grad_()
    y = F.conv3d(x, w, None, 1, 1)
    y.backward(torch.from_numpy(np.array(case.grad_y))[:, None])
    return {"y": y.detach().numpy()[:, 0], "grad_x": x.grad.numpy(), "grad_weight": w.grad.numpy()[0]}


@pytest.mark.parametrize("case", GENERAL, ids=repr)
def test_yardstick_agrees_with_aten(case):
    """ATen's fp32 convolution is one more float32 evaluation of the definition: held to the same bars"""
    res = dc.check(case, _aten(case), verbose=False)
    print(f"{case.id}: ATen against the statement, worst error / bar  " + "  ".join(f"{q} {v:.3f}" for q, v in res.items()))


@pytest.mark.parametrize("case", EXACT, ids=repr)
def test_yardstick_equals_aten_on_the_exact_family(case):
    dc.premises(case)
    dc.check(case, _aten(case), verbose=False)             # kind "exact": equality


def _constants(hdr):
    c = {}
    for name, expr in re.findall(r"constexpr int (DCV_\w+) = ([^;]+);", hdr):
        c[name] = int(eval(expr, {}, dict(c)))
    return c


def test_case_table_reaches_what_it_claims():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "ganet_amd", "csrc", "disp_conv_kernels.h")).read()
    k = _constants(hdr)
    # the geometry and the roundings the statement's bound assumes are the ones written next to the kernels
    assert (k["DCV_WAVES"], k["DCV_PX"], k["DCV_DEPTH"], k["DCV_CB"], k["DCV_MAX_C"]) == (ref.WAVES, ref.PX, ref.DEPTH, ref.CB, ref.MAX_C)
    assert (k["DCV_L_FWD_PER_CHANNEL"], k["DCV_L_FWD_MERGE"], k["DCV_L_BWD_DATA"], k["DCV_L_BWD_WEIGHT"]) == \
        (ref.L_FWD_PER_CHANNEL, ref.L_FWD_MERGE, ref.L_BWD_DATA, ref.L_BWD_WEIGHT) == (27, 2, 27, 39)
    assert "blockIdx.x * 64" in hdr and dc.GROUPS_PER_BLOCK == 64
    # ... as the kernels sum: three FMA chains, (r0 + r1) + (r2 + r3), a wave reduction, rows added in fp64
    assert hdr.count("fmaf(") == 3 and "(r0.x + r1.x) + (r2.x + r3.x)" in hdr and "seg_allsum<64>(acc[j][t])" in hdr
    assert "a += (double)ws[r * K + col];" in hdr and "atomicAdd" not in hdr
    for c in dc.CASES:
        N, C, D, H, W = c.shape
        L = c.ref.L
        assert L["y"] <= 27 * C and L["grad_x"] <= 27 and L["grad_weight"] <= N * D * H * W
    assert ref.roundings(32, 10 ** 6) == {"y": 27 * 8 + 2, "grad_x": 27, "grad_weight": 39}
    by = lambda name: dc.by_name(name)                                           # noqa: E731
    assert sorted({c.shape[1] for c in dc.CASES} & {1, 3, 32, 64}) == [1, 3, 32, 64]
    assert by("C32-W70-N2-rows").shape == (2, 32, 3, 5, 70) and by("W130-N2").shape == (2, 5, 4, 6, 130)   # the issue's own two
    assert by("C3").shape[1] % ref.CB and by("C64").shape[1] == ref.MAX_C == 4 * ref.WAVES * ref.CB        # a block not full; four passes
    assert by("D1").shape[2] == 1 and by("D2").shape[2] == 2 and by("H1").shape[3] == 1 and by("W1").shape[4] == 1
    assert by("one").shape == (1, 1, 1, 1, 1)
    w = by("Wsmall").shape[4]
    assert w % 4 and w < 64
    for name in ("C32-W70-N2-rows", "W130-N2"):
        c = by(name)
        assert c.shape[4] % 4 and c.blocks > 1 and dc.GROUPS_PER_BLOCK % -(-c.shape[4] // 4) and c.shape[0] == 2
    assert by("W4").shape[4] == 4
    c = by("Hblocks")
    assert -(-c.shape[4] // 4) < dc.GROUPS_PER_BLOCK < c.groups and c.blocks == 2
    assert by("D9").shape[2] == ref.DEPTH + 1 and by("D9").chunks == 2 and by("D17").shape[2] == 2 * ref.DEPTH + 1 and by("D17").chunks == 3
    assert by("N2").shape[0] == 2
    a, o = by("aligned"), by("offset")
    assert a.shape == o.shape and a.shape[4] % 4 == 0 and a.shape[4] > 8 and (a.offset, o.offset) == (0, 1) and a.blocks > 1 and a.chunks > 1
    assert by("C1-row1").rows == 1 and by("C32-W70-N2-rows").rows == 4 and a.rows == 8
    for c in EXACT:
        dc.premises(c)


def _applies(case):
    return min(case.shape[2:]) > 1


@pytest.mark.parametrize("mutation", ref.MUTATIONS)
def test_comparison_discriminates(mutation):
    """each wrong definition exceeds the bar on every general case with more than one element per axis"""
    hit = []
    for case in GENERAL:
        if not _applies(case):
            continue
        res = dc.ratios(case, ref.mutant(case.x, case.weight, case.grad_y, mutation))
        assert max(res.values()) > 1, (case.id, mutation, res)
        hit.append(case.id)
    print(mutation, "exceeds the bar on", len(hit), "cases")
    assert len(hit) == len(GENERAL) - 4                      # (all but D1, H1, W1 and one)


def test_the_statement_itself_passes_the_comparison():
    for case in GENERAL:
        got = {q: a.astype(F32) for q, a in case.ref.results().items()}
        assert max(dc.ratios(case, got).values()) <= 0.5     # one rounding of the exact value: u |value| <= u sum |terms|


# ---- the kernels ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", dc.CASES, ids=repr)
def test_case(sim, dev, case):
    dc.check(case, dc.run(sim, dev, case))


def test_weight_gradient_twice_gives_the_same_bits(sim):
    case = dc.by_name("C32-W70-N2-rows")
    a, b = (dc.run(sim, pc.NumpyDev(), case)["grad_weight"] for _ in range(2))
    assert np.array_equal(a, b)


def test_bad_arguments(sim):
    dc.check_bad_arguments(sim, pc.NumpyDev())


def test_exports_and_abi():
    from ganet_amd import _native
    assert _native.ABI_VERSION == 14
    for name in ("ganet_disp_conv_workspace", "ganet_disp_conv_forward", "ganet_disp_conv_backward_data",
                 "ganet_disp_conv_backward_weight"):
        assert name in _native.EXPORTS
