"""DispTail's kernels (ganet_amd/csrc/disp_tail_kernels.h: ganet_up_softmin_regression_forward / _backward) on the CPU emulator
build: the case table of tests/disp_tail_cases.py (tests/test_gpu_disp_tail.py runs the same table on the device), every case
in both guard modes -- each buffer ENDS at an inaccessible page, resp. BEGINS right behind one -- with the workspace and every
output pre-filled with NaN, against the float64 statement of tests/disp_tail_ref64.py.  The first tests calibrate that
yardstick on the CPU: it agrees with ATen's chain to within the bars (and how closely is printed), the float32 model of the
kernels' arithmetic stays inside half of every bar in both variants of lambda, the comparison discriminates against five wrong
definitions, and the table reaches the branches its ids name."""
import os

import numpy as np
import pytest

import disp_tail_cases as dc
import disp_tail_ref64 as ref
import parity_cases as pc

F32 = np.float32
GENERAL = [c for c in dc.CASES if c.kind == "general"]


@pytest.fixture(scope="module")
def sim():
    from sim_util import sim_api
    return sim_api()


@pytest.fixture(params=["end", "start"])
def dev(request):
    return pc.NumpyDev(request.param)


# ---- the yardstick and the table ------------------------------------------------------------------------------------------

def _aten_chain(x, size, gout):
    """F.interpolate(trilinear) -> Softmin(dim=1) -> sum_d d * p, and autograd's backward, in fp32 on the CPU"""
    import torch
    import torch.nn.functional as F
    xt = torch.from_numpy(np.array(x)).requires_grad_()
    v = F.interpolate(xt[:, None], size=list(size), mode="trilinear", align_corners=False).squeeze(1)
    p = F.softmin(v, dim=1)
    out = (p * torch.arange(size[0], dtype=torch.float32)[None, :, None, None]).sum(1)
    out.backward(torch.from_numpy(np.array(gout)))
    return v.detach().numpy(), out.detach().numpy(), xt.grad.numpy()


@pytest.mark.parametrize("case", [c for c in GENERAL if c.id.split("-")[0] not in ("stride2",)], ids=repr)
def test_yardstick_agrees_with_aten(case):
    """ATen's fp32 chain is one more float32 evaluation of the definition: held to the bars of out and grad_x; v to twice
    its bound"""
    v, out, gx = _aten_chain(case.x, case.size, case.grad_out)
    r = case.ref
    res = dc.ratios(case, {"out": out, "grad_x": gx}, ("out", "grad_x"))
    with np.errstate(all="ignore"):
        rv = float(np.where(np.abs(v - r.v) == 0, 0.0, np.abs(v - r.v) / (2 * r.ev)).max())
    print(f"{case.id}: ATen against the statement: |v| off by {np.abs(v - r.v).max():.2e} ({rv:.3f} of the bar), "
          f"out by {np.abs(out - r.out).max():.2e} ({res['out']:.3f}), grad_x {res['grad_x']:.3f}")
    assert rv <= 1 and res["out"] <= 1 and res["grad_x"] <= 1


def test_case_table_reaches_what_it_claims():
    by = dc.BY_ID
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    capi = open(os.path.join(root, "ganet_amd", "csrc", "ganet_capi.hip")).read()
    # ew_grid: 256 lanes per block, at most 256 * 16 blocks, through the launchers' one clamp
    assert "int ew_grid(i64 n) { return clamp_grid(n, 256, 256 * 16); }" in capi and dc.MAX_LANES == 256 * 16 * 256
    clamp = capi[capi.index("int clamp_grid(i64 count, int per_block, i64 cap)"):][:200]
    assert "(count + per_block - 1) / per_block;" in clamp and "return (int)(g < 1 ? 1 : (g < cap ? g : cap));" in clamp
    hdr = open(os.path.join(root, "ganet_amd", "csrc", "disp_tail_kernels.h")).read()
    assert f"od0 += {ref.CHUNK})" in hdr
    misc = open(os.path.join(root, "ganet_amd", "csrc", "misc_kernels.h")).read()
    assert "constexpr int UP_MAXFP = 12;" in misc
    c = by["stride2-1x1x6x20561-to-2x17x61681"]
    assert c.shape[0] * c.size[1] * c.size[2] == dc.MAX_LANES + 1 and c.size[0] == 2 and c.shape[1] == 1
    assert sorted(c.size[0] for c in dc.CASES if c.id.startswith("Do")) == [1, 7, 8, 9, 17]
    m = by["model-2x5x4x6-to-13x12x18"]
    assert m.shape[1] == m.size[0] // 3 + 1 and m.size[1:] == (3 * m.shape[2], 3 * m.shape[3])
    # skipped planes, planes in front of the first d0 and behind the last d1
    skip = by["down-skip-1x9x3x3-to-4x7x5"].ref.ad
    assert (np.diff(skip.i0) > 1).any() and skip.unread()[1:-1].any()
    tail = by["down-tail-1x12x2x2-to-2x4x4"].ref.ad
    assert tail.i0[0] > 0 and tail.i1[-1] < 11 and tail.unread()[0] and tail.unread()[-1]
    for cid in ("down-skip-1x9x3x3-to-4x7x5", "down-tail-1x12x2x2-to-2x4x4"):
        u = by[cid].ref.ad.unread()
        assert not by[cid].ref.gc[:, u].any() and by[cid].ref.gc[:, ~u].all()
    # d1 == d0 on the last plane, and with a single plane
    assert (m.ref.ad.i1[-1] == m.ref.ad.i0[-1]) and m.ref.ad.lam[-1] > 0
    assert not by["Di1-1x1x3x4-to-5x6x8"].ref.ad.i1.any()
    # the reuse of c[d1] as the next c[d0], and a stay on the same pair
    assert (np.diff(m.ref.ad.i0) == 1).any() and (np.diff(m.ref.ad.i0) == 0).any()
    # stage 2's slow loop: an input column with UP_MAXFP + 1 readers or more has a footprint of at least UP_MAXFP + 1 outputs
    assert by["slowloop-1x3x2x2-to-7x5x29"].ref.aw.readers().max() >= 13
    assert all(c.ref.aw.readers().max() < 12 for c in dc.CASES if not c.id.startswith("slowloop"))
    # the edge columns: the maximum rises to the last plane and the first terms underflow in fp32; resp. it stays in chunk 0
    f, r = by["fall-1x7x2x3-to-19x5x7"].ref, by["rise-1x7x2x3-to-19x5x7"].ref
    assert (np.argmax(-f.v, 1) == 18).all() and (np.exp(-f.v[:, 0] - f.mx) < 1e-45).all()
    assert (np.argmax(-r.v, 1) == 0).all() and (np.exp(-r.v[:, -1] - r.mx) < 1e-45).all()
    # the exact family's premises
    for c in dc.CASES:
        if c.kind in ("exact", "dyadic"):
            for ax in (c.ref.ad, c.ref.ah, c.ref.aw):
                fma = ref.Axis(ax.n_in, ax.n_out, "fma")
                assert ax.n_out in (2 * ax.n_in, 4 * ax.n_in) and np.array_equal(ax.lam, fma.lam) and np.array_equal(ax.i0, fma.i0)
                assert np.array_equal(ax.lam * 8, np.round(ax.lam * 8))
            assert np.array_equal(c.x * 16, np.round(c.x * 16))
        if c.kind == "exact":
            assert (c.x == c.x[:, :1]).all() and c.size[0] in (8, 16)
            for a in c.ref.results().values():
                assert np.array_equal(a.astype(F32).astype(np.float64), a)
        if c.kind == "dyadic":
            assert (c.x != c.x[:, :1]).any() and np.array_equal(c.ref.mx.astype(F32).astype(np.float64), c.ref.mx)


@pytest.mark.parametrize("variant", ["plain", "fma"])
@pytest.mark.parametrize("case", dc.CASES, ids=repr)
def test_float32_model_stays_inside_half_of_every_bar(case, variant):
    got = ref.Float32Model(case.x, case.size, case.grad_out, variant).results()
    dc.check(case, got, limit=0.5)


def test_lambda_variants_differ_somewhere():
    """the two evaluations of src do part (otherwise the lambda term would be untested) at 65 -> 193, the model's depth axis:
    by at most dlam, and at od = 96, where src is 32 but for its rounding, they even choose neighbouring planes"""
    a, b = ref.Axis(65, 193, "plain"), ref.Axis(65, 193, "fma")
    d = np.abs(a.src.astype(np.float64) - b.src)
    same = a.i0 == b.i0
    assert d.max() > 0 and (d <= a.dlam).all() and np.array_equal(a.lam[same] != b.lam[same], d[same] > 0)
    assert list(np.nonzero(~same)[0]) == [96] and {int(a.i0[96]), int(b.i0[96])} == {31, 32}
    assert 2.0 ** -19 <= a.dlam[190] <= 2.0 ** -17


def _applies(case, mutation):
    Di, Hi, Wi = case.shape[1:]
    if mutation == "align_corners":
        return max(Di, Hi, Wi) > 1
    if mutation == "swap_lambda_d":            # (down-tail's depth weights are all 1/2: the swap is the identity there)
        ad = case.ref.ad
        return Di > 1 and bool(((ad.i1 != ad.i0) & (ad.lam != 0.5)).any())
    if mutation == "gc_skipped_unwritten":
        return bool(case.ref.ad.unread().any())
    return case.size[0] > 1 or mutation == "od_plus_1"


@pytest.mark.parametrize("mutation", ref.MUTATIONS)
def test_comparison_discriminates(mutation):
    """each wrong definition exceeds the bar on every general case it applies to"""
    hit = []
    for case in GENERAL:
        if not _applies(case, mutation):
            continue
        res = dc.ratios(case, ref.mutant(case.x, case.size, case.grad_out, mutation))
        assert max(res.values()) > 1, (case.id, mutation, res)
        hit.append(case.id)
    print(mutation, "exceeds the bar on", len(hit), "cases")
    if mutation == "gc_skipped_unwritten":
        assert hit == ["down-skip-1x9x3x3-to-4x7x5", "down-tail-1x12x2x2-to-2x4x4"]
    else:
        # (a single input plane has no depth weights to swap, a single output plane no distribution to regress over)
        assert "model-2x5x4x6-to-13x12x18" in hit and len(hit) >= len(GENERAL) - 5, hit


# ---- the kernels ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", dc.CASES, ids=repr)
def test_case(sim, dev, case):
    dc.check(case, dc.run(sim, dev, case))


def test_bad_arguments(sim):
    dc.check_bad_arguments(sim, pc.NumpyDev())


def test_exports_and_abi():
    from ganet_amd import _native
    assert _native.ABI_VERSION == 14
    for name in ("ganet_up_softmin_regression_forward", "ganet_up_softmin_regression_backward"):
        assert name in _native.EXPORTS


# ---- the host side (no device) --------------------------------------------------------------------------------------------

def test_module_refuses_cpu_and_non_fp32():
    import torch
    from ganet_amd.modules.fused import DispTail
    tail = DispTail(12)
    with pytest.raises((RuntimeError, ValueError, TypeError)):
        tail(torch.zeros(1, 1, 5, 4, 6))
    with pytest.raises((RuntimeError, ValueError, TypeError)):
        tail(torch.zeros(1, 1, 5, 4, 6, dtype=torch.float16))


def test_use_fused_disp_tail_rebinds_every_disp_and_nothing_else():
    import torch
    from ganet_amd.modules.fused import DispTail, SoftminDisparityRegression
    from harness import fuse

    class Disp(torch.nn.Module):
        def __init__(self, maxdisp=12):
            super().__init__()
            self.maxdisp = maxdisp
            self.conv32x1 = torch.nn.Conv3d(32, 1, 3, 1, 1, bias=False)

    class DispAgg(Disp):
        pass

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.disp0, self.disp1, self.disp2 = Disp(), Disp(), DispAgg()

    net = Net()
    keys = list(net.state_dict())
    assert fuse.use_fused_disp_tail(net) == 2
    assert isinstance(net.disp0._fused_tail, DispTail) and net.disp0._fused_tail.ndisp == 13 and net.disp0._fused_tail.zoom == 3
    assert "_fused_tail" not in net.disp2.__dict__ and "forward" not in net.disp2.__dict__
    assert list(net.state_dict()) == keys
    # after use_fused_ops: the Disp call sites move on, the DispAgg one stays what use_fused_ops made it
    net = Net()
    net.disp2.__class__.__name__ = "DispAgg"
    assert fuse.use_fused_ops(net) == 3 and isinstance(net.disp0._fused_tail, SoftminDisparityRegression)
    agg_tail = net.disp2._fused_tail
    assert fuse.use_fused_disp_tail(net) == 2
    assert isinstance(net.disp0._fused_tail, DispTail) and isinstance(net.disp1._fused_tail, DispTail)
    assert net.disp2._fused_tail is agg_tail and list(net.state_dict()) == keys
