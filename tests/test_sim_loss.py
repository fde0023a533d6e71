"""The fused criterion (ganet_amd/csrc/loss_kernels.h: ganet_disparity_loss_workspace / _forward / _backward) on the CPU
emulator build: the case table of tests/loss_cases.py (tests/test_gpu_loss.py runs the same table on the device), every
case in both guard modes -- each buffer ENDS at an inaccessible page, resp. BEGINS right behind one
(parity_cases.guarded_empty) -- against the float64 yardstick of tests/loss_ref64.py, which the first tests here tie to
the project's own harness.steps.loss_mix and to the five values of the sequential MyLoss2 chain."""
import numpy as np
import pytest

import loss_cases as lc
import loss_ref64 as ref
import parity_cases as pc


@pytest.fixture(scope="module")
def sim():
    from sim_util import sim_api
    return sim_api()


@pytest.fixture(params=["end", "start"])
def dev(request):
    return pc.NumpyDev(request.param)


# ---- the yardstick itself -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,kitti", [("GANet_deep", True), ("GANet_deep", False), ("GANet11", True), ("GANet11", False)])
def test_yardstick_equals_loss_mix_in_float64(name, kitti):
    """harness.steps.loss_mix (boolean indexing, F.smooth_l1_loss, MyLoss2) on float64 CPU tensors, for both models' mixes.
    Maps on a 2^-10 grid below 64: p - t is exact in fp32, so the yardstick's fl32 residual is the float64 one."""
    import torch
    from harness import steps
    rng = np.random.default_rng(7)
    P = 2 if name == "GANet11" else 3
    t = (rng.integers(0, 60 * 1024, (2, 9, 11)) / 1024.0).astype(np.float32)
    preds = [(t + (rng.integers(-8 * 1024, 8 * 1024, t.shape) / 1024.0).astype(np.float32)).astype(np.float32) for _ in range(P)]
    kinds = ((0, 1) if P == 2 else (0, 0, 1)) if kitti else (0,) * P
    case = lc.Case("tie", t.shape, preds, t, kinds, lc.G11 if P == 2 else lc.DEEP, thresh=3, alpha=2)
    tt = torch.from_numpy(t).double()
    mask = tt < lc.HI
    assert 0 < int(mask.sum()) < t.size
    outs = [torch.from_numpy(p).double().requires_grad_() for p in preds]
    loss = steps.loss_mix(name, outs, tt, mask, steps.criterion(kitti))
    # the mix with the weights as Python floats, the way loss_mix holds them (the kernels read them as fp32: `ref.loss`)
    weights = lc.G11 if P == 2 else lc.DEEP
    want = sum(w * m for w, m in zip(weights, case.ref.mean_rho))
    assert abs(float(loss.detach()) - want) <= 1e-12 * want
    assert abs(case.ref.loss - want) <= 2.0 ** -24 * want
    err = torch.mean(torch.abs(outs[-1][mask] - tt[mask]))
    assert abs(float(err.detach()) - case.ref.epe[-1]) <= 1e-12 * case.ref.epe[-1]
    (loss * 0.37).backward()
    for k, (o, g) in enumerate(zip(outs, case.ref.grads(0.37, np.float64))):
        # (the statement holds 0.37 and the weight as the fp32 values the backward reads: rescaled here, not 1e-8 off)
        scale = float(np.float32(0.37)) / 0.37 * float(np.float32(weights[k])) / weights[k]
        assert np.allclose(o.grad.numpy() * scale, g, rtol=1e-12, atol=0)


@pytest.mark.parametrize("thresh,alpha,v,value,slope", lc.SPOTS)
def test_yardstick_spot_values_of_the_sequential_chain(thresh, alpha, v, value, slope):
    assert abs(float(ref.rho64(v, 1, thresh, alpha)) - value) <= 1e-12 * value
    assert abs(float(ref.slope(v, 1, thresh, alpha, np.float64)) - slope) <= 1e-12 * slope


def test_case_table_reaches_what_it_claims():
    by = {c.name: c for c in lc.CASES}
    n = lambda name: int(np.prod(by[name].shape))      # noqa: E731
    assert [n(f"shape-{k}") for k in ("1", "255", "256", "257")] == [1, 255, 256, 257]
    assert n("shape-257") > lc.BLOCK and n("shape-vec-2blocks") % 4 == 0 and n("shape-vec-2blocks") // 4 == lc.BLOCK + 1
    assert n("shape-scalar-stride2") == lc.STRIDE + 1 and n("shape-scalar-stride2") % 4
    assert n("shape-vec-stride2") == 4 * (lc.STRIDE + 1)
    for mode in (0, 1):
        c = by[f"targets-mode{mode}"]
        assert c.ref.ok.ravel().tolist() == lc.EDGE_VALID[mode]
    for c in lc.CASES:
        if c.exact:
            assert c.ref.count == c.target.size and c.ref.count & (c.ref.count - 1) == 0
            assert all(np.array_equal(r * 8, np.round(r * 8)) and np.abs(r).max() <= 4 for r in c.ref.r)
        if c.name.startswith("all-invalid"):
            assert c.ref.count == 0
    rs = {k for c in lc.CASES if not c.name.startswith(("all-invalid", "nan")) for k in np.unique(c.ref.ok)}
    assert rs == {True, False}


# ---- the kernels ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", lc.CASES, ids=repr)
def test_case(sim, dev, case):
    lc.check(case, lc.run(sim, dev, case))


@pytest.mark.parametrize("thresh,alpha,v,value,slope", lc.SPOTS)
def test_spot_values(sim, thresh, alpha, v, value, slope):
    """one pixel, weight 1, grad_loss 1: loss = rho(v) and the gradient = the slope, against the literal values"""
    case = next(c for c in lc.CASES if c.name == f"spot-t{thresh}a{alpha}-v{v}")
    got = lc.run(sim, pc.NumpyDev(), case)
    assert lc.close(got["loss"], value, lc.SUM_RTOL) and lc.close(got["grads"][0].item(), slope, lc.GRAD_RTOL)


@pytest.mark.parametrize("offset", [0, 1])
def test_poisoned_invalid_pixels_change_nothing(sim, dev, offset):
    clean, dirty = lc.poison_pair(offset=offset)
    a, b = lc.run(sim, dev, clean), lc.run(sim, dev, dirty)
    assert np.isfinite(b["loss"]) and np.isfinite(b["stats"]).all()
    assert lc.bits(a["loss"]) == lc.bits(b["loss"]) and np.array_equal(lc.bits(a["stats"]), lc.bits(b["stats"]))
    lc.check(dirty, b)
    for ga, gb in zip(a["grads"], b["grads"]):
        assert np.array_equal(lc.bits(ga), lc.bits(gb))


def test_bad_arguments(sim):
    from ganet_amd._native import E_INVALID, E_UNSUPPORTED, GanetError
    dev, case = pc.NumpyDev(), lc.CASES[1]
    N, H, W = case.shape
    bufs = [dev.to(a.ravel()) for a in case.preds + [case.target]]
    par, ws = dev.to(case.param_array()), dev.empty((2 * sim.query("ganet_disparity_loss_workspace", N, H, W),))
    loss, stats = dev.empty((1,)), dev.empty((10,))
    p = [dev.ptr(b) for b in bufs]

    def fwd(P=3, kinds=(0, 0, 1), mode=0, dims=(N, H, W), p2=p[2]):
        sim.call("ganet_disparity_loss_forward", p[0], p[1], p2, p[3], dev.ptr(par), dev.ptr(ws), dev.ptr(loss), dev.ptr(stats),
                 *dims, P, *kinds, mode, None)

    fwd()
    for kw in (dict(P=0), dict(P=4), dict(kinds=(0, 2, 0)), dict(mode=2), dict(dims=(0, H, W)), dict(p2=None)):
        with pytest.raises(GanetError) as e:
            fwd(**kw)
        assert e.value.code == E_INVALID, kw
    fwd(P=2, p2=None)                                   # an unused map is NULL
    for call in (lambda: fwd(dims=(1, 4096, 4096)), lambda: sim.query("ganet_disparity_loss_workspace", 1, 4096, 4096)):
        with pytest.raises(GanetError) as e:
            call()
        assert e.value.code == E_UNSUPPORTED
    assert sim.query("ganet_disparity_loss_workspace", 1, 4095, 4096) >= lc.GRID_CAP * 10
