"""DispTail on the gfx950 build: the case table of tests/disp_tail_cases.py through the C ABI (tests/test_sim_disp_tail.py runs it
on the emulator) -- same inputs, same float64 statement, same bars -- and, device only, through
ganet_amd.modules.fused.DispTail: against the two-op chain TrilinearUpsample -> SoftminDisparityRegression with both held to the
statement, the autograd properties of tests/test_gpu_autograd.py (backward twice, awkward incoming gradients, partial
requires_grad, accumulation, inputs unwritten, graph capture, no host synchronisation), harness.fuse.use_fused_disp_tail on a
stand-in for the reference's Disp, and the peak memory of forward + backward."""
import copy

import numpy as np
import pytest

import disp_tail_cases as dc
import disp_tail_ref64 as ref
from test_gpu_parity import TorchDev

pytestmark = pytest.mark.gpu
F32 = np.float32
MODEL = dc.BY_ID["model-2x5x4x6-to-13x12x18"]


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


def host(t):
    return t.detach().cpu().numpy()


# ---- C ABI: the shared table ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", dc.CASES, ids=repr)
def test_case(api, dev, case):
    dc.check(case, dc.run(api, dev, case))


def test_bad_arguments(api, dev):
    dc.check_bad_arguments(api, dev)


# ---- the module ------------------------------------------------------------------------------------------------------------

def tail_and_chain(case):
    """(DispTail, the two-op chain use_fused_ops installs) for a table case with a 3x zoom in H and W"""
    from ganet_amd.modules.fused import DispTail, SoftminDisparityRegression, TrilinearUpsample
    Do, Ho, Wo = case.size
    assert (Ho, Wo) == (3 * case.shape[2], 3 * case.shape[3])
    up, reg = TrilinearUpsample(), SoftminDisparityRegression(Do - 1)
    return DispTail(Do - 1), lambda c: reg(up(c, [Do, Ho, Wo]).squeeze(1))


def forward_backward(op, case, dev, five_d=True):
    x = dev.to(np.array(case.x[:, None] if five_d else case.x)).requires_grad_()
    out = op(x)
    out.backward(dev.to(np.array(case.grad_out)))
    return {"out": host(out), "grad_x": host(x.grad).reshape(case.shape)}


def test_module_against_the_two_op_chain(api, dev):
    """the same input through DispTail and through TrilinearUpsample -> SoftminDisparityRegression: both are float32 evaluations
    of one definition, both are held to its float64 statement"""
    tail, chain = tail_and_chain(MODEL)
    mine = dc.check(MODEL, forward_backward(tail, MODEL, dev), ("out", "grad_x"), verbose=False)
    theirs = dc.check(MODEL, forward_backward(chain, MODEL, dev), ("out", "grad_x"), verbose=False)
    print("worst error / bar  " + "  ".join(f"{q}: DispTail {mine[q]:.3f} two-op chain {theirs[q]:.3f}" for q in mine))
    four = forward_backward(tail, MODEL, dev, five_d=False)                    # [N,D,H,W] is accepted as well
    five = forward_backward(tail, MODEL, dev)
    assert all(np.array_equal(four[q], five[q]) for q in four)


def _fresh(dev, case, seed):
    rng = np.random.default_rng(seed)
    return (dev.to(rng.standard_normal((case.shape[0], 1) + case.shape[1:]).astype(F32)),
            dev.to(rng.standard_normal((case.shape[0],) + case.size[1:]).astype(F32)))


def test_backward_twice_and_accumulation(api, dev):
    """the context is re-entrant (nothing saved is used as scratch), and .grad accumulates"""
    import torch
    tail, _ = tail_and_chain(MODEL)
    x, g = dev.to(np.array(MODEL.x[:, None])).requires_grad_(), dev.to(np.array(MODEL.grad_out))
    out = tail(x)
    saved = [t.clone() for t in out.grad_fn.saved_tensors]
    assert len(saved) == 4
    first, = torch.autograd.grad(out, x, g, retain_graph=True)
    second, = torch.autograd.grad(out, x, g, retain_graph=True)
    assert torch.equal(first, second) and all(torch.equal(a, b) for a, b in zip(out.grad_fn.saved_tensors, saved))
    dc.check(MODEL, {"grad_x": host(first).reshape(MODEL.shape)}, ("grad_x",), verbose=False)
    out.backward(g, retain_graph=True)
    out.backward(g)
    assert torch.equal(x.grad, first + first)


@pytest.mark.parametrize("form", ["expanded", "permuted", "offset"])
def test_awkward_incoming_gradient(api, dev, form):
    """stride-0 (what out.sum().backward() delivers), a permuted view, a contiguous slice 4 bytes into a buffer; never written"""
    import torch
    tail, _ = tail_and_chain(MODEL)
    x, g = dev.to(np.array(MODEL.x[:, None])).requires_grad_(), dev.to(np.array(MODEL.grad_out))
    if form == "expanded":
        go = torch.ones((), device=g.device).expand(g.shape)
    elif form == "permuted":
        go = g.transpose(-1, -2).contiguous().transpose(-1, -2)
        assert not go.is_contiguous()
    else:
        buf = torch.empty(g.numel() + 1, device=g.device)
        go = buf[1:].view(g.shape)
        go.copy_(g)
        assert go.is_contiguous() and go.data_ptr() % 16 == 4
    keep = go.clone()
    want, = torch.autograd.grad(tail(x), x, go.contiguous().clone())
    got, = torch.autograd.grad(tail(x), x, go)
    assert torch.equal(got, want) and torch.equal(go, keep) and bool(torch.isfinite(got).all())


def test_partial_requires_grad_and_inputs_unwritten(api, dev, monkeypatch):
    """an input that wants no gradient, and no_grad: the same output, nothing saved, the backward entry never called; the
    input is not written by either direction"""
    import torch
    tail, _ = tail_and_chain(MODEL)
    calls, call = [], api.call
    monkeypatch.setattr(api, "call", lambda name, *a: (calls.append(name), call(name, *a))[1])
    x = dev.to(np.array(MODEL.x[:, None]))
    keep = x.clone()
    plain = tail(x)
    with torch.no_grad():
        quiet = tail(x.clone().requires_grad_())
    assert not plain.requires_grad and not quiet.requires_grad and torch.equal(plain, quiet)
    xr = x.clone().requires_grad_()
    out = tail(xr)
    assert torch.equal(out, plain) and torch.equal(xr, keep)
    assert calls == ["ganet_up_softmin_regression_forward"] * 3
    out.backward(dev.to(np.array(MODEL.grad_out)))
    assert calls[-1] == "ganet_up_softmin_regression_backward" and torch.equal(xr, keep) and torch.equal(x, keep)
    # behind a frozen convolution whose input wants the gradient, and behind a trainable one on a constant input
    conv = torch.nn.Conv3d(2, 1, 3, padding=1, bias=False).cuda()
    inp = dev.to(np.random.default_rng(5).standard_normal((2, 2) + MODEL.shape[1:]).astype(F32))
    for freeze, inp_grad in ((True, True), (False, False)):
        conv.requires_grad_(not freeze)
        conv.weight.grad = None
        i = inp.clone().requires_grad_(inp_grad)
        tail(conv(i)).backward(dev.to(np.array(MODEL.grad_out)))
        assert (i.grad is not None) == inp_grad and (conv.weight.grad is not None) == (not freeze)


def test_no_host_synchronisation(api, dev):
    import torch
    tail, _ = tail_and_chain(MODEL)
    forward_backward(tail, MODEL, dev)                       # first use: library load, allocator warm-up
    x, g = dev.to(np.array(MODEL.x[:, None])).requires_grad_(), dev.to(np.array(MODEL.grad_out))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = tail(x)
        out.backward(g)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    dc.check(MODEL, {"out": host(out), "grad_x": host(x.grad).reshape(MODEL.shape)}, ("out", "grad_x"), verbose=False)


def test_graph_capture_and_replay(api, dev):
    """forward + backward captured once on a single stream and replayed on new data: bit-equal to the eager call"""
    import torch
    tail, _ = tail_and_chain(MODEL)
    x, g = _fresh(dev, MODEL, 1)
    x.requires_grad_()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            torch.autograd.grad(tail(x), x, g)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = tail(x)
        gx, = torch.autograd.grad(out, x, g)
    for seed in (2, 3):
        nx, ng = _fresh(dev, MODEL, seed)
        with torch.no_grad():
            x.copy_(nx), g.copy_(ng)
        graph.replay()
        torch.cuda.synchronize()
        eo = tail(x)
        eg, = torch.autograd.grad(eo, x, g)
        assert torch.equal(out, eo) and torch.equal(gx, eg) and bool(torch.isfinite(gx).all())


# ---- harness.fuse.use_fused_disp_tail on a stand-in -------------------------------------------------------------------------

def stand_in(maxdisp):
    """the reference's Disp (models/GANet_deep.py:203-219 is not on a test machine: restated here by what use_fused_disp_tail
    reads -- the class name, maxdisp and conv32x1 -- and by its forward)"""
    import torch
    import torch.nn.functional as F

    class Disp(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.maxdisp = maxdisp
            self.conv32x1 = torch.nn.Conv3d(32, 1, (3, 3, 3), (1, 1, 1), (1, 1, 1), bias=False)

        def forward(self, x):
            x = F.interpolate(self.conv32x1(x), [self.maxdisp + 1, x.size()[3] * 3, x.size()[4] * 3], mode="trilinear", align_corners=False)
            x = F.softmin(torch.squeeze(x, 1), dim=1)
            d = torch.arange(self.maxdisp + 1, device=x.device, dtype=x.dtype).view(1, -1, 1, 1)
            return torch.sum(x * d, 1)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.disp0 = Disp()

        def forward(self, x):
            return self.disp0(x)

    torch.manual_seed(31)
    return Net().cuda()


def test_use_fused_disp_tail_on_a_stand_in(api, dev):
    """Conv3d(32,1,3) + the tail, stock and rebound, alone and after use_fused_ops.  The bars: the statement at each form's own
    convolution output c (read by a forward hook) gives out, grad_c and their bounds;
    the weight gradient is the correlation of the input with grad_c over n = N D H W positions: the bound of grad_c passes
    through it with |input|, and its own fp32 accumulation adds at most n u of the same correlation of the absolute values.
    Twice that, as everywhere; the stock chain's distance in the same unit is printed beside ours."""
    import torch
    from harness import fuse
    N, Di, Hi, Wi = MODEL.shape
    stock = stand_in(MODEL.size[0] - 1)
    alone, after = copy.deepcopy(stock), copy.deepcopy(stock)
    assert fuse.use_fused_disp_tail(alone) == 1
    assert fuse.use_fused_ops(after) == 1 and fuse.use_fused_disp_tail(after) == 1
    assert list(alone.state_dict()) == list(stock.state_dict()) == list(after.state_dict())
    rng = np.random.default_rng(32)
    inp = dev.to((0.2 * rng.standard_normal((N, 32, Di, Hi, Wi))).astype(F32))
    g = dev.to(np.array(MODEL.grad_out))
    w = stock.disp0.conv32x1.weight
    corr = lambda a, b: torch.nn.grad.conv3d_weight(torch.from_numpy(np.ascontiguousarray(a)), w.shape,   # noqa: E731
                                                    torch.from_numpy(np.ascontiguousarray(b))[:, None], padding=1).numpy()
    i64, ai64 = host(inp).astype(np.float64), np.abs(host(inp)).astype(np.float64)
    res = {}
    for name, model in (("stock", stock), ("alone", alone), ("after use_fused_ops", after)):
        seen = []
        hook = model.disp0.conv32x1.register_forward_hook(lambda mod, args, y: seen.append(y.detach()))
        model.zero_grad()
        out = model(inp)
        out.backward(g)
        hook.remove()
        c = host(seen[0])[:, 0]                                  # this form's own convolution output
        st = ref.Statement(c, MODEL.size, MODEL.grad_out)
        want_gw = corr(i64, st.grad_x)
        bound_gw = corr(ai64, st.b_grad_x) + c.size * ref.U * corr(ai64, np.abs(st.grad_x))
        r_out = float((np.abs(host(out) - st.out) / (2 * st.b_out)).max())
        r_gw = float((np.abs(host(model.disp0.conv32x1.weight.grad) - want_gw) / (2 * bound_gw)).max())
        res[name] = (r_out, r_gw)
        print(f"{name}: worst error / bar  out {r_out:.3f}  grad of the convolution weight {r_gw:.3f}")
    for name in ("alone", "after use_fused_ops"):
        assert res[name][0] <= 1 and res[name][1] <= 1, (name, res[name])
    assert res["alone"] == res["after use_fused_ops"]


# ---- memory ----------------------------------------------------------------------------------------------------------------

def test_peak_memory_stays_below_one_upsampled_volume(api, dev):
    """[1,33,40,52] -> (97,120,156): the up-sampled volume is 7.3 MB, the column workspace 2.5 MB.  Forward + backward of
    DispTail must raise torch.cuda.max_memory_allocated by less than ONE volume; the two-op chain raises it by at least two
    (the volume, saved for the backward, and its gradient)."""
    import torch
    from ganet_amd.modules.fused import DispTail, SoftminDisparityRegression, TrilinearUpsample
    shape, size = (1, 1, 33, 40, 52), (97, 120, 156)
    volume = 4 * size[0] * size[1] * size[2]
    rng = np.random.default_rng(41)
    x_np, g_np = rng.standard_normal(shape).astype(F32), rng.standard_normal((1,) + size[1:]).astype(F32)
    up, reg, tail = TrilinearUpsample(), SoftminDisparityRegression(size[0] - 1), DispTail(size[0] - 1)
    rise, outs = {}, {}
    for name, op in (("two-op chain", lambda c: reg(up(c, list(size)).squeeze(1))), ("DispTail", tail)):
        for attempt in range(2):                                   # (the first pass warms the library and the allocator)
            x, g = dev.to(x_np).requires_grad_(), dev.to(g_np)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = op(x)
            out.backward(g)
            torch.cuda.synchronize()
            rise[name] = torch.cuda.max_memory_allocated() - base
            outs[name] = (out.detach(), x.grad)
            del out, x, g
    print("peak memory over forward + backward, in up-sampled volumes: " + "  ".join(f"{k} {v / volume:.2f}" for k, v in rise.items()))
    assert rise["DispTail"] < volume, rise
    assert rise["two-op chain"] >= 2 * volume, rise
    assert all(bool(torch.isfinite(t).all()) for pair in outs.values() for t in pair)
