"""DispConv on the gfx950 build: the case table of tests/disp_conv_cases.py through the C ABI (tests/test_sim_disp_conv.py runs it on
the emulator) -- same inputs, same float64 statement, same bars -- and, device only, through ganet_amd.modules.fused.DispConv:
against torch.nn.functional.conv3d with both held to the statement, the autograd properties of tests/test_gpu_autograd.py
(backward twice, accumulation, awkward incoming gradients, partial requires_grad, inputs unwritten, graph capture, a side
stream, no host synchronisation), the bit-reproducible weight gradient, and harness.fuse.use_fused_disp_conv on stand-ins for the
reference's Disp and DispAgg."""
import copy

import numpy as np
import pytest

import disp_conv_cases as dc
import disp_conv_ref64 as ref
from test_gpu_parity import TorchDev

pytestmark = pytest.mark.gpu
F32 = np.float32
MODEL = dc.by_name("C32-W70-N2-rows")          # [2,32,3,5,70]: the model's channel count, W % 4 != 0, four partial rows
ALIGNED = dc.by_name("aligned")                # [2,4,9,5,68]: the 16-byte kernels, two depth chunks


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

def conv_of(case, dev):
    import torch
    conv = torch.nn.Conv3d(case.shape[1], 1, (3, 3, 3), (1, 1, 1), (1, 1, 1), bias=False).cuda()
    with torch.no_grad():
        conv.weight.copy_(dev.to(np.array(case.weight)))
    return conv


def forward_backward(op, conv, case, dev):
    conv.weight.grad = None
    x = dev.to(np.array(case.x)).requires_grad_()
    y = op(x)
    y.backward(dev.to(np.array(case.grad_y))[:, None])
    return {"y": host(y)[:, 0], "grad_x": host(x.grad), "grad_weight": host(conv.weight.grad)[0]}


@pytest.mark.parametrize("case", [MODEL, ALIGNED], ids=repr)
def test_module_against_conv3d(api, dev, case):
    """the same input through DispConv and through F.conv3d (MIOpen): both are float32 evaluations of one definition, both
    are held to its float64 statement"""
    from ganet_amd.modules.fused import DispConv
    conv = conv_of(case, dev)
    mine = dc.check(case, forward_backward(DispConv(conv), conv, case, dev), verbose=False)
    theirs = dc.check(case, forward_backward(conv, conv, case, dev), verbose=False)
    print(f"{case.id}: worst error / bar  " + "  ".join(f"{q}: DispConv {mine[q]:.3f} conv3d {theirs[q]:.3f}" for q in mine))


def test_directions_left_on_aten(api, dev, monkeypatch):
    """every subset of directions gives results inside the bars, and only the chosen entries are called"""
    from ganet_amd.modules.fused import DispConv
    calls, call = [], api.call
    monkeypatch.setattr(api, "call", lambda name, *a: (calls.append(name), call(name, *a))[1])
    conv = conv_of(ALIGNED, dev)
    for directions in (("forward",), ("data",), ("weight",), ("forward", "weight"), ()):
        del calls[:]
        dc.check(ALIGNED, forward_backward(DispConv(conv, directions), conv, ALIGNED, dev), verbose=False)
        want = [n for d, n in (("forward", "ganet_disp_conv_forward"), ("data", "ganet_disp_conv_backward_data"),
                               ("weight", "ganet_disp_conv_backward_weight")) if d in directions]
        assert calls == want, (directions, calls)


def test_backward_twice_and_accumulation(api, dev):
    """the context is re-entrant (nothing saved is used as scratch), and .grad of both x and the weight accumulates"""
    import torch
    from ganet_amd.modules.fused import DispConv
    conv = conv_of(MODEL, dev)
    op = DispConv(conv)
    x, g = dev.to(np.array(MODEL.x)).requires_grad_(), dev.to(np.array(MODEL.grad_y))[:, None]
    y = op(x)
    saved = [t.clone() for t in y.grad_fn.saved_tensors]
    assert len(saved) == 2 and saved[0].shape == x.shape and saved[1].shape == conv.weight.shape
    first = torch.autograd.grad(y, (x, conv.weight), g, retain_graph=True)
    second = torch.autograd.grad(y, (x, conv.weight), g, retain_graph=True)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    assert all(torch.equal(a, b) for a, b in zip(y.grad_fn.saved_tensors, saved))
    dc.check(MODEL, {"grad_x": host(first[0]), "grad_weight": host(first[1])[0]}, ("grad_x", "grad_weight"), verbose=False)
    y.backward(g, retain_graph=True)
    y.backward(g)
    assert torch.equal(x.grad, first[0] + first[0]) and torch.equal(conv.weight.grad, first[1] + first[1])


@pytest.mark.parametrize("form", ["expanded", "permuted", "offset"])
def test_awkward_incoming_gradient(api, dev, form):
    """stride-0 (what y.sum().backward() delivers), a permuted view, a contiguous slice 4 bytes into a buffer; never written"""
    import torch
    from ganet_amd.modules.fused import DispConv
    conv = conv_of(ALIGNED, dev)
    op = DispConv(conv)
    x, g = dev.to(np.array(ALIGNED.x)).requires_grad_(), dev.to(np.array(ALIGNED.grad_y))[:, None]
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
    want = torch.autograd.grad(op(x), (x, conv.weight), go.contiguous().clone())
    got = torch.autograd.grad(op(x), (x, conv.weight), go)
    # (the offset form runs the 4-byte kernels, the aligned clone the 16-byte ones: the same sums in the same order)
    assert all(torch.equal(a, b) and bool(torch.isfinite(a).all()) for a, b in zip(got, want)) and torch.equal(go, keep)


def test_partial_requires_grad_and_inputs_unwritten(api, dev, monkeypatch):
    """a frozen weight, an input that wants no gradient, and no_grad: the same output, only the entries that are needed are
    called, nothing is saved under no_grad; neither x nor the weight is written by any direction"""
    import torch
    from ganet_amd.modules.fused import DispConv
    FWD, DATA, WEIGHT = "ganet_disp_conv_forward", "ganet_disp_conv_backward_data", "ganet_disp_conv_backward_weight"
    calls, call = [], api.call
    monkeypatch.setattr(api, "call", lambda name, *a: (calls.append(name), call(name, *a))[1])
    conv = conv_of(MODEL, dev)
    op = DispConv(conv)
    x, g = dev.to(np.array(MODEL.x)), dev.to(np.array(MODEL.grad_y))[:, None]
    keep_x, keep_w = x.clone(), conv.weight.detach().clone()
    with torch.no_grad():
        quiet = op(x.clone().requires_grad_())
    assert not quiet.requires_grad and quiet.grad_fn is None and calls == [FWD]
    # both want a gradient
    del calls[:]
    xr = x.clone().requires_grad_()
    y = op(xr)
    assert torch.equal(y, quiet)
    y.backward(g)
    assert calls[0] == FWD and sorted(calls[1:]) == [DATA, WEIGHT] and xr.grad is not None and conv.weight.grad is not None
    # frozen weight: the weight gradient is never computed
    del calls[:]
    conv.requires_grad_(False)
    conv.weight.grad = None
    xr = x.clone().requires_grad_()
    op(xr).backward(g)
    assert calls == [FWD, DATA] and conv.weight.grad is None and xr.grad is not None
    # constant input: the data gradient is never computed
    del calls[:]
    conv.requires_grad_(True)
    y = op(x)
    assert y.requires_grad
    y.backward(g)
    assert calls == [FWD, WEIGHT] and x.grad is None and conv.weight.grad is not None
    # neither: nothing to differentiate
    del calls[:]
    conv.requires_grad_(False)
    plain = op(x)
    assert not plain.requires_grad and torch.equal(plain, quiet) and calls == [FWD]
    assert torch.equal(x, keep_x) and torch.equal(xr, keep_x) and torch.equal(conv.weight, keep_w)


def test_weight_gradient_is_bit_reproducible(api, dev):
    """two runs of the weight gradient give identical bits (no atomics: fixed-order partial rows, fixed-order fp64 sum); what
    the stock path does on the same input is printed beside it, not asserted"""
    import torch
    from ganet_amd.modules.fused import DispConv
    conv = conv_of(MODEL, dev)
    x, g = dev.to(np.array(MODEL.x)), dev.to(np.array(MODEL.grad_y))[:, None]
    runs = {}
    for name, op in (("DispConv", DispConv(conv)), ("conv3d", conv)):
        runs[name] = [torch.autograd.grad(op(x), conv.weight, g)[0] for _ in range(3)]
    print("stock weight gradient identical over three runs:", all(torch.equal(runs["conv3d"][0], t) for t in runs["conv3d"]))
    assert all(torch.equal(runs["DispConv"][0], t) for t in runs["DispConv"])


def test_no_host_synchronisation(api, dev):
    import torch
    from ganet_amd.modules.fused import DispConv
    conv = conv_of(MODEL, dev)
    op = DispConv(conv)
    forward_backward(op, conv, MODEL, dev)                   # first use: library load, allocator warm-up
    conv.weight.grad = None
    x, g = dev.to(np.array(MODEL.x)).requires_grad_(), dev.to(np.array(MODEL.grad_y))[:, None]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        y = op(x)
        y.backward(g)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    dc.check(MODEL, {"y": host(y)[:, 0], "grad_x": host(x.grad), "grad_weight": host(conv.weight.grad)[0]}, verbose=False)


def _fresh(dev, case, seed):
    rng = np.random.default_rng(seed)
    N, C, D, H, W = case.shape
    return dev.to(rng.standard_normal(case.shape).astype(F32)), dev.to(rng.standard_normal((N, 1, D, H, W)).astype(F32))


def test_graph_capture_and_replay(api, dev):
    """forward + both gradients captured once and replayed on new data: bit-equal to the eager call"""
    import torch
    from ganet_amd.modules.fused import DispConv
    conv = conv_of(ALIGNED, dev)
    op = DispConv(conv)
    x, g = _fresh(dev, ALIGNED, 1)
    x.requires_grad_()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            torch.autograd.grad(op(x), (x, conv.weight), g)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = op(x)
        gx, gw = torch.autograd.grad(y, (x, conv.weight), g)
    for seed in (2, 3):
        nx, ng = _fresh(dev, ALIGNED, seed)
        with torch.no_grad():
            x.copy_(nx), g.copy_(ng)
        graph.replay()
        torch.cuda.synchronize()
        ey = op(x)
        egx, egw = torch.autograd.grad(ey, (x, conv.weight), g)
        assert torch.equal(y, ey) and torch.equal(gx, egx) and torch.equal(gw, egw) and bool(torch.isfinite(gw).all())


def test_side_stream(api, dev):
    """the launches go to the current stream, whichever it is"""
    import torch
    from ganet_amd.modules.fused import DispConv
    conv = conv_of(ALIGNED, dev)
    op = DispConv(conv)
    x, g = dev.to(np.array(ALIGNED.x)).requires_grad_(), dev.to(np.array(ALIGNED.grad_y))[:, None]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        y = op(x)
        gx, gw = torch.autograd.grad(y, (x, conv.weight), g)
    side.synchronize()
    dc.check(ALIGNED, {"y": host(y)[:, 0], "grad_x": host(gx), "grad_weight": host(gw)[0]}, verbose=False)


# ---- harness.fuse.use_fused_disp_conv on stand-ins ---------------------------------------------------------------------------

def stand_in(maxdisp):
    """the reference's Disp and DispAgg (models/GANet_deep.py:203-247 is not on a test machine: restated here by what the
    rebinders read -- the class names, maxdisp and conv32x1 -- and by their forwards; DispAgg's guided tail is left out of the
    stock forward, which use_fused_ops would replace anyway: the stand-in for it is only ever run on the stock path or under
    use_fused_disp_conv alone)"""
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

    class DispAgg(Disp):
        pass

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.disp0 = Disp()
            self.disp2 = DispAgg()

        def forward(self, x):
            return self.disp0(x), self.disp2(x)

    torch.manual_seed(33)
    return Net().cuda()


def test_use_fused_disp_conv_on_stand_ins(api, dev):
    """Conv3d(32,1,3) + a tail, stock and rebound: alone, after use_fused_ops and after use_fused_disp_tail (the two forms that
    replace Disp's tail).  The bars: DispTail's statement (tests/disp_tail_ref64.py) at each form's own convolution output c
    (read by a forward hook) gives out, grad_c and their bounds; c itself is held to DispConv's statement of the input.  The
    weight gradient is the correlation of the input with grad_c: the bound of grad_c passes through it with |input|, and
    DispConv's own summation adds its bound L u corr(|input|, |grad_c|).  Twice that, as everywhere."""
    import torch
    import disp_tail_ref64 as tail_ref
    from harness import fuse
    N, D, H, W = 2, 5, 4, 6
    size = (13, 3 * H, 3 * W)
    stock = stand_in(size[0] - 1)
    keys = list(stock.state_dict())
    rng = np.random.default_rng(34)
    inp_np = (0.2 * rng.standard_normal((N, 32, D, H, W))).astype(F32)
    g_np = rng.standard_normal((N,) + size[1:]).astype(F32)
    inp, g = dev.to(inp_np), dev.to(g_np)

    def build(order):
        m = copy.deepcopy(stock)
        del m.disp2                                            # (the DispAgg stand-in has no guided tail to fuse)
        for step in order:
            if step == "conv":
                assert fuse.use_fused_disp_conv(m) == 1
            elif step == "ops":
                assert fuse.use_fused_ops(m) == 1
            else:
                assert fuse.use_fused_disp_tail(m) == 1
        return m

    both = copy.deepcopy(stock)
    assert fuse.use_fused_disp_conv(both) == 2 and list(both.state_dict()) == keys
    assert both.disp2.conv32x1._fused_conv.conv.weight is both.disp2.conv32x1.weight
    forms = {"stock": (build(()), "disp0"), "alone": (build(("conv",)), "disp0"), "after use_fused_ops": (build(("ops", "conv")), "disp0"),
             "after use_fused_disp_tail": (build(("tail", "conv")), "disp0"),
             "before use_fused_disp_tail": (build(("conv", "tail")), "disp0"), "DispAgg alone": (both, "disp2")}
    res = {}
    for name, (model, site) in forms.items():
        assert list(model.state_dict()) == [k for k in keys if model is both or k.startswith("disp0.")]
        tail = getattr(model, site)
        conv = tail.conv32x1
        seen = []
        hook = conv.register_forward_hook(lambda mod, args, y: seen.append(y.detach()))
        model.zero_grad()
        out = tail(inp)
        out.backward(g)
        hook.remove()
        c = host(seen[0])[:, 0]                                  # this form's own convolution output
        st = tail_ref.Statement(c, size, g_np)
        cs = ref.Statement(inp_np, host(conv.weight), st.grad_x.astype(F32))
        with np.errstate(all="ignore"):
            r_c = float((np.abs(c - cs.y) / (2 * cs.b_y)).max())
            r_out = float((np.abs(host(out) - st.out) / (2 * st.b_out)).max())
            # grad_c in float64 against its fp32 rounding: one more u |grad_c| on the bound of grad_c
            want_gw = ref.backward_weight(inp_np.astype(np.float64), st.grad_x)
            bound_gw = (ref.backward_weight(np.abs(inp_np).astype(np.float64), st.b_grad_x + ref.U * np.abs(st.grad_x))
                        + cs.b_grad_weight)
            r_gw = float((np.abs(host(conv.weight.grad)[0] - want_gw) / (2 * bound_gw)).max())
        res[name] = (r_c, r_out, r_gw)
        print(f"{name}: worst error / bar  conv output {r_c:.3f}  out {r_out:.3f}  grad of the convolution weight {r_gw:.3f}")
    for name in forms:
        if name != "stock":
            assert max(res[name]) <= 1, (name, res[name])
    assert res["after use_fused_disp_tail"] == res["before use_fused_disp_tail"]
