"""The fused BatchNorm + residual + ReLU on the gfx950 build: the case table of tests/bn_cases.py through the C ABI
(tests/test_sim_bn.py runs it on the emulator) -- same inputs, same float64 statement, same bars -- and, device only, through
ganet_amd.modules.fused.BnRelu: against the stock chain F.relu(bn(x) + rem) with both held to the float64 statement, mode
switching, no host synchronisation, graph capture, partial requires_grad, accumulation, and harness.fuse.use_fused_bn on a
stand-in for the reference model."""
import copy

import numpy as np
import pytest

import bn_cases as bc
from test_gpu_parity import TorchDev

pytestmark = pytest.mark.gpu
F32 = np.float32


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
    return None if t is None else t.detach().cpu().numpy()


# ---- C ABI: the shared table ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", bc.CASES, ids=repr)
def test_case(api, dev, case):
    bc.check(case, bc.run(api, dev, case))


@pytest.mark.parametrize("name", bc.REPRODUCIBLE)
def test_reproducible_whatever_the_workspace_held(api, dev, name):
    bc.check_reproducible(api, dev, bc.BY_NAME[name])


@pytest.mark.parametrize("pair", bc.nan_pairs(), ids=lambda p: p[1].name)
def test_nan(api, dev, pair):
    bc.check_nan_pair(api, dev, pair)


@pytest.mark.parametrize("want", bc.WANTED)
def test_null_outputs_are_not_computed(api, dev, want):
    case = bc.BY_NAME["odd-2x5x819-relu-rem"]
    bc.check(case, bc.run(api, dev, case, want=want), want=want)


@pytest.mark.parametrize("name", bc.EVAL_FORM)
@pytest.mark.parametrize("inplace", [False, True])
def test_eval_form(api, dev, name, inplace):
    bc.check_eval_form(api, dev, bc.BY_NAME[name], inplace)


def test_bad_arguments(api, dev):
    bc.check_bad_arguments(api, dev)


# ---- the module ------------------------------------------------------------------------------------------------------------

def make_bn(C, dims, seed=0, **kw):
    """a BatchNorm of the given dimensionality with non-trivial parameters and running statistics, on the device"""
    import torch
    rng = np.random.default_rng(seed)
    bn = (torch.nn.BatchNorm2d if dims == 2 else torch.nn.BatchNorm3d)(C, **kw)
    with torch.no_grad():
        if bn.affine:
            bn.weight.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, C).astype(F32) * np.where(np.arange(C) % 3 == 1, -1, 1).astype(F32)))
            bn.bias.copy_(torch.from_numpy(rng.normal(0, 0.5, C).astype(F32)))
        if bn.track_running_stats:
            bn.running_mean.copy_(torch.from_numpy(rng.normal(0, 1, C).astype(F32)))
            bn.running_var.copy_(torch.from_numpy(rng.uniform(0.5, 2, C).astype(F32)))
    return bn.cuda()


def step_case(bn, shape, seed, rem, relu=True):
    """a table case on the module's current parameters and running statistics: [N,C,*] flattened to [N,C,S], nudged off the
    ReLU kink like every case of the table"""
    N, C = shape[:2]
    c = bc.Case(f"module-{seed}", (N, C, int(np.prod(shape[2:]))), seed, relu=relu, rem=rem, weight=host(bn.weight), bias=host(bn.bias),
                momentum=bn.momentum, eps=bn.eps)
    c.running_mean, c.running_var, c._ref = host(bn.running_mean).copy(), host(bn.running_var).copy(), None
    assert int(c.ref.undecided().sum()) == 0
    return c


def forward_backward(op, bn, case, shape, dev):
    """one training step's forward + backward through `op(x, rem)`; the results in the layout bn_cases.check reads"""
    x = dev.to(case.x.reshape(shape)).requires_grad_()
    rem = dev.to(case.rem.reshape(shape)).requires_grad_() if case.rem is not None else None
    for p in bn.parameters():
        p.grad = None
    y = op(x, rem)
    y.backward(dev.to(case.gy.reshape(shape)))
    flat = lambda t: host(t).reshape(case.shape)   # noqa: E731
    got = {"y": flat(y), "grad_x": flat(x.grad), "grad_weight": host(bn.weight.grad), "grad_bias": host(bn.bias.grad),
           "running_mean": host(bn.running_mean), "running_var": host(bn.running_var)}
    if rem is not None:
        got["grad_rem"] = flat(rem.grad)
    return got


@pytest.mark.parametrize("shape", [(2, 6, 9, 13), (2, 3, 5, 6, 8)], ids=["2d", "3d"])
@pytest.mark.parametrize("rem", [False, True], ids=["plain", "rem"])
def test_module_against_the_stock_chain(api, dev, shape, rem):
    """three training steps of BnRelu(bn) and of F.relu(bn_copy(x) + rem) on the same data: each step's output, gradients
    (x, rem, weight, bias) and running statistics against the float64 statement -- ours by the bars, asserted; the stock
    kernels' distance in the same unit printed beside it: a measurement for profiles/, not asserted."""
    import torch
    import torch.nn.functional as F
    from ganet_amd.modules.fused import BnRelu
    ours = make_bn(shape[1], len(shape) - 2, seed=3)
    stock = copy.deepcopy(ours)
    fused = BnRelu(ours)
    chain = lambda x, r: F.relu(stock(x) if r is None else stock(x) + r)   # noqa: E731
    for k in range(3):
        case = step_case(ours, shape, 300 + k, rem)
        mine = bc.check(case, forward_backward(fused, ours, case, shape, dev), saved=False, verbose=False)
        case.running_mean, case.running_var, case._ref = host(stock.running_mean).copy(), host(stock.running_var).copy(), None
        theirs = bc.check(case, forward_backward(chain, stock, case, shape, dev), saved=False, verbose=False, enforce=False)
        print(f"step {k} {shape} rem={rem}: worst error / bar  " + "  ".join(f"{q} ours {mine[q]:.3f} stock {theirs[q]:.3f}" for q in mine))
        # the two modules' statistics may part by the bars' width from here on: each is held to its own recursion
    assert int(ours.num_batches_tracked) == int(stock.num_batches_tracked) == 3
    assert torch.allclose(ours.running_mean, stock.running_mean, rtol=1e-5, atol=1e-6)
    assert torch.allclose(ours.running_var, stock.running_var, rtol=1e-5, atol=1e-6)


def test_eval_after_train_uses_the_fresh_statistics(api, dev):
    """eval, one training forward, eval again with no optimiser step between: the second eval output is the fold of the
    running statistics the training forward has just written (a stale folded_bn pair would repeat the first)"""
    import torch
    from ganet_amd.functions.fused import BnApplyFunction
    from ganet_amd.modules.fused import BnRelu, folded_bn
    bn = make_bn(6, 2, seed=4)
    fused = BnRelu(bn)
    x = dev.to(np.random.default_rng(1).normal(0.5, 2, (2, 6, 9, 13)).astype(F32))
    bn.eval()
    with torch.no_grad():
        first = fused(x.clone())
    bn.train()
    fused(x)
    bn.eval()
    with torch.no_grad():
        second = fused(x.clone())
        scale, shift = folded_bn(bn, refresh=True)
        want = BnApplyFunction.apply(x.clone(), None, scale, shift, True, False)
        stock = torch.relu(bn(x))
    assert torch.equal(second, want) and not torch.equal(second, first)
    assert float((second - stock).abs().max()) <= 1e-5 * float(stock.abs().max())
    assert int(bn.num_batches_tracked) == 1


def test_eval_with_autograd(api, dev):
    """eval mode, frozen BatchNorm, an input that wants its gradient: one pass forward (not in place), the gradient of the
    folded affine behind the ReLU mask, for x and rem -- against autograd on the stock ops"""
    import torch
    from ganet_amd.modules.fused import BnRelu
    bn = make_bn(3, 3, seed=5).eval().requires_grad_(False)
    rng = np.random.default_rng(2)
    x_np, r_np = rng.normal(0, 1, (2, 3, 5, 6, 8)).astype(F32), rng.normal(0, 1, (2, 3, 5, 6, 8)).astype(F32)
    for relu in (True, False):
        stock = lambda x, r: torch.relu(bn(x) + r) if relu else bn(x) + r   # noqa: E731, B023
        outs = []
        for op in (BnRelu(bn, relu=relu), stock):
            x, r = dev.to(x_np).requires_grad_(), dev.to(r_np).requires_grad_()
            y = op(x, r)
            y.backward(torch.full_like(y, 0.5))
            assert np.array_equal(host(x), x_np)             # not in place: autograd is on
            outs.append((y.detach(), x.grad, r.grad))
        for a, b in zip(*outs):
            assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())


def test_no_host_synchronisation(api, dev):
    import torch
    from ganet_amd.modules.fused import BnRelu
    shape = (2, 6, 9, 13)
    bn = make_bn(6, 2, seed=6)
    fused = BnRelu(bn)
    case = step_case(bn, shape, 310, True)
    forward_backward(fused, bn, case, shape, dev)               # first use: library load, allocator warm-up
    case = step_case(bn, shape, 310, True)
    x = dev.to(case.x.reshape(shape)).requires_grad_()
    rem, gy = dev.to(case.rem.reshape(shape)).requires_grad_(), dev.to(case.gy.reshape(shape))
    for p in bn.parameters():
        p.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        y = fused(x, rem)
        y.backward(gy)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    got = {"y": host(y).reshape(case.shape), "grad_x": host(x.grad).reshape(case.shape), "grad_rem": host(rem.grad).reshape(case.shape),
           "grad_weight": host(bn.weight.grad), "grad_bias": host(bn.bias.grad), "running_mean": host(bn.running_mean),
           "running_var": host(bn.running_var)}
    bc.check(case, got, saved=False, verbose=False)


def test_graph_capture_and_replay(api, dev):
    """forward + backward captured once on a single stream and replayed on new data: bit-equal to the eager call"""
    import torch
    from ganet_amd.modules.fused import BnRelu
    shape = (2, 6, 9, 13)
    bn = make_bn(6, 2, seed=7)
    fused = BnRelu(bn)
    rng = np.random.default_rng(8)
    new = lambda: dev.to(rng.normal(0.3, 1.5, shape).astype(F32))   # noqa: E731
    x, rem, gy = new().requires_grad_(), new().requires_grad_(), new()
    params = [x, rem, bn.weight, bn.bias]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            y = fused(x, rem)
            grads = torch.autograd.grad(y, params, gy)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = fused(x, rem)
        grads = torch.autograd.grad(y, params, gy)
    for _ in range(2):
        with torch.no_grad():
            x.copy_(new()), rem.copy_(new()), gy.copy_(new())
        graph.replay()
        torch.cuda.synchronize()
        replayed = [t.clone() for t in (y,) + tuple(grads)]
        ye = fused(x, rem)
        eager = (ye,) + torch.autograd.grad(ye, params, gy)
        for a, b in zip(replayed, eager):
            assert torch.equal(a, b)
    assert int(bn.num_batches_tracked) == 2 + 2 + 2          # warm-up, two replays, two eager calls (capturing runs nothing)


def test_partial_requires_grad(api, dev, monkeypatch):
    """frozen weight and bias, and an x that wants no gradient: the backward entry gets NULL for what nobody asked for"""
    import torch
    from ganet_amd.modules.fused import BnRelu
    shape = (2, 6, 9, 13)
    bn = make_bn(6, 2, seed=9)
    fused = BnRelu(bn)
    seen, call = [], api.call

    def spy(name, *args):
        if name == "ganet_bn_train_backward":
            seen.append(tuple(a is not None for a in args[8:12]))      # grad_x, grad_rem, grad_weight, grad_bias
        return call(name, *args)

    monkeypatch.setattr(api, "call", spy)
    case = step_case(bn, shape, 320, True)
    for freeze, x_grad, rem_grad, want in ((True, True, True, (True, True, False, False)), (False, False, True, (False, True, True, True)),
                                           (False, False, False, (False, False, True, True)), (True, True, False, (True, False, False, False))):
        bn.requires_grad_(not freeze)
        x = dev.to(case.x.reshape(shape)).requires_grad_(x_grad)
        rem = dev.to(case.rem.reshape(shape)).requires_grad_(rem_grad)
        for p in bn.parameters():
            p.grad = None
        fused(x, rem).backward(dev.to(case.gy.reshape(shape)))
        assert seen[-1] == want, (seen[-1], want)
        assert (x.grad is not None) == x_grad and (rem.grad is not None) == rem_grad and (bn.weight.grad is not None) == (not freeze)
        got = {"y": None, "grad_x": x.grad, "grad_rem": rem.grad, "grad_weight": bn.weight.grad, "grad_bias": bn.bias.grad}
        r = case.ref
        for key, ref64, bar in (("grad_x", r.grad_x, r.bar_grad_x()), ("grad_weight", r.grad_weight, 2.0 ** -22 * r.invstd * r.sum_abs_gxm),
                                ("grad_bias", r.grad_bias, 2.0 ** -22 * r.sum_abs_g)):
            if got[key] is not None:
                bc.within(key, host(got[key]).reshape(ref64.shape), ref64, bar, verbose=False)
        if rem_grad:
            assert np.array_equal(host(rem.grad).reshape(case.shape), r.g.astype(F32))
    n = len(seen)
    frozen_x = dev.to(case.x.reshape(shape))
    bn.requires_grad_(False)
    assert not fused(frozen_x, None).requires_grad and len(seen) == n


def test_backward_twice_accumulates(api, dev):
    import torch
    from ganet_amd.modules.fused import BnRelu
    shape = (2, 3, 5, 6, 8)
    bn = make_bn(3, 3, seed=10)
    fused = BnRelu(bn)
    case = step_case(bn, shape, 330, True)
    x = dev.to(case.x.reshape(shape)).requires_grad_()
    rem, gy = dev.to(case.rem.reshape(shape)).requires_grad_(), dev.to(case.gy.reshape(shape))
    leaves = [x, rem, bn.weight, bn.bias]
    single = torch.autograd.grad(fused(x, rem), leaves, gy)
    for _ in range(2):
        fused(x, rem).backward(gy)
    for t, g in zip(leaves, single):
        assert torch.equal(t.grad, g + g)
    y = fused(x, rem)
    y.backward(gy, retain_graph=True)
    y.backward(gy)                                # the same graph twice: x, rem and the statistics are still saved
    for t, g in zip(leaves, single):
        assert torch.equal(t.grad, ((g + g) + g) + g)


# ---- harness.fuse.use_fused_bn on a stand-in -------------------------------------------------------------------------------

def stand_in():
    """the reference's BasicConv in two flavours (models/GANet_deep.py:15-41 is not on a test machine: restated here by what
    use_fused_bn reads -- the class name and conv / bn / relu / use_bn) and a three-layer module built from them"""
    import torch
    import torch.nn.functional as F

    def basic_conv(conv_cls, bn_cls):
        class BasicConv(torch.nn.Module):
            def __init__(self, cin, cout, bn=True, relu=True):
                super().__init__()
                self.relu, self.use_bn = relu, bn
                self.conv = conv_cls(cin, cout, 3, padding=1, bias=False)
                self.bn = bn_cls(cout)

            def forward(self, x):
                x = self.conv(x)
                if self.use_bn:
                    x = self.bn(x)
                if self.relu:
                    x = F.relu(x, inplace=True)
                return x
        return BasicConv

    conv2d, conv3d = basic_conv(torch.nn.Conv2d, torch.nn.BatchNorm2d), basic_conv(torch.nn.Conv3d, torch.nn.BatchNorm3d)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = conv2d(4, 6)                          # bn + relu
            self.b = conv3d(1, 3, relu=False)              # bn only
            self.c = conv3d(3, 2, bn=False)                # no bn: left alone

        def forward(self, x):
            return self.c(self.b(self.a(x).unsqueeze(1)))  # [N,6,H,W] -> [N,1,6,H,W] -> [N,3,6,H,W] -> [N,2,6,H,W]

    torch.manual_seed(21)
    net = Net()
    with torch.no_grad():
        for m in (net.a, net.b):
            m.bn.weight.uniform_(0.5, 1.5)
            m.bn.bias.normal_(0, 0.3)
    return net.cuda()


def test_use_fused_bn_on_a_stand_in(api, dev):
    """rebound call sites, unchanged state_dict keys, one training step against the unfused copy, and the eval output.
    The step's bound: both fp32 models are held to the float64 twin of the stand-in (the same modules in double).  Along the
    chain conv (fan-in K <= 36 fp32 products: K 2^-24) -> BnRelu (2^-21 of the terms, tests/bn_cases.py) -> conv (K = 27)
    -> BnRelu -> conv (K = 81) -> mean of squares, every stage's relative error is at most 2^-17.6 (the widest convolution),
    the BatchNorm divides by a batch deviation of order one and no stage cancels (the loss is a sum of squares), so the sum
    over the five stages and their backward twins stays below 10 x 2^-17 = 2^-13.7 of the largest entry of each tensor; the
    stock model's own distance is printed beside ours."""
    import torch
    from harness import fuse
    stock = stand_in()
    fused, twin = copy.deepcopy(stock), copy.deepcopy(stock).double().cpu()
    assert fuse.use_fused_bn(fused) == 2
    assert list(fused.state_dict()) == list(stock.state_dict())
    assert "_fused_bn" in fused.a.__dict__ and fused.a._fused_bn.relu and not fused.b._fused_bn.relu and "_fused_bn" not in fused.c.__dict__
    x = dev.to(np.random.default_rng(22).normal(0, 1, (2, 4, 10, 12)).astype(F32))
    res = []
    for model, inp in ((twin, x.double().cpu()), (stock, x), (fused, x)):
        loss = (model(inp) ** 2).mean()
        loss.backward()
        res.append((float(loss.detach()), {n: p.grad.double().cpu() for n, p in model.named_parameters() if p.grad is not None}))
    bound = 10 * 2.0 ** -17
    (l64, g64), (ls, gs), (lf, gf) = res
    print(f"loss: float64 {l64!r} stock {ls!r} fused {lf!r}; bound {bound * l64:.3e}")
    assert abs(lf - l64) <= bound * l64
    for n in g64:
        top = float(g64[n].abs().max())
        ef, es = float((gf[n] - g64[n]).abs().max()), float((gs[n] - g64[n]).abs().max())
        print(f"{n}: |grad - float64| / max|grad|  fused {ef / top:.3e} stock {es / top:.3e} bound {bound:.3e}")
        assert ef <= bound * top, n
    assert set(gf) == set(g64) and len(g64) == 7               # three convolutions, two BatchNorms in use
    for a, b in zip(fused.buffers(), stock.buffers()):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6) if a.is_floating_point() else torch.equal(a, b)
    stock.eval(), fused.eval()
    with torch.no_grad():
        want, got = stock(x), fused(x)
    assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())


def test_use_fused_bn_replaces_the_tail_of_use_fused_ops(api):
    """an SGABlock whose tail use_fused_ops has rebound gets a BnRelu on the same BatchNorm, with the same call form"""
    import torch
    from ganet_amd.modules.fused import BnRelu, ResidualBnRelu
    from harness import fuse

    class SGABlock(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.bn = torch.nn.BatchNorm3d(2)

    blk = SGABlock().cuda()
    assert fuse.use_fused_bn(blk) == 0                       # no tail to replace: use_fused_ops has not run
    object.__setattr__(blk, "_fused_tail", ResidualBnRelu(blk.bn))
    assert fuse.use_fused_bn(blk) == 1 and isinstance(blk._fused_tail, BnRelu) and blk._fused_tail.bn is blk.bn
    t, rem = torch.randn(2, 2, 3, 4, 5, device="cuda"), torch.randn(2, 2, 3, 4, 5, device="cuda")
    ref = copy.deepcopy(blk.bn)
    got, want = blk._fused_tail(t, rem), torch.relu(ref(t) + rem)
    assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())
    assert list(blk.state_dict()) == list(SGABlock().state_dict())
