"""conv32x1 on a 16-bit x on the gfx950 build: the case table of tests/mixed_conv_cases.py through the C ABI
(tests/test_sim_mixed_conv.py runs it on the emulator) -- equality of bits with the fp32 entries on the up-cast x, and with the
float64 statement on the exact family -- and, device only: the weight gradient twice, a graph capture replayed on new data,
MixedDispConv's two arms, and harness.fuse.use_mixed_disp_conv at the model: one training step (bf16, and fp16 with a GradScaler)
and one inference pass of tests/standin_net.py, every conv32x1 site recorded and replayed through both arms."""
import numpy as np
import pytest

import mixed_cases as mc
import mixed_conv_cases as mcc
from test_gpu_parity import TorchDev

pytestmark = pytest.mark.gpu
fmt_id = mc.FMT_NAME.get
MODEL = mcc.by_name("C33-W8-H3-D9-N2")


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


def tdtype(fmt):
    import torch
    return torch.float16 if fmt == mc.F16 else torch.bfloat16


def bits(t):
    """the patterns of a tensor, on the host (no cast kernel: a view)"""
    import torch
    t = t.detach().contiguous()
    return t.view(torch.int16 if t.dtype != torch.float32 else torch.int32).cpu().numpy()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def half(dev, patterns, fmt, shape):
    return dev.to(np.ascontiguousarray(patterns).view(np.int16)).view(tdtype(fmt)).view(shape)


# ---- C ABI: the shared table --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", mcc.FMTS, ids=fmt_id)
@pytest.mark.parametrize("case", mcc.CASES, ids=repr)
def test_case(api, dev, case, fmt):
    mcc.check_case(api, dev, case, fmt)


@pytest.mark.parametrize("fmt", mcc.FMTS, ids=fmt_id)
def test_weight_gradient_twice_gives_the_same_bits(api, dev, fmt):
    a, b = (mcc.run(api, dev, MODEL, fmt, which=("16",))["16"]["grad_weight"] for _ in range(2))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_bad_arguments(api, dev):
    mcc.check_bad_arguments(api, dev)


# ---- the Function and the module ------------------------------------------------------------------------------------------------

def conv_of(case, fmt, dev):
    import torch
    conv = torch.nn.Conv3d(case.shape[1], 1, (3, 3, 3), (1, 1, 1), (1, 1, 1), bias=False).cuda()
    with torch.no_grad():
        conv.weight.copy_(dev.to(np.array(case.made(fmt)[1])))
    return conv


def arms(conv, x, g, directions=("forward", "data", "weight")):
    """(y, grad_x, grad_weight) of MixedDispConv on its kernels and on its cast arm"""
    import torch
    from ganet_amd.modules.mixed_conv import MixedDispConv
    out = []
    for kernels in (True, False):
        xr = x.detach().clone().requires_grad_()
        y = MixedDispConv(conv, directions, kernels=kernels)(xr)
        out.append((y,) + torch.autograd.grad(y, (xr, conv.weight), g))
    return out


@pytest.mark.parametrize("fmt", mcc.FMTS, ids=fmt_id)
@pytest.mark.parametrize("case", [MODEL, mcc.by_name("round-vec", "rounding")], ids=repr)
def test_module_kernels_equal_the_cast_arm(api, dev, case, fmt, monkeypatch):
    """MixedDispConv(kernels=True) and its cast arm give the same bits in all three directions, the 16-bit grad_x included; the
    kernels arm calls the three new entries and nothing else, an fp32 input goes to DispConv's"""
    import torch
    calls, call = [], api.call
    monkeypatch.setattr(api, "call", lambda name, *a: (calls.append(name), call(name, *a))[1])
    N, C, D, H, W = case.shape
    x16, w, g = case.made(fmt)
    conv = conv_of(case, fmt, dev)
    x, gy = half(dev, x16, fmt, case.shape), dev.to(np.array(g))[:, None]
    k, a = arms(conv, x, gy)
    assert k[0].dtype == torch.float32 and k[1].dtype == tdtype(fmt) and k[2].dtype == torch.float32
    for q, got, want in zip(mcc.QUANTITIES, k, a):
        assert got.dtype == want.dtype, q
        view = np.float32 if got.dtype == torch.float32 else np.uint16
        mc.assert_same(bits(got).view(view), bits(want).view(view), mc.F32 if view is np.float32 else fmt, f"{case.id} {q}")
    assert calls[0] == "ganet_disp_conv_forward_16" and sorted(calls[:3]) == sorted(n for n, _ in mcc.ENTRIES16)
    assert sorted(calls[3:]) == sorted(n[:-3] for n, _ in mcc.ENTRIES16)          # the cast arm: the fp32 entries
    del calls[:]
    from ganet_amd.modules.mixed_conv import MixedDispConv
    from ganet_amd.modules.fused import DispConv
    x32 = x.float()
    assert torch.equal(MixedDispConv(conv)(x32), DispConv(conv)(x32)) and calls == ["ganet_disp_conv_forward"] * 2


@pytest.mark.parametrize("fmt", mcc.FMTS, ids=fmt_id)
def test_graph_capture_and_replay(api, dev, fmt):
    """forward + both gradients captured once and replayed on new data: bit-equal to the eager call"""
    import torch
    from ganet_amd.functions.mixed_conv import DispConv16Function
    case = mcc.by_name("offset8")
    conv = conv_of(case, fmt, dev)
    N, C, D, H, W = case.shape

    def fresh(seed):
        rng = np.random.default_rng(seed)
        x16 = mc.convert(rng.standard_normal(case.shape).astype(np.float32), fmt)
        return half(dev, x16, fmt, case.shape), dev.to(rng.standard_normal((N, 1, D, H, W)).astype(np.float32))

    x, g = fresh(1)
    x.requires_grad_()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            torch.autograd.grad(DispConv16Function.apply(x, conv.weight), (x, conv.weight), g)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = DispConv16Function.apply(x, conv.weight)
        gx, gw = torch.autograd.grad(y, (x, conv.weight), g)
    for seed in (2, 3):
        nx, ng = fresh(seed)
        with torch.no_grad():
            x.copy_(nx), g.copy_(ng)
        graph.replay()
        torch.cuda.synchronize()
        ey = DispConv16Function.apply(x, conv.weight)
        egx, egw = torch.autograd.grad(ey, (x, conv.weight), g)
        assert same_bits(y, ey) and same_bits(gx, egx) and same_bits(gw, egw) and bool(torch.isfinite(gw).all())


# ---- at the model ---------------------------------------------------------------------------------------------------------------

H_IMG, W_IMG, MAXD = 48, 96, 48


def _sites(model):
    return [(k, m.conv32x1) for k, m in model.named_modules() if type(m).__name__ in ("Disp", "DispAgg")]


def _record(model, recs):
    """hooks on every conv32x1: x and y of each call, the gradient that reaches y and the one that leaves through x"""
    handles, open_recs = [], {}

    def pre(name):
        def hook(conv, args):
            rec = {"site": name, "conv": conv, "x": args[0].detach().clone(), "y": None, "gy": None, "gx": None}
            open_recs[name] = rec
            if not (torch_grad_enabled() and args[0].requires_grad):
                return None
            # x has other consumers, whose gradients autograd adds to this one: the convolution gets an alias of its own, and the
            # hook on the alias sees what comes back through the convolution alone
            alias = args[0].view_as(args[0])
            alias.register_hook(lambda g_, rec=rec: rec.__setitem__("gx", g_.detach().clone()))
            return (alias,)
        return hook

    def post(name):
        def hook(conv, args, out):
            rec = open_recs.pop(name)
            rec["y"] = out.detach().clone()
            if out.requires_grad:
                out.register_hook(lambda g_, rec=rec: rec.__setitem__("gy", g_.detach().clone()))
            recs.append(rec)
        return hook

    for name, conv in _sites(model):
        handles += [conv.register_forward_pre_hook(pre(name)), conv.register_forward_hook(post(name))]
    return handles


def torch_grad_enabled():
    import torch
    return torch.is_grad_enabled()


def _cast_log(torch, log):
    """every ATen cast of a [N,1,D,H,W] tensor: what would stand between conv32x1 and the tail"""
    from torch.utils._python_dispatch import TorchDispatchMode

    class Log(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            out = func(*args, **(kwargs or {}))
            if func is torch.ops.aten._to_copy.default and args[0].dim() == 5 and args[0].shape[1] == 1 and out.dtype != args[0].dtype:
                log.append((tuple(args[0].shape), args[0].dtype, out.dtype))
            return out

    return Log()


def _replay(torch, rec, dt, scale=1.0, train=True):
    """the recorded tensors of one site through both arms: equal bits, and equal to what the step itself produced"""
    conv = rec["conv"]
    # (a site behind an fp32 producer -- an SGABlock without refine -- sees fp32 and runs DispConv's kernels on both arms)
    assert rec["x"].dtype in (dt, torch.float32) and rec["y"].dtype == torch.float32, (rec["site"], rec["x"].dtype, rec["y"].dtype)
    if not train:
        from ganet_amd.modules.mixed_conv import MixedDispConv
        with torch.no_grad():
            yk, ya = (MixedDispConv(conv, kernels=k)(rec["x"]) for k in (True, False))
        assert same_bits(yk, ya) and same_bits(yk, rec["y"]), rec["site"]
        return
    assert rec["gy"] is not None and rec["gx"] is not None and rec["gy"].dtype == torch.float32 and rec["gx"].dtype == rec["x"].dtype, rec["site"]
    k, a = arms(conv, rec["x"], rec["gy"])
    for q, got, want in zip(("y", "grad_x", "grad_weight"), k, a):
        assert same_bits(got, want), (rec["site"], q)
    assert same_bits(k[0], rec["y"]) and same_bits(k[1], rec["gx"]), rec["site"]
    # (the scaler has divided the parameter's gradient by its scale, a power of two)
    assert torch.equal(conv.weight.grad * scale, k[2]), rec["site"]


@pytest.mark.parametrize("order", ["mixed-first", "conv-first"])
@pytest.mark.parametrize("fmt", mcc.FMTS, ids=fmt_id)
def test_stand_in_training_step(api, fmt, order):
    """one steps.train_step of tests/standin_net.py under use_mixed_precision_training + use_mixed_disp_conv, in either order"""
    import torch
    import standin_net
    from harness import fuse, steps
    dt = tdtype(fmt)
    left, right, target = steps.synthetic_batch(1, H_IMG, W_IMG, MAXD, "cuda", seed=5)
    m = standin_net.build(MAXD, "cuda")
    keys = list(m.state_dict())
    if order == "conv-first":
        assert fuse.use_mixed_disp_conv(m) == 3
    assert fuse.use_mixed_precision_training(m, dt) > 0
    if order == "mixed-first":
        assert fuse.use_mixed_disp_conv(m) == 3
    assert list(m.state_dict()) == keys
    scale = 256.0 if fmt == mc.F16 else 1.0
    scaler = torch.amp.GradScaler("cuda", init_scale=scale) if fmt == mc.F16 else None
    recs, log = [], []
    handles = _record(m, recs)
    with _cast_log(torch, log):
        loss, _ = steps.train_step(m, torch.optim.SGD(m.parameters(), lr=0.0), "GANet_deep", left, right, target, MAXD, steps.criterion(True),
                                   amp=dt, scaler=scaler)
    for h in handles:
        h.remove()
    assert bool(torch.isfinite(loss)) and len(recs) == 3 and {r["site"] for r in recs} == {k for k, _ in _sites(m)}
    assert log == [], log
    assert sum(rec["x"].dtype == dt for rec in recs) >= 2, "the 16-bit kernels were reached"
    for rec in recs:
        _replay(torch, rec, dt, scale)


@pytest.mark.parametrize("net", ["mixed_standin", "standin_net"])
@pytest.mark.parametrize("fmt", mcc.FMTS, ids=fmt_id)
def test_stand_in_inference_pass(api, fmt, net):
    """steps.predict under use_mixed_precision + use_mixed_disp_conv.  tests/mixed_standin.py: its DispAgg sits behind a refine
    SGABlock, as every tail of GANet_deep does, and meets 16 bits; tests/standin_net.py: its last SGABlock has no refine and hands
    fp32 on, which MixedDispConv runs on DispConv's kernels"""
    import torch
    from harness import fuse, steps
    dt = tdtype(fmt)
    torch.manual_seed(9)
    if net == "mixed_standin":
        import mixed_standin
        m, n = mixed_standin.GANet(12).cuda().eval(), 1
        left, right = torch.randn(1, 3, 24, 48, device="cuda"), torch.randn(1, 3, 24, 48, device="cuda")
    else:
        import standin_net
        m, n = standin_net.build(MAXD, "cuda").eval(), 3
        left, right, _ = steps.synthetic_batch(1, H_IMG, W_IMG, MAXD, "cuda", seed=5)
    keys = list(m.state_dict())
    assert fuse.use_mixed_precision(m, dt) > 0 and fuse.use_mixed_disp_conv(m) == n and list(m.state_dict()) == keys
    recs, log = [], []
    handles = _record(m, recs)
    with torch.no_grad(), _cast_log(torch, log):
        out = steps.predict(m, left, right, dt)
    for h in handles:
        h.remove()
    assert bool(torch.isfinite(out).all()) and len(recs) == 1 and log == [], log
    assert recs[0]["x"].dtype == (dt if net == "mixed_standin" else torch.float32)
    for rec in recs:
        _replay(torch, rec, dt, train=False)
