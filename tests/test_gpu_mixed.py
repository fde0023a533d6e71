"""Mixed-precision inference on the gfx950 build: the case table of tests/mixed_cases.py through the C ABI (tests/test_sim_mixed.py
runs it on the emulator) -- the same inputs, the same yardstick without a tolerance: equality with the fp32 entry on the up-cast
input, rounded once -- and, device only, the modules against the cast arm (the fp32 op between ATen casts) and the whole model
under harness.steps.predict(..., amp=dtype): what harness.fuse.use_mixed_precision rebinds, which casts are left, and
kernels=True against kernels=False."""
import os
import sys

import numpy as np
import pytest

import mixed_cases as mc
from test_gpu_parity import TorchDev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMTS = [mc.F16, mc.BF16]
fmt_id = mc.FMT_NAME.get


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
    return {mc.F16: torch.float16, mc.BF16: torch.bfloat16, mc.F32: torch.float32}[fmt]


def bits(t):
    import torch
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b):
    import torch
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


# ---- C ABI: the shared table ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
def test_cast_16_to_32_every_pattern(api, dev, fmt):
    mc.check_cast(api, dev, np.arange(65536, dtype=np.uint32).astype(np.uint16), fmt, mc.F32)


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
def test_cast_32_to_16_table(api, dev, fmt):
    mc.check_cast(api, dev, mc.conversion_table(fmt), mc.F32, fmt)


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
def test_cast_sizes_and_bases(api, dev, fmt):
    table = mc.conversion_table(fmt)
    for n in mc.CAST_SIZES:
        mc.check_cast(api, dev, np.resize(table, n), mc.F32, fmt)
        mc.check_cast(api, dev, mc.convert(np.resize(table, n), fmt), fmt, mc.F32)
    for so, do in mc.CAST_OFFSETS:
        mc.check_cast(api, dev, table[:1027], mc.F32, fmt, src_off=so, dst_off=do)
        mc.check_cast(api, dev, mc.convert(table[:1027], fmt), fmt, mc.F32, src_off=so, dst_off=do)


def test_cast_copies_and_across_formats(api, dev):
    every = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    mc.check_cast(api, dev, mc.conversion_table(mc.BF16), mc.F32, mc.F32)
    for fmt in FMTS:
        mc.check_cast(api, dev, every, fmt, fmt)
        mc.check_cast(api, dev, every[:4099], fmt, fmt, src_off=1, dst_off=3)
    mc.check_cast(api, dev, every, mc.F16, mc.BF16)
    mc.check_cast(api, dev, every, mc.BF16, mc.F16)


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
@pytest.mark.parametrize("case", mc.BN_CASES, ids=repr)
def test_bn_apply_mixed(api, dev, case, fmt):
    mc.check_bn(api, dev, case, fmt)


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
@pytest.mark.parametrize("case", mc.CV_CASES, ids=repr)
def test_cost_volume_16(api, dev, case, fmt):
    mc.check_cv(api, dev, case, fmt)


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
@pytest.mark.parametrize("case", mc.L1_CASES, ids=repr)
def test_l1_normalize_mixed(api, dev, case, fmt):
    mc.check_l1(api, dev, case, fmt)


def test_bad_arguments(api, dev):
    mc.check_bad_arguments(api, dev)


# ---- functions and modules against the cast arm -----------------------------------------------------------------------------

def _bn(torch, dims, C, affine, seed=0):
    g = torch.Generator().manual_seed(seed)
    bn = (torch.nn.BatchNorm2d if dims == 2 else torch.nn.BatchNorm3d)(C, affine=affine)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(C, generator=g))
        bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
        if affine:
            bn.weight.copy_(torch.randn(C, generator=g))
            bn.bias.copy_(torch.randn(C, generator=g))
    return bn.cuda().eval()


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("dims", [2, 3], ids=["bn2d", "bn3d"])
def test_mixed_bn_relu_equals_the_cast_arm(api, dims, affine, fmt):
    """MixedBnRelu == BnRelu on the up-cast input followed by .to(): every relu x rem x out_dtype, in place, and the fold
    follows a train-mode forward of the BatchNorm in between"""
    import torch
    from ganet_amd.modules.fused import BnRelu
    from ganet_amd.modules.mixed import MixedBnRelu
    dt = tdtype(fmt)
    shape = (2, 5, 6, 12) if dims == 2 else (2, 5, 3, 4, 10)                  # S = 72 (a multiple of 8), 120
    torch.manual_seed(3)
    bn = _bn(torch, dims, shape[1], affine)
    x = (torch.randn(shape, device="cuda") * 2).to(dt)
    rems = {"none": None, "f32": torch.randn(shape, device="cuda"), "16": torch.randn(shape, device="cuda").to(dt)}

    def both(relu, rem, out):
        with torch.no_grad():
            want = BnRelu(bn, relu=relu, inplace=False)(x.float(), rem.float() if rem is not None else None).to(out or dt)
            got = MixedBnRelu(bn, relu=relu, out_dtype=out, inplace=False)(x, rem)
        return got, want

    for relu in (True, False):
        for kind, rem in rems.items():
            for out in (None, torch.float32):
                got, want = both(relu, rem, out)
                assert same_bits(got, want), (relu, kind, out)
    with torch.no_grad():                                                     # an fp32 x with a 16-bit output
        for kind in ("none", "f32"):
            x32 = torch.randn(shape, device="cuda") * 2
            rem = rems[kind]
            want = BnRelu(bn, inplace=False)(x32, rem).to(dt)
            assert same_bits(MixedBnRelu(bn, out_dtype=dt)(x32, rem), want), kind
        with pytest.raises(TypeError):
            MixedBnRelu(bn)(x32)                                              # fp32 to fp32 is BnRelu's
    with torch.no_grad():                                                     # in place: y IS x
        xc = x.clone()
        y = MixedBnRelu(bn)(xc, rems["f32"])
        assert y.data_ptr() == xc.data_ptr() and same_bits(y, both(True, rems["f32"], None)[1])
        before = both(True, None, None)[1]
        bn.train()
        bn(torch.randn(shape, device="cuda") * 3 + 1)                         # the running statistics move
        bn.eval()
        got, want = both(True, None, None)
        assert same_bits(got, want) and not same_bits(want, before)


def test_mixed_bn_relu_in_a_captured_graph(api):
    import torch
    from ganet_amd.modules.mixed import MixedBnRelu
    torch.manual_seed(4)
    bn = _bn(torch, 3, 4, True)
    op = MixedBnRelu(bn, out_dtype=torch.float32, inplace=False)
    xs = torch.randn(2, 4, 3, 4, 8, device="cuda").bfloat16()
    rem = torch.randn(2, 4, 3, 4, 8, device="cuda")
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            op(xs, rem)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = op(xs, rem)
        xs.copy_(torch.randn(2, 4, 3, 4, 8, device="cuda").bfloat16())
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(y, op(xs, rem))


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
def test_functions_equal_the_cast_arm(api, fmt):
    import torch
    from ganet_amd.functions import fused, mixed
    from ganet_amd.modules.GANet import GetCostVolume
    from ganet_amd.modules.mixed import MixedGetCostVolume
    dt = tdtype(fmt)
    torch.manual_seed(5)
    with torch.no_grad():
        g = torch.randn(2, 40, 6, 10, device="cuda").to(dt)
        for a, b in zip(mixed.normalize_guidance_mixed(g, 2), fused.normalize_guidance(g.float(), 2)):
            assert same_bits(a, b)
        f = torch.randn(1, 75, 6, 10, device="cuda").to(dt)
        assert same_bits(mixed.normalize_filters_mixed(f), fused.normalize_filters(f.float()))
        x, y = (torch.randn(1, 4, 5, 16, device="cuda").to(dt) for _ in range(2))
        assert same_bits(MixedGetCostVolume(6)(x, y), GetCostVolume(6)(x.float(), y.float()).to(dt))
        v = torch.randn(3, 1001, device="cuda") * 100
        assert same_bits(mixed.cast(v, dt), v.to(dt)) and same_bits(mixed.cast(v.to(dt), torch.float32), v.to(dt).float())
        assert mixed.cast(v, torch.float32) is v
    with pytest.raises(TypeError):
        mixed.normalize_guidance_mixed(g.float(), 2)                          # fp32 is the existing op's
    with pytest.raises(TypeError):
        mixed.cost_volume_16(x, y.float(), 3)
    with pytest.raises(RuntimeError, match="no_grad"):
        mixed.cast(v.clone().requires_grad_(), dt)
    with pytest.raises(RuntimeError, match="contiguous"):
        mixed.cast(v.t(), dt)




# ---- the whole model ----------------------------------------------------------------------------------------------------------

def _log_casts(torch, params, min_numel, log):
    from torch.utils._python_dispatch import TorchDispatchMode

    class Log(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            out = func(*args, **(kwargs or {}))
            if func is torch.ops.aten._to_copy.default:
                src = args[0]
                if src.numel() > min_numel and src.data_ptr() not in params and out.dtype != src.dtype:
                    log.append((tuple(src.shape), src.dtype, out.dtype))
            return out

    return Log()


def _check_model(torch, build, label, fmt, n_sga, sga_channels, left, right, max_disp, conv32_logged):
    """What use_mixed_precision promises, on any model `build()` returns twice with the same weights: see the numbered
    comments.  conv32_logged: whether conv32x1's output is larger than one image plane (it is in the reference's models)."""
    from harness import fuse, steps
    dt = tdtype(fmt)
    Hh, Ww = left.shape[-2:]
    arms = {}
    for kernels in (True, False):
        m = build()
        keys = list(m.state_dict())
        fuse.use_mixed_precision(m, dt, kernels=kernels)
        assert list(m.state_dict()) == keys
        arms[kernels] = m
    model = arms[True]
    # 2. hooks: what every SGABlock and the cost volume see and return
    seen, produced, hooks = [], [], []
    for mod in model.modules():
        kind = type(mod).__name__
        if kind == "SGABlock":
            hooks.append(mod.register_forward_hook(lambda m_, a, out: seen.append((a[0], a[1].dtype, out.dtype))))
        elif kind == "BasicConv":
            hooks.append(mod.register_forward_hook(lambda m_, a, out: produced.append(out)))
        elif kind == "GetCostVolume":
            hooks.append(mod.register_forward_hook(lambda m_, a, out: seen.append(("cv", a[0].dtype, out.dtype))))
    # 3. every ATen cast of a tensor larger than one image plane (the weights, which autocast rounds once per pass, aside)
    log = []
    with _log_casts(torch, {p.data_ptr() for p in model.parameters()}, Hh * Ww, log):
        out = steps.predict(model, left, right, amp=dt)
    for h in hooks:
        h.remove()
    assert out.dtype == torch.float32 and out.shape == (left.shape[0], Hh, Ww) and bool(torch.isfinite(out).all())
    cv = [s for s in seen if s[0] == "cv"]
    blocks = [s for s in seen if s[0] != "cv"]
    assert cv == [("cv", dt, dt)] and len(blocks) == n_sga
    for x, g_dtype, out_dtype in blocks:
        assert x.dtype == torch.float32 and any(x is p for p in produced), "an SGABlock's x is its producing BasicConv's own output"
        assert g_dtype == dt and out_dtype == dt
    is_sga = lambda c: len(c[0]) == 5 and c[0][1] in sga_channels and c[1] == torch.float32 and c[2] == dt      # noqa: E731
    is_conv32 = lambda c: len(c[0]) == 5 and c[0][1] == 1 and c[1] == dt and c[2] == torch.float32            # noqa: E731
    assert all(is_sga(c) or is_conv32(c) for c in log), [c for c in log if not (is_sga(c) or is_conv32(c))]
    # the SGA outputs in front of conv_refine: one per block; conv32x1's output goes through ganet_cast, not ATen
    assert sum(map(is_sga, log)) == n_sga and sum(map(is_conv32, log)) == 0, log
    # the cast arm leaves the same two families and many more
    log_c = []
    with _log_casts(torch, {p.data_ptr() for p in arms[False].parameters()}, Hh * Ww, log_c):
        c1 = steps.predict(arms[False], left, right, amp=dt)
    assert len(log_c) > len(log) + n_sga
    assert sum(map(is_conv32, log_c)) == (1 if conv32_logged else 0)
    # 4. kernels=True against kernels=False
    c2 = steps.predict(arms[False], left, right, amp=dt)
    floor = float((c1 - c2).abs().max())
    diff = float((out - c1).abs().max())
    print(f"{label} {mc.FMT_NAME[fmt]}: kernels vs cast arm |dd|max {diff:.3e}; cast arm twice {floor:.3e}; "
          f"ATen casts left {len(log)} (cast arm {len(log_c)})")
    if floor == 0.0:
        assert torch.equal(out, c1)
    else:
        assert diff <= 4 * floor, (diff, floor)
    # 5. against the fp32 pass of the same model (autocast off: every site takes its fp32 way): recorded, not asserted -- with
    #    random weights it says nothing about accuracy
    d32 = steps.predict(model, left, right)
    dev_ = (out - d32).abs()
    print(f"{label} {mc.FMT_NAME[fmt]}: against the fp32 pass max |dd| {float(dev_.max()):.4f} mean {float(dev_.mean()):.5f} "
          f"(disparities in [0, {max_disp}], random weights)")
    assert bool(torch.isfinite(d32).all())
    # ... and that fp32 pass is the one use_fused_ops + use_fused_bn alone give: the rebinding changes nothing without autocast
    plain = build()
    fuse.use_fused_ops(plain)
    fuse.use_fused_bn(plain)
    p1, p2 = steps.predict(plain, left, right), steps.predict(plain, left, right)
    floor32 = float((p1 - p2).abs().max())               # (the rule of 4. again: equal where that arm repeats its own bits)
    assert torch.equal(d32, p1) if floor32 == 0.0 else float((d32 - p1).abs().max()) <= 4 * floor32


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
def test_stand_in_model_under_autocast(api, fmt):
    """use_mixed_precision end to end on the tiny network of tests/mixed_standin.py (three SGABlocks, a Conv2x, a DispAgg, the
    cost volume): needs no reference model code, so it runs wherever the suite runs"""
    import torch
    import mixed_standin as ms
    sys.path.insert(0, ROOT)
    torch.manual_seed(9)
    first = ms.GANet(12).cuda().eval()

    def build():
        m = ms.GANet(12).cuda().eval()
        m.load_state_dict(first.state_dict())
        return m

    left, right = torch.randn(1, 3, 24, 48, device="cuda"), torch.randn(1, 3, 24, 48, device="cuda")
    # a conv32x1 output of 5 * 8 * 16 elements is smaller than the 24 * 48 image plane: below the log's threshold here
    _check_model(torch, build, "stand-in", fmt, 3, (ms.C,), left, right, 12, conv32_logged=False)
    # composes with use_fused_disp_conv in either order: the DispConv hands the 16-bit input to its convolution
    from harness import fuse, steps
    outs = []
    for order in ((fuse.use_mixed_precision, fuse.use_fused_disp_conv), (fuse.use_fused_disp_conv, fuse.use_mixed_precision), (fuse.use_mixed_precision,)):
        m = build()
        for step in order:
            step(m)
        outs.append(steps.predict(m, left, right, amp=tdtype(fmt)))
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[2])


MAX_DISP, H, W = 48, 96, 192                                                  # the crop of tests/test_gpu_model.py, batch 1
N_SGA = {"GANet11": 4, "GANet_deep": 7}


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    sys.path.insert(0, ROOT)
    from harness import refmodel
    if not refmodel.available():
        pytest.skip("no reference model code (GANET_REF_ROOT, /root/reference or oracle/_ref/pyref)")
    return torch


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
@pytest.mark.parametrize("name", ["GANet11", "GANet_deep"])
def test_whole_model_under_autocast(env, api, name, fmt):
    """The reference's two models (needs their files, as tests/test_gpu_model.py does).  The deviation from the fp32 pass is
    printed, not asserted.  Where the model files are not available (the test skips, with the model tests of
    tests/test_gpu_model.py) the same checks run on the stand-in
    network above, and the sites of both real models are checked on the CPU by tests/test_mixed_cpu.py."""
    torch = env
    from harness import steps
    torch.manual_seed(7)
    stock = steps.build_model(name, MAX_DISP, "cuda")
    left, right, _ = steps.synthetic_batch(1, H, W, MAX_DISP, "cuda", seed=5)
    # 1. what the feature adds: without the rebinding the first GA op refuses the 16-bit tensor autocast hands it
    with pytest.raises(TypeError, match="fp32 only"):
        steps.predict(stock, left, right, amp=tdtype(fmt))

    def build():
        m = steps.build_model(name, MAX_DISP, "cuda")
        m.load_state_dict(stock.state_dict())
        return m

    _check_model(torch, build, name, fmt, N_SGA[name], (32, 48), left, right, MAX_DISP, conv32_logged=True)
