"""Mixed-precision training on the gfx950 build: the case table of tests/mixed_train_cases.py through the C ABI
(tests/test_sim_mixed_train.py runs it on the emulator; what is checked and why is in the table's docstring) and, device only,
the autograd Functions and modules against their cast arm -- the fp32 op between ATen casts, which is what the same training step
costs without these kernels."""
import numpy as np
import pytest

import bn_cases as bc
import mixed_cases as mc
import mixed_train_cases as mt
from test_gpu_parity import TorchDev

pytestmark = pytest.mark.gpu
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


def tier(t):
    return [c for c in mt.BN_TRAIN_CASES if c.tier == t]


# ---- C ABI: the shared table ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
@pytest.mark.parametrize("case", tier("exact"), ids=repr)
def test_bn_train_exact(api, dev, case, fmt):
    for site in case.sites:
        for relu in case.relus:
            if fmt == mc.BF16 and relu:
                mt.check_fp32_twins_agree(api, dev, case.data(fmt, site, relu))
            mt.check_exact(api, dev, case, fmt, site, relu)


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
@pytest.mark.parametrize("case", tier("general"), ids=repr)
def test_bn_train_general(api, dev, case, fmt):
    for site in case.sites:
        for relu in case.relus:
            mt.check_general(api, dev, case, fmt, site, relu)


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
@pytest.mark.parametrize("case", tier("special"), ids=repr)
def test_bn_train_nan_inf_negative_zero(api, dev, case, fmt):
    for site in case.sites:
        for relu in case.relus:
            mt.check_special(api, dev, case, fmt, site, relu)


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
@pytest.mark.parametrize("name", mt.WANTED_CASES)
def test_bn_train_null_outputs(api, dev, name, fmt):
    case = mt.BN_BY_NAME[name]
    for want in bc.WANTED:
        for site in case.sites:
            mt.check_exact(api, dev, case, fmt, site, True, want=want)


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
@pytest.mark.parametrize("name", mt.REPRODUCIBLE)
def test_bn_train_two_runs_are_bit_identical(api, dev, name, fmt):
    mt.check_reproducible(api, dev, mt.BN_BY_NAME[name], fmt)


def test_bn_train_bad_arguments(api, dev):
    mt.check_bn_bad_arguments(api, dev)


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
@pytest.mark.parametrize("case", mt.CV_BWD_CASES, ids=repr)
def test_cost_volume_backward_16(api, dev, case, fmt):
    mt.check_cv_bwd(api, dev, case, fmt)


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
@pytest.mark.parametrize("case", mt.L1_BWD_CASES, ids=repr)
def test_l1_normalize_backward_mixed(api, dev, case, fmt):
    mt.check_l1_bwd(api, dev, case, fmt)


def test_misc_bad_arguments(api, dev):
    mt.check_misc_bad_arguments(api, dev)


# ---- functions and modules against the cast arm -----------------------------------------------------------------------------

def tdtype(fmt):
    import torch
    return {mc.F16: torch.float16, mc.BF16: torch.bfloat16, mc.F32: torch.float32}[fmt]


def bits(t):
    import torch
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b):
    import torch
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def _site(torch, fmt, site, tier_name="odd-2x5x819-exact", vol=(7, 9, 13)):
    """a BatchNorm3d and the tensors of one site, from the table's exact tier (so that kernel and cast arm owe the same bits)"""
    case = mt.BN_BY_NAME[tier_name]
    c = case.data(fmt, site, True)
    N, C, S = c.shape
    assert int(np.prod(vol)) == S
    bn = torch.nn.BatchNorm3d(C).cuda().train()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(c.weight)), bn.bias.copy_(torch.from_numpy(c.bias))
        bn.running_mean.copy_(torch.from_numpy(c.running_mean)), bn.running_var.copy_(torch.from_numpy(c.running_var))
    dt, ydt = tdtype(fmt), (tdtype(fmt) if mt.SITES[site][1] == "16" else torch.float32)
    x = torch.from_numpy(c.x).cuda().to(dt).reshape(N, C, *vol)
    rem = torch.from_numpy(c.rem).cuda().reshape(N, C, *vol) if c.rem is not None else None
    gy = torch.from_numpy(c.gy).cuda().to(ydt).reshape(N, C, *vol)
    assert torch.equal(x.float().cpu().reshape(c.shape), torch.from_numpy(c.x))
    return c, bn, x, rem, gy, ydt


def _run_site(torch, op, bn, x, rem, gy, sync_check=False):
    import copy
    bn = copy.deepcopy(bn)
    op = op(bn)
    x = x.clone().requires_grad_()
    rem = rem.clone().requires_grad_() if rem is not None else None
    torch.cuda.synchronize()
    if sync_check:
        torch.cuda.set_sync_debug_mode("error")
    try:
        y = op(x, rem) if rem is not None else op(x)
        y.backward(gy)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return {"y": y.detach(), "grad_x": x.grad, "grad_rem": rem.grad if rem is not None else None, "grad_weight": bn.weight.grad,
            "grad_bias": bn.bias.grad, "running_mean": bn.running_mean, "running_var": bn.running_var,
            "nbt": bn.num_batches_tracked}, bn, op


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
@pytest.mark.parametrize("site", list(mt.SITES))
def test_module_against_cast_arm_and_float64(api, fmt, site):
    """MixedTrainBnRelu against the cast arm (BnRelu on .float() inputs, .to(dtype) behind) on exact-tier data: the same bits in
    y, every gradient and the running buffers; both inside the float64 statement's bars; no host synchronisation; the running
    buffers and num_batches_tracked move exactly once"""
    import torch
    from ganet_amd.modules.mixed import MixedTrainBnRelu
    from harness.fuse import _CastArmBnRelu
    c, bn, x, rem, gy, ydt = _site(torch, fmt, site)
    out_dtype = torch.float32 if ydt == torch.float32 else None
    _run_site(torch, lambda b: MixedTrainBnRelu(b, out_dtype=out_dtype), bn, x, rem, gy)            # first use: library load
    k, kbn, _ = _run_site(torch, lambda b: MixedTrainBnRelu(b, out_dtype=out_dtype), bn, x, rem, gy, sync_check=True)
    a, abn, _ = _run_site(torch, lambda b: _CastArmBnRelu(b, True, out_dtype), bn, x, rem, gy)
    for key in k:
        if k[key] is not None and key != "nbt":
            assert same_bits(k[key], a[key]), key
    assert int(k["nbt"]) == 1 and int(a["nbt"]) == 1 and k["y"].dtype == ydt and k["grad_x"].dtype == x.dtype
    r = c.ref
    host = lambda t: t.detach().float().cpu().numpy()                                               # noqa: E731
    for arm in (k, a):
        bc.within("grad_weight", host(arm["grad_weight"]), r.grad_weight, 2.0 ** -22 * r.invstd * r.sum_abs_gxm, False)
        bc.within("grad_bias", host(arm["grad_bias"]), r.grad_bias, 2.0 ** -22 * r.sum_abs_g, False)
        m = r.m
        bc.within("running_mean", host(arm["running_mean"]), r.running_mean, 2.0 ** -22 * ((1 - m) * np.abs(r.old_mean) + m * np.abs(r.mean)), False)
        bc.within("running_var", host(arm["running_var"]), r.running_var, 2.0 ** -22 * ((1 - m) * np.abs(r.old_var) + m * np.abs(r.new_var)), False)
        gx = host(arm["grad_x"]).reshape(c.shape)
        bc.within("grad_x", gx, r.grad_x, r.bar_grad_x() + mt.half_ulp(np.abs(r.grad_x) + r.bar_grad_x(), fmt), False)
        yfmt = fmt if ydt != torch.float32 else mc.F32
        bar = r.bar_y() + (mt.half_ulp(np.abs(r.y) + r.bar_y(), fmt) if yfmt != mc.F32 else 0.0)
        bc.within("y", host(arm["y"]).reshape(c.shape), r.y, bar, False)


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
def test_module_autograd_properties(api, fmt):
    """partial requires_grad, accumulation into .grad, backward twice with retain_graph, eval after train, momentum=None"""
    import copy
    import torch
    from ganet_amd.modules.mixed import MixedBnRelu, MixedTrainBnRelu
    c, bn, x, rem, gy, _ = _site(torch, fmt, "tail")
    full, _, _ = _run_site(torch, MixedTrainBnRelu, bn, x, rem, gy)
    # x and rem want nothing: the parameter gradients alone, the same bits
    b2 = copy.deepcopy(bn)
    y = MixedTrainBnRelu(b2)(x, rem)
    y.backward(gy)
    assert same_bits(b2.weight.grad, full["grad_weight"]) and same_bits(b2.bias.grad, full["grad_bias"])
    # only x wants one, the parameters frozen
    b3 = copy.deepcopy(bn).requires_grad_(False)
    x3 = x.clone().requires_grad_()
    MixedTrainBnRelu(b3)(x3, rem).backward(gy)
    assert same_bits(x3.grad, full["grad_x"]) and b3.weight.grad is None
    # backward twice with retain_graph accumulates: g + g is exact
    b4 = copy.deepcopy(bn)
    x4 = x.clone().requires_grad_()
    y4 = MixedTrainBnRelu(b4)(x4, rem)
    y4.backward(gy, retain_graph=True)
    y4.backward(gy)
    assert torch.equal(b4.weight.grad, 2 * full["grad_weight"]) and torch.equal(x4.grad.float(), 2 * full["grad_x"].float())
    assert int(b4.num_batches_tracked) == 1
    # eval after train: MixedBnRelu's fold of the statistics the training pass left, its bits
    b4.eval()
    with torch.no_grad():
        assert same_bits(MixedTrainBnRelu(b4)(x, rem), MixedBnRelu(b4, inplace=False)(x, rem))
    b5 = copy.deepcopy(bn)
    b5.momentum = None
    with pytest.raises(RuntimeError, match="momentum=None"):
        MixedTrainBnRelu(b5)(x, rem)


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
def test_functions_against_cast_arm(api, fmt):
    """cost volume, both normalisations and the cast: forward and backward bits of the cast arm, without a host synchronisation"""
    import torch
    from ganet_amd.functions import mixed_train as F
    from ganet_amd.functions.fused import normalize_filters, normalize_guidance
    from ganet_amd.modules.GANet import GetCostVolume
    dt = tdtype(fmt)
    g = torch.Generator(device="cuda").manual_seed(3)
    rnd = lambda *s, d=dt: torch.randn(*s, device="cuda", generator=g).to(d)                        # noqa: E731
    x, y, gc = rnd(2, 3, 5, 16), rnd(2, 3, 5, 16), rnd(2, 6, 7, 5, 16)
    gd, ggs = rnd(1, 40, 7, 9), [rnd(1, 2, 5, 7, 9, d=torch.float32) for _ in range(4)]
    lf, glf = rnd(1, 75, 6, 10), rnd(1, 75, 6, 10, d=torch.float32)
    small, gsmall = rnd(1, 1, 5, 6, 10), rnd(1, 1, 5, 6, 10, d=torch.float32)

    def kernels():
        a, b = x.clone().requires_grad_(), y.clone().requires_grad_()
        F.CostVolume16Function.apply(a, b, 7).backward(gc)
        q = gd.clone().requires_grad_()
        ks = F.NormalizeGuidanceMixedFunction.apply(q, 2)
        torch.autograd.backward(ks, ggs)
        f = lf.clone().requires_grad_()
        nf = F.NormalizeFiltersMixedFunction.apply(f)
        nf.backward(glf)
        s = small.clone().requires_grad_()
        up = F.CastFunction.apply(s, torch.float32)
        up.backward(gsmall)
        return [a.grad, b.grad, q.grad, f.grad, s.grad, nf.detach(), up.detach()] + [k.detach() for k in ks]

    def cast_arm():
        a, b = x.clone().requires_grad_(), y.clone().requires_grad_()
        GetCostVolume(6)(a.float(), b.float()).to(dt).backward(gc)
        q = gd.clone().requires_grad_()
        ks = normalize_guidance(q.float(), 2)
        torch.autograd.backward(ks, ggs)
        f = lf.clone().requires_grad_()
        nf = normalize_filters(f.float())
        nf.backward(glf)
        s = small.clone().requires_grad_()
        up = s.float()
        up.backward(gsmall)
        return [a.grad, b.grad, q.grad, f.grad, s.grad, nf.detach(), up.detach()] + [k.detach() for k in ks]

    kernels()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = kernels()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for i, (a, b) in enumerate(zip(got, cast_arm())):
        assert same_bits(a, b), i


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
def test_graph_capture_and_replay(api, fmt):
    """forward + backward of every Function -- the three BatchNorm sites, the cost volume, both normalisations and the cast --
    captured once and replayed on new data: the eager call's bits"""
    import torch
    from ganet_amd.functions import mixed_train as F
    from ganet_amd.modules.mixed import MixedTrainBnRelu
    dt = tdtype(fmt)
    bns = [torch.nn.BatchNorm3d(6).cuda().train() for _ in range(3)]
    conv, pre, tail = MixedTrainBnRelu(bns[0]), MixedTrainBnRelu(bns[1], out_dtype=torch.float32), MixedTrainBnRelu(bns[2])
    g = torch.Generator(device="cuda").manual_seed(4)
    new = lambda d=dt, s=(2, 6, 5, 9, 16): (torch.randn(*s, device="cuda", generator=g) * 1.5 + 0.3).to(d)   # noqa: E731
    f32 = torch.float32
    x, rem, gy, gy32 = new().requires_grad_(), new(f32).requires_grad_(), new(), new(f32)
    a, b, gc = new(s=(2, 6, 9, 16)).requires_grad_(), new(s=(2, 6, 9, 16)).requires_grad_(), new(s=(2, 12, 4, 9, 16))
    gd, ggs = new(s=(1, 40, 7, 9)).requires_grad_(), [new(f32, (1, 2, 5, 7, 9)) for _ in range(4)]
    lf, glf = new(s=(1, 75, 6, 10)).requires_grad_(), new(f32, (1, 75, 6, 10))
    small, gsmall = new(s=(1, 1, 5, 6, 10)).requires_grad_(), new(f32, (1, 1, 5, 6, 10))
    data = [x, rem, gy, gy32, a, b, gc, gd, lf, glf, small, gsmall] + ggs
    grad = torch.autograd.grad

    def every():
        y0, y1, y2 = conv(x), pre(x), tail(x, rem)
        out = (y0, y1, y2) + grad(y0, [x, bns[0].weight, bns[0].bias], gy) + grad(y1, [x, bns[1].weight, bns[1].bias], gy32)
        out += grad(y2, [x, rem, bns[2].weight, bns[2].bias], gy)
        out += grad(F.CostVolume16Function.apply(a, b, 4), [a, b], gc)
        ks = F.NormalizeGuidanceMixedFunction.apply(gd, 2)
        nf = F.NormalizeFiltersMixedFunction.apply(lf)
        up = F.CastFunction.apply(small, f32)
        return out + ks + (nf, up) + grad(ks, [gd], ggs) + grad(nf, [lf], glf) + grad(up, [small], gsmall)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            every()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = every()
    for _ in range(2):
        with torch.no_grad():
            for t in data:
                t.copy_(new(t.dtype, tuple(t.shape)))
        graph.replay()
        torch.cuda.synchronize()
        replayed = [t.clone() for t in outs]
        for i, (r, e) in enumerate(zip(replayed, every())):
            assert same_bits(r, e), i
    assert all(int(bn.num_batches_tracked) == 2 + 2 + 2 for bn in bns)     # warm-up, two replays, two eager calls (capturing runs nothing)


# ---- one training step of the stand-in network ------------------------------------------------------------------------------

def _count_casts(torch, params, min_numel, log):
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


def _bn_ops(model):
    """every op module that can run a BatchNorm of a prepared model: the helpers harness.fuse keeps outside the module tree"""
    from ganet_amd.modules.fused import BnRelu
    from ganet_amd.modules.mixed import MixedTrainBnRelu
    found = []
    for owner in model.modules():
        for key in ("_mixed_bn", "_mixed_tail", "_mixed_bnrelu", "_fused_bn", "_fused_tail"):
            h = owner.__dict__.get(key)
            h = getattr(h, "op", h)                                        # the cast arm's BnRelu, between its casts
            if isinstance(h, (BnRelu, MixedTrainBnRelu)) and all(h is not f for f in found):
                found.append(h)
    return found


def _record_bn_calls(torch, model, calls):
    """hooks on every BatchNorm op: the fp32 values of the x, rem and y of each call (a 16-bit tensor's up-cast is exact), the
    gradient that reaches y, and the running buffers before and after"""
    handles = []

    def host(t):
        # (no ATen cast on the way: the step's cast census runs around these hooks; the up-cast is the table's own)
        if t is None:
            return None
        t = t.detach().contiguous().cpu()
        if t.dtype == torch.float32:
            return t.numpy()
        return mc.up(t.view(torch.int16).numpy().view(np.uint16), mc.F16 if t.dtype == torch.float16 else mc.BF16).reshape(tuple(t.shape))

    def pre(op, args):
        bn = op.bn
        op.__dict__["_before"] = (host(bn.running_mean), host(bn.running_var))

    def post(op, args, out):
        bn = op.bn
        rec = {"bn": bn, "relu": bool(op.relu), "x": host(args[0]), "rem": host(args[1]) if len(args) > 1 else None, "y": host(out),
               "before": op.__dict__.pop("_before"), "after": (host(bn.running_mean), host(bn.running_var)), "gy": None}
        out.register_hook(lambda g_, rec=rec: rec.__setitem__("gy", host(g_)))
        calls.append(rec)

    for op in _bn_ops(model):
        handles += [op.register_forward_pre_hook(pre), op.register_forward_hook(post)]
    return handles


def _check_bn_calls(torch, model, calls, scale, what):
    """every BatchNorm the step reached: grad_weight, grad_bias and each running-buffer update against bn_ref64.Reference on the
    RECORDED x, rem and grad_y, within bn_cases' bars (with its term for recorded model data, whose channels may sit far from
    zero).  Recorded data cannot be nudged off the ReLU's kink: where float64 cannot decide for fp32 the mask is the call's own
    y > 0 (tests/model_calls.py: check_bn_relu), and where a positive z left a zero in a 16-bit y, float64's.  A BatchNorm that
    served several calls (the feature tower: both images) has the sum of their gradients, rounded once more in fp32."""
    import bn_ref64
    by_bn = {}
    for rec in calls:
        by_bn.setdefault(id(rec["bn"]), []).append(rec)
    bns = {id(b): (k, b) for k, b in model.named_modules() if isinstance(b, torch.nn.modules.batchnorm._BatchNorm)}
    reached = {i for i, (k, b) in bns.items() if b.weight.grad is not None}
    assert set(by_bn) == reached and len(reached) > 10, "a BatchNorm ran somewhere the hooks do not see"
    worst = {}
    for i, recs in by_bn.items():
        name, bn = bns[i]
        gw = gb = bar_w = bar_b = 0.0
        for rec in recs:
            assert rec["gy"] is not None, name
            N, C = rec["x"].shape[:2]
            shape = (N, C, rec["x"].size // (N * C))
            rs = lambda a: None if a is None else np.ascontiguousarray(a, np.float32).reshape(shape)   # noqa: E731
            args = (rs(rec["x"]), rs(rec["rem"]), rs(rec["gy"]) / np.float32(scale), bn.weight.detach().cpu().numpy(),
                    bn.bias.detach().cpu().numpy(), rec["before"][0], rec["before"][1], bn.momentum, bn.eps, rec["relu"])
            y = rs(rec["y"])
            z64 = bn_ref64.Reference(*args).z
            r = bn_ref64.Reference(*args, relu_positive=np.where(y != 0, y > 0, z64 > 0))
            m = r.m
            q = bc.within("running_mean", rec["after"][0], r.running_mean, 2.0 ** -22 * ((1 - m) * np.abs(r.old_mean) + m * np.abs(r.mean)), False)
            worst["running_mean"] = max(worst.get("running_mean", 0.0), q)
            q = bc.within("running_var", rec["after"][1], r.running_var, 2.0 ** -22 * ((1 - m) * np.abs(r.old_var) + m * np.abs(r.new_var)), False)
            worst["running_var"] = max(worst.get("running_var", 0.0), q)
            gw, gb = gw + r.grad_weight, gb + r.grad_bias
            bar_w = bar_w + 2.0 ** -22 * r.invstd * r.sum_abs_gxm + 2.0 ** -22 * np.abs(r.mean) * r.invstd * np.abs(r.sum_g)
            bar_b = bar_b + 2.0 ** -22 * r.sum_abs_g
        if len(recs) > 1:                                                  # the accumulation into .grad: one fp32 rounding of the sum
            bar_w, bar_b = bar_w + 2.0 ** -24 * np.abs(gw), bar_b + 2.0 ** -24 * np.abs(gb)
        for key, got, want, bar in (("grad_weight", bn.weight.grad, gw, bar_w), ("grad_bias", bn.bias.grad, gb, bar_b)):
            worst[key] = max(worst.get(key, 0.0), bc.within(f"{what} {name} {key}", got.detach().cpu().numpy(), want, bar, False))
    return len(by_bn), worst


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
def test_stand_in_training_step_kernels_against_cast_arm(api, fmt):
    """use_mixed_precision_training(kernels=True) against kernels=False for one steps.train_step of tests/standin_net.py at its
    48 x 96 crop, maxdisp 48 (fp16 with a GradScaler), on both arms: every parameter the step reaches has a finite gradient; every
    BatchNorm's grad_weight, grad_bias and running-buffer updates are inside bn_cases' bars of the float64 statement on the inputs
    recorded at its site (_check_bn_calls); every BatchNorm's counter stands where the stock fp32 step leaves it (once per call of
    its site); and the kernel arm issues strictly fewer ATen casts of tensors larger than an image plane.  Both counts, the worst
    error / bar per quantity and the two losses are printed."""
    import torch
    import standin_net
    from harness import fuse, steps
    dt = tdtype(fmt)
    H, W, MAXD = 48, 96, 48
    left, right, target = steps.synthetic_batch(1, H, W, MAXD, "cuda", seed=5)
    first = standin_net.build(MAXD, "cuda")
    fuse.use_fused_ops(first), fuse.use_fused_bn(first)
    with pytest.raises(TypeError, match="fp32 only"):          # what the feature adds: un-rebound, the first GA op refuses 16 bits
        steps.train_step(first, torch.optim.SGD(first.parameters(), lr=0.0), "GANet_deep", left, right, target, MAXD, steps.criterion(True), amp=dt)
    res = {}
    for kernels in (True, False):
        m = standin_net.build(MAXD, "cuda")
        keys = list(m.state_dict())
        n = fuse.use_mixed_precision_training(m, dt, kernels=kernels)
        assert list(m.state_dict()) == keys and n > 0
        opt = torch.optim.SGD(m.parameters(), lr=0.0)
        scale = 256.0
        scaler = torch.amp.GradScaler("cuda", init_scale=scale) if fmt == mc.F16 else None
        log, calls = [], []
        handles = _record_bn_calls(torch, m, calls)
        torch.cuda.reset_peak_memory_stats()
        with _count_casts(torch, {p.data_ptr() for p in m.parameters()}, H * W, log):
            loss, err = steps.train_step(m, opt, "GANet_deep", left, right, target, MAXD, steps.criterion(True), amp=dt, scaler=scaler)
        peak = torch.cuda.max_memory_allocated()
        for h in handles:
            h.remove()
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(err))
        reached = [(k, p) for k, p in m.named_parameters() if p.grad is not None]
        assert len(reached) > 0 and all(bool(torch.isfinite(p.grad).all()) for _, p in reached), "a gradient is not finite"
        # (the scaler has divided the parameters' gradients by its scale, a power of two; the recorded grad_y still carry it)
        n_bn, worst = _check_bn_calls(torch, m, calls, scale if scaler is not None else 1.0, f"{mc.FMT_NAME[fmt]} kernels={kernels}")
        nbt = {k: int(b.num_batches_tracked) for k, b in m.named_modules() if isinstance(b, torch.nn.modules.batchnorm._BatchNorm)}
        res[kernels] = dict(m=m, loss=float(loss), casts=len(log), peak=peak, reached={k for k, _ in reached}, nbt=nbt)
        print(f"stand-in step {mc.FMT_NAME[fmt]} kernels={kernels}: {n_bn} BatchNorms in {len(calls)} calls, worst error / bar "
              + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    k, a = res[True], res[False]
    assert k["reached"] == a["reached"]
    # once per call of its site: the counters of the stock fp32 step (feature.bn serves both images: 2)
    stock = standin_net.build(MAXD, "cuda")
    steps.train_step(stock, torch.optim.SGD(stock.parameters(), lr=0.0), "GANet_deep", left, right, target, MAXD, steps.criterion(True))
    want = {n_: int(b.num_batches_tracked) for n_, b in stock.named_modules() if isinstance(b, torch.nn.modules.batchnorm._BatchNorm)}
    assert k["nbt"] == want and a["nbt"] == want and max(want.values()) >= 1
    print(f"stand-in step {mc.FMT_NAME[fmt]}: ATen casts of tensors larger than an image plane: kernels {k['casts']}, cast arm {a['casts']}; "
          f"peak memory {k['peak'] / 2 ** 20:.1f} MiB against {a['peak'] / 2 ** 20:.1f} MiB; loss {k['loss']:.6f} against {a['loss']:.6f}")
    assert k["casts"] < a["casts"]
