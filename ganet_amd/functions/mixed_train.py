"""Mixed-precision TRAINING: autograd Functions over the 16-bit-storage kernels (ganet_amd/csrc/bn_kernels.h, mixed_train_kernels.h and the
forward entries of ganet_amd.functions.mixed), for a training step under torch.autocast: MIOpen's convolutions read and write
fp16 / bf16, SGA, LGA and the tails stay fp32 with the backward they have, and no ATen cast pass stands between the two.

Each Function equals the fp32 Function of ganet_amd.functions.fused on the up-cast input, rounded once wherever a result is
stored in 16 bits; the BatchNorm's statistics are the same fp64 reductions over another lane geometry (tests/mixed_train_cases.py
states both tiers of that contract).  Nothing here synchronises with the host; every scratch buffer comes from the caching
allocator per call, so the Functions run on any stream and can be captured into a graph.  Not twice differentiable.
Tensors: contiguous, on one HIP device, of the dtypes each Function names."""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _native
from .fused import _float_bits, _opt
from .GANet import _p, _stream
from .mixed import _HALF, TYPE_CODE, _count

__all__ = ["MixedBnReluFunction", "CostVolume16Function", "NormalizeGuidanceMixedFunction", "NormalizeFiltersMixedFunction",
           "CastFunction"]


def _lib():
    return _native.lib()


def _check_train(what, *pairs):
    """(tensor, allowed dtypes) pairs: HIP, one device, contiguous -- the checks of functions.mixed without its inference-only one"""
    dev = None
    for t, allowed in pairs:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{what}: ganet_amd ops need HIP (cuda) tensors: there is no CPU path")
        if t.dtype not in allowed:
            raise TypeError(f"{what}: expected {' | '.join(str(d) for d in allowed)}, got {t.dtype}")
        if dev is not None and t.device != dev:
            raise RuntimeError(f"{what}: all tensors of a ganet_amd op must live on one device")
        dev = t.device
        if not t.is_contiguous():
            raise RuntimeError(f"{what}: ganet_amd ops need contiguous tensors")


_F32 = (torch.float32,)


class MixedBnReluFunction(Function):
    """y = MixedBnReluFunction.apply(x, rem, weight, bias, running_mean, running_var, momentum, eps, relu, out_dtype)

    BnReluFunction for a 16-bit x [N,C,*] (a convolution's output under autocast), batch statistics, in two launches each way
    (ganet_bn_train_forward_mixed / _backward_mixed).  The three sites of a model:
        rem None, out_dtype None (x's dtype)      every BasicConv
        rem None, out_dtype torch.float32         the BasicConv in front of an SGABlock
        rem fp32, out_dtype None                  the SGABlock tail
    weight, bias, running_*: fp32 [C] or None; the running buffers are updated in place.  Saved for the backward: x (16-bit),
    rem, weight, bias and the two fp32 [C] statistics -- never y.  grad_x has x's dtype, grad_rem is fp32; only the gradients
    autograd asks for are computed.  The fp64 scratch of each pass is a fresh tensor from the caching allocator."""

    @staticmethod
    def forward(ctx, x, rem, weight, bias, running_mean, running_var, momentum, eps, relu, out_dtype=None):
        what = "MixedBnReluFunction"
        _check_train(what, (x, _HALF))
        out_dtype = x.dtype if out_dtype is None else out_dtype
        if out_dtype not in (x.dtype, torch.float32):
            raise TypeError(f"{what}: out_dtype is {x.dtype} or torch.float32, got {out_dtype}")
        if rem is not None and out_dtype == torch.float32:
            raise TypeError(f"{what}: no kernel for a residual with an fp32 output")
        _check_train(what, (x, _HALF), *[(t, _F32) for t in (rem, weight, bias, running_mean, running_var) if t is not None])
        if x.dim() < 3:
            raise ValueError(f"expected [N,C,*], got {tuple(x.shape)}")
        if rem is not None and rem.shape != x.shape:
            raise ValueError(f"x and rem must have one shape, got {tuple(x.shape)} and {tuple(rem.shape)}")
        N, C = x.shape[:2]
        S = x.numel() // (N * C)
        if any(t is not None and t.numel() != C for t in (weight, bias, running_mean, running_var)):
            raise ValueError("weight / bias / running statistics must have one entry per channel")
        if (weight is None) != (bias is None) or (running_mean is None) != (running_var is None):
            raise ValueError("weight and bias, running_mean and running_var come together")
        ctx.args = (N, C, S, int(bool(relu)), TYPE_CODE[x.dtype], TYPE_CODE[out_dtype])
        with torch.cuda.device_of(x):
            ws = torch.empty(_lib().query("ganet_bn_workspace", N, C, S), dtype=torch.float64, device=x.device)
            y = torch.empty(x.shape, dtype=out_dtype, device=x.device)
            mean = torch.empty(C, dtype=torch.float32, device=x.device)
            invstd = torch.empty_like(mean)
            _lib().call("ganet_bn_train_forward_mixed", _p(x), _opt(rem), _opt(weight), _opt(bias), _opt(running_mean),
                        _opt(running_var), _p(ws), _p(y), _p(mean), _p(invstd), N, C, S, _float_bits(momentum), _float_bits(eps),
                        ctx.args[3], ctx.args[4], 0, ctx.args[5], _stream())
        ctx.save_for_backward(x, rem, weight, bias, mean, invstd)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        x, rem, weight, bias, mean, invstd = ctx.saved_tensors
        N, C, S, relu, x_type, y_type = ctx.args
        need = ctx.needs_input_grad
        g = grad_y.contiguous()
        _check_train("MixedBnReluFunction.backward", (g, (torch.float32,) if y_type == 0 else (x.dtype,)))
        with torch.cuda.device_of(x):
            gx = torch.empty_like(x) if need[0] else None
            g_rem = torch.empty_like(rem) if rem is not None and need[1] else None
            gw = torch.empty_like(mean) if weight is not None and need[2] else None
            gb = torch.empty_like(mean) if bias is not None and need[3] else None
            if gx is not None or g_rem is not None or gw is not None or gb is not None:
                ws = torch.empty(_lib().query("ganet_bn_workspace", N, C, S), dtype=torch.float64, device=x.device)
                _lib().call("ganet_bn_train_backward_mixed", _p(x), _opt(rem), _p(g), _opt(weight), _opt(bias), _p(mean), _p(invstd),
                            _p(ws), _opt(gx), _opt(g_rem), _opt(gw), _opt(gb), N, C, S, relu, x_type, 0, y_type, _stream())
        return gx, g_rem, gw, gb, None, None, None, None, None, None


class CostVolume16Function(Function):
    """cost = CostVolume16Function.apply(x, y, planes): GetCostVolume on 16-bit feature maps [N,C,H,W] -> [N,2C,planes,H,W]
    (ganet_cost_volume_forward_16); backward: its adjoint with fp32 sums over the disparity, rounded once
    (ganet_cost_volume_backward_16).  Nothing is saved."""

    @staticmethod
    def forward(ctx, x, y, planes):
        _check_train("CostVolume16Function", (x, _HALF))
        _check_train("CostVolume16Function", (x, _HALF), (y, (x.dtype,)))
        if x.dim() != 4 or x.shape != y.shape:
            raise ValueError(f"expected two [N,C,H,W] maps of one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
        N, C, H, W = x.shape
        ctx.args = (N, C, int(planes), H, W)
        with torch.cuda.device_of(x):
            cost = torch.empty((N, 2 * C, int(planes), H, W), dtype=x.dtype, device=x.device)
            _lib().call("ganet_cost_volume_forward_16", _p(x), _p(y), _p(cost), N, C, int(planes), H, W, _stream())
        return cost

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_cost):
        N, C, Dn, H, W = ctx.args
        g = grad_cost.contiguous()
        _check_train("CostVolume16Function.backward", (g, _HALF))
        with torch.cuda.device_of(g):
            gx = torch.empty((N, C, H, W), dtype=g.dtype, device=g.device)
            gy = torch.empty_like(gx)
            _lib().call("ganet_cost_volume_backward_16", _p(g), _p(gx), _p(gy), N, C, Dn, H, W, TYPE_CODE[g.dtype], _stream())
        return gx, gy, None


def _l1_forward(ctx, x, G, C, K):
    """L1NormalizeGroupsFunction.forward for a 16-bit x: fp32 outputs (ganet_l1_normalize_forward_mixed); x is saved"""
    _check_train("l1 normalise (mixed)", (x, _HALF))
    if x.dim() != 4 or x.shape[1] != G * C * K:
        raise ValueError(f"expected [N,{G * C * K},H,W], got {tuple(x.shape)}")
    N, _, H, W = x.shape
    ctx.dims = (N, G, C, K, H, W)
    with torch.cuda.device_of(x):
        y = torch.empty((G, N, C, K, H, W), dtype=torch.float32, device=x.device)
        ys = [y[g] for g in range(G)]
        _lib().call("ganet_l1_normalize_forward_mixed", _p(x), *([_p(t) for t in ys] + [None] * (4 - G)), N, G, C, K, H, W,
                    TYPE_CODE[x.dtype], _stream())
    ctx.save_for_backward(x)
    return ys


def _l1_backward(ctx, grads):
    """fp32 incoming gradients (a missing one counts as zeros), the gradient of x in x's dtype (ganet_l1_normalize_backward_mixed)"""
    x, = ctx.saved_tensors
    N, G, C, K, H, W = ctx.dims
    gs = []
    for g in grads:
        g = torch.zeros((N, C, K, H, W), dtype=torch.float32, device=x.device) if g is None else g.contiguous().view(N, C, K, H, W)
        _check_train("l1 normalise (mixed) backward", (g, _F32))
        gs.append(g)
    with torch.cuda.device_of(x):
        gx = torch.empty_like(x)
        _lib().call("ganet_l1_normalize_backward_mixed", _p(x), *([_p(t) for t in gs] + [None] * (4 - G)), _p(gx), N, G, C, K, H, W,
                    TYPE_CODE[x.dtype], _stream())
    return gx


class NormalizeGuidanceMixedFunction(Function):
    """(k1, k2, k3, k4) = NormalizeGuidanceMixedFunction.apply(g, channels): normalize_guidance for a 16-bit guidance
    [N, 20*channels, H, W] -> four fp32 [N, channels, 5, H, W], what GuidedSGA takes; the gradient of g has g's dtype."""

    @staticmethod
    def forward(ctx, g, channels):
        return tuple(_l1_forward(ctx, g, 4, int(channels), 5))

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        return _l1_backward(ctx, grads), None


class NormalizeFiltersMixedFunction(Function):
    """f = NormalizeFiltersMixedFunction.apply(g): normalize_filters for 16-bit LGA filters [N, K, H, W] -> fp32 [N, K, H, W];
    the gradient of g has g's dtype."""

    @staticmethod
    def forward(ctx, g):
        if g.dim() != 4:
            raise ValueError(f"expected [N,K,H,W], got {tuple(g.shape)}")
        N, K, H, W = g.shape
        (y,) = _l1_forward(ctx, g, 1, 1, K)
        return y.view(N, K, H, W)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        return _l1_backward(ctx, [grad])


class CastFunction(Function):
    """y = CastFunction.apply(t, dtype): t.to(dtype) between fp32, fp16 and bf16 by ganet_cast; backward: ganet_cast of the
    gradient to t's dtype.  The same dtype returns t itself."""

    @staticmethod
    def forward(ctx, t, dtype):
        _check_train("CastFunction", (t, tuple(TYPE_CODE)))
        if dtype not in TYPE_CODE:
            raise TypeError(f"CastFunction: expected one of {list(TYPE_CODE)}, got {dtype}")
        ctx.src = t.dtype
        return _cast(t, dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        g = grad.contiguous()
        _check_train("CastFunction.backward", (g, tuple(TYPE_CODE)))
        return _cast(g, ctx.src), None


def _cast(t, dtype):
    if dtype == t.dtype:
        return t.view_as(t)
    out = torch.empty(t.shape, dtype=dtype, device=t.device)
    if t.numel():
        with torch.cuda.device_of(t):
            _lib().call("ganet_cast", _p(t), _p(out), *_count(t.numel()), TYPE_CODE[t.dtype], TYPE_CODE[dtype], _stream())
    return out
