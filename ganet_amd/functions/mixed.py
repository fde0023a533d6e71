"""Mixed-precision inference: the streaming ops between a 16-bit convolution (torch.autocast: MIOpen in fp16 / bf16) and the
fp32 guided-aggregation ops, on 16-bit STORAGE with fp32 arithmetic inside (ganet_amd/csrc/mixed_kernels.h).  SGA, LGA and the
tails stay fp32, bit for bit as they are; these functions keep an ATen cast pass from standing between a convolution and them.

Every function here equals the fp32 op of ganet_amd.functions.fused on the up-cast input, rounded once to the output type
(tests/mixed_cases.py).  Inference only: nothing is recorded for autograd, and like sga_forward_infer they raise when autograd
is on and an input wants a gradient.  Tensors: fp16 or bf16 (fp32 where stated), contiguous, on one HIP device."""
import torch

from .. import _native
from .GANet import _p, _stream

__all__ = ["cast", "bn_apply_mixed", "cost_volume_16", "normalize_guidance_mixed", "normalize_filters_mixed", "TYPE_CODE"]

TYPE_CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}     # GANET_F32 / GANET_F16 / GANET_BF16
_HALF = (torch.float16, torch.bfloat16)


def _lib():
    return _native.lib()


def _check_mixed(what, *tensors, dtypes=_HALF):
    """tensors: (tensor, allowed dtypes or None for `dtypes`) pairs or plain tensors"""
    dev = None
    for item in tensors:
        t, allowed = item if isinstance(item, tuple) else (item, dtypes)
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{what}: ganet_amd ops need HIP (cuda) tensors: there is no CPU path")
        if t.dtype not in allowed:
            raise TypeError(f"{what}: expected {' | '.join(str(d) for d in allowed)}, got {t.dtype}")
        if dev is not None and t.device != dev:
            raise RuntimeError(f"{what}: all tensors of a ganet_amd op must live on one device")
        dev = t.device
        if not t.is_contiguous():
            raise RuntimeError(f"{what}: ganet_amd ops need contiguous tensors")
        if t.requires_grad and torch.is_grad_enabled():
            raise RuntimeError(f"{what} is inference only and keeps nothing for backward: wrap the call in torch.no_grad()")


def _count(n):
    return n >> 31, n & 0x7FFFFFFF


def cast(t, dtype):
    """t.to(dtype) between fp32, fp16 and bf16 in one vectorised pass (ganet_cast): round to nearest even, every NaN becomes
    the format's one quiet NaN.  The same dtype returns t itself."""
    _check_mixed("cast", (t, tuple(TYPE_CODE)))
    if dtype not in TYPE_CODE:
        raise TypeError(f"cast: expected one of {list(TYPE_CODE)}, got {dtype}")
    if dtype == t.dtype:
        return t
    if t.numel() == 0:
        return torch.empty(t.shape, dtype=dtype, device=t.device)
    with torch.cuda.device_of(t):
        out = torch.empty(t.shape, dtype=dtype, device=t.device)
        _lib().call("ganet_cast", _p(t), _p(out), *_count(t.numel()), TYPE_CODE[t.dtype], TYPE_CODE[dtype], _stream())
    return out


def bn_apply_mixed(x, rem, scale, shift, relu=True, out_dtype=None, inplace=False):
    """y = relu(scale[c] * x + shift[c] [+ rem]) for a 16-bit x [N,C,*] (ganet_bn_apply_forward_mixed): the folded BatchNorm,
    the residual and the ReLU in one pass, computed in fp32 and rounded once.  rem: None, fp32 or x's dtype; out_dtype: x's
    dtype (None) or torch.float32; scale, shift: fp32 [C].  inplace writes y over x (out_dtype x's own only).
    Also an fp32 x with a 16-bit out_dtype (rem None or fp32): the site behind an op that autocast runs in fp32."""
    _check_mixed("bn_apply_mixed", (x, _HALF + (torch.float32,)))
    if x.dtype == torch.float32:
        if out_dtype not in _HALF:
            raise TypeError(f"bn_apply_mixed: an fp32 x needs a 16-bit out_dtype (fp32 to fp32 is BnApplyFunction's), got {out_dtype}")
        rem_ok = (torch.float32,)
    else:
        out_dtype = x.dtype if out_dtype is None else out_dtype
        if out_dtype not in (x.dtype, torch.float32):
            raise TypeError(f"bn_apply_mixed: out_dtype is {x.dtype} or torch.float32, got {out_dtype}")
        rem_ok = (x.dtype, torch.float32)
    _check_mixed("bn_apply_mixed", (x, (x.dtype,)), (scale, (torch.float32,)), (shift, (torch.float32,)),
                 *([(rem, rem_ok)] if rem is not None else []))
    if x.dim() < 3 or (rem is not None and rem.shape != x.shape):
        raise ValueError("bn_apply_mixed: expected [N,C,*] volumes of one shape")
    N, C = x.shape[:2]
    S = x.numel() // (N * C)
    if scale.numel() != C or shift.numel() != C:
        raise ValueError("bn_apply_mixed: scale / shift must have one entry per channel")
    if inplace and out_dtype != x.dtype:
        raise ValueError("bn_apply_mixed: in place only where the output has the input's dtype")
    with torch.cuda.device_of(x):
        y = x if inplace else torch.empty(x.shape, dtype=out_dtype, device=x.device)
        _lib().call("ganet_bn_apply_forward_mixed", _p(x), _p(rem) if rem is not None else None, _p(scale), _p(shift), _p(y),
                    N, C, S, int(bool(relu)), TYPE_CODE[x.dtype], TYPE_CODE[rem.dtype] if rem is not None else 0,
                    TYPE_CODE[out_dtype], _stream())
    return y


def cost_volume_16(x, y, maxdisp):
    """GetCostVolume(maxdisp)(x, y) on 16-bit feature maps [N,C,H,W] -> [N,2C,maxdisp,H,W] of the same dtype
    (ganet_cost_volume_forward_16: a copy of patterns with zeros)."""
    _check_mixed("cost_volume_16", x)
    _check_mixed("cost_volume_16", x, (y, (x.dtype,)))
    if x.dim() != 4 or x.shape != y.shape:
        raise ValueError(f"cost_volume_16: expected two [N,C,H,W] maps of one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    N, C, H, W = x.shape
    with torch.cuda.device_of(x):
        cost = torch.empty((N, 2 * C, int(maxdisp), H, W), dtype=x.dtype, device=x.device)
        _lib().call("ganet_cost_volume_forward_16", _p(x), _p(y), _p(cost), N, C, int(maxdisp), H, W, _stream())
    return cost


def _l1_groups(what, x, G, C, K):
    _check_mixed(what, x)
    if x.dim() != 4 or x.shape[1] != G * C * K:
        raise ValueError(f"{what}: expected [N,{G * C * K},H,W], got {tuple(x.shape)}")
    N, _, H, W = x.shape
    with torch.cuda.device_of(x):
        y = torch.empty((G, N, C, K, H, W), dtype=torch.float32, device=x.device)
        ys = [y[g] for g in range(G)]
        _lib().call("ganet_l1_normalize_forward_mixed", _p(x), *([_p(t) for t in ys] + [None] * (4 - G)), N, G, C, K, H, W,
                    TYPE_CODE[x.dtype], _stream())
    return tuple(ys)


def normalize_guidance_mixed(g, channels):
    """normalize_guidance for a 16-bit guidance [N, 20*channels, H, W]: (k1, k2, k3, k4), fp32 [N, channels, 5, H, W] each, what
    sga_forward_infer takes (ganet_l1_normalize_forward_mixed)."""
    return _l1_groups("normalize_guidance_mixed", g, 4, channels, 5)


def normalize_filters_mixed(g):
    """normalize_filters for 16-bit LGA filters [N, K, H, W]: fp32 [N, K, H, W]."""
    if g.dim() != 4:
        raise ValueError(f"normalize_filters_mixed: expected [N,K,H,W], got {tuple(g.shape)}")
    N, K, H, W = g.shape
    (y,) = _l1_groups("normalize_filters_mixed", g, 1, 1, K)
    return y.view(N, K, H, W)
