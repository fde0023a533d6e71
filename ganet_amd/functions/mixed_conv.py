"""Mixed precision: the tails' conv32x1 on a 16-bit input (include/ganet_hip_conv16.h, ganet_amd/csrc/disp_conv_kernels.h on a 16-bit storage type).

Under torch.autocast the volume in front of conv32x1 is fp16 / bf16 and the tails behind it are fp32.  DispConv16Function reads
the 16-bit x and the fp32 weight PARAMETER (not autocast's rounded copy) and returns an fp32 y; its data gradient is 16-bit,
summed in fp32 and rounded once; its weight gradient is fp32.  Each direction equals DispConvFunction's on the exactly up-cast
x, bit for bit (grad_x: rounded once to x's dtype) -- tests/mixed_conv_cases.py."""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _native
from . import fused as fused_fn
from . import mixed as mixed_fn
from .GANet import _p, _stream

__all__ = ["DispConv16Function", "disp_conv16_grad_input", "disp_conv16_grad_weight"]

_HALF = (torch.float16, torch.bfloat16)


def _lib():
    return _native.lib()


def _check16(what, x16, *f32):
    for t, allowed in [(x16, _HALF)] + [(t, (torch.float32,)) for t in f32]:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{what}: ganet_amd ops need HIP (cuda) tensors: there is no CPU path")
        if t.dtype not in allowed:
            raise TypeError(f"{what}: expected {' | '.join(str(d) for d in allowed)}, got {t.dtype}")
        if t.device != x16.device:
            raise RuntimeError(f"{what}: all tensors of a ganet_amd op must live on one device")
        if not t.is_contiguous():
            raise RuntimeError(f"{what}: ganet_amd ops need contiguous tensors")


def disp_conv16_grad_input(grad_y, weight, x, native=True):
    """grad_x [N,C,D,H,W] in x's 16-bit dtype from an fp32 grad_y [N,1,D,H,W] and the fp32 weight:
    ganet_disp_conv_backward_data_16 (fp32 sums, one rounding), or ATen's 16-bit data gradient (native=False)."""
    if not native:
        return torch.ops.aten.convolution_backward(grad_y.to(x.dtype), x, weight.to(x.dtype), None, *fused_fn._CONV_BWD,
                                                   [True, False, False])[0]
    _check16("disp_conv16_grad_input", x, grad_y, weight)
    with torch.cuda.device_of(grad_y):
        gx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        _lib().call("ganet_disp_conv_backward_data_16", _p(grad_y), _p(weight), _p(gx), *x.shape, mixed_fn.TYPE_CODE[x.dtype], _stream())
    return gx


def disp_conv16_grad_weight(x, grad_y, weight, native=True):
    """grad_weight [1,C,3,3,3] in fp32 from a 16-bit x and an fp32 grad_y: ganet_disp_conv_backward_weight_16 (two launches, no
    atomics: two runs give the same bits), or ATen's 16-bit weight gradient up-cast (native=False)."""
    if not native:
        return torch.ops.aten.convolution_backward(grad_y.to(x.dtype), x, weight.to(x.dtype), None, *fused_fn._CONV_BWD,
                                                   [False, True, False])[1].float()
    _check16("disp_conv16_grad_weight", x, grad_y)
    with torch.cuda.device_of(x):
        ws = torch.empty(_lib().query("ganet_disp_conv_workspace", *x.shape), dtype=torch.float32, device=x.device)
        gw = torch.empty(weight.shape, dtype=torch.float32, device=x.device)
        _lib().call("ganet_disp_conv_backward_weight_16", _p(x), _p(grad_y), _p(ws), _p(gw), *x.shape, mixed_fn.TYPE_CODE[x.dtype],
                    _stream())
    return gw


class DispConv16Function(Function):
    """y fp32 [N,1,D,H,W] = conv3d(x fp16 | bf16 [N,C,D,H,W], weight fp32 [1,C,3,3,3], stride 1, padding 1) on the streaming
    kernels of disp_conv_kernels.h.  Saved: x and weight, nothing else; neither is written.  Only the gradients autograd asks
    for are computed: grad_x in x's dtype, grad_weight fp32.  No state, no host synchronisation, any stream, capturable.
    `directions`, as DispConvFunction's: which of "forward", "data", "weight" run here; the others go to ATen's 16-bit
    convolution on the rounded weight (what torch.autocast does with the stock module), its result up-cast."""

    ALL = fused_fn.DispConvFunction.ALL

    @staticmethod
    def forward(ctx, x, weight, directions=ALL):
        _check16("DispConv16Function", x, weight)
        if x.dim() != 5 or weight.dim() != 5 or tuple(weight.shape) != (1, x.shape[1], 3, 3, 3):
            raise ValueError(f"expected x [N,C,D,H,W] and weight [1,C,3,3,3], got {tuple(x.shape)} and {tuple(weight.shape)}")
        N, C, D, H, W = x.shape
        ctx.directions = tuple(directions)
        with torch.cuda.device_of(x):
            if "forward" in ctx.directions:
                y = torch.empty((N, 1, D, H, W), dtype=torch.float32, device=x.device)
                _lib().call("ganet_disp_conv_forward_16", _p(x), _p(weight), _p(y), N, C, D, H, W, mixed_fn.TYPE_CODE[x.dtype], _stream())
            else:
                y = torch.nn.functional.conv3d(x, weight.to(x.dtype), None, 1, 1).float()
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        x, weight = ctx.saved_tensors
        g = grad_y.contiguous()
        gx = disp_conv16_grad_input(g, weight, x, "data" in ctx.directions) if ctx.needs_input_grad[0] else None
        gw = disp_conv16_grad_weight(x, g, weight, "weight" in ctx.directions) if ctx.needs_input_grad[1] else None
        return gx, gw, None
