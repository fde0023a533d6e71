"""The channels-last inference path: the streaming ops between two 3-D convolutions on tensors whose MEMORY is [N,D,H,W,C]
(torch.channels_last_3d) -- the layout the convolution library computes in -- and the layout changes in front of and behind
the planar guided-aggregation ops, inside the same one pass (ganet_amd/csrc/cl_kernels.h, include/ganet_hip_cl.h).

Every function here equals the planar op of ganet_amd.functions.fused / .GANet on the same VALUES, bit for bit
(tests/cl_cases.py); only where the bytes lie differs.  A tensor's layout is read from its strides: contiguous means planar
(and wins where both formats hold: C == 1 or one position), dense channels-last means channels-last, anything else is made
planar-contiguous first.  Outputs carry the logical shape [N,C,*] and the requested memory format.  Inference only: nothing is
recorded for autograd.  fp32 tensors on one HIP device."""
import torch

from .. import _native
from .fused import BnApplyFunction
from .GANet import _p, _stream

__all__ = ["bn_apply_cl", "cost_volume_cl", "layout_of", "empty_cl", "PLANAR", "CL", "CL_FORMATS"]

PLANAR, CL = _native.LAYOUT_PLANAR, _native.LAYOUT_CL
CL_FORMATS = (torch.channels_last_3d, torch.channels_last)


def _lib():
    return _native.lib()


def _to_last(t):
    """the [N,*,C] view of a [N,C,*] tensor"""
    return t.permute(0, *range(2, t.dim()), 1)


def layout_of(t):
    """PLANAR, CL or None (dense in neither) for a [N,C,*] tensor, from its strides; planar wins where both hold"""
    if t.is_contiguous():
        return PLANAR
    if t.dim() >= 3 and _to_last(t).is_contiguous():
        return CL
    return None


def empty_cl(shape, device, dtype=torch.float32):
    """an uninitialised tensor of logical shape [N,C,*] whose memory is [N,*,C]"""
    shape = tuple(shape)
    t = torch.empty((shape[0],) + shape[2:] + (shape[1],), dtype=dtype, device=device)
    return t.permute(0, t.dim() - 1, *range(1, t.dim() - 1))


def _check_cl(what, *tensors):
    dev = tensors[0].device
    for t in tensors:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{what}: ganet_amd ops need HIP (cuda) tensors: there is no CPU path")
        if t.dtype != torch.float32:
            raise TypeError(f"{what}: fp32 only, got {t.dtype} (16-bit storage is ganet_amd.functions.mixed's; the two do not compose yet)")
        if t.device != dev:
            raise RuntimeError(f"{what}: all tensors of a ganet_amd op must live on one device")
        if t.requires_grad and torch.is_grad_enabled():
            raise RuntimeError(f"{what} is inference only and keeps nothing for backward: wrap the call in torch.no_grad()")


def bn_apply_cl(x, scale, shift, rem=None, relu=True, out_format=torch.channels_last_3d, inplace=False):
    """y = relu(scale[c] * x + shift[c] [+ rem]) for x [N,C,*] in either layout -> y [N,C,*] in `out_format`
    (torch.channels_last_3d / torch.channels_last: memory [N,*,C]; torch.contiguous_format: planar), one pass
    (ganet_bn_apply_forward_cl; an all-planar call is ganet_bn_apply_forward's).  rem: None or a tensor of x's shape, read as
    planar (a channels-last or non-dense rem is made planar-contiguous first).  scale, shift: fp32 [C].  inplace: y overwrites x
    where x already has the output's layout."""
    what = "bn_apply_cl"
    _check_cl(what, *[t for t in (x, rem, scale, shift) if t is not None])
    if out_format not in CL_FORMATS + (torch.contiguous_format,):
        raise ValueError(f"{what}: out_format is torch.channels_last_3d, torch.channels_last or torch.contiguous_format, got {out_format}")
    if x.dim() < 3 or (rem is not None and rem.shape != x.shape):
        raise ValueError(f"{what}: expected [N,C,*] volumes of one shape")
    N, C = x.shape[:2]
    S = x.numel() // (N * C)
    if scale.numel() != C or shift.numel() != C or not scale.is_contiguous() or not shift.is_contiguous():
        raise ValueError(f"{what}: scale / shift must be contiguous with one entry per channel")
    xl = layout_of(x)
    if xl is None:
        x, xl, inplace = x.contiguous(), PLANAR, False
    if rem is not None and not rem.is_contiguous():
        rem = rem.contiguous()
    yl = CL if out_format in CL_FORMATS else PLANAR
    if xl == PLANAR and yl == PLANAR:
        return BnApplyFunction.apply(x, rem, scale, shift, relu, inplace)
    with torch.cuda.device_of(x):
        if inplace and xl == yl:
            y = x
        else:
            y = empty_cl(x.shape, x.device) if yl == CL else torch.empty(x.shape, dtype=x.dtype, device=x.device)
        _lib().call("ganet_bn_apply_forward_cl", _p(x), _p(rem) if rem is not None else None, _p(scale), _p(shift), _p(y),
                    N, C, S, int(bool(relu)), xl, PLANAR, yl, _stream())
    return y


def cost_volume_cl(x, y, maxdisp):
    """GetCostVolume(maxdisp - 1)(x, y) for planar feature maps [N,C,H,W] -> [N,2C,maxdisp,H,W] whose memory is
    [N,maxdisp,H,W,2C] (torch.channels_last_3d): the same values, written where the first 3-D convolution reads them
    (ganet_cost_volume_forward_cl).  `maxdisp` counts planes, as GetCostVolumeFunction's does."""
    what = "cost_volume_cl"
    _check_cl(what, x, y)
    if x.dim() != 4 or x.shape != y.shape:
        raise ValueError(f"{what}: expected two [N,C,H,W] maps of one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    x, y = x.contiguous(), y.contiguous()
    N, C, H, W = x.shape
    with torch.cuda.device_of(x):
        cost = empty_cl((N, 2 * C, int(maxdisp), H, W), x.device)
        _lib().call("ganet_cost_volume_forward_cl", _p(x), _p(y), _p(cost), N, C, int(maxdisp), H, W, _stream())
    return cost
