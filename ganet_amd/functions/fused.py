"""Callers' normalisations folded into single kernels.

In the reference these are chains of stock PyTorch ops AROUND the guided-aggregation operators:
  * SGABlock.forward   (models/GANet_deep.py:263-268): torch.split + view + 4 x F.normalize(p=1, dim=2)
  * DispAgg.lga        (models/GANet_deep.py:235):     F.normalize(g, p=1, dim=1)
  * DispAgg.forward    (models/GANet_deep.py:246-247): F.normalize(x, p=1, dim=1) + DisparityRegression
They sit BESIDE the drop-in API (libs/GANet/... keeps the reference's call forms unchanged): a model opts in by
calling GuidedSGA / NormalizedLGA2 / DispAggTail from ganet_amd.modules.fused instead of the op chains.
"""
import struct

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _native
from .GANet import _check, _p, _sga_infer, _stream

__all__ = ["L1NormalizeGroupsFunction", "NormDisparityRegressionFunction", "normalize_guidance", "normalize_filters",
           "sga_forward_infer", "SoftminFunction", "SoftminDisparityRegressionFunction", "TrilinearUpsampleFunction",
           "UpSoftminRegressionFunction", "DispConvFunction", "disp_conv_grad_input", "disp_conv_grad_weight", "LgaRegressFunction",
           "ResidualReluFunction", "DisparityLossFunction", "disparity_loss_workspace", "BnReluFunction", "BnApplyFunction",
           "stereo_input", "window_f32", "disparity_to_u16"]


def _lib():
    return _native.lib()


class L1NormalizeGroupsFunction(Function):
    """x [N, G*C*K, H, W] (= [N,G,C,K,H,W]) -> G tensors [N,C,K,H,W], each L1-normalised over K.

    G=4, K=5 is SGABlock's split/view/normalize of the guidance; G=C=1 is F.normalize(g, p=1, dim=1)."""

    @staticmethod
    def forward(ctx, x, G, C, K):
        _check(x)
        if x.dim() != 4 or x.shape[1] != G * C * K:
            raise ValueError(f"expected [N,{G * C * K},H,W], got {tuple(x.shape)}")
        if not 1 <= G <= 4:
            raise ValueError("1 <= G <= 4")
        N, _, H, W = x.shape
        ctx.dims = (N, G, C, K, H, W)
        with torch.cuda.device_of(x):
            y = torch.empty((G, N, C, K, H, W), dtype=x.dtype, device=x.device)
            ys = [y[g] for g in range(G)]
            ptrs = [_p(t) for t in ys] + [None] * (4 - G)
            _lib().call("ganet_l1_normalize_forward", _p(x), *ptrs, N, G, C, K, H, W, _stream())
        ctx.save_for_backward(x)
        return tuple(ys)

    @staticmethod
    def backward(ctx, *grads):
        x, = ctx.saved_tensors
        N, G, C, K, H, W = ctx.dims
        gs = []
        for g in grads:
            g = torch.zeros((N, C, K, H, W), dtype=x.dtype, device=x.device) if g is None else g.contiguous()
            _check(g)
            gs.append(g)
        with torch.cuda.device_of(x):
            gx = torch.empty_like(x)
            ptrs = [_p(t) for t in gs] + [None] * (4 - G)
            _lib().call("ganet_l1_normalize_backward", _p(x), *ptrs, _p(gx), N, G, C, K, H, W, _stream())
        return gx, None, None, None


def normalize_guidance(g, channels):
    """[N, 20*channels, H, W] -> (k1, k2, k3, k4), each [N, channels, 5, H, W] and L1-normalised over dim 2
    (what SGABlock.forward computes with split + view + F.normalize, models/GANet_deep.py:263-268)."""
    return L1NormalizeGroupsFunction.apply(g.contiguous(), 4, channels, 5)


def normalize_filters(g):
    """F.normalize(g, p=1, dim=1) for LGA filters [N, K, H, W] (models/GANet_deep.py:235)."""
    N, K, H, W = g.shape
    (y,) = L1NormalizeGroupsFunction.apply(g.contiguous(), 1, 1, K)
    return y.view(N, K, H, W)


class NormDisparityRegressionFunction(Function):
    """out[N,H,W] = sum_d d * x[N,D,H,W] / max(sum_d |x|, 1e-12): F.normalize(x, p=1, dim=1) followed by
    DisparityRegression (models/GANet_deep.py:246-247, modules/GANet.py:136-148) in one pass."""

    @staticmethod
    def forward(ctx, x, ndisp):
        _check(x)
        if x.dim() != 4 or x.shape[1] != ndisp:
            raise ValueError(f"expected [N,{ndisp},H,W], got {tuple(x.shape)}")
        N, D, H, W = x.shape
        ctx.dims = (N, D, H, W)
        with torch.cuda.device_of(x):
            out = torch.empty((N, H, W), dtype=x.dtype, device=x.device)
            snorm = torch.empty_like(out)
            _lib().call("ganet_norm_disparity_regression_forward", _p(x), _p(out), _p(snorm), N, D, H, W, _stream())
        ctx.save_for_backward(x, out, snorm)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, out, snorm = ctx.saved_tensors
        g = grad_out.contiguous()
        _check(g)
        N, D, H, W = ctx.dims
        with torch.cuda.device_of(g):
            gx = torch.empty_like(x)
            _lib().call("ganet_norm_disparity_regression_backward", _p(x), _p(out), _p(snorm), _p(g), _p(gx),
                        N, D, H, W, _stream())
        return gx, None


def sga_forward_infer(x, g0, g1, g2, g3, bn_scale=None, bn_shift=None):
    """Inference-only SGA: relu(bn_scale[c] * SGA(x, g0..g3) + bn_shift[c]) in the merge kernel (plain SGA output when
    bn_scale is None).  Nothing is saved for a backward: call it under torch.no_grad()
    (SGABlock.forward, models/GANet_deep.py:269-271, in eval mode)."""
    ts = [x, g0, g1, g2, g3] + ([bn_scale, bn_shift] if bn_scale is not None else [])
    _check(*ts)
    if any(t.requires_grad for t in ts) and torch.is_grad_enabled():
        raise RuntimeError("sga_forward_infer keeps nothing for backward: wrap the call in torch.no_grad()")
    N, C, D, H, W = x.shape
    if bn_scale is not None and (bn_scale.numel() != C or bn_shift.numel() != C):
        raise ValueError("bn_scale / bn_shift must have one entry per channel")
    with torch.cuda.device_of(x):
        out = _sga_infer(x, g0, g1, g2, g3, torch.empty_like(x), bn_scale, bn_shift)
    return out


class SoftminFunction(Function):
    """nn.Softmin(dim=1) on [N,D,H,W] (models/GANet_deep.py:244) in one kernel each way."""

    @staticmethod
    def forward(ctx, x):
        _check(x)
        if x.dim() != 4:
            raise ValueError("expected [N,D,H,W]")
        N, D, H, W = x.shape
        with torch.cuda.device_of(x):
            y = torch.empty_like(x)
            _lib().call("ganet_softmin_forward", _p(x), _p(y), N, D, H, W, _stream())
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, grad_y):
        y, = ctx.saved_tensors
        g = grad_y.contiguous()
        _check(g)
        N, D, H, W = y.shape
        with torch.cuda.device_of(g):
            gx = torch.empty_like(y)
            _lib().call("ganet_softmin_backward", _p(y), _p(g), _p(gx), N, D, H, W, _stream())
        return gx


class SoftminDisparityRegressionFunction(Function):
    """out[N,H,W] = sum_d d * softmin_d(x): Disp.forward's Softmin(dim=1) + DisparityRegression
    (models/GANet_deep.py:217-219) in one pass; the probabilities are never materialised."""

    @staticmethod
    def forward(ctx, x, ndisp):
        _check(x)
        if x.dim() != 4 or x.shape[1] != ndisp:
            raise ValueError(f"expected [N,{ndisp},H,W], got {tuple(x.shape)}")
        N, D, H, W = x.shape
        with torch.cuda.device_of(x):
            out = torch.empty((N, H, W), dtype=x.dtype, device=x.device)
            mx, ssum = torch.empty_like(out), torch.empty_like(out)
            _lib().call("ganet_softmin_regression_forward", _p(x), _p(out), _p(mx), _p(ssum), N, D, H, W, _stream())
        ctx.save_for_backward(x, out, mx, ssum)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, out, mx, ssum = ctx.saved_tensors
        g = grad_out.contiguous()
        _check(g)
        N, D, H, W = x.shape
        with torch.cuda.device_of(g):
            gx = torch.empty_like(x)
            _lib().call("ganet_softmin_regression_backward", _p(x), _p(out), _p(mx), _p(ssum), _p(g), _p(gx),
                        N, D, H, W, _stream())
        return gx, None


class TrilinearUpsampleFunction(Function):
    """F.interpolate(x, size, mode='trilinear', align_corners=False) on [N,C,D,H,W] (the cost-volume up-sampling of
    Disp.forward / DispAgg.forward, models/GANet_deep.py:212, 240) with a GATHER backward: one lane per input voxel sums the
    output gradients that read it, instead of ATen's eight atomicAdds per output element."""

    @staticmethod
    def forward(ctx, x, size):
        _check(x)
        if x.dim() != 5 or len(size) != 3:
            raise ValueError("TrilinearUpsample expects [N,C,D,H,W] and a 3-element output size")
        N, C, Di, Hi, Wi = x.shape
        Do, Ho, Wo = (int(v) for v in size)
        ctx.dims = (N, C, Di, Hi, Wi, Do, Ho, Wo)
        with torch.cuda.device_of(x):
            y = torch.empty((N, C, Do, Ho, Wo), dtype=x.dtype, device=x.device)
            _lib().call("ganet_trilinear_upsample_forward", _p(x), _p(y), N * C, Di, Hi, Wi, Do, Ho, Wo, _stream())
        return y

    @staticmethod
    def backward(ctx, gy):
        g = gy.contiguous()
        _check(g)
        N, C, Di, Hi, Wi, Do, Ho, Wo = ctx.dims
        with torch.cuda.device_of(g):
            gx = torch.empty((N, C, Di, Hi, Wi), dtype=g.dtype, device=g.device)
            _lib().call("ganet_trilinear_upsample_backward", _p(g), _p(gx), N * C, Di, Hi, Wi, Do, Ho, Wo, _stream())
        return gx, None


class UpSoftminRegressionFunction(Function):
    """out[N,Ho,Wo] = sum_d d * softmin_d(F.interpolate(x, size, mode='trilinear', align_corners=False)): Disp.forward behind
    its conv32x1 (models/GANet_deep.py:214-219) without the up-sampled volume.  x is [N,1,Di,Hi,Wi] (the convolution's
    output) or [N,Di,Hi,Wi]; size = (Do, Ho, Wo).  Saved: x and three [N,Ho,Wo] maps.  The backward takes its column
    workspace [N,Di,Ho,Wo] from the caching allocator: no state, no host synchronisation, any stream, capturable."""

    @staticmethod
    def forward(ctx, x, size):
        _check(x)
        if x.dim() == 5 and x.shape[1] != 1:
            raise ValueError(f"expected [N,1,Di,Hi,Wi] or [N,Di,Hi,Wi], got {tuple(x.shape)}")
        if x.dim() not in (4, 5) or len(size) != 3:
            raise ValueError("UpSoftminRegression expects [N,1,Di,Hi,Wi] or [N,Di,Hi,Wi] and a 3-element output size")
        N, (Di, Hi, Wi) = x.shape[0], x.shape[-3:]
        Do, Ho, Wo = (int(v) for v in size)
        ctx.dims = (N, Di, Hi, Wi, Do, Ho, Wo)
        with torch.cuda.device_of(x):
            out = torch.empty((N, Ho, Wo), dtype=x.dtype, device=x.device)
            mx, ssum = torch.empty_like(out), torch.empty_like(out)
            _lib().call("ganet_up_softmin_regression_forward", _p(x), _p(out), _p(mx), _p(ssum), *ctx.dims, _stream())
        ctx.save_for_backward(x, out, mx, ssum)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, out, mx, ssum = ctx.saved_tensors
        g = grad_out.contiguous()
        _check(g)
        N, Di, Hi, Wi, Do, Ho, Wo = ctx.dims
        with torch.cuda.device_of(g):
            ws = torch.empty((N, Di, Ho, Wo), dtype=x.dtype, device=x.device)
            gx = torch.empty_like(x)
            _lib().call("ganet_up_softmin_regression_backward", _p(x), _p(out), _p(mx), _p(ssum), _p(g), _p(ws), _p(gx),
                        *ctx.dims, _stream())
        return gx, None


_CONV_BWD = ([1, 1, 1], [1, 1, 1], [1, 1, 1], False, [0, 0, 0], 1)     # stride, padding, dilation, transposed, output_padding, groups


def disp_conv_grad_input(grad_y, weight, x, native=True):
    """grad_x [N,C,D,H,W] of DispConvFunction from grad_y [N,1,D,H,W] (contiguous): ganet_disp_conv_backward_data, or ATen's
    data gradient of the same convolution (native=False).  Plain function, nothing is recorded for autograd."""
    if not native:
        return torch.ops.aten.convolution_backward(grad_y, x, weight, None, *_CONV_BWD, [True, False, False])[0]
    _check(grad_y, weight)
    with torch.cuda.device_of(grad_y):
        gx = torch.empty(x.shape, dtype=grad_y.dtype, device=grad_y.device)
        _lib().call("ganet_disp_conv_backward_data", _p(grad_y), _p(weight), _p(gx), *x.shape, _stream())
    return gx


def disp_conv_grad_weight(x, grad_y, weight, native=True):
    """grad_weight [1,C,3,3,3] of DispConvFunction: ganet_disp_conv_backward_weight (two launches, no atomics: two runs give the
    same bits; the workspace is a fresh tensor from the caching allocator), or ATen's weight gradient (native=False)."""
    if not native:
        return torch.ops.aten.convolution_backward(grad_y, x, weight, None, *_CONV_BWD, [False, True, False])[1]
    _check(x, grad_y)
    with torch.cuda.device_of(x):
        ws = torch.empty(_lib().query("ganet_disp_conv_workspace", *x.shape), dtype=x.dtype, device=x.device)
        gw = torch.empty(weight.shape, dtype=x.dtype, device=x.device)
        _lib().call("ganet_disp_conv_backward_weight", _p(x), _p(grad_y), _p(ws), _p(gw), *x.shape, _stream())
    return gw


class DispConvFunction(Function):
    """y [N,1,D,H,W] = F.conv3d(x [N,C,D,H,W], weight [1,C,3,3,3], stride 1, padding 1): the tails' conv32x1
    (models/GANet_deep.py:212, 232) on the streaming kernels of disp_conv_kernels.h instead of MIOpen's one-column GEMM.
    Saved: x and weight, nothing else; neither is written.  Only the gradients autograd asks for are computed
    (disp_conv_grad_input, disp_conv_grad_weight): no state, no host synchronisation, any stream, capturable.
    `directions`: which of "forward", "data", "weight" run here; the others go to ATen."""

    ALL = ("forward", "data", "weight")

    @staticmethod
    def forward(ctx, x, weight, directions=ALL):
        _check(x, weight)
        if x.dim() != 5 or weight.dim() != 5 or tuple(weight.shape) != (1, x.shape[1], 3, 3, 3):
            raise ValueError(f"expected x [N,C,D,H,W] and weight [1,C,3,3,3], got {tuple(x.shape)} and {tuple(weight.shape)}")
        N, C, D, H, W = x.shape
        ctx.directions = tuple(directions)
        with torch.cuda.device_of(x):
            if "forward" in ctx.directions:
                y = torch.empty((N, 1, D, H, W), dtype=x.dtype, device=x.device)
                _lib().call("ganet_disp_conv_forward", _p(x), _p(weight), _p(y), N, C, D, H, W, _stream())
            else:
                y = torch.nn.functional.conv3d(x, weight, None, 1, 1)
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        x, weight = ctx.saved_tensors
        g = grad_y.contiguous()
        _check(g)
        gx = disp_conv_grad_input(g, weight, x, "data" in ctx.directions) if ctx.needs_input_grad[0] else None
        gw = disp_conv_grad_weight(x, g, weight, "weight" in ctx.directions) if ctx.needs_input_grad[1] else None
        return gx, gw, None


class LgaRegressFunction(Function):
    """One LGA pass followed by F.normalize(p=1, dim=1) + DisparityRegression -- the last three statements of
    DispAgg.forward (models/GANet_deep.py:245-247 after the first pass of the second LGA2) -- with the two reductions over
    the disparity axis done in the LGA kernel's epilogue (ganet_lga_forward_regress): out = sum_d d*y / max(sum_d |y|, 1e-12)
    is a per-pixel finish, and without autograd the volume y is never written."""

    @staticmethod
    def forward(ctx, x, filters, radius, ndisp):
        _check(x, filters)
        if x.dim() != 4 or x.shape[1] != ndisp:
            raise ValueError(f"expected [N,{ndisp},H,W], got {tuple(x.shape)}")
        N, D, H, W = x.shape
        if tuple(filters.shape) != (N, 3 * (2 * radius + 1) ** 2, H, W):
            raise ValueError("LGA filters must be [N, 3(2r+1)^2, H, W]")
        ctx.radius, ctx.dims = radius, (N, D, H, W)
        keep = any(ctx.needs_input_grad[:2])
        with torch.cuda.device_of(x):
            y = torch.empty_like(x) if keep else None
            snorm = torch.empty((N, H, W), dtype=x.dtype, device=x.device)
            sdy = torch.empty_like(snorm)
            try:
                _lib().call("ganet_lga_forward_regress", _p(x), _p(filters), _p(y) if keep else None, _p(snorm), _p(sdy),
                            N, D, H, W, radius, _stream())
                snorm.clamp_(min=1e-12)
                out = sdy / snorm
            except _native.GanetError as e:                # no fused kernel for this shape: the two separate entries
                if e.code != _native.E_UNSUPPORTED:
                    raise
                y = torch.empty_like(x)
                out = sdy
                _lib().call("ganet_lga_forward", _p(x), _p(filters), _p(y), N, D, H, W, radius, _stream())
                _lib().call("ganet_norm_disparity_regression_forward", _p(y), _p(out), _p(snorm), N, D, H, W, _stream())
        if keep:
            ctx.save_for_backward(x, filters, y, out, snorm)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, filters, y, out, snorm = ctx.saved_tensors
        g = grad_out.contiguous()
        _check(g)
        N, D, H, W = ctx.dims
        with torch.cuda.device_of(g):
            gy = torch.empty_like(y)
            _lib().call("ganet_norm_disparity_regression_backward", _p(y), _p(out), _p(snorm), _p(g), _p(gy),
                        N, D, H, W, _stream())
            gx = torch.empty_like(x)
            gf = torch.empty_like(filters)
            _lib().call("ganet_lga_backward", _p(x), _p(filters), _p(gy), _p(gx), _p(gf), N, D, H, W, ctx.radius, 0, _stream())
        return gx, gf, None, None


class ResidualReluFunction(Function):
    """The end of SGABlock.forward (models/GANet_deep.py:270-277) in one pass each way:
        y = relu(bn_scale[c] * t + bn_shift[c] + rem)      bn_scale / bn_shift: conv_refine's BatchNorm3d folded from its running
                                                           statistics (eval mode; constants: they get no gradient here)
        y = relu(t + rem)                                  bn_scale is None: t = bn(conv(..)) from the framework (training mode)
    for `x = conv_refine(x); x += rem; return relu(x)`.  `inplace` writes y over t as the reference's `x += rem` does (t must
    be a temporary nobody else needs: the convolution's / BatchNorm's output -- BatchNorm's backward reads its input, not t).
    Backward: g = grad_y where y > 0; both inputs take g (bn_scale given: t takes bn_scale[c] * g)."""

    @staticmethod
    def forward(ctx, t, rem, bn_scale=None, bn_shift=None, inplace=False):
        ts = [t, rem] + ([bn_scale, bn_shift] if bn_scale is not None else [])
        _check(*ts)
        if t.dim() != 5 or t.shape != rem.shape:
            raise ValueError(f"expected two [N,C,D,H,W] volumes of one shape, got {tuple(t.shape)} and {tuple(rem.shape)}")
        N, C, D, H, W = t.shape
        if (bn_scale is None) != (bn_shift is None):
            raise ValueError("bn_scale and bn_shift come together")
        if bn_scale is not None and (bn_scale.numel() != C or bn_shift.numel() != C):
            raise ValueError("bn_scale / bn_shift must have one entry per channel")
        ctx.dims = (N, C, D, H, W)
        with torch.cuda.device_of(t):
            y = t if inplace else torch.empty_like(t)
            _lib().call("ganet_residual_relu_forward", _p(t), _p(rem), _p(bn_scale) if bn_scale is not None else None,
                        _p(bn_shift) if bn_shift is not None else None, _p(y), N, C, D, H, W, _stream())
        if inplace:
            ctx.mark_dirty(t)
        ctx.scaled = bn_scale is not None
        if ctx.scaled:
            ctx.save_for_backward(y, bn_scale)
        else:
            ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, grad_y):
        y = ctx.saved_tensors[0]
        g = grad_y.contiguous()
        _check(g)
        N, C, D, H, W = ctx.dims
        with torch.cuda.device_of(g):
            g_rem = torch.empty_like(y)
            if ctx.scaled:
                g_t = torch.empty_like(y)
                _lib().call("ganet_residual_relu_backward", _p(y), _p(g), _p(ctx.saved_tensors[1]), _p(g_t), _p(g_rem),
                            N, C, D, H, W, _stream())
            else:
                g_t = g_rem
                _lib().call("ganet_residual_relu_backward", _p(y), _p(g), None, None, _p(g_rem), N, C, D, H, W, _stream())
        return g_t, g_rem, None, None, None


def disparity_loss_workspace(like, N, H, W):
    """the fp64 scratch ganet_disparity_loss_forward wants for [N,H,W] maps, on `like`'s device"""
    n = _lib().query("ganet_disparity_loss_workspace", N, H, W)
    return torch.empty(n, dtype=torch.float64, device=like.device)


class DisparityLossFunction(Function):
    """loss, stats = DisparityLossFunction.apply(target, params, workspace, kinds, mask_mode, *predictions)

    The criterion of train.py:100-118 and the error read-out of train.py:126 / evaluation.py:199-202 in two launches (one
    more for the backward), with no `d[mask]` gather and no host round trip -- so it runs under
    torch.cuda.set_sync_debug_mode("error") and inside a captured graph.
      predictions  1..3 maps [N,H,W];  target [N,H,W] (never gets a gradient)
      params       device tensor of 8 floats {hi, lo, w0, w1, w2, thresh, alpha, rate_thresh}
      workspace    disparity_loss_workspace(...), private to the call until it has run on the stream
      kinds        per map 0 (smooth-L1) | 1 (MyLoss2(thresh, alpha), the reference's sequential masked updates)
      mask_mode    0: target < hi | 1: lo <= target <= hi
    loss: 0-d, sum_k w_k * mean over the valid pixels of rho_k;  stats: [1 + 3P] = count, then per map mean rho, mean |r|
    (EPE) and the fraction with |r| > rate_thresh; not differentiable.
    WITHOUT A VALID PIXEL the loss and all stats are 0 and the backward writes all-zero maps that are still attached to
    the forward graph -- deliberately not the NaN that stock torch gives for the mean of an empty selection."""

    @staticmethod
    def forward(ctx, target, params, workspace, kinds, mask_mode, *preds):
        P = len(preds)
        if not 1 <= P <= 3 or len(kinds) != P:
            raise ValueError("1..3 prediction maps with one kind each")
        _check(target, params, *preds)
        if target.dim() != 3 or any(p.shape != target.shape for p in preds):
            raise ValueError(f"expected [N,H,W] maps of one shape, got {[tuple(p.shape) for p in preds]} and {tuple(target.shape)}")
        if params.numel() != 8:
            raise ValueError("params: 8 floats {hi, lo, w0, w1, w2, thresh, alpha, rate_thresh}")
        if not workspace.is_cuda or workspace.device != target.device or workspace.dtype != torch.float64 or not workspace.is_contiguous():
            raise ValueError("workspace: a contiguous float64 tensor on the maps' device")
        N, H, W = target.shape
        if workspace.numel() < _lib().query("ganet_disparity_loss_workspace", N, H, W):
            raise ValueError("workspace too small: see disparity_loss_workspace")
        ctx.args = (N, H, W, P) + tuple(list(kinds) + [0] * (3 - P)) + (int(mask_mode),)
        with torch.cuda.device_of(target):
            loss = torch.empty((), dtype=target.dtype, device=target.device)
            stats = torch.empty(1 + 3 * P, dtype=target.dtype, device=target.device)
            ptrs = [_p(p) for p in preds] + [None] * (3 - P)
            _lib().call("ganet_disparity_loss_forward", *ptrs, _p(target), _p(params), _p(workspace), _p(loss), _p(stats),
                        *ctx.args, _stream())
        ctx.save_for_backward(target, params, stats, *preds)
        ctx.mark_non_differentiable(stats)
        return loss, stats

    @staticmethod
    def backward(ctx, grad_loss, _grad_stats):
        target, params, stats, *preds = ctx.saved_tensors
        P = len(preds)
        want = ctx.needs_input_grad[5:]
        grads = [None] * P
        if any(want):
            g = grad_loss.to(torch.float32).contiguous()
            _check(g)
            with torch.cuda.device_of(target):
                grads = [torch.empty_like(p) if w else None for p, w in zip(preds, want)]
                _lib().call("ganet_disparity_loss_backward", *([_p(p) for p in preds] + [None] * (3 - P)), _p(target), _p(params),
                            _p(stats), _p(g), *([_p(t) if t is not None else None for t in grads] + [None] * (3 - P)),
                            *ctx.args, _stream())
        return (None, None, None, None, None) + tuple(grads)


def _float_bits(v):
    """an fp32 value as the int that carries it across the C ABI"""
    return struct.unpack("<i", struct.pack("<f", float(v)))[0]


def _opt(t):
    return _p(t) if t is not None else None


class BnReluFunction(Function):
    """y = BnReluFunction.apply(x, rem, weight, bias, running_mean, running_var, momentum, eps, relu)

    `conv -> bn -> F.relu(inplace=True)` behind every BasicConv (models/GANet_deep.py:35-41) and the BatchNorm3d + `x += rem`
    + relu of SGABlock's tail (:270-277) with BATCH statistics, in two launches each way (ganet_bn_train_forward / _backward):
      y = relu(weight (x - mean) invstd + bias [+ rem])     x [N,C,*] contiguous fp32; rem, weight, bias, running_*: None or given
    running_mean / running_var are updated in place as F.batch_norm(training=True) does (momentum: a float).  Saved for the
    backward: x, rem (when given), weight, bias and the two [C] statistics -- never y: the backward recomputes the ReLU mask
    from x.  Only the gradients autograd asks for are computed.  Not twice differentiable.  The fp64 scratch of both passes is
    a fresh 2 * rows * C doubles from the caching allocator: no state, any stream, capturable."""

    @staticmethod
    def forward(ctx, x, rem, weight, bias, running_mean, running_var, momentum, eps, relu):
        _check(*[t for t in (x, rem, weight, bias, running_mean, running_var) if t is not None])
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
        ctx.args = (N, C, S, int(bool(relu)))
        with torch.cuda.device_of(x):
            ws = torch.empty(_lib().query("ganet_bn_workspace", N, C, S), dtype=torch.float64, device=x.device)
            y = torch.empty_like(x)
            mean = torch.empty(C, dtype=x.dtype, device=x.device)
            invstd = torch.empty_like(mean)
            _lib().call("ganet_bn_train_forward", _p(x), _opt(rem), _opt(weight), _opt(bias), _opt(running_mean), _opt(running_var),
                        _p(ws), _p(y), _p(mean), _p(invstd), N, C, S, _float_bits(momentum), _float_bits(eps), ctx.args[3], _stream())
        ctx.save_for_backward(x, rem, weight, bias, mean, invstd)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        x, rem, weight, bias, mean, invstd = ctx.saved_tensors
        N, C, S, relu = ctx.args
        need = ctx.needs_input_grad
        g = grad_y.contiguous()
        _check(g)
        with torch.cuda.device_of(x):
            gx = torch.empty_like(x) if need[0] else None
            # without the ReLU, g IS grad_y: the residual takes the incoming gradient itself
            g_rem = (torch.empty_like(x) if relu else g) if rem is not None and need[1] else None
            gw = torch.empty_like(mean) if weight is not None and need[2] else None
            gb = torch.empty_like(mean) if bias is not None and need[3] else None
            if gx is not None or gw is not None or gb is not None or (g_rem is not None and relu):
                ws = torch.empty(_lib().query("ganet_bn_workspace", N, C, S), dtype=torch.float64, device=x.device)
                _lib().call("ganet_bn_train_backward", _p(x), _opt(rem), _p(g), _opt(weight), _opt(bias), _p(mean), _p(invstd), _p(ws),
                            _opt(gx), _opt(g_rem) if relu else None, _opt(gw), _opt(gb), N, C, S, relu, _stream())
        return gx, g_rem, gw, gb, None, None, None, None, None


class BnApplyFunction(Function):
    """y = relu(scale[c] * x + shift[c] [+ rem]): a BatchNorm folded from its running statistics (eval mode; scale and shift
    are constants here), the residual and the ReLU in ONE pass (ganet_bn_apply_forward) -- `inplace` writes y over x.
    Backward: g = grad_y where y > 0; rem takes g, x takes scale[c] * g (ganet_residual_relu_backward on the saved y)."""

    @staticmethod
    def forward(ctx, x, rem, scale, shift, relu, inplace):
        _check(*[t for t in (x, rem, scale, shift) if t is not None])
        if x.dim() < 3 or (rem is not None and rem.shape != x.shape):
            raise ValueError("expected [N,C,*] volumes of one shape")
        N, C = x.shape[:2]
        S = x.numel() // (N * C)
        if scale.numel() != C or shift.numel() != C:
            raise ValueError("scale / shift must have one entry per channel")
        ctx.args = (N, C, S, int(bool(relu)))
        with torch.cuda.device_of(x):
            y = x if inplace else torch.empty_like(x)
            _lib().call("ganet_bn_apply_forward", _p(x), _opt(rem), _p(scale), _p(shift), _p(y), N, C, S, ctx.args[3], _stream())
        if inplace:
            ctx.mark_dirty(x)
        ctx.has_rem = rem is not None
        ctx.save_for_backward(scale, *([y] if relu else []))
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        scale = ctx.saved_tensors[0]
        N, C, S, relu = ctx.args
        g = grad_y.contiguous()
        _check(g)
        with torch.cuda.device_of(g):
            if relu:
                y = ctx.saved_tensors[1]
                g_rem, gx = torch.empty_like(g), torch.empty_like(g)
                _lib().call("ganet_residual_relu_backward", _p(y), _p(g), _p(scale), _p(gx), _p(g_rem), N, C, 1, 1, S, _stream())
            else:
                g_rem, gx = g, g * scale.view((1, C) + (1,) * (g.dim() - 2))
        return (gx if ctx.needs_input_grad[0] else None, g_rem if ctx.has_rem and ctx.needs_input_grad[1] else None,
                None, None, None, None)


# ---- image front and back end: plain functions, integers in, nothing differentiable out -----------------------------------------

def _check_io(t, dtype, dims, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{what}: ganet_amd ops need HIP (cuda) tensors: there is no CPU path")
    if t.dtype != dtype:
        raise TypeError(f"{what}: expected {dtype}, got {t.dtype}")
    if t.dim() != dims or not t.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous {dims}-d tensor, got {tuple(t.shape)}")


def stereo_input(left_u8, right_u8, crop_hw, oy, ox_left, ox_right, out_left=None, out_right=None, form=0):
    """The model's input from a stereo pair of uint8 images [H, W, 3 | 4] (ganet_stereo_input_stats / _apply; predict.py:92-114,
    :75-90, dataloader/dataset.py:64-92): every channel standardised with its own mean and std, then
    out[c, y, x] = pixel (y + oy, x + ox_left) of the left image, resp. (y + oy, x + ox_right) of the right one, 0 outside.
    Returns (left, right), fp32 [3, Hc, Wc] each -- out_left / out_right where given (contiguous, e.g. batch[i] of a
    [B, 3, Hc, Wc] tensor).  A constant channel gives 0 (the reference: NaN).  Two launches; the integer workspace is a fresh
    8 KB from the caching allocator: no state, no host synchronisation, any stream, capturable.  form=1: the direct form of
    the apply pass instead of the table (the same bits; for measurement)."""
    _check_io(left_u8, torch.uint8, 3, "left image")
    _check_io(right_u8, torch.uint8, 3, "right image")
    if left_u8.shape != right_u8.shape or left_u8.device != right_u8.device:
        raise ValueError(f"the two images must have one shape and device, got {tuple(left_u8.shape)} and {tuple(right_u8.shape)}")
    H, W, CP = left_u8.shape
    Hc, Wc = (int(v) for v in crop_hw)
    with torch.cuda.device_of(left_u8):
        outs = []
        for t in (out_left, out_right):
            if t is None:
                t = torch.empty((3, Hc, Wc), dtype=torch.float32, device=left_u8.device)
            _check_io(t, torch.float32, 3, "output")
            if tuple(t.shape) != (3, Hc, Wc) or t.device != left_u8.device:
                raise ValueError(f"output: expected [3, {Hc}, {Wc}] on the images' device, got {tuple(t.shape)}")
            outs.append(t)
        lib = _lib()
        ws = torch.empty(lib.query("ganet_stereo_input_workspace", H, W, CP), dtype=torch.int64, device=left_u8.device)
        lib.call("ganet_stereo_input_stats", _p(left_u8), _p(right_u8), _p(ws), H, W, CP, _stream())
        lib.call("ganet_stereo_input_apply", _p(left_u8), _p(right_u8), _p(ws), _p(outs[0]), _p(outs[1]), H, W, CP, Hc, Wc,
                 int(oy), int(ox_left), int(ox_right), int(form), _stream())
    return outs[0], outs[1]


def window_f32(src, crop_hw, oy, ox, sub=0.0, fill=0.0):
    """dst[Hc, Wc] = src[y + oy, x + ox] - sub inside the fp32 map src [H, W], `fill` outside (ganet_window_f32;
    dataloader/dataset.py:53-74: the training target)."""
    _check_io(src, torch.float32, 2, "map")
    Hc, Wc = (int(v) for v in crop_hw)
    with torch.cuda.device_of(src):
        dst = torch.empty((Hc, Wc), dtype=torch.float32, device=src.device)
        _lib().call("ganet_window_f32", _p(src), _p(dst), src.shape[0], src.shape[1], Hc, Wc, int(oy), int(ox), _float_bits(sub),
                    _float_bits(fill), _stream())
    return dst


def disparity_to_u16(disp, hw, oy=0, ox=0, scale=256.0):
    """torch.uint16 [h, w] = sat(trunc(disp[y + oy, x + ox] * scale)) from the fp32 map disp [Hd, Wd] (ganet_disparity_to_u16;
    predict.py:134-138).  Below 0 and NaN give 0, 65536 and above 65535 (the reference's astype wraps there)."""
    _check_io(disp, torch.float32, 2, "disparity map")
    h, w = (int(v) for v in hw)
    with torch.cuda.device_of(disp):
        out = torch.empty((h, w), dtype=torch.uint16, device=disp.device)
        _lib().call("ganet_disparity_to_u16", _p(disp), _p(out), disp.shape[0], disp.shape[1], h, w, int(oy), int(ox),
                    _float_bits(scale), _stream())
    return out
