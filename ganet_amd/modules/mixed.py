"""Mixed-precision modules (opt-in; see ganet_amd.functions.mixed and .mixed_train): 16-bit storage between MIOpen's 16-bit
convolutions and the fp32 guided-aggregation ops.  MixedBnRelu / MixedGetCostVolume are the inference forms; MixedTrainBnRelu /
MixedTrainGetCostVolume carry gradients.  Nothing here changes BnRelu, GetCostVolume or any other existing module."""
import torch
from torch.nn.modules.module import Module

from ..functions.mixed import bn_apply_mixed, cost_volume_16
from ..functions.mixed_train import CostVolume16Function, MixedBnReluFunction
from .fused import folded_bn

__all__ = ["MixedBnRelu", "MixedGetCostVolume", "MixedTrainBnRelu", "MixedTrainGetCostVolume"]


class MixedBnRelu(Module):
    """BnRelu's eval-mode fold for a 16-bit input: forward(x, rem=None) == relu(bn(x) + rem) with the arithmetic in fp32 and one
    rounding to `out_dtype` -- equal to BnRelu(bn)(x.float(), rem.float()).to(out_dtype), without the two cast passes.
      x          fp16 | bf16 [N,C,*], a convolution's output under torch.autocast; or fp32 with a 16-bit out_dtype (behind an
                 op that autocast runs in fp32, such as a bilinear up-sampling)
      rem        None, fp32 (an SGABlock's input) or x's dtype
      out_dtype  None: x's dtype; torch.float32 in front of an fp32 op (SGA)
      inplace    y overwrites x where the output has x's dtype (x: the convolution's output, a temporary)
    The BatchNorm is folded from its running statistics by folded_bn(bn), computed with autocast disabled: the (scale, shift)
    pair is fp32.  Inference only: in training mode, without running statistics, or with a BatchNorm whose parameters want
    gradients it raises -- that is BnRelu's ground."""

    def __init__(self, bn, relu=True, out_dtype=None, inplace=True):
        super().__init__()
        if not isinstance(bn, torch.nn.modules.batchnorm._BatchNorm):
            raise TypeError("MixedBnRelu wraps a BatchNorm2d / BatchNorm3d")
        if out_dtype not in (None, torch.float32, torch.float16, torch.bfloat16):
            raise TypeError(f"MixedBnRelu: out_dtype is None, torch.float32 or the input's dtype, got {out_dtype}")
        self.bn = bn                      # the caller's BatchNorm (shared, not copied)
        self.relu = relu
        self.out_dtype = out_dtype
        self.inplace = inplace

    def forward(self, x, rem=None):
        bn = self.bn
        if bn.training or not bn.track_running_stats:
            raise RuntimeError("MixedBnRelu is the eval-mode fold of a BatchNorm with running statistics (inference only); "
                               "batch statistics are BnRelu's: use BnRelu on fp32 tensors for training")
        if torch.is_grad_enabled() and any(p.requires_grad for p in bn.parameters()):
            raise RuntimeError("MixedBnRelu is inference only and the BatchNorm's parameters want gradients: wrap the call in "
                               "torch.no_grad(), or use BnRelu on fp32 tensors")
        with torch.autocast("cuda", enabled=False):
            scale, shift = folded_bn(bn)
        out_dtype = x.dtype if self.out_dtype is None and x.dtype != torch.float32 else self.out_dtype
        return bn_apply_mixed(x.contiguous(), rem.contiguous() if rem is not None else None, scale, shift, self.relu, out_dtype,
                              self.inplace and out_dtype == x.dtype)


class MixedGetCostVolume(Module):
    """GetCostVolume(maxdisp) (libs/GANet/modules/GANet.py:114-134) for 16-bit feature maps: forward(x, y) [N,C,H,W] ->
    [N,2C,maxdisp+1,H,W] of the same dtype."""

    def __init__(self, maxdisp):
        super().__init__()
        self.maxdisp = int(maxdisp) + 1   # planes, as GetCostVolume counts them

    def forward(self, x, y):
        return cost_volume_16(x.contiguous(), y.contiguous(), self.maxdisp)


class MixedTrainBnRelu(Module):
    """BnRelu for a 16-bit input under torch.autocast, with gradients: forward(x, rem=None) == relu(bn(x) + rem).
      training mode  batch statistics on the 16-bit x, fp32 / fp64 arithmetic, one rounding to the output's dtype, two launches
                     forward and two backward (MixedBnReluFunction); `bn`'s running buffers and num_batches_tracked are updated
                     as _BatchNorm.forward updates them.  x fp16 | bf16 [N,C,*]; rem None or fp32 (an SGABlock's input, and then
                     the output has x's dtype); out_dtype None (x's dtype) or torch.float32 in front of an fp32 op (SGA).
                     momentum=None (the cumulative average needs a host read of the batch counter) has no fused path: it raises.
      eval mode      MixedBnRelu's fold, with MixedBnRelu's refusals."""

    def __init__(self, bn, relu=True, out_dtype=None):
        super().__init__()
        if not isinstance(bn, torch.nn.modules.batchnorm._BatchNorm):
            raise TypeError("MixedTrainBnRelu wraps a BatchNorm2d / BatchNorm3d")
        if out_dtype not in (None, torch.float32, torch.float16, torch.bfloat16):
            raise TypeError(f"MixedTrainBnRelu: out_dtype is None, torch.float32 or the input's dtype, got {out_dtype}")
        self.bn = bn                      # the caller's BatchNorm (shared, not copied)
        self.relu = relu
        self.out_dtype = out_dtype
        object.__setattr__(self, "_eval", MixedBnRelu(bn, relu, out_dtype, inplace=False))     # (not a second registration of bn)

    def forward(self, x, rem=None):
        bn = self.bn
        if not (bn.training or not bn.track_running_stats):
            return self._eval(x, rem)
        if bn.track_running_stats and bn.momentum is None:
            raise RuntimeError("MixedTrainBnRelu: momentum=None (a cumulative average) has no fused path; give the BatchNorm a momentum")
        if bn.training and bn.track_running_stats and bn.num_batches_tracked is not None:
            bn.num_batches_tracked.add_(1)
        running = (bn.running_mean, bn.running_var) if bn.training and bn.track_running_stats else (None, None)
        return MixedBnReluFunction.apply(x.contiguous(), rem.contiguous() if rem is not None else None, bn.weight, bn.bias, *running,
                                         bn.momentum if bn.momentum is not None else 0.0, bn.eps, self.relu, self.out_dtype)


class MixedTrainGetCostVolume(Module):
    """MixedGetCostVolume with gradients: forward(x, y) [N,C,H,W] 16-bit -> [N,2C,maxdisp+1,H,W] of the same dtype; the backward
    sums in fp32 and rounds once (CostVolume16Function)."""

    def __init__(self, maxdisp):
        super().__init__()
        self.maxdisp = int(maxdisp) + 1   # planes, as GetCostVolume counts them

    def forward(self, x, y):
        return CostVolume16Function.apply(x.contiguous(), y.contiguous(), self.maxdisp)
