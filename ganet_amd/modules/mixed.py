"""Mixed-precision inference modules (opt-in; see ganet_amd.functions.mixed): 16-bit storage between MIOpen's 16-bit
convolutions and the fp32 guided-aggregation ops.  Nothing here changes BnRelu, GetCostVolume or any other existing module."""
import torch
from torch.nn.modules.module import Module

from ..functions.mixed import bn_apply_mixed, cost_volume_16
from .fused import folded_bn

__all__ = ["MixedBnRelu", "MixedGetCostVolume"]


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
