"""Channels-last inference modules (opt-in; see ganet_amd.functions.channels_last): the BatchNorm sites and the cost volume
between MIOpen's 3-D convolutions on channels_last_3d tensors, with the layout changes around the planar guided-aggregation
ops folded into the same pass.  Nothing here changes BnRelu, GetCostVolume or any other existing module."""
import torch
from torch.nn.modules.module import Module

from ..functions.channels_last import CL_FORMATS, bn_apply_cl, cost_volume_cl
from .fused import folded_bn

__all__ = ["ClBnRelu", "ClGetCostVolume"]


class ClBnRelu(Module):
    """BnRelu's eval-mode fold on either memory layout: forward(x, rem=None) == relu(bn(x) + rem), the bits of
    BnRelu(bn, relu)(x.contiguous(), rem) in eval mode, written in `out_format`.
      x           fp32 [N,C,*]: a convolution's output, channels-last or planar -- read from its strides
      rem         None or fp32 of x's shape, planar (an SGABlock's input)
      out_format  torch.channels_last_3d in front of a convolution, torch.contiguous_format in front of a planar op (SGA)
      inplace     y overwrites x where x already lies in out_format (x: the convolution's output, a temporary)
    The layout change, where there is one, is part of the one pass.  Inference only: in training mode, without running
    statistics, or with a BatchNorm whose parameters want gradients it raises -- that is BnRelu's ground."""

    def __init__(self, bn, relu=True, out_format=torch.channels_last_3d, inplace=True):
        super().__init__()
        if not isinstance(bn, torch.nn.modules.batchnorm._BatchNorm):
            raise TypeError("ClBnRelu wraps a BatchNorm2d / BatchNorm3d")
        if out_format not in CL_FORMATS + (torch.contiguous_format,):
            raise TypeError(f"ClBnRelu: out_format is torch.channels_last_3d or torch.contiguous_format, got {out_format}")
        self.bn = bn                      # the caller's BatchNorm (shared, not copied)
        self.relu = relu
        self.out_format = out_format
        self.inplace = inplace

    def forward(self, x, rem=None):
        bn = self.bn
        if bn.training or not bn.track_running_stats:
            raise RuntimeError("ClBnRelu is inference-only: the eval-mode fold of a BatchNorm with running statistics; batch "
                               "statistics are BnRelu's (planar tensors, training mode)")
        if torch.is_grad_enabled() and any(p.requires_grad for p in bn.parameters()):
            raise RuntimeError("ClBnRelu is inference-only and the BatchNorm's parameters want gradients: wrap the call in "
                               "torch.no_grad(), or use BnRelu")
        scale, shift = folded_bn(bn)
        return bn_apply_cl(x, scale, shift, rem, self.relu, self.out_format, self.inplace)


class ClGetCostVolume(Module):
    """GetCostVolume(maxdisp) (libs/GANet/modules/GANet.py:114-134) written channels-last: forward(x, y) [N,C,H,W] planar ->
    [N,2C,maxdisp+1,H,W] with memory [N,maxdisp+1,H,W,2C]: the same values, where the first 3-D convolution reads them."""

    def __init__(self, maxdisp):
        super().__init__()
        self.maxdisp = int(maxdisp) + 1   # planes, as GetCostVolume counts them

    def forward(self, x, y):
        return cost_volume_cl(x, y, self.maxdisp)
