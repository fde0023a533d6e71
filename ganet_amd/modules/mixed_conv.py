"""Mixed precision (opt-in): the tails' conv32x1 that keeps the HIP kernels under torch.autocast.  Nothing here changes DispConv."""
import torch

from ..functions import fused as fused_fn
from ..functions import mixed_conv as mixed_conv_fn
from . import fused as fused_mod

__all__ = ["MixedDispConv"]

_HALF = (torch.float16, torch.bfloat16)


class MixedDispConv(fused_mod.DispConv):
    """DispConv for the model under torch.autocast: MixedDispConv(conv, directions, kernels)(x) for conv32x1 =
    nn.Conv3d(C, 1, 3, 1, 1, bias=False), C <= 64.
      x fp16 | bf16   y is fp32 -- what the tails take, so no cast stands behind the convolution -- computed from the 16-bit x
                      and the fp32 weight PARAMETER (torch.autocast would round the weight to 16 bits first):
                      kernels=True   DispConv16Function: the 16-bit siblings of DispConv's kernels; grad_x comes back in x's
                                     dtype (fp32 sums, one rounding), grad_weight in fp32
                      kernels=False  the cast arm DispConvFunction.apply(x.float(), weight, directions): the same bits through an
                                     up-cast pass and an fp32 gradient volume -- the fallback, the tests' yardstick and the
                                     baseline of the measurement
      x fp32          exactly DispConv's forward.
    `directions` as DispConv's.  The module holds the convolution it was given and reads conv.weight at every call."""

    def __init__(self, conv, directions=fused_fn.DispConvFunction.ALL, kernels=True):
        super().__init__(conv, directions)
        self.kernels = bool(kernels)

    def forward(self, x):
        if x.dtype not in _HALF:
            return super().forward(x)
        w = self.conv.weight.contiguous()
        if self.kernels:
            return mixed_conv_fn.DispConv16Function.apply(x.contiguous(), w, self.directions)
        return fused_fn.DispConvFunction.apply(x.float().contiguous(), w, self.directions)
