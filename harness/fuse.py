"""Swaps the opt-in fused op chains (ganet_amd.modules.fused) into an instantiated reference
model, without touching its parameters or state_dict keys: the three call-site edits of INTEGRATION.md done by
rebinding `forward` on the SGABlock / DispAgg / Disp instances.

  SGABlock.forward  models/GANet_deep.py:262-277   split + view + 4x normalize + SGA (+ bn_relu) -> GuidedSGABnRelu;
                                                   conv_refine's BatchNorm3d + `x += rem` + relu -> ResidualBnRelu (the convolution
                                                   itself stays MIOpen's)
  DispAgg.forward   models/GANet_deep.py:239-247   after the upsampling: lga, Softmin, lga, normalize, regression -> DispAggTail
  Disp.forward      models/GANet_deep.py:213-219   after the upsampling: Softmin + regression -> SoftminDisparityRegression
  both tails        models/GANet_deep.py:212, 240  F.interpolate(trilinear) -> TrilinearUpsample (gather backward instead of
                                                   ATen's atomics: 22.5 ms of a 114 ms training step, profiles/r2_model_train_stock.json)
use_fused_bn (opt-in on top, or alone):
  BasicConv.forward models/GANet_deep.py:35-41     conv -> bn -> F.relu(inplace=True): BatchNorm (batch statistics in training
                                                   mode, folded in eval mode) and ReLU -> BnRelu; the convolution stays MIOpen's
  SGABlock's tail   models/GANet_deep.py:270-277   where use_fused_ops has put a ResidualBnRelu: -> BnRelu(bn)(t, rem)
use_fused_disp_tail (opt-in on top, or alone):
  Disp.forward      models/GANet_deep.py:214-219   everything behind conv32x1 -- up-sampling, Softmin, regression -> DispTail: the
                                                   up-sampled volume is never written, forward or backward
use_fused_disp_conv (opt-in, composes with all of the above in any order):
  conv32x1          models/GANet_deep.py:212, 232  Conv3d(32, 1, 3, 1, 1) in Disp and DispAgg -> DispConv: streaming HIP kernels instead
                                                   of MIOpen's one-column GEMM; the rebind is on the convolution INSTANCE, so whichever
                                                   forward its owner has calls it
"""
import types

import torch

from ganet_amd.modules.fused import (BnRelu, DispAggTail, DispConv, DispTail, GuidedSGA, GuidedSGABnRelu, ResidualBnRelu, SoftminDisparityRegression,
                                     TrilinearUpsample)

_UP = TrilinearUpsample()


def _upsampled(self, x):
    # (the reference: F.interpolate(..., mode='trilinear', align_corners=False), models/GANet_deep.py:212, 240)
    x = _UP(self.conv32x1(x), [self.maxdisp + 1, x.size()[3] * 3, x.size()[4] * 3])
    return torch.squeeze(x, 1)


def _sgablock_forward(self, x, g):
    rem = x
    self._fused_sga.train(self.training)      # the helpers are not submodules: they follow the block's mode by hand
    x = self._fused_sga(x, g)                 # normalise guidance + SGA (+ bn_relu)
    if self.refine:
        x = self.conv_refine.conv(x)          # BasicConv(relu=False) = Conv3d + BatchNorm3d (models/GANet_deep.py:238): the
    return self._fused_tail(x, rem)           # BatchNorm, `x += rem` and the ReLU (:270-277) are ResidualBnRelu's one pass


def _dispagg_forward(self, x, lg1, lg2):
    return self._fused_tail(_upsampled(self, x), lg1, lg2)


def _disp_forward(self, x):
    return self._fused_tail(_upsampled(self, x))


def use_fused_ops(model):
    """Returns the number of call sites rebound."""
    n = 0
    for m in model.modules():
        kind = type(m).__name__
        if kind == "SGABlock":
            # registered through object.__setattr__-free assignment would add a submodule (and state_dict keys):
            # keep the helper out of the module tree
            helper = GuidedSGABnRelu(m.bn_relu[0]) if m.refine else GuidedSGA()
            object.__setattr__(m, "_fused_sga", helper)
            object.__setattr__(m, "_fused_tail", ResidualBnRelu(m.conv_refine.bn if m.refine else m.bn))
            m.forward = types.MethodType(_sgablock_forward, m)
            n += 1
        elif kind == "DispAgg":
            object.__setattr__(m, "_fused_tail", DispAggTail(m.maxdisp))
            m.forward = types.MethodType(_dispagg_forward, m)
            n += 1
        elif kind == "Disp":
            object.__setattr__(m, "_fused_tail", SoftminDisparityRegression(m.maxdisp))
            m.forward = types.MethodType(_disp_forward, m)
            n += 1
    return n


def _basicconv_forward(self, x):
    return self._fused_bn(self.conv(x))       # bn + relu (models/GANet_deep.py:37-40) in BnRelu's passes


def use_fused_bn(model):
    """BatchNorm + ReLU behind every BasicConv with use_bn, and the tails use_fused_ops has rebound, on BnRelu.  Call it
    after use_fused_ops where both are wanted.  Returns the number of call sites rebound."""
    n = 0
    for m in model.modules():
        kind = type(m).__name__
        if kind == "BasicConv" and m.use_bn:
            # (object.__setattr__: the helper stays out of the module tree, state_dict keys do not move)
            object.__setattr__(m, "_fused_bn", BnRelu(m.bn, relu=bool(m.relu)))
            m.forward = types.MethodType(_basicconv_forward, m)
            n += 1
        elif kind == "SGABlock" and isinstance(m.__dict__.get("_fused_tail"), ResidualBnRelu):
            object.__setattr__(m, "_fused_tail", BnRelu(m._fused_tail.bn, relu=True))      # the same call form (t, rem)
            n += 1
    return n


def _disp_tail_forward(self, x):
    return self._fused_tail(self.conv32x1(x))


def use_fused_disp_tail(model):
    """Every Disp (the two auxiliary disparities of training) on DispTail.  Alone, or after use_fused_ops, whose
    TrilinearUpsample -> SoftminDisparityRegression pair it replaces; DispAgg is not touched.  Returns the number of call
    sites rebound."""
    n = 0
    for m in model.modules():
        if type(m).__name__ == "Disp":
            # (object.__setattr__: the helper stays out of the module tree, state_dict keys do not move)
            object.__setattr__(m, "_fused_tail", DispTail(m.maxdisp))
            m.forward = types.MethodType(_disp_tail_forward, m)
            n += 1
    return n


def _conv32x1_forward(self, x):
    return self._fused_conv(x)


def use_fused_disp_conv(model, directions=("forward", "data", "weight")):
    """conv32x1 of every Disp and DispAgg on DispConv.  `forward` is rebound on the Conv3d instance itself: the stock forwards,
    use_fused_ops' and use_fused_disp_tail's all call self.conv32x1(x), so it composes with them in any order.  The weight stays
    the convolution's own parameter.  `directions`: which of "forward", "data", "weight" run on the HIP kernels (the rest stay
    on ATen).  Returns the number of sites rebound: 3 on GANet_deep."""
    n = 0
    for m in model.modules():
        if type(m).__name__ in ("Disp", "DispAgg") and isinstance(getattr(m, "conv32x1", None), torch.nn.Conv3d):
            conv = m.conv32x1
            # (object.__setattr__: the helper stays out of the module tree, state_dict keys do not move)
            object.__setattr__(conv, "_fused_conv", DispConv(conv, directions))
            conv.forward = types.MethodType(_conv32x1_forward, conv)
            n += 1
    return n
