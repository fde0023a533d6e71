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
use_mixed_precision (opt-in, inference; applies use_fused_ops and use_fused_bn where they have not been):
  every site between a convolution and a guided-aggregation op on 16-bit storage, for torch.autocast: see the function
use_mixed_precision_training (opt-in): the same sites bound to forms that carry gradients, for a training step under autocast
use_mixed_disp_conv (opt-in, alone or in any order with all of the above):
  conv32x1          models/GANet_deep.py:212, 232  -> MixedDispConv: DispConv that also takes the 16-bit volume torch.autocast hands it
                                                   (16-bit siblings of the streaming kernels, fp32 out), so the call does not go
                                                   back to the library's 16-bit convolution; a later use_fused_disp_conv undoes it
use_channels_last (opt-in, inference, fp32; applies use_fused_ops and use_fused_bn where they have not been):
  the cost aggregation on channels_last_3d tensors: the cost volume, every BatchNorm site between two 3-D convolutions and the
  layout changes around the planar SGA in ClBnRelu's one pass each: see the function
"""
import types

import torch

from ganet_amd.functions import mixed as mixed_fn
from ganet_amd.functions import mixed_train as mixed_train_fn
from ganet_amd.functions.fused import (LgaRegressFunction, SoftminFunction, normalize_filters, normalize_guidance,
                                       sga_forward_infer)
from ganet_amd.functions.GANet import Lga2Function, LgaFunction, SgaFunction
from ganet_amd.modules.fused import (BnRelu, DispAggTail, DispConv, DispTail, GuidedSGA, GuidedSGABnRelu, ResidualBnRelu, SoftminDisparityRegression,
                                     TrilinearUpsample, folded_bn)
from ganet_amd.modules.channels_last import ClBnRelu, ClGetCostVolume
from ganet_amd.modules.mixed import MixedBnRelu, MixedTrainBnRelu
from ganet_amd.modules import mixed_conv as mixed_conv_mod

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
            if isinstance(m.__dict__.get("_fused_tail"), DispTail):
                continue                  # use_fused_disp_tail came first: its one op replaces the pair below, in either order
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
    """Every Disp (the two auxiliary disparities of training) on DispTail.  Alone, or with use_fused_ops in either order: it
    replaces that function's TrilinearUpsample -> SoftminDisparityRegression pair, and use_fused_ops leaves a Disp that holds a
    DispTail alone; DispAgg is not touched.  Returns the number of call sites rebound."""
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


# ---- mixed precision: 16-bit convolutions around the fp32 guided-aggregation ops (inference) --------------------------------------

_HALF = (torch.float16, torch.bfloat16)
# the BasicConv whose output is an SGABlock's x, by the names of CostAggregation (models/GANet_deep.py:318-357, GANet11.py:287-303):
# a Conv2x stands for its conv2
_SGA_PRODUCER = {"sga1": "conv_start", "sga11": "conv1a", "sga12": "deconv2a", "sga2": "deconv1a", "sga13": "conv1b",
                 "sga14": "deconv2b", "sga3": "deconv1b"}


class _CastArmBnRelu:
    """the cast arm of a BatchNorm site: the fp32 op on .float() inputs, then .to(out_dtype)"""

    def __init__(self, bn, relu, out_dtype):
        self.op, self.out_dtype = BnRelu(bn, relu=relu), out_dtype

    def __call__(self, x, rem=None):
        y = self.op(x.float(), rem.float() if rem is not None else None)
        return y.to(self.out_dtype if self.out_dtype is not None else x.dtype)


class _MixedOps:
    """what the rebound forwards call at each site: the 16-bit-storage kernels (kernels=True) or the cast arm -- the existing
    fp32 op between ATen casts (kernels=False: the fallback, the tests' yardstick and the baseline of the measurement)"""

    def __init__(self, kernels):
        self.kernels = bool(kernels)

    def bn(self, bn, relu, out_dtype=None):
        return MixedBnRelu(bn, relu=relu, out_dtype=out_dtype) if self.kernels else _CastArmBnRelu(bn, relu, out_dtype)

    def cast(self, t, dtype):
        return mixed_fn.cast(t.contiguous(), dtype) if self.kernels else t.to(dtype)

    def guidance(self, g, channels):
        if self.kernels:
            return mixed_fn.normalize_guidance_mixed(g.contiguous(), channels)
        return normalize_guidance(g.float(), channels)

    def filters(self, g):
        return mixed_fn.normalize_filters_mixed(g.contiguous()) if self.kernels else normalize_filters(g.float())

    def cost_volume(self, cv, x, y):
        if self.kernels:
            return mixed_fn.cost_volume_16(x.contiguous(), y.contiguous(), cv.maxdisp)     # (the module holds maxdisp + 1)
        return type(cv).forward(cv, x.float(), y.float()).to(x.dtype)


def _inference_only(m):
    if m.training or torch.is_grad_enabled():
        raise RuntimeError(f"use_mixed_precision is for inference: {type(m).__name__} met a 16-bit tensor in training mode or with "
                           "autograd on (model.eval() under torch.no_grad(), as harness.steps.predict does)")


def _mixed_basicconv_forward(self, x):
    t = self.conv(x)
    if t.dtype in _HALF:
        _inference_only(self)
        return self._mixed_bn(t)          # bn + relu on 16-bit storage, rounded once to this site's output type
    return self._fused_bn(t)              # autocast off: BnRelu as before


def _mixed_sgablock_forward(self, x, g):
    if g.dtype not in _HALF:
        return _sgablock_forward(self, x, g)
    _inference_only(self)
    mx = self._mixed
    if x.dtype != torch.float32:          # (a producer this file does not know: SGA is fp32)
        x = mx.cast(x, torch.float32)
    rem = x
    ks = mx.guidance(g, x.shape[1])       # 16-bit guidance -> four fp32 weight volumes, one pass
    with torch.autocast("cuda", enabled=False):
        fold = folded_bn(self.bn_relu[0]) if self.refine else ()
    x = sga_forward_infer(x, *ks, *fold)  # fp32 in and out, unchanged
    if not self.refine:
        return self._fused_tail(x, rem)
    x = self.conv_refine.conv(x)          # autocast rounds SGA's fp32 output for the convolution (DESIGN: out of scope)
    return self._mixed_tail(x, rem) if x.dtype in _HALF else self._fused_tail(x, rem)


def _mixed_cv_forward(self, x, y):
    if x.dtype in _HALF:
        return self._mixed.cost_volume(self, x, y)
    return type(self).forward(self, x, y)


def _mixed_top_conv_forward(self, x):
    c = type(self).forward(self, x)       # GANet.conv_refine: [N,32,H/3,W/3], small; the bilinear up-sampling behind it is
    return self._mixed.cast(c, torch.float32) if c.dtype in _HALF else c      # fp32 under autocast (ATen would cast it there)


def _mixed_top_bn_relu_forward(self, x):
    # GANet.bn_relu = Sequential(BatchNorm2d, ReLU) behind the up-sampling: fp32 in, and the concatenation and the convolution
    # behind it want 16 bits -- one pass that rounds on the store, instead of an fp32 result that ATen casts twice
    if x.is_cuda and x.dtype == torch.float32 and torch.is_autocast_enabled("cuda"):
        _inference_only(self)
        return self._mixed_bn(x, torch.get_autocast_dtype("cuda"))
    if x.dtype in _HALF:
        _inference_only(self)
        return self._mixed_bn(x, x.dtype)
    return type(self).forward(self, x)


class _TopBnRelu:
    """the BatchNorm + ReLU of GANet.bn_relu on either arm: (x fp32 | 16-bit, out_dtype 16-bit)"""

    def __init__(self, bn, kernels):
        self.bn, self.kernels = bn, kernels
        self.op = BnRelu(bn, relu=True)

    def __call__(self, x, out_dtype):
        if self.kernels:
            return MixedBnRelu(self.bn, relu=True, out_dtype=out_dtype, inplace=False)(x)
        return self.op(x.float()).to(out_dtype)


def _conv32x1_f32(self, x):
    c = self.conv32x1(x)                  # [N,1,D,H,W]: small; the tails are fp32
    return self._mixed.cast(c, torch.float32) if c.dtype in _HALF else c


def _up_size(self, x):
    return [self.maxdisp + 1, x.size()[3] * 3, x.size()[4] * 3]


def _mixed_dispagg_forward(self, x, lg1, lg2):
    mx, tail = self._mixed, self._fused_tail
    v = torch.squeeze(_UP(_conv32x1_f32(self, x), _up_size(self, x)), 1)
    if lg1.dtype not in _HALF:
        return tail(v, lg1, lg2)
    _inference_only(self)
    assert lg1.size() == lg2.size()
    f1, f2 = mx.filters(lg1), mx.filters(lg2)
    v = Lga2Function.apply(v, f1, tail.radius)                        # DispAggTail.forward on filters normalised from 16 bits
    v = SoftminFunction.apply(v.contiguous())
    v = LgaFunction.apply(v, f2, tail.radius)
    return LgaRegressFunction.apply(v, f2, tail.radius, tail.ndisp)


def _mixed_disp_forward(self, x):
    c, tail = _conv32x1_f32(self, x), self._fused_tail
    if isinstance(tail, DispTail):
        return tail(c)
    return tail(torch.squeeze(_UP(c, _up_size(self, x)), 1))


def use_mixed_precision(model, dtype=torch.bfloat16, kernels=True):
    """Prepares GANet_deep / GANet11 for inference under torch.autocast("cuda", dtype=dtype) -- harness.steps.predict(..., amp=dtype):
    MIOpen's convolutions run in 16 bits, SGA, LGA and the tails stay fp32 as they are, and the sites between them run on
    16-bit storage (ganet_amd.modules.mixed / functions.mixed) so that no ATen cast pass stands between a convolution and one
    of our ops.  Applies use_fused_ops and use_fused_bn first where the model has not been rebound; helpers stay out of the
    module tree (no state_dict key moves).  Rebinds:
      BasicConv (use_bn)   a 16-bit convolution output -> MixedBnRelu; fp32 (autocast off) -> the BnRelu it had
      ... in front of an SGABlock (conv_start, conv1a, the conv2 of the Conv2x before an sga*): out_dtype fp32 -- SGA's x
      SGABlock             guidance through normalize_guidance_mixed, SGA on sga_forward_infer (fp32), the tail
                           MixedBnRelu(t 16-bit, rem fp32) -> 16-bit
      GANet.cv             MixedGetCostVolume's kernel
      DispAgg              filters through normalize_filters_mixed; conv32x1's output up-cast by `cast` in front of TrilinearUpsample
      Disp                 the same up-cast (training only: never reached in inference)
      GANet.conv_refine    its small 16-bit output up-cast by `cast`: torch.autocast runs the bilinear up-sampling behind it in fp32
      GANet.bn_relu        Sequential(BatchNorm2d, ReLU) behind that up-sampling: fp32 in, 16-bit out in one pass (MixedBnRelu), so
                           that the concatenation and the Guidance convolution behind it see 16 bits
    kernels=False rebinds the same sites to the cast arm: the existing fp32 op on .float() inputs followed by .to(out_dtype).
    `dtype` is what the model is prepared for; the sites themselves follow the tensors they meet.  Returns the number of sites."""
    if dtype not in _HALF:
        raise TypeError(f"use_mixed_precision: dtype is torch.bfloat16 or torch.float16, got {dtype}")
    mods = list(model.modules())
    if not any("_fused_sga" in m.__dict__ for m in mods if type(m).__name__ == "SGABlock"):
        use_fused_ops(model)
    if not any("_fused_bn" in m.__dict__ for m in mods if type(m).__name__ == "BasicConv"):
        use_fused_bn(model)
    mx = _MixedOps(kernels)
    to_f32 = set()
    for m in mods:
        if type(m).__name__ == "CostAggregation":
            for sga, producer in _SGA_PRODUCER.items():
                p = getattr(m, producer, None)
                if hasattr(m, sga) and p is not None:
                    to_f32.add(id(p.conv2 if type(p).__name__ == "Conv2x" else p))
    n = 0
    for m in mods:
        kind = type(m).__name__
        # (object.__setattr__: the helpers stay out of the module tree, state_dict keys do not move)
        if kind == "BasicConv" and m.use_bn:
            object.__setattr__(m, "_mixed_bn", mx.bn(m.bn, bool(m.relu), torch.float32 if id(m) in to_f32 else None))
            m.forward = types.MethodType(_mixed_basicconv_forward, m)
            n += 1
        elif kind == "SGABlock":
            object.__setattr__(m, "_mixed", mx)
            object.__setattr__(m, "_mixed_tail", mx.bn(m.conv_refine.bn if m.refine else m.bn, True))
            m.forward = types.MethodType(_mixed_sgablock_forward, m)
            n += 1
        elif kind == "GetCostVolume":
            object.__setattr__(m, "_mixed", mx)
            m.forward = types.MethodType(_mixed_cv_forward, m)
            n += 1
        elif kind in ("Disp", "DispAgg"):
            object.__setattr__(m, "_mixed", mx)
            m.forward = types.MethodType(_mixed_dispagg_forward if kind == "DispAgg" else _mixed_disp_forward, m)
            n += 1
        elif kind == "GANet":
            conv, seq = getattr(m, "conv_refine", None), getattr(m, "bn_relu", None)
            if isinstance(conv, torch.nn.Conv2d):
                object.__setattr__(conv, "_mixed", mx)
                conv.forward = types.MethodType(_mixed_top_conv_forward, conv)
                n += 1
            if isinstance(seq, torch.nn.Sequential) and len(seq) == 2 and isinstance(seq[0], torch.nn.modules.batchnorm._BatchNorm) \
                    and isinstance(seq[1], torch.nn.ReLU):
                object.__setattr__(seq, "_mixed_bn", _TopBnRelu(seq[0], mx.kernels))
                seq.forward = types.MethodType(_mixed_top_bn_relu_forward, seq)
                n += 1
    return n


# ---- mixed precision, training: the same sites bound to forms that carry gradients ----------------------------------------------------

class _MixedTrainOps:
    """_MixedOps for training: the 16-bit-storage Functions of ganet_amd.functions.mixed_train (kernels=True) or the cast arm --
    the existing fp32 op between ATen casts, with autograd through both (kernels=False)"""

    def __init__(self, kernels):
        self.kernels = bool(kernels)

    def bn(self, bn, relu, out_dtype=None):
        return MixedTrainBnRelu(bn, relu=relu, out_dtype=out_dtype) if self.kernels else _CastArmBnRelu(bn, relu, out_dtype)

    def cast(self, t, dtype):
        return mixed_train_fn.CastFunction.apply(t.contiguous(), dtype) if self.kernels else t.to(dtype)

    def guidance(self, g, channels):
        if self.kernels:
            return mixed_train_fn.NormalizeGuidanceMixedFunction.apply(g.contiguous(), channels)
        return normalize_guidance(g.float(), channels)

    def filters(self, g):
        return mixed_train_fn.NormalizeFiltersMixedFunction.apply(g.contiguous()) if self.kernels else normalize_filters(g.float())

    def cost_volume(self, cv, x, y):
        if self.kernels:
            return mixed_train_fn.CostVolume16Function.apply(x.contiguous(), y.contiguous(), cv.maxdisp)   # (the module holds maxdisp + 1)
        return type(cv).forward(cv, x.float(), y.float()).to(x.dtype)


def _mixed_train_basicconv_forward(self, x):
    t = self.conv(x)
    return self._mixed_bn(t) if t.dtype in _HALF else self._fused_bn(t)


def _mixed_train_sgablock_forward(self, x, g):
    if g.dtype not in _HALF:
        return _sgablock_forward(self, x, g)
    mx = self._mixed
    if x.dtype != torch.float32:          # (a producer this file does not know: SGA is fp32)
        x = mx.cast(x, torch.float32)
    rem = x
    ks = mx.guidance(g, x.shape[1])       # 16-bit guidance -> four fp32 weight volumes; the gradient comes back in 16 bits
    x = SgaFunction.apply(x.contiguous(), *ks)        # GuidedSGA's path: fp32 in and out, with its backward
    if not self.refine:
        return self._fused_tail(x, rem)
    x = self._mixed_bnrelu(x)             # bn_relu behind SGA: fp32 in and out, BnRelu's training kernels on both arms
    x = self.conv_refine.conv(x)          # autocast rounds the fp32 volume for the convolution (a 16-bit SGA epilogue is out of scope)
    return self._mixed_tail(x, rem) if x.dtype in _HALF else self._fused_tail(x, rem)


def _mixed_train_top_bn_relu_forward(self, x):
    # GANet.bn_relu behind the bilinear up-sampling: fp32 in, 16-bit out.  2-D and small: the cast arm on both settings of `kernels`
    if x.is_cuda and x.dtype == torch.float32 and torch.is_autocast_enabled("cuda"):
        return self._mixed_bn(x).to(torch.get_autocast_dtype("cuda"))
    if x.dtype in _HALF:
        return self._mixed_bn(x.float()).to(x.dtype)
    return type(self).forward(self, x)


def _mixed_train_dispagg_forward(self, x, lg1, lg2):
    mx, tail = self._mixed, self._fused_tail
    v = torch.squeeze(_UP(_conv32x1_f32(self, x), _up_size(self, x)), 1)
    if lg1.dtype not in _HALF:
        return tail(v, lg1, lg2)
    assert lg1.size() == lg2.size()
    f1, f2 = mx.filters(lg1), mx.filters(lg2)
    v = Lga2Function.apply(v, f1, tail.radius)                        # DispAggTail.forward on filters normalised from 16 bits
    v = SoftminFunction.apply(v.contiguous())
    v = LgaFunction.apply(v, f2, tail.radius)
    return LgaRegressFunction.apply(v, f2, tail.radius, tail.ndisp)


def use_mixed_precision_training(model, dtype=torch.bfloat16, kernels=True):
    """Prepares GANet_deep / GANet11 for TRAINING under torch.autocast("cuda", dtype=dtype) -- harness.steps.train_step(..., amp=dtype):
    the sites of use_mixed_precision, bound to forms that carry gradients (ganet_amd.modules.mixed.MixedTrain*, functions.mixed_train).
    The fp32 SGA / LGA / tail Functions, DispConv, DispTail and the loss stay what they are.  Applies use_fused_ops and
    use_fused_bn first where the model has not been rebound; helpers stay out of the module tree (no state_dict key moves).
      BasicConv (use_bn)   a 16-bit convolution output -> MixedTrainBnRelu (batch statistics on 16-bit storage in training mode,
                           MixedBnRelu's fold in eval mode); fp32 (autocast off) -> the BnRelu it had
      ... in front of an SGABlock (the producers of _SGA_PRODUCER, as in use_mixed_precision): out_dtype fp32 -- SGA's x
      SGABlock             guidance through NormalizeGuidanceMixedFunction, SGA on SgaFunction (GuidedSGA's path), bn_relu on BnRelu
                           (fp32 in and out: no cast stands there, so both settings of `kernels` share it), the tail
                           MixedTrainBnRelu(t 16-bit, rem fp32) -> 16-bit
      GANet.cv             CostVolume16Function
      Disp / DispAgg       conv32x1's small output up-cast by CastFunction; filters through NormalizeFiltersMixedFunction
      GANet.conv_refine    its small 16-bit output up-cast by CastFunction in front of the bilinear up-sampling
      GANet.bn_relu        fp32 in, 16-bit out: the cast arm (BnRelu, then .to) -- 2-D and small; a fourth type combination of the
                           training kernels is out of scope
    kernels=False binds every site to the cast arm: the existing fp32 op on .float() inputs followed by .to(out_dtype), with
    autograd -- the fallback, the tests' yardstick and the baseline of the measurement.  Returns the number of sites."""
    if dtype not in _HALF:
        raise TypeError(f"use_mixed_precision_training: dtype is torch.bfloat16 or torch.float16, got {dtype}")
    mods = list(model.modules())
    if not any("_fused_sga" in m.__dict__ for m in mods if type(m).__name__ == "SGABlock"):
        use_fused_ops(model)
    if not any("_fused_bn" in m.__dict__ for m in mods if type(m).__name__ == "BasicConv"):
        use_fused_bn(model)
    mx = _MixedTrainOps(kernels)
    to_f32 = set()
    for m in mods:
        if type(m).__name__ == "CostAggregation":
            for sga, producer in _SGA_PRODUCER.items():
                p = getattr(m, producer, None)
                if hasattr(m, sga) and p is not None:
                    to_f32.add(id(p.conv2 if type(p).__name__ == "Conv2x" else p))
    n = 0
    for m in mods:
        kind = type(m).__name__
        # (object.__setattr__: the helpers stay out of the module tree, state_dict keys do not move)
        if kind == "BasicConv" and m.use_bn:
            object.__setattr__(m, "_mixed_bn", mx.bn(m.bn, bool(m.relu), torch.float32 if id(m) in to_f32 else None))
            m.forward = types.MethodType(_mixed_train_basicconv_forward, m)
            n += 1
        elif kind == "SGABlock":
            object.__setattr__(m, "_mixed", mx)
            object.__setattr__(m, "_mixed_tail", mx.bn(m.conv_refine.bn if m.refine else m.bn, True))
            if m.refine:
                object.__setattr__(m, "_mixed_bnrelu", BnRelu(m.bn_relu[0], relu=True))
            m.forward = types.MethodType(_mixed_train_sgablock_forward, m)
            n += 1
        elif kind == "GetCostVolume":
            object.__setattr__(m, "_mixed", mx)
            m.forward = types.MethodType(_mixed_cv_forward, m)
            n += 1
        elif kind in ("Disp", "DispAgg"):
            object.__setattr__(m, "_mixed", mx)
            m.forward = types.MethodType(_mixed_train_dispagg_forward if kind == "DispAgg" else _mixed_disp_forward, m)
            n += 1
        elif kind == "GANet":
            conv, seq = getattr(m, "conv_refine", None), getattr(m, "bn_relu", None)
            if isinstance(conv, torch.nn.Conv2d):
                object.__setattr__(conv, "_mixed", mx)
                conv.forward = types.MethodType(_mixed_top_conv_forward, conv)
                n += 1
            if isinstance(seq, torch.nn.Sequential) and len(seq) == 2 and isinstance(seq[0], torch.nn.modules.batchnorm._BatchNorm) \
                    and isinstance(seq[1], torch.nn.ReLU):
                object.__setattr__(seq, "_mixed_bn", BnRelu(seq[0], relu=True))
                seq.forward = types.MethodType(_mixed_train_top_bn_relu_forward, seq)
                n += 1
    return n


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


def use_mixed_disp_conv(model, kernels=True, directions=("forward", "data", "weight")):
    """conv32x1 of every Disp and DispAgg on MixedDispConv: DispConv for fp32 input, and for the fp16 / bf16 volume that
    torch.autocast puts in front of it the 16-bit siblings of the same kernels (DispConv16Function: the fp32 weight parameter
    itself, an fp32 output, a 16-bit data gradient rounded once) instead of the library's 16-bit convolution.  kernels=False binds
    the 16-bit case to the cast arm, DispConvFunction on x.float(): the same bits through a cast pass.  `directions`: as
    use_fused_disp_conv's, for both input widths.
    Rebinds `forward` on the Conv3d instance, as use_fused_disp_conv does: it works alone, and before or after any other rebinder
    of this file -- the _conv32x1_f32 of use_mixed_precision / use_mixed_precision_training then meets an fp32 tensor and casts
    nothing.  The helper stays out of the module tree and no state_dict key moves.  The two rebinders of conv32x1 share one slot:
    whichever runs LAST holds the site, so a later use_fused_disp_conv puts the fp32-only DispConv back (a 16-bit input then goes
    to the wrapped convolution again).  Returns the number of sites rebound: 3 on GANet_deep."""
    n = 0
    for m in model.modules():
        if type(m).__name__ in ("Disp", "DispAgg") and isinstance(getattr(m, "conv32x1", None), torch.nn.Conv3d):
            conv = m.conv32x1
            # (object.__setattr__: the helper stays out of the module tree, state_dict keys do not move)
            object.__setattr__(conv, "_fused_conv", mixed_conv_mod.MixedDispConv(conv, directions, kernels))
            conv.forward = types.MethodType(_conv32x1_forward, conv)
            n += 1
    return n


# ---- channels-last: the cost aggregation on [N,D,H,W,C] memory (inference, fp32) ---------------------------------------------------

def _cl_inference_only(m):
    if m.training or torch.is_grad_enabled():
        raise RuntimeError(f"use_channels_last is inference-only: {type(m).__name__} was called in training mode or with autograd on "
                           "(model.eval() under torch.no_grad(), as harness.steps.predict does)")


def _cl_basicconv_forward(self, x):
    _cl_inference_only(self)
    return self._cl_bn(self.conv(x))          # bn + relu in the layout the consumer reads


def _cl_sgablock_forward(self, x, g):
    _cl_inference_only(self)
    rem = x                                   # planar: the producer's ClBnRelu wrote it so
    ks = normalize_guidance(g, x.shape[1])
    x = sga_forward_infer(x.contiguous(), *ks)        # SGA alone: planar in and out, its kernels untouched
    if self.refine:
        x = self._cl_bnrelu(x)                # bn_relu, the merge kernel's expression, on the way to channels-last
        x = self.conv_refine.conv(x)
    return self._cl_tail(x, rem)              # BatchNorm + rem + ReLU


def _cl_cv_forward(self, x, y):
    return self._cl_cv(x, y)


def cl_final_sga(agg):
    """the SGABlock of a CostAggregation whose output the (planar) disparity tail reads: of the full-resolution blocks sga1,
    sga2, ... (one digit; sga11 ... sit a level down) the last -- sga3 in GANet_deep, sga2 in GANet11"""
    blocks = sorted(name for name, m in agg.named_children() if type(m).__name__ == "SGABlock" and len(name) == 4 and name[3].isdigit())
    return blocks[-1] if blocks else None


def use_channels_last(model):
    """Prepares GANet_deep / GANet11 for fp32 inference with the cost aggregation on channels_last_3d tensors -- the layout
    MIOpen's 3-D solvers compute in, so that the library has nothing to repack around a convolution.  Applies use_fused_ops and
    use_fused_bn first where the model has not been rebound; helpers stay out of the module tree (no state_dict key moves).
    Rebinds, in `cost_agg` only:
      GANet.cv             ClGetCostVolume: the same values, written [N,D,H,W,2C]
      BasicConv (3-D, use_bn)   ClBnRelu behind the convolution, whatever layout the convolution answered in (read from strides):
                           planar out for the producers of an SGABlock's input (_SGA_PRODUCER), channels-last out otherwise
      SGABlock             sga_forward_infer WITHOUT its BatchNorm epilogue (planar); that BatchNorm + ReLU is ClBnRelu's
                           planar -> channels-last form (the same expression, the same bits); conv_refine.conv; the tail
                           ClBnRelu(t, rem planar) -> channels-last -- planar for the last block, whose consumer (conv32x1 /
                           DispConv) is planar
      Conv3d / ConvTranspose3d weights of cost_agg   converted once to channels_last_3d (values and state_dict keys unchanged)
    Conv2x's torch.cat needs nothing: both operands are channels-last by construction.  Every site gives the bits of the planar
    site it replaces; the convolutions' solvers may differ between layouts.  Refuses a model in training mode and one bound by
    use_mixed_precision*: 16-bit storage and channels-last do not compose yet.  harness.miopen_env.suggest_channels_last() asks
    PyTorch to hand MIOpen the tensors as they are; call it before the first convolution of the process.
    Returns the number of sites."""
    if model.training:
        raise RuntimeError("use_channels_last is inference-only: call model.eval() first")
    mods = list(model.modules())
    if any("_mixed" in m.__dict__ or "_mixed_bn" in m.__dict__ for m in mods):
        raise RuntimeError("use_channels_last: the model is bound by use_mixed_precision*; channels-last with 16-bit storage is out of scope")
    if not any("_fused_sga" in m.__dict__ for m in mods if type(m).__name__ == "SGABlock"):
        use_fused_ops(model)
    if not any("_fused_bn" in m.__dict__ for m in mods if type(m).__name__ == "BasicConv"):
        use_fused_bn(model)
    aggs = [m for m in mods if type(m).__name__ == "CostAggregation"]
    planar_out, n = set(), 0
    for agg in aggs:
        for sga, producer in _SGA_PRODUCER.items():
            p = getattr(agg, producer, None)
            if hasattr(agg, sga) and p is not None:
                planar_out.add(id(p.conv2 if type(p).__name__ == "Conv2x" else p))
        final = cl_final_sga(agg)
        tails = {id(m.conv32x1) for m in agg.modules() if type(m).__name__ in ("Disp", "DispAgg") and hasattr(m, "conv32x1")}     # planar consumers
        for m in agg.modules():
            kind = type(m).__name__
            # (object.__setattr__: the helpers stay out of the module tree, state_dict keys do not move)
            if kind == "BasicConv" and m.use_bn and isinstance(m.bn, torch.nn.BatchNorm3d):
                fmt = torch.contiguous_format if id(m) in planar_out else torch.channels_last_3d
                object.__setattr__(m, "_cl_bn", ClBnRelu(m.bn, relu=bool(m.relu), out_format=fmt))
                m.forward = types.MethodType(_cl_basicconv_forward, m)
                n += 1
            elif kind == "SGABlock":
                fmt = torch.contiguous_format if final is not None and m is getattr(agg, final) else torch.channels_last_3d
                if m.refine:
                    object.__setattr__(m, "_cl_bnrelu", ClBnRelu(m.bn_relu[0], relu=True, out_format=torch.channels_last_3d, inplace=False))
                object.__setattr__(m, "_cl_tail", ClBnRelu(m.conv_refine.bn if m.refine else m.bn, relu=True, out_format=fmt))
                m.forward = types.MethodType(_cl_sgablock_forward, m)
                n += 1
            elif isinstance(m, (torch.nn.Conv3d, torch.nn.ConvTranspose3d)) and id(m) not in tails:
                m.weight.data = m.weight.data.contiguous(memory_format=torch.channels_last_3d)     # the same values, the same Parameter
    for m in mods:
        if type(m).__name__ == "GetCostVolume" and aggs:
            object.__setattr__(m, "_cl_cv", ClGetCostVolume(m.maxdisp - 1))        # (the module holds maxdisp + 1)
            m.forward = types.MethodType(_cl_cv_forward, m)
            n += 1
    return n
