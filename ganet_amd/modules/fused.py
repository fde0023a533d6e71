"""Fused forms of the op chains around SGA / LGA in models/GANet_deep.py.  Opt-in: the
reference-compatible modules in ganet_amd.modules.GANet are unchanged."""
import torch
from torch.nn.modules.module import Module

from ..functions.fused import (BnApplyFunction, BnReluFunction, DisparityLossFunction, DispConvFunction, LgaRegressFunction, NormDisparityRegressionFunction, ResidualReluFunction,
                               SoftminDisparityRegressionFunction, SoftminFunction, TrilinearUpsampleFunction, UpSoftminRegressionFunction,
                               disparity_loss_workspace, disparity_to_u16, normalize_filters, normalize_guidance, sga_forward_infer,
                               stereo_input, window_f32)
from ..functions.GANet import Lga2Function, LgaFunction, SgaFunction

__all__ = ["GuidedSGA", "GuidedSGABnRelu", "NormalizedLGA2", "NormDisparityRegression", "SoftminDisparityRegression",
           "DispAggTail", "TrilinearUpsample", "DispTail", "DispConv", "ResidualBnRelu", "DisparityLoss", "folded_bn", "BnRelu", "bn_relu_path",
           "StereoInput", "DisparityOutput", "predict_offsets"]


def folded_bn(bn, refresh=False):
    """(scale, shift) with bn(x) == scale[c] * x + shift[c] for a BatchNorm in eval mode (running statistics).  The pair is
    kept on the module and recomputed when any of its tensors has been written since: six tiny launches per call otherwise,
    which is what an SGABlock tail on a 26 MB volume costs altogether.

    What "written since" sees: the autograd version counters of running_mean / running_var / weight / bias (optimizer steps,
    copy_, load_state_dict) AND of num_batches_tracked -- a train-mode forward updates the running statistics inside
    batch_norm without bumping THEIR counters, but the module counts the batch with an in-place add first.  A module met in
    training mode gets its pair dropped and none kept.  All of this is host-side bookkeeping: no launch, no synchronisation
    on the steady eval path.  A write that bypasses the counters altogether (through `.data`, through a raw pointer, or a
    functional batch_norm called on the buffers) is invisible to any host-side key; seeing it would take a comparison of
    values on the device and a synchronisation per call.  After such a write call folded_bn(bn, refresh=True) once."""
    if bn.training:
        bn.__dict__.pop("_ganet_folded", None)
        refresh = True
    src = (bn.running_mean, bn.running_var) + ((bn.weight, bn.bias) if bn.affine else ())
    nbt = getattr(bn, "num_batches_tracked", None)
    key = tuple((t.data_ptr(), t._version) for t in src + ((nbt,) if nbt is not None else ())) + (bn.eps,)
    hit = bn.__dict__.get("_ganet_folded")
    if not refresh and hit is not None and hit[0] == key:
        return hit[1]
    with torch.no_grad():
        scale = torch.rsqrt(bn.running_var + bn.eps)
        if bn.affine:
            scale = scale * bn.weight
            shift = bn.bias - bn.running_mean * scale
        else:
            shift = -bn.running_mean * scale
        pair = (scale.float().contiguous(), shift.float().contiguous())
    if not bn.training:
        bn.__dict__["_ganet_folded"] = (key, pair)   # not a buffer, not a parameter: state_dict keys stay the reference's
    return pair


class GuidedSGA(Module):
    """SGA on the RAW guidance: forward(x [N,C,D,H,W], g [N,20C,H,W]) == SGABlock.forward lines
    models/GANet_deep.py:263-269 (split, view, 4 x F.normalize(p=1, dim=2), SGA)."""

    def forward(self, x, g):
        k1, k2, k3, k4 = normalize_guidance(g, x.shape[1])
        return SgaFunction.apply(x, k1, k2, k3, k4)


class GuidedSGABnRelu(Module):
    """SGABlock.forward lines models/GANet_deep.py:263-271 for refine=True blocks: normalise the guidance, SGA, then
    `bn_relu` = BatchNorm3d + ReLU.  In eval mode without autograd the BatchNorm affine and the ReLU are applied inside
    the direction-merge kernel (no mask / arg-max / saved volumes); otherwise the ops run one after the other."""

    def __init__(self, bn):
        super().__init__()
        self.bn = bn                      # the block's torch.nn.BatchNorm3d (shared, not copied)

    def forward(self, x, g):
        ks = normalize_guidance(g, x.shape[1])
        if self.training or torch.is_grad_enabled() or not self.bn.track_running_stats:
            return torch.relu(self.bn(SgaFunction.apply(x, *ks)))
        return sga_forward_infer(x, *ks, *folded_bn(self.bn))


class ResidualBnRelu(Module):
    """The end of SGABlock.forward (models/GANet_deep.py:270-277): forward(t, rem) == relu(bn(t) + rem) for
    `x = conv_refine(x); x += rem; return relu(x)`, where conv_refine = Conv3d + `bn` (BasicConv(relu=False), :238) and the
    caller passes t = conv_refine.conv(x).  (refine=False blocks, :273: t = the SGA output, bn = the block's own `bn`.)

    Eval mode with frozen statistics: the BatchNorm is folded into a per-channel affine and the whole tail is ONE pass over the
    volumes (stock PyTorch: batch_norm + add_ + relu_ = 7 volume passes, here 3); its backward hands g = grad * [y > 0] to
    `rem` and bn_scale[c] * g to t.  Training mode, or a BatchNorm whose parameters want gradients: `bn` runs in the framework
    (batch statistics, running-stat updates, SyncBatchNorm's collectives all stay what they were) and add + ReLU are fused."""

    def __init__(self, bn, inplace=True):
        super().__init__()
        self.bn = bn                      # the block's BatchNorm3d (shared, not copied)
        self.inplace = inplace            # y overwrites t, as the reference's `x += rem` does (t: the convolution's output)

    def forward(self, t, rem):
        bn = self.bn
        frozen = (not bn.training and bn.track_running_stats and
                  not (torch.is_grad_enabled() and any(p.requires_grad for p in bn.parameters())))
        t, rem = t.contiguous(), rem.contiguous()
        if frozen:
            # autograd refuses an in-place write to a leaf that wants a gradient; anything else (a convolution's output: its
            # backward does not read it) may be overwritten
            inplace = self.inplace and not (torch.is_grad_enabled() and t.requires_grad and t.is_leaf)
            return ResidualReluFunction.apply(t, rem, *folded_bn(bn), inplace)
        return ResidualReluFunction.apply(bn(t), rem, None, None, True)     # bn(t) is a temporary of this call: always in place


def bn_relu_path(bn, x, rem=None):
    """Which way BnRelu(bn) takes for these inputs -- decided on the host from types and flags alone:
      "train"      batch statistics (training mode, or track_running_stats=False): the native training kernels
      "fold"       eval mode with frozen statistics: folded_bn(bn) and the one-pass apply kernel
      "framework"  bn(x) in PyTorch followed by the add and the ReLU: eval mode where the BatchNorm's parameters want
                   gradients; momentum=None (the cumulative average needs a host read of the batch counter); tensors that
                   are not fp32 on a HIP device; a SyncBatchNorm while a process group of more than one rank is initialised
                   (its statistics need a collective between the partial sums and the finishing step)"""
    ts = [x] + ([rem] if rem is not None else []) + [t for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var) if t is not None]
    if any(not t.is_cuda or t.dtype != torch.float32 or t.device != x.device for t in ts) or x.dim() < 3:
        return "framework"
    if bn.training or not bn.track_running_stats:
        if bn.track_running_stats and bn.momentum is None:
            return "framework"
        if isinstance(bn, torch.nn.SyncBatchNorm) and torch.distributed.is_available() and torch.distributed.is_initialized() \
                and torch.distributed.get_world_size() > 1:
            return "framework"
        return "train"
    if torch.is_grad_enabled() and any(p.requires_grad for p in bn.parameters()):
        return "framework"
    return "fold"


class BnRelu(Module):
    """`bn` + optional residual + optional ReLU as one op: forward(x, rem=None) == relu(bn(x) + rem) for the
    `conv -> bn -> F.relu(inplace=True)` of every BasicConv (models/GANet_deep.py:35-41; the caller passes x = conv(..)) and
    for SGABlock's tail (:270-277), for BatchNorm2d and BatchNorm3d.

    Training mode: batch statistics, running-stat update and normalise + add + ReLU in two launches forward and two
    backward (stock PyTorch: about 5 volume passes forward and 8 backward, here 3 and 5); the output is not kept for the
    backward.  Eval mode with frozen statistics: the folded affine, the add and the ReLU in one pass, in place under no_grad.
    Everything else goes to the framework: see bn_relu_path."""

    def __init__(self, bn, relu=True, inplace=True):
        super().__init__()
        if not isinstance(bn, torch.nn.modules.batchnorm._BatchNorm):
            raise TypeError("BnRelu wraps a BatchNorm2d / BatchNorm3d")
        self.bn = bn                      # the caller's BatchNorm (shared, not copied)
        self.relu = relu
        self.inplace = inplace            # eval mode under no_grad: y overwrites x (x: the convolution's output, a temporary)

    def forward(self, x, rem=None):
        bn = self.bn
        path = bn_relu_path(bn, x, rem)
        if path == "framework":
            t = bn(x)
            if rem is not None and self.relu and t.is_cuda and t.dtype == torch.float32 and t.dim() == 5:
                return ResidualReluFunction.apply(t.contiguous(), rem.contiguous(), None, None, True)
            if rem is not None:
                t = t + rem
            return torch.relu(t) if self.relu else t
        x = x.contiguous()
        rem = rem.contiguous() if rem is not None else None
        if path == "fold":
            # in place only where nothing can ask for the overwritten values again
            return BnApplyFunction.apply(x, rem, *folded_bn(bn), self.relu, self.inplace and not torch.is_grad_enabled())
        if bn.training and bn.track_running_stats and bn.num_batches_tracked is not None:
            bn.num_batches_tracked.add_(1)          # as the module does; folded_bn sees the statistics change through it
        running = (bn.running_mean, bn.running_var) if bn.training and bn.track_running_stats else (None, None)
        return BnReluFunction.apply(x, rem, bn.weight, bn.bias, *running, bn.momentum if bn.momentum is not None else 0.0,
                                    bn.eps, self.relu)


class NormalizedLGA2(Module):
    """DispAgg.lga (models/GANet_deep.py:234-237): LGA2(x, F.normalize(g, p=1, dim=1))."""

    def __init__(self, radius=2):
        super().__init__()
        self.radius = radius

    def forward(self, x, g):
        return Lga2Function.apply(x, normalize_filters(g), self.radius)


class NormDisparityRegression(Module):
    """F.normalize(x, p=1, dim=1) + DisparityRegression(maxdisp) in one pass (models/GANet_deep.py:246-247)."""

    def __init__(self, maxdisp):
        super().__init__()
        self.maxdisp = maxdisp + 1

    def forward(self, x):
        return NormDisparityRegressionFunction.apply(x.contiguous(), self.maxdisp)


class SoftminDisparityRegression(Module):
    """Disp.forward after the upsampling (models/GANet_deep.py:217-219): Softmin(dim=1) + DisparityRegression(maxdisp)
    in one pass over the volume (used for the two auxiliary disparities in training)."""

    def __init__(self, maxdisp):
        super().__init__()
        self.maxdisp = maxdisp + 1

    def forward(self, x):
        return SoftminDisparityRegressionFunction.apply(x.contiguous(), self.maxdisp)


class DispAggTail(Module):
    """DispAgg.forward after the trilinear upsampling (models/GANet_deep.py:243-247):
    lga(x, lg1) -> Softmin(dim=1) -> lga(x, lg2) -> F.normalize(p=1, dim=1) -> DisparityRegression.
    The last LGA pass carries the normalise + regression reductions in its epilogue (LgaRegressFunction): three LGA passes,
    one Softmin, one fused pass and a per-pixel division -- under no_grad the final volume is never written."""

    def __init__(self, maxdisp=192, radius=2):
        super().__init__()
        self.radius = radius
        self.ndisp = maxdisp + 1
        self.lga = NormalizedLGA2(radius)

    def forward(self, x, lg1, lg2):
        assert lg1.size() == lg2.size()
        x = self.lga(x, lg1)
        x = SoftminFunction.apply(x.contiguous())
        f2 = normalize_filters(lg2)
        x = LgaFunction.apply(x, f2, self.radius)                       # first pass of the second LGA2
        return LgaRegressFunction.apply(x, f2, self.radius, self.ndisp)  # second pass + normalise + regression


class TrilinearUpsample(Module):
    """F.interpolate(x, size, mode='trilinear', align_corners=False) for [N,C,D,H,W] volumes: the up-sampling in front of
    the Softmin / LGA tails (models/GANet_deep.py:212, 240), with a gather backward (see TrilinearUpsampleFunction)."""

    def forward(self, x, size):
        return TrilinearUpsampleFunction.apply(x.contiguous(), tuple(int(v) for v in size))


class DispTail(Module):
    """Disp.forward behind its conv32x1 (models/GANet_deep.py:214-219) as ONE op: forward(c), c = the convolution's output
    [N,1,D,H,W] (or [N,D,H,W]) -> the disparity map [N, zoom*H, zoom*W] =
    DisparityRegression(Softmin(dim=1)(F.interpolate(c, [maxdisp+1, zoom*H, zoom*W], mode='trilinear'))).  The up-sampled
    volume exists in neither direction (TrilinearUpsample -> SoftminDisparityRegression writes, saves, re-reads and mirrors
    it with a gradient volume); the backward's workspace is a third of it at zoom 3."""

    def __init__(self, maxdisp, zoom=3):
        super().__init__()
        self.ndisp = maxdisp + 1
        self.zoom = zoom

    def forward(self, c):
        H, W = c.shape[-2:]
        return UpSoftminRegressionFunction.apply(c.contiguous(), (self.ndisp, self.zoom * H, self.zoom * W))


class DispConv(Module):
    """The tails' conv32x1 (models/GANet_deep.py:212, 232) on our own kernels: DispConv(conv)(x) == conv(x) for
    conv = nn.Conv3d(C, 1, (3,3,3), (1,1,1), (1,1,1), bias=False), C <= 64.  The module holds the convolution it was given and
    reads conv.weight at every call: the parameter object, its state_dict key and whatever the optimizer holds do not move.
    `directions`: which of "forward", "data" (gradient of the input), "weight" (gradient of the weight) run on the HIP kernels;
    the others stay on ATen.  An fp16 / bf16 input is handed to the convolution itself."""

    def __init__(self, conv, directions=DispConvFunction.ALL):
        super().__init__()
        if not isinstance(conv, torch.nn.Conv3d):
            raise TypeError("DispConv wraps an nn.Conv3d")
        want = dict(out_channels=1, kernel_size=(3, 3, 3), stride=(1, 1, 1), padding=(1, 1, 1), dilation=(1, 1, 1), groups=1,
                    padding_mode="zeros")
        for k, v in want.items():
            assert getattr(conv, k) == v, f"DispConv: the convolution has {k}={getattr(conv, k)}, expected {v}"
        assert conv.bias is None, "DispConv: the convolution has a bias"
        assert conv.in_channels <= 64, f"DispConv: {conv.in_channels} input channels, at most 64"
        directions = tuple(directions)
        if any(d not in DispConvFunction.ALL for d in directions):
            raise ValueError(f"directions: a subset of {DispConvFunction.ALL}")
        self.conv = conv                  # the caller's convolution (shared, not copied)
        self.directions = directions

    def forward(self, x):
        if x.dtype in (torch.float16, torch.bfloat16):
            # mixed-precision inference (torch.autocast): the kernels are fp32, a 16-bit input is the wrapped convolution's.  The
            # class's forward, not the instance's: harness.fuse rebinds the instance's to this module.
            return type(self.conv).forward(self.conv, x)
        return DispConvFunction.apply(x.contiguous(), self.conv.weight.contiguous(), self.directions)


class DisparityLoss(Module):
    """The training criterion of train.py:100-118 with its error read-out (train.py:126, evaluation.py:199-202) as ONE op:
    loss, stats = DisparityLoss(...)(outputs, target), outputs = the model's 1..3 disparity maps [N,H,W].

      loss   = sum_k weights[k] * mean over the valid pixels of rho_k(|outputs[k] - target|)
               kinds[k]: "sl1" (F.smooth_l1_loss) | "myloss2" (MyLoss2(thresh, alpha))
      stats  = [count, then per map: mean rho, mean |r| (end-point error), fraction with |r| > rate_threshold]
               (stats[self.epe_index] is the last map's EPE, what train.py:126 reports); not differentiable
      valid  mask="train": target < max_disp (train.py:100);  "eval": lo <= target <= max_disp (evaluation.py:199)

    No boolean indexing, no host synchronisation: the op can be captured in a graph.  WITHOUT A VALID PIXEL the loss and the
    stats are 0 (stock torch: NaN) and the backward hands all-zero gradients to every map -- what a rank with an empty
    shard needs to run the same backward graph as its peers (harness/steps.py).
    The parameter tensor and the fp64 workspace are kept per device; the workspace is in use from the call until its two
    launches have run, so one instance serves one stream at a time."""

    KINDS = {"sl1": 0, "myloss2": 1}

    def __init__(self, max_disp, weights, kinds, thresh=3, alpha=2, rate_threshold=3.0, mask="train", lo=0.001):
        super().__init__()
        if not 1 <= len(weights) <= 3 or len(kinds) != len(weights):
            raise ValueError("1..3 weights with one kind each")
        if mask not in ("train", "eval"):
            raise ValueError('mask: "train" | "eval"')
        self.kinds = tuple(self.KINDS[k] for k in kinds)
        self.mask_mode = 0 if mask == "train" else 1
        w = [float(v) for v in weights] + [0.0] * (3 - len(weights))
        self.values = [float(max_disp), float(lo)] + w + [float(thresh), float(alpha), float(rate_threshold)]
        self.epe_index = 3 * (len(weights) - 1) + 2
        self._params, self._workspace = {}, {}

    @classmethod
    def ganet_deep(cls, max_disp=192, kitti=True, **kw):
        """train.py:106-111: 0.2 * sl1(disp0) + 0.6 * sl1(disp1) + L(disp2), L = MyLoss2(thresh=3, alpha=2) on KITTI, else sl1"""
        return cls(max_disp, (0.2, 0.6, 1.0), ("sl1", "sl1", "myloss2" if kitti else "sl1"), thresh=3, alpha=2, **kw)

    @classmethod
    def ganet11(cls, max_disp=192, kitti=True, **kw):
        """train.py:112-118: 0.4 * sl1(disp1) + 1.2 * L(disp2)"""
        return cls(max_disp, (0.4, 1.2), ("sl1", "myloss2" if kitti else "sl1"), thresh=3, alpha=2, **kw)

    @classmethod
    def for_model(cls, name, max_disp=192, kitti=True, **kw):
        return (cls.ganet11 if name == "GANet11" else cls.ganet_deep)(max_disp, kitti, **kw)

    def forward(self, outputs, target):
        outputs = [o.contiguous() for o in outputs]
        target = target.contiguous()
        dev = target.device
        if dev not in self._params:
            self._params[dev] = torch.tensor(self.values, dtype=torch.float32).to(dev)
        need = (dev, tuple(target.shape))
        if need not in self._workspace:
            self._workspace[need] = disparity_loss_workspace(target, *target.shape)
        return DisparityLossFunction.apply(target, self._params[dev], self._workspace[need], self.kinds, self.mask_mode, *outputs)


def predict_offsets(h, w, crop_height, crop_width):
    """(oy, ox) of predict.py:75-90 for an [h, w] image: output pixel (y, x) is image pixel (y + oy, x + ox).  An image no
    larger than the crop sits in the bottom-right corner (oy = h - Hc, ox = w - Wc, both <= 0); one larger BOTH ways is
    centre-cropped with int((w - Wc) / 2).  Larger one way only: the reference takes its crop branch with a negative start,
    which slices from the far end and returns an array of another shape; here it is a ValueError."""
    if h <= crop_height and w <= crop_width:
        return h - crop_height, w - crop_width
    if h > crop_height and w > crop_width:
        return int((h - crop_height) / 2), int((w - crop_width) / 2)
    raise ValueError(f"a {h}x{w} image is larger than the {crop_height}x{crop_width} crop one way and not the other: "
                     "the reference's test_transform has no answer for it")


class StereoInput(Module):
    """The front end of predict.py as one op: forward(left_u8, right_u8) == test_transform(load_data(..)) (predict.py:92-114,
    :75-90) for two uint8 images [H, W, 3 | 4] ON THE DEVICE: every channel standardised, padded to the bottom-right or
    centre-cropped to [crop_height, crop_width].  Returns (left, right, (h, w)), fp32 [1, 3, Hc, Wc] each.
    A constant channel gives 0 where the reference has NaN (its std is 0).  Two launches, no host synchronisation,
    capturable, any stream; uint8 tensors on a HIP device only."""

    def __init__(self, crop_height, crop_width):
        super().__init__()
        self.crop_height, self.crop_width = int(crop_height), int(crop_width)

    def forward(self, left_u8, right_u8):
        h, w = left_u8.shape[:2]
        oy, ox = predict_offsets(h, w, self.crop_height, self.crop_width)
        left, right = self.window(left_u8, right_u8, oy, ox, ox)
        return left[None], right[None], (h, w)

    def window(self, left_u8, right_u8, oy, ox_left, ox_right, out_left=None, out_right=None):
        """The same with explicit offsets: the training crop of dataloader/dataset.py:64-92 (oy = start_y - pad_y,
        ox_right = start_x - pad_x, ox_left = ox_right + shift_x).  Returns fp32 [3, Hc, Wc] each, written to out_left /
        out_right where given (slices of batch tensors)."""
        return stereo_input(left_u8, right_u8, (self.crop_height, self.crop_width), oy, ox_left, ox_right, out_left, out_right)

    def target_window(self, disp, oy, ox, sub=0.0, fill=1000.0):
        """The training target under the same crop (dataset.py:53-74): disp [H, W] fp32 -> [Hc, Wc], `fill` outside the
        map, `sub` subtracted inside (the reference lowers the whole crop by shift_x: sub = shift_x, fill = 1000 - shift_x)."""
        return window_f32(disp, (self.crop_height, self.crop_width), oy, ox, sub, fill)


class DisparityOutput(Module):
    """The back end of predict.py:132-138: forward(disp [1, Hc, Wc] or [Hc, Wc] fp32, (h, w)) -> torch.uint16 [h, w], the
    padding of StereoInput taken off again (a cropped image keeps the whole map), values scaled by 256 and truncated.
    Values below 0 and NaN give 0, 65536 and above 65535; the reference's astype('uint16') wraps there."""

    def __init__(self, scale=256.0):
        super().__init__()
        self.scale = float(scale)

    def forward(self, disp, hw):
        if disp.dim() == 3 and disp.shape[0] == 1:
            disp = disp[0]
        Hc, Wc = disp.shape
        h, w = hw
        if h <= Hc and w <= Wc:
            return disparity_to_u16(disp.contiguous(), (h, w), Hc - h, Wc - w, self.scale)
        return disparity_to_u16(disp.contiguous(), (Hc, Wc), 0, 0, self.scale)
