"""TEST INFRASTRUCTURE: records of the mixed-precision kinds of tests/model_calls.py, built WITHOUT a device -- the Functions of
ganet_amd.functions.mixed_train refuse CPU tensors, so tests/test_model_calls_cpu.py calibrates their checkers on a numpy model, as
tests/test_large_cases_cpu.py does for the large shapes.

Data: what the CPU-oracle twin of tests/standin_net.py hands to each site at its 48 x 96 crop (convolution outputs, guidance and
filter maps, feature maps, and the gradients that reached them), rounded to bf16 / fp16 by mixed_cases.convert.  Model: each
table's own statement -- the fp32 statement of the op on the up-cast input, evaluated in float32, converted ONCE where the result
is stored in 16 bits (tests/mixed_cases.py, tests/mixed_train_cases.py).  Every 16-bit result keeps the float32 value it was rounded
from (`Record.pre`), so that the mutations can round it another way:
  zeros      an all-zero output or gradient
  truncated  the 16-bit store truncates toward zero instead of rounding to nearest
  twice      the value is rounded twice: first to an intermediate grid, then to the format.  bf16: through fp16's 11-bit grid, three
             bits more than its own 8 (what fp32 -> fp16 -> bf16 does).  The result differs from the single rounding only where the
             first rounding lands on a tie of the second, about one element in 16, and then by one ulp of the format -- which puts
             it between 1/2 and 9/16 ulp from the float32 value: an excess over half an ulp of up to 2^-12 |v|, far above every fp32
             part of a bar.  fp16: through a 12-bit grid, ONE bit more than its own 11 (one element in 4 differs, the excess
             reaches 1/4 ulp, 2^-13 .. 2^-12 of |v|).  With three more bits the excess would stay below 2^-15 |v|, under the
             rtol = 1e-4 that the L1 adjoint's fp32 bar has and keeps: that finer double rounding of an fp16 gx is NOT seen by
             check_l1_mixed, by this arithmetic; every other 16-bit result here has an fp32 part of 2^-20 or less and sees both.
             MIN_TWICE elements must differ for the mutation to count as applied; every record here has thousands.
  x256       a gradient left at the wrong power of the GradScaler's scale
  one term   the cost-volume adjoint without its last plane, the L1 adjoint without its sign term, BatchNorm's grad_x without its
             mean term"""
import copy

import numpy as np
import torch

import bn_ref64
import mixed_cases as mxc
import mixed_train_cases as mtc
import model_calls as M

F32 = np.float32
FMTS = (mxc.BF16, mxc.F16)
TORCH = {mxc.F32: torch.float32, mxc.F16: torch.float16, mxc.BF16: torch.bfloat16}
SCALE = {mxc.BF16: 1.0, mxc.F16: 256.0}            # fp16 trains under GradScaler(init_scale=256): its gradients carry the scale
MIN_TWICE = 8
# the BasicConvs whose output is an SGABlock's x (harness.fuse._SGA_PRODUCER on the stand-in): y and grad_y are fp32 there
PRE_SGA = ("cost_agg.conv_start", "cost_agg.conv1a", "cost_agg.deconv1a.conv2", "cost_agg.deconv1b.conv2")


def half(a, fmt):
    """float32 values -> the recorder's 16-bit array, rounded to nearest even once"""
    a = np.asarray(a, F32)
    return M.Half(mxc.convert(a, fmt).reshape(a.shape), fmt)


def truncated(a, fmt):
    """float32 -> 16-bit patterns, toward zero (both formats are sign-magnitude: one pattern down is one step toward zero)"""
    a = np.ascontiguousarray(a, F32)
    if fmt == mxc.BF16:
        return M.Half((a.view(np.uint32) >> 16).astype(np.uint16).reshape(a.shape), fmt)
    h = mxc.convert(a, fmt).reshape(a.shape)
    beyond = np.abs(mxc.up(h, fmt).reshape(a.shape).astype(np.float64)) > np.abs(a.astype(np.float64))
    return M.Half(np.where(beyond, h - np.uint16(1), h), fmt)


def twice(a, fmt):
    """float32 -> the intermediate grid (11 significant bits for bf16, 12 for fp16; nearest even, on the float32 pattern) -> the
    format (nearest even)"""
    a = np.ascontiguousarray(a, F32)
    drop = 24 - (11 if fmt == mxc.BF16 else 12)
    u = a.view(np.uint32).astype(np.uint64)
    u = ((u + np.uint64((1 << (drop - 1)) - 1) + ((u >> np.uint64(drop)) & np.uint64(1))) >> np.uint64(drop)) << np.uint64(drop)
    return half(u.astype(np.uint32).view(F32).reshape(a.shape), fmt)


def record(kind, args, outputs, grad_out=None, grad_in=None, pre=None, **extra):
    r = M.Record(kind, args, grad_out is not None)
    r.outputs, r.grad_out, r.grad_in = outputs, grad_out, grad_in
    r.pre = pre or {}                       # (attribute, index) -> the float32 array a 16-bit result was rounded from
    for k, v in extra.items():
        setattr(r, k, v)
    return r


# ---- the records --------------------------------------------------------------------------------------------------------------------
def cast_records(t32, g32, fmt):
    """CastFunction 16 -> 32 with its backward 32 -> 16 (conv32x1's output in front of the tails), and `cast` 32 -> 16 (the images)"""
    t = half(t32, fmt)
    g = (g32 * F32(SCALE[fmt])).astype(F32)
    return [record("CastFunction", [t, torch.float32], [M.up(t)], [g], [half(g, fmt), None], pre={("grad_in", 0): g}),
            record("cast", [np.asarray(t32, F32), TORCH[fmt]], [half(t32, fmt)], pre={("outputs", 0): np.asarray(t32, F32)})]


def _cost_adjoint32(g, C, W, planes):
    N, _, Dn, H, _ = g.shape
    gx, gy = np.zeros((N, C, H, W), F32), np.zeros((N, C, H, W), F32)
    for i in range(planes):                      # one fp32 addition per plane, in order
        gx[..., i:] += g[:, :C, i, :, i:]
        gy[..., :W - i] += g[:, C:, i, :, i:]
    return gx, gy


def cost_volume_records(s, fmt):
    """s: the stand-in's cost-volume site (x, y, Dn, g).  CostVolume16Function with its adjoint; cost_volume_16 forward only"""
    x, y, Dn = half(s["x"], fmt), half(s["y"], fmt), s["Dn"]
    N, C, H, W = x.shape
    cost = np.zeros((N, 2 * C, Dn, H, W), np.uint16)
    for i in range(min(Dn, W)):
        cost[:, :C, i, :, i:], cost[:, C:, i, :, i:] = np.asarray(x)[..., i:], np.asarray(y)[..., :W - i]
    cost = M.Half(cost, fmt)
    g = half(s["g"] * F32(SCALE[fmt]), fmt)
    gx, gy = _cost_adjoint32(M.up(g), C, W, min(Dn, W))
    r = record("CostVolume16Function", [x, y, Dn], [cost], [g], [half(gx, fmt), half(gy, fmt), None],
               pre={("grad_in", 0): gx, ("grad_in", 1): gy})
    mx, my = _cost_adjoint32(M.up(g), C, W, min(Dn, W) - 1)
    r.one_term = {("grad_in", 0): half(mx, fmt), ("grad_in", 1): half(my, fmt)}
    return [r, record("cost_volume_16", [x, y, Dn], [cost])]


def l1_records(raw32, G, C, K, gys, fmt, train_kind, infer_kind):
    """raw32: a guidance [N,20C,H,W] or filter [N,K,H,W] map; gys: the fp32 gradients that reached its G normalised groups"""
    x = half(raw32, fmt)
    x32 = M.up(x)
    N, _, H, W = x32.shape
    x6 = x32.reshape(N, G, C, K, H, W)
    s = np.maximum(np.abs(x6).sum(3, keepdims=True, dtype=F32), F32(1e-12))
    y = x6 / s
    shape = (N, C, K, H, W) if G > 1 else (N, K, H, W)
    outs = [np.ascontiguousarray(y[:, g]).reshape(shape) for g in range(G)]
    gy = np.stack([(g * F32(SCALE[fmt])).astype(F32).reshape(N, C, K, H, W) for g in gys], 1)
    dot = (gy * y).sum(3, keepdims=True, dtype=F32)
    gx = ((gy - np.sign(x6) * dot) / s).astype(F32).reshape(x32.shape)
    args = [x, C] if G > 1 else [x]
    r = record(train_kind, args, outs, [np.ascontiguousarray(gy[:, g]).reshape(shape) for g in range(G)], [half(gx, fmt)] + [None] * (len(args) - 1),
               pre={("grad_in", 0): gx})
    r.one_term = {("grad_in", 0): half((gy / s).astype(F32).reshape(x32.shape), fmt)}          # without sgn(x) sum_u gy_u y_u
    return [r, record(infer_kind, args, outs)]


def _site_kind(s):
    return "tail" if s["rem"] is not None else "pre-sga" if s["name"] in PRE_SGA else "conv"


def bn_train_record(s, fmt):
    """s: a BatchNorm site of the stand-in's training step.  bn_ref64.Float32Model on the up-cast x -- fp64 sums, fp32 elements --
    with y from model_calls.mixed_bn_z32 on the model's statistics, rounded once to the site's storage"""
    kind = _site_kind(s)
    y_fmt = mxc.F32 if kind == "pre-sga" else fmt
    x = half(s["x"], fmt)
    N, C = x.shape[:2]
    flat = lambda a: None if a is None else np.ascontiguousarray(a, F32).reshape(N, C, -1)      # noqa: E731
    g = (s["g"] * F32(SCALE[fmt])).astype(F32)
    gy = g if y_fmt == mxc.F32 else half(g, fmt)
    m = bn_ref64.Float32Model(flat(M.up(x)), flat(s["rem"]), flat(M.up(gy)), s["weight"], s["bias"], s["running_mean"], s["running_var"],
                              s["momentum"], s["eps"], s["relu"])
    z = M.mixed_bn_z32(flat(M.up(x)), flat(s["rem"]), s["weight"], s["bias"], m.save_mean, m.save_invstd)
    y32 = (np.where(z <= 0, F32(0), z) if s["relu"] else z).reshape(x.shape)
    gx32 = np.ascontiguousarray(m.grad_x, F32).reshape(x.shape)
    grem = np.ascontiguousarray(m.grad_rem, F32).reshape(x.shape) if s["rem"] is not None else None
    pre = {("grad_in", 0): gx32}
    if y_fmt != mxc.F32:
        pre["outputs", 0] = y32
    r = record("MixedBnReluFunction", [x, s["rem"], s["weight"], s["bias"], s["running_mean"], s["running_var"], s["momentum"], s["eps"], s["relu"],
                                       torch.float32 if kind == "pre-sga" else None],
               [y32 if y_fmt == mxc.F32 else half(y32, fmt)], [gy], [half(gx32, fmt), grem, m.grad_weight, m.grad_bias] + [None] * 6, pre=pre,
               saved={"mean": m.save_mean, "invstd": m.save_invstd}, after={4: m.running_mean, 5: m.running_var}, site=kind)
    # grad_x without its mean term k1 = sum g / M, from the float64 statement of the same call
    ref = bn_ref64.Reference(flat(M.up(x)), flat(s["rem"]), flat(M.up(gy)), s["weight"], s["bias"], s["running_mean"], s["running_var"],
                             s["momentum"], s["eps"], s["relu"], relu_positive=z > 0)
    r.one_term = {("grad_in", 0): half((ref.scale[None, :, None] * (ref.g - ref.xm * ref.q[None, :, None])).astype(F32).reshape(x.shape), fmt)}
    return r


def bn_apply_record(e, fmt):
    """e: a BatchNorm site of the stand-in's steps.predict: the folded BatchNorm in float32 on the up-cast x, rounded once; in place
    where the output has x's type (ganet_amd.modules.mixed.MixedBnRelu's default)"""
    kind = _site_kind(e)
    x = half(e["x"], fmt)
    scale = (e["weight"].astype(F32) / np.sqrt(e["running_var"] + F32(e["eps"]), dtype=F32)).astype(F32)
    shift = (e["bias"] - e["running_mean"] * scale).astype(F32)
    C = x.shape[1]
    b = lambda v: v.reshape((1, C) + (1,) * (x.ndim - 2))      # noqa: E731
    y = mtc.fma32(M.up(x), b(scale), b(shift))
    y = y if e["rem"] is None else (y + e["rem"]).astype(F32)
    y = np.maximum(y, F32(0)) if e["relu"] else y
    out = torch.float32 if kind == "pre-sga" else TORCH[fmt]
    return record("bn_apply_mixed", [x, e["rem"], scale, shift, e["relu"], out, kind != "pre-sga"], [y if kind == "pre-sga" else half(y, fmt)],
                  pre={} if kind == "pre-sga" else {("outputs", 0): y}, site=kind)


# ---- the mutations ------------------------------------------------------------------------------------------------------------------
def spoilt(r, slot, value):
    attr, i = slot
    s = copy.copy(r)
    held = copy.copy(getattr(r, attr))
    held[i] = value
    setattr(s, attr, held)
    s.reference = None
    return s


def _times256(a):
    if isinstance(a, M.Half):
        with np.errstate(over="ignore"):
            return half(M.up(a) * F32(256), a.fmt)
    return (a * F32(256)).astype(a.dtype)


def mutations(r):
    """[(name, slot, the spoilt record)] -- every listed mutation that applies to this record"""
    res = []
    slots = [("outputs", i) for i, o in enumerate(r.outputs) if isinstance(o, np.ndarray)]
    grads = [("grad_in", i) for i, g in enumerate(r.grad_in or ()) if g is not None]
    for slot in slots + grads:
        a = getattr(r, slot[0])[slot[1]]
        if np.any(a):
            res.append(("zeros", slot, spoilt(r, slot, np.zeros_like(a))))
    for slot, f in r.pre.items():
        fmt = getattr(r, slot[0])[slot[1]].fmt
        good = getattr(r, slot[0])[slot[1]]
        t = truncated(f, fmt)
        assert (np.asarray(t) != np.asarray(good)).any(), (r, slot, "truncation changes nothing: no value was rounded up")
        res.append(("truncated", slot, spoilt(r, slot, t)))
        w = twice(f, fmt)
        assert int((np.asarray(w) != np.asarray(good)).sum()) >= MIN_TWICE, (r, slot, "too few elements for the double rounding to show")
        res.append(("twice", slot, spoilt(r, slot, w)))
    for slot in grads:
        a = getattr(r, slot[0])[slot[1]]
        if np.any(a):
            res.append(("x256", slot, spoilt(r, slot, _times256(a))))
    for slot, a in getattr(r, "one_term", {}).items():
        res.append(("one term", slot, spoilt(r, slot, a)))
    return res
