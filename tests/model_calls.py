"""TEST INFRASTRUCTURE: every guided-aggregation op call of a MODEL run, held to the float64 statement of its operation --
shared by tests/test_model_calls_cpu.py (the CPU-oracle twin: the yardstick alone, and its teeth),
tests/test_gpu_model_calls.py (the product, call by call, on the reference's models) and tests/test_gpu_standin_calls.py (the same
on the stand-in network of tests/standin_net.py, which needs no reference file: `run_model` takes any ready model and the
rebinders of harness.fuse to apply, in a given order).

Why: the per-op case tables feed inputs of magnitude about 1 and hold gradients to parity_cases.TOL = 1e-4 ABSOLUTE; a model
drives the ops with gradients of 1e-2 .. 1e-4, where that bar lets an all-zero LGA2 data gradient through.  The float64
statements (sga_ref64, lga_ref64.chain_bound, misc_ref64, bn_ref64, loss_ref64, disp_tail_ref64, disp_conv_ref64) scale with
the data, so they are applied here to the tensors a model run really hands to each op.

`recording` wraps forward / backward of a list of autograd Functions (and plain launch functions) for its duration and keeps
one `Record` per call: kind, arguments (host copies of the tensors, cloned BEFORE the call), outputs, incoming and returned
gradients, SgaFunction's saved A / mask / kp, LgaRegressFunction's saved y / snorm, and every input that was written.  `check_all(records, oracle)` runs each
record through the checker of its kind and FAILS, naming the kinds, if a recorded call has none: no op call of a model run
goes unexamined.

The checkers evaluate the statements on the RECORDED inputs (which came from the device), never on regenerated ones.  SGA
and LGA are split in two -- `*_reference(record)` (the expensive float64 side, computed once) and `*_judge(reference, got)`
-- so that the CPU test can hand the same reference results that are wrong on purpose.

Absolute bars of the case tables (misc_cases: `atol`) belong to data of magnitude about 1 (randn, dyadic grids).  The absolute
error of an fp32 operation scales with its data, down as well as up -- an absolute bar below one ulp of the data cannot be
met by any fp32 code, and one far above the data checks nothing -- so on recorded data the bar becomes
atol * max |float64 result| of that output (`_atol`).  The regressions' outputs are in disparity units: their 1e-4 was set for
disparities up to 192 and becomes 1e-4 * (D - 1) / 192 (`_atol_px`).  The relative parts (`rtol`) stay as they are.

Non-smooth points.  A reference may apply a sign, a threshold or a selection to an EXACT input, never to a quantity the op
computed itself: there float64 and a correct fp32 evaluation can land on different sides, and the two results differ by far
more than any rounding bar.  The checkers were read for this.  check_lga_regress had it -- sgn(y) of the pass's own fp32 y,
taken from the float64 y -- and now takes the call's sign where float64 cannot decide (its docstring).  The others do not:
NormDisparityRegression, L1NormalizeGroups and their adjoints take sgn of the recorded input, and their clamp at eps = 1e-12 acts
on a sum of |inputs| that model data only reach as an exact zero; ResidualRelu and BnApply take the ReLU mask of the backward from
the call's own y, and hold the forward's zero set only outside the bar; BnRelu has `undecided` with the call's mask; SGA's
arg-max is the oracle's, held by equality, and float64 is evaluated on those selections; the losses' thresholds act on
fl32(p - t), one defined rounding of exact inputs that both sides perform alike; Softmin, the regressions, the cost volume
and the convolution are smooth or linear; trilinear interpolation is continuous across its cell boundaries (the weight of the
cell that changes is 0 there), and its reference is ATen's own fp32 index arithmetic.

Mixed precision.  A step under torch.autocast (`run_model(amp=, scaler=, mixed=)`: harness.steps.predict / train_step themselves) is
recorded the same way: the Functions of ganet_amd.functions.mixed_train and the launch functions of ganet_amd.functions.mixed are
wrapped, a 16-bit tensor is kept as its bit patterns with a format tag (`Half`; `up` is the exact up-cast; no ATen cast stands in
the recorder), and each 16-bit form is held to the float64 statement of the CORRESPONDING fp32 op on the up-cast inputs, a 16-bit
output getting half an ulp of its format on top of the fp32 kind's bar (the section in front of CHECKERS).  The fp32 kinds
inside such a step -- on rounded activations and, under a GradScaler, on gradients that carry its scale -- go through the
checkers they have.  tests/test_gpu_mixed_calls.py runs it on the device, tests/mixed_call_cases.py is the numpy model the
checkers are calibrated on."""
import collections
import contextlib
import inspect
import types

import numpy as np
import torch

import bn_cases
import bn_ref64
import disp_conv_cases
import disp_conv_ref64
import disp_tail_cases
import disp_tail_ref64
import io_cases
import io_ref64
import lga_ref64
import loss_cases
import loss_ref64
import misc_cases as mc
import misc_ref64 as m64
import mixed_cases as mxc
import mixed_train_cases as mtc
import sga_ref64_cases as sc
import value_cases as vc

U = 2.0 ** -24
FACTOR = sc.FACTOR                      # the project's allowance for the second-order terms of a first-order bound
ONE_ROUNDING = U * (1 + 2.0 ** -20)     # |fl32(s) - s| <= u |s|; the margin covers the float64 evaluation of s itself


# ---- the recorder ---------------------------------------------------------------------------------------------------------------
class Record:
    """one op call.  args: the call's positional arguments in order, tensors as host arrays cloned before the call;
    outputs / grad_out / grad_in: lists of host arrays (None where autograd passed or got None); saved: name -> array;
    written: [(phase, what)] -- every input (or incoming gradient) whose values differ after the phase from before it"""

    def __init__(self, kind, args, needs_grad):
        self.kind, self.args, self.needs_grad = kind, args, needs_grad
        self.outputs, self.grad_out, self.grad_in, self.saved, self.written = None, None, None, {}, []
        self.live, self.after, self.reference = None, {}, None

    def __repr__(self):
        shapes = [tuple(a.shape) for a in self.args if isinstance(a, np.ndarray)]
        return f"{self.kind}{shapes}"


class Half(np.ndarray):
    """a 16-bit tensor as the recorder keeps it: its bit patterns (uint16) with the format tag `fmt` (mixed_cases.F16 / BF16).
    numpy has no bfloat16 and an ATen cast would be an operation of the product standing inside its own check, so the bits
    travel as they are; `up(a)` is mixed_cases' exact up-cast.  Views, copies and zeros_like keep the tag."""

    def __new__(cls, bits, fmt):
        a = np.asarray(bits, np.uint16).view(cls)
        a.fmt = fmt
        return a

    def __array_finalize__(self, obj):
        self.fmt = getattr(obj, "fmt", None)


_TORCH_FMT = {torch.float32: mxc.F32, torch.float16: mxc.F16, torch.bfloat16: mxc.BF16}


def fmt_of(a):
    return a.fmt if isinstance(a, Half) else mxc.F32


def up(a):
    """the float32 values of a recorded array: exact for a Half, the array itself otherwise (None stays None)"""
    return mxc.up(np.asarray(a), a.fmt).reshape(a.shape) if isinstance(a, Half) else a


def _bits(t):
    t = t.detach().cpu()
    if t.dtype in (torch.float16, torch.bfloat16):
        return Half(t.contiguous().view(torch.int16).numpy().view(np.uint16), _TORCH_FMT[t.dtype])
    return t.numpy()


def _host(t):
    return _bits(t).copy() if isinstance(t, torch.Tensor) else t


def _seq(v):
    return list(v) if isinstance(v, (tuple, list)) else [v]


def _same(t, before):
    now = _bits(t)
    return now.shape == before.shape and now.dtype == before.dtype and fmt_of(now) == fmt_of(before) \
        and now.tobytes() == before.tobytes()                                                               # bits: a NaN is itself


def _changed(tensors, before, phase, prefix, record):
    """notes what was written; -> index -> the values found afterwards"""
    after = {}
    for i, (t, b) in enumerate(zip(tensors, before)):
        if isinstance(t, torch.Tensor) and not _same(t, b):
            record.written.append((phase, f"{prefix}{i}"))
            after[i] = _host(t)
    return after


def _wrap_function(patch, records, cls):
    fwd, bwd, kind = cls.forward, cls.backward, cls.__name__

    def forward(ctx, *args):
        r = Record(kind, [_host(a) for a in args], any(getattr(ctx, "needs_input_grad", ())))
        out = fwd(ctx, *args)
        r.outputs = [_host(o) for o in _seq(out)]
        r.after = _changed(args, r.args, "forward", "arg", r)
        r.live = [a for a in args if isinstance(a, torch.Tensor)]
        ctx._model_call = r
        records.append(r)
        return out

    def backward(ctx, *grads):
        r = ctx._model_call
        r.grad_out = [_host(g) for g in grads]
        if kind == "SgaFunction" and not ctx.recompute:
            A, mask, kp = ctx.saved_tensors[5:8]
            r.saved = {"A": _host(A), "mask": _host(mask), "kp": _host(kp).view(np.uint16)}
        elif kind == "SgaFunction":
            tmp, mask = ctx.saved_tensors[5:7]
            r.saved = {"tmp": _host(tmp), "mask": _host(mask)}
        elif kind == "LgaRegressFunction":             # the pass's own volume and norm: the call's signs (check_lga_regress)
            r.saved = {"y": _host(ctx.saved_tensors[2]), "snorm": _host(ctx.saved_tensors[4])}
        elif kind == "MixedBnReluFunction":            # the call's own statistics: y is held to THEIR fp32 expression, bit for bit
            r.saved = {"mean": _host(ctx.saved_tensors[4]), "invstd": _host(ctx.saved_tensors[5])}
        # (between forward and backward other ops may legitimately write an input -- BatchNorm's running statistics on the
        # next call of a shared module -- so the backward is compared with what it found, not with the forward's clones)
        before = [_host(t) for t in r.live]
        res = bwd(ctx, *grads)
        r.grad_in = [_host(g) if isinstance(g, torch.Tensor) else None for g in _seq(res)]
        _changed(r.live, before, "backward", "tensor", r)
        _changed(grads, r.grad_out, "backward", "grad_out", r)
        return res

    patch.setattr(cls, "forward", staticmethod(forward))
    patch.setattr(cls, "backward", staticmethod(backward))


def _wrap_plain(patch, records, owners, name):
    orig = getattr(owners[0], name)
    sig = inspect.signature(orig)

    def call(*args, **kw):
        bound = sig.bind(*args, **kw)
        bound.apply_defaults()
        vals = list(bound.arguments.values())
        r = Record(name, [_host(a) for a in vals], False)
        out = orig(*args, **kw)
        r.outputs = [_host(o) for o in _seq(out)]
        _changed(vals, r.args, "forward", "arg", r)
        records.append(r)
        return out

    for owner in owners:
        assert getattr(owner, name) is orig, (owner, name)
        patch.setattr(owner, name, call)


@contextlib.contextmanager
def recording(monkeypatch, functions, plain=()):
    """functions: autograd Function classes; plain: (modules that hold the name, name) of functions that launch a kernel without
    a Function.  Yields the list the records are appended to; nothing stays patched afterwards (pytest's monkeypatch)."""
    records = []
    with monkeypatch.context() as patch:
        for cls in dict.fromkeys(functions):
            _wrap_function(patch, records, cls)
        for owners, name in plain:
            _wrap_plain(patch, records, owners, name)
        yield records


def product_functions():
    """everything in ganet_amd.functions.GANet.__all__, every Function of ganet_amd.functions.fused, and the plain functions
    that launch a kernel without one: the two inference forms of SGA and the image front and back end; the mixed-precision
    forms: every Function of ganet_amd.functions.mixed_train and the five launch functions of ganet_amd.functions.mixed (owners:
    every module that binds the name -- harness.fuse and harness.steps reach `cast` and the normalisations through the module)"""
    import ganet_amd.functions.fused as ff
    import ganet_amd.functions.GANet as fg
    import ganet_amd.functions.mixed as fm
    import ganet_amd.functions.mixed_train as ft
    import ganet_amd.modules.fused as mf
    import ganet_amd.modules.mixed as mm
    from harness import fuse
    fns = [getattr(fg, n) for n in fg.__all__]
    fns += [v for v in vars(ff).values() if isinstance(v, type) and issubclass(v, torch.autograd.Function) and v.__module__ == ff.__name__]
    fns += [getattr(ft, n) for n in ft.__all__]
    # (harness.fuse binds sga_forward_infer by name for the mixed-precision inference forward: without it among the owners the
    # four calls of such a pass go unrecorded -- found by the binder census of tests/test_model_calls_cpu.py)
    return fns, [((fg, ff), "_sga_infer"), ((ff, mf, fuse), "sga_forward_infer"), ((ff, mf), "stereo_input"), ((ff, mf), "window_f32"),
                 ((ff, mf), "disparity_to_u16"), ((fm,), "cast"), ((fm, mm), "bn_apply_mixed"), ((fm, mm), "cost_volume_16"),
                 ((fm,), "normalize_guidance_mixed"), ((fm,), "normalize_filters_mixed")]


MIXED_PLAIN = ("cast", "bn_apply_mixed", "cost_volume_16", "normalize_guidance_mixed", "normalize_filters_mixed")


REBINDERS = ("use_fused_ops", "use_fused_bn", "use_fused_disp_tail", "use_fused_disp_conv")


def run_model(monkeypatch, model, batch, max_disp, rebinders=(), name="GANet_deep", fused_loss=None, amp=None, scaler=None, mixed=None,
              kernels=True):
    """A ready model (already on its device) under the recorder: `rebinders` -- names of harness.fuse's functions out of REBINDERS
    -- applied in the order given (each must find a site), then steps.predict under no_grad, then one training step:
    steps.loss_mix on the stock call forms, the fused DisparityLoss on the fused ones (fused_loss: default, whether anything
    was rebound).  batch = (left, right, target).  -> (records of predict, records of the training step)

    amp = torch.bfloat16 | torch.float16 with mixed = "infer" | "train": after the rebinders, harness.fuse.use_mixed_precision resp.
    use_mixed_precision_training(model, amp, kernels=kernels), then the harness's OWN step under the recorder --
    steps.predict(model, left, right, amp=amp) resp. steps.train_step(..., amp=amp, scaler=scaler) with SGD at lr = 0 and the
    fused DisparityLoss -- so that its autocast region, its cast of the images and scaler.scale / step / update are what runs.
    A model prepared for one of the two runs that one alone: -> (records of predict, []) resp. ([], records of the step)."""
    from ganet_amd.modules.fused import DisparityLoss
    from harness import fuse, steps
    for rb in rebinders:
        assert rb in REBINDERS, rb
        assert getattr(fuse, rb)(model) > 0, rb
    left, right, target = batch
    if amp is not None:
        assert mixed in ("infer", "train"), mixed
        prepare = fuse.use_mixed_precision if mixed == "infer" else fuse.use_mixed_precision_training
        assert prepare(model, amp, kernels=kernels) > 0
        with recording(monkeypatch, *product_functions()) as records:
            if mixed == "infer":
                steps.predict(model, left, right, amp=amp)
                return records, []
            loss, _ = steps.train_step(model, torch.optim.SGD(model.parameters(), lr=0.0), name, left, right, target, max_disp,
                                       steps.criterion(True), fused_loss=DisparityLoss.for_model(name, max_disp), amp=amp, scaler=scaler)
            assert loss is not None and bool(torch.isfinite(loss)), loss
        return [], records
    assert scaler is None and mixed is None, "a GradScaler and the mixed-precision sites belong to a step under autocast: give amp"
    fused_loss = bool(rebinders) if fused_loss is None else fused_loss
    with recording(monkeypatch, *product_functions()) as records:
        steps.predict(model, left, right)
        n_infer = len(records)
        model.train()
        outs = model(left, right)
        if fused_loss:
            loss, _ = DisparityLoss.for_model(name, max_disp)(outs, target)
        else:
            loss = steps.loss_mix(name, outs, target, target < max_disp, steps.criterion(True))
        loss.backward()
    return records[:n_infer], records[n_infer:]


def run_product(monkeypatch, name, crop, max_disp, device, fused_ops=False, fused_bn=False, seed=0):
    """The product model (harness.steps.build_model on the drop-in `libs/`, optionally with harness.fuse's call sites) through
    run_model.  crop = (H, W, B).  -> (records of predict, records of the training step)"""
    from harness import steps
    H, W, B = crop
    torch.manual_seed(seed)
    model = steps.build_model(name, max_disp, device)
    rebinders = (("use_fused_ops",) if fused_ops else ()) + (("use_fused_bn",) if fused_bn else ())
    return run_model(monkeypatch, model, steps.synthetic_batch(B, H, W, max_disp, device), max_disp, rebinders, name, fused_loss=fused_ops)


def oracle_functions():
    from oracle.cpu_ops import OracleLgaChain, OracleSga
    return [OracleSga, OracleLgaChain], []


# what an op's own docstring declares written, kind -> record -> names of `args`: the in-place forms (`inplace=True`), the running
# statistics, an output that is passed in, scratch
DECLARED = {
    "ResidualReluFunction": lambda r: {"arg0"} if r.args[4] else set(),        # y overwrites t
    "BnApplyFunction": lambda r: {"arg0"} if r.args[5] else set(),             # y overwrites x
    "BnReluFunction": lambda r: {"arg4", "arg5"},                              # running_mean / running_var, as F.batch_norm does
    "_sga_infer": lambda r: {"arg5"},                                          # `output`
    "DisparityLossFunction": lambda r: {"arg2"},                               # the fp64 workspace
    "stereo_input": lambda r: {"arg6", "arg7"},                                # out_left / out_right, where given
    "MixedBnReluFunction": lambda r: {"arg4", "arg5"},                         # running_mean / running_var, as BnReluFunction
    "bn_apply_mixed": lambda r: {"arg0"} if r.args[6] else set(),              # inplace: y overwrites x
    # the other mixed-precision forms (cost volume, both normalisations, the casts) declare nothing written: no entry
    # UpSoftminRegressionFunction and DispConvFunction declare nothing written ("neither is written"; their workspaces are
    # their own): no entry, any write is reported
}


def undeclared_writes(records):
    """[(index, kind, phase, what)] of every written input that its op does not declare consumed.  Nothing may be written in
    a backward, and an incoming gradient never."""
    bad = []
    for i, r in enumerate(records):
        allowed = DECLARED.get(r.kind, lambda r: set())(r)
        for phase, what in r.written:
            if phase != "forward" or what not in allowed:
                bad.append((i, r.kind, phase, what))
    return bad


# ---- helpers ----------------------------------------------------------------------------------------------------------------------
def _ratio(err, bound):
    """largest err / bound over the elements (an element whose bound is 0 must be met exactly)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    return float(np.max(q, initial=0.0))


def _within(name, got, want, bound, factor=1.0):
    got, want = np.asarray(got), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert np.isfinite(got).all(), (name, "not finite")
    q = _ratio(np.abs(got.astype(np.float64) - want), np.broadcast_to(bound, want.shape))
    assert q <= factor, (name, f"error / bound = {q:.4g} > {factor}")
    return q


def _atol(atol, want, where=None):
    v = np.abs(np.asarray(want, np.float64))
    if where is not None:
        v = v[where]
    return atol * float(v.max(initial=0.0))


def _atol_px(atol, D):
    return atol * (D - 1) / 192.0


def _close(name, got, want, rtol, atol, rel_only=None, px=None):
    """misc_cases' "close" with its absolute part restated (module docstring) -> the largest error / (atol' + rtol |want|).
    px: the output is in disparity units, of a volume with that many disparities"""
    keep = None if rel_only is None or not rel_only.any() else ~np.broadcast_to(rel_only, np.shape(want))
    a = _atol(atol, want, keep) if px is None else _atol_px(atol, px)
    mc.check([mc.Cmp(name, np.asarray(got), want, "close", rtol, a, rel_only=rel_only if keep is not None else None)])
    w = np.asarray(want, np.float64)
    return _ratio(np.abs(np.asarray(got, np.float64) - w), a + rtol * np.abs(w))


# ---- SGA ------------------------------------------------------------------------------------------------------------------------
def _sga_inputs(r):
    a = r.args[1:6] if r.kind == "OracleSga" else r.args[:5]
    return a[0], list(a[1:5])


def sga_reference(r, oracle):
    """the oracle on the recorded inputs (out, mask, A0..A3, tmp, kp = first arg-max, gradients) and, where a gradient came in,
    the float64 statement evaluated on the ORACLE's selections"""
    x, gs = _sga_inputs(r)
    if r.grad_out is None:
        return {"want": {"out": oracle.sga_forward(x, *gs)[0]}, "ref": None}
    go = r.grad_out[0]
    want = sc.oracle_results(oracle, x, gs, go)
    return {"want": want, "ref": sc.ref64(x, gs, go, kp=want["kp"], mask=want["mask"])}


def sga_got(r, R):
    """what the call produced, under sga_ref64's keys.  OracleSga keeps no volumes: the oracle's own, from `R`"""
    got = {"out": r.outputs[0]}
    if r.grad_in is not None:
        grads = r.grad_in[1:6] if r.kind == "OracleSga" else r.grad_in[:5]
        got.update(zip(sc.GRADS, grads))
    if r.kind == "OracleSga":
        got.update({k: R["want"][k] for k in ("A0", "A1", "A2", "A3", "tmp", "mask", "kp") if k in R["want"]})
    elif "A" in r.saved:
        got.update({f"A{d}": r.saved["A"][d] for d in range(4)})
        got.update(tmp=r.saved["A"][3], mask=r.saved["mask"], kp=r.saved["kp"])
    elif "tmp" in r.saved:                           # GANET_SGA_SAVE=recompute keeps A_left and a float mask
        got.update(tmp=r.saved["tmp"], mask=r.saved["mask"])
    return got


def sga_judge(R, got, equality=True, what=""):
    """out / mask / A / kp EQUAL to the oracle's -- the standing guarantee, on model data -- then forward volumes and all five
    gradients within FACTOR x sga_ref64's bound of float64 on the oracle's selections.  Only what `got` holds is compared
    (the no-grad path: out; recompute mode: out, tmp, mask, gradients).  -> key -> error / bound"""
    want, ref = R["want"], R["ref"]
    if equality:
        sc.assert_equal(got, want, [k for k in sc.FWD if k in got and k in want], what)
        if "mask" in got:
            assert np.array_equal(np.asarray(got["mask"]).astype(np.uint8), want["mask"]), (what, "mask")
        if "kp" in got:
            assert np.array_equal(np.asarray(got["kp"], np.int64), want["kp"]), (what, "kp")
    if ref is None:
        return {"out": 0.0}
    keys = [k for k in sc.FWD + sc.GRADS if k in got]
    assert all(k in got for k in sc.GRADS), (what, "a gradient is missing")
    return sc.assert_within_bound(got, ref, keys, what)


def reference_of(r, oracle):
    """the float64 side of an SGA / LGA / DispTail / DispConv record, computed once and kept on the record"""
    if r.reference is None:
        if r.kind in ("SgaFunction", "OracleSga"):
            r.reference = sga_reference(r, oracle)
        elif r.kind == "UpSoftminRegressionFunction":
            r.reference = tail_reference(r)
        elif r.kind == "DispConvFunction":
            r.reference = conv_reference(r)
        else:
            r.reference = lga_reference(r)
    return r.reference


def check_sga(r, oracle):
    R = reference_of(r, oracle)
    return sga_judge(R, sga_got(r, R), what=repr(r))


def check_sga_infer(r, oracle):
    """_sga_infer / sga_forward_infer: out equal to the oracle's; through the folded BN + ReLU with value_cases.bn_relu_exact's
    rule where the float64 sum is exact, else within ONE rounding of relu(scale[c] * out + shift[c]) -- the epilogue is one
    fma on the exact fp32 `out`, so |got - s| <= u |s| and nothing else"""
    x, gs = r.args[0], list(r.args[1:5])
    scale, shift = (r.args[6], r.args[7]) if r.kind == "_sga_infer" else (r.args[5], r.args[6])
    out = oracle.sga_forward(x, *gs)[0]
    got = r.outputs[0]
    if scale is None:
        sc.assert_equal({"out": got}, {"out": out}, ["out"], repr(r))
        return {"out": 0.0}
    try:
        exp = vc.bn_relu_exact(out, scale, shift)
    except AssertionError:
        C = scale.size
        s = out.astype(np.float64) * scale.astype(np.float64).reshape(1, C, 1, 1, 1) + shift.astype(np.float64).reshape(1, C, 1, 1, 1)
        assert not (got < 0).any()
        return {"out": _within("out", got, np.maximum(s, 0.0), ONE_ROUNDING * np.abs(s))}
    sc.assert_equal({"out": got}, {"out": exp}, ["out"], repr(r))
    return {"out": 0.0}


# ---- LGA chains -----------------------------------------------------------------------------------------------------------------
LGA_PASSES = {"LgaFunction": 1, "Lga2Function": 2, "Lga3Function": 3, "Lga3dFunction": 1, "Lga3d2Function": 2, "Lga3d3Function": 3}
LGA_KEYS = ("y", "gx", "gf")


def _lga_inputs(r):
    if r.kind == "OracleLgaChain":
        return r.args[1], r.args[2], int(r.args[3]), int(r.args[4])
    return r.args[0], r.args[1], int(r.args[2]) if len(r.args) > 2 else 1, LGA_PASSES[r.kind]


def lga_reference(r):
    """lga_ref64.chain_bound on the recorded x, f and incoming gradient (no gradient came in: the forward chain, and only y is
    compared)"""
    x, f, radius, passes = _lga_inputs(r)
    if r.grad_out is None:
        return lga_ref64.chain_bound(x, f, None, radius, passes, backward=False)
    return lga_ref64.chain_bound(x, f, r.grad_out[0], radius, passes)


def lga_got(r):
    got = {"y": r.outputs[0]}
    if r.grad_in is not None:
        g = r.grad_in[1:3] if r.kind == "OracleLgaChain" else r.grad_in[:2]
        got.update(gx=g[0], gf=g[1])
    return got


def lga_ratios(R, got):
    return {k: _ratio(np.abs(np.asarray(got[k], np.float64) - R["want"][k]), R[k]) for k in LGA_KEYS if k in got}


def lga_judge(R, got, what=""):
    """|got - float64| <= FACTOR x chain_bound per element of y, gx and gf -> key -> error / bound"""
    for k in got:
        assert np.shape(got[k]) == R["want"][k].shape and np.isfinite(got[k]).all(), (what, k)
    q = lga_ratios(R, got)
    assert max(q.values()) <= FACTOR, (what, {k: v for k, v in q.items() if v > FACTOR})
    return q


def check_lga(r, oracle=None):
    return lga_judge(reference_of(r, oracle), lga_got(r), repr(r))


# ---- everything else the fused configurations call ---------------------------------------------------------------------------
def _gamma(n):
    return n * U / (1 - n * U)


def check_cost_volume(r, oracle=None):
    """forward: copies and zeros, the same bits.  backward: each gradient is a plain sum of at most Dn fp32 terms -- the case
    table's EQUAL on integer gradients becomes gamma_Dn sum |terms| on real ones (n terms, n - 1 additions, any order)"""
    x, y, Dn = r.args
    mc.check([mc.Cmp("cost", r.outputs[0], m64.cost_volume(x, y, Dn), "bits")])
    q = {"cost": 0.0}
    if r.grad_in is not None:
        g, C = r.grad_out[0], x.shape[1]
        want, mag = m64.cost_volume_adjoint(g, C), m64.cost_volume_adjoint(np.abs(g), C)
        for k, i in (("gx", 0), ("gy", 1)):
            q[k] = _within(k, r.grad_in[i], want[i], _gamma(Dn) * mag[i])
    return q


def check_disparity_regression(r, oracle=None):
    """out = sum_d d x_d: D products and D - 1 additions, gamma_D sum d |x_d| (the case table's EQUAL holds on its dyadic
    inputs only); the backward is one product per element: one rounding"""
    x, Dn = r.args
    q = {"out": _within("out", r.outputs[0], m64.regression(x), _gamma(Dn) * m64.regression(np.abs(x)))}
    if r.grad_in is not None:
        want = m64.regression_adjoint(r.grad_out[0], Dn)
        q["gx"] = _within("gx", r.grad_in[0], want, ONE_ROUNDING * np.abs(want))
    return q


def check_l1_normalize(r, oracle=None):
    x, G, C, K = r.args
    N, _, H, W = x.shape
    x6 = x.reshape(N, G, C, K, H, W)
    want, clamped = m64.l1_normalize(x6, 3), m64.l1_clamped(x6, 3)
    q = {}
    for g in range(G):
        q[f"y{g}"] = _close(f"y{g}", r.outputs[g], want[:, g], 1e-5, 1e-6, rel_only=clamped[:, g])
        mc.check([mc.Cmp(f"y{g} zero set", r.outputs[g], x6[:, g] == 0, "zeros")])
    if r.grad_in is not None:
        gys = np.stack([np.zeros_like(r.outputs[g]) if r.grad_out[g] is None else r.grad_out[g] for g in range(G)], 1)
        q["gx"] = _close("gx", r.grad_in[0].reshape(x6.shape), m64.l1_normalize_adjoint(x6, gys, 3), 1e-4, 1e-5, rel_only=clamped)
    return q


def check_norm_regression(r, oracle=None):
    x = r.args[0]
    q = {"out": _close("out", r.outputs[0], m64.norm_regression(x)[0], 1e-5, 1e-4, px=x.shape[1])}
    if r.grad_in is not None:
        q["gx"] = _close("gx", r.grad_in[0], m64.norm_regression_adjoint(x, r.grad_out[0]), 1e-4, 1e-4, rel_only=m64.l1_clamped(x, 1))
    return q


def check_softmin(r, oracle=None):
    """the backward is a function of the OUTPUT: the float64 adjoint at the y the call itself returned, as in misc_cases"""
    x = r.args[0]
    q = {"y": _close("y", r.outputs[0], m64.softmin(x), 2e-6, 1e-7)}
    if r.grad_in is not None:
        q["gx"] = _close("gx", r.grad_in[0], m64.softmin_adjoint(r.outputs[0], r.grad_out[0]), 1e-5, 1e-5)
    return q


def check_softmin_regression(r, oracle=None):
    x = r.args[0]
    q = {"out": _close("out", r.outputs[0], m64.softmin_regression(x), 1e-5, 1e-4, px=x.shape[1])}
    if r.grad_in is not None:
        q["gx"] = _close("gx", r.grad_in[0], m64.softmin_regression_adjoint(x, r.grad_out[0]), 1e-4, 1e-4)
    return q


def check_trilinear(r, oracle=None):
    """misc_ref64 has no float64 statement on purpose: the reference is ATen on the CPU in fp32 (misc_cases._aten_trilinear)"""
    x, size = r.args
    gy = r.grad_out[0] if r.grad_out is not None else np.zeros(x.shape[:2] + tuple(size), np.float32)
    wy, wgx = mc._aten_trilinear(x, gy, size)
    q = {"y": _close("y", r.outputs[0], wy, 1e-5, 1e-6)}
    if r.grad_in is not None:
        q["gx"] = _close("gx", r.grad_in[0], wgx, 1e-5, 1e-5)
    return q


UNDECIDED_CAP = 4.8e-4        # check_lga_regress: four times the largest share of undecided elements measured on stand-in data


def check_lga_regress(r, oracle=None, planted=None):
    """One LGA pass y = LGA(x, f), then out = sum_d d y_d / max(sum_d |y_d|, eps).  Bars composed of the two ops' own:
      out       misc_cases' bar of the normalised regression (rtol 1e-5, atol' in disparity units) on the float64 pass, PLUS what
                the pass's own roundings do to it: to first order sum_d |d - out sgn(y_d)| / s * E_y, E_y = FACTOR x chain_bound
                (y is signed -- filters are -- so sum_d d y_d cancels, and E_y / s is not small against 1e-5)
      backward  gy = the float64 adjoint of the regression, held by ITS bar (rtol 1e-4, atol' as everywhere) or, where that is
                smaller, by what the asserted bars of out and y leave room for (derived in the code below); the LGA pass
                behind it gets FACTOR x chain_bound for its own roundings plus that allowance on gy pushed through |f| (gx)
                and through |taps of x| (gf), both by lga_backward on absolute values.
    The adjoint holds sgn(y_d), and y is a quantity the op computed ITSELF, in fp32: where |y64| <= E_y float64 cannot say which
    sign an fp32 pass within its bound arrives at, and the two adjoints differ by 2 |go out| / s -- thousands of times the bar
    on gy.  So, as check_bn_relu does at the ReLU's kink:
      y         the call's own volume (saved for its backward: Record.saved) within E_y of the float64 pass.  This is what
                entitles the call to its own sign at the elements below -- and to nothing else
      decided   |y64| > E_y (or E_y = 0: every product is an exact zero, y64 = 0, and any fp32 sum of them is): the call's
                sign must EQUAL float64's, else the check fails by the name "sign"
      undecided the other elements: the reference adjoint takes the CALL's sign there, and `through` the larger of the two
                |d -+ out| = d + |out|.  Their count is returned, and how many of them differ from float64's sign (`flipped`)
      cap       undecided <= max(8, UNDECIDED_CAP y.size): a condition on the DATA (float64 and the bound decide it, never the
                call's result), so that a volume that is zero or tiny everywhere is not excused wholesale.  Measured shares of
                undecided elements: synthetic softmin volumes [2,49,48,120] at most 1.6e-5; the stand-in's LgaRegress site on
                the CPU (tests/test_model_calls_cpu.py prints them) 12 and 14 of 225,792 at 48x96 (6.2e-5), 84 and 56 of
                2,257,920 at 96x240x2 (3.7e-5); the same site on the inputs a device run recorded 27 of 225,792 at 48x96
                (1.2e-4) and 63 and 85 of 2,257,920 at 96x240x2 (3.8e-5).  The stand-in's data exceed the 1e-4 first thought
                of, so the cap is FOUR TIMES the largest measured share, 4 x 1.2e-4 = 4.8e-4.
                planted: a mask of elements the caller PUT at the kink (tests/lga_regress_cases.py) -- all of them must be
                undecided, and the cap then holds for the undecided elements outside the mask.
    A record with gradients and without the saved y cannot be judged and fails."""
    x, f, radius, ndisp = r.args
    what = repr(r)
    go = r.grad_out[0] if r.grad_in is not None else np.zeros(x.shape[:1] + x.shape[2:], np.float32)
    y, E_y, und = lga_regress_undecided(x, f, radius)
    if planted is not None:
        assert und[planted].all(), (what, "planted elements that float64 decides", int((planted & ~und).sum()))
    stray = int((und & ~planted).sum()) if planted is not None else int(und.sum())
    assert stray <= max(8, UNDECIDED_CAP * y.size), (what, f"{stray} of {y.size} elements undecided: the data sit at the kink, not the call")
    q = {"undecided": float(und.sum())}
    sign = np.sign(y)
    if "y" in r.saved:
        yc = r.saved["y"].astype(np.float64)
        wrong = ~und & (np.sign(yc) != sign)
        assert not wrong.any(), (what, "sign", f"{int(wrong.sum())} decided elements, the first at {tuple(np.argwhere(wrong)[0])}")
        q["y"] = _within("y", r.saved["y"], y, E_y)
        q["flipped"] = float((und & (np.sign(yc) != sign)).sum())
        sign = np.where(und, np.sign(yc), sign)
    else:
        assert r.grad_in is None, (what, "a call with gradients must keep its own y (Record.saved)")
    gy = m64.norm_regression_adjoint(y, go, sign)
    out, s = m64.norm_regression(y)
    D = x.shape[1]
    d = np.arange(D, dtype=np.float64).reshape(1, D, 1, 1)
    lever = np.where(und, d + np.abs(out[:, None]), np.abs(d - out[:, None] * np.sign(y)))
    through = (lever * E_y).sum(1) / s
    bar_out = 1e-5 * np.abs(out) + _atol_px(1e-4, D) + through
    q["out"] = _within("out", r.outputs[0], out, bar_out)
    if r.grad_in is not None:
        R = lga_ref64.chain_bound(x, f, gy, radius, 1)
        e_gy = 1e-4 * np.abs(gy) + _atol(1e-4, gy)
        # The table's atol' is 1e-4 of the LARGEST |gy| of the volume -- a pixel whose norm is small -- granted to every element:
        # on the stand-in's data it hides a relative error of 2^-12 in gx and gf (tests/test_model_calls_cpu.py).  What the
        # call's gy can differ by is known from what has been asserted above: gy = go (d - out sgn) / s in three roundings,
        # on the call's out (within bar_out of float64's) and on its norm s = sum |y_d| (each y_d within E_y, D - 1 additions):
        #   |d gy| <= FACTOR (3 u + gamma_D) |gy| + |go| bar_out / s + |gy| sum_d E_y / s.
        # The allowance is the smaller of the two, element by element, so no element's bar is wider than it was; where the
        # norm is clamped (s = eps exactly, in any arithmetic) the table's stays.
        derived = FACTOR * (3 * U + _gamma(D)) * np.abs(gy) + (np.abs(go) * bar_out / s)[:, None] + np.abs(gy) * (E_y.sum(1) / s)[:, None]
        e_gy = np.where((np.abs(y).sum(1) < m64.EPS)[:, None], e_gy, np.minimum(e_gy, derived))
        extra = lga_ref64.lga_backward(np.abs(x), np.abs(f), e_gy, radius)
        for k, i in (("gx", 0), ("gf", 1)):
            bar = FACTOR * R[k] + extra[i]
            try:
                q[k] = _within(k, r.grad_in[i], R["want"][k], bar)
            except AssertionError as e:
                raise AssertionError(*e.args, _lga_regress_element(k, r.grad_in[i], R["want"][k], bar, y, r.saved["y"], E_y, und, radius)) from None
    return q


def lga_regress_undecided(x, f, radius):
    """-> (the float64 pass y, E_y = FACTOR x chain_bound's bound of it, the mask of elements whose sign float64 cannot decide
    for an fp32 pass: |y| <= E_y, where E_y > 0)"""
    R = lga_ref64.chain_bound(x, f, None, radius, 1, backward=False)
    y, E_y = R["want"]["y"], FACTOR * R["y"]
    return y, E_y, (np.abs(y) <= E_y) & (E_y > 0)


def _lga_regress_element(k, got, want, bar, y, y_call, E_y, und, radius):
    """what a failure of gx / gf is to be explained from: the element with the largest error / bar, and the y that its
    adjoint reads -- gx[b,d,i,j]: the taps' readers, d +- 1, i +- r, j +- r; gf[b,t,i,j]: the column of its pixel"""
    err = np.abs(got.astype(np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        idx = np.unravel_index(np.argmax(np.where(err == 0, 0.0, err / bar)), err.shape)
    b, c, i, j = (int(v) for v in idx)
    D, H, W = y.shape[1:]
    if k == "gx":
        win = (b, slice(max(c - 1, 0), min(c + 2, D)), slice(max(i - radius, 0), min(i + radius + 1, H)), slice(max(j - radius, 0), min(j + radius + 1, W)))
    else:
        win = (b, slice(None), i, j)
    lines = [f"{k}{list(idx)}: got {got[idx]!r} float64 {want[idx]!r} bar {bar[idx]:.3g}; y it reads (float64 / the call's / E_y / undecided):"]
    order = np.argsort((np.abs(y[win]) / np.maximum(E_y[win], 1e-300)).ravel())[:6]
    for o in order:
        lines.append(f"  {y[win].ravel()[o]!r} / {y_call[win].ravel()[o]!r} / {E_y[win].ravel()[o]:.3g} / {bool(und[win].ravel()[o])}")
    return "\n".join(lines)


def _relu_adjoint(r, y, scale, i_t, i_rem):
    """g = grad_y where the call's own y > 0; rem takes g (the same bits), t takes scale[c] * g: one rounding of an exact product"""
    gy = r.grad_out[0]
    g = np.where(y > 0, gy, np.float32(0))
    q = {}
    if i_rem is not None and r.grad_in[i_rem] is not None:
        mc.check([mc.Cmp("g_rem", r.grad_in[i_rem], g, "bits")])
        q["g_rem"] = 0.0
    if r.grad_in[i_t] is not None:
        C = g.shape[1]
        want = g if scale is None else (g.astype(np.float64) * scale.astype(np.float64).reshape((1, C) + (1,) * (g.ndim - 2))).astype(np.float32)
        mc.check([mc.Cmp("g_t", r.grad_in[i_t], want, "equal")])
        q["g_t"] = 0.0
    return q


def _affine_relu(name, got, t, rem, scale, shift, relu=True, fmt=mxc.F32):
    """y = relu(scale[c] t + shift[c] + rem) in at most three fp32 roundings (product, two additions; an fma build has two),
    each at most u times a partial result that |scale t| + |shift| + |rem| bounds: the case tables' EQUAL on dyadic inputs
    becomes 3 u (|scale t| + |shift| + |rem|) on real ones, one rounding where there is nothing but t + rem.  The ReLU is
    1-Lipschitz: the bar holds through it, and where float64 is above / below the bar the sign is decided.
    fmt: the format y was stored in (`got`: its up-cast) -- a 16-bit store adds its one rounding, half an ulp of fmt at
    |s| + bar, to the bar and to the band in which the zero set is not decided; fp32 (the default): nothing is added."""
    C = t.shape[1]
    b = lambda v: v.astype(np.float64).reshape((1, C) + (1,) * (t.ndim - 2))      # noqa: E731
    t64 = t.astype(np.float64)
    rem64 = 0.0 if rem is None else rem.astype(np.float64)
    if scale is None:
        s, bar = t64 + rem64, ONE_ROUNDING * np.abs(t64 + rem64)
    else:
        s = b(scale) * t64 + b(shift) + rem64
        bar = 3 * ONE_ROUNDING * (np.abs(b(scale) * t64) + np.abs(b(shift)) + np.abs(rem64))
    if fmt != mxc.F32:
        bar = bar + mtc.half_ulp(np.abs(np.maximum(s, 0.0) if relu else s) + bar, fmt)     # (of the value that is stored)
    if relu:
        assert not (got[s < -bar] != 0).any() and not (got[s > bar] <= 0).any(), (name, "zero set")
    return _within(name, got, np.maximum(s, 0.0) if relu else s, bar)


def check_residual_relu(r, oracle=None):
    t, rem, scale, shift, _ = r.args
    q = {"y": _affine_relu("y", r.outputs[0], t, rem, scale, shift)}
    if r.grad_in is not None:
        q.update(_relu_adjoint(r, r.outputs[0], scale, 0, 1))
    return q


def check_bn_apply(r, oracle=None):
    x, rem, scale, shift, relu, _ = r.args
    q = {"y": _affine_relu("y", r.outputs[0], x, rem, scale, shift, relu)}
    if r.grad_in is not None:
        y = r.outputs[0] if relu else np.ones_like(r.outputs[0])
        q.update(_relu_adjoint(r, y, scale, 0, 1 if rem is not None else None))
    return q


def check_bn_relu(r, oracle=None, enforce=True):
    """bn_cases.check on the recorded tensors: a Case built around them (nothing generated, nothing nudged).  Recorded data
    cannot be nudged away from the ReLU's kink, so at the elements that float64 cannot decide for fp32 (|z| <= 4 B_y) the
    mask is the call's own y > 0; everywhere else float64 decides (bn_ref64.Reference, relu_positive).  enforce=False: a
    measurement (of ATen's chain), nothing is asserted."""
    x, rem, weight, bias, rmean, rvar, momentum, eps, relu = r.args
    N, C = x.shape[:2]
    shape = (N, C, x.size // (N * C))
    c = object.__new__(bn_cases.Case)
    c.name, c.shape, c.relu, c.offset, c.exact, c.momentum, c.eps = repr(r), shape, bool(relu), 0, False, momentum, eps
    c.x, c.rem = x.reshape(shape), None if rem is None else rem.reshape(shape)
    c.compare_grads = r.grad_in is not None
    c.gy = r.grad_out[0].reshape(shape) if c.compare_grads else np.zeros(shape, np.float32)
    c.weight, c.bias, c.running_mean, c.running_var, c.nudged = weight, bias, rmean, rvar, 0
    c.mean_term = True                               # model data: channels whose spread is far below their mean (bn_cases)
    y = r.outputs[0].reshape(shape)
    c._ref = bn_ref64.Reference(*c.inputs(), relu_positive=y > 0)
    got = {"y": y, "running_mean": None, "running_var": None}
    if rmean is not None:
        # the op updates its running statistics in place: what the call left in them is what the NEXT reader found
        got["running_mean"], got["running_var"] = r.after.get(4, rmean), r.after.get(5, rvar)
    want = [False] * 4
    if c.compare_grads:
        for i, key in enumerate(("grad_x", "grad_rem", "grad_weight", "grad_bias")):
            if r.grad_in[i] is not None:
                got[key], want[i] = (r.grad_in[i].reshape(shape) if i < 2 else r.grad_in[i]), True
    q = bn_cases.check(c, got, want=tuple(want), verbose=False, enforce=enforce, saved=False)
    q["undecided"] = float(c.ref.undecided().sum())
    return q


def check_disparity_loss(r, oracle=None):
    target, params, _, kinds, mask_mode, *preds = r.args
    p = dict(zip(loss_ref64.PARAMS, (float(v) for v in params)))
    P = len(preds)
    gl = float(r.grad_out[0]) if r.grad_out is not None else 1.0
    want = tuple(g is not None for g in r.grad_in[5:5 + P]) if r.grad_in is not None else (False,) * P
    c = loss_cases.Case(repr(r), target.shape, preds, target, tuple(kinds), [p["w0"], p["w1"], p["w2"]][:P], thresh=p["thresh"],
                        alpha=p["alpha"], mask_mode=int(mask_mode), grad_loss=gl, want=want, hi=p["hi"], lo=p["lo"], rate=p["rate"])
    loss_cases.check_forward(c, r.outputs[0], r.outputs[1], verbose=False)
    if r.grad_in is not None:
        loss_cases.check_grads(c, list(r.grad_in[5:5 + P]))
    return {"loss": abs(float(r.outputs[0]) - c.ref.loss) / (loss_cases.SUM_RTOL * abs(c.ref.loss) + loss_cases.TINY)}


def check_myloss2(r, oracle=None):
    """MyLoss2Function is pure tensor arithmetic (kept for API parity): loss_ref64's stage-by-stage statement, every element
    valid, loss_cases' relative bars (sums 2^-18, gradients 2^-20 against float64)"""
    a, b = r.args[:2]
    thresh, alpha = (r.args[2] if len(r.args) > 2 else 1), (r.args[3] if len(r.args) > 3 else 2)      # the Function's defaults
    c = loss_cases.Case(repr(r), (1, 1, a.size), [a], b, (1,), (1.0,), thresh=thresh, alpha=alpha, hi=np.inf,
                        grad_loss=float(r.grad_out[0]) if r.grad_out is not None else 1.0)
    assert c.ref.count == a.size
    assert loss_cases.close(r.outputs[0], c.ref.loss, loss_cases.SUM_RTOL), (float(r.outputs[0]), c.ref.loss)
    q = {"loss": abs(float(r.outputs[0]) - c.ref.loss) / (loss_cases.SUM_RTOL * abs(c.ref.loss) + loss_cases.TINY)}
    if r.grad_in is not None:
        g64 = c.ref.grads(c.grad_loss, np.float64)[0].reshape(a.shape)
        q["grad"] = _within("grad", r.grad_in[0], g64, loss_cases.GRAD_RTOL * np.abs(g64) + loss_cases.TINY)
    return q


# ---- the Disp tails: DispTail and DispConv -----------------------------------------------------------------------------------------
# Both bars are the case tables' own, unchanged: twice a first-order bound that is computed FROM the data it is applied to
# (disp_tail_ref64: every term is u or an ulp of lambda times sums of |x|, slopes of x, p |od - out|, |gv|; disp_conv_ref64:
# L u sum |terms|).  Nothing in them assumes magnitude 1 or dyadic inputs -- those belong to the tables' "exact" kinds, which are
# not applied here -- so on recorded data (a convolution output of 1e-1, gradients of 1e-4 .. 1e-6) they scale down with it and
# need no restating.  tests/test_model_calls_cpu.py calibrates them on such data against disp_tail_ref64.Float32Model (both
# variants of lambda), resp. an fp32 accumulation of the convolution, never against the device's results.
def _volume(x):
    return x.reshape((x.shape[0],) + x.shape[-3:])


def tail_reference(r):
    """disp_tail_ref64.Statement on the recorded c, size and incoming gradient (none came in: zeros, and only out is compared)"""
    x, size = r.args
    c = _volume(x)
    size = tuple(int(v) for v in size)
    g = r.grad_out[0] if r.grad_out is not None else np.zeros((c.shape[0],) + size[1:], np.float32)
    return disp_tail_ref64.Statement(c, size, np.ascontiguousarray(g, np.float32))


def tail_got(r):
    got = {"out": r.outputs[0]}
    if r.grad_in is not None:
        got["grad_x"] = _volume(r.grad_in[0])
    return got


def tail_judge(S, got, what=""):
    """|got - float64| <= twice the statement's bound per element of out and grad_x: disp_tail_cases.check -> key -> error / bar"""
    case = types.SimpleNamespace(id=what, kind="general", ref=S)
    return disp_tail_cases.check(case, {k: np.ascontiguousarray(v) for k, v in got.items()}, quantities=tuple(got), verbose=False)


def check_up_softmin_regression(r, oracle=None):
    return tail_judge(reference_of(r, oracle), tail_got(r), repr(r))


def conv_reference(r):
    """disp_conv_ref64.Statement on the recorded x, weight and incoming gradient (none came in: zeros, and only y is compared)"""
    x, w = r.args[:2]
    gy = _volume(r.grad_out[0]) if r.grad_out is not None else np.zeros((x.shape[0],) + x.shape[2:], np.float32)
    return disp_conv_ref64.Statement(x, w, np.ascontiguousarray(gy, np.float32))


def conv_got(r):
    got = {"y": _volume(r.outputs[0])}
    if r.grad_in is not None:
        C = r.args[0].shape[1]
        for key, g, shape in (("grad_x", r.grad_in[0], r.args[0].shape), ("grad_weight", r.grad_in[1], (C, 3, 3, 3))):
            if g is not None:                        # (autograd did not ask for it)
                got[key] = g.reshape(shape)
    return got


def conv_judge(S, got, what=""):
    """|got - float64| <= 2 L u sum |terms| per element of y, grad_x and grad_weight: disp_conv_cases.check.  A direction the
    record's `directions` leaves on ATen is held to the same bound (its L is never more than the number of terms)"""
    case = types.SimpleNamespace(id=what, kind="general", ref=S)
    return disp_conv_cases.check(case, {k: np.ascontiguousarray(v) for k, v in got.items()}, quantities=tuple(got), verbose=False)


def check_disp_conv(r, oracle=None):
    if r.grad_in is not None:
        assert r.grad_in[1] is not None, (repr(r), "the convolution's weight got no gradient")
    return conv_judge(reference_of(r, oracle), conv_got(r), repr(r))


# ---- the image front and back end: io_ref64's statement (a), bit for bit, as io_cases holds the kernels to it ------------------------
def _same_bits(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    bad = io_cases.bits(got) != io_cases.bits(want) if got.dtype == np.float32 else got != want
    assert not bad.any(), (name, f"{int(bad.sum())} of {bad.size} elements differ from the statement")
    return 0.0


def check_stereo_input(r, oracle=None):
    """equality needs io_cases' premise: every occurring quotient at least io_ref64.MARGIN from a rounding boundary of float32"""
    left, right, crop, oy, oxl, oxr = r.args[:6]
    assert io_ref64.margin(left, right) >= io_ref64.MARGIN, (repr(r), "a quotient sits at a rounding boundary: draw other images")
    want = io_ref64.stereo_input(left, right, int(crop[0]), int(crop[1]), int(oy), int(oxl), int(oxr))
    return {"left": _same_bits("left", r.outputs[0], want[0]), "right": _same_bits("right", r.outputs[1], want[1])}


def check_window_f32(r, oracle=None):
    src, crop, oy, ox, sub, fill = r.args
    return {"dst": _same_bits("dst", r.outputs[0], io_ref64.window_f32(src, int(crop[0]), int(crop[1]), int(oy), int(ox), sub, fill))}


def check_disparity_to_u16(r, oracle=None):
    disp, hw, oy, ox, scale = r.args
    return {"u16": _same_bits("u16", r.outputs[0], io_ref64.disparity_u16(disp, int(hw[0]), int(hw[1]), int(oy), int(ox), scale))}


# ---- the mixed-precision forms: 16-bit storage around fp32 arithmetic (ganet_amd.functions.mixed / mixed_train) --------------------------
# A 16-bit value's up-cast is exact, so every checker below evaluates the float64 statement of the CORRESPONDING fp32 op on the
# up-cast recorded inputs -- the statements above, no other -- and holds each output by its storage: an fp32 output to the fp32
# kind's bar, restated relative to the recorded data as above; a 16-bit output to that bar plus half an ulp of its format at
# |want| + bar (mixed_train_cases.half_ulp), the one rounding the store adds.  There is no new tolerance constant.  Gradients are
# compared at the magnitude they were recorded at: under a GradScaler they carry its scale, a power of two, and every adjoint
# below is linear in its incoming gradient -- statement and bar scale with it exactly, short of the format's range, which
# `_within` (not finite) and check_cast (a finite value that left the range) report.
def _held(name, got, want, bar):
    want = np.asarray(want, np.float64)
    if isinstance(got, Half):
        bar = bar + mtc.half_ulp(np.abs(want) + bar, got.fmt)
    return _within(name, up(got), want, bar)


def _cast_bits(name, got, src, dst):
    """got: bits equal to mixed_cases.convert (round to nearest even) of `src` to the format dst; the same format: a copy"""
    assert fmt_of(got) == dst and got.shape == src.shape, (name, fmt_of(got), dst, got.shape, src.shape)
    want = mxc.cast_expected(np.asarray(src), fmt_of(src), dst)
    if fmt_of(src) == dst:
        assert np.asarray(got).tobytes() == want.tobytes(), (name, "a cast to the same type changed a pattern")
    else:
        mxc.assert_same(np.ascontiguousarray(np.asarray(got)).ravel(), want, dst, name)
        s = np.asarray(up(src)).ravel()
        lost = np.isfinite(s) & ~np.isfinite(mxc.up(want, dst) if dst != mxc.F32 else want)
        assert not lost.any(), (name, f"{int(lost.sum())} finite values left the range of {mxc.FMT_NAME[dst]}, the largest {np.abs(s[lost]).max():.3g}")
    return 0.0


def check_cast(r, oracle=None):
    """CastFunction / cast: a conversion has no bar.  Forward: the recorded input converted to the asked type; backward: the
    incoming gradient converted to the input's type"""
    t, dtype = r.args[:2]
    q = {"y": _cast_bits(f"{r!r} y", r.outputs[0], t, _TORCH_FMT[dtype])}
    if r.grad_in is not None:
        q["g"] = _cast_bits(f"{r!r} g", r.grad_in[0], r.grad_out[0], fmt_of(t))
    return q


def check_cost_volume_16(r, oracle=None):
    """forward: a copy with a mask -- misc_ref64.cost_volume on the recorded BIT PATTERNS (integers below 2^16, exact in float64;
    the mask's zero is the pattern 0).  backward: check_cost_volume's, fp32 sums over at most Dn planes of the up-cast gradient
    (gamma_Dn sum |terms|), stored in the gradient's format"""
    x, y, Dn = r.args[:3]
    cost = r.outputs[0]
    assert isinstance(x, Half) and fmt_of(y) == x.fmt and fmt_of(cost) == x.fmt, (repr(r), fmt_of(x), fmt_of(y), fmt_of(cost))
    want = m64.cost_volume(np.asarray(x), np.asarray(y), Dn)
    assert cost.shape == want.shape and np.array_equal(np.asarray(cost), want.astype(np.uint16)), (repr(r), "cost: not the copy")
    q = {"cost": 0.0}
    if r.grad_in is not None:
        assert all(fmt_of(g) == fmt_of(r.grad_out[0]) for g in r.grad_in[:2]), repr(r)
        g, C = up(r.grad_out[0]), x.shape[1]
        want, mag = m64.cost_volume_adjoint(g, C), m64.cost_volume_adjoint(np.abs(g), C)
        for k, i in (("gx", 0), ("gy", 1)):
            q[k] = _held(k, r.grad_in[i], want[i], _gamma(Dn) * mag[i])
    return q


def _l1_dims(r):
    x = r.args[0]
    if r.kind in ("NormalizeGuidanceMixedFunction", "normalize_guidance_mixed"):
        return x, 4, int(r.args[1]), 5
    return x, 1, 1, x.shape[1]


def check_l1_mixed(r, oracle=None):
    """both normalisations, Function and inference form: check_l1_normalize's statement and bars on the up-cast x (sign, zero set
    and clamp act on the recorded input); the outputs are fp32; gx is stored in x's format"""
    x16, G, C, K = _l1_dims(r)
    assert isinstance(x16, Half), (repr(r), "a 16-bit input was expected")
    x = up(x16)
    N, _, H, W = x.shape
    x6 = x.reshape(N, G, C, K, H, W)
    want, clamped = m64.l1_normalize(x6, 3), m64.l1_clamped(x6, 3)
    assert len(r.outputs) == G and all(not isinstance(o, Half) and o.dtype == np.float32 for o in r.outputs), repr(r)
    q = {}
    for g in range(G):
        y = r.outputs[g].reshape(N, C, K, H, W)
        q[f"y{g}"] = _close(f"y{g}", y, want[:, g], 1e-5, 1e-6, rel_only=clamped[:, g])
        mc.check([mc.Cmp(f"y{g} zero set", y, x6[:, g] == 0, "zeros")])
    if r.grad_in is not None:
        gys = np.stack([np.zeros((N, C, K, H, W), np.float32) if r.grad_out[g] is None else r.grad_out[g].reshape(N, C, K, H, W) for g in range(G)], 1)
        wgx = m64.l1_normalize_adjoint(x6, gys, 3)
        gx = r.grad_in[0]
        assert fmt_of(gx) == x16.fmt, (repr(r), "the gradient of x has x's format")
        a = _atol(1e-5, wgx, ~clamped if clamped.any() else None)                # `_close`, as check_l1_normalize calls it
        q["gx"] = _held("gx", gx.reshape(x6.shape), wgx, np.where(clamped, 0.0, a) + 1e-4 * np.abs(wgx))
    return q


def mixed_bn_z32(x, rem, weight, bias, mean, invstd):
    """bn_kernels.h's fp32 expression behind a 16-bit x, with the statistics the call returned: scale = fl(weight invstd),
    shift = fma(-mean, scale, bias), z = fma(x, scale, shift), then -- where a residual is added -- z = fl(z + rem): ONE more fp32
    rounding, before the ReLU and before the store's (bn_z).  x: [N,C,S] float32"""
    C = x.shape[1]
    w = np.ones(C, np.float32) if weight is None else weight
    b = np.zeros(C, np.float32) if bias is None else bias
    with np.errstate(all="ignore"):
        scale = (w * invstd).astype(np.float32)
        shift = mtc.fma32(-mean, scale, b)
        z = mtc.fma32(x, scale[None, :, None], shift[None, :, None])
        return z if rem is None else (z + rem).astype(np.float32)


def check_mixed_bn_relu(r, oracle=None):
    """MixedBnReluFunction: check_bn_relu's construction -- a bn_cases.Case around the recorded tensors, x and a 16-bit grad_y
    up-cast, mean_term=True -- with mixed_train_cases' general tier and tests/test_gpu_mixed_train.py's bars:
      mean, invstd  the call's own (Record.saved) inside bn_cases' bars; a record with gradients and without them fails
      y             BITS equal to convert(relu(z32), y's type), z32 = mixed_bn_z32 on those statistics: no bar.  The ReLU's mask,
                    forward and backward, is z32 > 0 (the backward recomputes the same expression): that is the call's own mask,
                    handed to bn_ref64.Reference for the elements float64 cannot decide, and it must agree with float64's
                    everywhere else
      running_*     bn_cases' bars, on what the call left in the buffers
      grad_x        bar_grad_x(mean term) + half an ulp of x's format
      grad_rem      fp32, equal to the masked gradient
      grad_weight, grad_bias   bn_cases' bars with the mean term"""
    x16, rem, weight, bias, rmean, rvar, momentum, eps, relu = r.args[:9]
    out_dtype = r.args[9] if len(r.args) > 9 else None
    what = repr(r)
    assert isinstance(x16, Half), (what, "a 16-bit x was expected")
    y16 = r.outputs[0]
    assert fmt_of(y16) == (x16.fmt if out_dtype is None else _TORCH_FMT[out_dtype]), (what, "y's type", fmt_of(y16))
    N, C = x16.shape[:2]
    shape = (N, C, x16.size // (N * C))
    x = up(x16).reshape(shape)
    rem3 = None if rem is None else rem.reshape(shape)
    grads = r.grad_in is not None
    c = object.__new__(bn_cases.Case)
    c.name, c.shape, c.relu, c.offset, c.exact, c.momentum, c.eps = what, shape, bool(relu), 0, False, momentum, eps
    c.x, c.rem, c.compare_grads, c.mean_term, c.nudged = x, rem3, grads, True, 0
    if grads:
        assert fmt_of(r.grad_out[0]) == fmt_of(y16), (what, "grad_y has y's type")
    c.gy = up(r.grad_out[0]).reshape(shape) if grads else np.zeros(shape, np.float32)
    c.weight, c.bias, c.running_mean, c.running_var = weight, bias, rmean, rvar
    q = {}
    y = up(y16).reshape(shape)
    if "mean" in r.saved:
        z32 = mixed_bn_z32(x, rem3, weight, bias, r.saved["mean"], r.saved["invstd"])
        with np.errstate(invalid="ignore"):
            positive = z32 > 0
            y32 = np.where(z32 <= 0, np.float32(0), z32) if relu else z32
        mxc.assert_same(np.asarray(y16).reshape(shape), mxc.convert(y32, fmt_of(y16)).reshape(shape), fmt_of(y16), f"{what}: y")
        q["y"] = 0.0
    else:
        assert not grads, (what, "a call with gradients must keep its own mean and invstd (Record.saved)")
        positive = y > 0
    c._ref = ref = bn_ref64.Reference(*c.inputs(), relu_positive=positive)
    if relu:
        wrong = ~ref.undecided() & (positive != (ref.z > 0))
        assert not wrong.any(), (what, f"the ReLU's mask differs from float64's at {int(wrong.sum())} decided elements")
    if "mean" in r.saved:
        q["mean"] = bn_cases.within("save_mean", r.saved["mean"], ref.mean, 2.0 ** -23 * ref.mean_abs_x, False)
        q["invstd"] = bn_cases.within("save_invstd", r.saved["invstd"], ref.invstd, 2.0 ** -22 * ref.invstd, False)
    else:
        q["y"] = _held("y", y16.reshape(shape), ref.y, ref.bar_y())
    if rmean is not None:
        m = ref.m
        q["running_mean"] = bn_cases.within("running_mean", r.after.get(4, rmean), ref.running_mean,
                                            2.0 ** -22 * ((1 - m) * np.abs(ref.old_mean) + m * np.abs(ref.mean)), False)
        q["running_var"] = bn_cases.within("running_var", r.after.get(5, rvar), ref.running_var,
                                           2.0 ** -22 * ((1 - m) * np.abs(ref.old_var) + m * np.abs(ref.new_var)), False)
    if grads:
        gx, grem, gw, gb = r.grad_in[:4]
        if gx is not None:
            assert fmt_of(gx) == x16.fmt, (what, "grad_x has x's type")
            q["grad_x"] = _held("grad_x", gx.reshape(shape), ref.grad_x, ref.bar_grad_x(True))
        if grem is not None:
            mxc.assert_same(np.ascontiguousarray(grem).reshape(shape), ref.g.astype(np.float32), mxc.F32, f"{what}: grad_rem is not g")
            q["grad_rem"] = 0.0
        if gw is not None:
            bar = 2.0 ** -22 * ref.invstd * ref.sum_abs_gxm + 2.0 ** -22 * np.abs(ref.mean) * ref.invstd * np.abs(ref.sum_g)
            q["grad_weight"] = bn_cases.within("grad_weight", gw, ref.grad_weight, bar, False)
        if gb is not None:
            q["grad_bias"] = bn_cases.within("grad_bias", gb, ref.grad_bias, 2.0 ** -22 * ref.sum_abs_g, False)
    q["undecided"] = float(ref.undecided().sum())
    return q


def check_bn_apply_mixed(r, oracle=None):
    """the folded BatchNorm of inference on 16-bit storage: `_affine_relu`'s bound on the up-cast x / rem, plus half an ulp of the
    format y is stored in"""
    x, rem, scale, shift, relu, out_dtype, _ = r.args
    y = r.outputs[0]
    assert fmt_of(y) == (fmt_of(x) if out_dtype is None else _TORCH_FMT[out_dtype]), (repr(r), "y's type", fmt_of(y))
    return {"y": _affine_relu("y", up(y), up(x), up(rem), scale, shift, relu, fmt=fmt_of(y))}


MIXED_CHECKERS = {
    "MixedBnReluFunction": check_mixed_bn_relu, "CostVolume16Function": check_cost_volume_16,
    "NormalizeGuidanceMixedFunction": check_l1_mixed, "NormalizeFiltersMixedFunction": check_l1_mixed, "CastFunction": check_cast,
    "cast": check_cast, "bn_apply_mixed": check_bn_apply_mixed, "cost_volume_16": check_cost_volume_16,
    "normalize_guidance_mixed": check_l1_mixed, "normalize_filters_mixed": check_l1_mixed,
}

CHECKERS = {
    **MIXED_CHECKERS,
    "SgaFunction": check_sga, "OracleSga": check_sga, "_sga_infer": check_sga_infer, "sga_forward_infer": check_sga_infer,
    "OracleLgaChain": check_lga, **{k: check_lga for k in LGA_PASSES},
    "GetCostVolumeFunction": check_cost_volume, "DisparityRegressionFunction": check_disparity_regression,
    "L1NormalizeGroupsFunction": check_l1_normalize, "NormDisparityRegressionFunction": check_norm_regression,
    "SoftminFunction": check_softmin, "SoftminDisparityRegressionFunction": check_softmin_regression,
    "TrilinearUpsampleFunction": check_trilinear, "LgaRegressFunction": check_lga_regress,
    "ResidualReluFunction": check_residual_relu, "BnApplyFunction": check_bn_apply, "BnReluFunction": check_bn_relu,
    "DisparityLossFunction": check_disparity_loss, "MyLoss2Function": check_myloss2,
    "UpSoftminRegressionFunction": check_up_softmin_regression, "DispConvFunction": check_disp_conv,
    "stereo_input": check_stereo_input, "window_f32": check_window_f32, "disparity_to_u16": check_disparity_to_u16,
}


def check_all(records, oracle, kinds=None, report=None):
    """every record through the checker of its kind (kinds: only these -- the CPU calibration).  A recorded kind without a
    checker fails here, by name.  -> {(kind, key): largest error / bound over the records of that kind}; report: a list that
    gets one line per record"""
    missing = sorted({r.kind for r in records if r.kind not in CHECKERS})
    assert not missing, f"recorded op calls without a checker: {missing}"
    worst = collections.OrderedDict()
    for i, r in enumerate(records):
        if kinds is not None and r.kind not in kinds:
            continue
        q = CHECKERS[r.kind](r, oracle)
        for k, v in q.items():
            worst[(r.kind, k)] = max(worst.get((r.kind, k), 0.0), v)
        if report is not None:
            report.append(f"{i:3d} {r!r}: " + " ".join(f"{k}={v:.3g}" for k, v in q.items()))
    return worst


def kinds_of(records):
    return collections.Counter(r.kind for r in records)


def fmt(worst):
    return "\n".join(f"  {kind:36s} {key:12s} {v:.3f}" for (kind, key), v in worst.items())
