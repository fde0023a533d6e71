"""TEST INFRASTRUCTURE: the case table of the fused BatchNorm + residual + ReLU (ganet_bn_workspace / _train_forward /
_train_backward / _apply_forward), shared by tests/test_sim_bn.py (emulator build, guard pages) and tests/test_gpu_bn.py
(gfx950 build, C ABI and module).  `run(api, dev, case)` drives the C ABI on either build; `check(case, got)` compares with
the float64 statement of tests/bn_ref64.py.

Bars (from the arithmetic of ganet_amd/csrc/bn_kernels.h, none of them taken from what the kernels return; bn_ref64's
Float32Model, that arithmetic on numpy, has to stay inside half of each -- tests/test_sim_bn.py):
  save_mean      |mean - mean64| <= 2^-23 sum|x| / M: the one rounding of an fp64 mean (2^-24 |mean|) and the fp64 sum's own
                 error, far below.  `exact` cases (integer x, M a power of two): save_mean == float32(mean64)
  save_invstd    2^-22 relative: one rounding (2^-24) plus the fp64 statistic
  running stats  2^-22 relative to (1 - m) |old| + m |new|
  y              B_y = 2^-21 ((|x| + |mean64|) |scale64| + |bias| + |rem|) per element: scale (2 roundings), the rounded mean,
                 shift's and z's fmaf and the residual add, each at most 2^-24 of a term of that sum
  grad_x         |scale64| (2^-20 (|g| + |k1| + |xhat q~|) + 2^-23 |mean64| invstd64 |q~|), xhat = (x - mean64) invstd64,
                 q~ = grad_weight64 / M; the second term is the fp32 rounding of the saved mean
  grad_weight,   2^-22 relative to the sum of the absolute terms (invstd sum |g (x - mean)|, sum |g|)
  grad_bias      `mean_term` cases add 2^-22 |mean64| invstd64 |sum g| to grad_weight's (and |scale64| |xhat| invstd64 |k1| times
                 the same to grad_x's, through q): the kernels subtract the SAVED fp32 mean,
                 whose rounding (2^-24 |mean|) reaches the sum as sum g times that -- nothing beside the first term while the
                 spread of a channel is comparable with its mean, as in every randn case, and all of the error where it is not
                 (the far-mean cases: two elements per channel, 0.002 apart at a mean of order 1 -- the shape and values GANet_deep's
                 deepest feature level has at a 48x96 crop, where tests/model_calls.py met it)
  grad_rem       equal to g
The gradient bars mean something only where the ReLU mask is decided: `Case` nudges every element with |z64| <= 4 B_y away
from the kink (the residual where there is one, else x) and tests/test_sim_bn.py asserts that none is left; nothing is masked
out of a comparison.  The cancellation family (x = 1000 + 0.01 randn) has thousands of such elements: its statistics and y
are compared, its gradients are not."""
import numpy as np

import bn_ref64 as ref

F32 = np.float32
BLOCK, MAX_ROWS, TARGET_BLOCKS = 256, 64, 2048      # ganet_amd/csrc/bn_kernels.h: BN_BLOCK, BN_MAX_ROWS, BN_TARGET_BLOCKS
STRIDE = BLOCK * MAX_ROWS                           # lanes of one trip of a channel's grid-stride loop (C <= 32)
EPS = 1e-5


def rows(N, C, S, vec):
    """(Rs, Rn) as the launcher chooses them (ganet_capi.hip: bn_geom)"""
    cap = min(MAX_ROWS, max(1, TARGET_BLOCKS // C))
    rs = min(cap, -(-(S // 4 if vec else S) // BLOCK))
    return rs, min(N, cap // rs)


class Case:
    def __init__(self, name, shape, seed, relu=True, rem=False, offset=0, affine=True, running=True, momentum=0.1, eps=EPS,
                 weight=None, bias=None, x=None, exact=False, compare_grads=True, nudge=True, step=0.25, mean_term=False):
        rng = np.random.default_rng(seed)
        N, C, S = shape
        self.name, self.shape, self.relu, self.offset, self.exact = name, tuple(shape), bool(relu), offset, exact
        self.momentum, self.eps, self.compare_grads, self.mean_term = momentum, eps, compare_grads, mean_term
        if x is None:
            x = rng.normal(0, 1.5, shape) + rng.normal(0, 1, (1, C, 1))
        self.x = np.ascontiguousarray(x, F32).reshape(shape)
        self.rem = rng.normal(0, 1, shape).astype(F32) if rem else None
        self.gy = rng.normal(0, 1, shape).astype(F32)
        if affine:
            self.weight = (rng.uniform(0.5, 1.5, C) if weight is None else np.asarray(weight)).astype(F32)
            self.bias = (rng.normal(0, 0.5, C) if bias is None else np.asarray(bias)).astype(F32)
        else:
            self.weight = self.bias = None
        self.running_mean = rng.normal(0, 1, C).astype(F32) if running else None
        self.running_var = rng.uniform(0.5, 2, C).astype(F32) if running else None
        self._ref = None
        self.nudged = 0
        if relu and nudge:
            for _ in range(20):
                und = self.ref.undecided()
                if not und.any():
                    break
                self.nudged += int(und.sum())
                sign = np.where(self.ref.z[und] < 0, -1, 1).astype(F32)
                if self.rem is not None:
                    self.rem[und] += sign * F32(0.5)
                else:
                    self.x[und] += F32(step) * sign * np.broadcast_to(np.sign(self.ref.scale)[None, :, None], shape)[und].astype(F32)
                self._ref = None

    def __repr__(self):
        return self.name

    @property
    def vec(self):
        return self.shape[2] % 4 == 0 and self.offset % 4 == 0

    def inputs(self):
        return (self.x, self.rem, self.gy, self.weight, self.bias, self.running_mean, self.running_var, self.momentum, self.eps, self.relu)

    @property
    def ref(self):
        """computed once, shared by every test that runs the case"""
        if self._ref is None:
            self._ref = ref.Reference(*self.inputs())
        return self._ref

    def with_x(self, name, x=None, rem=None):
        """the same case on other values (no nudging: the NaN pairs)"""
        import copy
        c = copy.copy(self)
        c.name, c._ref = name, None
        c.x = self.x if x is None else np.ascontiguousarray(x, F32)
        c.rem = self.rem if rem is None else np.ascontiguousarray(rem, F32)
        return c


def _cases():
    cs = []
    seed = [200]

    def add(tag, shape, R=False, **kw):
        for relu in (True, False):
            for rem in ((False, True) if R else (False,)):
                seed[0] += 1
                cs.append(Case(f"{tag}{'-relu' if relu else ''}{'-rem' if rem else ''}", shape, seed[0], relu=relu, rem=rem, **kw))

    # vector twin and scalar twin
    add("min-1x1x2", (1, 1, 2))
    add("scalar-3x2x7", (3, 2, 7))
    add("vec-2x3x8", (2, 3, 8))
    add("vec-size-offset1-2x3x12", (2, 3, 12), offset=1)
    add("odd-2x5x819", (2, 5, 819), R=True)
    # tails: one lane past a block's 256 (BN_BLOCK); second trips: one lane past 64 rows x 256 lanes (BN_MAX_ROWS x BN_BLOCK)
    # with N = 2 on Rn = 1, so the loop over the slices, the grid-stride loop and the loop over the 64 rows all come round again
    add("tail-scalar-1x2x257", (1, 2, BLOCK + 1))
    add("tail-vec-1x2x1028", (1, 2, 4 * (BLOCK + 1)))
    add("trip2-scalar-2x1x16385", (2, 1, STRIDE + 1), R=True)
    add("trip2-vec-2x1x65540", (2, 1, 4 * (STRIDE + 1)))
    add("blocks-2x4x1024", (2, 4, 1024), R=True)
    # slices per channel: N > C, the rows of one channel come from five slices; many channels: the row cap below 64
    add("slices-5x1x64", (5, 1, 64))
    add("channels-2x70x4", (2, 70, 4))
    # sign and degenerate parameters
    add("neg-weights", (2, 4, 36), R=True, weight=[-1.25, 0.75, -0.5, 1.0])
    add("weight0-bias0", (2, 3, 40), weight=[1.0, 0.0, -0.75], bias=[0.25, 0.0, -0.5])       # channel 1: z exactly 0
    add("weight0-bias0-offset1", (2, 3, 40), weight=[1.0, 0.0, -0.75], bias=[0.25, 0.0, -0.5], offset=1)
    add("no-affine", (2, 3, 20), R=True, affine=False)
    add("no-running", (2, 3, 20), running=False)
    add("momentum1", (2, 3, 20), momentum=1.0)
    # cancellation: an fp32 sum of squares loses this variance entirely
    rng = np.random.default_rng(77)
    x = (1000.0 + 0.01 * rng.normal(0, 1, (1, 5, 4097))).astype(F32)
    for relu in (True, False):
        cs.append(Case(f"cancellation-1x5x4097{'-relu' if relu else ''}", (1, 5, 4097), 78, relu=relu, x=x, compare_grads=False, nudge=False))
    # a channel's two elements 0.002 apart at a mean of order 1: the rounding of the saved mean is all of grad_weight's error
    rng = np.random.default_rng(79)
    x = (rng.normal(0, 1, (1, 128, 1)) + 0.002 * rng.normal(0, 1, (1, 128, 2))).astype(F32)
    for relu in (True, False):
        cs.append(Case(f"far-mean-1x128x2{'-relu' if relu else ''}", (1, 128, 2), 80, relu=relu, x=x, step=5e-4, mean_term=True))
    # exact: integer x in [-8, 8], M a power of two
    for tag, shape, off in (("256", (2, 3, 128), 0), ("64-offset1", (4, 2, 16), 1), ("32768", (2, 2, 8192), 0)):
        x = np.random.default_rng(90).integers(-8, 9, shape).astype(F32)
        x[0, :, 0] = 8                      # (an origin other than zero for the sums)
        cs.append(Case("exact-" + tag, shape, 91, x=x, exact=True, offset=off, momentum=1.0, step=1.0))
    return cs


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


def nan_pairs():
    """(clean, dirty, channel, where): one NaN in x's channel `channel`; one NaN in rem alone"""
    out = []
    for name in ("odd-2x5x819-relu-rem", "blocks-2x4x1024-relu", "blocks-2x4x1024"):
        base = BY_NAME[name]
        x = base.x.copy()
        x[1, 2, 5] = np.nan
        out.append((base, base.with_x(name + "-nan-x", x=x), 2, "x"))
    base = BY_NAME["odd-2x5x819-relu-rem"]
    rem = base.rem.copy()
    rem[0, 3, 11] = np.nan
    out.append((base, base.with_x(base.name + "-nan-rem", rem=rem), 3, "rem"))
    return out


# ---- running a case through the C ABI on either build ---------------------------------------------------------------------

def fbits(v):
    return int(F32(v).view(np.int32))


def run(api, dev, case, want=(True, True, True, True), ws_fill=None):
    """forward + backward through the C ABI.  dev: parity_cases.NumpyDev (emulator) or test_gpu_parity.TorchDev.  Outputs are
    poisoned first, so an element that is not written shows.  offset: every volume starts 4 * offset bytes behind a 16-byte
    boundary.  want: (grad_x, grad_rem, grad_weight, grad_bias); ws_fill: the workspace's prior content (default: NaN)."""
    N, C, S = case.shape
    n, off = N * C * S, case.offset
    keep = {}

    def put(key, a):
        if a is None:
            return None
        buf = dev.to(np.concatenate([np.full(off, 7.0, F32), np.asarray(a, F32).ravel()]))
        keep[key] = buf
        return dev.ptr(buf) + 4 * off

    def out(key, wanted=True):
        if not wanted:
            return None
        keep[key] = dev.empty((off + n,))
        return dev.ptr(keep[key]) + 4 * off

    def small_in(key, a):
        if a is None:
            return None
        keep[key] = dev.to(np.asarray(a, F32))
        return dev.ptr(keep[key])

    def small(key, wanted=True):
        if not wanted:
            return None
        keep[key] = dev.empty((C,))
        return dev.ptr(keep[key])

    xp, rp, gp = put("x", case.x), put("rem", case.rem), put("gy", case.gy)
    wp, bp = small_in("in_w", case.weight), small_in("in_b", case.bias)
    rmp, rvp = small_in("in_rm", case.running_mean), small_in("in_rv", case.running_var)
    nws = api.query("ganet_bn_workspace", N, C, S)
    ws = dev.empty((2 * nws,), np.float32)             # fp64 scratch, NaN bit patterns all over
    if ws_fill is not None:
        ws = dev.to(np.full(2 * nws, ws_fill, F32))
    yp, smp, sip = out("y"), small("save_mean"), small("save_invstd")
    api.call("ganet_bn_train_forward", xp, rp, wp, bp, rmp, rvp, dev.ptr(ws), yp, smp, sip, N, C, S, fbits(case.momentum),
             fbits(case.eps), int(case.relu), dev.stream)
    want = (want[0], want[1] and case.rem is not None, want[2] and case.weight is not None, want[3] and case.weight is not None)
    gxp, grp = out("grad_x", want[0]), out("grad_rem", want[1])
    gwp, gbp = small("grad_weight", want[2]), small("grad_bias", want[3])
    api.call("ganet_bn_train_backward", xp, rp, gp, wp, bp, smp, sip, dev.ptr(ws), gxp, grp, gwp, gbp, N, C, S,
             int(case.relu), dev.stream)
    dev.sync()
    got = {}
    for key, buf in keep.items():
        a = np.array(dev.host(buf))
        got[key] = a[off:].reshape(case.shape) if a.size == off + n and key in ("x", "rem", "gy", "y", "grad_x", "grad_rem") else a
        if a.size == off + n and off:
            assert (a[:off] == 7.0).all() or np.isnan(a[:off]).all(), f"{key}: written in front of the tensor"
    got["running_mean"], got["running_var"] = got.pop("in_rm", None), got.pop("in_rv", None)
    return got


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def within(what, got, want, bar, verbose=True, enforce=True):
    """|got - want| <= bar element by element; a NaN exactly where the statement has one.  Returns the worst error / bar.
    enforce=False: a measurement (of the stock kernels), nothing is asserted."""
    got, want, bar = np.asarray(got, np.float64), np.asarray(want, np.float64), np.broadcast_to(np.asarray(bar, np.float64), np.shape(want))
    nan = np.isnan(want)
    assert not enforce or np.array_equal(np.isnan(got), nan), f"{what}: NaNs elsewhere than the float64 statement has them"
    err = np.abs(got - want)[~nan]
    ok = err <= bar[~nan]
    with np.errstate(all="ignore"):
        ratio = float(np.max(np.where(bar[~nan] > 0, err / bar[~nan], np.where(err > 0, np.inf, 0.0)), initial=0.0))
    if verbose:
        print(f"  {what}: worst error / bar = {ratio:.3f}")
    assert not enforce or ok.all(), f"{what}: {int((~ok).sum())} of {ok.size} outside the bar, worst ratio {ratio:.3g}"
    return ratio


def check(case, got, want=(True, True, True, True), verbose=True, enforce=True, saved=True):
    """got: what `run` returns.  saved=False: a module's results -- no save_mean / save_invstd to look at, no input copies.
    enforce=False: measure only (the stock chain).  Returns the worst error / bar per quantity."""
    r = case.ref
    if verbose:
        print(case.name)
    ratios = {}
    if saved:
        # inputs untouched
        for key, a in (("x", case.x), ("rem", case.rem), ("gy", case.gy), ("in_w", case.weight), ("in_b", case.bias)):
            if a is not None:
                assert np.array_equal(bits(got[key]).ravel(), bits(a).ravel()), f"{key} was written"
        if case.exact:
            assert np.array_equal(bits(got["save_mean"]), bits(r.mean.astype(F32))), (got["save_mean"], r.mean)
        ratios["save_mean"] = within("save_mean", got["save_mean"], r.mean, 2.0 ** -23 * r.mean_abs_x, verbose)
        ratios["save_invstd"] = within("save_invstd", got["save_invstd"], r.invstd, 2.0 ** -22 * r.invstd, verbose)
    if case.running_mean is not None:
        m = r.m
        ratios["running_mean"] = within("running_mean", got["running_mean"], r.running_mean,
                                        2.0 ** -22 * ((1 - m) * np.abs(r.old_mean) + m * np.abs(r.mean)), verbose, enforce)
        ratios["running_var"] = within("running_var", got["running_var"], r.running_var,
                                       2.0 ** -22 * ((1 - m) * np.abs(r.old_var) + m * np.abs(r.new_var)), verbose, enforce)
    else:
        assert got["running_mean"] is None
    ratios["y"] = within("y", got["y"], r.y, r.bar_y(), verbose, enforce)
    if not case.compare_grads:
        return ratios
    want = (want[0], want[1] and case.rem is not None, want[2] and case.weight is not None, want[3] and case.weight is not None)
    for key, w in zip(("grad_x", "grad_rem", "grad_weight", "grad_bias"), want):
        assert (key in got) == bool(w), key
    if want[0]:
        ratios["grad_x"] = within("grad_x", got["grad_x"], r.grad_x, r.bar_grad_x(getattr(case, "mean_term", False)), verbose, enforce)
    if want[1]:
        g32 = r.g.astype(F32)
        nan = np.isnan(g32)
        assert not enforce or (np.array_equal(np.isnan(got["grad_rem"]), nan) and np.array_equal(got["grad_rem"][~nan], g32[~nan])), "grad_rem is not g"
    if want[2]:
        bar = 2.0 ** -22 * r.invstd * r.sum_abs_gxm
        if getattr(case, "mean_term", False):
            bar = bar + 2.0 ** -22 * np.abs(r.mean) * r.invstd * np.abs(r.sum_g)
        ratios["grad_weight"] = within("grad_weight", got["grad_weight"], r.grad_weight, bar, verbose, enforce)
    if want[3]:
        ratios["grad_bias"] = within("grad_bias", got["grad_bias"], r.grad_bias, 2.0 ** -22 * r.sum_abs_g, verbose, enforce)
    return ratios


def model_as_got(case):
    """bn_ref64.Float32Model's results in the layout `run` returns"""
    m = ref.Float32Model(*case.inputs())
    got = {"x": case.x, "rem": case.rem, "gy": case.gy, "in_w": case.weight, "in_b": case.bias, "y": m.y,
           "save_mean": m.save_mean, "save_invstd": m.save_invstd, "grad_x": m.grad_x,
           "running_mean": getattr(m, "running_mean", None), "running_var": getattr(m, "running_var", None)}
    if case.rem is not None:
        got["grad_rem"] = m.grad_rem
    if case.weight is not None:
        got["grad_weight"], got["grad_bias"] = m.grad_weight, m.grad_bias
    return got


# ---- test bodies both builds share ----------------------------------------------------------------------------------------

RESULTS = ("y", "save_mean", "save_invstd", "running_mean", "running_var", "grad_x", "grad_rem", "grad_weight", "grad_bias")
REPRODUCIBLE = ["odd-2x5x819-relu-rem", "trip2-vec-2x1x65540-relu", "slices-5x1x64"]
EVAL_FORM = ["odd-2x5x819-relu-rem", "vec-2x3x8-relu", "vec-size-offset1-2x3x12", "tail-vec-1x2x1028-relu", "min-1x1x2"]
WANTED = [(True, False, False, False), (False, True, True, True), (False, False, True, True), (False, False, False, False)]


def same(a, b):
    for k in RESULTS:
        if a.get(k) is not None or b.get(k) is not None:
            assert np.array_equal(bits(a[k]), bits(b[k])), k


def check_reproducible(api, dev, case):
    """two runs are bit-identical, and so is one whose workspace held zeros instead of NaN"""
    a, b, c = run(api, dev, case), run(api, dev, case), run(api, dev, case, ws_fill=0.0)
    same(a, b)
    same(a, c)


def check_nan_pair(api, dev, pair):
    """a NaN in x: its channel's y, statistics, grad_x and grad_weight are NaN -- grad_bias = sum g is not: z <= 0 is false for
    a NaN, so g = grad_y there, the ATen rule, and the float64 statement has the same finite sum -- and every other channel is
    bit-equal to the run without; a NaN in rem alone passes through at its element and leaves the statistics finite"""
    clean, dirty, ch, where = pair
    a, b = run(api, dev, clean), run(api, dev, dirty)
    others = [c for c in range(clean.shape[1]) if c != ch]
    if where == "x":
        for k in ("y", "grad_x"):                       # (grad_rem is g = grad_y there)
            assert np.isnan(b[k][:, ch]).all(), k
        for k in ("save_mean", "save_invstd", "running_mean", "running_var", "grad_weight"):
            assert np.isnan(b[k][ch]), k
        assert np.isfinite(b["grad_bias"]).all()
    else:
        assert np.isnan(b["y"][0, ch, 11]) and np.isnan(b["y"]).sum() == 1 and np.isfinite(b["save_mean"]).all()
        assert np.isfinite(b["save_invstd"]).all() and np.isfinite(b["running_var"]).all() and np.isfinite(b["grad_x"]).all()
    check(dirty, b)                                     # NaNs exactly where the float64 statement has them
    for k in ("y", "grad_x", "grad_rem"):
        if k in a:
            assert np.array_equal(bits(a[k][:, others]), bits(b[k][:, others])), k
    for k in ("save_mean", "save_invstd", "running_mean", "running_var", "grad_weight", "grad_bias"):
        assert np.array_equal(bits(a[k][others]), bits(b[k][others])), k


def check_eval_form(api, dev, c, inplace):
    """ganet_bn_apply_forward: y = relu(scale[c] x + shift[c] [+ rem]), bit-equal to the fp32 statement; y may be x"""
    N, C, S = c.shape
    rng = np.random.default_rng(5)
    scale, shift = rng.normal(0, 1, C).astype(F32), rng.normal(0, 1, C).astype(F32)
    off = c.offset
    put = lambda a: dev.to(np.concatenate([np.full(off, 7.0, F32), np.asarray(a, F32).ravel()]))   # noqa: E731
    xb, rb = put(c.x), (put(c.rem) if c.rem is not None else None)
    yb = xb if inplace else dev.empty((off + c.x.size,))
    sb, hb = dev.to(scale), dev.to(shift)
    api.call("ganet_bn_apply_forward", dev.ptr(xb) + 4 * off, dev.ptr(rb) + 4 * off if rb is not None else None, dev.ptr(sb), dev.ptr(hb),
             dev.ptr(yb) + 4 * off, N, C, S, int(c.relu), dev.stream)
    dev.sync()
    z = ref._fma32(c.x, scale[None, :, None], shift[None, :, None])
    if c.rem is not None:
        z = (z + c.rem).astype(F32)
    want = np.where(z <= 0, F32(0), z) if c.relu else z
    assert np.array_equal(bits(np.array(dev.host(yb))[off:]), bits(want).ravel())
    if not inplace:
        assert np.array_equal(bits(np.array(dev.host(xb))[off:]), bits(c.x).ravel())


def check_bad_arguments(api, dev):
    import pytest
    from ganet_amd._native import E_INVALID, E_UNSUPPORTED, GanetError
    c = BY_NAME["vec-2x3x8-relu"]
    N, C, S = c.shape
    x, gy, y, gx = dev.to(c.x.ravel()), dev.to(c.gy.ravel()), dev.empty((c.x.size,)), dev.empty((c.x.size,))
    sm, si = dev.empty((C,)), dev.empty((C,))
    ws = dev.empty((2 * api.query("ganet_bn_workspace", N, C, S),))
    p = dev.ptr

    def fwd(xp=p(x), yp=p(y), dims=(N, C, S)):
        api.call("ganet_bn_train_forward", xp, None, None, None, None, None, p(ws), yp, p(sm), p(si), *dims, fbits(0.1),
                 fbits(1e-5), 1, dev.stream)

    def bwd(xp=p(x), gxp=p(gx), dims=(N, C, S)):
        api.call("ganet_bn_train_backward", xp, None, p(gy), None, None, p(sm), p(si), p(ws), gxp, None, None, None, *dims, 1, dev.stream)

    fwd()
    bwd()
    for call in (fwd, bwd):
        for kw in (dict(xp=None), dict(dims=(N, 0, S)), dict(dims=(1, C, 1)), dict(dims=(0, C, S)), dict(dims=(N, C, -4))):
            with pytest.raises(GanetError) as e:
                call(**kw)
            assert e.value.code == E_INVALID and "ganet_bn_train" in str(e.value), kw
            assert "ganet_bn_train" in api.last_error()
    for call in (lambda: fwd(yp=p(x)), lambda: bwd(gxp=p(x)), lambda: bwd(gxp=p(gy))):          # no aliasing in the training entries
        with pytest.raises(GanetError) as e:
            call()
        assert e.value.code == E_INVALID
    for dims, code in (((1, 0, 4), E_INVALID), ((1, 1, 1), E_INVALID), ((1, 70000, 4), E_UNSUPPORTED)):
        with pytest.raises(GanetError) as e:
            api.query("ganet_bn_workspace", *dims)
        assert e.value.code == code
    assert api.query("ganet_bn_workspace", 1, 1, 2) == 2 * MAX_ROWS and api.query("ganet_bn_workspace", 1, 4096, 2) == 2 * 4096
    with pytest.raises(GanetError) as e:
        api.call("ganet_bn_apply_forward", p(x), None, None, p(si), p(y), N, C, S, 1, dev.stream)
    assert e.value.code == E_INVALID
    dev.sync()
