"""TEST INFRASTRUCTURE: the case table of the mixed-precision TRAINING kernels (ganet_amd/csrc/bn_kernels.h, mixed_train_kernels.h and
misc_kernels.h's l1norm_bwd<KT, Tx>: ganet_bn_train_forward_mixed / _backward_mixed, ganet_cost_volume_backward_16,
ganet_l1_normalize_backward_mixed), run on the emulator by tests/test_sim_mixed_train.py and on the device by
tests/test_gpu_mixed_train.py through one `dev` (parity_cases.NumpyDev / test_gpu_parity.TorchDev), as tests/mixed_cases.py is.

Per-element outputs have no tolerance: the cost-volume and the normalise backward fix their summation order per output element, so
    op_16(a16, ...) == convert(op_fp32(upcast(a16), ...), out_type)            bit for bit, NaN positions equal
with op_fp32 the fp32 entry of the SAME build.

The BatchNorm statistics are reductions whose order the geometry decides (eight elements per lane here, four in the fp32
kernels), so their contract has two tiers:
  exact    inputs on a dyadic grid, representable in both 16-bit formats, every channel's mean on the grid: the four fp64 sums
           (sum d, sum d^2, sum g, sum g (x - mean)) are exact whatever their order -- `assert_exact` shows it in integer
           arithmetic, every term a multiple of a unit u with sum |term| / u < 2^53 -- and EVERY output equals the fp32 entry's on
           the up-cast input, rounded once where it is stored in 16 bits.  The fp32 entry's own vector and scalar twins are held
           to the same bits on these inputs first (`check_fp32_twins_agree`).
  general  seeded randn rounded to 16 bits, and bn_cases' cancellation and far-mean families: save_mean, save_invstd, the running
           buffers, grad_weight and grad_bias inside the bars tests/bn_cases.py derives for the fp32 kernels (the arithmetic is the
           same, so are the bars; no new number), against bn_ref64.Reference on the up-cast input.  y == convert(z32, y_type) bit
           for bit, z32 the float32 expression of bn_kernels.h (scale = weight invstd, shift = fmaf(-mean, scale, bias),
           z = fmaf(x, scale, shift) [+ rem]) evaluated with the statistics THE KERNEL RETURNED; ReLU cases are nudged off the
           kink first and none is left undecided.  grad_x within bar_grad_x plus half a unit in the last place of the stored
           format (the one rounding the store adds: `half_ulp`, at most 2^-8 |v| for bf16 and 2^-11 |v| for fp16, from the
           formats' 8 and 11 significant bits); grad_rem is fp32 and equals g.  Two runs are bit-identical.
Sizes come from the launchers' constants (bn_kernels.h / mixed_kernels.h, checked against the sources by the sim test)."""
import numpy as np

import bn_cases as bc
from mixed_cases import BF16, BN_BLOCK, BN_MAX_ROWS, BN_TARGET_BLOCKS, CV_CASES, F16, F32, FMT_NAME, MX_V, Buf, CvCase, L1Case
from mixed_cases import E_INVALID, E_UNSUPPORTED, _rc, assert_same, convert, is_nan, l1_data, up

f32 = np.float32
EW_GRID_LANES = 256 * 16 * 256           # ganet_capi.hip: ew_grid's cap of 256 * 16 blocks of 256 lanes

# the three sites of a model under autocast: (rem, y / grad_y storage)
SITES = {"conv": (False, "16"), "pre-sga": (False, "f32"), "tail": (True, "16")}


def half_ulp(v, fmt):
    """half a unit in the last place of `fmt` at |v| (8 significant bits for bf16, 11 for fp16; subnormal spacing below)"""
    p, emin = (8, -126) if fmt == BF16 else (11, -14)
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.maximum(np.abs(np.asarray(v, np.float64)), 2.0 ** emin)))
    return 2.0 ** (e - p)


def fma32(a, b, c):
    """fmaf on fp32 arrays, correctly rounded: bn_ref64._fma32 (an exact product, one float64 add, one rounding to fp32) is off by
    an ulp only where the float64 sum was inexact AND lies on a tie of fp32; those elements are redone in rationals"""
    from fractions import Fraction
    a, b, c = (np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32)))
    p, c64 = a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64)
    with np.errstate(all="ignore"):
        s = p + c64
        t = s - p
        err = (p - (s - t)) + (c64 - t)                    # TwoSum: s + err == p + c exactly
        out = s.astype(f32)
        tie = np.isfinite(s) & (err != 0) & ((s.view(np.uint64) & np.uint64((1 << 29) - 1)) == np.uint64(1 << 28))
    for i in np.flatnonzero(tie.ravel()):
        exact = Fraction(float(p.ravel()[i])) + Fraction(float(c64.ravel()[i]))
        lo, hi = np.nextafter(out.ravel()[i], f32(-np.inf)), np.nextafter(out.ravel()[i], f32(np.inf))
        out.ravel()[i] = min((out.ravel()[i], lo, hi), key=lambda v: abs(Fraction(float(v)) - exact))
    return out


# ---- BatchNorm -----------------------------------------------------------------------------------------------------------------

class Case:
    """one shape and parameter set; `data(fmt, site)` makes its inputs for a tier:
    exact    x = c0[c] + k / 4, k a symmetric set of integers in [-8, 8] (so the channel's mean is c0[c], on the grid),
             grad_y = integers in [-4, 4] / 8, rem = integers in [-4, 4] / 2
    general  randn (bn_cases.Case's own draw) rounded to the format; `x=` replaces it (the cancellation and far-mean families)
    special  exact with NaN, +-inf and -0 put in (`check_special`)"""

    def __init__(self, name, shape, tier, seed, off=0, weight="rand", running=True, momentum=0.1, x=None, compare_grads=True,
                 mean_term=False, step=0.25, sites=tuple(SITES), relus=(True, False), special="x"):
        self.name, self.shape, self.tier, self.seed, self.off = name, tuple(shape), tier, seed, off
        self.weight, self.running, self.momentum, self.x = weight, running, momentum, x
        self.compare_grads, self.mean_term, self.step, self.sites, self.relus = compare_grads, mean_term, step, sites, relus
        self.special = special
        self._data = {}

    def __repr__(self):
        return self.name

    def vec(self):
        return self.shape[2] % MX_V == 0 and self.off == 0

    def data(self, fmt, site, relu):
        """a bn_cases.Case whose x (and grad_y where the site stores it in 16 bits) are exact in `fmt`; computed once"""
        key = (fmt, site, relu)
        if key not in self._data:
            self._data[key] = self._make(fmt, site, relu)
        return self._data[key]

    def _make(self, fmt, site, relu):
        N, C, S = self.shape
        has_rem, y_kind = SITES[site]
        rng = np.random.default_rng(self.seed)
        r16 = lambda a: up(convert(np.asarray(a, f32), fmt), fmt).reshape(np.shape(a))        # noqa: E731
        kw = dict(relu=relu, rem=has_rem, running=self.running, momentum=self.momentum, nudge=False, mean_term=self.mean_term)
        if isinstance(self.weight, tuple):
            kw.update(weight=self.weight[0], bias=self.weight[1])
        elif self.weight is None:
            kw.update(affine=False)
        if self.tier in ("exact", "special"):
            M = N * S
            k = rng.integers(-8, 9, (C, M // 2))
            k = np.concatenate([k, -k] + ([np.zeros((C, 1), np.int64)] if M % 2 else []), axis=1)
            k = rng.permuted(k, axis=1)
            c0 = np.resize(np.array([1.0, -0.5, 0.0, 2.0, -1.25]), C)
            x = (c0[:, None] + k / 4.0).reshape(C, N, S).transpose(1, 0, 2)
            c = bc.Case(self.name, self.shape, self.seed, x=x, **kw)
            c.gy = (rng.integers(-4, 5, self.shape) / 8.0).astype(f32)
            if has_rem:
                c.rem = (rng.integers(-4, 5, self.shape) / 2.0).astype(f32)
            c.c0 = c0
            for a in (c.x, c.gy):
                assert np.array_equal(r16(a), a), "an exact-tier input is not representable in the 16-bit format"
            if self.tier == "special":
                # on top of exact data (checked as such first): channel 0 keeps finite statistics -- -0 in x, and NaN, +-inf and
                # -0 in rem pass through at their elements; channel 1 has one NaN in x, channel 2 an infinity; `gy`: NaN and
                # +inf in channel 0's grad_y as well
                assert_exact(c)
                assert C >= 3
                c.x[0, 0, np.flatnonzero(c.x[0, 0] == 0)[::2]] = -0.0
                c.x[N - 1, 1, S // 2] = np.nan
                c.x[0, 2, S - 1] = np.inf if self.seed % 2 else -np.inf
                c.gy[0, 1, 3] = -0.0
                if has_rem:
                    c.rem[0, 0, 1], c.rem[0, 0, 5], c.rem[0, 0, 9], c.rem[0, 0, 13] = np.nan, np.inf, -np.inf, -0.0
                if self.special == "gy":
                    c.gy[0, 0, 2], c.gy[N - 1, 0, S - 2] = np.nan, np.inf
            return c
        c = bc.Case(self.name, self.shape, self.seed, x=self.x, **kw)
        c.x = r16(c.x)
        if y_kind == "16":
            c.gy = r16(c.gy)
        if relu:
            # bn_cases.Case's nudge, with x brought back onto the format's grid after every step
            for _ in range(40):
                c._ref = None
                und = c.ref.undecided()
                if not und.any():
                    break
                sign = np.where(c.ref.z[und] < 0, -1, 1).astype(f32)
                if c.rem is not None:
                    c.rem[und] += sign * f32(0.5)
                else:
                    c.x[und] += f32(self.step) * sign * np.broadcast_to(np.sign(c.ref.scale)[None, :, None], self.shape)[und].astype(f32)
                    c.x = r16(c.x)
            c._ref = None
        return c


def assert_exact(c):
    """an exact-tier bn_cases.Case: every term of the four sums is an integer multiple of a unit, and the sum of the absolute
    terms stays below 2^53 units -- so each fp64 sum is exact in any order.  Integer arithmetic throughout."""
    N, C, S = c.shape
    xi = np.rint(c.x.astype(np.float64) * 4).astype(np.int64)                 # units of 1/4
    gi = np.rint(c.gy.astype(np.float64) * 8).astype(np.int64)                # units of 1/8
    assert np.array_equal(xi / 4.0, c.x) and np.array_equal(gi / 8.0, c.gy)
    c0i = np.rint(c.c0 * 4).astype(np.int64)
    assert np.array_equal(c0i / 4.0, c.c0)
    assert np.array_equal(xi.sum(axis=(0, 2)), c0i * N * S), "a channel's mean is off the grid"
    assert np.array_equal(f32(c.c0).astype(np.float64), c.c0)                 # the fp32-rounded mean IS the mean
    d = xi - xi[0, :, 0][None, :, None]                                       # d = x - x0, units of 1/4
    for terms in (d, d * d, gi, gi * (xi - c0i[None, :, None])):              # units 1/4, 1/16, 1/8, 1/32
        assert int(np.abs(terms).sum(axis=(0, 2)).max()) < 2 ** 53
    if c.rem is not None:
        assert np.array_equal(np.rint(c.rem * 2) / 2.0, c.rem)


def _cases():
    cs, seed = [], [400]

    def add(name, shape, tiers=("exact", "general"), **kw):
        for tier in tiers:
            seed[0] += 1
            cs.append(Case(f"{name}-{tier}", shape, tier, seed[0], **kw))

    one_trip = BN_MAX_ROWS * BN_BLOCK
    add("vec-2x3x8", (2, 3, 8))
    add("odd-2x5x819", (2, 5, 819))
    add("S12", (2, 3, 12))                                   # S % 8 == 4: fp32's vector, this kernel's scalar twin
    add("S10", (2, 3, 10))                                   # S % 8 == 2
    add("offset1-2x3x16", (2, 3, 16), off=1)
    add("tail-vec", (1, 2, MX_V * (BN_BLOCK + 1)))           # one lane past a block
    add("tail-scalar", (1, 2, BN_BLOCK + 1))
    add("tail-vec+4", (1, 2, MX_V * BN_BLOCK + 4), sites=("tail",))
    add("trip2-vec", (2, 1, MX_V * one_trip + MX_V))         # the second trip of the partial-sum and apply loops, 64 rows
    add("trip2-scalar", (2, 1, one_trip + 1), sites=("tail",))
    add("slices-5x1x64", (5, 1, 64))                         # N > C
    add("channels-2x70x8", (2, BN_TARGET_BLOCKS // 29, 8), sites=("conv", "tail"), relus=(True,))   # C = 70: the row cap below BN_MAX_ROWS
    add("neg-weights", (2, 4, 40), weight=([-1.25, 0.75, -0.5, 1.0], [0.25, -0.5, 0.0, 1.0]))
    add("weight0-bias0", (2, 3, 40), weight=([1.0, 0.0, -0.75], [0.25, 0.0, -0.5]))
    add("no-affine", (2, 3, 24), weight=None)
    add("no-running", (2, 3, 24), running=False)
    add("momentum1", (2, 3, 24), momentum=1.0)
    add("M2-1x1x2", (1, 1, 2))
    add("M2-2x3x1", (2, 3, 1))
    add("special-vec", (2, 3, 64), tiers=("special",))
    add("special-odd", (2, 3, 61), tiers=("special",))
    add("special-gy-vec", (2, 3, 64), tiers=("special",), special="gy")
    rng = np.random.default_rng(77)
    cs.append(Case("cancellation-1x5x4097-general", (1, 5, 4097), "general", 78, x=(1000.0 + 0.01 * rng.normal(0, 1, (1, 5, 4097))).astype(f32),
                   compare_grads=False, sites=("conv", "pre-sga")))
    rng = np.random.default_rng(79)
    cs.append(Case("far-mean-1x128x2-general", (1, 128, 2), "general", 80, mean_term=True, step=2.0 ** -6,
                   x=(rng.normal(0, 1, (1, 128, 1)) + 0.002 * rng.normal(0, 1, (1, 128, 2))).astype(f32)))
    assert BN_TARGET_BLOCKS // 29 == 70
    return cs


BN_TRAIN_CASES = _cases()
BN_BY_NAME = {c.name: c for c in BN_TRAIN_CASES}
REPRODUCIBLE = ["odd-2x5x819-general", "trip2-vec-general", "slices-5x1x64-general"]
WANTED_CASES = ["vec-2x3x8-exact", "odd-2x5x819-exact"]
OUT_KEYS = ("y", "save_mean", "save_invstd", "running_mean", "running_var", "grad_x", "grad_rem", "grad_weight", "grad_bias")


def run_bn(api, dev, c, fmt, site, off=0, want=(True, True, True, True), ws_fill=None):
    """forward + backward of the mixed entries on the bn_cases.Case `c` (whose x, and grad_y at a 16-bit site, are exact in fmt).
    Every volume starts `off` elements of its own type behind its allocation; outputs are poisoned.  Returns float32 / uint16
    arrays by bn_cases.run's names, y and grad_x as patterns where they are 16-bit."""
    N, C, S = c.shape
    n = N * C * S
    _, y_kind = SITES[site]
    y_fmt = fmt if y_kind == "16" else F32
    as_fmt = lambda a, t: convert(a, t) if t != F32 else np.asarray(a, f32)            # noqa: E731
    small = lambda a: Buf(dev, F32, data=a) if a is not None else None                 # noqa: E731
    p = lambda b: b.ptr if b is not None else None                                     # noqa: E731
    x = Buf(dev, fmt, data=as_fmt(c.x, fmt), off=off)
    rem = Buf(dev, F32, data=c.rem, off=off) if c.rem is not None else None
    gy = Buf(dev, y_fmt, data=as_fmt(c.gy, y_fmt), off=off)
    w, b, rm, rv = small(c.weight), small(c.bias), small(c.running_mean), small(c.running_var)
    nws = api.query("ganet_bn_workspace", N, C, S)
    ws = dev.empty((2 * nws,), np.float32) if ws_fill is None else dev.to(np.full(2 * nws, ws_fill, f32))
    y, sm, si = Buf(dev, y_fmt, n=n, off=off), Buf(dev, F32, n=C), Buf(dev, F32, n=C)
    api.call("ganet_bn_train_forward_mixed", x.ptr, p(rem), p(w), p(b), p(rm), p(rv), dev.ptr(ws), y.ptr, sm.ptr, si.ptr, N, C, S,
             bc.fbits(c.momentum), bc.fbits(c.eps), int(c.relu), fmt, F32, y_fmt, dev.stream)
    want = (want[0], want[1] and c.rem is not None, want[2] and c.weight is not None, want[3] and c.weight is not None)
    gx = Buf(dev, fmt, n=n, off=off) if want[0] else None
    gr = Buf(dev, F32, n=n, off=off) if want[1] else None
    gw, gb = (Buf(dev, F32, n=C) if want[2] else None), (Buf(dev, F32, n=C) if want[3] else None)
    api.call("ganet_bn_train_backward_mixed", x.ptr, p(rem), gy.ptr, p(w), p(b), sm.ptr, si.ptr, dev.ptr(ws), p(gx), p(gr), p(gw), p(gb),
             N, C, S, int(c.relu), fmt, F32, y_fmt, dev.stream)
    dev.sync()
    for buf, a, t in ((x, c.x, fmt), (gy, c.gy, y_fmt), (rem, c.rem, F32), (w, c.weight, F32), (b, c.bias, F32)):
        if buf is not None:
            assert np.array_equal(buf.host().view(np.uint8), as_fmt(a, t).ravel().view(np.uint8)), "an input was written"
    got = {"y": y.host(c.shape), "save_mean": sm.host(), "save_invstd": si.host(), "y_fmt": y_fmt,
           "running_mean": rm.host() if rm else None, "running_var": rv.host() if rv else None}
    for key, buf in (("grad_x", gx), ("grad_rem", gr)):
        if buf is not None:
            got[key] = buf.host(c.shape)
    for key, buf in (("grad_weight", gw), ("grad_bias", gb)):
        if buf is not None:
            got[key] = buf.host()
    return got


def run_fp32(api, dev, c, offset=0, want=(True, True, True, True)):
    """the fp32 entries on the same values (bn_cases.run), at a chosen base offset"""
    import copy
    c = copy.copy(c)
    c.offset = offset
    return bc.run(api, dev, c, want=want)


def check_fp32_twins_agree(api, dev, c):
    """exact tier: the fp32 entry's vector twin (aligned bases) and its scalar twin (bases one element off) return the same bits"""
    a, b = run_fp32(api, dev, c, 0), run_fp32(api, dev, c, 1)
    for k in OUT_KEYS:
        if a.get(k) is not None:
            assert_same(a[k], b[k], F32, f"{c.name}: fp32 vector against scalar twin, {k}")


def check_exact(api, dev, case, fmt, site, relu, want=(True, True, True, True)):
    c = case.data(fmt, site, relu)
    assert_exact(c)
    got, fp32 = run_bn(api, dev, c, fmt, site, off=case.off, want=want), run_fp32(api, dev, c, 0, want=want)
    what = f"{case.name} {FMT_NAME[fmt]} {site} relu={relu} want={want}"
    assert set(k for k in OUT_KEYS if got.get(k) is not None) == set(k for k in OUT_KEYS if fp32.get(k) is not None), what
    for k in OUT_KEYS:
        if fp32.get(k) is None:
            continue
        t = got["y_fmt"] if k == "y" else fmt if k == "grad_x" else F32
        assert_same(got[k], convert(fp32[k], t), t, f"{what}: {k}")
    return got


def model_y(c, got):
    """bn_kernels.h's float32 expression of y, with the statistics the kernel returned"""
    w = np.ones(c.shape[1], f32) if c.weight is None else c.weight
    b = np.zeros(c.shape[1], f32) if c.bias is None else c.bias
    with np.errstate(all="ignore"):
        scale = (w * got["save_invstd"]).astype(f32)
        shift = fma32(-got["save_mean"], scale, b)
        z = fma32(c.x, scale[None, :, None], shift[None, :, None])
        if c.rem is not None:
            z = (z + c.rem).astype(f32)
        return np.where(z <= 0, f32(0), z) if c.relu else z


def check_general(api, dev, case, fmt, site, relu, verbose=True):
    c = case.data(fmt, site, relu)
    r = c.ref
    what = f"{case.name} {FMT_NAME[fmt]} {site} relu={relu}"
    und = r.undecided()
    if case.tier == "general" and case.compare_grads:
        assert not und.any(), f"{what}: {int(und.sum())} elements left on the ReLU's kink"
    got = run_bn(api, dev, c, fmt, site, off=case.off)
    if verbose:
        print(what)
    # statistics and parameter gradients: bn_cases' bars, bn_cases' expressions
    bc.within("save_mean", got["save_mean"], r.mean, 2.0 ** -23 * r.mean_abs_x, verbose)
    bc.within("save_invstd", got["save_invstd"], r.invstd, 2.0 ** -22 * r.invstd, verbose)
    if c.running_mean is not None:
        m = r.m
        bc.within("running_mean", got["running_mean"], r.running_mean, 2.0 ** -22 * ((1 - m) * np.abs(r.old_mean) + m * np.abs(r.mean)), verbose)
        bc.within("running_var", got["running_var"], r.running_var, 2.0 ** -22 * ((1 - m) * np.abs(r.old_var) + m * np.abs(r.new_var)), verbose)
    else:
        assert got["running_mean"] is None
    # y: the fp32 expression of the returned statistics, rounded once; nothing else is allowed outside the undecided elements
    y_fmt = got["y_fmt"]
    want_y = convert(model_y(c, got), y_fmt).reshape(c.shape)
    keep = ~und
    assert_same(got["y"][keep], want_y[keep], y_fmt, f"{what}: y")
    if not case.compare_grads:
        return got
    gx64 = r.grad_x
    bc.within("grad_x", up(got["grad_x"], fmt).reshape(c.shape), gx64, r.bar_grad_x(case.mean_term) + half_ulp(np.abs(gx64) + r.bar_grad_x(case.mean_term), fmt), verbose)
    if c.rem is not None:
        assert_same(got["grad_rem"], r.g.astype(f32), F32, f"{what}: grad_rem is not g")
    if c.weight is not None:
        bar = 2.0 ** -22 * r.invstd * r.sum_abs_gxm
        if case.mean_term:
            bar = bar + 2.0 ** -22 * np.abs(r.mean) * r.invstd * np.abs(r.sum_g)
        bc.within("grad_weight", got["grad_weight"], r.grad_weight, bar, verbose)
        bc.within("grad_bias", got["grad_bias"], r.grad_bias, 2.0 ** -22 * r.sum_abs_g, verbose)
    return got


def check_special(api, dev, case, fmt, site, relu):
    """NaN, +-inf and -0 in x, rem and grad_y on exact-tier data, under the fp32 contract's rule: every output equals the fp32
    entry's on the up-cast input, NaN positions included.  A NaN or an infinity in x takes its channel's y, statistics, grad_x and
    grad_weight with it and NOT grad_bias (z <= 0 is false for a NaN z, so g = grad_y there: the ATen rule, DESIGN's remark);
    one in rem alone passes through at its element and leaves the statistics finite."""
    c = case.data(fmt, site, relu)
    got, fp32 = run_bn(api, dev, c, fmt, site, off=case.off), run_fp32(api, dev, c, 0)
    what = f"{case.name} {FMT_NAME[fmt]} {site} relu={relu}"
    for k in OUT_KEYS:
        if fp32.get(k) is None:
            continue
        t = got["y_fmt"] if k == "y" else fmt if k == "grad_x" else F32
        assert_same(got[k], convert(fp32[k], t), t, f"{what}: {k}")
    y_nan, gx_nan = is_nan(got["y"], got["y_fmt"]), is_nan(got["grad_x"], fmt)
    for ch in (1, 2):
        assert y_nan[:, ch].all() and gx_nan[:, ch].all(), what
        for k in ("save_invstd", "running_var", "grad_weight"):
            assert np.isnan(got[k][ch]), (what, k)
        for k in ("save_mean", "running_mean"):                 # (an infinity in x: the mean is that infinity)
            assert not np.isfinite(got[k][ch]), (what, k)
    assert np.isfinite(got["grad_bias"][1:]).all(), what
    assert np.isfinite(got["save_mean"][0]) and np.isfinite(got["save_invstd"][0]) and np.isfinite(got["running_var"][0]), what
    if case.special == "gy":
        assert np.isnan(got["grad_bias"][0]) and np.isnan(got["grad_weight"][0]) and gx_nan[:, 0].all(), what
    else:
        assert np.isfinite(got["grad_bias"][0]) and np.isfinite(got["grad_weight"][0]), what
        assert y_nan[:, 0].sum() == (1 if c.rem is not None else 0), what
        assert not gx_nan[:, 0].any(), what


def check_reproducible(api, dev, case, fmt):
    """two runs are bit-identical, and so is one whose workspace held zeros instead of NaN patterns"""
    site = case.sites[-1]
    c = case.data(fmt, site, True)
    a, b, z = run_bn(api, dev, c, fmt, site), run_bn(api, dev, c, fmt, site), run_bn(api, dev, c, fmt, site, ws_fill=0.0)
    for k in OUT_KEYS:
        if a.get(k) is not None:
            t = a["y_fmt"] if k == "y" else fmt if k == "grad_x" else F32
            assert_same(b[k], a[k], t, f"{case.name}: second run, {k}")
            assert_same(z[k], a[k], t, f"{case.name}: zeroed workspace, {k}")


def check_bn_bad_arguments(api, dev):
    st = dev.stream
    N, C, S = 2, 3, 16
    n = N * C * S
    x16, g16, y16, gx16 = (Buf(dev, BF16, data=convert(np.arange(n, dtype=f32) % 7, BF16)) for _ in range(4))
    r32, y32, gr32 = Buf(dev, F32, data=np.ones(n, f32)), Buf(dev, F32, n=n), Buf(dev, F32, n=n)
    sm, si, gw = Buf(dev, F32, n=C), Buf(dev, F32, n=C), Buf(dev, F32, n=C)
    rm = Buf(dev, F32, data=np.zeros(C, f32))
    ws = dev.empty((2 * api.query("ganet_bn_workspace", N, C, S),), np.float32)
    mb, eb = bc.fbits(0.1), bc.fbits(1e-5)
    fwd = lambda x, rem, rmean, rvar, w, y, s1, s2, N, C, S, xt, rt, yt: _rc(   # noqa: E731
        api, "ganet_bn_train_forward_mixed", x, rem, None, None, rmean, rvar, w, y, s1, s2, N, C, S, mb, eb, 1, xt, rt, yt, st)
    good = (x16.ptr, None, None, None, dev.ptr(ws), y16.ptr, sm.ptr, si.ptr, N, C, S, BF16, F32, BF16)
    assert fwd(*good) == 0
    for i in (0, 4, 5, 6, 7):
        bad = list(good); bad[i] = None
        assert fwd(*bad) == E_INVALID
    for i, v in ((8, 0), (9, 0), (10, -4), (11, 3), (12, 7), (13, -1)):
        bad = list(good); bad[i] = v
        assert fwd(*bad) == E_INVALID
    bad = list(good); bad[8:11] = [1, C, 1]
    assert fwd(*bad) == E_INVALID                                                                   # M = 1
    bad = list(good); bad[2] = rm.ptr
    assert fwd(*bad) == E_INVALID                                                                   # running_mean without running_var
    bad = list(good); bad[5] = x16.ptr
    assert fwd(*bad) == E_INVALID                                                                   # y is x
    bad = list(good); bad[1] = r32.ptr; bad[5] = r32.ptr
    assert fwd(*bad) == E_INVALID                                                                   # y is rem
    bad = list(good); bad[9] = 70000
    assert fwd(*bad) == E_UNSUPPORTED
    for xt, rem, rt, y, yt in ((F32, None, F32, y16.ptr, BF16),                                     # an fp32 x
                               (F32, None, F32, y32.ptr, F32),
                               (BF16, None, F32, y16.ptr, F16),                                     # two 16-bit formats
                               (BF16, r32.ptr, BF16, y16.ptr, BF16),                                # a 16-bit rem
                               (BF16, r32.ptr, F32, y32.ptr, F32)):                                 # a residual with an fp32 y
        bad = list(good); bad[11], bad[1], bad[12], bad[5], bad[13] = xt, rem, rt, y, yt
        assert fwd(*bad) == E_UNSUPPORTED, (xt, rt, yt)
    assert fwd(x16.ptr, None, None, None, dev.ptr(ws), y32.ptr, sm.ptr, si.ptr, N, C, S, BF16, F32, F32) == 0
    assert fwd(x16.ptr, r32.ptr, None, None, dev.ptr(ws), y16.ptr, sm.ptr, si.ptr, N, C, S, BF16, F32, BF16) == 0
    bwd = lambda x, rem, gy, s1, s2, w, gx, grem, gwp, N, C, S, xt, rt, gt: _rc(   # noqa: E731
        api, "ganet_bn_train_backward_mixed", x, rem, gy, None, None, s1, s2, w, gx, grem, gwp, None, N, C, S, 1, xt, rt, gt, st)
    good = (x16.ptr, r32.ptr, g16.ptr, sm.ptr, si.ptr, dev.ptr(ws), gx16.ptr, gr32.ptr, gw.ptr, N, C, S, BF16, F32, BF16)
    assert bwd(*good) == 0
    for i in (0, 2, 3, 4, 5):
        bad = list(good); bad[i] = None
        assert bwd(*bad) == E_INVALID
    for i, v in ((9, 0), (10, 0), (11, 0), (12, 3), (13, 3), (14, 3)):
        bad = list(good); bad[i] = v
        assert bwd(*bad) == E_INVALID
    for i, v in ((6, x16.ptr), (6, g16.ptr), (7, r32.ptr), (6, gr32.ptr)):                          # a gradient that is an input; one buffer twice
        bad = list(good); bad[i] = v
        assert bwd(*bad) == E_INVALID
    for xt, rt, gt in ((F32, F32, BF16), (BF16, BF16, BF16), (BF16, F32, F16), (BF16, F32, F32)):
        bad = list(good); bad[12:15] = [xt, rt, gt]
        assert bwd(*bad) == E_UNSUPPORTED, (xt, rt, gt)
    bad = list(good); bad[6:9] = [None, None, None]
    assert bwd(*bad) == 0                                                                           # nothing wanted: nothing done
    dev.sync()


# ---- cost volume backward ------------------------------------------------------------------------------------------------------

CV_BWD_CASES = list(CV_CASES) + [
    CvCase("W8-D13-beyond-W-odd", (1, 2, 2, 8), 13),                  # Dn > W, Dn % 8 != 0: a partial group behind a full one
    CvCase("W16-D8-one-group", (1, 1, 3, 16), 8),
    CvCase("W10-D3-scalar", (2, 1, 2, 10), 3),                        # W % 8 != 0
    CvCase("W13-D9-offset1-scalar", (1, 2, 3, 13), 9, off=1),
    # the second trip of the grid-stride loop: one vector group, and one scalar element, beyond ew_grid's cap
    CvCase("trip2-vector", (1, 1, EW_GRID_LANES // 64 + 1, 8 * 64), 1),
    CvCase("trip2-scalar", (1, 1, EW_GRID_LANES // 4 + 1, 4), 2),
]


def cv_bwd_data(case, fmt, seed=0):
    N, C, H, W = case.shape
    rng = np.random.RandomState(seed + fmt)
    n = N * 2 * C * case.Dn * H * W
    g = rng.standard_normal(n).astype(f32)
    g[3::17] *= 2.0 ** -9                  # a sum whose order shows: small terms beside large ones
    g = convert(g, fmt)
    g[5::29] = 0x8000
    if n < 10 ** 6:
        nan, inf = (0x7E01, 0x7C00) if fmt == F16 else (0x7FC1, 0x7F80)
        g[7::211] = nan
        g[11::223] = inf
        g[13::227] = inf | 0x8000
    return g


def check_cv_bwd(api, dev, case, fmt):
    N, C, H, W = case.shape
    g = cv_bwd_data(case, fmt)
    n = N * C * H * W
    dg = Buf(dev, fmt, data=g, off=case.off)
    dx, dy = Buf(dev, fmt, n=n, off=case.off), Buf(dev, fmt, n=n, off=case.off)
    api.call("ganet_cost_volume_backward_16", dg.ptr, dx.ptr, dy.ptr, N, C, case.Dn, H, W, fmt, dev.stream)
    fg, fx, fy = Buf(dev, F32, data=up(g, fmt)), Buf(dev, F32, n=n), Buf(dev, F32, n=n)
    api.call("ganet_cost_volume_backward", fg.ptr, fx.ptr, fy.ptr, N, C, case.Dn, H, W, dev.stream)
    dev.sync()
    assert np.array_equal(dg.host(), g), "the input was written"
    what = f"cost volume backward {case.name} {FMT_NAME[fmt]}"
    assert_same(dx.host(), convert(fx.host(), fmt), fmt, what + " grad_x")
    assert_same(dy.host(), convert(fy.host(), fmt), fmt, what + " grad_y")
    if n < 10 ** 5:
        # the definition, once, in float64 (libs/GANet/modules/GANet.py:114-134), to the fp32 sum's and the store's rounding
        g64 = up(g, fmt).astype(np.float64).reshape(N, 2 * C, case.Dn, H, W)
        wx, wy, ax = np.zeros((N, C, H, W)), np.zeros((N, C, H, W)), np.zeros((N, C, H, W))
        with np.errstate(invalid="ignore"):
            for i in range(min(case.Dn, W)):
                wx[..., i:] += g64[:, :C, i, :, i:]
                wy[..., :W - i] += g64[:, C:, i, :, i:]
                ax[..., i:] += np.abs(g64[:, :C, i, :, i:])
                ax[..., :W - i] += np.abs(g64[:, C:, i, :, i:])
        for got, want in ((dx.host(), wx), (dy.host(), wy)):
            got = up(got, fmt).astype(np.float64).reshape(want.shape)
            ok = np.isfinite(want) & np.isfinite(ax)
            got, want, ax = np.where(ok, got, 0.0), np.where(ok, want, 0.0), np.where(ok, ax, 0.0)
            assert (np.abs(got - want)[ok] <=(case.Dn * 2.0 ** -24 * ax + half_ulp(np.abs(want) + case.Dn * 2.0 ** -24 * ax, fmt))[ok]).all(), what


# ---- L1 normalisation backward -------------------------------------------------------------------------------------------------

def check_l1_bwd(api, dev, case, fmt):
    N, G, C, K, H, W = case.dims
    x = l1_data(case, fmt)
    n = N * C * K * H * W
    rng = np.random.RandomState(3 + fmt)
    gys = [rng.standard_normal(n).astype(f32) for _ in range(G)]
    given = G if case.unused_null else 4
    outs = {}
    for which in ("fp32", "mixed"):
        t = F32 if which == "fp32" else fmt
        dx = Buf(dev, t, data=up(x, fmt) if which == "fp32" else x)
        gs = [Buf(dev, F32, data=gys[min(g, G - 1)]) for g in range(given)]
        ptrs = [b.ptr for b in gs] + [None] * (4 - given)
        gx = Buf(dev, t, n=x.size)
        if which == "fp32":
            api.call("ganet_l1_normalize_backward", dx.ptr, *ptrs, gx.ptr, N, G, C, K, H, W, dev.stream)
        else:
            api.call("ganet_l1_normalize_backward_mixed", dx.ptr, *ptrs, gx.ptr, N, G, C, K, H, W, fmt, dev.stream)
        dev.sync()
        outs[which] = gx.host()
        assert np.array_equal(dx.host().view(np.uint8), (up(x, fmt) if which == "fp32" else x).ravel().view(np.uint8)), "x was written"
    what = f"l1 backward {case.name} {FMT_NAME[fmt]}"
    assert_same(outs["mixed"], convert(outs["fp32"], fmt), fmt, what)
    assert not is_nan(outs["mixed"], fmt).any()                              # every element written
    # the clamped norm: an all-zero column's gradient is gy / eps, beyond both formats' range or not, sign kept
    col = up(outs["mixed"], fmt).reshape(N, G, C, K, H * W)[0, 0, 0, :, 0]
    want = convert((gys[0].reshape(N, C, K, H * W)[0, 0, :, 0] / f32(1e-12)).astype(f32), fmt)
    assert np.array_equal(convert(col, fmt), want), what + ": the clamped column"


def check_misc_bad_arguments(api, dev):
    st = dev.stream
    a16, b16, c16 = (Buf(dev, BF16, data=np.zeros(256, np.uint16)) for _ in range(3))
    a32, b32 = Buf(dev, F32, data=np.zeros(256, f32)), Buf(dev, F32, data=np.zeros(256, f32))
    cv = lambda g, x, y, N, C, D, H, W, t: _rc(api, "ganet_cost_volume_backward_16", g, x, y, N, C, D, H, W, t, st)   # noqa: E731
    good = (a16.ptr, b16.ptr, c16.ptr, 1, 1, 2, 2, 8, BF16)
    assert cv(*good) == 0
    for i in (0, 1, 2):
        bad = list(good); bad[i] = None
        assert cv(*bad) == E_INVALID
    for i in (3, 4, 5, 6, 7):
        bad = list(good); bad[i] = 0
        assert cv(*bad) == E_INVALID
    assert cv(*good[:8], 3) == E_INVALID and cv(*good[:8], -1) == E_INVALID
    assert cv(*good[:8], F32) == E_UNSUPPORTED
    assert cv(a16.ptr, a16.ptr, c16.ptr, *good[3:]) == E_INVALID
    assert cv(a16.ptr, b16.ptr, a16.ptr, *good[3:]) == E_INVALID
    assert cv(a16.ptr, b16.ptr, b16.ptr, *good[3:]) == E_INVALID
    l1 = lambda x, g0, g1, gx, N, G, C, K, H, W, t: _rc(api, "ganet_l1_normalize_backward_mixed", x, g0, g1, None, None, gx, N, G, C, K, H, W, t, st)   # noqa: E731
    good = (a16.ptr, a32.ptr, b32.ptr, b16.ptr, 1, 2, 1, 5, 2, 2, BF16)
    assert l1(*good) == 0
    for i in (0, 2, 3):
        bad = list(good); bad[i] = None
        assert l1(*bad) == E_INVALID                                         # x, a gradient in use, grad_x
    for i in (4, 5, 6, 7, 8, 9):
        bad = list(good); bad[i] = 0
        assert l1(*bad) == E_INVALID
    assert l1(*good[:10], 7) == E_INVALID
    assert l1(*good[:10], F32) == E_UNSUPPORTED
    assert l1(a16.ptr, a32.ptr, b32.ptr, a16.ptr, *good[4:]) == E_INVALID    # grad_x is x
    bad = list(good); bad[5] = 5
    assert l1(*bad) == E_UNSUPPORTED                                         # more than four groups
    dev.sync()


L1_BWD_CASES = [L1Case("G4-K5-C2-7x9", 1, 4, 2, 5, 7, 9), L1Case("G4-K5-C2-8x8-N2", 2, 4, 2, 5, 8, 8), L1Case("G1-K75", 1, 1, 1, 75, 5, 7),
                L1Case("G1-K27-run-time", 1, 1, 1, 27, 5, 7), L1Case("G2-K7-run-time", 2, 2, 1, 7, 3, 5),
                L1Case("G3-K5-unused-given", 1, 3, 1, 5, 4, 6, unused_null=False)]
