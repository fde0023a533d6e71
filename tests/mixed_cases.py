"""TEST INFRASTRUCTURE: the case table of the mixed-precision kernels (ganet_amd/csrc/mixed_kernels.h: ganet_cast,
ganet_bn_apply_forward_mixed, ganet_cost_volume_forward_16, ganet_l1_normalize_forward_mixed), run on the emulator by
tests/test_sim_mixed.py and on the device by tests/test_gpu_mixed.py through one `dev` (parity_cases.NumpyDev / test_gpu_parity.TorchDev).

The yardstick has no tolerance in it.  For 16-bit inputs a16, ...
    op_mixed(a16, ...) == convert(op_fp32(upcast(a16), ...), out_type)         bit for bit, NaN positions equal
op_fp32 is the existing fp32 entry point run on the SAME build (held to its float64 statement by tests/bn_ref64.py and
tests/misc_ref64.py), upcast is exact, and convert is this file's own round-to-nearest-even: integer arithmetic for bf16,
numpy's astype(float16) for fp16.  16-bit values travel as uint16 patterns (int16 on the torch side)."""
import numpy as np

F32, F16, BF16 = 0, 1, 2
FMT_NAME = {F32: "f32", F16: "f16", BF16: "bf16"}
E_INVALID, E_UNSUPPORTED = -1, -2
POISON16 = 0x7FC1              # a NaN in both 16-bit formats: an element the kernel fails to write is noticed

# ---- the formats, stated in numpy ---------------------------------------------------------------------------------------------


def up(h, fmt):
    """uint16 patterns -> float32, exact"""
    h = np.ascontiguousarray(h, dtype=np.uint16)
    if fmt == BF16:
        return (h.astype(np.uint32) << 16).view(np.float32)
    return h.view(np.float16).astype(np.float32)


def convert(f, fmt):
    """float32 -> uint16 patterns, round to nearest even; a NaN becomes some NaN"""
    f = np.ascontiguousarray(f, dtype=np.float32)
    if fmt == F32:
        return f
    if fmt == F16:
        with np.errstate(over="ignore", invalid="ignore"):
            return f.astype(np.float16).view(np.uint16)
    u = f.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(f), np.uint16(0x7FC0), r)


def is_nan(a, fmt):
    return np.isnan(a) if fmt == F32 else np.isnan(up(a, fmt))


def assert_same(got, want, fmt, what=""):
    """equal bit for bit, with NaN positions equal"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = is_nan(got, fmt), is_nan(want, fmt)
    gb = got.view(np.uint32) if fmt == F32 else got.view(np.uint16)
    wb = want.view(np.uint32) if fmt == F32 else want.view(np.uint16)
    bad = (gn != wn) | (~wn & (gb != wb))
    if bad.any():
        i = np.flatnonzero(bad.ravel())[:5]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} differ; first at {i.tolist()}: got "
                             f"{[hex(int(v)) for v in gb.ravel()[i]]} want {[hex(int(v)) for v in wb.ravel()[i]]}")


def np_dtype(fmt):
    return np.float32 if fmt == F32 else np.uint16


# ---- buffers at a chosen element offset ---------------------------------------------------------------------------------------

class Buf:
    """a device buffer of `n` elements whose first element sits `off` elements behind an allocation's start"""

    def __init__(self, dev, fmt, n=None, data=None, off=0):
        self.dev, self.fmt, self.off = dev, fmt, off
        dt = np_dtype(fmt)
        if data is not None:
            data = np.ascontiguousarray(data, dtype=dt).ravel()
            n = data.size
            full = np.zeros(n + off, dtype=dt)
            full[off:] = data
            self.t = dev.to(full if fmt == F32 else full.view(np.int16))
        else:
            self.t = dev.empty((n + off,), np.float32 if fmt == F32 else np.uint16)
            if fmt != F32:
                (self.t.fill_ if hasattr(self.t, "fill_") else self.t.fill)(POISON16)
        self.n = n
        self.ptr = dev.ptr(self.t) + off * np.dtype(dt).itemsize

    def host(self, shape=None):
        a = np.asarray(self.dev.host(self.t))
        a = a if self.fmt == F32 else a.view(np.uint16)
        head, body = a[:self.off], a[self.off:]
        if self.off:           # nothing in front of the buffer was written
            assert is_nan(head, self.fmt).all() or (head == 0).all(), "an element in front of the buffer was written"
        return body.reshape(shape) if shape is not None else body


def count_args(n):
    return int(n >> 31), int(n & 0x7FFFFFFF)


# ---- conversions --------------------------------------------------------------------------------------------------------------

def _f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def tie_neighbours(fmt):
    """lower-neighbour patterns h (positive) whose midpoint with h + 1 goes into the table: near 1, near the largest finite
    value (its upper neighbour is the overflow threshold) and across the subnormal range, both parities everywhere"""
    one, top, first_normal = (0x3C00, 0x7BFF, 0x0400) if fmt == F16 else (0x3F80, 0x7F7F, 0x0080)
    hs = list(range(one - 4, one + 5)) + list(range(top - 4, top + 1)) + list(range(0, 6)) + \
        list(range(first_normal - 4, first_normal + 4))
    if fmt == F16:
        hs += list(range(0x01FE, 0x0203))
    return np.array(sorted(set(hs)), dtype=np.uint16)


def conversion_table(fmt, seed=0):
    """float32 inputs of the 32 -> 16 test: every tie of tie_neighbours with the values one fp32 ulp to either side, both signs;
    +-0; the largest finite value and the first that overflows; fp32 subnormals; +-inf; NaNs of both signs; 2^16 random patterns"""
    h = tie_neighbours(fmt)
    lo = up(h, fmt).astype(np.float64)
    top = h == (0x7BFF if fmt == F16 else 0x7F7F)
    hi = np.where(top, 2.0 ** (16 if fmt == F16 else 128), up(np.where(top, h, h + 1).astype(np.uint16), fmt).astype(np.float64))
    mid64 = (lo + hi) / 2
    mid = mid64.astype(np.float32)
    assert (mid.astype(np.float64) == mid64).all()              # every tie is an fp32 value
    below, above = np.nextafter(mid, np.float32(-np.inf)), np.nextafter(mid, np.float32(np.inf))
    pos = np.concatenate([mid, below, above, up(h, fmt)])
    largest = up(np.array([0x7BFF if fmt == F16 else 0x7F7F], dtype=np.uint16), fmt)
    special = _f32([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00000002, 0x007FFFFF, 0x807FFFFF, 0x00400000, 0x00800000,
                    0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FA00000])
    rng = np.random.RandomState(seed)
    rand = rng.randint(0, 2 ** 32, size=2 ** 16, dtype=np.uint64).astype(np.uint32).view(np.float32)
    return np.concatenate([pos, -pos, largest, -largest, special, rand]).astype(np.float32)


def run_cast(api, dev, src, src_fmt, dst_fmt, src_off=0, dst_off=0):
    src = np.ascontiguousarray(src, dtype=np_dtype(src_fmt)).ravel()
    s = Buf(dev, src_fmt, data=src, off=src_off)
    d = Buf(dev, dst_fmt, n=src.size, off=dst_off)
    api.call("ganet_cast", s.ptr, d.ptr, *count_args(src.size), src_fmt, dst_fmt, dev.stream)
    dev.sync()
    return d.host()


def cast_expected(src, src_fmt, dst_fmt):
    src = np.ascontiguousarray(src, dtype=np_dtype(src_fmt)).ravel()
    if src_fmt == dst_fmt:
        return src
    return convert(src if src_fmt == F32 else up(src, src_fmt), dst_fmt)


def check_cast(api, dev, src, src_fmt, dst_fmt, **kw):
    got = run_cast(api, dev, src, src_fmt, dst_fmt, **kw)
    want = cast_expected(src, src_fmt, dst_fmt)
    what = f"cast {FMT_NAME[src_fmt]}->{FMT_NAME[dst_fmt]} n={want.size} {kw}"
    if src_fmt == dst_fmt:                                     # a copy: the patterns themselves, NaNs included
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), what
    else:
        assert_same(got, want, dst_fmt, what)


CAST_SIZES = (1, 7, 8, 9, 2 ** 20 + 3)
CAST_OFFSETS = ((0, 0), (1, 0), (0, 1), (1, 1), (3, 5))


# ---- BatchNorm apply ----------------------------------------------------------------------------------------------------------

BN_BLOCK, BN_MAX_ROWS, BN_TARGET_BLOCKS, MX_V = 256, 64, 2048, 8         # bn_kernels.h / mixed_kernels.h (checked by the sim test)
# C = 32 gives the largest row count (BN_TARGET_BLOCKS / 32 = BN_MAX_ROWS = 64 blocks along the slice); one trip of the vector
# path covers MX_V * BN_MAX_ROWS * BN_BLOCK elements, and MX_V more start the second trip of lane 0 of block 0
BN_SECOND_TRIP_S = MX_V * BN_MAX_ROWS * BN_BLOCK + MX_V
REM_KINDS = ("none", "f32", "16")
Y_KINDS = ("16", "f32")


class BnCase:
    def __init__(self, name, shape, kind="general", off=0, inplace=False, combos=None):
        self.name, self.shape, self.kind, self.off, self.inplace = name, shape, kind, off, inplace
        self.combos = combos if combos is not None else [(r, y) for r in REM_KINDS for y in Y_KINDS]
        if inplace:
            self.combos = [(r, "16") for r in REM_KINDS]

    def __repr__(self):
        return self.name

    def data(self, fmt, seed=0):
        """x (patterns), rem (float32 values that are exact in fmt, so that one array serves both rem types), scale, shift"""
        N, C, S = self.shape
        rng = np.random.RandomState(seed + 17 * fmt)
        if self.kind == "ties":
            # x = +-integers with a full significand (p bits), z = m + 1/2, 2m + 1, m/2 + 1/4: a tie of the 16-bit format between
            # two neighbours, every parity of the lower one; the residual is a multiple of the format's spacing there
            p = 11 if fmt == F16 else 8
            m = rng.randint(2 ** (p - 1), 2 ** p, size=(N, C, S)).astype(np.float32) * rng.choice([-1.0, 1.0], size=(N, C, S))
            x = convert(m.astype(np.float32), fmt)
            assert (up(x, fmt) == m).all()
            scale = np.array([1.0, 2.0, 0.5] * C, dtype=np.float32)[:C]
            shift = np.array([0.5, 1.0, 0.25] * C, dtype=np.float32)[:C]
            rem = rng.randint(-4, 5, size=(N, C, S)).astype(np.float32) * scale[None, :, None] * 2
        else:
            x = convert(rng.standard_normal((N, C, S)).astype(np.float32) * 3, fmt)
            rem = up(convert(rng.standard_normal((N, C, S)).astype(np.float32), fmt), fmt)
            scale = (rng.standard_normal(C) + 0.5).astype(np.float32)
            shift = rng.standard_normal(C).astype(np.float32)
        if self.kind == "special":
            # NaN and +-inf in x and in rem; a channel with scale = 0 (0 * inf is a NaN there); -0
            nan, pinf, ninf, nzero = (0x7E01, 0x7C00, 0xFC00, 0x8000) if fmt == F16 else (0x7FC1, 0x7F80, 0xFF80, 0x8000)
            xf = x.reshape(-1)
            xf[0::7] = nan; xf[1::7] = pinf; xf[2::7] = ninf; xf[3::7] = nzero
            rf = rem.reshape(-1)
            rf[0::5] = np.nan; rf[1::5] = np.inf; rf[2::5] = -np.inf; rf[3::11] = -0.0
            scale[C - 1] = 0.0
            if C > 1:
                scale[0] = -1.0
        return x, rem.astype(np.float32), scale, shift


BN_CASES = [
    BnCase("S64-vector", (2, 3, 64)),
    BnCase("S68", (2, 3, 68)),
    BnCase("S66", (2, 3, 66)),
    BnCase("S61-odd", (1, 2, 61)),
    BnCase("S64-offset1", (2, 3, 64), off=1),
    BnCase("S64-inplace", (2, 3, 64), inplace=True),
    BnCase("S61-inplace", (1, 2, 61), inplace=True),
    BnCase("S64-ties", (2, 3, 64), kind="ties"),
    BnCase("S61-ties", (2, 3, 61), kind="ties"),
    BnCase("S64-special", (2, 3, 64), kind="special"),
    BnCase("S61-special", (1, 3, 61), kind="special"),
    BnCase("second-trip", (1, 32, BN_SECOND_TRIP_S), combos=[("16", "16"), ("f32", "f32")]),
]


def run_bn(api, dev, case, fmt, rem_kind, y_kind, relu, data=None, x_kind="16"):
    """(got, want): the mixed entry, and convert(ganet_bn_apply_forward(upcast ...)) on the same build.  x_kind "f32": the
    fp32-in, 16-bit-out form; its x has bits below the 16-bit format's last place on the general cases."""
    N, C, S = case.shape
    x, rem, scale, shift = data if data is not None else case.data(fmt)
    off = case.off
    y_fmt = fmt if y_kind == "16" else F32
    rem_fmt = fmt if rem_kind == "16" else F32
    x_fmt = fmt if x_kind == "16" else F32
    if x_kind == "f32":
        x = up(x, fmt) * np.float32(1.0 + 2.0 ** -11 + 2.0 ** -20 if case.kind == "general" else 1.0)
    dsc, dsh = Buf(dev, F32, data=scale), Buf(dev, F32, data=shift)
    # the yardstick
    x32 = Buf(dev, F32, data=up(x, fmt) if x_kind == "16" else x)
    r32 = Buf(dev, F32, data=rem) if rem_kind != "none" else None
    y32 = Buf(dev, F32, n=x.size)
    api.call("ganet_bn_apply_forward", x32.ptr, r32.ptr if r32 else None, dsc.ptr, dsh.ptr, y32.ptr, N, C, S, relu, dev.stream)
    # the kernel under test
    dx = Buf(dev, x_fmt, data=x, off=off)
    dr = None
    if rem_kind != "none":
        dr = Buf(dev, rem_fmt, data=convert(rem, fmt) if rem_kind == "16" else rem, off=off)
    dy = dx if case.inplace else Buf(dev, y_fmt, n=x.size, off=off)
    api.call("ganet_bn_apply_forward_mixed", dx.ptr, dr.ptr if dr else None, dsc.ptr, dsh.ptr, dy.ptr, N, C, S, relu,
             x_fmt, rem_fmt, y_fmt, dev.stream)
    dev.sync()
    want = convert(y32.host(), y_fmt)
    if not case.inplace:
        assert np.array_equal(dx.host().view(np.uint8), np.ascontiguousarray(x).ravel().view(np.uint8)), "the input was written"
    return dy.host(), want, y_fmt


def check_bn(api, dev, case, fmt):
    data = case.data(fmt)
    for rem_kind, y_kind in case.combos:
        for relu in (0, 1):
            got, want, y_fmt = run_bn(api, dev, case, fmt, rem_kind, y_kind, relu, data)
            assert_same(got, want, y_fmt, f"bn {case.name} {FMT_NAME[fmt]} rem={rem_kind} y={y_kind} relu={relu}")
    if case.inplace:
        return
    for rem_kind in ("none", "f32"):                                         # an fp32 x with a 16-bit y
        for relu in (0, 1):
            got, want, y_fmt = run_bn(api, dev, case, fmt, rem_kind, "16", relu, data, x_kind="f32")
            assert_same(got, want, y_fmt, f"bn {case.name} x=f32 -> {FMT_NAME[fmt]} rem={rem_kind} relu={relu}")


# ---- cost volume --------------------------------------------------------------------------------------------------------------

class CvCase:
    def __init__(self, name, shape, Dn, off=0):
        self.name, self.shape, self.Dn, self.off = name, shape, Dn, off

    def __repr__(self):
        return self.name


CV_CASES = [
    CvCase("W8-D3", (1, 1, 1, 8), 3),
    CvCase("W16-D5-vector", (2, 3, 2, 16), 5),
    CvCase("W13-D4-scalar", (1, 2, 3, 13), 4),
    CvCase("W8-D11-beyond-W", (1, 1, 2, 8), 11),
    CvCase("W16-D5-offset1", (2, 3, 2, 16), 5, off=1),
    CvCase("W24-D9", (1, 2, 2, 24), 9),
]


def cv_data(case, fmt, seed=0):
    rng = np.random.RandomState(seed + fmt)
    n = int(np.prod(case.shape))
    x = convert(rng.standard_normal(n).astype(np.float32), fmt)
    y = convert(rng.standard_normal(n).astype(np.float32), fmt)
    # -0 and NaN patterns with payloads: they must arrive unchanged -- a copy of bits
    for a, k in ((x, 0), (y, 1)):
        a[k::5] = 0x8000
        a[k + 2::7] = 0x7FC1 if fmt == BF16 else 0x7E01
        a[k + 3::11] = 0xFFFF
        a[k + 4::13] = 0x7F81 if fmt == BF16 else 0x7C01       # a signalling NaN
    return x, y


def cv_expected_bits(x, y, case):
    """the definition on patterns (libs/GANet/modules/GANet.py:114-134)"""
    N, C, H, W = case.shape
    x, y = x.reshape(case.shape), y.reshape(case.shape)
    cost = np.zeros((N, 2 * C, case.Dn, H, W), dtype=np.uint16)
    for i in range(min(case.Dn, W)):
        cost[:, :C, i, :, i:] = x[:, :, :, i:]
        cost[:, C:, i, :, i:] = y[:, :, :, :W - i]
    return cost.ravel()


def check_cv(api, dev, case, fmt):
    N, C, H, W = case.shape
    x, y = cv_data(case, fmt)
    n = N * 2 * C * case.Dn * H * W
    dx, dy = Buf(dev, fmt, data=x, off=case.off), Buf(dev, fmt, data=y, off=case.off)
    dc = Buf(dev, fmt, n=n, off=case.off)
    api.call("ganet_cost_volume_forward_16", dx.ptr, dy.ptr, dc.ptr, N, C, case.Dn, H, W, dev.stream)
    # the yardstick: the fp32 entry on the up-cast input, where the input has no NaN (an fp32 copy may quieten one)
    clean = lambda a: np.where(is_nan(a, fmt), np.uint16(0x3C00 if fmt == F16 else 0x3F80), a)       # noqa: E731
    fx, fy, fc = Buf(dev, F32, data=up(clean(x), fmt)), Buf(dev, F32, data=up(clean(y), fmt)), Buf(dev, F32, n=n)
    api.call("ganet_cost_volume_forward", fx.ptr, fy.ptr, fc.ptr, N, C, case.Dn, H, W, dev.stream)
    dev.sync()
    got = dc.host()
    want = cv_expected_bits(x, y, case)
    assert np.array_equal(got, want), f"cost volume {case.name} {FMT_NAME[fmt]}: {int((got != want).sum())} of {n} patterns differ"
    want32 = convert(fc.host(), fmt)
    ok = cv_expected_bits(~is_nan(x, fmt), ~is_nan(y, fmt), case).astype(bool) | (want == 0)
    assert np.array_equal(got[ok], want32[ok]), f"cost volume {case.name}: differs from convert(fp32 op)"


# ---- L1 normalisation ---------------------------------------------------------------------------------------------------------

class L1Case:
    def __init__(self, name, N, G, C, K, H, W, unused_null=True):
        self.name, self.dims, self.unused_null = name, (N, G, C, K, H, W), unused_null

    def __repr__(self):
        return self.name


L1_CASES = [
    L1Case("G4-K5-C2-7x9", 1, 4, 2, 5, 7, 9),
    L1Case("G4-K5-C2-8x8-N2", 2, 4, 2, 5, 8, 8),
    L1Case("G1-K75", 1, 1, 1, 75, 5, 7),
    L1Case("G1-K27", 1, 1, 1, 27, 5, 7),
    L1Case("G1-K7-no-template", 2, 1, 1, 7, 3, 5),
    L1Case("G3-K5-unused-given", 1, 3, 1, 5, 4, 6, unused_null=False),
]


def l1_data(case, fmt, seed=0):
    N, G, C, K, H, W = case.dims
    rng = np.random.RandomState(seed + fmt)
    x = rng.standard_normal((N, G, C, K, H * W)).astype(np.float32)          # signed
    x[0, 0, 0, :, 0] = 0.0                                                   # an all-zero column: the clamped norm
    x[0, 0, 0, :, 1] = 0.0
    x[0, 0, 0, :3, 1] = [1.0, 2.0 ** -24, -(2.0 ** -24)]                     # 1 + 2^-24 is a tie of fp32: the order of the sum shows
    x[0, 0, 0, :2, 2] = [-0.0, 3.0]
    return convert(x, fmt)


def check_l1(api, dev, case, fmt):
    N, G, C, K, H, W = case.dims
    x = l1_data(case, fmt)
    n = N * C * K * H * W
    outs = {}
    for which in ("fp32", "mixed"):
        dx = Buf(dev, F32, data=up(x, fmt)) if which == "fp32" else Buf(dev, fmt, data=x)
        ys = [Buf(dev, F32, n=n) for _ in range(G if case.unused_null else 4)]
        ptrs = [b.ptr for b in ys] + [None] * (4 - len(ys))
        if which == "fp32":
            api.call("ganet_l1_normalize_forward", dx.ptr, *ptrs, N, G, C, K, H, W, dev.stream)
        else:
            api.call("ganet_l1_normalize_forward_mixed", dx.ptr, *ptrs, N, G, C, K, H, W, fmt, dev.stream)
        dev.sync()
        outs[which] = [b.host() for b in ys]
    for g in range(G):
        assert_same(outs["mixed"][g], outs["fp32"][g], F32, f"l1 {case.name} {FMT_NAME[fmt]} output {g}")
        assert not np.isnan(outs["mixed"][g]).any()                          # every element written
    for g in range(G, len(outs["mixed"])):
        assert np.isnan(outs["mixed"][g]).all(), "an unused output was written"
    # the clamp and the definition, once, in numpy: y = x / max(sum |x|, 1e-12)
    xf = up(x, fmt).reshape(N, G, C, K, H * W)
    assert (outs["mixed"][0].reshape(N, C, K, H * W)[0, 0, :, 0] == 0).all()
    with np.errstate(invalid="ignore", divide="ignore"):
        ref = xf.astype(np.float64) / np.maximum(np.abs(xf.astype(np.float64)).sum(3, keepdims=True), 1e-12)
    for g in range(G):
        err = np.abs(outs["mixed"][g].reshape(N, C, K, H * W) - ref[:, g])
        assert err.max() <= (K + 2) * 2.0 ** -24, (case.name, g, err.max())       # K - 1 additions, one division


# ---- bad arguments ------------------------------------------------------------------------------------------------------------

def _rc(api, name, *args):
    from ganet_amd._native import GanetError
    try:
        api.call(name, *args)
    except GanetError as e:
        assert api.last_error(), name
        return e.code
    return 0


def check_bad_arguments(api, dev):
    st = dev.stream
    a16, b16, c16 = (Buf(dev, BF16, n=256) for _ in range(3))
    a32, b32 = Buf(dev, F32, n=256), Buf(dev, F32, n=256)
    sc, sh = Buf(dev, F32, data=np.ones(4, np.float32)), Buf(dev, F32, data=np.zeros(4, np.float32))
    # ganet_cast
    cast = lambda *a: _rc(api, "ganet_cast", *a)                             # noqa: E731
    assert cast(None, b16.ptr, 0, 8, F32, BF16, st) == E_INVALID
    assert cast(a32.ptr, None, 0, 8, F32, BF16, st) == E_INVALID
    assert cast(a32.ptr, b16.ptr, 0, 0, F32, BF16, st) == E_INVALID
    assert cast(a32.ptr, b16.ptr, 0, -1, F32, BF16, st) == E_INVALID
    assert cast(a32.ptr, b16.ptr, -1, 8, F32, BF16, st) == E_INVALID
    assert cast(a32.ptr, b16.ptr, 0, 8, 3, BF16, st) == E_INVALID
    assert cast(a32.ptr, b16.ptr, 0, 8, F32, -1, st) == E_INVALID
    assert cast(a32.ptr, a32.ptr, 0, 8, F32, BF16, st) == E_INVALID
    # ganet_bn_apply_forward_mixed
    bn = lambda x, r, s, h, y, N, C, S, xt, rt, yt: _rc(api, "ganet_bn_apply_forward_mixed", x, r, s, h, y, N, C, S, 1, xt, rt, yt, st)   # noqa: E731
    good = (a16.ptr, None, sc.ptr, sh.ptr, b16.ptr, 2, 4, 16, BF16, F32, BF16)
    assert bn(*good) == 0
    for i in (0, 2, 3, 4):
        bad = list(good)
        bad[i] = None
        assert bn(*bad) == E_INVALID
    for i in (5, 6, 7):
        bad = list(good)
        bad[i] = 0
        assert bn(*bad) == E_INVALID
    for i in (8, 9, 10):
        bad = list(good)
        bad[i] = 3
        assert bn(*bad) == E_INVALID
    assert bn(a16.ptr, None, sc.ptr, sh.ptr, a16.ptr, 2, 4, 16, BF16, F32, BF16) == 0              # in place, one width
    assert bn(a16.ptr, None, sc.ptr, sh.ptr, a16.ptr, 2, 4, 16, BF16, F32, F32) == E_INVALID       # aliasing across widths
    assert bn(a16.ptr, b16.ptr, sc.ptr, sh.ptr, b16.ptr, 2, 4, 16, BF16, BF16, BF16) == E_INVALID  # y is rem
    assert bn(a32.ptr, None, sc.ptr, sh.ptr, b16.ptr, 2, 4, 16, F32, F32, BF16) == 0               # an fp32 x with a 16-bit y
    assert bn(a32.ptr, None, sc.ptr, sh.ptr, b32.ptr, 2, 4, 16, F32, F32, F32) == E_UNSUPPORTED    # all fp32: the fp32 entry's
    assert bn(a32.ptr, c16.ptr, sc.ptr, sh.ptr, b16.ptr, 2, 4, 16, F32, BF16, BF16) == E_UNSUPPORTED   # an fp32 x with a 16-bit rem
    assert bn(a32.ptr, None, sc.ptr, sh.ptr, a32.ptr, 2, 4, 16, F32, F32, BF16) == E_INVALID       # aliasing across widths
    assert bn(a16.ptr, None, sc.ptr, sh.ptr, b16.ptr, 2, 4, 16, BF16, F32, F16) == E_UNSUPPORTED   # two 16-bit formats
    assert bn(a16.ptr, c16.ptr, sc.ptr, sh.ptr, b16.ptr, 2, 4, 16, F16, BF16, F16) == E_UNSUPPORTED
    # ganet_cost_volume_forward_16
    cv = lambda x, y, c, N, C, D, H, W: _rc(api, "ganet_cost_volume_forward_16", x, y, c, N, C, D, H, W, st)   # noqa: E731
    good = (a16.ptr, b16.ptr, c16.ptr, 1, 1, 2, 2, 8)
    assert cv(*good) == 0
    for i in (0, 1, 2):
        bad = list(good)
        bad[i] = None
        assert cv(*bad) == E_INVALID
    for i in (3, 4, 5, 6, 7):
        bad = list(good)
        bad[i] = 0
        assert cv(*bad) == E_INVALID
    assert cv(a16.ptr, b16.ptr, a16.ptr, 1, 1, 2, 2, 8) == E_INVALID
    # ganet_l1_normalize_forward_mixed
    l1 = lambda x, y0, y1, N, G, C, K, H, W, t: _rc(api, "ganet_l1_normalize_forward_mixed", x, y0, y1, None, None, N, G, C, K, H, W, t, st)   # noqa: E731
    good = (a16.ptr, a32.ptr, b32.ptr, 1, 2, 1, 5, 2, 2, BF16)
    assert l1(*good) == 0
    assert l1(None, *good[1:]) == E_INVALID
    assert l1(a16.ptr, a32.ptr, None, *good[3:]) == E_INVALID                                      # an output in use is NULL
    for i in (3, 4, 5, 6, 7, 8):
        bad = list(good)
        bad[i] = 0
        assert l1(*bad) == E_INVALID
    assert l1(*good[:9], 7) == E_INVALID
    assert l1(*good[:9], F32) == E_UNSUPPORTED
    assert l1(a16.ptr, a32.ptr, b32.ptr, 1, 5, 1, 5, 2, 2, BF16) == E_UNSUPPORTED                  # more than four groups
    dev.sync()
