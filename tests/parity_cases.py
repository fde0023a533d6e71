"""Parity checks shared by the CPU-emulator tests (numpy buffers, tests/hipsim) and the
GPU tests (torch device buffers): every check drives the C ABI of include/ganet_hip.h
and compares with the oracle / golden fixtures.  `dev` abstracts buffer handling."""
import ctypes
import mmap

import os

import numpy as np

TOL = 1e-4   # north_star: fp32 max-abs <= 1e-4 for SGA/LGA forward + backward


def l1norm(g, axis):
    return (g / np.abs(g).sum(axis, keepdims=True)).astype(np.float32)


def sga_inputs(shape, seed):
    rng = np.random.default_rng(seed)
    N, C, D, H, W = shape
    x = rng.standard_normal(shape).astype(np.float32)
    gs = [l1norm(rng.standard_normal((N, C, 5, H, W)), 2) for _ in range(4)]
    go = rng.standard_normal(shape).astype(np.float32)
    return x, gs, go


# ---- value families: inputs that make ties frequent and (select, lga exact) every partial sum exactly representable ----------
_SELECT_P = (0.35, 0.2, 0.1, 0.1, 0.25)
_DYADIC_PATTERNS = np.array([[1, 0, 0, 0, 0], [.5, .5, 0, 0, 0], [.5, 0, 0, 0, .5], [.5, .25, .25, 0, 0], [.25, .25, .25, 0, .25],
                             [0, 0, 0, 0, 1], [0, 1, 0, 0, 0], [.5, 0, .25, .25, 0], [0, 0, 0, 0, 0]], np.float32)


def sga_inputs_select(shape, seed):
    """*selection* family: x, go integers in [-2, 2]; per (n, c, h, w) exactly one of the five guidance taps is 1.0.  Every
    volume entry is then one of five values whatever the scanline length, every gradient an integer: ties everywhere, and
    results that do not depend on summation order or contraction (equality with the oracle, gradients included)."""
    rng = np.random.default_rng(seed)
    N, C, D, H, W = shape
    x = rng.integers(-2, 3, shape).astype(np.float32)
    gs = []
    for _ in range(4):
        tap = rng.choice(5, size=(N, C, H, W), p=_SELECT_P)
        g = np.zeros((N, C, 5, H, W), np.float32)
        np.put_along_axis(g, tap[:, :, None], 1.0, axis=2)
        gs.append(g)
    go = rng.integers(-2, 3, shape).astype(np.float32)
    return x, gs, go


def sga_inputs_dyadic(shape, seed):
    """per pixel one of nine dyadic tap patterns (|w|_1 <= 1, an all-zero one among them), each entry negated with probability
    1/4; integer x, go.  Bounded, signed weights; ties that decay along the scanline.  Gradients are not exact here."""
    rng = np.random.default_rng(seed)
    N, C, D, H, W = shape
    x = rng.integers(-2, 3, shape).astype(np.float32)
    gs = []
    for _ in range(4):
        g = _DYADIC_PATTERNS[rng.integers(0, len(_DYADIC_PATTERNS), (N, C, H, W))]            # N C H W 5
        sign = rng.choice(np.array([1, 1, 1, -1], np.float32), g.shape)
        gs.append(np.ascontiguousarray(np.moveaxis(g * sign, -1, 2)))
    go = rng.integers(-2, 3, shape).astype(np.float32)
    return x, gs, go


def sga_inputs_sparse(shape, seed):
    """model-like: x = relu(randn) with the cost volume's wedge zeroed (x[..., d, :, w] = 0 for w < d); guidance = randn with
    30 % of the taps exactly 0, L1-normalised (0 where the norm is 0), 10 % of the pixels zeroed entirely; go = randn."""
    rng = np.random.default_rng(seed)
    N, C, D, H, W = shape
    x = np.maximum(rng.standard_normal(shape), 0).astype(np.float32)
    wedge = np.arange(W)[None, :] < np.arange(D)[:, None]                                      # D W
    x[np.broadcast_to(wedge[None, None, :, None, :], shape)] = 0
    gs = []
    for _ in range(4):
        g = rng.standard_normal((N, C, 5, H, W)) * (rng.random((N, C, 5, H, W)) > 0.3)
        s = np.abs(g).sum(2, keepdims=True)
        g = np.where(s > 0, g / np.maximum(s, 1e-12), 0)
        g = g * (rng.random((N, C, 1, H, W)) > 0.1)
        gs.append(g.astype(np.float32))
    go = rng.standard_normal(shape).astype(np.float32)
    return x, gs, go


SGA_FAMILIES = {"select": sga_inputs_select, "dyadic": sga_inputs_dyadic, "sparse": sga_inputs_sparse}
# floors of (elements with a direction tie, pixels with an arg-max tie in each direction, pixels whose first arg-max is > 0),
# for D >= 6 and at least 35 pixels per slice; set well under what the families give (select 0.55-0.74 / 0.50-1.0 / 0.41-0.65,
# dyadic 0.13-0.21 / 0.46-0.87, sparse 0.07-0.21 / 0.18-0.41)
SGA_TIE_FLOORS = {"select": (0.30, 0.30, 0.30), "dyadic": (0.05, 0.30, None), "sparse": (0.03, 0.10, None)}


def sga_tie_stats(A):
    """A: the four directional volumes [N,C,D,H,W] -> (fraction of elements where two or more directions share the maximum,
    [per direction: fraction of pixels whose maximum over depth is attained more than once],
    fraction of all (direction, pixel) pairs whose first arg-max is not disparity 0)"""
    S = np.stack(A)
    dir_ties = float(((S == S.max(0)).sum(0) > 1).mean())
    am = [float(((a == a.max(2, keepdims=True)).sum(2) > 1).mean()) for a in A]
    nz = float(np.mean([(np.argmax(a, 2) > 0).mean() for a in A]))
    return dir_ties, am, nz


def assert_sga_ties(family, A):
    """the family's floors hold for these volumes (so that a test on them cannot pass vacuously)"""
    dir_ties, am, nz = sga_tie_stats(A)
    f_dir, f_am, f_nz = SGA_TIE_FLOORS[family]
    assert dir_ties >= f_dir, (family, "direction ties", dir_ties)
    assert min(am) >= f_am, (family, "arg-max ties", am)
    assert f_nz is None or nz >= f_nz, (family, "first arg-max > 0", nz)
    return dir_ties, am, nz


def lga_inputs_exact(shape, r, seed):
    """x, gy: integers in [-4, 4]; filters: integers in [-4, 4] / 8 with 40 % exactly 0, not normalised: every product and
    partial sum of one to three passes is a multiple of 1/8, 1/64, 1/512 below 2^24 of them (lga_ref64.assert_lga_exact)."""
    rng = np.random.default_rng(seed)
    fs = list(shape)
    fs[-3] = 3 * (2 * r + 1) ** 2
    x = rng.integers(-4, 5, shape).astype(np.float32)
    f = (rng.integers(-4, 5, fs) * (rng.random(fs) > 0.4)).astype(np.float32) / 8
    gy = rng.integers(-4, 5, shape).astype(np.float32)
    return x, f, gy


# ---- non-finite inputs for the fused BatchNorm + ReLU epilogue of ganet_sga_forward_infer ------------------------------------------
NONFINITE_SHAPES = [(2, 3, 9, 4, 8), (2, 3, 8, 3, 5), (2, 3, 5, 3, 5)]     # row kernel's epilogue | merge, 16-byte form | merge, scalar
NONFINITE_SCALE = np.array([-2.0, 0.5, -0.5], np.float32)                  # powers of two: scale * v is exact, so fmaf(v, sc, sh)
NONFINITE_SHIFT = np.array([0.75, -1.25, 0.5], np.float32)                 # and fp32 multiply-then-add round once, alike


def sga_inputs_nonfinite(shape, seed):
    """x = randn with ONE special element per (n, c) slice -- NaN, +Inf or -Inf, kind (n + c) % 3 -- and strictly positive
    normalised guidance taps, so that an infinity spreads as that infinity (no 0 * Inf, no Inf - Inf inside a slice).  With
    NONFINITE_SCALE every kind meets a scale of either sign in some slice: -Inf under a negative scale becomes +Inf.
    -> (x, gs, raw guidance [N, 20 C, H, W] that L1-normalises to gs' ratios, for the module form)"""
    rng = np.random.default_rng(seed)
    N, C, D, H, W = shape
    assert C == 3 and N >= 2
    x = rng.standard_normal(shape).astype(np.float32)
    for n in range(N):
        for c in range(C):
            x[n, c, D // 2, H // 2, W // 2] = (np.nan, np.inf, -np.inf)[(n + c) % 3]
    raw = (np.abs(rng.standard_normal((N, 4, C, 5, H, W))) + 0.05).astype(np.float32)
    gs = [l1norm(raw[:, k], 2) for k in range(4)]
    return x, gs, np.ascontiguousarray(raw.reshape(N, 20 * C, H, W))


def bn_relu_keep_nan(v, scale, shift):
    """relu(scale[c] * v + shift[c]) on [N,C,D,H,W] in fp32 with the ReLU of ATen: a NaN passes through"""
    C = v.shape[1]
    with np.errstate(invalid="ignore"):
        pre = v.astype(np.float32) * scale.astype(np.float32).reshape(1, C, 1, 1, 1) + shift.astype(np.float32).reshape(1, C, 1, 1, 1)
        return np.where(pre <= 0, np.float32(0), pre).astype(np.float32)


def assert_same_with_nan(got, want, what=""):
    """the NaN positions and every other value (infinities included) are equal"""
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "NaN positions", int(np.isnan(got).sum()), int(np.isnan(want).sum()))
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok], want[ok]), (what, int((got[ok] != want[ok]).sum()), "values differ")


def assert_nonfinite_reach_the_epilogue(plain, want):
    """the plain maximum holds each kind, and the epilogue's yardstick turns a -Inf into +Inf somewhere (negative scale)"""
    assert np.isnan(plain).any() and np.isposinf(plain).any() and np.isneginf(plain).any()
    assert (np.isneginf(plain) & np.isposinf(want)).any() and (np.isposinf(plain) & (want == 0)).any()
    assert (np.isneginf(plain) & (want == 0)).any() and (np.isposinf(plain) & np.isposinf(want)).any()


def oracle_sga_want(oracle, x, gs, go):
    """everything check_sga_forward_backward / check_sga_compat compare with, from the oracle (A0..A3 included)"""
    out, tmp, mask = oracle.sga_forward(x, *gs)
    grads = oracle.sga_backward(x, *gs, tmp, mask, go)
    want = {"out": out, "mask": mask.astype(np.uint8), "tmp": tmp, "gx": grads[0]}
    for d in range(4):
        want[f"gw{d}"] = grads[1 + d]
        want[f"A{d}"] = oracle.sga_scan(x, gs[d], d)
    return want


def assert_select_exact(x, gs, go):
    """Exactness condition of the *select* family, whatever the routing of the gradient (mask, arg-max) and the order of the
    sums.  With one tap of 1.0 per pixel every forward entry is a copy of an x entry (|A| <= max|x|), and the adjoint scan
    hands each element's gradient to exactly one predecessor: gradient mass is merged (tap 4 collects a whole depth column
    in its arg-max) but never duplicated.  So the absolute partial sums of any adjoint entry stay within
    M = scanline length * max over pixels of sum_d |go|; those of gX within 4 M (four directions), those of a guidance
    gradient (sum over d of adjoint * x or * A) within max|x| * M.  All are integers: exact in fp32 below 2^24."""
    assert all(np.array_equal(g, np.round(g)) and np.array_equal(g.sum(2), np.ones_like(g[:, :, 0])) and g.min() == 0 for g in gs)
    assert np.array_equal(x, np.round(x)) and np.array_equal(go, np.round(go))
    M = max(x.shape[3], x.shape[4]) * float(np.abs(go).sum(2).max())
    bound = 4 * M * max(1.0, float(np.abs(x).max()))
    assert bound < 2 ** 24, bound
    return bound


_PAGE = mmap.PAGESIZE
_libc = ctypes.CDLL(None, use_errno=True)
_libc.mprotect.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]


def guarded_empty(shape, dtype=np.float32, guard="end"):
    """An array whose last byte is followed by an inaccessible page (and whose mapping is preceded by one): a kernel that
    reads or writes past the end of a tensor -- harmless on the GPU as long as the neighbouring memory happens to be mapped,
    a memory access fault once it is not (the 528x960 volumes of round 2) -- dies right here on the emulator.
    guard="start": the array BEGINS right behind the leading inaccessible page instead (accesses in front of a tensor)."""
    dtype = np.dtype(dtype)
    count = int(np.prod(shape, dtype=np.int64))
    nbytes = count * dtype.itemsize
    body = -(-max(nbytes, 1) // _PAGE) * _PAGE
    mm = mmap.mmap(-1, body + 2 * _PAGE)
    base = ctypes.addressof(ctypes.c_char.from_buffer(mm))
    for off in (0, _PAGE + body):
        if _libc.mprotect(base + off, _PAGE, 0) != 0:
            raise OSError(ctypes.get_errno(), "mprotect")
    start = _PAGE if guard == "start" else (_PAGE + body - nbytes) & ~15     # 16-byte aligned like any device allocation
    return np.frombuffer(mm, dtype, count, start).reshape(shape)


class NumpyDev:
    """Host buffers for the emulator build (every buffer ends at a guard page, see guarded_empty)."""
    stream = None

    def __init__(self, guard="end"):
        self.guard = guard

    def to(self, a):
        a = np.asarray(a)
        g = guarded_empty(a.shape, a.dtype, self.guard)
        g[...] = a
        return g

    def empty(self, shape, dtype=np.float32):
        a = guarded_empty(shape, dtype, self.guard)
        a.fill(np.nan if dtype == np.float32 else 113)     # poison: unwritten elements get noticed
        return a

    def zeros(self, shape, dtype=np.float32):
        a = guarded_empty(shape, dtype, self.guard)
        a.fill(0)
        return a

    def ptr(self, a):
        return a.ctypes.data

    def host(self, a):
        return a

    def sync(self):
        pass


class _PtrAt:
    """a device address inside a buffer that is kept alive alongside it"""
    def __init__(self, addr, keep):
        self.addr, self.keep = addr, keep


class _OffsetDev:
    """a device whose ptr() also understands _PtrAt"""
    def __init__(self, dev):
        self._dev = dev

    def __getattr__(self, name):
        return getattr(self._dev, name)

    def ptr(self, a):
        return a.addr if isinstance(a, _PtrAt) else self._dev.ptr(a)


def check_sga_scan(api, dev, oracle, x, g, direction):
    N, C, D, H, W = x.shape
    dx, dg = dev.to(x), dev.to(g)
    A = dev.empty(x.shape)
    api.call("ganet_sga_scan_forward", dev.ptr(dx), dev.ptr(dg), dev.ptr(A), N, C, D, H, W, direction, dev.stream)
    dev.sync()
    want = oracle.sga_scan(x, g, direction)
    got = dev.host(A)
    assert np.array_equal(got, want), f"dir {direction}: {int((got != want).sum())} of {got.size} differ, max {np.abs(got - want).max()}"


def untile_ws(t):
    """[N,C,D,H,W] array holding a vertical direction's volume in SgaFunction's private tiled layout
    ([slice][W/16][H/4][D][4][16], include/ganet_hip.h: ganet_sga_workspace_layout) -> the API layout."""
    N, C, D, H, W = t.shape
    v = t.reshape(N * C, W // 16, H // 4, D, 4, 16)          # (s, cb, rb, d, rj, cw)
    return np.ascontiguousarray(v.transpose(0, 3, 2, 4, 1, 5)).reshape(N, C, D, H, W)


def run_sga_forward(api, dev, x, gs):
    N, C, D, H, W = x.shape
    dx = dev.to(x)
    dg = [dev.to(g) for g in gs]
    A = dev.empty((4,) + x.shape)
    out = dev.empty(x.shape)
    mask = dev.empty(x.shape, np.uint8)
    kp = dev.empty((4, N, C, H, W), np.uint16)
    api.call("ganet_sga_forward", dev.ptr(dx), *[dev.ptr(g) for g in dg], dev.ptr(A), dev.ptr(out), dev.ptr(mask),
             dev.ptr(kp), N, C, D, H, W, dev.stream)
    dev.sync()
    return dx, dg, A, out, mask, kp


def check_sga_forward_backward(api, dev, x, gs, go, want, per_dir=True, results=None):
    """want: dict(out, mask(uint8), gx, gw0..gw3, optional A0..A3) from the oracle/golden.
    per_dir=False skips the cross-check of the per-direction entry point (large volumes)."""
    N, C, D, H, W = x.shape
    dx, dg, A, out, mask, kp = run_sga_forward(api, dev, x, gs)
    hA = dev.host(A)
    for d in range(4):
        if f"A{d}" in want:
            assert np.array_equal(hA[d], want[f"A{d}"]), f"A{d}"
    assert np.array_equal(dev.host(out), want["out"]), "out"
    assert np.array_equal(dev.host(mask), want["mask"]), "direction mask must be bit-exact"
    # arg-max indices: first maximum over d of each directional volume (MaxDepth semantics)
    assert np.array_equal(dev.host(kp).astype(np.int64), np.argmax(hA, axis=3)), "arg-max must be bit-exact"
    dgo = dev.to(go)
    gx = dev.empty(x.shape)
    gw = [dev.empty(gs[0].shape) for _ in range(4)]
    G = dev.empty((4,) + x.shape)
    api.call("ganet_sga_backward", dev.ptr(dx), *[dev.ptr(g) for g in dg], dev.ptr(A), dev.ptr(mask), dev.ptr(kp),
             dev.ptr(dgo), dev.ptr(G), dev.ptr(gx), *[dev.ptr(g) for g in gw], N, C, D, H, W, dev.stream)
    dev.sync()
    # the per-direction entry point must agree with the fused one
    gx1 = dev.empty(x.shape) if per_dir else gx
    G1 = dev.empty(x.shape) if per_dir else None
    for d in range(4 if per_dir else 0):
        gw1 = dev.empty(gs[0].shape)
        api.call("ganet_sga_backward_dir", dev.ptr(dx), dev.ptr(dg[d]), dev.ptr(A) + 4 * d * x.size,
                 dev.ptr(mask), dev.ptr(kp) + 2 * d * (N * C * H * W), dev.ptr(dgo), dev.ptr(G1), dev.ptr(gx1),
                 dev.ptr(gw1), N, C, D, H, W, d, 1 if d else 0, dev.stream)
        dev.sync()
        assert np.abs(dev.host(gw1) - dev.host(gw[d])).max() <= 1e-6
    assert np.abs(dev.host(gx1) - dev.host(gx)).max() <= 1e-5
    if per_dir:
        # ABI 8: the composite entries are their steps -- 4 x scan + ganet_sga_merge, 4 x adjoint scan +
        # ganet_sga_backward_point -- bit for bit (bench.py times the steps in place)
        A2, out2 = dev.empty((4,) + x.shape), dev.empty(x.shape)
        mask2, kp2 = dev.empty(x.shape, np.uint8), dev.empty((4, N, C, H, W), np.uint16)
        for d in range(4):
            api.call("ganet_sga_scan_forward_ws", dev.ptr(dx), dev.ptr(dg[d]), dev.ptr(A2), N, C, D, H, W, d, dev.stream)
        api.call("ganet_sga_merge", dev.ptr(A2), dev.ptr(out2), dev.ptr(mask2), dev.ptr(kp2), N, C, D, H, W, dev.stream)
        dev.sync()
        assert np.array_equal(dev.host(out2), dev.host(out)) and np.array_equal(dev.host(mask2), dev.host(mask))
        assert np.array_equal(dev.host(kp2), dev.host(kp))
        G2, gx2 = dev.empty((4,) + x.shape), dev.empty(x.shape)
        gw2 = [dev.empty(gs[0].shape) for _ in range(4)]
        for d in range(4):
            api.call("ganet_sga_backward_scan_ws", dev.ptr(dg[d]), dev.ptr(mask), dev.ptr(kp), dev.ptr(dgo),
                     dev.ptr(G2), N, C, D, H, W, d, dev.stream)
        api.call("ganet_sga_backward_point", dev.ptr(dx), *[dev.ptr(g) for g in dg], dev.ptr(A), dev.ptr(G2), dev.ptr(gx2),
                 *[dev.ptr(g) for g in gw2], N, C, D, H, W, dev.stream)
        dev.sync()
        # the adjoint volumes themselves: the vertical directions' may be tiled in the private workspace
        hG, hG2 = dev.host(G), dev.host(G2)
        assert np.array_equal(hG, hG2)
        if api.query("ganet_sga_workspace_layout", N, C, D, H, W):
            G3 = dev.empty(x.shape)
            for d in range(2):
                api.call("ganet_sga_backward_scan", dev.ptr(dg[d]), dev.ptr(mask), dev.ptr(kp) + 2 * d * (N * C * H * W), dev.ptr(dgo),
                         dev.ptr(G3), N, C, D, H, W, d, dev.stream)
                dev.sync()
                assert np.array_equal(untile_ws(hG[d]), dev.host(G3)), f"tiled adjoint volume of direction {d}"
        assert np.array_equal(dev.host(gx2), dev.host(gx))
        for d in range(4):
            assert np.array_equal(dev.host(gw2[d]), dev.host(gw[d]))
    err = {"gx": float(np.abs(dev.host(gx) - want["gx"]).max())}
    for d in range(4):
        err[f"gw{d}"] = float(np.abs(dev.host(gw[d]) - want[f"gw{d}"]).max())
    assert max(err.values()) <= TOL, err
    if results is not None:                  # (`results`: dict that receives the gradients)
        results["gx"] = dev.host(gx)
        for d in range(4):
            results[f"gw{d}"] = dev.host(gw[d])
    return err


def run_sga_backward_only(api, dev, x, gs, go, go_offset=0):
    """forward + backward through the composite entries, gradients as host arrays (no oracle: the caller compares runs);
    go_offset: the incoming gradient starts that many floats into its buffer (contiguous, 4-byte aligned)"""
    N, C, D, H, W = x.shape
    dx, dg, A, out, mask, kp = run_sga_forward(api, dev, x, gs)
    if go_offset:
        dgo_buf = dev.to(np.concatenate([np.zeros(go_offset, np.float32), go.ravel()]))
        dgo = _PtrAt(dev.ptr(dgo_buf) + 4 * go_offset, dgo_buf)
        dev = _OffsetDev(dev)
    else:
        dgo = dev.to(go)
    gx = dev.empty(x.shape)
    gw = [dev.empty(gs[0].shape) for _ in range(4)]
    G = dev.empty((4,) + x.shape)
    api.call("ganet_sga_backward", dev.ptr(dx), *[dev.ptr(g) for g in dg], dev.ptr(A), dev.ptr(mask), dev.ptr(kp),
             dev.ptr(dgo), dev.ptr(G), dev.ptr(gx), *[dev.ptr(g) for g in gw], N, C, D, H, W, dev.stream)
    dev.sync()
    res = {"gx": dev.host(gx)}
    for d in range(4):
        res[f"gw{d}"] = dev.host(gw[d])
    return res


def check_sga_compat(api, dev, x, gs, go, want):
    """Reference buffer contract (sga_cuda_forward / sga_cuda_backward)."""
    N, C, D, H, W = x.shape
    dx = dev.to(x)
    dg = [dev.to(g) for g in gs]
    tmp, out, mask = dev.zeros(x.shape), dev.zeros(x.shape), dev.zeros(x.shape)
    api.call("ganet_sga_forward_compat", dev.ptr(dx), *[dev.ptr(g) for g in dg], dev.ptr(tmp), dev.ptr(out),
             dev.ptr(mask), N, C, D, H, W, dev.stream)
    dev.sync()
    assert np.array_equal(dev.host(out), want["out"])
    assert np.array_equal(dev.host(mask).astype(np.uint8), want["mask"])
    assert np.array_equal(dev.host(tmp), want["tmp"]), "temp_out must hold A_left"
    dgo = dev.to(go)
    gx = dev.zeros(x.shape)
    gw = [dev.zeros(gs[0].shape) for _ in range(4)]
    tgrad = dev.zeros(x.shape)
    idx = dev.zeros((N, C, H, W))
    api.call("ganet_sga_backward_compat", dev.ptr(dx), *[dev.ptr(g) for g in dg], dev.ptr(tmp), dev.ptr(mask),
             dev.ptr(idx), dev.ptr(dgo), dev.ptr(tgrad), dev.ptr(gx), *[dev.ptr(g) for g in gw],
             N, C, D, H, W, dev.stream)
    dev.sync()
    err = {"gx": float(np.abs(dev.host(gx) - want["gx"]).max())}
    for d in range(4):
        err[f"gw{d}"] = float(np.abs(dev.host(gw[d]) - want[f"gw{d}"]).max())
    assert max(err.values()) <= TOL, err
    return err


def lga_dims(x):
    if x.ndim == 5:
        return x.shape[0] * x.shape[1], x.shape[2], x.shape[3], x.shape[4]
    return x.shape


def _lga_errs(got, want):
    """max abs error per result against the oracle's (`want` None: no oracle at this size, the caller compares runs)"""
    if want is None:
        return {k: 0.0 for k in got}
    err = {k: float(np.abs(got[k] - want[k]).max()) for k in got}
    assert max(err.values()) <= TOL, err
    return err


def check_lga_chain(api, dev, x, f, gy, r, passes, want, out=None):
    """Chained LGA passes (Lga/Lga2/Lga3 and the 3d forms) through the one-pass ABI.  `out`: dict that receives the results."""
    B, D, H, W = lga_dims(x)
    df = dev.to(f)
    ins = [dev.to(x)]
    for _ in range(passes):
        y = dev.empty(x.shape)
        api.call("ganet_lga_forward", dev.ptr(ins[-1]), dev.ptr(df), dev.ptr(y), B, D, H, W, r, dev.stream)
        ins.append(y)
    dev.sync()
    got = {"y": dev.host(ins[-1])}
    g = dev.to(gy)
    gf = dev.empty(f.shape)
    for k, xin in enumerate(reversed(ins[:-1])):
        gx = dev.empty(x.shape)
        api.call("ganet_lga_backward", dev.ptr(xin), dev.ptr(df), dev.ptr(g), dev.ptr(gx), dev.ptr(gf),
                 B, D, H, W, r, 1 if k > 0 else 0, dev.stream)
        g = gx
    dev.sync()
    got["gx"], got["gf"] = dev.host(g), dev.host(gf)
    if out is not None:
        out.update(got)
    return _lga_errs(got, want)


def check_lga2_paired(api, dev, x, f, gy, r, passes, want, out=None):
    """The call sequence of Lga2Function with its private intermediate (and the intermediate's gradient) pair-interleaved
    (ganet_amd/functions/GANet.py: _LgaChain): x -> t1 (interleaved) -> y;  gf = gF(t1, gy);  g_t1 (interleaved) = gX(gy);
    gf += gF(x, g_t1);  gx = gX(g_t1).  Radius 2, two passes, even W."""
    assert r == 2 and passes == 2
    B, D, H, W = lga_dims(x)
    dx, df, dgy = dev.to(x), dev.to(f), dev.to(gy)
    pshape = (B, (D + 1) // 2, H, W, 2)
    t1p, y = dev.empty(pshape), dev.empty(x.shape)
    api.call("ganet_lga_apply_paired", dev.ptr(dx), dev.ptr(df), dev.ptr(t1p), B, D, H, W, 2, 0, 0, 1, dev.stream)
    api.call("ganet_lga_apply_paired", dev.ptr(t1p), dev.ptr(df), dev.ptr(y), B, D, H, W, 2, 0, 1, 0, dev.stream)
    gf, gt1p, gx = dev.empty(f.shape), dev.empty(pshape), dev.empty(x.shape)
    api.call("ganet_lga_filter_grad_paired", dev.ptr(t1p), dev.ptr(dgy), dev.ptr(gf), B, D, H, W, 2, 0, 1, 0, dev.stream)
    api.call("ganet_lga_apply_paired", dev.ptr(dgy), dev.ptr(df), dev.ptr(gt1p), B, D, H, W, 2, 1, 0, 1, dev.stream)
    api.call("ganet_lga_filter_grad_paired", dev.ptr(dx), dev.ptr(gt1p), dev.ptr(gf), B, D, H, W, 2, 1, 0, 1, dev.stream)
    api.call("ganet_lga_apply_paired", dev.ptr(gt1p), dev.ptr(df), dev.ptr(gx), B, D, H, W, 2, 1, 1, 0, dev.stream)
    dev.sync()
    got = {"y": dev.host(y), "gx": dev.host(gx), "gf": dev.host(gf)}
    if out is not None:
        out.update(got)
    err = _lga_errs(got, want)
    # The same chain with the filters' edge sums as a side channel (ganet_lga_apply_paired_edges, what Lga2Function runs when a
    # backward will follow): written by the first pass, read by both data-backward launches.  The sums are the same loads added
    # in the same order on either side, so every result is bit-identical; the buffer itself is checked against its definition.
    edge = dev.empty((B, 3, H, W))
    t1e, gt1e, gxe = dev.empty(pshape), dev.empty(pshape), dev.empty(x.shape)
    api.call("ganet_lga_apply_paired_edges", dev.ptr(dx), dev.ptr(df), dev.ptr(t1e), dev.ptr(edge), B, D, H, W, 2, 0, 0, 1, dev.stream)
    api.call("ganet_lga_apply_paired_edges", dev.ptr(dgy), dev.ptr(df), dev.ptr(gt1e), dev.ptr(edge), B, D, H, W, 2, 1, 0, 1, dev.stream)
    api.call("ganet_lga_apply_paired_edges", dev.ptr(gt1e), dev.ptr(df), dev.ptr(gxe), dev.ptr(edge), B, D, H, W, 2, 1, 1, 0, dev.stream)
    dev.sync()
    assert np.array_equal(dev.host(t1e), dev.host(t1p)) and np.array_equal(dev.host(gt1e), dev.host(gt1p))
    assert np.array_equal(dev.host(gxe), dev.host(gx))
    he = dev.host(edge)
    inside = np.zeros((25, H, W), bool)
    for a in range(-2, 3):
        for b in range(-2, 3):
            ii, jj = np.arange(H)[:, None] + a, np.arange(W)[None, :] + b
            inside[(a + 2) * 5 + (b + 2)] = (ii >= 0) & (ii < H) & (jj >= 0) & (jj < W)
    f3 = f.reshape(B, 3, 25, H, W)
    want_edge = np.stack([(f3 * ~inside).sum((1, 2)), (f3[:, 0] * inside).sum(1), (f3[:, 2] * inside).sum(1)], 1)
    assert np.abs(he - want_edge).max() <= 1e-5, float(np.abs(he - want_edge).max())
    return err


def to_paired(v):
    """[B, D, H, W] -> the pair-interleaved layout [B, ceil(D/2), H, W, 2] of ganet_lga_apply_paired (odd D: zero odd half)."""
    B, D, H, W = v.shape
    out = np.zeros((B, (D + 1) // 2, H, W, 2), np.float32)
    out[..., 0] = v[:, 0::2]
    out[:, :D // 2, :, :, 1] = v[:, 1::2]
    return out


def from_paired(p, D):
    B, _, H, W, _ = p.shape
    v = np.empty((B, D, H, W), np.float32)
    v[:, 0::2] = p[..., 0][:, :(D + 1) // 2]
    v[:, 1::2] = p[..., 1][:, :D // 2]
    return v

