"""The edge-shape cases of the streaming and fused kernels (ganet_amd/csrc/misc_kernels.h), shared by
tests/test_sim_misc_edges.py (emulator build, numpy buffers behind guard pages) and tests/test_gpu_misc_edges.py (gfx950
build, device buffers).  Like parity_cases.py / value_cases.py: a case takes the C ABI (`api`) and a device object with
to / empty / host / ptr / sync / stream, calls the entry points directly -- so the dispatch branch taken is known from the
shape and the pointers' alignment -- and returns the arrays to compare as a list of Cmp; check() asserts them.

References are the float64 statements of tests/misc_ref64.py (trilinear: ATen on the CPU in fp32, see there).  Bars:
  * "bits"   the same bit pattern (pure copies, or two kernel forms that evaluate one expression per element);
  * "equal"  IEEE equality with the float64 result, on inputs that make every product and partial sum representable in
             fp32 (small integers, multiples of 2^-10 / 2^-4): no order of summation, no contraction may show;
  * "close"  the bars of tests/test_sim_fused.py for the same op; where the L1 norm is clamped to 1e-12 the values are
             x / 1e-12 resp. gy / 1e-12, and the comparison is relative only there.

A case id names the branch it reaches: `-vec4` / `-scalar` (the 16-byte form and its scalar twin: size not a multiple of
four, or `-offset1`: every tensor starts 4 bytes behind a 16-byte boundary), `-D<n>` (depth against the chunks of 8 resp.
4 of the depth loops: 1, below, equal, one more, many), `-DgtW`, `-stride2` (a grid-stride loop's second trip: more lanes
than the 4096 x 256 of one launch), `-gridy` (more slices than gridDim.y can hold), `-slowloop` (trilinear backward with
a W footprint of 12 outputs or more)."""
import numpy as np

import misc_ref64 as r64

MAX_LANES = 4096 * 256            # ew_grid() in ganet_capi.hip: blocks are capped, the kernels loop


class Cmp:
    def __init__(self, name, got, want, kind, rtol=0.0, atol=0.0, rel_only=None):
        self.name, self.got, self.want, self.kind = name, got, want, kind
        self.rtol, self.atol, self.rel_only = rtol, atol, rel_only


class Case:
    """device_only: too slow for the emulator (it pays per launched block, not per element of work)"""

    def __init__(self, id, fn, *args, device_only=False):
        self.id, self.fn, self.args, self.device_only = id, fn, args, device_only

    def run(self, api, dev):
        return self.fn(api, dev, *self.args)

    def __repr__(self):
        return self.id


def check(cmps):
    assert cmps
    for c in cmps:
        got = np.asarray(c.got)
        if c.kind == "zeros":                 # want: where the result must be exactly zero -- there and nowhere else
            assert np.array_equal(got == 0, c.want), (c.name, int(((got == 0) != c.want).sum()))
            continue
        assert got.dtype == np.float32 and got.shape == np.shape(c.want), (c.name, got.dtype, got.shape, np.shape(c.want))
        if c.kind == "bits":
            want = np.asarray(c.want)
            if want.dtype != np.float32:
                assert np.array_equal(want.astype(np.float32).astype(np.float64), want), c.name
                want = want.astype(np.float32)
            bad = got.view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)
            assert not bad.any(), (c.name, f"{int(bad.sum())} of {bad.size} elements differ in their bits")
        elif c.kind == "equal":
            want = np.asarray(c.want, np.float64)
            bad = ~(got.astype(np.float64) == want)                   # (a NaN is unequal)
            assert not bad.any(), (c.name, f"{int(bad.sum())} of {bad.size} elements differ",
                                   float(np.nanmax(np.abs(got - want))))
        else:
            assert c.kind == "close"
            want = np.asarray(c.want, np.float64)
            assert np.isfinite(got).all(), (c.name, "not finite", int((~np.isfinite(got)).sum()))
            if c.rel_only is None:
                np.testing.assert_allclose(got, want, rtol=c.rtol, atol=c.atol, err_msg=c.name)
            else:
                m = np.broadcast_to(c.rel_only, got.shape)
                np.testing.assert_allclose(got[~m], want[~m], rtol=c.rtol, atol=c.atol, err_msg=c.name)
                np.testing.assert_allclose(got[m], want[m], rtol=c.rtol, atol=0, err_msg=c.name + " (clamped norm)")


# ---- buffers at 16-byte aligned + 4 k bytes ------------------------------------------------------------------------------------
def put(dev, a, offset_elems=0):
    """a copy of `a` on the device; offset_elems = k: a view that starts k floats into a larger flat allocation, which ends
    with the tensor's last element (contiguous, 4-byte aligned: what the entries document as supported)"""
    a = np.ascontiguousarray(a, np.float32)
    k = offset_elems
    if k == 0:
        v = dev.to(a)
    else:
        flat = dev.to(np.concatenate([np.full(k, np.nan, np.float32), a.ravel()]))
        v = flat[k:].reshape(a.shape)
    assert dev.ptr(v) % 16 == 4 * k
    return v


def new(dev, shape, offset_elems=0):
    """an output buffer poisoned with NaN (dev.empty), placed like put()"""
    k = offset_elems
    v = dev.empty(tuple(shape)) if k == 0 else dev.empty((int(np.prod(shape)) + k,))[k:].reshape(tuple(shape))
    assert dev.ptr(v) % 16 == 4 * k
    return v


def _p(dev, *vs):
    return [None if v is None else dev.ptr(v) for v in vs]


def _form(vec4):
    return "vec4" if vec4 else "scalar"


def _rng(*key):
    return np.random.default_rng([int(v) for v in key])


# ---- cost volume -------------------------------------------------------------------------------------------------------------
def costvol(api, dev, shape, k):
    """forward: copies and zeros, bit-equal; backward on integer gradients in [-3, 3]: every sum exact, EQUAL element by
    element to the float64 adjoint (the clamped loads at Dn-1 / W-1 of the chunks of 8 are masked by value)"""
    N, C, H, W, Dn = shape
    rng = _rng(1, *shape)
    x = rng.standard_normal((N, C, H, W)).astype(np.float32)
    y = rng.standard_normal((N, C, H, W)).astype(np.float32)
    g = rng.integers(-3, 4, (N, 2 * C, Dn, H, W)).astype(np.float32)
    dx, dy, dg = put(dev, x, k), put(dev, y, k), put(dev, g, k)
    cost, gx, gy = new(dev, g.shape, k), new(dev, x.shape, k), new(dev, x.shape, k)
    api.call("ganet_cost_volume_forward", *_p(dev, dx, dy, cost), N, C, Dn, H, W, dev.stream)
    api.call("ganet_cost_volume_backward", *_p(dev, dg, gx, gy), N, C, Dn, H, W, dev.stream)
    dev.sync()
    wgx, wgy = r64.cost_volume_adjoint(g, C)
    assert np.abs(g).sum(2).max() < 2 ** 24
    return [Cmp("cost", dev.host(cost), r64.cost_volume(x, y, Dn), "bits"),
            Cmp("gx", dev.host(gx), wgx, "equal"), Cmp("gy", dev.host(gy), wgy, "equal")]


COSTVOL_SHAPES = [(1, 2, 3, 5, 9), (2, 1, 2, 4, 17), (1, 1, 2, 1, 3), (1, 2, 2, 8, 8), (1, 1, 1, 12, 30), (1, 3, 2, 7, 1),
                  (1, 2, 3, 8, 9)]                                    # (N, C, H, W, Dn)


def _depth_tag(Dn, W=None):
    return f"D{Dn}" + ("-DgtW" if W is not None and Dn > W else "")


# ---- disparity regression ----------------------------------------------------------------------------------------------------
def dispreg(api, dev, N, Dn, H, W, k):
    """x: multiples of 2^-10 in [0, 1], gout: multiples of 2^-10 in [-1, 1]: d * x and every partial sum (non-negative terms,
    total below 2^14) are exact, so both directions are EQUAL to float64"""
    rng = _rng(2, N, Dn, H, W)
    x = (rng.integers(0, 1025, (N, Dn, H, W)) / 1024.0).astype(np.float32)
    go = (rng.integers(-1024, 1025, (N, H, W)) / 1024.0).astype(np.float32)
    want = r64.regression(x)
    assert want.max() * 1024 < 2 ** 24, "the sums must stay on fp32's grid"
    dx, dgo = put(dev, x, k), put(dev, go, k)
    out, gx = new(dev, go.shape, k), new(dev, x.shape, k)
    api.call("ganet_disparity_regression_forward", *_p(dev, dx, out), N, Dn, H, W, dev.stream)
    api.call("ganet_disparity_regression_backward", *_p(dev, dgo, gx), N, Dn, H, W, dev.stream)
    dev.sync()
    return [Cmp("out", dev.host(out), want, "equal"), Cmp("gx", dev.host(gx), r64.regression_adjoint(go, Dn), "equal")]


# ---- L1 normalise ------------------------------------------------------------------------------------------------------------
def l1norm(api, dev, K, G, C, H, W):
    """x [N,G,C,K,H,W] -> y_g [N,C,K,H,W]: 30 % exact-zero taps, negative taps, all-zero groups and groups of +-1e-15 taps
    (sum |x| = K * 1e-15: clamped, but not zero)"""
    N = 4
    rng = _rng(3, K, G, C, H, W)
    gk = rng.standard_normal((N, G, C, H, W, K)) * (rng.random((N, G, C, H, W, K)) > 0.3)
    flat = gk.reshape(-1, K)
    tiny = 1e-15 * rng.choice([-1.0, 1.0], K)
    flat[0, 0], flat[0, K // 2] = -1.5, 0.0
    flat[1], flat[2] = 0.0, tiny
    if len(flat) > 8:
        flat[-1], flat[-2] = 0.0, -tiny
    x = np.ascontiguousarray(np.moveaxis(gk, -1, 3)).astype(np.float32)
    clamped = r64.l1_clamped(x, 3)
    assert clamped.any() and (x[clamped] != 0).any() and (x[~clamped] == 0).any() and (x < 0).any()
    gys = rng.standard_normal((G, N, C, K, H, W)).astype(np.float32)
    dx = put(dev, x)
    ys = [new(dev, gys[0].shape) if g < G else None for g in range(4)]
    dgys = [put(dev, gys[g]) if g < G else None for g in range(4)]
    gx = new(dev, x.shape)
    api.call("ganet_l1_normalize_forward", *_p(dev, dx, *ys), N, G, C, K, H, W, dev.stream)
    api.call("ganet_l1_normalize_backward", *_p(dev, dx, *dgys, gx), N, G, C, K, H, W, dev.stream)
    dev.sync()
    want = r64.l1_normalize(x, 3)
    out = []
    for g in range(G):
        out += [Cmp(f"y{g}", dev.host(ys[g]), want[:, g], "close", 1e-5, 1e-6, rel_only=clamped[:, g]),
                Cmp(f"y{g} zero set", dev.host(ys[g]), x[:, g] == 0, "zeros")]
    out.append(Cmp("gx", dev.host(gx), r64.l1_normalize_adjoint(x, np.moveaxis(gys, 0, 1), 3), "close", 1e-4, 1e-5,
                   rel_only=clamped))
    return out


# ---- normalised regression ---------------------------------------------------------------------------------------------------
def _special_pixels(HW):
    """where the four special columns go: pixels 0..3 (HW = 4: every pixel), and the last four of a large image as well (the
    grid-stride trips' far end)"""
    return [0, 1, 2, 3] if HW < 64 else [0, 1, 2, 3, HW - 4, HW - 3, HW - 2, HW - 1]


def normreg_inputs(N, D, H, W):
    rng = _rng(4, N, D, H, W)
    x = rng.standard_normal((N, D, H * W)).astype(np.float32)
    sp = _special_pixels(H * W)
    for j in range(0, len(sp), 4):                       # (pixel sp[j] stays an ordinary signed one)
        x[0, :, sp[j + 1]] = 0.0
        x[0, :, sp[j + 2]] = 1e-15 * rng.choice([-1.0, 1.0], D)
        x[0, 1::2, sp[j + 3]] = 0.0
    go = rng.standard_normal((N, H, W)).astype(np.float32)
    return x.reshape(N, D, H, W), go


def normreg(api, dev, N, D, H, W, k):
    """signed inputs with an all-zero pixel, a pixel of +-1e-15 entries (norm clamped, values not zero) and a pixel whose
    every second entry is exactly zero (sgn(0) = 0); the backward reads the forward's own out / snorm, as the autograd
    Function does"""
    x, go = normreg_inputs(N, D, H, W)
    dx, dgo = put(dev, x, k), put(dev, go, k)
    out, sn, gx = new(dev, go.shape, k), new(dev, go.shape, k), new(dev, x.shape, k)
    api.call("ganet_norm_disparity_regression_forward", *_p(dev, dx, out, sn), N, D, H, W, dev.stream)
    api.call("ganet_norm_disparity_regression_backward", *_p(dev, dx, out, sn, dgo, gx), N, D, H, W, dev.stream)
    dev.sync()
    wout, wsn = r64.norm_regression(x)
    clamped = r64.l1_clamped(x, 1)
    assert clamped.any() and (x[clamped] != 0).any()
    return [Cmp("out", dev.host(out), wout, "close", 1e-5, 1e-4), Cmp("snorm", dev.host(sn), wsn, "close", 1e-5, 0.0),
            Cmp("gx", dev.host(gx), r64.norm_regression_adjoint(x, go), "close", 1e-4, 1e-4, rel_only=clamped)]


VOLUME_SHAPES = [(1, 1, 1, 4), (1, 9, 2, 4), (1, 13, 3, 5), (2, 193, 1, 4), (1, 12, 2, 6)]         # (N, D, H, W)


# ---- softmin, softmin + regression -------------------------------------------------------------------------------------------
def softmin_inputs(N, D, H, W):
    """5 * randn, and four special columns: +1e4 .. -1e4 (every chunk moves the running maximum by thousands: whatever was
    summed before must rescale to exactly 0, not to NaN), a constant one, +300 .. -300 (the rescale factors are ordinary
    numbers and matter), and 50 everywhere but -50 at the very last index (the minimum sits in the tail chunk)"""
    rng = _rng(5, N, D, H, W)
    x = (5 * rng.standard_normal((N, D, H * W))).astype(np.float32)
    sp = _special_pixels(H * W)
    for j in range(0, len(sp), 4):
        x[0, :, sp[j]] = np.linspace(1e4, -1e4, D)
        x[0, :, sp[j + 1]] = 7.25
        x[0, :, sp[j + 2]] = np.linspace(300.0, -300.0, D)
        x[0, :, sp[j + 3]] = 50.0
        x[0, D - 1, sp[j + 3]] = -50.0
    return x.reshape(N, D, H, W), rng


def softmin(api, dev, N, D, H, W, k):
    """forward against float64; the backward is a function of the OUTPUT: it is handed the float64 result rounded to fp32
    and compared with the float64 adjoint at that same y"""
    x, rng = softmin_inputs(N, D, H, W)
    gy = rng.standard_normal(x.shape).astype(np.float32)
    want = r64.softmin(x)
    y32 = want.astype(np.float32)
    dx, dy32, dgy = put(dev, x, k), put(dev, y32, k), put(dev, gy, k)
    y, gx = new(dev, x.shape, k), new(dev, x.shape, k)
    api.call("ganet_softmin_forward", *_p(dev, dx, y), N, D, H, W, dev.stream)
    api.call("ganet_softmin_backward", *_p(dev, dy32, dgy, gx), N, D, H, W, dev.stream)
    dev.sync()
    return [Cmp("y", dev.host(y), want, "close", 2e-6, 1e-7),
            Cmp("gx", dev.host(gx), r64.softmin_adjoint(y32, gy), "close", 1e-5, 1e-5)]


def softminreg(api, dev, N, D, H, W, k):
    """out = sum_d d * softmin(x) in one walk; mx must be max(-x) exactly; the backward recomputes the probabilities from the
    forward's own mx / ssum / out"""
    x, rng = softmin_inputs(N, D, H, W)
    go = rng.standard_normal((N, H, W)).astype(np.float32)
    dx, dgo = put(dev, x, k), put(dev, go, k)
    out, mx, ss, gx = new(dev, go.shape, k), new(dev, go.shape, k), new(dev, go.shape, k), new(dev, x.shape, k)
    api.call("ganet_softmin_regression_forward", *_p(dev, dx, out, mx, ss), N, D, H, W, dev.stream)
    api.call("ganet_softmin_regression_backward", *_p(dev, dx, out, mx, ss, dgo, gx), N, D, H, W, dev.stream)
    dev.sync()
    hss = dev.host(ss)
    assert np.isfinite(hss).all() and (hss >= 1).all() and (hss <= D).all()
    return [Cmp("out", dev.host(out), r64.softmin_regression(x), "close", 1e-5, 1e-4),
            Cmp("mx", dev.host(mx), (-x.astype(np.float64)).max(1), "equal"),
            Cmp("gx", dev.host(gx), r64.softmin_regression_adjoint(x, go), "close", 1e-4, 1e-4)]


# ---- residual tail -----------------------------------------------------------------------------------------------------------
def _dyadic(rng, shape):
    return (rng.integers(-64, 65, shape) / 16.0).astype(np.float32)             # multiples of 2^-4, |.| <= 4


def residual(api, dev, shape, folded):
    """dyadic t, rem, scale, shift, gy: scale * t + shift + rem and scale * g are exact -- EQUAL to float64, zero set included"""
    N, C, D, H, W = shape
    rng = _rng(6, *shape, folded)
    t, rem, gy = _dyadic(rng, shape), _dyadic(rng, shape), _dyadic(rng, shape)
    scale, shift = (_dyadic(rng, C), _dyadic(rng, C)) if folded else (None, None)
    dt, drem, dgy = put(dev, t), put(dev, rem), put(dev, gy)
    dsc, dsh = (put(dev, scale), put(dev, shift)) if folded else (None, None)
    y, g_rem = new(dev, shape), new(dev, shape)
    g_t = new(dev, shape) if folded else None
    api.call("ganet_residual_relu_forward", *_p(dev, dt, drem, dsc, dsh, y), N, C, D, H, W, dev.stream)
    api.call("ganet_residual_relu_backward", *_p(dev, y, dgy, dsc, g_t, g_rem), N, C, D, H, W, dev.stream)
    dev.sync()
    want = r64.residual_relu(t, rem, scale, shift)
    assert 0.2 < (want == 0).mean() < 0.8
    w_t, w_rem = r64.residual_relu_adjoint(want, gy, scale)
    out = [Cmp("y", dev.host(y), want, "equal"), Cmp("y zero set", dev.host(y), want == 0, "zeros"),
           Cmp("g_rem", dev.host(g_rem), w_rem, "equal")]
    if folded:
        out.append(Cmp("g_t", dev.host(g_t), w_t, "equal"))
    return out


# ---- the 16-byte form and its scalar twin evaluate one expression per element ---------------------------------------------------
def twin_costvol(api, dev):
    N, C, H, W, Dn = 2, 3, 5, 12, 9
    rng = _rng(7)
    x, y = (rng.standard_normal((N, C, H, W)).astype(np.float32) for _ in range(2))
    res = []
    for k in (0, 1):
        dx, dy, cost = put(dev, x, k), put(dev, y, k), new(dev, (N, 2 * C, Dn, H, W), k)
        api.call("ganet_cost_volume_forward", *_p(dev, dx, dy, cost), N, C, Dn, H, W, dev.stream)
        dev.sync()
        res.append(np.array(dev.host(cost)))
    return [Cmp("cost: offset 1 against offset 0", res[1], res[0], "bits")]


def twin_dispreg_bwd(api, dev):
    N, Dn, H, W = 2, 13, 3, 8
    go = _rng(8).standard_normal((N, H, W)).astype(np.float32)
    res = []
    for k in (0, 1):
        dgo, gx = put(dev, go, k), new(dev, (N, Dn, H, W), k)
        api.call("ganet_disparity_regression_backward", *_p(dev, dgo, gx), N, Dn, H, W, dev.stream)
        dev.sync()
        res.append(np.array(dev.host(gx)))
    assert np.isfinite(res[0]).all()
    return [Cmp("gx: offset 1 against offset 0", res[1], res[0], "bits")]


def twin_residual(api, dev, folded):
    shape = (2, 3, 5, 3, 8)
    N, C, D, H, W = shape
    rng = _rng(9, folded)
    t, rem, gy = (rng.standard_normal(shape).astype(np.float32) for _ in range(3))
    scale, shift = (rng.standard_normal(C).astype(np.float32) for _ in range(2)) if folded else (None, None)
    res = []
    for k in (0, 1):
        dsc, dsh = (put(dev, scale), put(dev, shift)) if folded else (None, None)
        dt, drem, dgy = put(dev, t, k), put(dev, rem, k), put(dev, gy, k)
        y, g_rem = new(dev, shape, k), new(dev, shape, k)
        g_t = new(dev, shape, k) if folded else None
        api.call("ganet_residual_relu_forward", *_p(dev, dt, drem, dsc, dsh, y), N, C, D, H, W, dev.stream)
        api.call("ganet_residual_relu_backward", *_p(dev, y, dgy, dsc, g_t, g_rem), N, C, D, H, W, dev.stream)
        dev.sync()
        res.append([np.array(dev.host(v)) for v in ((y, g_rem, g_t) if folded else (y, g_rem))])
    assert all(np.isfinite(v).all() for v in res[0]) and 0.2 < (res[0][0] == 0).mean() < 0.8
    return [Cmp(f"{n}: offset 1 against offset 0", b, a, "bits") for n, a, b in zip(("y", "g_rem", "g_t"), res[0], res[1])]


# ---- trilinear -----------------------------------------------------------------------------------------------------------------
def _aten_trilinear(x, gy, osz):
    import torch
    import torch.nn.functional as F
    xt = torch.from_numpy(x).requires_grad_()
    yt = F.interpolate(xt, size=list(osz), mode="trilinear", align_corners=False)
    yt.backward(torch.from_numpy(gy))
    return yt.detach().numpy(), xt.grad.numpy()


def _trilinear_launch(api, dev, x, gy, isz, osz):
    """-> (y, gx, the input buffers: they must outlive the launches)"""
    S = x.shape[1]
    dx, dgy, y, gx = put(dev, x), put(dev, gy), new(dev, gy.shape), new(dev, x.shape)
    api.call("ganet_trilinear_upsample_forward", *_p(dev, dx, y), S, *isz, *osz, dev.stream)
    api.call("ganet_trilinear_upsample_backward", *_p(dev, dgy, gx), S, *isz, *osz, dev.stream)
    return y, gx, (dx, dgy)


def _trilinear_cmps(tag, y, gx, x, gy, osz):
    wy, wgx = _aten_trilinear(x, gy, osz)
    return [Cmp(f"y{tag}", y, wy, "close", 1e-5, 1e-6), Cmp(f"gx{tag}", gx, wgx, "close", 1e-5, 1e-5)]


def trilinear(api, dev, isz, osz):
    S = 2
    rng = _rng(10, *isz, *osz)
    x = rng.standard_normal((1, S) + isz).astype(np.float32)
    gy = rng.standard_normal((1, S) + osz).astype(np.float32)
    y, gx, keep = _trilinear_launch(api, dev, x, gy, isz, osz)
    dev.sync()
    return _trilinear_cmps("", dev.host(y), dev.host(gx), x, gy, osz)


TRILINEAR_PAIRS = [("slowloop", (2, 3, 4), (3, 4, 29)), ("slowloop", (3, 2, 5), (2, 2, 64)), ("slowloop", (1, 1, 2), (1, 1, 40)),
                   ("slowloop-deep", (2, 2, 3), (13, 15, 31)), ("slowloop-onevoxel", (1, 1, 1), (9, 9, 30)),
                   ("down", (1, 1, 7), (1, 1, 3)), ("down", (1, 1, 100), (1, 1, 33)), ("up", (1, 1, 33), (1, 1, 100))]
SWEEP_IN, SWEEP_OUT = range(1, 13), range(1, 40)


def trilinear_sweep(api, dev):
    """every (in, out) with in = 1..12, out = 1..39 on the W axis: up_range's promise (a superset of the outputs that read an
    input) and both loops of the backward at every ratio between 1/12 and 39.  Every launch is issued first; one
    synchronisation; then the comparisons."""
    rng = _rng(11)
    runs = []
    for wi in SWEEP_IN:
        for wo in SWEEP_OUT:
            x = rng.standard_normal((1, 2, 1, 1, wi)).astype(np.float32)
            gy = rng.standard_normal((1, 2, 1, 1, wo)).astype(np.float32)
            runs.append((wi, wo, x, gy) + _trilinear_launch(api, dev, x, gy, (1, 1, wi), (1, 1, wo)))
    dev.sync()
    out = []
    for wi, wo, x, gy, y, gx, _ in runs:
        out += _trilinear_cmps(f" {wi}->{wo}", dev.host(y), dev.host(gx), x, gy, (1, 1, wo))
    return out


# ---- the case tables -----------------------------------------------------------------------------------------------------------
def _cases():
    cs = []
    for shape in COSTVOL_SHAPES:
        N, C, H, W, Dn = shape
        for k in (0, 1):
            cs.append(Case(f"costvol-{N}x{C}x{H}x{W}-{_depth_tag(Dn, W)}-{_form(W % 4 == 0 and k == 0)}-offset{k}", costvol, shape, k))
    for Dn in (1, 7, 8, 9, 193):
        for H, W in ((1, 4), (3, 5), (2, 6)):
            for k in (0, 1):
                cs.append(Case(f"dispreg-{H}x{W}-D{Dn}-{_form(H * W % 4 == 0 and k == 0)}-offset{k}", dispreg, 2, Dn, H, W, k))
    for K in (5, 75, 9):
        for G, C in ((4, 2), (1, 1)):
            for H, W in ((1, 1), (3, 5)):
                cs.append(Case(f"l1norm-K{K}-{'registers' if K in (5, 75) else 'walk'}-G{G}C{C}-{H}x{W}", l1norm, K, G, C, H, W))
    for name, fn in (("normreg", normreg), ("softmin", softmin), ("softminreg", softminreg)):
        for N, D, H, W in VOLUME_SHAPES:
            for k in (0, 1):
                form = "" if name == "softminreg" else "-" + _form(H * W % 4 == 0 and k == 0)
                cs.append(Case(f"{name}-{N}x{D}x{H}x{W}{form}-offset{k}", fn, N, D, H, W, k))
    for shape in ((2, 32769, 1, 1, 4), (2, 32769, 1, 1, 3)):
        for folded in (True, False):
            # 65538 slices of 4 resp. 3 elements: the `s += gridDim.y` trip.  Two launches of 65535 blocks cost the emulator
            # 26 s per case: on the device only
            cs.append(Case(f"residual-gridy-{_form(shape[-1] % 4 == 0)}-{'folded' if folded else 'noscale'}", residual, shape, folded,
                           device_only=True))
    cs += [Case("twin-costvol-fwd", twin_costvol), Case("twin-dispreg-bwd", twin_dispreg_bwd),
           Case("twin-residual-folded", twin_residual, True), Case("twin-residual-noscale", twin_residual, False)]
    for tag, isz, osz in TRILINEAR_PAIRS:
        cs.append(Case("trilinear-%s-%s-to-%s" % (tag, "x".join(map(str, isz)), "x".join(map(str, osz))), trilinear, isz, osz))
    cs.append(Case("trilinear-sweep-w", trilinear_sweep))
    return cs


def _grid_cases():
    """The second trip of the grid-stride loops: more lanes than one launch holds.  [1,2,1025,1024] (1,049,600 pixels, a
    multiple of four) and [1,3,1025,1025] (1,050,625, odd) for the one-pixel-per-lane forms -- at the first, the entries
    that have a four-pixel form take it (262,400 lanes, one trip) unless the pointers are misaligned, so softmin runs there
    at offset 1 as well; [1,2,2049,2048] for the four-pixel forms (1,049,088 lanes).  The special columns sit at both ends
    of the image."""
    cs = []
    for name, fn in (("dispreg", dispreg), ("normreg", normreg), ("softmin", softmin), ("softminreg", softminreg)):
        for (N, D, H, W), ks in (((1, 2, 1025, 1024), (0, 1) if name == "softmin" else (0,)), ((1, 3, 1025, 1025), (0,)),
                                 ((1, 2, 2049, 2048), (0,))):
            for k in ks:
                vec4 = H * W % 4 == 0 and k == 0
                lanes = N * H * W // 4 if vec4 else N * H * W
                assert lanes > MAX_LANES or (H, W) == (1025, 1024)
                form = "" if name == "softminreg" else "-" + _form(vec4)      # (dispreg / normreg: the backward's form)
                cs.append(Case(f"{name}-stride2-{H}x{W}-D{D}{form}-offset{k}", fn, N, D, H, W, k))
    return cs


CASES = _cases()
GRID_CASES = _grid_cases()
