"""TEST INFRASTRUCTURE: the case table of the channels-last kernels (ganet_amd/csrc/cl_kernels.h: ganet_bn_apply_forward_cl,
ganet_cost_volume_forward_cl), run on the emulator by tests/test_sim_cl.py and on the device by tests/test_gpu_cl.py through one
`dev` (parity_cases.NumpyDev / test_gpu_parity.TorchDev).

The yardstick has no tolerance in it.  For every layout combination the output bits equal
    the planar entry of the SAME build (ganet_bn_apply_forward, ganet_cost_volume_forward) on the permuted input, permuted back,
and, independently, a numpy float32 statement with a correctly rounded fused multiply-add (mixed_train_cases.fma32).
NaN positions must agree; every other element bit for bit (mixed_cases.assert_same)."""
import numpy as np

import mixed_cases as mc
from mixed_train_cases import fma32

F32 = np.float32
PLANAR, CL = 0, 1                                   # GANET_LAYOUT_PLANAR / GANET_LAYOUT_CL
E_INVALID, E_UNSUPPORTED = -1, -2
ENTRIES = ("ganet_bn_apply_forward_cl", "ganet_cost_volume_forward_cl")

# cl_kernels.h (held to the source by tests/test_cl_cpu.py)
CL_BLOCK, CL_T, CL_CB, CL_MAX_BLOCKS = 256, 128, 64, 2048
CV_TW, CV_DB, CV_CB = 64, 32, 32
T = CL_T

# (x, rem, y) layouts: "none" = no rem
COMBOS = {
    "cl-none-cl": (CL, None, CL),
    "cl-none-planar": (CL, None, PLANAR),
    "planar-none-cl": (PLANAR, None, CL),
    "cl-planar-cl": (CL, PLANAR, CL),
    "cl-planar-planar": (CL, PLANAR, PLANAR),
    "planar-planar-cl": (PLANAR, PLANAR, CL),       # beyond the five call sites: a tail whose convolution answered in planar
}
BN_C = (1, 3, 4, 5, 32, 48, 64, 67, 130)            # 67, 130: more than one channel block of CL_CB
BN_S = (1, 2, T - 1, T, T + 1, 4 * T + 3, 1031)
BN_N = (1, 2)
RELU_OFF_S = (T + 1,)                               # sizes that also run with relu = 0


# ---- layouts ------------------------------------------------------------------------------------------------------------------

def to_cl(a):
    """[N,C,S] values -> the [N,S,C] memory image"""
    return np.ascontiguousarray(np.asarray(a).transpose(0, 2, 1))


def from_cl(b):
    """the [N,S,C] memory image -> [N,C,S] values"""
    return np.ascontiguousarray(np.asarray(b).transpose(0, 2, 1))


def image(a, layout):
    return to_cl(a) if layout == CL else np.ascontiguousarray(a)


def values(buf, layout, N, C, S):
    return from_cl(buf.reshape(N, S, C)) if layout == CL else buf.reshape(N, C, S)


def cv_to_cl(cost):
    """[N,2C,Dn,H,W] -> the [N,Dn,H,W,2C] memory image"""
    return np.ascontiguousarray(np.asarray(cost).transpose(0, 2, 3, 4, 1))


def cv_from_cl(cost):
    return np.ascontiguousarray(np.asarray(cost).transpose(0, 4, 1, 2, 3))


# ---- the statement ------------------------------------------------------------------------------------------------------------

def bn_statement(x, rem, scale, shift, relu):
    """z = fmaf(x, scale[c], shift[c]) [+ rem]; y = relu ? (z <= 0 ? 0 : z) : z -- on [N,C,S] float32, every operation rounded once"""
    with np.errstate(all="ignore"):
        z = fma32(x, scale[None, :, None], shift[None, :, None])
        if rem is not None:
            z = (z + rem).astype(F32)
        return np.where(z <= 0, F32(0), z).astype(F32) if relu else z


def cv_statement(x, y, Dn):
    """cost[n,d,h,w,c] = w >= d ? x[n,c,h,w] : +0, cost[n,d,h,w,C+c] = w >= d ? y[n,c,h,w-d] : +0, as bit patterns [N,Dn,H,W,2C]"""
    N, C, H, W = x.shape
    xb, yb = x.view(np.uint32), y.view(np.uint32)
    cost = np.zeros((N, Dn, H, W, 2 * C), dtype=np.uint32)
    for d in range(min(Dn, W)):
        cost[:, d, :, d:, :C] = xb[:, :, :, d:].transpose(0, 2, 3, 1)
        cost[:, d, :, d:, C:] = yb[:, :, :, :W - d].transpose(0, 2, 3, 1)
    return cost


# ---- BatchNorm apply ----------------------------------------------------------------------------------------------------------

_DATA = {}


def bn_data(N, C, S, family="general"):
    """x, rem [N,C,S], scale, shift [C]: seeded values of both signs, moved off the ReLU kink (|z| < 2^-8, with and without
    the rem) as bn_cases.Case does; "special": exact zeros, -0, +-inf and NaN in x and in rem, a channel with scale = 0"""
    key = (N, C, S, family)
    if key in _DATA:
        return _DATA[key]
    rng = np.random.default_rng(1000003 * N + 1009 * C + S)
    x = (rng.normal(0, 1.5, (N, C, S)) + rng.normal(0, 1, (1, C, 1))).astype(F32)
    rem = rng.normal(0, 1, (N, C, S)).astype(F32)
    scale = (rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C)).astype(F32)
    shift = rng.normal(0, 0.5, C).astype(F32)
    for _ in range(20):
        z = x.astype(np.float64) * scale[None, :, None] + shift[None, :, None]
        near = (np.abs(z) < 2.0 ** -8) | (np.abs(z + rem) < 2.0 ** -8)
        if not near.any():
            break
        x[near] += F32(0.25)
    else:
        raise AssertionError("bn_data: values stay on the ReLU kink")
    if family == "special":
        xf, rf = x.reshape(-1), rem.reshape(-1)
        xf[0::7] = np.nan; xf[1::7] = np.inf; xf[2::7] = -np.inf; xf[3::7] = -0.0; xf[4::13] = 0.0
        rf[0::5] = np.nan; rf[1::5] = np.inf; rf[2::5] = -np.inf; rf[3::11] = -0.0; rf[4::17] = 0.0
        scale[C - 1] = 0.0
    for a in (x, rem, scale, shift):
        a.setflags(write=False)
    _DATA[key] = (x, rem, scale, shift)
    return _DATA[key]


_PLANAR = {}


def planar_entry(api, dev, N, C, S, family, has_rem, relu):
    """ganet_bn_apply_forward of this build on the planar operands: computed once per (build, case), shared by the combinations"""
    key = (id(api), N, C, S, family, has_rem, relu)
    if key not in _PLANAR:
        x, rem, scale, shift = bn_data(N, C, S, family)
        dx, dsc, dsh = mc.Buf(dev, mc.F32, data=x), mc.Buf(dev, mc.F32, data=scale), mc.Buf(dev, mc.F32, data=shift)
        dr = mc.Buf(dev, mc.F32, data=rem) if has_rem else None
        dy = mc.Buf(dev, mc.F32, n=x.size)
        api.call("ganet_bn_apply_forward", dx.ptr, dr.ptr if dr else None, dsc.ptr, dsh.ptr, dy.ptr, N, C, S, relu, dev.stream)
        dev.sync()
        want = np.array(dy.host((N, C, S)))
        stated = bn_statement(x, rem if has_rem else None, scale, shift, relu)
        mc.assert_same(want, stated, mc.F32, f"the planar entry against the statement N={N} C={C} S={S} {family} rem={has_rem} relu={relu}")
        want.setflags(write=False)
        _PLANAR[key] = want
    return _PLANAR[key]


def run_bn(api, dev, combo, N, C, S, relu, family="general", off=(0, 0, 0), inplace=False):
    """the entry under test on one case -> y as [N,C,S] values.  off: element offsets of the x, rem and y bases"""
    xl, rl, yl = COMBOS[combo]
    x, rem, scale, shift = bn_data(N, C, S, family)
    dsc, dsh = mc.Buf(dev, mc.F32, data=scale), mc.Buf(dev, mc.F32, data=shift)
    dx = mc.Buf(dev, mc.F32, data=image(x, xl), off=off[0])
    dr = mc.Buf(dev, mc.F32, data=image(rem, rl), off=off[1]) if rl is not None else None
    dy = dx if inplace else mc.Buf(dev, mc.F32, n=x.size, off=off[2])
    api.call("ganet_bn_apply_forward_cl", dx.ptr, dr.ptr if dr else None, dsc.ptr, dsh.ptr, dy.ptr, N, C, S, relu,
             xl, rl if rl is not None else PLANAR, yl, dev.stream)
    dev.sync()
    if not inplace:
        assert np.array_equal(np.asarray(dx.host()).view(np.uint32), image(x, xl).ravel().view(np.uint32)), "x was written"
    if dr is not None:
        assert np.array_equal(np.asarray(dr.host()).view(np.uint32), image(rem, rl).ravel().view(np.uint32)), "rem was written"
    return values(np.asarray(dy.host()), yl, N, C, S)


def check_bn(api, dev, combo, N, C, S, relu, family="general", **kw):
    has_rem = COMBOS[combo][1] is not None
    x, rem, scale, shift = bn_data(N, C, S, family)
    got = run_bn(api, dev, combo, N, C, S, relu, family, **kw)
    what = f"bn {combo} N={N} C={C} S={S} relu={relu} {family} {kw}"
    mc.assert_same(got, planar_entry(api, dev, N, C, S, family, has_rem, relu), mc.F32, what + ": against the planar entry")
    mc.assert_same(got, bn_statement(x, rem if has_rem else None, scale, shift, relu), mc.F32, what + ": against the statement")
    if family == "general":
        assert not np.isnan(got).any(), what + ": an element was not written"


def check_bn_table(api, dev, combo, C):
    for S in BN_S:
        for N in BN_N:
            for relu in ((1, 0) if S in RELU_OFF_S else (1,)):
                check_bn(api, dev, combo, N, C, S, relu)


SPECIAL_SHAPES = ((2, 5, T + 1), (1, 32, 2 * T))
OFFSET_SHAPE = (2, 32, 2 * T + 4)                   # C % 4 == 0 and S % 4 == 0: only the base decides the path
INPLACE = ("cl-none-cl", "cl-planar-cl")
INPLACE_SHAPES = ((2, 32, T + 4), (1, 5, T + 1), (2, 67, 3))
# the grid clamp: CL_MAX_BLOCKS = 2048 blocks per launch.
#   the stream launcher (cl -> cl) takes CL_BLOCK = 256 lane items per block: C = 3 is the scalar form, one element per item,
#   2048 * 256 = 524288 elements fill one trip and 524295 start the second
#   the transposing launcher takes one tile of CL_T = 128 positions x CL_CB channels per block: C = 1, S = 2048 * 128 + 1
#   are 2049 tiles
SECOND_TRIP = {
    "cl-none-cl": (1, 3, 174765),
    "cl-none-planar": (1, 1, CL_MAX_BLOCKS * CL_T + 1),
    "planar-none-cl": (1, 1, CL_MAX_BLOCKS * CL_T + 1),
}


def check_special(api, dev, combo):
    for N, C, S in SPECIAL_SHAPES:
        for relu in (1, 0):
            check_bn(api, dev, combo, N, C, S, relu, family="special")


def check_offsets(api, dev, combo):
    """each base in turn 4 bytes behind an aligned address: that side's scalar requests"""
    N, C, S = OFFSET_SHAPE
    check_bn(api, dev, combo, N, C, S, 1)
    for i in range(3):
        if i == 1 and COMBOS[combo][1] is None:
            continue
        off = [0, 0, 0]
        off[i] = 1
        check_bn(api, dev, combo, N, C, S, 1, off=tuple(off))
    check_bn(api, dev, combo, N, C, S, 1, off=(1, 1, 1))


def check_inplace(api, dev, combo):
    for N, C, S in INPLACE_SHAPES:
        check_bn(api, dev, combo, N, C, S, 1, inplace=True)


def check_second_trip(api, dev, combo):
    N, C, S = SECOND_TRIP[combo]
    if combo == "cl-none-cl":
        assert N * C * S > CL_MAX_BLOCKS * CL_BLOCK and C % 4 != 0
    else:
        assert N * -(-S // CL_T) * -(-C // CL_CB) > CL_MAX_BLOCKS
    check_bn(api, dev, combo, N, C, S, 1)


# ---- cost volume --------------------------------------------------------------------------------------------------------------

CV_C, CV_DN, CV_W, CV_H, CV_N = (1, 3, 32), (1, 5, 9), (1, 4, 7, 70), (1, 3), (1, 2)
# beyond the table: a second chunk of CV_DB = 32 disparities, a second block of CV_CB = 32 channels (with and without 16-byte
# stores), and more tiles than the grid clamp (CL_MAX_BLOCKS = 2048 blocks, one (n, h, columns, disparities, channels) tile each)
CV_EXTRA = ((1, 36, 40, 2, 70), (1, 33, 33, 1, 65), (1, 1, 1, CL_MAX_BLOCKS + 1, 1))


def cv_data(N, C, H, W):
    """every element its own value, x positive and y negative: a misplaced element, or a swapped half, cannot pass"""
    n = N * C * H * W
    x = (1 + np.arange(n, dtype=np.float64)).astype(F32).reshape(N, C, H, W)
    y = (-(1 + np.arange(n, dtype=np.float64)) - 0.5).astype(F32).reshape(N, C, H, W)
    assert n < 2 ** 22
    return x, y


def check_cv(api, dev, N, C, Dn, H, W, off=(0, 0, 0)):
    x, y = cv_data(N, C, H, W)
    n = N * 2 * C * Dn * H * W
    dx, dy = mc.Buf(dev, mc.F32, data=x, off=off[0]), mc.Buf(dev, mc.F32, data=y, off=off[1])
    dc = mc.Buf(dev, mc.F32, n=n, off=off[2])
    api.call("ganet_cost_volume_forward_cl", dx.ptr, dy.ptr, dc.ptr, N, C, Dn, H, W, dev.stream)
    px, py, pc = mc.Buf(dev, mc.F32, data=x), mc.Buf(dev, mc.F32, data=y), mc.Buf(dev, mc.F32, n=n)
    api.call("ganet_cost_volume_forward", px.ptr, py.ptr, pc.ptr, N, C, Dn, H, W, dev.stream)
    dev.sync()
    got = np.asarray(dc.host()).view(np.uint32).reshape(N, Dn, H, W, 2 * C)
    what = f"cost volume N={N} C={C} Dn={Dn} H={H} W={W} off={off}"
    planar = cv_to_cl(np.asarray(pc.host()).reshape(N, 2 * C, Dn, H, W)).view(np.uint32)
    assert np.array_equal(got, planar), what + f": {int((got != planar).sum())} patterns differ from the planar entry, permuted"
    stated = cv_statement(x, y, Dn)
    assert np.array_equal(got, stated), what + f": {int((got != stated).sum())} patterns differ from the statement"
    d, w = np.arange(Dn)[:, None], np.arange(W)[None, :]
    assert (got.transpose(0, 2, 1, 3, 4)[:, :, w < d] == 0).all(), what + ": a masked element is not +0"


def check_cv_table(api, dev, C, Dn):
    for W in CV_W:
        for H in CV_H:
            for N in CV_N:
                check_cv(api, dev, N, C, Dn, H, W)


def check_cv_extra(api, dev):
    for N, C, Dn, H, W in CV_EXTRA:
        check_cv(api, dev, N, C, Dn, H, W)
    for i in range(3):                              # each base in turn 4 bytes behind an aligned address
        off = [0, 0, 0]
        off[i] = 1
        check_cv(api, dev, 2, 32, 5, 3, 8, off=tuple(off))
    check_cv(api, dev, 2, 32, 5, 3, 8, off=(1, 1, 1))


# ---- bad arguments: every row of the error table of include/ganet_hip_cl.h --------------------------------------------------------

def check_bad_arguments(api, dev):
    st = dev.stream
    rc = mc._rc
    a, b, c = (mc.Buf(dev, mc.F32, n=256) for _ in range(3))
    sc, sh = mc.Buf(dev, mc.F32, data=np.ones(4, F32)), mc.Buf(dev, mc.F32, data=np.zeros(4, F32))
    bn = lambda *args: rc(api, "ganet_bn_apply_forward_cl", *args, st)      # noqa: E731
    good = [a.ptr, None, sc.ptr, sh.ptr, b.ptr, 2, 4, 16, 1, CL, PLANAR, PLANAR]
    assert bn(*good) == 0
    for i in (0, 2, 3, 4):                                                   # a NULL pointer
        bad = list(good)
        bad[i] = None
        assert bn(*bad) == E_INVALID
    for i in (5, 6, 7):                                                      # a non-positive size
        for v in (0, -1):
            bad = list(good)
            bad[i] = v
            assert bn(*bad) == E_INVALID
    for i in (9, 10, 11):                                                    # an unknown layout code
        for v in (2, -1):
            bad = list(good)
            bad[i] = v
            assert bn(*bad) == E_INVALID
    # forbidden aliases
    assert bn(a.ptr, None, sc.ptr, sh.ptr, a.ptr, 2, 4, 16, 1, CL, PLANAR, PLANAR) == E_INVALID       # y is x across layouts
    assert bn(a.ptr, None, sc.ptr, sh.ptr, a.ptr, 2, 4, 16, 1, PLANAR, PLANAR, CL) == E_INVALID
    assert bn(a.ptr, c.ptr, sc.ptr, sh.ptr, c.ptr, 2, 4, 16, 1, CL, PLANAR, CL) == E_INVALID          # y is rem
    assert bn(a.ptr, None, sc.ptr, sh.ptr, a.ptr, 2, 4, 16, 1, CL, PLANAR, CL) == 0                   # in place, one layout
    assert bn(a.ptr, c.ptr, sc.ptr, sh.ptr, a.ptr, 2, 4, 16, 1, CL, PLANAR, CL) == 0
    # unsupported
    assert bn(a.ptr, None, sc.ptr, sh.ptr, b.ptr, 2, 4, 16, 1, PLANAR, PLANAR, PLANAR) == E_UNSUPPORTED
    assert "ganet_bn_apply_forward" in api.last_error()                      # ... and says whose job it is
    assert bn(a.ptr, c.ptr, sc.ptr, sh.ptr, b.ptr, 2, 4, 16, 1, PLANAR, PLANAR, PLANAR) == E_UNSUPPORTED
    assert bn(a.ptr, c.ptr, sc.ptr, sh.ptr, b.ptr, 2, 4, 16, 1, CL, CL, CL) == E_UNSUPPORTED          # a channels-last rem
    assert bn(a.ptr, c.ptr, sc.ptr, sh.ptr, b.ptr, 2, 4, 16, 1, CL, CL, PLANAR) == E_UNSUPPORTED
    assert bn(a.ptr, c.ptr, sc.ptr, sh.ptr, b.ptr, 2, 4, 16, 1, PLANAR, CL, CL) == E_UNSUPPORTED
    assert bn(a.ptr, None, sc.ptr, sh.ptr, b.ptr, 1, 65536, 1, 1, CL, PLANAR, PLANAR) == E_UNSUPPORTED
    assert bn(a.ptr, None, sc.ptr, sh.ptr, b.ptr, 1, 65536, 1, 1, CL, PLANAR, CL) == E_UNSUPPORTED
    cv = lambda *args: rc(api, "ganet_cost_volume_forward_cl", *args, st)    # noqa: E731
    good = [a.ptr, b.ptr, c.ptr, 1, 1, 2, 2, 8]
    assert cv(*good) == 0
    for i in (0, 1, 2):
        bad = list(good)
        bad[i] = None
        assert cv(*bad) == E_INVALID
    for i in (3, 4, 5, 6, 7):
        for v in (0, -1):
            bad = list(good)
            bad[i] = v
            assert cv(*bad) == E_INVALID
    assert cv(a.ptr, b.ptr, a.ptr, 1, 1, 2, 2, 8) == E_INVALID
    assert cv(a.ptr, b.ptr, b.ptr, 1, 1, 2, 2, 8) == E_INVALID
    dev.sync()


# ---- numpy models of the kernels' index maps (tests/test_cl_cpu.py holds them to the statement and to wrong variants) ------------

def model_transpose(x_img, N, C, S, src_cl, tile=CL_T, cb=CL_CB, edge=0):
    """the tile walk of cl_bn_transpose on an identity op: the image of one layout -> the image of the other.  edge: the tile
    width is taken as min(tile, S - s0) + edge (an off-by-one tile edge must be rejected)"""
    src = np.asarray(x_img).ravel()
    dst = np.full(N * C * S, -1, dtype=src.dtype)
    cl_at = lambda n, s, c: (n * S + s) * C + c                              # noqa: E731
    pl_at = lambda n, s, c: (n * C + c) * S + s                              # noqa: E731
    for n in range(N):
        for s0 in range(0, S, tile):
            tw = min(tile, S - s0) + edge
            for c0 in range(0, C, cb):
                cw = min(cb, C - c0)
                for s in range(max(tw, 0)):
                    for c in range(cw):
                        if s0 + s >= S:
                            continue
                        a, b = cl_at(n, s0 + s, c0 + c), pl_at(n, s0 + s, c0 + c)
                        if src_cl:
                            dst[b] = src[a]
                        else:
                            dst[a] = src[b]
    return dst


def model_cost_volume(x, y, Dn, swap=False, strict=False, tw=CV_TW, db=CV_DB, edge=0):
    """the tile walk of cost_volume_cl -> bit patterns [N,Dn,H,W,2C].  swap: the halves exchanged; strict: w > d in place of
    w >= d; edge: the y window starts `edge` columns off"""
    N, C, H, W = x.shape
    xb, yb = x.view(np.uint32), y.view(np.uint32)
    cost = np.full((N, Dn, H, W, 2 * C), 0xFFFFFFFF, dtype=np.uint32)
    for w0 in range(0, W, tw):
        twc = min(tw, W - w0)
        for d0 in range(0, Dn, db):
            dw = min(db, Dn - d0)
            yw0 = w0 - (d0 + dw - 1) + edge
            win = np.zeros((N, C, H, twc + dw - 1), dtype=np.uint32)
            for u in range(twc + dw - 1):
                if 0 <= yw0 + u < W:
                    win[..., u] = yb[..., yw0 + u]
            for d in range(d0, d0 + dw):
                for w in range(twc):
                    gw = w0 + w
                    on = gw > d if strict else gw >= d
                    xv = xb[:, :, :, gw] if on else 0
                    yv = win[:, :, :, gw - d - (w0 - (d0 + dw - 1))] if on else 0
                    lo, hi = (yv, xv) if swap else (xv, yv)
                    cost[:, d, :, gw, :C] = np.transpose(lo, (0, 2, 1)) if on else 0
                    cost[:, d, :, gw, C:] = np.transpose(hi, (0, 2, 1)) if on else 0
    return cost
