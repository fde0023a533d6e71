"""The value-family cases shared by tests/test_sim_values.py (emulator build, numpy buffers) and tests/test_gpu_values.py
(gfx950 build, device buffers): tie-heavy and exactly representable inputs (parity_cases.sga_inputs_select / _dyadic /
_sparse, lga_inputs_exact) through the parity checks, with the tie floors and exactness conditions asserted on the
oracle / the float64 reference BEFORE any kernel is compared.

Equality below is IEEE equality of every element (np.array_equal: a NaN fails it, +0 and -0 compare equal -- the sign of
a zero sum depends on which zero product a kernel starts from and carries no information)."""
import contextlib

import numpy as np

import lga_ref64
import parity_cases as pc

# ---- SGA ------------------------------------------------------------------------------------------------------------------
# default dispatch, shapes that reach the fast kernels: H*W % 4 == 0 (four-pixel merge), W % 16 == 0 and H % 4 == 0 (tiled
# adjoint workspace), partial column blocks (W % 16 != 0), several row batches (H > 4, H % 4 != 0), and the scalar merge (35 px)
# (the tiled shapes run under both settings of GANET_SGA_TILED, the default among them)
SGA_DEFAULT_SHAPES = [(2, 1, 20, 9, 20), (1, 1, 9, 6, 14), (1, 2, 6, 5, 7)]
SGA_TILED_SHAPES = [(1, 1, 33, 8, 32), (1, 1, 65, 4, 48)]
SGA_ROW_DEPTHS = [39, 40, 41, 48, 49, 64, 65, 72, 73]                 # boundaries of the row kernels' depth dispatch
SGA_SEGMENT_FALLBACK_SHAPE = (1, 1, 240, 4, 12)                       # D in (208, 272]
# forced kernel families: (option, value, value to restore, shapes)
SGA_FORCED = [
    ("GANET_SGA_ROWWAVE", 0, 1, [(1, 1, 65, 4, 48), (1, 2, 33, 3, 20)]),
    ("GANET_SGA_COLBLOCK", 0, 1, [(2, 1, 20, 9, 20), (1, 1, 65, 5, 20)]),
    ("GANET_SGA_WIDE_COL", 2, 1, [(1, 1, 100, 5, 20), (1, 1, 65, 7, 12)]),
    ("GANET_SGA_WIDE_SCAN", 2, 1, [(1, 1, 65, 5, 12), (1, 1, 300, 3, 12)]),          # the second: D > 272
]
SGA_COMPAT_SHAPES = [(1, 2, 33, 8, 32), (1, 1, 49, 5, 7)]
SGA_INFER_SHAPES = [(1, 3, 33, 4, 12), (2, 2, 9, 5, 7)]               # slice % 4 == 0 (16-byte path) and not


def seed_of(shape, extra=0):
    return sum(shape) + extra


@contextlib.contextmanager
def option(api, name, value, restore=None):
    was = api.get_option(name) if restore is None else restore
    api.set_option(name, value)
    try:
        yield
    finally:
        api.set_option(name, was)


def sga_case(oracle, family, shape, seed=None):
    """inputs of the family, what the oracle makes of them, and the family's conditions asserted on that"""
    x, gs, go = pc.SGA_FAMILIES[family](shape, seed_of(shape) if seed is None else seed)
    want = pc.oracle_sga_want(oracle, x, gs, go)
    pc.assert_sga_ties(family, [want[f"A{d}"] for d in range(4)])
    if family == "select":
        pc.assert_select_exact(x, gs, go)
        for k in ("gx", "gw0", "gw1", "gw2", "gw3"):
            assert np.array_equal(want[k], np.round(want[k])), k
    return x, gs, go, want


def run_sga(api, dev, oracle, family, shape, seed=None, per_dir=None, compat=False):
    """Forward volumes, out, mask, arg-max bit-exact (check_sga_forward_backward); gradients EQUAL to the oracle's for
    *select*, within parity_cases.TOL otherwise.  per_dir (the cross-check of the per-direction and step entry points, which
    triples the work): by default for *select* only -- the emulator's time; the device tests ask for it everywhere."""
    x, gs, go, want = sga_case(oracle, family, shape, seed)
    per_dir = family == "select" if per_dir is None else per_dir
    res = {}
    err = pc.check_sga_forward_backward(api, dev, x, gs, go, want, per_dir=per_dir, results=res)
    if family == "select":
        for k, v in res.items():
            assert np.array_equal(v, want[k]), (k, int((v != want[k]).sum()), float(np.abs(v - want[k]).max()))
    if compat:
        pc.check_sga_compat(api, dev, x, gs, go, want)
    return err


def bn_relu_exact(v, scale, shift):
    """relu(fma(v, scale[c], shift[c])) in fp32, by float64: the product of two fp32 numbers is exact there, and the sum is
    checked to be (its TwoSum error term is zero), so that the conversion to fp32 is the fma's single rounding."""
    C = scale.size
    p = v.astype(np.float64) * scale.astype(np.float64).reshape(1, C, 1, 1, 1)
    t = np.broadcast_to(shift.astype(np.float64).reshape(1, C, 1, 1, 1), p.shape)
    s = p + t
    bb = s - p
    assert not ((p - (s - bb)) + (t - bb)).any(), "the float64 sum is not exact for these values"
    return np.maximum(s, 0).astype(np.float32)


def check_sga_infer(api, dev, x, gs, want_out, with_bn):
    """ganet_sga_forward_infer (running maximum, no mask): `out` equal to want_out, through the folded BN + ReLU epilogue
    (dyadic scale / shift) as well."""
    shape = x.shape
    N, C, D, H, W = shape
    scale = np.array([0.5, 1.5, -0.75, 2.0], np.float32)[:C]
    shift = np.array([0.25, -1.0, 0.5, -0.125], np.float32)[:C]
    dx, dg = dev.to(x), [dev.to(g) for g in gs]
    A, out = dev.empty((4,) + shape), dev.empty(shape)
    ds, dt = dev.to(scale), dev.to(shift)
    api.call("ganet_sga_forward_infer", dev.ptr(dx), *[dev.ptr(g) for g in dg], dev.ptr(A), dev.ptr(out),
             dev.ptr(ds) if with_bn else None, dev.ptr(dt) if with_bn else None, N, C, D, H, W, dev.stream)
    dev.sync()
    exp = bn_relu_exact(want_out, scale, shift) if with_bn else want_out
    got = dev.host(out)
    assert np.array_equal(got, exp), (int((got != exp).sum()), float(np.abs(got - exp).max()))


def run_sga_infer(api, dev, oracle, family, shape, with_bn):
    """check_sga_infer on the family's inputs with the oracle's `out`"""
    x, gs, go, want = sga_case(oracle, family, shape)
    check_sga_infer(api, dev, x, gs, want["out"], with_bn)


# ---- LGA ------------------------------------------------------------------------------------------------------------------
# (shape, radius, passes): r = 1, 2, 3; one to three passes; W % 4 == 0 and not; odd and even D; 5-D
LGA_CHAIN_CASES = [((1, 9, 7, 12), 2, 2), ((1, 7, 16, 36), 1, 3), ((1, 12, 19, 33), 3, 1), ((2, 6, 5, 34), 2, 3),
                   ((1, 8, 6, 13), 2, 1), ((2, 3, 9, 5, 8), 2, 2), ((1, 5, 4, 9), 1, 2), ((1, 4, 5, 40), 3, 2)]
LGA_PAIRED_SHAPES = [(1, 9, 7, 12), (2, 7, 9, 40), (1, 12, 5, 34), (2, 3, 9, 5, 8)]          # radius 2, two passes, even W
LGA_OPTION_SHAPES = [(1, 33, 7, 36), (2, 9, 3, 64)]                                          # radius 2
LGA_ITEM_LISTS = [(0, 0), (1, 0), (0, 2)]             # (GANET_LGA_MIX, GANET_LGA_SEGS): whole tiles, mixed list, depth segments


def lga_case(oracle, shape, r, passes, seed=None, big=False):
    """-> x, f, gy, want (fp32, equal to the float64 reference: asserted), after the exactness condition.  `big`: the volume
    is too large for the float64 chain -- the condition from norms, and the oracle alone as `want` (it is held to float64 on
    the small cases and to the reference by the digest of this case)."""
    x, f, gy = pc.lga_inputs_exact(shape, r, seed_of(shape, r) if seed is None else seed)
    y, ins = oracle.lga_chain_forward(x, f, r, passes)
    gx, gf = oracle.lga_chain_backward(ins, f, gy, r)
    want = {"y": y, "gx": gx, "gf": gf}
    if big:
        lga_ref64.assert_lga_exact_by_norms(x, f, gy, r, passes)
    else:
        w64 = lga_ref64.assert_lga_exact(x, f, gy, r, passes)
        for k in want:
            assert np.array_equal(want[k].astype(np.float64), w64[k]), f"oracle differs from the float64 reference: {k}"
    return x, f, gy, want


def assert_lga_equal(got, want):
    for k in ("y", "gx", "gf"):
        assert np.array_equal(got[k], want[k]), (k, int((got[k] != want[k]).sum()), float(np.abs(got[k] - want[k]).max()))


def run_lga(api, dev, oracle, shape, r, passes, paired=False, seed=None, big=False):
    x, f, gy, want = lga_case(oracle, shape, r, passes, seed, big)
    got = {}
    (pc.check_lga2_paired if paired else pc.check_lga_chain)(api, dev, x, f, gy, r, passes, want, out=got)
    assert_lga_equal(got, want)
