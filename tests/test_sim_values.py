"""Kernel VALUES on the CPU emulator (tests/hipsim) for inputs where the tie rules decide the result and, for two families,
where equality with the oracle is available (tests/value_cases.py; the same matrix runs on the gfx950 build in
tests/test_gpu_values.py).  SGA's results depend on two tie rules of the reference -- the direction merge keeps the LOWEST
direction among equal maxima, the best previous disparity is the FIRST arg-max over depth -- which continuous random inputs
practically never exercise: with the *select* / *dyadic* / *sparse* families a large share of all elements and pixels tie
(floors asserted per case).  The LGA family is exactly representable throughout: y, gX, gF equal a float64 evaluation."""
import numpy as np
import pytest

import lga_ref64
import parity_cases as pc
import value_cases as vc
import golden_util as gu
from golden_util import load

FAMILIES = ["select", "dyadic", "sparse"]
DEV = pc.NumpyDev()


@pytest.fixture(scope="module")
def sim():
    from sim_util import sim_api
    return sim_api()


# ---- the float64 reference itself, and the oracle against it (no kernel involved) -----------------------------------------
def test_float64_lga_reference_is_what_its_definition_says():
    """the vectorised float64 statement against the literal triple loop over taps and positions, on a tiny volume"""
    rng = np.random.default_rng(5)
    B, D, H, W, r = 2, 3, 4, 5, 1
    x, f = rng.standard_normal((B, D, H, W)), rng.standard_normal((B, 27, H, W))
    y = np.zeros((B, D, H, W))
    for b in range(B):
        for d in range(D):
            for i in range(H):
                for j in range(W):
                    for dd in (-1, 0, 1):
                        for a in range(-r, r + 1):
                            for c in range(-r, r + 1):
                                t = (dd + 1) * 9 + (a + r) * 3 + (c + r)
                                ok = 0 <= d + dd < D and 0 <= i + a < H and 0 <= j + c < W
                                y[b, d, i, j] += f[b, t, i, j] * (x[b, d + dd, i + a, j + c] if ok else x[b, d, i, j])
    assert np.abs(lga_ref64.lga_forward(x, f, r) - y).max() < 1e-13
    gy = rng.standard_normal(y.shape)
    gx, gf = lga_ref64.lga_backward(x, f, gy, r)                  # adjoints: <y, gy> == <x, gx> == <f, gf> (bilinear)
    assert abs((y * gy).sum() - (x * gx).sum()) < 1e-11 and abs((y * gy).sum() - (f * gf).sum()) < 1e-11
    x2, f2 = rng.standard_normal(x.shape), rng.standard_normal(f.shape)          # ... and against other arguments
    assert abs((lga_ref64.lga_forward(x2, f, r) * gy).sum() - (x2 * gx).sum()) < 1e-11
    assert abs((lga_ref64.lga_forward(x, f2, r) * gy).sum() - (f2 * gf).sum()) < 1e-11


@pytest.mark.parametrize("shape,r,passes", vc.LGA_CHAIN_CASES + [((1, 33, 9, 20), 2, 2), ((1, 4, 3, 3), 2, 3), ((2, 2, 1, 1, 4), 1, 1)])
def test_oracle_equals_float64_reference_on_the_exact_family(port_oracle, shape, r, passes):
    """The C oracle descends from the reference's code; lga_ref64 does not.  On the exact family every result is
    representable, so the two must agree in every element: forward of the chained passes, data and filter gradients,
    4-D and 5-D, r = 1, 2, 3.  (vc.lga_case asserts the exactness condition and the equality.)"""
    x, f, gy, want = vc.lga_case(port_oracle, shape, r, passes)
    w64 = lga_ref64.lga_chain(x, f, gy, r, passes)
    _, ins = port_oracle.lga_chain_forward(x, f, r, passes)
    for a, b in zip(ins, w64["ins"]):
        assert np.array_equal(a.astype(np.float64), b)
    assert np.abs(want["y"]).max() > 1 and np.abs(want["gf"]).max() > 1


# ---- SGA ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", vc.SGA_DEFAULT_SHAPES)
def test_sga_default_dispatch(sim, port_oracle, shape, family):
    vc.run_sga(sim, DEV, port_oracle, family, shape)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("tiled", [0, 1])
@pytest.mark.parametrize("shape", vc.SGA_TILED_SHAPES)
def test_sga_tiled_workspace(sim, port_oracle, shape, tiled, family):
    N, C, D, H, W = shape
    with vc.option(sim, "GANET_SGA_TILED", tiled):
        assert sim.query("ganet_sga_workspace_layout", N, C, D, H, W) == tiled
        vc.run_sga(sim, DEV, port_oracle, family, shape, seed=vc.seed_of(shape, 1 + tiled))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("D", vc.SGA_ROW_DEPTHS)
def test_sga_row_kernels_depth_boundaries(sim, port_oracle, D, family):
    vc.run_sga(sim, DEV, port_oracle, family, (1, 1, D, 2, 40))


@pytest.mark.parametrize("family", FAMILIES)
def test_sga_deep_volume_segment_fallback(sim, port_oracle, family):
    vc.run_sga(sim, DEV, port_oracle, family, vc.SGA_SEGMENT_FALLBACK_SHAPE, per_dir=False)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("opt,value,restore,shapes", vc.SGA_FORCED, ids=[o[0] for o in vc.SGA_FORCED])
def test_sga_forced_kernel_families(sim, port_oracle, opt, value, restore, shapes, family):
    with vc.option(sim, opt, value, restore):
        for shape in shapes:
            vc.run_sga(sim, DEV, port_oracle, family, shape, per_dir=family == "select" and shape[2] < 100)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", vc.SGA_COMPAT_SHAPES)
def test_sga_reference_buffer_contract(sim, port_oracle, shape, family):
    """float mask, sga_argmax_px, the running merge (ganet_sga_forward_compat / _backward_compat)"""
    x, gs, go, want = vc.sga_case(port_oracle, family, shape, seed=vc.seed_of(shape, 5))
    pc.check_sga_compat(sim, DEV, x, gs, go, want)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", vc.SGA_INFER_SHAPES)
def test_sga_forward_infer(sim, port_oracle, shape, family):
    vc.run_sga_infer(sim, DEV, port_oracle, family, shape, with_bn=False)


@pytest.mark.parametrize("family", ["select", "dyadic"])     # (dyadic values: the float64 restatement of the fma is exact)
@pytest.mark.parametrize("shape", vc.SGA_INFER_SHAPES)
def test_sga_forward_infer_bn_relu_epilogue(sim, port_oracle, shape, family):
    vc.run_sga_infer(sim, DEV, port_oracle, family, shape, with_bn=True)


# ---- LGA ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wave", [2, 1, 0])
@pytest.mark.parametrize("shape,r,passes", vc.LGA_CHAIN_CASES)
def test_lga_chain_equals_float64(sim, port_oracle, shape, r, passes, wave):
    with vc.option(sim, "GANET_LGA_WAVE", wave, 2):
        vc.run_lga(sim, DEV, port_oracle, shape, r, passes)


@pytest.mark.parametrize("shape", vc.LGA_PAIRED_SHAPES)
def test_lga2_paired_chain_equals_float64(sim, port_oracle, shape):
    """the pair-interleaved private intermediate of Lga2Function, with and without the edge sums (check_lga2_paired runs both)"""
    vc.run_lga(sim, DEV, port_oracle, shape, 2, 2, paired=True)


@pytest.mark.parametrize("mix,segs", vc.LGA_ITEM_LISTS)
@pytest.mark.parametrize("shape", vc.LGA_OPTION_SHAPES)
def test_lga_item_lists_equal_float64(sim, port_oracle, shape, mix, segs):
    try:
        sim.set_option("GANET_LGA_MIX", mix)
        sim.set_option("GANET_LGA_SEGS", segs)
        vc.run_lga(sim, DEV, port_oracle, shape, 2, 2)
        vc.run_lga(sim, DEV, port_oracle, shape, 2, 2, paired=True)
    finally:
        sim.set_option("GANET_LGA_MIX", 1)
        sim.set_option("GANET_LGA_SEGS", 0)


# ---- the fixtures made from the reference's own kernel bodies (tests/golden/make_golden.py --values) ------------------------
def _golden_sga(name):
    z = gu.load_values_sga(name)
    gs = [z[f"{name}.g{d}"] for d in range(4)]
    want = {k: z[f"{name}.{k}"] for k in ("out", "mask", "tmp", "gx")}
    for d in range(4):
        want[f"A{d}"], want[f"gw{d}"] = z[f"{name}.A{d}"], z[f"{name}.gw{d}"]
    return z[f"{name}.x"], gs, z[f"{name}.go"], want


@pytest.mark.parametrize("name", gu.values_sga_case_names())
def test_sga_value_fixtures(sim, name):
    x, gs, go, want = _golden_sga(name)
    res = {}
    pc.check_sga_forward_backward(sim, DEV, x, gs, go, want, results=res)
    if name.startswith("select"):
        for k, v in res.items():
            assert np.array_equal(v, want[k]), k
    pc.check_sga_compat(sim, DEV, x, gs, go, want)


@pytest.mark.parametrize("name", [c[0] for c in gu.VALUES_LGA_CASES])
def test_lga_value_fixtures(sim, name):
    z = load("lga_values_golden.npz")
    r, passes = (int(v) for v in z[f"{name}.meta"])
    want = {k: z[f"{name}.{k}"] for k in ("y", "gx", "gf")}
    got = {}
    pc.check_lga_chain(sim, DEV, z[f"{name}.x"], z[f"{name}.f"], z[f"{name}.gy"], r, passes, want, out=got)
    vc.assert_lga_equal(got, want)
