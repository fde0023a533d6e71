"""Kernel VALUES on the gfx950 build for tie-heavy and exactly representable inputs (tests/value_cases.py; the emulator runs the
same matrix in tests/test_sim_values.py), plus what only the device can run: the full model shapes, the autograd Functions,
power-of-two scaling into the fp32 subnormal range, and forward AND gradient digests of the reference at full size.
The device build differs from the emulator build exactly where the emulator cannot execute it (DPP / row_bcast reductions,
ds_read2_b32 planar staging, the packed-fma rows, the compiler's contraction of plain C++ sums): on the exact families none of
that may change a single element."""
import numpy as np
import pytest

import golden_util as gu
import parity_cases as pc
import value_cases as vc
from golden_util import load
from test_gpu_parity import TorchDev

pytestmark = pytest.mark.gpu

FAMILIES = ["select", "dyadic", "sparse"]


@pytest.fixture(scope="module")
def api():
    from ganet_amd import _native
    lib = _native.lib()
    assert not lib.is_simulator, "GPU tests must run the gfx950 build"
    assert lib.path.endswith("ganet_amd/libganet_hip.so")
    return lib


@pytest.fixture(scope="module")
def dev():
    return TorchDev()


# ---- SGA: the matrix of tests/test_sim_values.py ------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", vc.SGA_DEFAULT_SHAPES)
def test_sga_default_dispatch(api, dev, port_oracle, shape, family):
    vc.run_sga(api, dev, port_oracle, family, shape, per_dir=True)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("tiled", [0, 1])
@pytest.mark.parametrize("shape", vc.SGA_TILED_SHAPES)
def test_sga_tiled_workspace(api, dev, port_oracle, shape, tiled, family):
    N, C, D, H, W = shape
    with vc.option(api, "GANET_SGA_TILED", tiled):
        assert api.query("ganet_sga_workspace_layout", N, C, D, H, W) == tiled
        vc.run_sga(api, dev, port_oracle, family, shape, seed=vc.seed_of(shape, 1 + tiled), per_dir=True)


@pytest.mark.parametrize("family", FAMILIES)
def test_sga_row_kernels_depth_boundaries(api, dev, port_oracle, family):
    for D in vc.SGA_ROW_DEPTHS:
        vc.run_sga(api, dev, port_oracle, family, (1, 1, D, 2, 40), per_dir=True)
        vc.run_sga(api, dev, port_oracle, family, (1, 2, D, 3, 104), per_dir=False)


@pytest.mark.parametrize("family", FAMILIES)
def test_sga_deep_volume_segment_fallback(api, dev, port_oracle, family):
    vc.run_sga(api, dev, port_oracle, family, vc.SGA_SEGMENT_FALLBACK_SHAPE, per_dir=True)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("opt,value,restore,shapes", vc.SGA_FORCED, ids=[o[0] for o in vc.SGA_FORCED])
def test_sga_forced_kernel_families(api, dev, port_oracle, opt, value, restore, shapes, family):
    with vc.option(api, opt, value, restore):
        for shape in shapes:
            vc.run_sga(api, dev, port_oracle, family, shape, per_dir=True)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", vc.SGA_COMPAT_SHAPES)
def test_sga_reference_buffer_contract(api, dev, port_oracle, shape, family):
    x, gs, go, want = vc.sga_case(port_oracle, family, shape, seed=vc.seed_of(shape, 5))
    pc.check_sga_compat(api, dev, x, gs, go, want)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", vc.SGA_INFER_SHAPES)
def test_sga_forward_infer(api, dev, port_oracle, shape, family):
    vc.run_sga_infer(api, dev, port_oracle, family, shape, with_bn=False)


@pytest.mark.parametrize("family", ["select", "dyadic"])
@pytest.mark.parametrize("shape", vc.SGA_INFER_SHAPES)
def test_sga_forward_infer_bn_relu_epilogue(api, dev, port_oracle, shape, family):
    vc.run_sga_infer(api, dev, port_oracle, family, shape, with_bn=True)


# ---- SGA: the model shapes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", [(1, 32, 65, 80, 208), (1, 48, 33, 40, 104)])
def test_sga_model_shapes(api, dev, port_oracle, shape, family):
    """BASELINE configs[1]'s volume and the 1/6-resolution one: forward volumes / out / mask / arg-max bit-exact, gradients
    EQUAL to the oracle's for *select* (tie floors and exactness asserted at this size), within 1e-4 otherwise."""
    err = vc.run_sga(api, dev, port_oracle, family, shape, seed=123, per_dir=False)
    print("SGA", family, shape, "max-abs errors:", err)


def _sga_autograd(torch, x, gs, go):
    from ganet_amd.functions.GANet import SgaFunction
    xt = torch.from_numpy(x).cuda().requires_grad_()
    gt = [torch.from_numpy(g).cuda().requires_grad_() for g in gs]
    out = SgaFunction.apply(xt, *gt)
    grads = torch.autograd.grad(out, [xt] + gt, torch.from_numpy(go).cuda())
    torch.cuda.synchronize()
    return out.detach().cpu().numpy(), [g.cpu().numpy() for g in grads]


@pytest.mark.parametrize("save_mode", ["", "recompute"])
@pytest.mark.parametrize("shape", [(1, 4, 33, 8, 48), (2, 3, 65, 9, 20)])
def test_sga_function_autograd_on_select(dev, port_oracle, monkeypatch, shape, save_mode):
    """SgaFunction with saved volumes (default) and with GANET_SGA_SAVE=recompute (the reference's memory profile: float mask,
    volumes recomputed in backward): output and all five gradients equal the oracle's on the *select* family."""
    monkeypatch.setenv("GANET_SGA_SAVE", save_mode)
    x, gs, go, want = vc.sga_case(port_oracle, "select", shape)
    out, grads = _sga_autograd(dev.torch, x, gs, go)
    assert np.array_equal(out, want["out"])
    for k, g in zip(("gx", "gw0", "gw1", "gw2", "gw3"), grads):
        assert np.array_equal(g, want[k]), (k, int((g != want[k]).sum()))


# ---- LGA ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wave", [2, 1, 0])
@pytest.mark.parametrize("shape,r,passes", vc.LGA_CHAIN_CASES)
def test_lga_chain_equals_float64(api, dev, port_oracle, shape, r, passes, wave):
    with vc.option(api, "GANET_LGA_WAVE", wave, 2):
        vc.run_lga(api, dev, port_oracle, shape, r, passes)


@pytest.mark.parametrize("shape", vc.LGA_PAIRED_SHAPES)
def test_lga2_paired_chain_equals_float64(api, dev, port_oracle, shape):
    vc.run_lga(api, dev, port_oracle, shape, 2, 2, paired=True)


@pytest.mark.parametrize("mix,segs", vc.LGA_ITEM_LISTS)
@pytest.mark.parametrize("shape", vc.LGA_OPTION_SHAPES)
def test_lga_item_lists_equal_float64(api, dev, port_oracle, shape, mix, segs):
    try:
        api.set_option("GANET_LGA_MIX", mix)
        api.set_option("GANET_LGA_SEGS", segs)
        vc.run_lga(api, dev, port_oracle, shape, 2, 2)
        vc.run_lga(api, dev, port_oracle, shape, 2, 2, paired=True)
    finally:
        api.set_option("GANET_LGA_MIX", 1)
        api.set_option("GANET_LGA_SEGS", 0)


LGA_BIG = [((1, 193, 240, 624), True), ((1, 33, 17, 36), False)]      # cfg2's volume; W % 4 == 0 with an odd height


@pytest.fixture(scope="module")
def lga_big_cases(port_oracle):
    """the exact family at the two device shapes, with the oracle's results (computed once: the full size takes a while)"""
    return {shape: vc.lga_case(port_oracle, shape, 2, 2, seed=123, big=big) for shape, big in LGA_BIG}


@pytest.mark.parametrize("shape", [s for s, _ in LGA_BIG])
def test_lga2_model_shape_equals_oracle_in_every_kernel_family(api, dev, lga_big_cases, shape):
    """two chained passes, radius 2: one-pass entries on the API layout with the plane-pair kernels on workgroup rings (2),
    on one-wave rings (1) and with the tile kernels (0), then the pair-interleaved chain with and without edge sums -- y, gX
    and gF equal the oracle's in every element (which equals float64 on the small cases and the reference at this size)."""
    x, f, gy, want = lga_big_cases[shape]
    for wave in (2, 1, 0):
        with vc.option(api, "GANET_LGA_WAVE", wave, 2):
            got = {}
            pc.check_lga_chain(api, dev, x, f, gy, 2, 2, want, out=got)
            vc.assert_lga_equal(got, want)
    got = {}
    pc.check_lga2_paired(api, dev, x, f, gy, 2, 2, want, out=got)
    vc.assert_lga_equal(got, want)


@pytest.mark.parametrize("paired", ["1", "0"])
@pytest.mark.parametrize("shape", [s for s, _ in LGA_BIG])
def test_lga2_function_autograd_equals_oracle(dev, lga_big_cases, monkeypatch, shape, paired):
    """Lga2Function through autograd, with its pair-interleaved private intermediate and with GANET_LGA_PAIRED=0"""
    torch = dev.torch
    from ganet_amd.functions.GANet import Lga2Function
    monkeypatch.setenv("GANET_LGA_PAIRED", paired)
    x, f, gy, want = lga_big_cases[shape]
    xt, ft = torch.from_numpy(x).cuda().requires_grad_(), torch.from_numpy(f).cuda().requires_grad_()
    y = Lga2Function.apply(xt, ft, 2)
    gx, gf = torch.autograd.grad(y, [xt, ft], torch.from_numpy(gy).cuda())
    torch.cuda.synchronize()
    vc.assert_lga_equal({"y": y.detach().cpu().numpy(), "gx": gx.cpu().numpy(), "gf": gf.cpu().numpy()}, want)


# ---- power-of-two scaling on the exact families -----------------------------------------------------------------------------
# Scaling by a power of two changes exponents only: every product and sum stays exactly representable as long as nothing
# overflows or falls off the subnormal grid (multiples of 2^-149).  2^-125 puts LGA's products (|x| 2^-125 * |f| >= 2^-3) and
# the first partial sums of every element into the fp32 SUBNORMAL range (most results end up normal again); 2^-130 makes the
# inputs themselves and most results subnormal as well (grids down to 2^-139: still on the 2^-149 grid).  The oracle does not
# flush subnormals, nor does the reference's CUDA build.  Only one of (x, gy) is scaled down at a time: the filter gradient
# is their product.
@pytest.mark.parametrize("sx,sg", [(2.0 ** 40, 2.0 ** 40), (2.0 ** -125, 1.0), (1.0, 2.0 ** -125), (2.0 ** -130, 1.0), (1.0, 2.0 ** -130)],
                         ids=["2^40", "x*2^-125", "gy*2^-125", "x*2^-130", "gy*2^-130"])
@pytest.mark.parametrize("shape,r,passes", [((1, 33, 17, 36), 2, 2), ((2, 9, 7, 13), 2, 2), ((1, 12, 19, 33), 3, 1), ((1, 7, 16, 36), 1, 3)])
def test_lga_power_of_two_scaling(api, dev, port_oracle, shape, r, passes, sx, sg):
    x, f, gy, want1 = vc.lga_case(port_oracle, shape, r, passes)
    xs, gs_ = (x * np.float32(sx)).astype(np.float32), (gy * np.float32(sg)).astype(np.float32)
    y, ins = port_oracle.lga_chain_forward(xs, f, r, passes)
    gx, gf = port_oracle.lga_chain_backward(ins, f, gs_, r)
    want = {"y": y, "gx": gx, "gf": gf}
    # the oracle itself scales exactly (float64 products of fp32 numbers and powers of two are exact)
    for k, s in (("y", sx), ("gx", sg), ("gf", sx * sg)):
        assert np.array_equal(want[k].astype(np.float64), want1[k].astype(np.float64) * s), k
    if min(sx, sg) < 1:
        tiny, small = np.float32(2.0 ** -126), (xs if sx < 1 else gs_)
        assert np.abs(f[f != 0]).min() * np.abs(small[small != 0]).min() < tiny, "subnormal products expected"
        if min(sx, sg) < 2.0 ** -126:
            res = want["y"] if sx < 1 else want["gx"]
            assert ((np.abs(res) < tiny) & (res != 0)).mean() > 0.3, "subnormal results expected"
    for wave in (2, 0):
        with vc.option(api, "GANET_LGA_WAVE", wave, 2):
            got = {}
            # (the 1e-4 bar inside check_lga_chain is absolute; equality is what is asserted here)
            pc.check_lga_chain(api, dev, xs, f, gs_, r, passes, None, out=got)
            vc.assert_lga_equal(got, want)
    if r == 2 and passes == 2 and shape[-1] % 2 == 0:
        got = {}
        pc.check_lga2_paired(api, dev, xs, f, gs_, 2, 2, None, out=got)
        vc.assert_lga_equal(got, want)


@pytest.mark.parametrize("sx,sg", [(2.0 ** 40, 2.0 ** 40), (2.0 ** -125, 1.0)], ids=["2^40", "x*2^-125"])
@pytest.mark.parametrize("family", ["select", "dyadic"])
@pytest.mark.parametrize("shape", [(1, 2, 33, 8, 32), (1, 1, 65, 5, 20)])
def test_sga_power_of_two_scaling(api, dev, port_oracle, shape, family, sx, sg):
    """*select*: volumes are copies of x and gradients integers times the scales -- equality at either scale.  *dyadic*: the
    weights (1/4 .. 1) push x * 2^-125 below 2^-126 along the scanline: forward volumes, out, mask and arg-max stay bit-exact
    against the oracle only if the kernels keep subnormals as the oracle does (gradients: compared after scaling back)."""
    x, gs, go = pc.SGA_FAMILIES[family](shape, vc.seed_of(shape))
    xs, gos = (x * np.float32(sx)).astype(np.float32), (go * np.float32(sg)).astype(np.float32)
    want = pc.oracle_sga_want(port_oracle, xs, gs, gos)
    pc.assert_sga_ties(family, [want[f"A{d}"] for d in range(4)])
    if family == "dyadic" and sx < 1:
        assert ((np.abs(want["A0"]) < np.float32(2.0 ** -126)) & (want["A0"] != 0)).mean() > 0.05, "subnormal volumes expected"
    dx, dg, A, out, mask, kp = pc.run_sga_forward(api, dev, xs, gs)
    hA = dev.host(A)
    for d in range(4):
        assert np.array_equal(hA[d], want[f"A{d}"]), f"A{d}"
    assert np.array_equal(dev.host(out), want["out"]) and np.array_equal(dev.host(mask), want["mask"])
    assert np.array_equal(dev.host(kp).astype(np.int64), np.argmax(hA, axis=3))
    got = pc.run_sga_backward_only(api, dev, xs, gs, gos)
    for k, s in (("gx", sg), ("gw0", sx * sg), ("gw1", sx * sg), ("gw2", sx * sg), ("gw3", sx * sg)):
        if family == "select":
            assert np.array_equal(got[k], want[k]), k
        else:
            assert np.abs(got[k].astype(np.float64) / s - want[k].astype(np.float64) / s).max() <= pc.TOL, k


# ---- the reference's fixtures and full-size digests -------------------------------------------------------------------------
@pytest.mark.parametrize("name", gu.values_sga_case_names())
def test_sga_value_fixtures(api, dev, name):
    z = gu.load_values_sga(name)
    gs = [z[f"{name}.g{d}"] for d in range(4)]
    want = {k: z[f"{name}.{k}"] for k in ("out", "mask", "tmp", "gx")}
    for d in range(4):
        want[f"A{d}"], want[f"gw{d}"] = z[f"{name}.A{d}"], z[f"{name}.gw{d}"]
    res = {}
    pc.check_sga_forward_backward(api, dev, z[f"{name}.x"], gs, z[f"{name}.go"], want, results=res)
    if name.startswith("select"):
        for k, v in res.items():
            assert np.array_equal(v, want[k]), k
    pc.check_sga_compat(api, dev, z[f"{name}.x"], gs, z[f"{name}.go"], want)


@pytest.mark.parametrize("name", [c[0] for c in gu.VALUES_LGA_CASES])
def test_lga_value_fixtures(api, dev, name):
    z = load("lga_values_golden.npz")
    r, passes = (int(v) for v in z[f"{name}.meta"])
    want = {k: z[f"{name}.{k}"] for k in ("y", "gx", "gf")}
    got = {}
    pc.check_lga_chain(api, dev, z[f"{name}.x"], z[f"{name}.f"], z[f"{name}.gy"], r, passes, want, out=got)
    vc.assert_lga_equal(got, want)


def test_sga_select_full_size_forward_and_gradients_match_reference_digests(api, dev):
    """[1,32,65,80,208], *select*: out, mask, the four volumes AND the five gradients hashed on the host equal the sha256 of
    what the REFERENCE's kernel bodies gave (tests/golden/digests.json: sga_cfg2_select; -0 hashed as +0).  The results do
    not depend on the order of the sums here, so this holds for gradients too -- no oracle, no tolerance."""
    name, shape, seed = gu.SGA_SELECT_DIGEST
    want = gu.load_digests()[name]["sha256"]
    x, gs, go = pc.sga_inputs_select(shape, seed)
    assert gu.sha(x) == want["in.x"] and gu.sha(go) == want["in.go"] and all(gu.sha(gs[k]) == want[f"in.g{k}"] for k in range(4))
    _, _, A, out, mask, _ = pc.run_sga_forward(api, dev, x, gs)
    hA = dev.host(A)
    c = gu.canon_zero
    got = {"out": gu.sha(c(dev.host(out))), "mask_u8": gu.sha(dev.host(mask)), "temp_out": gu.sha(c(hA[3])),
           **{f"A{k}": gu.sha(c(hA[k])) for k in range(4)}}
    del A, out, mask, hA
    got.update({k: gu.sha(c(v)) for k, v in pc.run_sga_backward_only(api, dev, x, gs, go).items()})
    assert set(got) == set(k for k in want if not k.startswith("in."))
    assert got == {k: want[k] for k in got}, [k for k in got if got[k] != want[k]]


def test_lga2_exact_full_size_forward_and_gradients_match_reference_digests(api, dev):
    """[1,193,240,624], the exact family through the one-pass entries: intermediate, output, data and filter gradients"""
    name, shape, seed = gu.LGA_EXACT_DIGEST
    want = gu.load_digests()[name]["sha256"]
    x, f, gy = pc.lga_inputs_exact(shape, 2, seed)
    assert gu.sha(x) == want["in.x"] and gu.sha(f) == want["in.f"] and gu.sha(gy) == want["in.gy"]
    B, D, H, W = shape
    dx, df = dev.to(x), dev.to(f)
    t1 = dev.empty(shape)
    api.call("ganet_lga_forward", dev.ptr(dx), dev.ptr(df), dev.ptr(t1), B, D, H, W, 2, dev.stream)
    dev.sync()
    out = {}
    pc.check_lga_chain(api, dev, x, f, gy, 2, 2, None, out=out)
    c = gu.canon_zero
    got = {"t1": gu.sha(c(dev.host(t1))), **{k: gu.sha(c(out[k])) for k in ("y", "gx", "gf")}}
    assert got == {k: want[k] for k in got}, [k for k in got if got[k] != want[k]]
