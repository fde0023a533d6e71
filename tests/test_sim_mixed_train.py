"""The mixed-precision training kernels (ganet_amd/csrc/bn_kernels.h, mixed_train_kernels.h, l1norm_bwd<KT, Tx>) on the CPU emulator build: the
case table of tests/mixed_train_cases.py (tests/test_gpu_mixed_train.py runs the same table on the device), every buffer at a
guard page -- ENDING at one, resp. BEGINNING right behind one -- and every output pre-filled with a NaN pattern.  What is checked
and why is in the table's docstring; the first tests hold the table to what it claims."""
import os
import re

import numpy as np
import pytest

import bn_cases as bc
import mixed_cases as mc
import mixed_train_cases as mt
import parity_cases as pc

FMTS = [mc.F16, mc.BF16]
fmt_id = mc.FMT_NAME.get
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = ("trip2-vec", "trip2-scalar")                       # run at one guard side: the loops come round, the bases are the same
SMALL = [c for c in mt.BN_TRAIN_CASES if not c.name.startswith(BIG)]


@pytest.fixture(scope="module")
def sim():
    from sim_util import sim_api
    return sim_api()


@pytest.fixture(params=["end", "start"])
def dev(request):
    return pc.NumpyDev(request.param)


def tier(cases, t):
    return [c for c in cases if c.tier == t]


# ---- the table ------------------------------------------------------------------------------------------------------------------

def test_case_table_reaches_what_it_claims():
    src = "".join(open(os.path.join(ROOT, "ganet_amd", "csrc", f)).read() for f in ("bn_kernels.h", "mixed_kernels.h", "ganet_capi.hip"))
    k = {n: int(v) for n, v in re.findall(r"constexpr int (BN_BLOCK|BN_MAX_ROWS|BN_TARGET_BLOCKS|MX_V) = (\d+);", src)}
    assert (k["BN_BLOCK"], k["BN_MAX_ROWS"], k["BN_TARGET_BLOCKS"], k["MX_V"]) == (mc.BN_BLOCK, mc.BN_MAX_ROWS, mc.BN_TARGET_BLOCKS, mc.MX_V)
    assert "int ew_grid(i64 n) { return clamp_grid(n, 256, 256 * 16); }" in src and mt.EW_GRID_LANES == 256 * 256 * 16
    by = mt.BN_BY_NAME
    N, C, S = by["trip2-vec-exact"].shape
    assert mc.BN_TARGET_BLOCKS // C >= mc.BN_MAX_ROWS and S % mc.MX_V == 0 and N == 2
    assert S // mc.MX_V == mc.BN_MAX_ROWS * mc.BN_BLOCK + 1                    # one group beyond a full trip of every lane
    assert by["trip2-scalar-exact"].shape[2] == mc.BN_MAX_ROWS * mc.BN_BLOCK + 1
    assert by["channels-2x70x8-exact"].shape[1] == 70 and mc.BN_TARGET_BLOCKS // 70 < mc.BN_MAX_ROWS
    assert {c.shape[2] % 8 for c in mt.BN_TRAIN_CASES} >= {0, 2, 4, 3, 1}
    assert any(c.off for c in mt.BN_TRAIN_CASES) and any(c.shape[0] > c.shape[1] for c in mt.BN_TRAIN_CASES)
    assert any(c.shape[0] * c.shape[2] == 2 for c in mt.BN_TRAIN_CASES)
    for name in mt.REPRODUCIBLE + mt.WANTED_CASES:
        assert name in by
    cv = {c.name: c for c in mt.CV_BWD_CASES}
    assert all(c in mt.CV_BWD_CASES for c in mc.CV_CASES)
    assert any(c.Dn > c.shape[3] for c in mt.CV_BWD_CASES) and any(c.Dn % 8 for c in mt.CV_BWD_CASES) and any(c.Dn % 8 == 0 for c in mt.CV_BWD_CASES)
    assert any(c.shape[3] % 8 for c in mt.CV_BWD_CASES) and any(c.off for c in mt.CV_BWD_CASES)
    for name, v in (("trip2-vector", 8), ("trip2-scalar", 1)):
        n = int(np.prod(cv[name].shape))
        assert (cv[name].shape[3] % 8 == 0) == (v == 8) and mt.EW_GRID_LANES < n // v <= mt.EW_GRID_LANES + cv[name].shape[3]
    assert {c.dims[3] for c in mt.L1_BWD_CASES} >= {5, 75, 27, 7}


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
def test_exact_tier_is_exact_and_general_tier_is_decided(fmt):
    """in integer arithmetic, for every exact case, site and ReLU setting; and no general case is left on the ReLU's kink"""
    for case in mt.BN_TRAIN_CASES:
        for site in case.sites:
            for relu in case.relus:
                c = case.data(fmt, site, relu)
                assert np.array_equal(mc.up(mc.convert(c.x, fmt), fmt).ravel()[~np.isnan(c.x.ravel())], c.x.ravel()[~np.isnan(c.x.ravel())])
                if case.tier == "exact":
                    mt.assert_exact(c)
                elif case.tier == "general" and case.compare_grads and relu:
                    assert not c.ref.undecided().any(), (case.name, site)


def test_fma32_is_fmaf():
    """the table's fmaf against rationals on random operands and on constructed ties of the float64 sum"""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    a, b = rng.normal(0, 1, 4000).astype(np.float32), rng.normal(0, 1, 4000).astype(np.float32)
    c = rng.normal(0, 1, 4000).astype(np.float32)
    # a * b + c with c = 1 + 2^-24-ish ties: the product's low bits decide the side
    a[:8] = np.float32(1 + 2.0 ** -23); b[:8] = np.float32(2.0 ** -25) * np.float32(1 + 2.0 ** -23); c[:8] = 1.0
    a[8:16] = np.float32(2.0 ** -30); b[8:16] = np.float32(2.0 ** -30); c[8:16] = np.float32(1 + 2.0 ** -23) + np.float32(2.0 ** -24)
    got = mt.fma32(a, b, c)
    for i in range(len(a)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        cands = [got[i], np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))]
        best = min(abs(Fraction(float(v)) - exact) for v in cands)
        assert abs(Fraction(float(got[i])) - exact) == best, i


# ---- BatchNorm --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", tier(SMALL, "exact"), ids=repr)
def test_fp32_entry_twins_agree_on_exact_inputs(sim, case):
    """before any device run: on the exact tier's inputs the fp32 entry itself returns one set of bits from both twins"""
    for site in case.sites:
        mt.check_fp32_twins_agree(sim, pc.NumpyDev(), case.data(mc.BF16, site, True))


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
@pytest.mark.parametrize("case", tier(SMALL, "exact"), ids=repr)
def test_bn_train_exact(sim, dev, case, fmt):
    for site in case.sites:
        for relu in case.relus:
            mt.check_exact(sim, dev, case, fmt, site, relu)


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
@pytest.mark.parametrize("case", tier(SMALL, "general"), ids=repr)
def test_bn_train_general(sim, dev, case, fmt):
    for site in case.sites:
        for relu in case.relus:
            mt.check_general(sim, dev, case, fmt, site, relu)


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
@pytest.mark.parametrize("case", [c for c in mt.BN_TRAIN_CASES if c.name.startswith(BIG)], ids=repr)
def test_bn_train_second_trip(sim, case, fmt):
    dev = pc.NumpyDev()
    site = case.sites[-1]
    if case.tier == "exact":
        mt.check_fp32_twins_agree(sim, dev, case.data(fmt, site, True))
        mt.check_exact(sim, dev, case, fmt, site, True)
    else:
        mt.check_general(sim, dev, case, fmt, site, True)


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
@pytest.mark.parametrize("case", tier(SMALL, "special"), ids=repr)
def test_bn_train_nan_inf_negative_zero(sim, dev, case, fmt):
    for site in case.sites:
        for relu in case.relus:
            mt.check_special(sim, dev, case, fmt, site, relu)


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
@pytest.mark.parametrize("want", bc.WANTED, ids=lambda w: "".join("xrwb"[i] if f else "-" for i, f in enumerate(w)))
@pytest.mark.parametrize("name", mt.WANTED_CASES)
def test_bn_train_null_outputs(sim, dev, name, want, fmt):
    """every NULL-output pattern of bn_cases.WANTED: what is asked for has the fp32 entry's bits, nothing else is written"""
    case = mt.BN_BY_NAME[name]
    for site in case.sites:
        mt.check_exact(sim, dev, case, fmt, site, True, want=want)


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
@pytest.mark.parametrize("name", mt.REPRODUCIBLE)
def test_bn_train_two_runs_are_bit_identical(sim, name, fmt):
    mt.check_reproducible(sim, pc.NumpyDev(), mt.BN_BY_NAME[name], fmt)


def test_bn_train_bad_arguments(sim):
    mt.check_bn_bad_arguments(sim, pc.NumpyDev())


# ---- cost volume and normalise backward -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
@pytest.mark.parametrize("case", [c for c in mt.CV_BWD_CASES if not c.name.startswith("trip2")], ids=repr)
def test_cost_volume_backward_16(sim, dev, case, fmt):
    mt.check_cv_bwd(sim, dev, case, fmt)


@pytest.mark.parametrize("case", [c for c in mt.CV_BWD_CASES if c.name.startswith("trip2")], ids=repr)
def test_cost_volume_backward_16_second_trip(sim, case):
    mt.check_cv_bwd(sim, pc.NumpyDev(), case, mc.BF16)


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
@pytest.mark.parametrize("case", mt.L1_BWD_CASES, ids=repr)
def test_l1_normalize_backward_mixed(sim, dev, case, fmt):
    mt.check_l1_bwd(sim, dev, case, fmt)


def test_misc_bad_arguments(sim):
    mt.check_misc_bad_arguments(sim, pc.NumpyDev())


def test_exports_and_abi():
    from ganet_amd import _native
    assert _native.ABI_VERSION == 14
    for name in ("ganet_bn_train_forward_mixed", "ganet_bn_train_backward_mixed", "ganet_cost_volume_backward_16",
                 "ganet_l1_normalize_backward_mixed"):
        assert name in _native.EXPORTS
