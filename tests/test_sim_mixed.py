"""The mixed-precision kernels (ganet_amd/csrc/mixed_kernels.h) on the CPU emulator build: the case table of tests/mixed_cases.py
(tests/test_gpu_mixed.py runs the same table on the device), every buffer at a guard page -- ENDING at one, resp. BEGINNING right
behind one -- and every output pre-filled with a NaN pattern.  The yardstick is equality with the fp32 entry of the same build on
the up-cast input, rounded by the table's own numpy statement of round-to-nearest-even; the first tests hold that statement to
torch's CPU conversion."""
import os
import re

import numpy as np
import pytest

import mixed_cases as mc
import parity_cases as pc

FMTS = [mc.F16, mc.BF16]
fmt_id = mc.FMT_NAME.get


@pytest.fixture(scope="module")
def sim():
    from sim_util import sim_api
    return sim_api()


@pytest.fixture(params=["end", "start"])
def dev(request):
    return pc.NumpyDev(request.param)


def _torch_dtype(fmt):
    import torch
    return {mc.F16: torch.float16, mc.BF16: torch.bfloat16}[fmt]


# ---- the yardstick ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
def test_convert_is_torchs_cpu_conversion(fmt):
    import torch
    table = mc.conversion_table(fmt)
    theirs = torch.from_numpy(table).to(_torch_dtype(fmt)).view(torch.int16).numpy().view(np.uint16)
    mc.assert_same(mc.convert(table, fmt), theirs, fmt, "convert against torch")
    every = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    theirs = torch.from_numpy(every.view(np.int16)).view(_torch_dtype(fmt)).float().numpy()
    mc.assert_same(mc.up(every, fmt), theirs, mc.F32, "up against torch")
    assert np.array_equal(mc.convert(mc.up(every, fmt), fmt)[~mc.is_nan(every, fmt)], every[~mc.is_nan(every, fmt)])    # a round trip


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
def test_conversion_table_holds_what_it_claims(fmt):
    table = mc.conversion_table(fmt)
    got = mc.convert(table, fmt)
    h = mc.tie_neighbours(fmt)
    k = len(h)
    mid, below, above = table[:k], table[k:2 * k], table[2 * k:3 * k]
    even = (h & 1) == 0
    # a tie goes to the even neighbour, one fp32 ulp to either side decides it
    assert np.array_equal(got[:k], np.where(even, h, h + 1))
    assert np.array_equal(got[k:2 * k], h) and np.array_equal(got[2 * k:3 * k], h + 1)
    assert (below < mid).all() and (mid < above).all()
    assert even.any() and (~even).any()
    inf = 0x7C00 if fmt == mc.F16 else 0x7F80
    assert inf in got[:k] and (inf | 0x8000) in got and 0x8000 in got and 0 in got and (inf - 1) in got
    assert np.isnan(table).sum() >= 6 and np.isinf(table).sum() >= 2
    sub = (np.abs(table) > 0) & (np.abs(table) < np.float32(2.0 ** -126))
    assert sub.sum() >= 6
    assert len(table) >= 2 ** 16 + 6 * k


def test_case_table_reaches_what_it_claims():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "ganet_amd", "csrc", "bn_kernels.h")).read() + open(os.path.join(root, "ganet_amd", "csrc", "mixed_kernels.h")).read()
    k = {n: int(v) for n, v in re.findall(r"constexpr int (BN_BLOCK|BN_MAX_ROWS|BN_TARGET_BLOCKS|MX_V) = (\d+);", src)}
    assert (k["BN_BLOCK"], k["BN_MAX_ROWS"], k["BN_TARGET_BLOCKS"], k["MX_V"]) == (mc.BN_BLOCK, mc.BN_MAX_ROWS, mc.BN_TARGET_BLOCKS, mc.MX_V)
    big = [c for c in mc.BN_CASES if c.name == "second-trip"][0]
    N, C, S = big.shape
    assert mc.BN_TARGET_BLOCKS // C == mc.BN_MAX_ROWS and S % mc.MX_V == 0
    assert S // mc.MX_V == mc.BN_MAX_ROWS * mc.BN_BLOCK + 1                    # one group beyond a full trip of every lane
    assert sorted({c.shape[2] % 8 for c in mc.BN_CASES}) == [0, 2, 4, 5]
    assert any(c.off for c in mc.BN_CASES) and any(c.inplace for c in mc.BN_CASES)
    assert any(c.off for c in mc.CV_CASES) and any(c.Dn > c.shape[3] for c in mc.CV_CASES)
    assert {c.dims[3] for c in mc.L1_CASES} >= {5, 75, 27, 7}


# ---- the kernels --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
def test_cast_16_to_32_every_pattern(sim, dev, fmt):
    every = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    mc.check_cast(sim, dev, every, fmt, mc.F32)


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
def test_cast_32_to_16_table(sim, dev, fmt):
    mc.check_cast(sim, dev, mc.conversion_table(fmt), mc.F32, fmt)


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
def test_cast_sizes_and_bases(sim, fmt):
    dev = pc.NumpyDev()
    table = mc.conversion_table(fmt)
    for n in mc.CAST_SIZES:
        mc.check_cast(sim, dev, np.resize(table, n), mc.F32, fmt)
        mc.check_cast(sim, dev, mc.convert(np.resize(table, n), fmt), fmt, mc.F32)
    for so, do in mc.CAST_OFFSETS:
        mc.check_cast(sim, dev, table[:1027], mc.F32, fmt, src_off=so, dst_off=do)
        mc.check_cast(sim, dev, mc.convert(table[:1027], fmt), fmt, mc.F32, src_off=so, dst_off=do)


def test_cast_copies_and_across_formats(sim, dev):
    every = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    table = mc.conversion_table(mc.BF16)
    mc.check_cast(sim, dev, table, mc.F32, mc.F32)                             # 32 -> 32: a copy, NaN payloads included
    for fmt in FMTS:
        mc.check_cast(sim, dev, every, fmt, fmt)                               # 16 -> 16 of one type: a copy
        mc.check_cast(sim, dev, every[:4099], fmt, fmt, src_off=1, dst_off=3)
    mc.check_cast(sim, dev, every, mc.F16, mc.BF16)
    mc.check_cast(sim, dev, every, mc.BF16, mc.F16)
    # the one-element-per-lane forms of the same three: a base that is not 16-byte aligned, and fewer elements than a vector
    mc.check_cast(sim, dev, table[:1027], mc.F32, mc.F32, src_off=1, dst_off=3)
    mc.check_cast(sim, dev, table[:7], mc.F32, mc.F32)
    mc.check_cast(sim, dev, every[:4099], mc.F16, mc.BF16, src_off=1, dst_off=3)
    mc.check_cast(sim, dev, every[:4099], mc.BF16, mc.F16, src_off=1, dst_off=3)


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
@pytest.mark.parametrize("case", [c for c in mc.BN_CASES if c.name != "second-trip"], ids=repr)
def test_bn_apply_mixed(sim, dev, case, fmt):
    mc.check_bn(sim, dev, case, fmt)


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
def test_bn_apply_mixed_second_trip(sim, fmt):
    mc.check_bn(sim, pc.NumpyDev(), [c for c in mc.BN_CASES if c.name == "second-trip"][0], fmt)


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
@pytest.mark.parametrize("case", mc.CV_CASES, ids=repr)
def test_cost_volume_16(sim, dev, case, fmt):
    mc.check_cv(sim, dev, case, fmt)


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_id)
@pytest.mark.parametrize("case", mc.L1_CASES, ids=repr)
def test_l1_normalize_mixed(sim, dev, case, fmt):
    mc.check_l1(sim, dev, case, fmt)


def test_bad_arguments(sim):
    mc.check_bad_arguments(sim, pc.NumpyDev())


def test_exports_and_abi():
    from ganet_amd import _native
    assert _native.ABI_VERSION == 14
    for name in ("ganet_cast", "ganet_bn_apply_forward_mixed", "ganet_cost_volume_forward_16", "ganet_l1_normalize_forward_mixed"):
        assert name in _native.EXPORTS
