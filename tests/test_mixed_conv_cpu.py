"""conv32x1 on a 16-bit x without a device: the comparison of tests/mixed_conv_cases.py rejects four wrong kernels stated in
numpy; the rounding family contains what it claims; harness.fuse.use_mixed_disp_conv on tests/standin_net.py and (where they are
importable) on the reference's models; include/ganet_hip_conv16.h, _native._PROTOS_CONV16 and the library agree; and every new
entry has a large-offset case whose checker rejects wrapped offsets on a numpy model.  The kernels themselves:
tests/test_sim_mixed_conv.py (emulator) and tests/test_gpu_mixed_conv.py (device)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import disp_conv_ref64 as ref
import large_cases as lc
import large_cases_conv16 as lc16
import mixed_cases as mc
import mixed_conv_cases as mcc
import test_large_cases_cpu as lcc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
fmt_id = mc.FMT_NAME.get
F32 = np.float32

from harness import fuse, refmodel  # noqa: E402

needs_models = pytest.mark.skipif(not refmodel.available(), reason="no reference model code (harness.refmodel.available())")


# ---- the table and its comparison -----------------------------------------------------------------------------------------------

def test_case_table_reaches_what_it_claims():
    mcc.check_table()
    # geometry and arithmetic are not merely shared with the fp32 kernels: they are the same text, with the storage type of the
    # big volume as a template parameter, so there is no second copy that could drift
    csrc = os.path.join(ROOT, "ganet_amd", "csrc")
    assert not os.path.exists(os.path.join(csrc, "disp_conv16_kernels.h"))
    hdr = open(os.path.join(csrc, "disp_conv_kernels.h")).read()
    for kernel in ("disp_conv_fwd", "disp_conv_bwd_data", "disp_conv_bwd_weight_partials"):
        assert len(re.findall(r"^%s\(" % kernel, hdr, re.M)) == 1, kernel
        assert len(re.findall(r"template <typename ST, bool VEC>\nstatic __global__ void __launch_bounds__\(64 \* DCV_WAVES\)\n%s\(" % kernel, hdr)) == 1, kernel
    assert len(re.findall(r"__global__", hdr)) == 4 and "disp_conv16" not in hdr        # (the fourth: disp_conv_bwd_weight_sum)
    for const in ("DCV_WAVES", "DCV_PX", "DCV_DEPTH", "DCV_CB"):
        assert hdr.count("constexpr int %s = " % const) == 1, const
    assert hdr.count("fmaf(") == 3, "one FMA chain per direction, whatever the storage type"
    for shared in ("dcv_lane(g)", "dcv_fma9(", "dcv_plane<VEC>(", "dcv_store4<st_f32, VEC>(y + ", "dcv_store4<ST, VEC>(gx + ", "dcv_own4<ST, VEC>(x + ",
                   "seg_allsum<64>(acc[j][t])", "(r0.x + r1.x) + (r2.x + r3.x)"):
        assert shared in hdr, shared
    assert hdr.count("dcv_lane(g)") == 3 and hdr.count("seg_allsum<64>(acc[j][t])") == 1 and hdr.count("(r0.x + r1.x) + (r2.x + r3.x)") == 1
    assert "atomic" not in re.sub(r"//[^\n]*", "", hdr)                 # (the header's comment says "no atomics"; the code has none)
    # the host side: each direction is launched from one place, by the fp32 entry and by the _16 entry
    capi = open(os.path.join(csrc, "ganet_capi.hip")).read()
    for kernel in ("disp_conv_fwd<", "disp_conv_bwd_data<", "disp_conv_bwd_weight_partials<", "disp_conv_bwd_weight_sum,"):
        assert capi.count("GA_LAUNCH((" + kernel) + capi.count("GA_LAUNCH(" + kernel) == 1, kernel


@pytest.mark.parametrize("fmt", mcc.FMTS, ids=fmt_id)
def test_exact_family_premises(fmt):
    for case in mcc.CASES:
        if case.kind == "exact":
            mcc.premises(case, fmt)


@pytest.mark.parametrize("fmt", mcc.FMTS, ids=fmt_id)
@pytest.mark.parametrize("case", [c for c in mcc.CASES if c.kind == "rounding"], ids=repr)
def test_rounding_family_contains_what_it_claims(case, fmt):
    """on the float64 statement rounded to fp32 (channels 0 and 1 are +-grad_y exactly, whichever kernel computes them): ties of
    both parities, overflow, fp16 subnormals, a NaN, and a truncating store would differ on a quarter of the elements or more"""
    with np.errstate(all="ignore"):
        gx32 = case.statement(fmt).grad_x.astype(F32)
    x16, w, g = case.made(fmt)
    assert np.array_equal(gx32[:, 0][~np.isnan(gx32[:, 0])], g[~np.isnan(gx32[:, 0])])
    assert mcc.rounding_premises(case, fmt, gx32) >= 0.25


def _model(case, fmt, mutation=None):
    """{"16": ..., "32": ...} as mixed_conv_cases.run returns them, from the float64 statement rounded once -- the stand-in for a
    kernel pair that is right -- with the "16" arm under a wrong definition where `mutation` names one"""
    x16, w, g = case.made(fmt)
    st = case.statement(fmt)
    with np.errstate(all="ignore"):
        y, gx, gw = st.y.astype(F32), st.grad_x.astype(F32), st.grad_weight.astype(F32)
    good32 = {"y": y, "grad_x": gx, "grad_weight": gw, "fmt": mc.F32}
    y16, gx16 = y, mc.convert(gx, fmt)
    if mutation == "truncating_store":
        gx16 = mcc.truncate(gx, fmt)
    elif mutation == "doubly_rounded":                     # through a format with two more bits, then to 16
        keep = 16 + 2
        u = gx.view(np.uint32).astype(np.uint64)
        if fmt == mc.BF16:
            sh = 32 - keep
            mid = (((u + ((1 << (sh - 1)) - 1) + ((u >> sh) & 1)) >> sh) << sh).astype(np.uint32).view(F32)
        else:
            sh = 13 - 2                                    # fp16 keeps 10 of the 23 fraction bits
            mid = (((u + ((1 << (sh - 1)) - 1) + ((u >> sh) & 1)) >> sh) << sh).astype(np.uint32).view(F32)
        gx16 = mc.convert(mid, fmt)
    elif mutation == "missing_halo_column":                # the tap kw = 0 of a lane's first pixel: the word left of its four
        x64, w64 = mc.up(x16, fmt).astype(np.float64), w.astype(np.float64).reshape(-1, 3, 3, 3)
        wl = w64.copy()
        wl[:, :, :, 1:] = 0
        left = ref.forward(x64, wl)
        left[..., np.arange(left.shape[-1]) % ref.PX != 0] = 0
        y16 = (st.y - left).astype(F32)
    elif mutation == "weight_rounded_first":               # what torch.autocast does to the parameter
        wr = mc.up(mc.convert(w, fmt), fmt)
        y16 = ref.forward(mc.up(x16, fmt).astype(np.float64), wr.astype(np.float64).reshape(-1, 3, 3, 3)).astype(F32)
    else:
        assert mutation is None
    return {"16": {"y": y16, "grad_x": gx16, "grad_weight": gw, "fmt": fmt}, "32": good32}


MUTATIONS = {"truncating_store": "rounding", "doubly_rounded": "rounding", "missing_halo_column": "general", "weight_rounded_first": "general"}


@pytest.mark.parametrize("fmt", mcc.FMTS, ids=fmt_id)
@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_comparison_rejects(mutation, fmt):
    """the comparison accepts the model of a right kernel and rejects each wrong one, on every case of the family that shows it"""
    hit = 0
    for case in mcc.CASES:
        if case.kind != MUTATIONS[mutation] or (mutation == "missing_halo_column" and case.shape[4] <= ref.PX):
            continue
        good = _model(case, fmt)
        mcc.compare(case, fmt, good["16"], good["32"])
        bad = _model(case, fmt, mutation)
        with pytest.raises(AssertionError, match="differ"):
            mcc.compare(case, fmt, bad["16"], bad["32"])
        hit += 1
    assert hit >= 3, (mutation, hit)


@pytest.mark.parametrize("fmt", mcc.FMTS, ids=fmt_id)
def test_exact_comparison_rejects_a_missing_halo_column(fmt):
    for name in ("C33-W8-H3-D9-N2", "blocks-twin"):
        case = mcc.by_name(name, "exact")
        mcc.compare_exact(case, fmt, _model(case, fmt)["16"])
        with pytest.raises(AssertionError, match="differ"):
            mcc.compare_exact(case, fmt, _model(case, fmt, "missing_halo_column")["16"])


# ---- the rebinder ---------------------------------------------------------------------------------------------------------------

def _sites(model):
    return [m.conv32x1 for m in model.modules() if type(m).__name__ in ("Disp", "DispAgg")]


def _check_rebound(model, keys, params, n, kernels=True):
    from ganet_amd.modules.mixed_conv import MixedDispConv
    assert list(model.state_dict()) == keys and [id(p) for p in model.parameters()] == params
    sites = _sites(model)
    assert len(sites) == n
    for conv in sites:
        helper = conv.__dict__["_fused_conv"]
        assert type(helper) is MixedDispConv and helper.conv is conv and helper.conv.weight is conv.weight and helper.kernels is kernels
        assert "forward" in conv.__dict__ and "_fused_conv" not in conv._modules


ORDERS = [("conv16",), ("infer", "conv16"), ("conv16", "infer"), ("train", "conv16"), ("conv16", "train"), ("ops", "bn", "tail", "conv16", "train"),
          ("conv", "conv16"), ("conv16", "ops", "tail")]


def _apply(model, order, n):
    for step in order:
        if step == "conv16":
            assert fuse.use_mixed_disp_conv(model) == n
        elif step == "conv":
            assert fuse.use_fused_disp_conv(model) == n
        elif step == "infer":
            assert fuse.use_mixed_precision(model) > n
        elif step == "train":
            assert fuse.use_mixed_precision_training(model) > n
        elif step == "ops":
            assert fuse.use_fused_ops(model) > 0
        elif step == "bn":
            assert fuse.use_fused_bn(model) > 0
        else:
            assert fuse.use_fused_disp_tail(model) == n - 1


@pytest.mark.parametrize("order", ORDERS, ids="-".join)
def test_use_mixed_disp_conv_on_the_stand_in(order):
    import standin_net
    model = standin_net.build(48)
    keys, params = list(model.state_dict()), [id(p) for p in model.parameters()]
    _apply(model, order, 3)
    _check_rebound(model, keys, params, 3)
    for conv in _sites(model):                              # both input widths reach our ops: neither has a CPU path
        for dt in (torch.float32, torch.bfloat16, torch.float16):
            with pytest.raises(RuntimeError, match="no CPU path"):
                conv(torch.zeros(1, conv.in_channels, 2, 3, 4, dtype=dt))


@needs_models
@pytest.mark.parametrize("name,n", [("GANet_deep", 3), ("GANet11", 2)])
def test_use_mixed_disp_conv_on_the_reference_models(name, n):
    from harness import steps
    for order in ORDERS:
        torch.manual_seed(0)
        model = steps.build_model(name, 48, "cpu")
        keys, params = list(model.state_dict()), [id(p) for p in model.parameters()]
        _apply(model, order, n)
        _check_rebound(model, keys, params, n)


def test_a_later_use_fused_disp_conv_puts_the_fp32_only_module_back():
    """documented in use_mixed_disp_conv: the two rebinders share one slot, the last one holds the site"""
    import standin_net
    from ganet_amd.modules.fused import DispConv
    model = standin_net.build(48)
    keys = list(model.state_dict())
    assert fuse.use_mixed_disp_conv(model, kernels=False, directions=("forward",)) == 3
    assert all(c._fused_conv.kernels is False and c._fused_conv.directions == ("forward",) for c in _sites(model))
    assert fuse.use_fused_disp_conv(model) == 3 and list(model.state_dict()) == keys
    for conv in _sites(model):
        assert type(conv._fused_conv) is DispConv
        with pytest.raises(RuntimeError, match="no CPU path"):
            conv(torch.zeros(1, conv.in_channels, 2, 3, 4))
        # a 16-bit input is the wrapped convolution's again (ATen, on the CPU here: under autocast its output has the input's dtype)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            assert conv(torch.zeros(1, conv.in_channels, 2, 3, 4, dtype=torch.bfloat16)).dtype == torch.bfloat16
    assert fuse.use_mixed_disp_conv(model) == 3
    assert "last" in fuse.use_mixed_disp_conv.__doc__.lower() and "use_fused_disp_conv" in fuse.use_mixed_disp_conv.__doc__


def test_existing_rebinders_are_what_they_were():
    import standin_net
    from ganet_amd.modules.fused import DispConv
    model = standin_net.build(48)
    fuse.use_fused_disp_conv(model)
    fuse.use_mixed_precision_training(model)
    assert all(type(c._fused_conv) is DispConv for c in _sites(model))
    with pytest.raises(ValueError):
        fuse.use_mixed_disp_conv(standin_net.build(48), directions=("sideways",))


def test_functions_refuse_cpu_tensors_and_wrong_types():
    from ganet_amd.functions.mixed_conv import DispConv16Function
    with pytest.raises(RuntimeError, match="no CPU path"):
        DispConv16Function.apply(torch.zeros(1, 2, 3, 4, 5, dtype=torch.float16), torch.zeros(1, 2, 3, 3, 3))
    import ganet_amd.functions.mixed_train as ft
    assert len(ft.__all__) == 5


def test_flags_exist():
    from harness import predict, train
    assert train.parse(["--amp", "bf16", "--amp_conv32"]).amp_conv32 and not train.parse([]).amp_conv32
    args = ["--left", "l.png", "--right", "r.png", "--out", "o.png"]
    assert predict.parse_args(args + ["--amp", "fp16", "--amp_conv32"]).amp_conv32
    with pytest.raises(SystemExit):
        predict.parse_args(args + ["--amp_conv32"])
    src = open(os.path.join(ROOT, "harness", "infer.py")).read()
    assert '"--amp_conv32"' in src and "fuse.use_mixed_disp_conv(model" in src and "--amp_conv32 needs --amp" in src
    assert "--amp_conv32 needs --amp" in open(os.path.join(ROOT, "harness", "train.py")).read()


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------

def _declared():
    hdr = open(os.path.join(ROOT, "include", "ganet_hip_conv16.h")).read()
    protos = {}
    for name, params in re.findall(r"^int\s+(ganet_\w+)\(([^)]*)\);", hdr, re.M):
        protos[name] = [ctypes.c_void_p if "*" in p else ctypes.c_int for p in params.split(",")]
    return hdr, protos


def test_header_protos_and_library_agree():
    from ganet_amd import _native
    hdr, protos = _declared()
    assert set(protos) == set(_native._PROTOS_CONV16) == {n for n, _ in mcc.ENTRIES16}
    for name, want in protos.items():
        assert _native._PROTOS_CONV16[name] == want, name
    assert not set(protos) & set(_native.EXPORTS) and _native.ABI_VERSION == 14 and "GANET_ABI_VERSION" not in hdr.replace("GANET_ABI_VERSION stays 14", "")
    assert "bit for bit" in hdr and "convert(" in hdr and "GANET_E_INVALID" in hdr
    main = open(os.path.join(ROOT, "include", "ganet_hip.h")).read()
    assert not any(name in main for name in protos)
    lib = ctypes.CDLL(_native.lib_path())                  # the gfx950 build: loads without a GPU
    for name in protos:
        assert hasattr(lib, name), f"{name} declared in ganet_hip_conv16.h but not exported"
    src = open(os.path.join(ROOT, "ganet_amd", "build.py")).read()
    assert "ganet_hip_conv16.h" in src


def test_the_emulator_build_binds_the_new_entries():
    from sim_util import sim_api
    api = sim_api()
    assert all(api.has(n) for n, _ in mcc.ENTRIES16)


# ---- large offsets ------------------------------------------------------------------------------------------------------------------

def test_every_new_entry_has_a_large_offset_case():
    from ganet_amd import _native
    covered = {e for c in lc16.CASES for e in c.entries}
    assert covered == set(_native._PROTOS_CONV16)
    assert {lc16._fmt(c) for c in lc16.CASES} == {mc.F16, mc.BF16}


@pytest.mark.parametrize("case", lc16.CASES, ids=repr)
def test_large_case_premises_and_teeth(case):
    lcc.test_case_premises(case)
    assert case.tensors["x16"].itemsize == 2 and case.tensors["gx16"].itemsize == 2
    assert lc.assert_teeth(case) >= 4


class DataGradModel(lcc.ModelStore):
    """grad_x written with wrapped offsets: the pattern computed for true offset i is stored at wrap(i); an element nothing
    was stored to keeps the poison"""

    def _slice(self, spec, k):
        lay, fmt = self.case.layout, spec.fmt
        comp = mc.convert(np.asarray(self.case.want[self.out], F32), fmt).reshape(lay.nb, spec.per)

        def at(idx):
            q = idx // spec.per
            return comp[lay.block_of[q % lay.R], idx % spec.per]

        j = np.arange(k * spec.per, (k + 1) * spec.per, dtype=np.int64)
        if self.thr is None:
            return at(j)
        out = np.where(self.wrap(j) == j, at(j), np.uint16(lc.POISON[np.dtype(np.uint16)]))
        for m in (1, 2):
            src = j + m * self.period
            ok = src < self.total
            lands = ok & (self.wrap(np.minimum(src, self.total - 1)) == j)
            out = np.where(lands, at(np.where(ok, src, 0)), out)
        return out.astype(np.uint16)


@pytest.mark.parametrize("case", lc16.CASES, ids=repr)
def test_large_checker_accepts_exact_offsets(case):
    assert lc.Checker(case, DataGradModel(case, "gx16", lcc.CORRECT)).check("gx16") <= 1.0


@pytest.mark.parametrize("kind", lcc.WRAPS, ids=lambda k: k[0].replace(" ", "-"))
@pytest.mark.parametrize("case", lc16.CASES, ids=repr)
def test_large_checker_rejects_wrapped_offsets(case, kind):
    """int32 element offsets, and 32-bit byte offsets of either signedness, on 2-byte elements"""
    store = DataGradModel(case, "gx16", kind)
    assert store.thr < store.total, "the tensor is large enough for this truncation to matter"
    with pytest.raises(AssertionError):
        lc.Checker(case, store).check("gx16")
    spec = case.tensors["gx16"]
    hit = [k for k in case.layout.special if (k + 1) * spec.per > store.thr]
    assert hit, "a special slice lies where offsets wrap"
    b = case.layout.block_of[hit[0]]
    assert lc.ratio_of(mc.up(store.host("gx16", 0, hit[0]), spec.fmt), case.want["gx16"][b], spec.kind) == math.inf
