"""The channels-last path without a device: the case table's own helpers and numpy models (tests/cl_cases.py), the constants
it shares with ganet_amd/csrc/cl_kernels.h, the binding of include/ganet_hip_cl.h, and what harness.fuse.use_channels_last
rebinds -- on the stand-in networks everywhere, on the reference's models where their files are available."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import cl_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


# ---- the table --------------------------------------------------------------------------------------------------------------------

def test_constants_are_the_kernels():
    src = _read("ganet_amd", "csrc", "cl_kernels.h")
    k = {n: int(v) for n, v in re.findall(r"constexpr int (CL_BLOCK|CL_T|CL_CB|CL_MAX_BLOCKS|CV_TW|CV_DB|CV_CB) = (\d+);", src)}
    assert k == {"CL_BLOCK": cc.CL_BLOCK, "CL_T": cc.CL_T, "CL_CB": cc.CL_CB, "CL_MAX_BLOCKS": cc.CL_MAX_BLOCKS,
                 "CV_TW": cc.CV_TW, "CV_DB": cc.CV_DB, "CV_CB": cc.CV_CB}
    hdr = _read("include", "ganet_hip_cl.h")
    assert re.search(r"#define GANET_LAYOUT_PLANAR 0\b", hdr) and re.search(r"#define GANET_LAYOUT_CL 1\b", hdr)
    assert (cc.PLANAR, cc.CL) == (0, 1)


def test_case_table_reaches_what_it_claims():
    T = cc.CL_T
    assert set(cc.BN_S) >= {1, 2, T - 1, T, T + 1, 4 * T + 3, 1031} and set(cc.BN_C) >= {1, 3, 4, 5, 32, 48, 64, 67, 130}
    assert any(C > cc.CL_CB for C in cc.BN_C) and any(C > 2 * cc.CL_CB for C in cc.BN_C)
    assert {S % 4 for S in cc.BN_S} >= {0, 1, 2, 3} and {C % 4 for C in cc.BN_C} >= {0, 1, 2, 3}
    N, C, S = cc.OFFSET_SHAPE
    assert C % 4 == 0 and S % 4 == 0 and S > T
    N, C, S = cc.SECOND_TRIP["cl-none-cl"]
    assert C % 4 != 0 and cc.CL_MAX_BLOCKS * cc.CL_BLOCK < N * C * S <= cc.CL_MAX_BLOCKS * cc.CL_BLOCK + 8
    for combo in ("cl-none-planar", "planar-none-cl"):
        N, C, S = cc.SECOND_TRIP[combo]
        assert N * -(-S // T) * -(-C // cc.CL_CB) == cc.CL_MAX_BLOCKS + 1
    assert any(Dn > W for Dn in cc.CV_DN for W in cc.CV_W) and max(cc.CV_W) > cc.CV_TW
    assert any(c[1] > cc.CV_CB and c[1] % 4 == 0 for c in cc.CV_EXTRA) and any(c[1] > cc.CV_CB and c[1] % 4 for c in cc.CV_EXTRA)
    assert any(c[2] > cc.CV_DB for c in cc.CV_EXTRA) and any(c[0] * c[3] > cc.CL_MAX_BLOCKS for c in cc.CV_EXTRA)
    x, rem, scale, shift = cc.bn_data(2, 5, T + 1, "special")
    for a in (x, rem):
        assert np.isnan(a).any() and np.isposinf(a).any() and np.isneginf(a).any()
        assert ((a == 0) & np.signbit(a)).any() and ((a == 0) & ~np.signbit(a)).any()
    x, rem, scale, shift = cc.bn_data(2, 5, T + 1)
    assert (x < 0).any() and (x > 0).any() and (scale < 0).any() and (scale > 0).any()
    z = x.astype(np.float64) * scale[None, :, None] + shift[None, :, None]
    assert np.abs(z).min() >= 2.0 ** -8 and np.abs(z + rem).min() >= 2.0 ** -8          # off the kink
    assert (z < 0).any() and (z + rem < 0).any()


def test_every_entry_of_the_header_is_bound_and_in_the_table():
    from ganet_amd import _native
    hdr = _read("include", "ganet_hip_cl.h")
    declared = re.findall(r"^int (ganet_\w+)\(([^;]*)\);", hdr, flags=re.M)
    assert sorted(n for n, _ in declared) == sorted(_native._PROTOS_CL) == sorted(cc.ENTRIES)
    for name, args in declared:                                              # the argument lists, type by type
        want = [_native._P if "*" in a else _native._I for a in args.split(",")]
        assert _native._PROTOS_CL[name] == want, name
    assert not set(_native._PROTOS_CL) & set(_native.EXPORTS)                # include/ganet_hip.h's table is untouched
    cases = _read("tests", "cl_cases.py")
    capi = _read("ganet_amd", "csrc", "ganet_capi.hip")
    for name, _ in declared:
        assert f'"{name}"' in cases and f"GA_EXPORT int {name}(" in capi
    assert "ganet_hip_cl.h" in _read("ganet_amd", "build.py")


# ---- helpers and index maps -----------------------------------------------------------------------------------------------------

def test_permutation_helpers_round_trip():
    rng = np.random.default_rng(0)
    a = rng.normal(size=(2, 5, 7)).astype(np.float32)
    b = cc.to_cl(a)
    assert b.shape == (2, 7, 5) and b[1, 3, 4] == a[1, 4, 3] and b.flags["C_CONTIGUOUS"]
    assert np.array_equal(cc.from_cl(b), a)
    assert np.array_equal(cc.values(cc.image(a, cc.CL).ravel(), cc.CL, 2, 5, 7), a)
    assert np.array_equal(cc.values(cc.image(a, cc.PLANAR).ravel(), cc.PLANAR, 2, 5, 7), a)
    c = rng.normal(size=(2, 6, 3, 4, 5)).astype(np.float32)
    d = cc.cv_to_cl(c)
    assert d.shape == (2, 3, 4, 5, 6) and d[1, 2, 3, 4, 5] == c[1, 5, 2, 3, 4]
    assert np.array_equal(cc.cv_from_cl(d), c)
    t = torch.from_numpy(c)                                                  # torch's channels_last_3d is that image
    assert np.array_equal(t.contiguous(memory_format=torch.channels_last_3d).permute(0, 2, 3, 4, 1).contiguous().numpy(), d)


@pytest.mark.parametrize("shape", [(2, 5, 3), (1, 67, 130), (2, 4, 257), (1, 130, 129)])
def test_transpose_model_and_its_wrong_variants(shape):
    N, C, S = shape
    a = np.arange(N * C * S, dtype=np.int64).reshape(N, C, S)
    for src_cl in (True, False):
        src, want = (cc.to_cl(a), a) if src_cl else (a, cc.to_cl(a))
        assert np.array_equal(cc.model_transpose(src, N, C, S, src_cl), want.ravel())
        short = cc.model_transpose(src, N, C, S, src_cl, edge=-1)            # an off-by-one tile edge leaves elements unwritten
        assert (short == -1).sum() == N * C * -(-S // cc.CL_T)
        assert np.array_equal(cc.model_transpose(src, N, C, S, src_cl, tile=7, cb=3), want.ravel())


@pytest.mark.parametrize("dims", [(1, 3, 5, 2, 7), (2, 2, 9, 1, 4), (1, 1, 40, 2, 70), (1, 33, 3, 1, 66)])
def test_cost_volume_model_and_its_wrong_variants(dims):
    N, C, Dn, H, W = dims
    x, y = cc.cv_data(N, C, H, W)
    want = cc.cv_statement(x, y, Dn)
    assert np.array_equal(cc.model_cost_volume(x, y, Dn), want)
    assert np.array_equal(cc.model_cost_volume(x, y, Dn, tw=5, db=3), want)
    assert not np.array_equal(cc.model_cost_volume(x, y, Dn, swap=True), want)           # the halves exchanged
    if min(Dn, W) > 0:
        assert not np.array_equal(cc.model_cost_volume(x, y, Dn, strict=True), want)     # w > d in place of w >= d
    if W > 1 and Dn > 1:
        assert not np.array_equal(cc.model_cost_volume(x, y, Dn, edge=1), want)          # the y window one column off
        assert not np.array_equal(cc.model_cost_volume(x, y, Dn, edge=-1), want)
    # the statement against the planar definition (libs/GANet/modules/GANet.py:114-134), permuted
    planar = np.zeros((N, 2 * C, Dn, H, W), np.float32)
    for i in range(min(Dn, W)):
        planar[:, :C, i, :, i:] = x[:, :, :, i:]
        planar[:, C:, i, :, i:] = y[:, :, :, :W - i]
    assert np.array_equal(cc.cv_to_cl(planar).view(np.uint32), want)


def test_statement_is_the_planar_ops_arithmetic():
    """bn_statement against bn_cases' eval-form expression on one of its cases"""
    import bn_ref64
    x, rem, scale, shift = cc.bn_data(2, 5, 129)
    z = bn_ref64._fma32(x, scale[None, :, None], shift[None, :, None]) + rem
    want = np.where(z <= 0, np.float32(0), z)
    got = cc.bn_statement(x, rem, scale, shift, 1)
    assert np.abs(got - want).max() <= 2.0 ** -22 and (got == want).mean() > 0.999      # (double rounding in _fma32: rare, one ulp)
    assert np.array_equal(cc.bn_statement(np.float32([[[-0.0, np.nan]]]), None, np.float32([1]), np.float32([0]), 1).view(np.uint32)[0, 0, :1],
                          np.uint32([0]))
    assert np.isnan(cc.bn_statement(np.float32([[[np.nan]]]), None, np.float32([1]), np.float32([0]), 1)).all()


# ---- Python layer, no device --------------------------------------------------------------------------------------------------------

def test_layout_is_read_from_strides():
    from ganet_amd.functions import channels_last as fcl
    x = torch.randn(2, 4, 3, 5, 6)
    assert fcl.layout_of(x) == fcl.PLANAR
    assert fcl.layout_of(x.contiguous(memory_format=torch.channels_last_3d)) == fcl.CL
    assert fcl.layout_of(x[:, :, :, :, ::2]) is None                         # dense in neither
    one = torch.randn(2, 1, 3, 5, 6)                                         # C == 1: both hold, planar wins
    assert fcl.layout_of(one.contiguous(memory_format=torch.channels_last_3d)) == fcl.PLANAR
    assert fcl.layout_of(torch.randn(2, 4, 1, 1, 1).contiguous(memory_format=torch.channels_last_3d)) == fcl.PLANAR
    e = fcl.empty_cl((2, 4, 3, 5, 6), "cpu")
    assert e.shape == (2, 4, 3, 5, 6) and e.is_contiguous(memory_format=torch.channels_last_3d) and fcl.layout_of(e) == fcl.CL
    e4 = fcl.empty_cl((2, 4, 5, 6), "cpu")
    assert e4.is_contiguous(memory_format=torch.channels_last)
    # both cat operands channels-last -> the result is: what Conv2x relies on
    a, b = (torch.randn(1, 3, 2, 4, 5).contiguous(memory_format=torch.channels_last_3d) for _ in range(2))
    assert fcl.layout_of(torch.cat((a, b), 1)) == fcl.CL


def test_functions_and_modules_refuse_misuse():
    from ganet_amd.functions import channels_last as fcl
    from ganet_amd.modules.channels_last import ClBnRelu, ClGetCostVolume
    x = torch.randn(1, 2, 3, 4, 5)
    with pytest.raises(RuntimeError, match="HIP"):
        fcl.bn_apply_cl(x, torch.ones(2), torch.zeros(2))
    with pytest.raises(RuntimeError, match="HIP"):
        fcl.cost_volume_cl(torch.randn(1, 2, 3, 4), torch.randn(1, 2, 3, 4), 3)
    bn = torch.nn.BatchNorm3d(2)
    with pytest.raises(RuntimeError, match="inference-only"):
        ClBnRelu(bn)(x)                                                      # training mode
    bn.eval()
    with pytest.raises(RuntimeError, match="inference-only"):
        ClBnRelu(bn)(x)                                                      # autograd on, parameters want gradients
    with pytest.raises(TypeError):
        ClBnRelu(torch.nn.ReLU())
    with pytest.raises(TypeError):
        ClBnRelu(bn, out_format=torch.preserve_format)
    assert ClGetCostVolume(4).maxdisp == 5 and not list(ClBnRelu(bn).state_dict()) == ["x"]


# ---- use_channels_last ------------------------------------------------------------------------------------------------------------

def _bound(model):
    from harness import fuse
    convs = {k: m for k, m in model.named_modules() if type(m).__name__ == "BasicConv" and "_cl_bn" in m.__dict__}
    blocks = {k: m for k, m in model.named_modules() if type(m).__name__ == "SGABlock"}
    assert all(m.forward.__func__ is fuse._cl_sgablock_forward for m in blocks.values())
    planar_convs = sorted(k for k, m in convs.items() if m._cl_bn.out_format == torch.contiguous_format)
    planar_tails = sorted(k for k, m in blocks.items() if m._cl_tail.out_format == torch.contiguous_format)
    return convs, blocks, planar_convs, planar_tails


def _check_binding(model, producers, final, n_sga):
    from harness import fuse
    before = {k: v.clone() for k, v in model.state_dict().items()}
    n = fuse.use_channels_last(model)
    after = model.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    convs, blocks, planar_convs, planar_tails = _bound(model)
    assert planar_convs == sorted("cost_agg." + p for p in producers) and len(planar_convs) == n_sga == len(blocks)
    assert planar_tails == ["cost_agg." + final]
    assert all(k.startswith("cost_agg.") and isinstance(m.bn, torch.nn.BatchNorm3d) for k, m in convs.items())
    in_agg = [m for k, m in model.named_modules() if type(m).__name__ == "BasicConv" and k.startswith("cost_agg.") and m.use_bn]
    assert len(convs) == len(in_agg)                                         # every 3-D BasicConv with use_bn, and only those
    assert all("_cl_bn" not in m.__dict__ for k, m in model.named_modules() if not k.startswith("cost_agg."))
    assert isinstance(model.cv._cl_cv, __import__("ganet_amd.modules.channels_last", fromlist=["x"]).ClGetCostVolume)
    assert model.cv._cl_cv.maxdisp == model.cv.maxdisp
    assert n == len(convs) + len(blocks) + 1
    for k, m in blocks.items():
        if m.refine:
            assert m._cl_bnrelu.bn is m.bn_relu[0] and m._cl_bnrelu.out_format == torch.channels_last_3d and m._cl_tail.bn is m.conv_refine.bn
        else:
            assert m._cl_tail.bn is m.bn
    for k, m in model.named_modules():                                       # the weights: channels-last in cost_agg, conv32x1 aside
        if isinstance(m, (torch.nn.Conv3d, torch.nn.ConvTranspose3d)):
            cl = m.weight.is_contiguous(memory_format=torch.channels_last_3d)
            assert cl if k.startswith("cost_agg.") and not k.endswith("conv32x1") else (m.weight.is_contiguous() or cl), k
    return n


def test_use_channels_last_on_the_stand_in_networks():
    import mixed_standin as ms
    import standin_net as sn
    from harness import fuse
    _check_binding(ms.GANet(12).eval(), ["conv_start", "conv1a", "deconv1a.conv2"], "sga2", 3)
    _check_binding(sn.GANet(48).eval(), ["conv_start", "conv1a", "deconv1a.conv2", "deconv1b.conv2"], "sga3", 4)
    with pytest.raises(RuntimeError, match="inference-only"):
        fuse.use_channels_last(ms.GANet(12).train())
    mixed = ms.GANet(12).eval()
    fuse.use_mixed_precision(mixed, torch.bfloat16)
    with pytest.raises(RuntimeError, match="use_mixed_precision"):
        fuse.use_channels_last(mixed)
    mixed = sn.GANet(48).eval()
    fuse.use_mixed_precision_training(mixed, torch.bfloat16)
    with pytest.raises(RuntimeError, match="use_mixed_precision"):
        fuse.use_channels_last(mixed)
    bound = ms.GANet(12).eval()                                              # an earlier rebinding is kept, the call is refused in training mode
    fuse.use_fused_ops(bound)
    fuse.use_fused_bn(bound)
    fuse.use_channels_last(bound)
    bound.train()
    with pytest.raises(RuntimeError, match="inference-only"):
        bound.cost_agg.conv1a(torch.zeros(1, ms.C, 2, 4, 4))


@pytest.mark.parametrize("name,final,producers", [
    ("GANet11", "sga2", ["conv_start", "conv1a", "deconv1a.conv2", "deconv2a.conv2"]),
    ("GANet_deep", "sga3", ["conv_start", "conv1a", "deconv1a.conv2", "deconv2a.conv2", "conv1b.conv2", "deconv1b.conv2", "deconv2b.conv2"])])
def test_use_channels_last_on_the_reference_models(name, final, producers):
    """the binding table on the reference's own two models (where their files are available; no device: nothing is run)"""
    from harness import fuse, refmodel, steps
    if not refmodel.available():
        pytest.skip("no reference model code (GANET_REF_ROOT, /root/reference or oracle/_ref/pyref)")
    model = steps.build_model(name, 48, "cpu").eval()
    _check_binding(model, producers, final, len(producers))
    with pytest.raises(RuntimeError, match="inference-only"):
        fuse.use_channels_last(steps.build_model(name, 48, "cpu").train())
    mixed = steps.build_model(name, 48, "cpu").eval()
    fuse.use_mixed_precision(mixed, torch.float16)
    with pytest.raises(RuntimeError, match="use_mixed_precision"):
        fuse.use_channels_last(mixed)


def test_command_lines_and_the_switch(monkeypatch):
    from harness import miopen_env, predict as hp
    args = hp.parse_args(["--left", "a.png", "--right", "b.png", "--out", "o.png", "--channels_last"])
    assert args.channels_last and not hp.parse_args(["--left", "a", "--right", "b", "--out", "o"]).channels_last
    assert "--channels_last" in _read("harness", "infer.py")
    monkeypatch.delenv("PYTORCH_MIOPEN_SUGGEST_NHWC", raising=False)
    assert miopen_env.suggest_channels_last() == "1" and os.environ["PYTORCH_MIOPEN_SUGGEST_NHWC"] == "1"
    monkeypatch.setenv("PYTORCH_MIOPEN_SUGGEST_NHWC", "0")
    assert miopen_env.suggest_channels_last() == "0"                         # the caller's setting stands


# ---- large offsets ------------------------------------------------------------------------------------------------------------------

import math  # noqa: E402

import large_cases as lc  # noqa: E402
import large_cases_cl as lccl  # noqa: E402
import test_large_cases_cpu as lcc  # noqa: E402


def test_both_directions_have_a_large_offset_case():
    assert {c.entries for c in lccl.CASES} == {("ganet_bn_apply_forward_cl",)}
    assert sorted(lccl.FORMS.values()) == [(cc.PLANAR, cc.CL), (cc.CL, cc.PLANAR)]
    C, S = lccl.DIMS
    assert C % 4 == 0 and S % 4 == 0 and S % cc.CL_T != 0 and S > cc.CL_T    # 16-byte requests on both sides, a partial tile


@pytest.mark.parametrize("case", lccl.CASES, ids=repr)
def test_large_case_premises_and_teeth(case):
    lcc.test_case_premises(case)
    assert lc.assert_teeth(case) >= 4


class WrappedStoreModel(lcc.ModelStore):
    """y written with wrapped offsets: the value computed for true offset i is stored at wrap(i); an element nothing was stored
    to keeps the NaN it was filled with"""

    def _slice(self, spec, k):
        lay = self.case.layout
        comp = np.asarray(self.case.want[self.out], np.float32).reshape(lay.nb, spec.per)

        def at(idx):
            q = idx // spec.per
            return comp[lay.block_of[q % lay.R], idx % spec.per]

        j = np.arange(k * spec.per, (k + 1) * spec.per, dtype=np.int64)
        if self.thr is None:
            return at(j)
        out = np.where(self.wrap(j) == j, at(j), np.float32(np.nan))
        for m in (1, 2):
            src = j + m * self.period
            ok = src < self.total
            lands = ok & (self.wrap(np.minimum(src, self.total - 1)) == j)
            out = np.where(lands, at(np.where(ok, src, 0)), out)
        return out.astype(np.float32)


@pytest.mark.parametrize("case", lccl.CASES, ids=repr)
def test_large_checker_accepts_exact_offsets(case):
    assert lc.Checker(case, WrappedStoreModel(case, "y", lcc.CORRECT)).check("y") <= 1.0


@pytest.mark.parametrize("kind", lcc.WRAPS, ids=lambda k: k[0].replace(" ", "-"))
@pytest.mark.parametrize("case", lccl.CASES, ids=repr)
def test_large_checker_rejects_wrapped_offsets(case, kind):
    store = WrappedStoreModel(case, "y", kind)
    assert store.thr < store.total, "the tensor is large enough for this truncation to matter"
    with pytest.raises(AssertionError):
        lc.Checker(case, store).check("y")
    spec = case.tensors["y"]
    hit = [k for k in case.layout.special if (k + 1) * spec.per > store.thr]
    assert hit, "a special slice lies where offsets wrap"
    assert lc.ratio_of(store.host("y", 0, hit[0]), case.want["y"][case.layout.block_of[hit[0]]], spec.kind) == math.inf
