"""The channels-last inference path on the gfx950 build: the case table of tests/cl_cases.py through the C ABI
(tests/test_sim_cl.py runs it on the emulator) -- the same inputs, the same yardstick without a tolerance: the bits of the planar
entry on the permuted input, and of the numpy statement -- and, device only, the modules against BnRelu, the tail form in a
captured graph, harness.fuse.use_channels_last on the stand-in network with every call of the two new functions held to the
planar entry on its own recorded inputs, and what PyTorch answers to a channels-last convolution in a process of its own."""
import collections
import json
import os
import subprocess
import sys

import pytest

import cl_cases as cc
from test_gpu_parity import TorchDev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def same_bits(a, b):
    import torch
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- C ABI: the shared table ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", cc.BN_C)
@pytest.mark.parametrize("combo", list(cc.COMBOS))
def test_bn_apply_cl(api, dev, combo, C):
    cc.check_bn_table(api, dev, combo, C)


@pytest.mark.parametrize("combo", list(cc.COMBOS))
def test_bn_apply_cl_special_values(api, dev, combo):
    cc.check_special(api, dev, combo)


@pytest.mark.parametrize("combo", list(cc.COMBOS))
def test_bn_apply_cl_offset_bases(api, dev, combo):
    cc.check_offsets(api, dev, combo)


@pytest.mark.parametrize("combo", cc.INPLACE)
def test_bn_apply_cl_in_place(api, dev, combo):
    cc.check_inplace(api, dev, combo)


@pytest.mark.parametrize("combo", list(cc.SECOND_TRIP))
def test_bn_apply_cl_second_trip(api, dev, combo):
    cc.check_second_trip(api, dev, combo)


@pytest.mark.parametrize("Dn", cc.CV_DN)
@pytest.mark.parametrize("C", cc.CV_C)
def test_cost_volume_cl(api, dev, C, Dn):
    cc.check_cv_table(api, dev, C, Dn)


def test_cost_volume_cl_blocks_and_bases(api, dev):
    cc.check_cv_extra(api, dev)


def test_bad_arguments(api, dev):
    cc.check_bad_arguments(api, dev)


# ---- modules ------------------------------------------------------------------------------------------------------------------

def _bn(torch, C, seed=0):
    g = torch.Generator().manual_seed(seed)
    bn = torch.nn.BatchNorm3d(C)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(C, generator=g))
        bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
        bn.weight.copy_(torch.randn(C, generator=g))
        bn.bias.copy_(torch.randn(C, generator=g))
    return bn.cuda().eval()


@pytest.mark.parametrize("C", [1, 5, 8])
def test_cl_bn_relu_equals_bn_relu(api, C):
    """ClBnRelu == BnRelu(bn)(x.contiguous(), rem) in eval mode, bit for bit, for every input layout (channels-last, planar,
    dense in neither; C == 1 where both formats hold), rem none / planar / channels-last, both output formats; the output has
    the requested memory format and the logical shape"""
    import torch
    from ganet_amd.functions import channels_last as fcl
    from ganet_amd.modules.channels_last import ClBnRelu
    from ganet_amd.modules.fused import BnRelu
    torch.manual_seed(3)
    bn = _bn(torch, C)
    shape = (2, C, 3, 5, 12)
    base = torch.randn(shape, device="cuda") * 2
    wide = torch.randn(2, C, 3, 5, 24, device="cuda")
    xs = {"planar": base, "cl": base.contiguous(memory_format=torch.channels_last_3d), "strided": wide[..., ::2]}
    r = torch.randn(shape, device="cuda")
    rems = {"none": None, "planar": r, "cl": r.contiguous(memory_format=torch.channels_last_3d)}
    assert fcl.layout_of(xs["strided"]) is None and fcl.layout_of(xs["cl"]) == (fcl.PLANAR if C == 1 else fcl.CL)
    with torch.no_grad():
        for relu in (True, False):
            for xk, x in xs.items():
                for rk, rem in rems.items():
                    want = BnRelu(bn, relu=relu, inplace=False)(x.contiguous(), rem.contiguous() if rem is not None else None)
                    for fmt in (torch.channels_last_3d, torch.contiguous_format):
                        got = ClBnRelu(bn, relu=relu, out_format=fmt, inplace=False)(x, rem)
                        assert got.shape == x.shape and got.is_contiguous(memory_format=fmt), (xk, rk, fmt)
                        assert same_bits(got, want), (relu, xk, rk, fmt)
        # in place where x already lies in the output's format; never otherwise
        for xk, fmt, shared in (("cl", torch.channels_last_3d, C > 1), ("planar", torch.contiguous_format, True), ("cl", torch.contiguous_format, C == 1),
                                ("strided", torch.contiguous_format, False)):
            x = xs[xk].clone(memory_format=torch.preserve_format) if xk != "strided" else xs[xk]
            want = BnRelu(bn, inplace=False)(xs[xk].contiguous(), r)
            got = ClBnRelu(bn, out_format=fmt)(x, r)
            assert (got.data_ptr() == x.data_ptr()) == shared, (xk, fmt)
            assert same_bits(got, want)
    bn.train()
    with pytest.raises(RuntimeError, match="inference-only"):
        ClBnRelu(bn)(base)
    bn.eval()
    with pytest.raises(RuntimeError, match="inference-only"):
        ClBnRelu(bn)(base)                                                   # autograd on, parameters want gradients
    with torch.no_grad(), pytest.raises(TypeError):
        ClBnRelu(bn)(base.half())


def test_cl_cost_volume_equals_get_cost_volume(api):
    import torch
    from ganet_amd.modules.channels_last import ClGetCostVolume
    from ganet_amd.modules.GANet import GetCostVolume
    torch.manual_seed(5)
    with torch.no_grad():
        for shape, maxdisp in (((1, 4, 5, 16), 5), ((2, 3, 2, 7), 8), ((1, 32, 3, 70), 33)):
            x, y = torch.randn(shape, device="cuda"), torch.randn(shape, device="cuda")
            got, want = ClGetCostVolume(maxdisp)(x, y), GetCostVolume(maxdisp)(x, y)
            assert got.shape == want.shape and got.is_contiguous(memory_format=torch.channels_last_3d)
            assert same_bits(got, want)
            assert same_bits(ClGetCostVolume(maxdisp)(x.transpose(2, 3).contiguous().transpose(2, 3), y), want)     # a non-contiguous map


def test_tail_in_a_captured_graph(api):
    """the tail form (t channels-last, rem planar -> channels-last) captured and replayed on new data gives the plain call's bits"""
    import torch
    from ganet_amd.modules.channels_last import ClBnRelu
    torch.manual_seed(4)
    bn = _bn(torch, 8)
    op = ClBnRelu(bn, out_format=torch.channels_last_3d, inplace=False)
    xs = torch.randn(2, 8, 3, 4, 8, device="cuda").contiguous(memory_format=torch.channels_last_3d)
    rem = torch.randn(2, 8, 3, 4, 8, device="cuda")
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            op(xs, rem)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = op(xs, rem)
        xs.copy_(torch.randn(2, 8, 3, 4, 8, device="cuda"))
        rem.copy_(torch.randn(2, 8, 3, 4, 8, device="cuda"))
        assert xs.is_contiguous(memory_format=torch.channels_last_3d)
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(y, op(xs, rem)) and y.is_contiguous(memory_format=torch.channels_last_3d)


# ---- the stand-in network -------------------------------------------------------------------------------------------------------

def test_stand_in_network_channels_last(api, monkeypatch):
    """use_channels_last end to end on the tiny network of tests/mixed_standin.py under steps.predict: every call of bn_apply_cl
    and cost_volume_cl equals the planar entry on its own recorded inputs, the sites are the declared ones, both operands of the
    Conv2x concatenation share a layout.  No end-to-end tolerance: the convolution solvers may differ between the layouts; the
    difference against the planar arm is printed."""
    import torch
    import mixed_standin as ms
    sys.path.insert(0, ROOT)
    from ganet_amd.functions import channels_last as fcl
    from ganet_amd.functions.fused import BnApplyFunction
    from ganet_amd.functions.GANet import GetCostVolumeFunction
    from ganet_amd.modules import channels_last as mcl
    from harness import fuse, steps
    torch.manual_seed(9)
    first = ms.GANet(12).cuda().eval()
    model = ms.GANet(12).cuda().eval()
    model.load_state_dict(first.state_dict())
    keys = list(model.state_dict())
    n = fuse.use_channels_last(model)
    assert n == 4 + 3 + 3 + 1 and list(model.state_dict()) == keys          # BasicConvs (conv_refine's included), SGABlocks, cv
    calls, cvs, cats = [], [], []
    real_bn, real_cv, real_cat = mcl.bn_apply_cl, mcl.cost_volume_cl, torch.cat

    def rec_bn(x, scale, shift, rem=None, relu=True, out_format=torch.channels_last_3d, inplace=False):
        xl = fcl.layout_of(x)
        kept = (x.clone(memory_format=torch.preserve_format), scale, shift, rem, relu)
        out = real_bn(x, scale, shift, rem, relu, out_format, inplace)
        calls.append((xl, rem is not None, out_format, kept, out))
        return out

    def rec_cv(x, y, maxdisp):
        out = real_cv(x, y, maxdisp)
        cvs.append((x, y, maxdisp, out))
        return out

    def rec_cat(tensors, *a, **kw):
        if len(tensors) == 2 and tensors[0].dim() == 5:
            cats.append(tuple(fcl.layout_of(t) for t in tensors))
        return real_cat(tensors, *a, **kw)

    monkeypatch.setattr(mcl, "bn_apply_cl", rec_bn)
    monkeypatch.setattr(mcl, "cost_volume_cl", rec_cv)
    monkeypatch.setattr(torch, "cat", rec_cat)
    left, right = torch.randn(1, 3, 24, 48, device="cuda"), torch.randn(1, 3, 24, 48, device="cuda")
    out = steps.predict(model, left, right)
    monkeypatch.undo()
    assert out.dtype == torch.float32 and out.shape == (1, 24, 48) and bool(torch.isfinite(out).all())
    with torch.no_grad():
        for xl, has_rem, fmt, (x, scale, shift, rem, relu), got in calls:
            want = BnApplyFunction.apply(x.contiguous(), rem.contiguous() if has_rem else None, scale, shift, relu, False)
            assert got.is_contiguous(memory_format=fmt) and same_bits(got, want), (xl, has_rem, fmt)
        assert len(cvs) == 1
        x, y, maxdisp, got = cvs[0]
        assert got.is_contiguous(memory_format=torch.channels_last_3d) and same_bits(got, GetCostVolumeFunction.apply(x.contiguous(), y.contiguous(), maxdisp))
    sites = collections.Counter((has_rem, fmt) for _, has_rem, fmt, _, _ in calls)
    assert sites == {(False, torch.contiguous_format): 3,                    # conv_start, conv1a, deconv1a.conv2: SGA's inputs
                     (False, torch.channels_last_3d): 4,                     # deconv1a.conv1 and bn_relu behind each of the three SGAs
                     (True, torch.channels_last_3d): 2,                      # the tails of sga1 and sga11
                     (True, torch.contiguous_format): 1}, sites              # the tail of sga2, in front of conv32x1
    # x: planar behind SGA by construction; behind a convolution whatever the library answered (dense either way)
    behind_sga = [c for c in calls if not c[1] and c[2] == torch.channels_last_3d and c[0] == fcl.PLANAR]
    conv_layouts = collections.Counter(c[0] for c in calls)
    assert len(behind_sga) >= 3 and None not in conv_layouts
    assert 3 <= conv_layouts[fcl.PLANAR] <= 10, conv_layouts                 # 3: all seven convolution outputs channels-last; 10: none
    assert len(cats) == 1 and cats[0] == (fcl.CL, fcl.CL), cats
    planar = ms.GANet(12).cuda().eval()
    planar.load_state_dict(first.state_dict())
    fuse.use_fused_ops(planar)
    fuse.use_fused_bn(planar)
    ref = steps.predict(planar, left, right)
    print(f"stand-in: convolution outputs channels-last: {conv_layouts[fcl.PLANAR] == 3}; "
          f"channels-last arm against the planar arm max |dd| {float((out - ref).abs().max()):.3e} (disparities in [0, 12])")


# ---- what PyTorch does with a channels-last convolution ---------------------------------------------------------------------------

_CHILD = """
import json, os, torch
import torch.nn.functional as F
x = torch.randn(1, 8, 5, 6, 8, device="cuda").contiguous(memory_format=torch.channels_last_3d)
w = torch.randn(8, 8, 3, 3, 3, device="cuda").contiguous(memory_format=torch.channels_last_3d)
with torch.no_grad():
    y = F.conv3d(x, w, padding=1)
torch.cuda.synchronize()
print(json.dumps({"switch": os.environ.get("PYTORCH_MIOPEN_SUGGEST_NHWC"),
                  "output_channels_last": bool(y.is_contiguous(memory_format=torch.channels_last_3d)),
                  "output_planar": bool(y.is_contiguous()), "torch": torch.__version__}))
"""


def test_layout_precondition_in_a_child_process(api):
    """a fresh process with PYTORCH_MIOPEN_SUGGEST_NHWC=1 (the switch is read once per process) runs one conv3d on
    channels-last input and weight and reports the output's memory format.  Asserted: that it ran and reported; the answer is
    recorded by scripts/bench_channels_last.py and printed here."""
    env = dict(os.environ, PYTORCH_MIOPEN_SUGGEST_NHWC="1")
    done = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    report = json.loads(done.stdout.strip().splitlines()[-1])
    assert report["switch"] == "1" and isinstance(report["output_channels_last"], bool)
    print("conv3d on channels_last_3d operands with PYTORCH_MIOPEN_SUGGEST_NHWC=1:", report)
