"""The host side of mixed-precision inference (no device): the new modules and functions refuse what they cannot do, and
harness.fuse.use_mixed_precision, run on stand-ins for the reference's classes, rebinds the declared sites and nothing else,
moves no state_dict key, and composes with use_fused_disp_conv in either order."""
import pytest
import torch


def test_exports_and_abi():
    from ganet_amd import _native
    assert _native.ABI_VERSION == 14
    for name in ("ganet_cast", "ganet_bn_apply_forward_mixed", "ganet_cost_volume_forward_16", "ganet_l1_normalize_forward_mixed"):
        assert name in _native.EXPORTS
    from ganet_amd.functions import fused, mixed
    assert set(mixed.__all__) >= {"cast", "bn_apply_mixed", "cost_volume_16", "normalize_guidance_mixed", "normalize_filters_mixed"}
    assert not set(mixed.__all__) & set(fused.__all__)                       # new names beside the old ones
    assert mixed.TYPE_CODE == {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def test_functions_refuse_cpu_tensors_and_wrong_types():
    from ganet_amd.functions import mixed
    h = torch.zeros(1, 20, 4, 6, dtype=torch.bfloat16)
    for call in (lambda: mixed.cast(h, torch.float32), lambda: mixed.normalize_guidance_mixed(h, 1),
                 lambda: mixed.normalize_filters_mixed(h), lambda: mixed.cost_volume_16(h, h, 3),
                 lambda: mixed.bn_apply_mixed(h, None, torch.ones(20), torch.zeros(20))):
        with pytest.raises(RuntimeError, match="HIP"):
            call()


def test_mixed_bn_relu_refuses_training_autograd_and_misuse():
    from ganet_amd.modules.mixed import MixedBnRelu, MixedGetCostVolume
    with pytest.raises(TypeError):
        MixedBnRelu(torch.nn.Conv2d(3, 3, 1))
    with pytest.raises(TypeError):
        MixedBnRelu(torch.nn.BatchNorm2d(3), out_dtype=torch.float64)
    x = torch.zeros(2, 3, 4, 4, dtype=torch.bfloat16)
    bn = torch.nn.BatchNorm2d(3)
    with pytest.raises(RuntimeError, match="BnRelu"):                        # training mode
        MixedBnRelu(bn)(x)
    with pytest.raises(RuntimeError, match="BnRelu"):
        MixedBnRelu(torch.nn.BatchNorm2d(3, track_running_stats=False).eval())(x)
    bn.eval()
    with pytest.raises(RuntimeError, match="BnRelu"):                        # autograd on, parameters want gradients
        MixedBnRelu(bn)(x)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="HIP"):                       # a CPU tensor
            MixedBnRelu(bn)(x)
        with pytest.raises(RuntimeError, match="HIP"):
            MixedGetCostVolume(3)(x, x)
    assert MixedGetCostVolume(3).maxdisp == 4                                # planes, as GetCostVolume(3) counts them
    assert list(MixedBnRelu(bn).state_dict()) == ["bn." + k for k in bn.state_dict()] and MixedBnRelu(bn).bn is bn


# ---- use_mixed_precision on stand-ins -----------------------------------------------------------------------------------------

def _net():
    class BasicConv(torch.nn.Module):
        def __init__(self, cin, cout, is_3d=False, bn=True, relu=True):
            super().__init__()
            self.relu, self.use_bn = relu, bn
            self.conv = (torch.nn.Conv3d if is_3d else torch.nn.Conv2d)(cin, cout, 3, 1, 1, bias=False)
            self.bn = (torch.nn.BatchNorm3d if is_3d else torch.nn.BatchNorm2d)(cout)

    class Conv2x(torch.nn.Module):
        def __init__(self, c):
            super().__init__()
            self.conv1, self.conv2 = BasicConv(c, c, True), BasicConv(2 * c, c, True)

    class SGABlock(torch.nn.Module):
        def __init__(self, c=4):
            super().__init__()
            self.refine = True
            self.bn_relu = torch.nn.Sequential(torch.nn.BatchNorm3d(c), torch.nn.ReLU(inplace=True))
            self.conv_refine = BasicConv(c, c, True, relu=False)

    class Disp(torch.nn.Module):
        def __init__(self, maxdisp=12):
            super().__init__()
            self.maxdisp = maxdisp
            self.conv32x1 = torch.nn.Conv3d(32, 1, 3, 1, 1, bias=False)

    class DispAgg(Disp):
        pass

    class GetCostVolume(torch.nn.Module):
        def __init__(self, maxdisp):
            super().__init__()
            self.maxdisp = maxdisp + 1

    class CostAggregation(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv_start = BasicConv(8, 4, True, relu=False)
            self.conv1a, self.conv2a = BasicConv(4, 4, True), BasicConv(4, 4, True)
            self.deconv1a, self.deconv2a = Conv2x(4), Conv2x(4)
            self.sga1, self.sga2, self.sga11, self.sga12 = SGABlock(), SGABlock(), SGABlock(), SGABlock()
            self.disp0, self.disp1 = Disp(), DispAgg()

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv_x = BasicConv(3, 4)
            self.plain = BasicConv(3, 4, bn=False)
            self.cost_agg = CostAggregation()
            self.cv = GetCostVolume(4)

    net = Net()
    net.cost_agg.disp1.__class__.__name__ = "DispAgg"
    return net


@pytest.mark.parametrize("kernels", [True, False])
def test_use_mixed_precision_rebinds_the_declared_sites_and_nothing_else(kernels):
    from ganet_amd.modules.fused import BnRelu
    from ganet_amd.modules.mixed import MixedBnRelu
    from harness import fuse
    net = _net()
    keys = list(net.state_dict())
    n = fuse.use_mixed_precision(net, torch.bfloat16, kernels=kernels)
    ca = net.cost_agg
    convs = [m for m in net.modules() if type(m).__name__ == "BasicConv" and m.use_bn]
    assert n == len(convs) + 4 + 1 + 2                                       # BasicConvs, SGABlocks, cv, Disp + DispAgg
    assert list(net.state_dict()) == keys
    assert all(not n_.startswith("_") for n_, _ in net.named_modules() if n_) and not any("_mixed" in k or "_fused" in k for k in keys)
    site = MixedBnRelu if kernels else fuse._CastArmBnRelu
    f32 = {id(ca.conv_start), id(ca.conv1a), id(ca.deconv2a.conv2), id(ca.deconv1a.conv2)}
    for m in convs:
        assert isinstance(m._fused_bn, BnRelu) and isinstance(m._mixed_bn, site)          # use_fused_bn came first, and stays
        assert m._mixed_bn.out_dtype == (torch.float32 if id(m) in f32 else None), m
        assert (m._mixed_bn.bn if kernels else m._mixed_bn.op.bn) is m.bn
        assert m.forward.__func__ is fuse._mixed_basicconv_forward
    assert "forward" not in net.plain.__dict__ and "_mixed_bn" not in net.plain.__dict__    # no BatchNorm: not a site
    for m in (ca.sga1, ca.sga2, ca.sga11, ca.sga12):
        assert isinstance(m._mixed_tail, site) and m._mixed_tail.out_dtype is None and m._mixed.kernels is kernels
        assert m.forward.__func__ is fuse._mixed_sgablock_forward and "_fused_sga" in m.__dict__
    assert net.cv.forward.__func__ is fuse._mixed_cv_forward
    assert ca.disp1.forward.__func__ is fuse._mixed_dispagg_forward and ca.disp0.forward.__func__ is fuse._mixed_disp_forward
    for m in net.modules():                                                   # nothing else carries a rebound forward
        if "forward" in m.__dict__:
            assert type(m).__name__ in ("BasicConv", "SGABlock", "GetCostVolume", "Disp", "DispAgg"), type(m).__name__
    with pytest.raises(TypeError):
        fuse.use_mixed_precision(_net(), torch.float32)


def test_use_mixed_precision_rebinds_the_top_level_guidance_branch():
    """on a class named GANet: the plain conv_refine and the Sequential(BatchNorm2d, ReLU) around the bilinear up-sampling"""
    import mixed_standin as ms
    from harness import fuse
    net = ms.GANet(12).eval()
    keys = list(net.state_dict())
    n = fuse.use_mixed_precision(net, torch.bfloat16)
    convs = [m for m in net.modules() if type(m).__name__ == "BasicConv"]
    assert n == len(convs) + 3 + 1 + 1 + 2 and list(net.state_dict()) == keys
    assert net.conv_refine.forward.__func__ is fuse._mixed_top_conv_forward
    assert net.bn_relu.forward.__func__ is fuse._mixed_top_bn_relu_forward
    with torch.no_grad():                                                    # autocast off, fp32: the Sequential as it was
        x = torch.randn(1, 16, 4, 6)
        assert torch.equal(net.bn_relu(x.clone()), torch.relu(net.bn_relu[0](x)))
        assert net.conv_refine(torch.randn(1, 8, 4, 6)).dtype == torch.float32
    assert "forward" not in net.weight_lg["lg1"].__dict__                    # other plain convolutions are not sites


def test_use_mixed_precision_keeps_an_earlier_rebinding():
    from harness import fuse
    net = _net()
    fuse.use_fused_ops(net)
    fuse.use_fused_bn(net)
    sga, bn = net.cost_agg.sga1._fused_sga, net.conv_x._fused_bn
    fuse.use_mixed_precision(net)
    assert net.cost_agg.sga1._fused_sga is sga and net.conv_x._fused_bn is bn


@pytest.mark.parametrize("first", ["mixed", "disp_conv"])
def test_use_mixed_precision_composes_with_use_fused_disp_conv(first):
    from ganet_amd.modules.fused import DispConv
    from harness import fuse
    net = _net()
    keys = list(net.state_dict())
    steps = [lambda: fuse.use_mixed_precision(net), lambda: fuse.use_fused_disp_conv(net)]
    for step in (steps if first == "mixed" else steps[::-1]):
        step()
    for d in (net.cost_agg.disp0, net.cost_agg.disp1):
        assert isinstance(d.conv32x1._fused_conv, DispConv) and d.conv32x1.forward.__func__ is fuse._conv32x1_forward
        assert d.forward.__func__ in (fuse._mixed_disp_forward, fuse._mixed_dispagg_forward)
        # a 16-bit input goes to the convolution the DispConv wraps (here: on the CPU, in bf16), not to the fp32 kernels
        conv = d.conv32x1
        x = torch.randn(1, 32, 3, 4, 5)
        with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
            y = conv(x.bfloat16())
        assert y.dtype == torch.bfloat16 and y.shape == (1, 1, 3, 4, 5)
    assert list(net.state_dict()) == keys


@pytest.mark.parametrize("name,n_sga,producers", [
    ("GANet11", 4, ["conv_start", "conv1a", "deconv1a.conv2", "deconv2a.conv2"]),
    ("GANet_deep", 7, ["conv_start", "conv1a", "deconv1a.conv2", "deconv2a.conv2", "conv1b.conv2", "deconv1b.conv2", "deconv2b.conv2"])])
def test_use_mixed_precision_on_the_reference_models(name, n_sga, producers):
    """the sites on the reference's own two models (where their files are available; no device: nothing is run)"""
    from harness import fuse, refmodel, steps
    if not refmodel.available():
        pytest.skip("no reference model code (GANET_REF_ROOT, /root/reference or oracle/_ref/pyref)")
    model = steps.build_model(name, 48, "cpu")
    keys = list(model.state_dict())
    n = fuse.use_mixed_precision(model, torch.float16)
    assert list(model.state_dict()) == keys
    convs = {k: m for k, m in model.named_modules() if type(m).__name__ == "BasicConv"}
    assert all(m.use_bn and "_mixed_bn" in m.__dict__ for m in convs.values())
    f32 = sorted(k for k, m in convs.items() if m._mixed_bn.out_dtype == torch.float32)
    assert f32 == sorted("cost_agg." + p for p in producers) and len(f32) == n_sga           # one producer per SGABlock
    blocks = [m for m in model.modules() if type(m).__name__ == "SGABlock"]
    assert len(blocks) == n_sga and all(m.forward.__func__ is fuse._mixed_sgablock_forward for m in blocks)
    tails = [m for m in model.modules() if type(m).__name__ in ("Disp", "DispAgg")]
    assert n == len(convs) + n_sga + 1 + len(tails) + 2
    assert model.cv.forward.__func__ is fuse._mixed_cv_forward
    # the top-level guidance branch: torch.autocast runs the bilinear up-sampling between these two in fp32
    assert model.conv_refine.forward.__func__ is fuse._mixed_top_conv_forward
    assert model.bn_relu.forward.__func__ is fuse._mixed_top_bn_relu_forward and model.bn_relu._mixed_bn.bn is model.bn_relu[0]
    rebound = {type(m).__name__ for m in model.modules() if "forward" in m.__dict__}
    assert rebound == {"BasicConv", "SGABlock", "GetCostVolume", "Disp", "DispAgg", "Conv2d", "Sequential"}
    assert sum("forward" in m.__dict__ for m in model.modules() if type(m).__name__ in ("Conv2d", "Sequential")) == 2


def test_predict_signature_and_command_lines():
    import inspect
    from harness import predict as hp, steps
    assert inspect.signature(steps.predict).parameters["amp"].default is None
    assert inspect.signature(steps.predict_images).parameters["amp"].default is None
    args = hp.parse_args(["--left", "a.png", "--right", "b.png", "--out", "o.png", "--amp", "bf16", "--amp_cast_arm"])
    assert args.amp == "bf16" and args.amp_cast_arm
    args = hp.parse_args(["--left", "a.png", "--right", "b.png", "--out", "o.png"])
    assert args.amp is None and not args.amp_cast_arm
