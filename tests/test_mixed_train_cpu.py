"""The host side of mixed-precision training (no device): harness.fuse.use_mixed_precision_training rebinds the sites of
use_mixed_precision to forms that carry gradients -- on both real models where the reference exists, on the stand-in network
otherwise -- moves no state_dict key and leaves every old entry point with the refusals it had; the new Functions and modules
refuse what they cannot do; train_step and harness.train take the new keywords with defaults that leave them as they were."""
import inspect

import pytest
import torch


def test_exports_and_names():
    from ganet_amd import _native
    assert _native.ABI_VERSION == 14
    for name in ("ganet_bn_train_forward_mixed", "ganet_bn_train_backward_mixed", "ganet_cost_volume_backward_16",
                 "ganet_l1_normalize_backward_mixed"):
        assert name in _native.EXPORTS
    from ganet_amd.functions import fused, mixed, mixed_train
    from ganet_amd.modules import mixed as mm
    assert set(mixed_train.__all__) == {"MixedBnReluFunction", "CostVolume16Function", "NormalizeGuidanceMixedFunction",
                                        "NormalizeFiltersMixedFunction", "CastFunction"}
    assert not set(mixed_train.__all__) & (set(fused.__all__) | set(mixed.__all__))          # new names beside the old ones
    assert set(mm.__all__) == {"MixedBnRelu", "MixedGetCostVolume", "MixedTrainBnRelu", "MixedTrainGetCostVolume"}


def test_new_functions_and_modules_refuse_what_they_cannot_do():
    from ganet_amd.functions import mixed_train as F
    from ganet_amd.modules.mixed import MixedTrainBnRelu, MixedTrainGetCostVolume
    h = torch.zeros(1, 20, 4, 6, dtype=torch.bfloat16, requires_grad=True)
    for call in (lambda: F.CastFunction.apply(h, torch.float32), lambda: F.NormalizeGuidanceMixedFunction.apply(h, 1),
                 lambda: F.NormalizeFiltersMixedFunction.apply(h), lambda: F.CostVolume16Function.apply(h, h, 3),
                 lambda: F.MixedBnReluFunction.apply(h, None, None, None, None, None, 0.1, 1e-5, True, None)):
        with pytest.raises(RuntimeError, match="HIP"):        # a CPU tensor -- and not "inference only": these carry gradients
            call()
    with pytest.raises(TypeError):
        MixedTrainBnRelu(torch.nn.Conv2d(3, 3, 1))
    with pytest.raises(TypeError):
        MixedTrainBnRelu(torch.nn.BatchNorm2d(3), out_dtype=torch.float64)
    bn = torch.nn.BatchNorm2d(3, momentum=None)
    x = torch.zeros(2, 3, 4, 4, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="momentum=None"):
        MixedTrainBnRelu(bn)(x)
    bn = torch.nn.BatchNorm2d(3)
    with pytest.raises(RuntimeError, match="HIP"):            # training mode reaches the Function (MixedBnRelu would refuse the mode)
        MixedTrainBnRelu(bn)(x)
    bn.eval()
    with pytest.raises(RuntimeError, match="BnRelu"):         # eval mode is MixedBnRelu's fold, with its refusals
        MixedTrainBnRelu(bn)(x)
    assert list(MixedTrainBnRelu(bn).state_dict()) == ["bn." + k for k in bn.state_dict()] and MixedTrainBnRelu(bn).bn is bn
    assert [k for k, _ in MixedTrainBnRelu(bn).named_modules()] == ["", "bn"]
    assert MixedTrainGetCostVolume(3).maxdisp == 4


def _check_sites(model, n_sga, producers, kernels, top):
    from ganet_amd.modules.fused import BnRelu
    from ganet_amd.modules.mixed import MixedTrainBnRelu
    from harness import fuse
    keys = list(model.state_dict())
    n = fuse.use_mixed_precision_training(model, torch.float16, kernels=kernels)
    assert list(model.state_dict()) == keys
    assert all(not k.split(".")[-1].startswith("_") for k, _ in model.named_modules() if k)
    site = MixedTrainBnRelu if kernels else fuse._CastArmBnRelu
    convs = {k: m for k, m in model.named_modules() if type(m).__name__ == "BasicConv" and m.use_bn}
    for m in convs.values():
        assert isinstance(m._fused_bn, BnRelu) and isinstance(m._mixed_bn, site)
        assert (m._mixed_bn.bn if kernels else m._mixed_bn.op.bn) is m.bn
        assert m.forward.__func__ is fuse._mixed_train_basicconv_forward
    f32 = sorted(k for k, m in convs.items() if m._mixed_bn.out_dtype == torch.float32)
    assert f32 == sorted("cost_agg." + p for p in producers) and len(f32) == n_sga           # one fp32 producer per SGABlock
    blocks = [m for m in model.modules() if type(m).__name__ == "SGABlock"]
    assert len(blocks) == n_sga
    for m in blocks:
        assert m.forward.__func__ is fuse._mixed_train_sgablock_forward and isinstance(m._mixed_tail, site)
        assert m._mixed_tail.out_dtype is None and m._mixed.kernels is kernels and "_fused_sga" in m.__dict__
        if m.refine:                                      # bn_relu behind SGA (fp32 in and out): BnRelu on both arms
            assert isinstance(m._mixed_bnrelu, BnRelu) and m._mixed_bnrelu.bn is m.bn_relu[0] and m._mixed_bnrelu.relu
        else:
            assert "_mixed_bnrelu" not in m.__dict__
    tails = [m for m in model.modules() if type(m).__name__ in ("Disp", "DispAgg")]
    for m in tails:
        want = fuse._mixed_train_dispagg_forward if type(m).__name__ == "DispAgg" else fuse._mixed_disp_forward
        assert m.forward.__func__ is want and isinstance(m._mixed, fuse._MixedTrainOps)
    assert model.cv.forward.__func__ is fuse._mixed_cv_forward and isinstance(model.cv._mixed, fuse._MixedTrainOps)
    assert n == len(convs) + n_sga + 1 + len(tails) + (2 if top else 0)
    rebound = {type(m).__name__ for m in model.modules() if "forward" in m.__dict__}
    assert rebound == {"BasicConv", "SGABlock", "GetCostVolume", "Disp", "DispAgg"} | ({"Conv2d", "Sequential"} if top else set())
    if top:
        assert model.conv_refine.forward.__func__ is fuse._mixed_top_conv_forward
        assert model.bn_relu.forward.__func__ is fuse._mixed_train_top_bn_relu_forward
        assert isinstance(model.bn_relu._mixed_bn, BnRelu) and model.bn_relu._mixed_bn.bn is model.bn_relu[0]     # the cast arm on both settings


REAL = [("GANet11", 4, ["conv_start", "conv1a", "deconv1a.conv2", "deconv2a.conv2"]),
        ("GANet_deep", 7, ["conv_start", "conv1a", "deconv1a.conv2", "deconv2a.conv2", "conv1b.conv2", "deconv1b.conv2", "deconv2b.conv2"])]


@pytest.mark.parametrize("kernels", [True, False])
@pytest.mark.parametrize("name,n_sga,producers", REAL)
def test_sites_on_the_models(name, n_sga, producers, kernels):
    """both real models where the reference's files are available, the stand-in network (four SGABlocks) otherwise: nothing is run"""
    from harness import refmodel, steps
    if refmodel.available():
        _check_sites(steps.build_model(name, 48, "cpu"), n_sga, producers, kernels, top=True)
    else:
        import standin_net
        # (its four SGABlocks are sga1 / sga11 / sga2 / sga3: the producers fuse._SGA_PRODUCER names for them)
        _check_sites(standin_net.build(48), 4, ["conv_start", "conv1a", "deconv1a.conv2", "deconv1b.conv2"], kernels, top=False)


def test_old_entry_points_keep_their_refusals_on_a_prepared_model():
    """a model prepared by the new function still gives the old error texts from the old entry points"""
    import standin_net
    from ganet_amd.functions import mixed
    from ganet_amd.modules.mixed import MixedBnRelu
    from harness import fuse
    model = standin_net.build(48)
    fuse.use_mixed_precision_training(model)
    bn = model.feature.bn
    x = torch.zeros(1, bn.num_features, 4, 4, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="inference only.*use BnRelu on fp32 tensors for training"):
        MixedBnRelu(bn)(x)                                                    # training mode
    with pytest.raises(RuntimeError, match="HIP"):
        mixed.cast(x, torch.float32)
    xg = torch.zeros(1, 20, 4, 6, dtype=torch.bfloat16, requires_grad=True)
    for call in (lambda: mixed.normalize_guidance_mixed(xg, 1), lambda: mixed.cost_volume_16(xg, xg, 3)):
        with pytest.raises(RuntimeError, match="HIP"):                        # (the device check comes first, as before)
            call()
    assert "is inference only and keeps nothing for backward" in inspect.getsource(mixed._check_mixed)
    with pytest.raises(RuntimeError, match="use_mixed_precision is for inference"):
        fuse._inference_only(model.train())
    with pytest.raises(TypeError):
        fuse.use_mixed_precision_training(standin_net.build(48), torch.float32)
    assert fuse.use_mixed_precision(standin_net.build(48)) > 0      # the inference rebinder itself is untouched by the new one


def test_train_step_and_command_line_take_the_new_keywords():
    import sys
    from harness import steps, train
    sig = inspect.signature(steps.train_step).parameters
    assert sig["amp"].default is None and sig["scaler"].default is None
    assert list(sig)[:9] == ["model", "optimizer", "name", "left", "right", "target", "max_disp", "crit", "fused_loss"]
    argv = sys.argv
    try:
        sys.argv = ["train", "--amp", "fp16", "--amp_cast_arm"]
        a = train.parse()
        assert a.amp == "fp16" and a.amp_cast_arm
        sys.argv = ["train"]
        a = train.parse()
        assert a.amp == "" and not a.amp_cast_arm
    finally:
        sys.argv = argv
