"""The host side of DispConv without a device: harness.fuse.use_fused_disp_conv on the reference's models (where they are
importable) and on stand-ins, the module's refusals, and the "no CPU path" error.  The kernels: tests/test_sim_disp_conv.py
(emulator) and tests/test_gpu_disp_conv.py (device)."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from harness import fuse, refmodel  # noqa: E402

needs_models = pytest.mark.skipif(not refmodel.available(), reason="no reference model code (harness.refmodel.available())")


def _sites(model):
    return [m.conv32x1 for m in model.modules() if type(m).__name__ in ("Disp", "DispAgg")]


def _check_rebound(model, keys, params, n):
    from ganet_amd.modules.fused import DispConv
    assert list(model.state_dict()) == keys
    assert [id(p) for p in model.parameters()] == params
    sites = _sites(model)
    assert len(sites) == n
    for conv in sites:
        helper = conv.__dict__["_fused_conv"]
        assert isinstance(helper, DispConv) and helper.conv is conv and helper.conv.weight is conv.weight
        assert "forward" in conv.__dict__ and "_fused_conv" not in conv._modules


@needs_models
@pytest.mark.parametrize("name,n", [("GANet_deep", 3), ("GANet11", 2)])
def test_use_fused_disp_conv_on_the_reference_models(name, n):
    """site counts, state_dict keys and parameter identities; alone, and in every order with the other two rebinders"""
    from harness import steps
    orders = [("conv",), ("ops", "conv"), ("conv", "ops"), ("tail", "conv"), ("conv", "tail"), ("ops", "tail", "conv"),
              ("conv", "ops", "tail")]
    for order in orders:
        torch.manual_seed(0)
        model = steps.build_model(name, 48, "cpu")
        keys, params = list(model.state_dict()), [id(p) for p in model.parameters()]
        for step in order:
            if step == "conv":
                assert fuse.use_fused_disp_conv(model) == n
            elif step == "ops":
                assert fuse.use_fused_ops(model) > n
            else:
                assert fuse.use_fused_disp_tail(model) == n - 1       # every Disp; the DispAgg is not its business
        _check_rebound(model, keys, params, n)
        # whichever forward the owner has now, it reaches the convolution through self.conv32x1(x): the rebound instance
        for m in model.modules():
            if type(m).__name__ in ("Disp", "DispAgg"):
                with pytest.raises(RuntimeError, match="no CPU path"):
                    m.conv32x1(torch.zeros(1, 32, 2, 3, 4))


class _Disp(torch.nn.Module):
    def __init__(self, maxdisp=12):
        super().__init__()
        self.maxdisp = maxdisp
        self.conv32x1 = torch.nn.Conv3d(32, 1, (3, 3, 3), (1, 1, 1), (1, 1, 1), bias=False)


def _stand_in():
    Disp = type("Disp", (_Disp,), {})
    DispAgg = type("DispAgg", (_Disp,), {})

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.disp0, self.disp1, self.disp2 = Disp(), Disp(), DispAgg()
            self.other = torch.nn.Conv3d(32, 1, 3, 1, 1, bias=False)          # not a conv32x1 of a tail: left alone
    return Net()


@pytest.mark.parametrize("order", [("conv",), ("ops", "conv"), ("conv", "ops"), ("tail", "conv"), ("conv", "tail"),
                                   ("conv", "ops", "tail")], ids="-".join)
def test_use_fused_disp_conv_on_a_stand_in(order):
    net = _stand_in()
    keys, params = list(net.state_dict()), [id(p) for p in net.parameters()]
    for step in order:
        if step == "conv":
            assert fuse.use_fused_disp_conv(net) == 3
        elif step == "ops":
            assert fuse.use_fused_ops(net) == 3
        else:
            assert fuse.use_fused_disp_tail(net) == 2
    _check_rebound(net, keys, params, 3)
    assert "forward" not in net.other.__dict__
    import copy
    twin = copy.deepcopy(net)                               # the helper and its convolution refer to each other: still copyable
    assert list(twin.state_dict()) == keys and twin.disp0.conv32x1._fused_conv.conv is twin.disp0.conv32x1


def test_use_fused_ops_does_not_call_it():
    net = _stand_in()
    fuse.use_fused_ops(net)
    fuse.use_fused_disp_tail(net)
    assert all("forward" not in c.__dict__ and "_fused_conv" not in c.__dict__ for c in _sites(net))


def test_directions_flag():
    net = _stand_in()
    assert fuse.use_fused_disp_conv(net, directions=("forward", "data")) == 3
    assert all(c._fused_conv.directions == ("forward", "data") for c in _sites(net))
    with pytest.raises(ValueError):
        fuse.use_fused_disp_conv(_stand_in(), directions=("sideways",))


def test_cpu_tensor_raises_no_cpu_path():
    from ganet_amd.functions.fused import DispConvFunction
    from ganet_amd.modules.fused import DispConv
    with pytest.raises(RuntimeError, match="no CPU path"):
        DispConvFunction.apply(torch.zeros(1, 2, 3, 4, 5), torch.zeros(1, 2, 3, 3, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        DispConv(torch.nn.Conv3d(2, 1, 3, 1, 1, bias=False))(torch.zeros(1, 2, 3, 4, 5))


@pytest.mark.parametrize("what,conv", [
    ("out_channels", lambda: torch.nn.Conv3d(32, 2, 3, 1, 1, bias=False)),
    ("kernel_size", lambda: torch.nn.Conv3d(32, 1, (3, 3, 1), 1, (1, 1, 0), bias=False)),
    ("kernel_size", lambda: torch.nn.Conv3d(32, 1, 5, 1, 2, bias=False)),
    ("stride", lambda: torch.nn.Conv3d(32, 1, 3, 2, 1, bias=False)),
    ("padding", lambda: torch.nn.Conv3d(32, 1, 3, 1, 0, bias=False)),
    ("padding_mode", lambda: torch.nn.Conv3d(32, 1, 3, 1, 1, bias=False, padding_mode="replicate")),
    ("dilation", lambda: torch.nn.Conv3d(32, 1, 3, 1, 1, dilation=2, bias=False)),
    ("bias", lambda: torch.nn.Conv3d(32, 1, 3, 1, 1, bias=True)),
    ("at most 64", lambda: torch.nn.Conv3d(65, 1, 3, 1, 1, bias=False)),
])
def test_module_refuses_any_other_geometry(what, conv):
    from ganet_amd.modules.fused import DispConv
    with pytest.raises(AssertionError, match=what):
        DispConv(conv())


def test_module_refuses_what_is_no_conv3d_and_takes_the_models_own():
    from ganet_amd.modules.fused import DispConv
    with pytest.raises(TypeError):
        DispConv(torch.nn.Conv2d(32, 1, 3, 1, 1, bias=False))
    conv = torch.nn.Conv3d(32, 1, (3, 3, 3), (1, 1, 1), (1, 1, 1), bias=False)
    assert DispConv(conv).conv.weight is conv.weight
    # groups = 1 is implied by out_channels = 1; transposed convolutions are another class
    with pytest.raises(TypeError):
        DispConv(torch.nn.ConvTranspose3d(32, 1, 3, 1, 1, bias=False))


def test_flags_exist():
    from harness import train
    assert train.parse(["--fused_conv32"]).fused_conv32 and not train.parse([]).fused_conv32
    src = open(os.path.join(ROOT, "harness", "infer.py")).read()
    assert '"--fused_conv32"' in src and "fuse.use_fused_disp_conv(model)" in src
