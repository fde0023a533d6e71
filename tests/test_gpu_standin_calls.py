"""The product, call by call, on a model that travels: the stand-in network of tests/standin_net.py runs on the MI355X under the
recorder of tests/model_calls.py -- steps.predict under no_grad, then one training step -- un-rebound and under the rebinders
of harness.fuse, alone and chained, and EVERY recorded op call is held to the float64 statement of its operation, evaluated
on the tensors that call really got from the device.  tests/test_gpu_model_calls.py does the same on the reference's models
and skips where their files are missing; this file needs none of them and never skips.

Per case, as there: the gfx950 build, not the emulator; the multiset of op kinds the case must produce (a call site that
silently fell back to another form shows as a count); no input written that the op does not declare; no incoming gradient
under predict and one on every training record; check_all.  tests/test_model_calls_cpu.py calibrates every bar used here on
the CPU, on the same network's data, and ties the network's blocks to the reference's.

The census of tests/standin_net.py that the expected multisets are written from:
  SGABlock   3 with refine (sga1, sga11, sga2: bn_relu + conv_refine) and 1 without (sga3: its own bn)
  BasicConv  with a BatchNorm, CALLS per forward outside the SGABlocks: feature twice (left, right), guide_small, guide_down,
             guide_full, conv_start, conv1a and two each in deconv1a, conv1b, deconv1b = 13; the 3 conv_refine are called by
             the stock SGABlock.forward only (the rebound one calls conv_refine.conv and hands its bn to the tail)
  tails      2 Disp (training mode only) and 1 DispAgg, one conv32x1 each
The GPU work of a case is one small model step; the float64 statements then run on the host in numpy."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_DISP = 48
CROP, SECOND_CROP = (48, 96, 1), (96, 240, 2)

OPS, BN, TAIL, CONV = "use_fused_ops", "use_fused_bn", "use_fused_disp_tail", "use_fused_disp_conv"

# (kinds of steps.predict, kinds of the training step)
_STOCK = (
    {"GetCostVolumeFunction": 1,               # GANet.cv
     "SgaFunction": 4, "_sga_infer": 4,        # four SGABlocks; under no_grad SgaFunction takes its inference path, one _sga_infer inside
     "Lga2Function": 2,                        # DispAgg: lga(x, lg1), lga(x, lg2)
     "DisparityRegressionFunction": 1},        # eval mode: the DispAgg alone
    {"GetCostVolumeFunction": 1,
     "SgaFunction": 4,
     "Lga2Function": 2,
     "DisparityRegressionFunction": 3,         # training mode: two Disp and the DispAgg
     "MyLoss2Function": 1})                    # steps.loss_mix: MyLoss2 on the last map (the two smooth-L1 terms are torch's)
_OPS = (
    {"GetCostVolumeFunction": 1,
     "L1NormalizeGroupsFunction": 6,           # four guidance splits, two LGA filter tensors
     "sga_forward_infer": 3,                   # GuidedSGABnRelu (refine): the folded bn_relu inside the merge kernel
     "SgaFunction": 1,                         # GuidedSGA (sga3) calls SgaFunction, which under no_grad ...
     "_sga_infer": 4,                          # ... goes through _sga_infer, as the three sga_forward_infer do
     "ResidualReluFunction": 4,                # every SGABlock's tail, folded
     "TrilinearUpsampleFunction": 1, "Lga2Function": 1, "SoftminFunction": 1, "LgaFunction": 1, "LgaRegressFunction": 1},      # DispAggTail
    {"GetCostVolumeFunction": 1,
     "L1NormalizeGroupsFunction": 6,
     "SgaFunction": 4,                         # training: bn_relu stays the framework's
     "ResidualReluFunction": 4,                # relu(bn(t) + rem) on the framework's bn(t)
     "TrilinearUpsampleFunction": 3,           # two Disp and the DispAgg
     "SoftminDisparityRegressionFunction": 2,  # the two Disp
     "Lga2Function": 1, "SoftminFunction": 1, "LgaFunction": 1, "LgaRegressFunction": 1,
     "DisparityLossFunction": 1})
_N_BN = 13 + 4                                 # BasicConv calls + the four SGABlock tails, which are no ResidualRelu calls any more


def _without(kinds, *names):
    return {k: v for k, v in kinds.items() if k not in names}


_OPS_BN = ({**_without(_OPS[0], "ResidualReluFunction"), "BnApplyFunction": _N_BN},       # folded under no_grad
           {**_without(_OPS[1], "ResidualReluFunction"), "BnReluFunction": _N_BN})        # batch statistics in training
_ALL = (
    {**_OPS_BN[0], "DispConvFunction": 1},                                                # the DispAgg's conv32x1
    {**_without(_OPS_BN[1], "SoftminDisparityRegressionFunction"),
     "TrilinearUpsampleFunction": 1,           # the DispAgg's alone: DispTail up-samples inside
     "UpSoftminRegressionFunction": 2,         # the two Disp
     "DispConvFunction": 3})
EXPECT = {
    "stock": ((), _STOCK),
    "ops": ((OPS,), _OPS),
    "ops+bn": ((OPS, BN), _OPS_BN),
    # Disp is not reached in eval mode; any rebound form trains on the fused DisparityLoss
    "tail": ((TAIL,), (_STOCK[0], {**_without(_STOCK[1], "MyLoss2Function"), "DisparityRegressionFunction": 1,
                                   "UpSoftminRegressionFunction": 2, "DisparityLossFunction": 1})),
    "conv": ((CONV,), ({**_STOCK[0], "DispConvFunction": 1},
                       {**_without(_STOCK[1], "MyLoss2Function"), "DispConvFunction": 3, "DisparityLossFunction": 1})),
    "all": ((OPS, BN, TAIL, CONV), _ALL),
    "all-reversed": ((CONV, TAIL, OPS, BN), _ALL),
}


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    sys.path.insert(0, ROOT)
    return torch


def _run(torch, monkeypatch, oracle, case, crop=CROP):
    import model_calls as M
    import standin_net
    from ganet_amd import _native
    from harness import steps
    assert not _native.lib().is_simulator
    rebinders, (want_infer, want_train) = EXPECT[case]
    H, W, B = crop
    model = standin_net.build(MAX_DISP, "cuda")
    keys = list(model.state_dict())
    infer, train = M.run_model(monkeypatch, model, steps.synthetic_batch(B, H, W, MAX_DISP, "cuda"), MAX_DISP, rebinders)
    torch.cuda.synchronize()
    assert list(model.state_dict()) == keys
    assert dict(M.kinds_of(infer)) == want_infer, ("steps.predict", dict(M.kinds_of(infer)))
    assert dict(M.kinds_of(train)) == want_train, ("training step", dict(M.kinds_of(train)))
    assert all(r.grad_in is None for r in infer) and all(r.grad_in is not None for r in train)
    assert M.undeclared_writes(infer + train) == []
    report = []
    try:
        worst = M.check_all(infer + train, oracle, report=report)
    finally:
        print("\n".join(report))
    print(f"stand-in {case} {H}x{W} B={B}: product on the device, largest error / bar per kind and key\n" + M.fmt(worst))
    sga = sorted({r.args[0].shape for r in train if r.kind == "SgaFunction"})
    h, w = H // 3, W // 3
    assert sga == sorted({(B, standin_net.C, MAX_DISP // 3 + 1, h, w), (B, standin_net.C, MAX_DISP // 6 + 1, h // 2, w // 2)}), sga
    return infer, train, model


@pytest.mark.parametrize("case", list(EXPECT))
def test_every_op_call_of_a_step(env, monkeypatch, port_oracle, case):
    """48 x 96, B = 1: SGA on [1,8,17,16,32] (W % 16 == 0 and H % 4 == 0: the tiled adjoint workspace) and [1,8,9,8,16], LGA on
    [1,49,48,96] with radius 2, DispConv on [1,8,17,16,32]"""
    _, train, _ = _run(env, monkeypatch, port_oracle, case)
    assert all(set(r.saved) == {"A", "mask", "kp"} for r in train if r.kind == "SgaFunction")
    lga = {r.args[0].shape for r in train if r.kind in ("Lga2Function", "LgaFunction", "LgaRegressFunction")}
    assert lga == {(1, MAX_DISP + 1, 48, 96)}, lga
    conv = {r.args[0].shape for r in train if r.kind == "DispConvFunction"}
    assert conv <= {(1, 8, 17, 16, 32)}, conv


def test_the_rebinders_in_either_order(env, monkeypatch, port_oracle):
    """"all" and "all-reversed" share one expected multiset (asserted by their cases above); here: every rebound site holds a
    helper of the same type after either order, on the device model"""
    import standin_net
    from harness import fuse
    assert EXPECT["all"][1] is EXPECT["all-reversed"][1] and sorted(EXPECT["all"][0]) == sorted(EXPECT["all-reversed"][0])
    held = []
    for rebinders, _ in (EXPECT["all"], EXPECT["all-reversed"]):
        model = standin_net.build(MAX_DISP, "cuda")
        for rb in rebinders:
            assert getattr(fuse, rb)(model) > 0
        held.append({(name, h): (type(m.__dict__[h]).__name__, getattr(m.__dict__.get("forward"), "__func__", None))
                     for name, m in model.named_modules() for h in ("_fused_sga", "_fused_tail", "_fused_bn", "_fused_conv") if h in m.__dict__})
    assert held[0] == held[1] and len(held[0]) == 4 + 4 + 3 + 15 + 3       # GuidedSGA*, the blocks' and tails' _fused_tail, BnRelu, DispConv


def test_stock_call_forms_in_recompute_mode(env, monkeypatch, port_oracle):
    """GANET_SGA_SAVE=recompute: A_left and a float mask saved, the rest recomputed; only what that mode keeps is compared.
    monkeypatch puts the environment back."""
    monkeypatch.setenv("GANET_SGA_SAVE", "recompute")
    _, train, _ = _run(env, monkeypatch, port_oracle, "stock")
    assert all(set(r.saved) == {"tmp", "mask"} for r in train if r.kind == "SgaFunction")


@pytest.mark.parametrize("case", ["stock", "all"])
def test_the_second_crop_with_two_samples(env, monkeypatch, port_oracle, case):
    """96 x 240, B = 2: N > 1, and SGA volumes [2,8,17,32,80] and [2,8,9,16,40] -- 40 columns: two 16-column blocks and a partial
    one (asserted in _run).  The device step is as short as at the first crop; the host side is not (16 - 19 s per case):
    nearly all of it is lga_ref64.chain_bound on the [2,49,96,240] LGA volumes, whose size the crop and max_disp fix -- the
    network's channel count does not enter it (the four SGA records together take under 2 s)."""
    _, train, _ = _run(env, monkeypatch, port_oracle, case, crop=SECOND_CROP)
    assert any(r.args[0].shape[-1] % 16 for r in train if r.kind == "SgaFunction")


def _seeded_images(h, w, first_seed=0):
    """two uint8 images whose quotients keep io_ref64.MARGIN from every rounding boundary of float32 (io_cases' premise, decided
    here on the host): the first seed for which they do"""
    import numpy as np
    import io_ref64
    for seed in range(first_seed, first_seed + 16):
        rng = np.random.default_rng(seed)
        left, right = (rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(2))
        if io_ref64.margin(left, right) >= io_ref64.MARGIN:
            return left, right, seed
    raise AssertionError("no seed keeps the margin")


def test_predict_images_front_and_back_end(env, monkeypatch, port_oracle):
    """steps.predict_images on two seeded uint8 images smaller than the crop (padded to the bottom-right, un-padded again):
    stereo_input and disparity_to_u16 bit for bit against io_ref64 on the recorded arguments, every op call between them as
    above; the training target's window_f32 under the same recorder"""
    torch = env
    import numpy as np
    import io_ref64
    import model_calls as M
    import standin_net
    from ganet_amd.modules.fused import StereoInput
    from harness import steps
    left, right, seed = _seeded_images(45, 90)
    assert io_ref64.margin(left, right) >= io_ref64.MARGIN, seed
    model = standin_net.build(MAX_DISP, "cuda")
    disp = np.random.default_rng(1).uniform(0, MAX_DISP, (45, 90)).astype(np.float32)
    with M.recording(monkeypatch, *M.product_functions()) as records:
        out = steps.predict_images(model, torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda(), CROP[:2])
        StereoInput(*CROP[:2]).target_window(torch.from_numpy(disp).cuda(), -3, -6, sub=2.0, fill=998.0)
    torch.cuda.synchronize()
    assert out.dtype == torch.uint16 and tuple(out.shape) == (45, 90)
    kinds = dict(M.kinds_of(records))
    assert kinds == {"stereo_input": 1, **EXPECT["stock"][1][0], "disparity_to_u16": 1, "window_f32": 1}, kinds
    assert records[0].kind == "stereo_input" and records[-2].kind == "disparity_to_u16" and records[-1].kind == "window_f32"
    assert M.undeclared_writes(records) == []
    report = []
    try:
        worst = M.check_all(records, port_oracle, report=report)
    finally:
        print("\n".join(report))
    print(f"stand-in predict_images (seed {seed}): largest error / bar per kind and key\n" + M.fmt(worst))
    assert int(out.cpu().numpy().max()) > 0
