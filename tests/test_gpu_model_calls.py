"""The product, call by call: the reference's models run on the MI355X through the drop-in `libs/` (and through harness.fuse's
call sites) under the recorder of tests/model_calls.py -- steps.predict under no_grad, then one training step -- and EVERY
recorded op call is held to the float64 statement of its operation, evaluated on the tensors that call really got from the
device.  tests/test_gpu_model.py compares whole models with sanity bars on a chaotic system; a failure here names the call.

Per configuration: check_all (SGA: out / mask / A / kp EQUAL to the oracle's, volumes and gradients within 2 x sga_ref64's
bound on the oracle's selections; LGA chains within 2 x lga_ref64.chain_bound; every other op by the statement and bar of
its own case table), the multiset of op kinds the configuration must produce -- a call site that silently fell back to
another form shows as a count -- no input written that the op does not declare consumed, and the gfx950 build, not the
emulator.  tests/test_model_calls_cpu.py shows on the CPU that the oracle itself meets these yardsticks on the same kind of
data and that they reject wrong results.

The GPU work of a test is one model step on a 48x96 crop; the float64 statements then run on the host in numpy (about 1 s
per SGA or LGA2 record).  The second crop (96x240, B = 2: N > 1 and SGA volumes 40 columns wide, a partial 16-column block)
costs ten times that on the host and is run for GANet_deep's stock call forms only."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_DISP = 48
CROP, SECOND_CROP = (48, 96, 1), (96, 240, 2)

# (kinds of steps.predict, kinds of the training step).  Under no_grad SgaFunction takes its inference path: one _sga_infer
# inside each call.  GANet11: four SGA layers; GANet_deep: seven, and three disparity outputs in training mode.
_DEEP_STOCK = ({"GetCostVolumeFunction": 1, "SgaFunction": 7, "_sga_infer": 7, "Lga2Function": 2, "DisparityRegressionFunction": 1},
               {"GetCostVolumeFunction": 1, "SgaFunction": 7, "Lga2Function": 2, "DisparityRegressionFunction": 3, "MyLoss2Function": 1})
EXPECT = {
    ("GANet11", False, False): ({"GetCostVolumeFunction": 1, "SgaFunction": 4, "_sga_infer": 4, "Lga2Function": 2, "DisparityRegressionFunction": 1},
                                {"GetCostVolumeFunction": 1, "SgaFunction": 4, "Lga2Function": 2, "DisparityRegressionFunction": 2, "MyLoss2Function": 1}),
    ("GANet_deep", False, False): _DEEP_STOCK,
    # harness.fuse.use_fused_ops: nine L1 normalisations (seven guidance splits, two LGA filter tensors), the folded BN + ReLU
    # inside the merge kernel and the residual tail under no_grad, three up-samplings and two softmin regressions in training
    ("GANet_deep", True, False): (
        {"GetCostVolumeFunction": 1, "L1NormalizeGroupsFunction": 9, "sga_forward_infer": 7, "_sga_infer": 7, "ResidualReluFunction": 7,
         "TrilinearUpsampleFunction": 1, "Lga2Function": 1, "SoftminFunction": 1, "LgaFunction": 1, "LgaRegressFunction": 1},
        {"GetCostVolumeFunction": 1, "L1NormalizeGroupsFunction": 9, "SgaFunction": 7, "ResidualReluFunction": 7,
         "TrilinearUpsampleFunction": 3, "SoftminDisparityRegressionFunction": 2, "Lga2Function": 1, "SoftminFunction": 1,
         "LgaFunction": 1, "LgaRegressFunction": 1, "DisparityLossFunction": 1}),
    # + use_fused_bn: the 93 BasicConv with a BatchNorm and the seven tails -- folded (BnApply) under no_grad, batch statistics
    # (BnRelu) in training; the tails are no ResidualRelu calls any more
    ("GANet_deep", True, True): (
        {"BnApplyFunction": 100, "GetCostVolumeFunction": 1, "L1NormalizeGroupsFunction": 9, "sga_forward_infer": 7, "_sga_infer": 7,
         "TrilinearUpsampleFunction": 1, "Lga2Function": 1, "SoftminFunction": 1, "LgaFunction": 1, "LgaRegressFunction": 1},
        {"BnReluFunction": 100, "GetCostVolumeFunction": 1, "L1NormalizeGroupsFunction": 9, "SgaFunction": 7,
         "TrilinearUpsampleFunction": 3, "SoftminDisparityRegressionFunction": 2, "Lga2Function": 1, "SoftminFunction": 1,
         "LgaFunction": 1, "LgaRegressFunction": 1, "DisparityLossFunction": 1}),
}


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    sys.path.insert(0, ROOT)
    from harness import refmodel
    if not refmodel.available():
        pytest.skip("no reference model code (GANET_REF_ROOT, /root/reference or oracle/_ref/pyref)")
    return torch


def _run(torch, monkeypatch, oracle, name, crop=CROP, fused_ops=False, fused_bn=False):
    import model_calls as M
    from ganet_amd import _native
    assert not _native.lib().is_simulator
    infer, train = M.run_product(monkeypatch, name, crop, MAX_DISP, "cuda", fused_ops, fused_bn)
    torch.cuda.synchronize()
    want_infer, want_train = EXPECT[name, fused_ops, fused_bn]
    assert dict(M.kinds_of(infer)) == want_infer, ("steps.predict", dict(M.kinds_of(infer)))
    assert dict(M.kinds_of(train)) == want_train, ("training step", dict(M.kinds_of(train)))
    assert all(r.grad_in is None for r in infer) and all(r.grad_in is not None for r in train)
    assert M.undeclared_writes(infer + train) == []
    report = []
    try:
        worst = M.check_all(infer + train, oracle, report=report)
    finally:
        print("\n".join(report))
    tag = f"{name}{' fused_ops' if fused_ops else ''}{' fused_bn' if fused_bn else ''} {crop[0]}x{crop[1]} B={crop[2]}"
    print(f"{tag}: product on the device, largest error / bar per kind and key\n" + M.fmt(worst))
    return infer, train


@pytest.mark.parametrize("name", ["GANet11", "GANet_deep"])
def test_stock_call_forms(env, monkeypatch, port_oracle, name):
    _, train = _run(env, monkeypatch, port_oracle, name)
    assert all(set(r.saved) == {"A", "mask", "kp"} for r in train if r.kind == "SgaFunction")


def test_fused_ops(env, monkeypatch, port_oracle):
    _run(env, monkeypatch, port_oracle, "GANet_deep", fused_ops=True)


def test_fused_ops_and_fused_bn(env, monkeypatch, port_oracle):
    _run(env, monkeypatch, port_oracle, "GANet_deep", fused_ops=True, fused_bn=True)


def test_stock_call_forms_at_the_second_crop_with_two_samples(env, monkeypatch, port_oracle):
    """N = 2, and [2,48,9,16,40] SGA volumes: 40 columns = two 16-column blocks and a partial one"""
    _, train = _run(env, monkeypatch, port_oracle, "GANet_deep", crop=SECOND_CROP)
    shapes = {r.args[0].shape for r in train if r.kind == "SgaFunction"}
    assert shapes == {(2, 32, 17, 32, 80), (2, 48, 9, 16, 40)}, shapes


def test_stock_call_forms_in_recompute_mode(env, monkeypatch, port_oracle):
    """GANET_SGA_SAVE=recompute: the reference's memory profile (A_left and a float mask saved, the rest recomputed); only
    what that mode keeps is compared.  monkeypatch puts the environment back."""
    monkeypatch.setenv("GANET_SGA_SAVE", "recompute")
    _, train = _run(env, monkeypatch, port_oracle, "GANet_deep")
    assert all(set(r.saved) == {"tmp", "mask"} for r in train if r.kind == "SgaFunction")
