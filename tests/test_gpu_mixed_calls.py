"""A mixed-precision step, call by call: the stand-in network of tests/standin_net.py, prepared by harness.fuse.use_mixed_precision
resp. use_mixed_precision_training, runs harness.steps.predict(amp=) resp. steps.train_step(amp=, scaler=) THEMSELVES on the MI355X
under the recorder of tests/model_calls.py, and EVERY recorded op call -- the 16-bit-storage forms of ganet_amd.functions.mixed and
mixed_train, and the fp32 ops between them, which under autocast get rounded activations and, under fp16, gradients that carry the
GradScaler's scale -- is held to the float64 statement of its operation on the tensors that call really got from the device.
tests/test_gpu_standin_calls.py does this for the fp32 step; tests/test_model_calls_cpu.py calibrates the mixed checkers on a numpy
model and shows that they reject a zero, a truncated, a doubly rounded and a mis-scaled result and a left-out term.

Per case: the gfx950 build, not the emulator; the multiset of recorded kinds (a site that silently fell back to fp32 or to ATen
shows as a count); no input written that its op does not declare; gradients on every training Function record and on no
inference record; every 16-bit tensor of every record in the case's format; check_all.  fp16 trains under
GradScaler(init_scale=256): the last op's incoming gradient is the scale, exactly, and every parameter's .grad is finite after
the step.

The census the expected multisets are written from (tests/test_gpu_standin_calls.py's, and harness/fuse.py's site list):
  the images           2 `cast` by the harness itself (steps.predict / steps.train_step), on either arm
  BasicConv            13 calls outside the SGABlocks, 4 of them in front of an SGABlock (conv_start, conv1a, deconv1a.conv2,
                       deconv1b.conv2: fp32 out); + the 3 tails behind a conv_refine (fp32 residual, 16-bit out) = 16 sites on
                       16-bit storage
  SGABlock             4 guidance normalisations, 4 SGA; bn_relu behind SGA (3, refine) and sga3's own bn + residual (1) see fp32
                       on both sides and stay BnRelu / BnApply: 4
  GANet.cv             1
  Disp (2, training) and DispAgg (1): conv32x1's 16-bit output up-cast, 1 cast each; the DispAgg's 2 filter normalisations.
                       A DispConv hands a 16-bit input to the convolution itself (ganet_amd.modules.fused.DispConv), so
                       DispConvFunction is not reached under autocast and use_fused_disp_conv is not applied here.
  the cast arm         (kernels=False) the fp32 Functions between ATen casts: nothing 16-bit is recorded but the harness's 2 casts;
                       these cases run with use_fused_disp_tail, so that both forms of the Disp tail are seen under autocast.
  the guidance branch  tests/mixed_standin.py, inference: GANet.conv_refine's 16-bit output up-cast (a third `cast` site) and
                       GANet.bn_relu, fp32 in and 16 bits out (a thirteenth bn_apply_mixed, the one form that reads fp32);
                       the training-capable stand-in has neither site
The GPU work of a case is one small model step; the float64 statements then run on the host in numpy."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_DISP = 48
CROP, SECOND_CROP = (48, 96, 1), (96, 240, 2)
SCALE = 256.0
TAIL = "use_fused_disp_tail"

_DISPAGG = {"TrilinearUpsampleFunction": 1, "Lga2Function": 1, "SoftminFunction": 1, "LgaFunction": 1, "LgaRegressFunction": 1}
INFER_KERNELS = {
    "cast": 2 + 1,                             # the two images; the DispAgg's conv32x1 output
    "bn_apply_mixed": 13 + 3,
    "BnApplyFunction": 1,                      # sga3's bn + residual: fp32 in and out
    "cost_volume_16": 1,
    "normalize_guidance_mixed": 4, "sga_forward_infer": 4, "_sga_infer": 4,
    "normalize_filters_mixed": 2,
    **_DISPAGG}
# tests/mixed_standin.py (inference only, 4 channels, three SGABlocks with refine, one DispAgg): the reference's top-level guidance
# branch -- a plain convolution whose 16-bit output is up-cast in front of a bilinear up-sampling, and a Sequential(BatchNorm2d,
# ReLU) behind it that reads fp32 and writes 16 bits
INFER_GUIDANCE_BRANCH = {
    "cast": 2 + 1 + 1,                         # the images; GANet.conv_refine's output; the DispAgg's conv32x1 output
    "bn_apply_mixed": 9 + 3 + 1,               # BasicConv calls (feature twice); the SGABlocks' tails; GANet.bn_relu
    "cost_volume_16": 1,
    "normalize_guidance_mixed": 3, "sga_forward_infer": 3, "_sga_infer": 3,
    "normalize_filters_mixed": 2,
    **_DISPAGG}
GUIDANCE_MAX_DISP, GUIDANCE_CROP = 12, (24, 48, 1)
TRAIN_KERNELS = {
    "cast": 2,
    "MixedBnReluFunction": 13 + 3,
    "BnReluFunction": 3 + 1,                   # bn_relu behind SGA; sga3's bn + residual
    "CostVolume16Function": 1,
    "NormalizeGuidanceMixedFunction": 4, "SgaFunction": 4,
    "CastFunction": 3,                         # conv32x1's output in two Disp and the DispAgg
    "NormalizeFiltersMixedFunction": 2,
    **_DISPAGG, "TrilinearUpsampleFunction": 3,
    "SoftminDisparityRegressionFunction": 2,
    "DisparityLossFunction": 1}
TRAIN_CAST_ARM = {                             # with use_fused_disp_tail
    "cast": 2,
    "BnReluFunction": 16 + 4,
    "GetCostVolumeFunction": 1,
    "L1NormalizeGroupsFunction": 4 + 2, "SgaFunction": 4,
    **_DISPAGG,
    "UpSoftminRegressionFunction": 2,
    "DisparityLossFunction": 1}


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    sys.path.insert(0, ROOT)
    return torch


def _run(torch, monkeypatch, oracle, mixed, fmt, kernels=True, rebinders=(), crop=CROP, guidance_branch=False):
    import mixed_cases as mxc
    import model_calls as M
    import standin_net
    from ganet_amd import _native
    from harness import steps
    assert not _native.lib().is_simulator
    dt = {mxc.BF16: torch.bfloat16, mxc.F16: torch.float16}[fmt]
    H, W, B = crop
    if guidance_branch:
        import mixed_standin
        torch.manual_seed(9)
        max_disp, model = GUIDANCE_MAX_DISP, mixed_standin.GANet(GUIDANCE_MAX_DISP).cuda()
    else:
        max_disp, model = MAX_DISP, standin_net.build(MAX_DISP, "cuda")
    keys = list(model.state_dict())
    scaler = torch.amp.GradScaler("cuda", init_scale=SCALE) if mixed == "train" and fmt == mxc.F16 else None
    infer, train = M.run_model(monkeypatch, model, steps.synthetic_batch(B, H, W, max_disp, "cuda"), max_disp, rebinders,
                               amp=dt, scaler=scaler, mixed=mixed, kernels=kernels)
    torch.cuda.synchronize()
    assert list(model.state_dict()) == keys
    records = infer + train
    what = f"stand-in{' with the guidance branch' if guidance_branch else ''} {mixed} {mxc.FMT_NAME[fmt]} kernels={kernels} {H}x{W} B={B}"
    print(f"{what}: recorded kinds {dict(M.kinds_of(records))}")
    want = INFER_GUIDANCE_BRANCH if guidance_branch else (INFER_KERNELS if mixed == "infer" else TRAIN_KERNELS) if kernels else TRAIN_CAST_ARM
    assert dict(M.kinds_of(records)) == want, (what, dict(M.kinds_of(records)))
    assert M.undeclared_writes(records) == []
    assert all(r.grad_in is None and r.grad_out is None for r in infer)
    assert [r.kind for r in records[:2]] == ["cast", "cast"] and all(not isinstance(r.args[0], M.Half) for r in records[:2]), "the images' cast comes first"
    if mixed == "train":
        plain = [r for r in train if r.kind in M.MIXED_PLAIN]
        assert [r.kind for r in plain] == ["cast", "cast"] and plain == train[:2], "the harness casts the two images, and nothing else is plain"
        assert all(r.grad_in is not None and r.grad_out is not None for r in train[2:])
    halves = [a for r in records for a in list(r.args) + list(r.outputs) + list(r.grad_out or ()) + list(r.grad_in or ()) if isinstance(a, M.Half)]
    assert halves and all(a.fmt == fmt for a in halves), (what, "a 16-bit tensor of another format")
    assert kernels == any(isinstance(a, M.Half) for r in records[2:] for a in r.args), (what, "16-bit storage on the kernel arm alone")
    report = []
    try:
        worst = M.check_all(records, oracle, report=report)
    finally:
        print("\n".join(report))
    print(f"{what}: product on the device, largest error / bar per kind and key\n" + M.fmt(worst))
    if mixed == "train":
        last = train[-1]
        assert last.kind == "DisparityLossFunction" and float(last.grad_out[0]) == (SCALE if scaler is not None else 1.0), float(last.grad_out[0])
        grads = [p.grad for p in model.parameters() if p.grad is not None]
        assert len(grads) > 10 and all(bool(torch.isfinite(g).all()) for g in grads), (what, "a parameter's gradient is not finite")
        sga = sorted({r.args[0].shape for r in train if r.kind == "SgaFunction"})
        h, w = H // 3, W // 3
        assert sga == sorted({(B, standin_net.C, MAX_DISP // 3 + 1, h, w), (B, standin_net.C, MAX_DISP // 6 + 1, h // 2, w // 2)}), sga
    return records


def _fmts():
    import mixed_cases as mxc
    return [pytest.param(mxc.BF16, id="bf16"), pytest.param(mxc.F16, id="f16")]


@pytest.mark.parametrize("fmt", _fmts())
def test_every_op_call_of_a_mixed_inference_pass(env, monkeypatch, port_oracle, fmt):
    """steps.predict(amp=) after use_mixed_precision(kernels=True), 48 x 96, B = 1"""
    import model_calls as M
    records = _run(env, monkeypatch, port_oracle, "infer", fmt)
    lga = {r.args[0].shape for r in records if r.kind in ("Lga2Function", "LgaFunction", "LgaRegressFunction")}
    assert lga == {(1, MAX_DISP + 1, 48, 96)}, lga
    sites = [r for r in records if r.kind == "bn_apply_mixed"]
    # the three forms: 9 plain and 3 with an fp32 residual write 16 bits over their input; 4 in front of an SGABlock return fp32
    assert sum(bool(r.args[6]) for r in sites) == 12 and sum(r.args[1] is not None for r in sites) == 3
    assert sum(not isinstance(r.outputs[0], M.Half) for r in sites) == 4


@pytest.mark.parametrize("fmt", _fmts())
def test_the_guidance_branch_of_a_mixed_inference_pass(env, monkeypatch, port_oracle, fmt):
    """the network of tests/mixed_standin.py, 24 x 48, maxdisp 12: the two top-level sites the training-capable stand-in does not
    have -- bn_apply_mixed with an fp32 x and a 16-bit y (never in place), and the up-cast of a 2-D convolution's output"""
    import model_calls as M
    records = _run(env, monkeypatch, port_oracle, "infer", fmt, crop=GUIDANCE_CROP, guidance_branch=True)
    sites = [r for r in records if r.kind == "bn_apply_mixed"]
    top = [r for r in sites if not isinstance(r.args[0], M.Half)]
    assert len(top) == 1 and top[0].args[0].ndim == 4 and isinstance(top[0].outputs[0], M.Half) and not top[0].args[6]
    assert sum(bool(r.args[6]) for r in sites) == 9 and sum(not isinstance(r.outputs[0], M.Half) for r in sites) == 3
    ups = [r for r in records[2:] if r.kind == "cast"]
    assert sorted(r.args[0].ndim for r in ups) == [4, 5] and all(isinstance(r.args[0], M.Half) and not isinstance(r.outputs[0], M.Half) for r in ups)


@pytest.mark.parametrize("fmt", _fmts())
def test_every_op_call_of_a_mixed_training_step(env, monkeypatch, port_oracle, fmt):
    """steps.train_step(amp=, scaler=) after use_mixed_precision_training(kernels=True), 48 x 96, B = 1: SGA on [1,8,17,16,32] and
    [1,8,9,8,16], LGA on [1,49,48,96] with radius 2; fp16 under GradScaler(init_scale=256).  The three sites of MixedBnReluFunction
    are all met: 9 plain, 4 with an fp32 output, 3 with an fp32 residual."""
    import model_calls as M
    records = _run(env, monkeypatch, port_oracle, "train", fmt)
    bn = [r for r in records if r.kind == "MixedBnReluFunction"]
    assert sum(r.args[1] is not None for r in bn) == 3 and sum(not isinstance(r.outputs[0], M.Half) for r in bn) == 4
    assert all(set(r.saved) == {"mean", "invstd"} for r in bn)
    assert all(isinstance(r.grad_in[0], M.Half) for r in bn if r.grad_in[0] is not None)
    lga = {r.args[0].shape for r in records if r.kind in ("Lga2Function", "LgaFunction", "LgaRegressFunction")}
    assert lga == {(1, MAX_DISP + 1, 48, 96)}, lga


@pytest.mark.parametrize("fmt", _fmts())
def test_every_op_call_of_a_training_step_on_the_cast_arm(env, monkeypatch, port_oracle, fmt):
    """the same step with kernels=False (and use_fused_disp_tail): only fp32 kinds are recorded, on activations that were rounded to
    16 bits between them and, under fp16, on gradients 256 times their size"""
    _run(env, monkeypatch, port_oracle, "train", fmt, kernels=False, rebinders=(TAIL,))


def test_the_second_crop_with_two_samples(env, monkeypatch, port_oracle):
    """96 x 240, B = 2, bf16, kernels: N > 1, and SGA volumes [2,8,17,32,80] and [2,8,9,16,40] -- 40 columns: two 16-column blocks and
    a partial one.  The device step is as short as at the first crop; the host's float64 side is what takes the time
    (tests/test_gpu_standin_calls.py: the same crop), which is why this crop has this one case."""
    import mixed_cases as mxc
    records = _run(env, monkeypatch, port_oracle, "train", mxc.BF16, crop=SECOND_CROP)
    assert any(r.args[0].shape[-1] % 16 for r in records if r.kind == "SgaFunction")
