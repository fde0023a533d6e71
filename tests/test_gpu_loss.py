"""The fused criterion on the gfx950 build: the case table of tests/loss_cases.py through the C ABI (tests/test_sim_loss.py
runs it on the emulator) -- same inputs, same float64 yardstick, same bars; the device's fp32 arithmetic has to produce the
float32 statement's gradients bit for bit, which it does not if the compiler contracts a multiply-add or reorders -- and,
device only, through ganet_amd.modules.fused.DisparityLoss: autograd, run-to-run reproducibility, no host synchronisation,
graph capture, and harness.steps.train_step(fused_loss=...) against the default step."""
import copy

import numpy as np
import pytest

import loss_cases as lc
from test_gpu_parity import TorchDev

pytestmark = pytest.mark.gpu

BY_NAME = {c.name: c for c in lc.CASES}
MODULE_CASES = ["shape-1", "shape-255", "shape-256", "shape-n2-vec", "shape-vec-2blocks", "p1-myloss2-eval", "p2-kinds10",
                "p3-eval-t1a2", "boundary-t1a2", "boundary-t3a2", "targets-mode1", "all-invalid", "exact-2048"]


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


def module_for(case):
    from ganet_amd.modules.fused import DisparityLoss
    p, P = case.params, len(case.preds)
    return DisparityLoss(p["hi"], [p[f"w{k}"] for k in range(P)], [("sl1", "myloss2")[k] for k in case.kinds],
                         thresh=p["thresh"], alpha=p["alpha"], rate_threshold=p["rate"],
                         mask="train" if case.mask_mode == 0 else "eval", lo=p["lo"])


def tensors(dev, case, requires_grad=True):
    preds = [dev.to(p).requires_grad_(requires_grad) for p in case.preds]
    return preds, dev.to(case.target)


def host(t):
    return None if t is None else t.detach().cpu().numpy()


# ---- C ABI: the shared table ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", lc.CASES, ids=repr)
def test_case(api, dev, case):
    lc.check(case, lc.run(api, dev, case))


@pytest.mark.parametrize("thresh,alpha,v,value,slope", lc.SPOTS)
def test_spot_values(api, dev, thresh, alpha, v, value, slope):
    """one pixel, weight 1, grad_loss 1: loss = rho(v) and the gradient = the slope, against the literal values"""
    got = lc.run(api, dev, BY_NAME[f"spot-t{thresh}a{alpha}-v{v}"])
    assert lc.close(got["loss"], value, lc.SUM_RTOL) and lc.close(got["grads"][0].item(), slope, lc.GRAD_RTOL)


@pytest.mark.parametrize("offset", [0, 1])
def test_poisoned_invalid_pixels_change_nothing(api, dev, offset):
    clean, dirty = lc.poison_pair(offset=offset)
    a, b = lc.run(api, dev, clean), lc.run(api, dev, dirty)
    assert np.isfinite(b["loss"]) and np.isfinite(b["stats"]).all()
    assert lc.bits(a["loss"]) == lc.bits(b["loss"]) and np.array_equal(lc.bits(a["stats"]), lc.bits(b["stats"]))
    lc.check(dirty, b)
    for ga, gb in zip(a["grads"], b["grads"]):
        assert np.array_equal(lc.bits(ga), lc.bits(gb))


def test_two_runs_are_bit_identical(api, dev):
    case = BY_NAME["shape-vec-stride2"]
    a, b = lc.run(api, dev, case), lc.run(api, dev, case)
    assert lc.bits(a["loss"]) == lc.bits(b["loss"]) and np.array_equal(lc.bits(a["stats"]), lc.bits(b["stats"]))
    for ga, gb in zip(a["grads"], b["grads"]):
        assert np.array_equal(lc.bits(ga), lc.bits(gb))


# ---- the module ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", MODULE_CASES)
def test_module_autograd(api, dev, name):
    """DisparityLoss + autograd with grad_loss != 1: (loss * 0.37).backward() hands fl32(0.37) to the backward kernel"""
    case = BY_NAME[name]
    preds, target = tensors(dev, case)
    loss, stats = module_for(case)(preds, target)
    assert loss.dim() == 0 and stats.shape == (1 + 3 * len(preds),) and loss.requires_grad and not stats.requires_grad
    (loss * 0.37).backward()
    lc.check_forward(case, host(loss), host(stats))
    lc.check_grads(case, [host(p.grad) for p in preds], grad_loss=0.37, want=(True,) * len(preds))


def test_prediction_without_grad_gets_no_map(api, dev, monkeypatch):
    import torch
    case = BY_NAME["shape-n2-vec"]
    preds, target = tensors(dev, case)
    preds[1].requires_grad_(False)
    target.requires_grad_(True)                  # asked for or not, the target never gets a gradient
    loss, _ = module_for(case)(preds, target)
    seen, call = [], api.call

    def spy(name, *args):
        if name == "ganet_disparity_loss_backward":
            seen.append(args[7:10])              # g0, g1, g2
        return call(name, *args)

    monkeypatch.setattr(api, "call", spy)
    g0, g2, gt = torch.autograd.grad(loss, [preds[0], preds[2], target], allow_unused=True)
    assert gt is None and len(seen) == 1 and seen[0][0] and seen[0][1] is None and seen[0][2]
    lc.check_grads(case, [host(g0), None, host(g2)], grad_loss=1.0, want=(True, False, True))
    frozen, _ = tensors(dev, case, requires_grad=False)
    loss, _ = module_for(case)(frozen, target.detach())
    assert not loss.requires_grad


def test_no_host_synchronisation(api, dev):
    """forward and backward of the module under set_sync_debug_mode("error"); the stock loss_mix under the same mode raises
    (every `d[mask]` is a nonzero with a device-to-host copy behind it).  The first call of a module uploads its eight
    parameters; that one is made before."""
    import torch
    from harness import steps
    case = BY_NAME["shape-256"]
    preds, target = tensors(dev, case)
    mod = module_for(case)
    mod(preds, target)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, stats = mod(preds, target)
        loss.backward()
        with pytest.raises(RuntimeError):
            steps.loss_mix("GANet_deep", preds, target, target < lc.HI, steps.criterion(True))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    lc.check_forward(case, host(loss), host(stats))
    lc.check_grads(case, [host(p.grad) for p in preds], grad_loss=1.0)


def test_graph_capture_and_replay(api, dev):
    """forward + backward captured once on a single stream; replayed with the target rewritten in between, the third time
    without a valid pixel"""
    import torch
    base = BY_NAME["shape-n2-vec"]
    rng = np.random.default_rng(5)
    targets = [base.target, rng.uniform(0, 1.2 * lc.HI, base.shape).astype(np.float32), np.full(base.shape, lc.HI, np.float32)]
    cases = [lc.Case(f"replay{i}", base.shape, base.preds, t, base.kinds, lc.DEEP) for i, t in enumerate(targets)]
    assert cases[2].ref.count == 0 < cases[1].ref.count
    preds, target = tensors(dev, base)
    mod = module_for(base)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            loss, stats = mod(preds, target)
            grads = torch.autograd.grad(loss * 0.37, preds)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, stats = mod(preds, target)
        grads = torch.autograd.grad(loss * 0.37, preds)
    for case in cases:
        target.copy_(dev.to(case.target))
        graph.replay()
        torch.cuda.synchronize()
        lc.check_forward(case, host(loss), host(stats))
        lc.check_grads(case, [host(g) for g in grads], grad_loss=0.37)


# ---- the training step -----------------------------------------------------------------------------------------------------

MAX_DISP = 8


def tiny_model():
    """a stand-in for the reference model: two convolutions, three disparity maps"""
    import torch

    class Tiny(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = torch.nn.Conv2d(6, 8, 3, padding=1)
            self.b = torch.nn.Conv2d(8, 3, 3, padding=1)

        def forward(self, left, right):
            y = 4.0 + 6.0 * self.b(torch.relu(self.a(torch.cat([left, right], 1))))
            return y[:, 0], y[:, 1], y[:, 2]

    torch.manual_seed(11)
    return Tiny().cuda()


def step_pair(target):
    """the default step and the fused step on two copies of one model; each step's own outputs (caught by a forward hook)
    make the case its loss is compared through"""
    import torch
    from ganet_amd.modules.fused import DisparityLoss
    from harness import steps
    left, right, _ = steps.synthetic_batch(2, 12, 20, MAX_DISP, "cuda", seed=3)
    stock = tiny_model()
    fused = copy.deepcopy(stock)
    res, cases = [], []
    for model, crit in ((stock, None), (fused, DisparityLoss.ganet_deep(MAX_DISP, kitti=True))):
        seen = []
        hook = model.register_forward_hook(lambda m, i, o: seen.append([t.detach().contiguous().cpu().numpy() for t in o]))
        opt = torch.optim.SGD(model.parameters(), lr=1e-3)
        res.append(steps.train_step(model, opt, "GANet_deep", left, right, target, MAX_DISP, steps.criterion(True), fused_loss=crit))
        hook.remove()
        cases.append(lc.Case("step", target.shape, seen[0], target.cpu().numpy(), (0, 0, 1), lc.DEEP, thresh=3, alpha=2, hi=MAX_DISP))
    return stock, fused, res, cases


def test_train_step_fused_against_default(api):
    from harness import steps
    target = steps.synthetic_batch(2, 12, 20, MAX_DISP, "cuda", seed=3)[2] * 1.3      # some pixels at or above max_disp
    stock, fused, results, cases = step_pair(target)
    for (loss, err), case in zip(results, cases):
        assert 0 < case.ref.count < target.numel()
        print("step loss", float(loss), case.ref.loss, "err", float(err), case.ref.epe[-1])
        assert lc.close(float(loss), case.ref.loss, lc.SUM_RTOL), (float(loss), case.ref.loss)
        assert lc.close(float(err), case.ref.epe[-1], lc.SUM_RTOL), (float(err), case.ref.epe[-1])
    for (n, a), b in zip(fused.named_parameters(), stock.parameters()):
        assert a.grad is not None and float((a.grad - b.grad).abs().max()) <= 1e-5 * float(b.grad.abs().max()), n


def test_train_step_fused_on_an_empty_shard(api, monkeypatch):
    """A rank without a valid pixel, in a job whose other rank has some (the collectives are stood in for: the peer reports
    five valid pixels and finite gradients): the fused step takes no branch of its own, runs the backward and leaves finite
    all-zero gradients on every parameter."""
    import torch
    from harness import steps

    def all_reduce(t, op=None):
        if t.numel() == 2:                        # [valid pixels, ranks with an empty shard], summed over the ranks
            t += torch.tensor([5, 0], dtype=t.dtype, device=t.device)

    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a: 2)
    monkeypatch.setattr(torch.distributed, "all_reduce", all_reduce)
    target = torch.full((2, 12, 20), float(MAX_DISP), device="cuda")
    _, fused, (_, (loss, err)), (_, case) = step_pair(target)
    assert case.ref.count == 0 and float(loss) == 0.0 and float(err) == 0.0
    for n, p in fused.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and not p.grad.any(), n
