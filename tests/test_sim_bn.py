"""The fused BatchNorm + residual + ReLU (ganet_amd/csrc/bn_kernels.h: ganet_bn_workspace / _train_forward / _train_backward /
_apply_forward) on the CPU emulator build: the case table of tests/bn_cases.py (tests/test_gpu_bn.py runs the same table on
the device), every case in both guard modes -- each buffer ENDS at an inaccessible page, resp. BEGINS right behind one
(parity_cases.guarded_empty) -- against the float64 statement of tests/bn_ref64.py, which the first tests here tie to
torch's own batch_norm in float64 and whose bars they check against the float32 model of the kernels' arithmetic."""
import os

import numpy as np
import pytest

import bn_cases as bc
import bn_ref64 as ref
import parity_cases as pc

F32 = np.float32


@pytest.fixture(scope="module")
def sim():
    from sim_util import sim_api
    return sim_api()


@pytest.fixture(params=["end", "start"])
def dev(request):
    return pc.NumpyDev(request.param)


# ---- the yardstick and the table ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["odd-2x5x819-relu-rem", "blocks-2x4x1024", "neg-weights-relu", "no-affine-relu-rem", "momentum1-relu"])
def test_yardstick_equals_torch_in_float64(name):
    """F.relu(F.batch_norm(x, training=True) + rem) and its autograd backward on float64 CPU tensors"""
    import torch
    import torch.nn.functional as F
    c = bc.BY_NAME[name]
    t = lambda a, g=False: None if a is None else torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(g)   # noqa: E731
    x, rem, w, b = t(c.x, True), t(c.rem, True), t(c.weight, True), t(c.bias, True)
    rm, rv = t(c.running_mean), t(c.running_var)
    z = F.batch_norm(x, rm, rv, w, b, True, float(F32(c.momentum)), float(F32(c.eps)))
    z = z if rem is None else z + rem
    y = F.relu(z) if c.relu else z
    y.backward(t(c.gy))
    r = c.ref
    close = lambda a, b: np.allclose(a.detach().numpy(), b, rtol=1e-9, atol=1e-11)   # noqa: E731
    assert close(y, r.y) and close(x.grad, r.grad_x) and close(rm, r.running_mean) and close(rv, r.running_var)
    if rem is not None:
        assert close(rem.grad, r.grad_rem)
    if w is not None:
        assert close(w.grad, r.grad_weight) and close(b.grad, r.grad_bias)


def test_case_table_reaches_what_it_claims():
    by = bc.BY_NAME
    assert (bc.BLOCK, bc.MAX_ROWS, bc.TARGET_BLOCKS) == (256, 64, 2048)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ganet_amd", "csrc", "bn_kernels.h")).read()
    for k, v in (("BN_BLOCK", bc.BLOCK), ("BN_MAX_ROWS", bc.MAX_ROWS), ("BN_TARGET_BLOCKS", bc.TARGET_BLOCKS)):
        assert f"constexpr int {k} = {v};" in hdr
    assert not by["scalar-3x2x7"].vec and by["vec-2x3x8"].vec and not by["vec-size-offset1-2x3x12"].vec and not by["odd-2x5x819"].vec
    # a partial last chunk; a second trip of the grid-stride loop, of the loop over the slices and of the loop over the rows
    assert bc.rows(1, 2, 257, False) == (2, 1) and bc.rows(1, 2, 1028, True) == (2, 1)
    for name, vec in (("trip2-scalar-2x1x16385", False), ("trip2-vec-2x1x65540", True)):
        N, C, S = by[name].shape
        rs, rn = bc.rows(N, C, S, vec)
        assert by[name].vec == vec and (rs, rn) == (bc.MAX_ROWS, 1) and N > rn and (S // 4 if vec else S) == rs * bc.BLOCK + 1
    assert bc.rows(5, 1, 64, True) == (1, 5) and bc.rows(2, 70, 4, True) == (1, 2) and bc.TARGET_BLOCKS // 70 < bc.MAX_ROWS
    assert bc.rows(2, 4, 1024, True) == (1, 2) and bc.rows(2, 5, 819, False) == (4, 2)
    # the mask-ambiguity condition: no element of a compared gradient sits within 4 B_y of the kink
    for c in bc.CASES:
        if c.compare_grads:
            assert int(c.ref.undecided().sum()) == 0, c.name
            assert c.nudged <= 3, (c.name, c.nudged)
        if c.exact:
            M = c.shape[0] * c.shape[2]
            assert M & (M - 1) == 0 and np.array_equal(c.x, np.round(c.x)) and np.abs(c.x).max() <= 8
    assert int(by["cancellation-1x5x4097-relu"].ref.undecided().sum()) > 1000
    # z exactly 0: y = 0 and g = 0 in the whole channel, whatever grad_y holds
    r = by["weight0-bias0-relu"].ref
    assert not r.z[:, 1].any() and not r.y[:, 1].any() and not r.g[:, 1].any() and np.abs(by["weight0-bias0-relu"].gy[:, 1]).min() > 0
    # cancellation: the fp32 sum of squares loses the variance, the statement does not
    c = by["cancellation-1x5x4097"]
    var32 = (c.x * c.x).sum(axis=(0, 2), dtype=F32) / F32(4097) - (c.x.sum(axis=(0, 2), dtype=F32) / F32(4097)) ** 2
    assert (np.abs(var32 - c.ref.var) > 0.5 * c.ref.var).any() and (np.abs(c.ref.var - 1e-4) < 2e-5).all()


@pytest.mark.parametrize("case", bc.CASES, ids=repr)
def test_float32_model_stays_inside_half_of_every_bar(case):
    ratios = bc.check(case, bc.model_as_got(case), verbose=False)
    assert max(ratios.values()) <= 0.5, ratios


# ---- the kernels ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", bc.CASES, ids=repr)
def test_case(sim, dev, case):
    bc.check(case, bc.run(sim, dev, case))


@pytest.mark.parametrize("name", bc.REPRODUCIBLE)
def test_reproducible_whatever_the_workspace_held(sim, name):
    bc.check_reproducible(sim, pc.NumpyDev(), bc.BY_NAME[name])


@pytest.mark.parametrize("pair", bc.nan_pairs(), ids=lambda p: p[1].name)
def test_nan(sim, dev, pair):
    bc.check_nan_pair(sim, dev, pair)


@pytest.mark.parametrize("want", bc.WANTED)
def test_null_outputs_are_not_computed(sim, dev, want):
    case = bc.BY_NAME["odd-2x5x819-relu-rem"]
    bc.check(case, bc.run(sim, dev, case, want=want), want=want)


@pytest.mark.parametrize("name", bc.EVAL_FORM)
@pytest.mark.parametrize("inplace", [False, True])
def test_eval_form(sim, dev, name, inplace):
    bc.check_eval_form(sim, dev, bc.BY_NAME[name], inplace)


def test_bad_arguments(sim):
    bc.check_bad_arguments(sim, pc.NumpyDev())


# ---- the module's host-side decisions (no device) ---------------------------------------------------------------------------

def test_fallback_predicate(monkeypatch):
    """bn_relu_path on CPU tensors that claim to be HIP tensors (is_cuda patched), so that the rule under test decides and not
    the device: momentum=None, an fp16 input and a SyncBatchNorm under a two-rank process group select the framework; their
    counterparts the native paths."""
    import torch
    from ganet_amd.modules.fused import bn_relu_path
    x = torch.zeros(2, 3, 4, 5)
    assert bn_relu_path(torch.nn.BatchNorm2d(3), x) == "framework"                  # not on a device
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    assert bn_relu_path(torch.nn.BatchNorm2d(3), x) == "train"
    assert bn_relu_path(torch.nn.BatchNorm2d(3), x, torch.zeros_like(x)) == "train"
    assert bn_relu_path(torch.nn.BatchNorm3d(3), x[..., None]) == "train"
    assert bn_relu_path(torch.nn.BatchNorm2d(3, momentum=None), x) == "framework"
    assert bn_relu_path(torch.nn.BatchNorm2d(3, momentum=None, track_running_stats=False), x) == "train"   # no average to keep
    assert bn_relu_path(torch.nn.BatchNorm2d(3), x.half()) == "framework"
    assert bn_relu_path(torch.nn.BatchNorm2d(3), x, torch.zeros_like(x).half()) == "framework"
    assert bn_relu_path(torch.nn.BatchNorm2d(3).half(), x) == "framework"
    ev = torch.nn.BatchNorm2d(3).eval()
    assert bn_relu_path(ev, x) == "framework"                                        # its parameters want gradients
    with torch.no_grad():
        assert bn_relu_path(ev, x) == "fold"
    assert bn_relu_path(ev.requires_grad_(False), x) == "fold"
    assert bn_relu_path(torch.nn.BatchNorm2d(3, track_running_stats=False).eval(), x) == "train"        # batch statistics
    sync = torch.nn.SyncBatchNorm(3)
    assert bn_relu_path(sync, x) == "train"                                          # no process group
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a: 2)
    assert bn_relu_path(sync, x) == "framework" and bn_relu_path(torch.nn.BatchNorm2d(3), x) == "train"
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a: 1)
    assert bn_relu_path(sync, x) == "train"
    with torch.no_grad():
        assert bn_relu_path(sync.eval(), x) == "fold"
