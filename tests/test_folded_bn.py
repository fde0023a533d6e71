"""ganet_amd.modules.fused.folded_bn on the CPU (plain torch, no kernel): the cached (scale, shift) of a BatchNorm must follow
every way the module's statistics and parameters change.  A train-mode forward updates running_mean / running_var WITHOUT
bumping their autograd version counters; a cache keyed on those alone served stale statistics to GuidedSGABnRelu and
ResidualBnRelu after eval -> train forward -> eval."""
import pytest
import torch

from ganet_amd.modules.fused import folded_bn


def _bn(C, affine, seed=0):
    bn = torch.nn.BatchNorm3d(C, affine=affine)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(C, generator=gen))
        bn.running_var.copy_(torch.rand(C, generator=gen) + 0.25)
        if affine:
            bn.weight.copy_(torch.randn(C, generator=gen))
            bn.bias.copy_(torch.randn(C, generator=gen))
    return bn.eval()


def _fresh(bn):
    """the fold from the module's current tensors, and a check that it IS what the module computes in eval mode"""
    scale = (bn.running_var + bn.eps).rsqrt() * (bn.weight if bn.affine else 1.0)
    shift = (bn.bias if bn.affine else 0.0) - bn.running_mean * scale
    x = torch.randn(2, bn.num_features, 2, 3, 4, generator=torch.Generator().manual_seed(1))
    was = bn.training
    with torch.no_grad():
        want = bn.eval()(x)
    bn.train(was)
    v = (1, -1, 1, 1, 1)
    assert torch.allclose(want, x * scale.view(v) + shift.view(v), atol=1e-5)
    return scale.detach(), shift.detach()


def _assert_current(bn, **kw):
    scale, shift = folded_bn(bn, **kw)
    want_scale, want_shift = _fresh(bn)
    assert torch.equal(scale, want_scale) and torch.equal(shift, want_shift), \
        (float((scale - want_scale).abs().max()), float((shift - want_shift).abs().max()))


@pytest.mark.parametrize("affine", [True, False])
def test_fold_follows_a_train_mode_forward_without_optimizer_step(affine):
    bn = _bn(5, affine)
    _assert_current(bn)
    before = [t.clone() for t in folded_bn(bn)]
    bn.train()
    gen = torch.Generator().manual_seed(2)
    bn(3.0 * torch.randn(4, 5, 2, 3, 3, generator=gen) + 1.0)
    bn.eval()
    _assert_current(bn)
    assert not torch.equal(folded_bn(bn)[1], before[1]), "the statistics did move"


def test_fold_is_kept_between_eval_calls_and_not_kept_in_training_mode():
    bn = _bn(4, True)
    a = folded_bn(bn)
    assert folded_bn(bn)[0] is a[0] and folded_bn(bn)[1] is a[1]         # steady eval path: the very same tensors
    bn.train()
    _assert_current(bn)
    assert "_ganet_folded" not in bn.__dict__
    bn(torch.randn(3, 4, 2, 2, 2, generator=torch.Generator().manual_seed(3)))
    _assert_current(bn)                                                  # still in training mode: computed afresh
    bn.eval()
    _assert_current(bn)


@pytest.mark.parametrize("affine", [True, False])
def test_fold_follows_load_state_dict_and_in_place_writes(affine):
    bn, other = _bn(3, affine, seed=0), _bn(3, affine, seed=7)
    _assert_current(bn)
    bn.load_state_dict(other.state_dict())
    _assert_current(bn)
    assert torch.equal(folded_bn(bn)[0], folded_bn(other)[0])
    with torch.no_grad():
        bn.running_var.mul_(2.0)
    _assert_current(bn)
    if affine:
        with torch.no_grad():
            bn.bias.add_(1.0)                                             # what an optimizer step does
        _assert_current(bn)


def test_a_write_through_data_needs_the_refresh_route():
    """`.data` shares the storage but not the version counter: no host-side key can see the write (folded_bn's docstring).
    The documented route after such a write is folded_bn(bn, refresh=True), which also renews what later calls return."""
    bn = _bn(3, True)
    _assert_current(bn)
    bn.running_mean.data.add_(1.0)
    _assert_current(bn, refresh=True)
    _assert_current(bn)
