"""The float64 yardsticks of tests/model_calls.py on MODEL data, without a GPU: the CPU-oracle twin of the reference models
(harness.steps.build_model + oracle.cpu_ops.route_cpu_through_oracle, as tests/test_model_harness_cpu.py builds it) runs one
training step and one steps.predict under the recorder; every SGA and LGA record then goes through the checkers with the
ORACLE's own results as `got`.

  calibration  the reference stays inside FACTOR x the bounds on model-distributed data -- x half zeros, L1-normalised
               convolution output as guidance, gradients of 1e-2 .. 1e-4, a post-softmin volume with |gy| up to 26 -- at a
               48x96 crop (B = 1) and at 96x240 with B = 2, where the SGA volumes are [2,32,17,32,80] and [2,48,9,16,40]:
               N > 1 and a width that is no multiple of 16.  The largest error / bound per kind and key is printed.
  teeth        a comparison that cannot fail proves nothing: on every SGA and LGA record a result replaced by zeros, one with
               a term left out (sga_ref64.mutated; lga_ref64.mutated_chain: one tap dropped, zero padding instead of the
               centre value) and one scaled by 1 + 2^-12 must each be REJECTED.  The all-zero LGA2 data gradient of
               GANet_deep is the case parity_cases.TOL lets through at this scale: that is asserted too, so that the motive
               of these tests stays checked.
  recorder     on toy Functions: an input written during forward is reported, a declared in-place form is not."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import lga_ref64  # noqa: E402
import model_calls as M  # noqa: E402
import parity_cases as pc  # noqa: E402
import sga_ref64 as s64  # noqa: E402
import sga_ref64_cases as sc  # noqa: E402
from harness import refmodel, steps  # noqa: E402

needs_models = pytest.mark.skipif(not refmodel.available(), reason="no reference model code (GANET_REF_ROOT, "
                                  "/root/reference or oracle/_ref/pyref)")

MAX_DISP = 48
CROPS = {"48x96": (48, 96, 1), "96x240x2": (96, 240, 2)}
# SGA calls per forward (models/GANet11.py, models/GANet_deep.py); both models call LGA2 twice
N_SGA = {"GANet11": 4, "GANet_deep": 7}
_RUNS = {}


@pytest.fixture(scope="module", autouse=True)
def _release_the_runs():
    """the records and the float64 references kept on them (hundreds of MB) go when this module's tests are done"""
    yield
    _RUNS.clear()


def _recorded(oracle, name, crop):
    """-> (records of one training step, records of one steps.predict) of the CPU twin, recorded once per (model, crop)"""
    if (name, crop) not in _RUNS:
        from oracle.cpu_ops import route_cpu_through_oracle
        H, W, B = CROPS[crop]
        torch.manual_seed(0)
        model = steps.build_model(name, MAX_DISP, "cpu", hook=lambda m: route_cpu_through_oracle(m, oracle))
        left, right, target = steps.synthetic_batch(B, H, W, MAX_DISP, "cpu")
        with pytest.MonkeyPatch.context() as patch, M.recording(patch, *M.oracle_functions()) as records:
            model.train()
            outs = model(left, right)
            steps.loss_mix(name, outs, target, target < MAX_DISP, steps.criterion(True)).backward()
            n_train = len(records)
            steps.predict(model, left, right)
        _RUNS[name, crop] = (records[:n_train], records[n_train:])
    return _RUNS[name, crop]


@needs_models
@pytest.mark.parametrize("name,crop", [("GANet11", "48x96"), ("GANet_deep", "48x96"), ("GANet_deep", "96x240x2")])
def test_oracle_stays_inside_the_float64_bounds_on_model_data(port_oracle, name, crop):
    train, infer = _recorded(port_oracle, name, crop)
    for part in (train, infer):
        assert M.kinds_of(part) == {"OracleSga": N_SGA[name], "OracleLgaChain": 2}, M.kinds_of(part)
    assert all(r.grad_in is not None for r in train) and all(r.grad_in is None for r in infer)
    assert M.undeclared_writes(train + infer) == []
    H, W, B = CROPS[crop]
    assert train[0].args[1].shape[0] == B and train[-1].args[1].shape == (B, MAX_DISP + 1, H, W)
    if crop != "48x96":
        assert any(r.args[1].shape[-1] % 16 for r in train if r.kind == "OracleSga"), "no partial 16-column block at this crop"
    report = []
    worst = M.check_all(train + infer, port_oracle, report=report)
    print(f"{name} {crop}: oracle, largest error / bound (bar: {M.FACTOR})\n" + M.fmt(worst))
    print("\n".join(report))
    assert {k for k, _ in worst} == {"OracleSga", "OracleLgaChain"} and max(worst.values()) <= M.FACTOR
    if crop != "48x96":
        del _RUNS[name, crop]                                       # nobody else uses the large crop: ten times the memory


def _rejected(judge, *args, **kw):
    try:
        judge(*args, **kw)
    except AssertionError:
        return True
    return False


def _scaled(got, keys):
    return {k: (v * np.float32(1 + 2.0 ** -12) if k in keys else v) for k, v in got.items()}


@needs_models
@pytest.mark.parametrize("name", ["GANet11", "GANet_deep"])
def test_every_sga_record_rejects_a_wrong_result(port_oracle, name):
    train, infer = _recorded(port_oracle, name, "48x96")
    exercised = dict.fromkeys(s64.DROPS, 0)
    for r in [r for r in train + infer if r.kind == "OracleSga"]:
        R = M.reference_of(r, port_oracle)
        got = M.sga_got(r, R)
        M.sga_judge(R, got)                                         # the unspoilt record passes
        x, gs = M._sga_inputs(r)
        if R["ref"] is None:                                        # steps.predict: `out` alone, held by equality
            assert _rejected(M.sga_judge, R, {"out": np.zeros_like(got["out"])})
            assert _rejected(M.sga_judge, R, _scaled(got, ("out",)))
            continue
        # a) zeros, c) scaled by 1 + 2^-12: through the BOUND (equality with the oracle would notice first: switched off)
        for k in sc.GRADS + sc.FWD:
            assert _rejected(M.sga_judge, R, {**got, k: np.zeros_like(got[k])}, equality=False), (r, k, "zeros pass")
            assert _rejected(M.sga_judge, R, _scaled(got, (k,)), equality=False), (r, k, "scaled passes")
        # b) one gradient term left out of the float64 statement itself.  A record on which a term never acts (no tie for
        # the last arg-max to differ on) leaves the statement's result as it was: counted, not asserted
        for drop in s64.DROPS:
            mut = s64.mutated(x, gs, r.grad_out[0], R["ref"], drop)
            if all(np.array_equal(mut[k], R["ref"][k]) for k in sc.GRADS):
                continue
            exercised[drop] += 1
            wrong = {**got, **{k: mut[k].astype(np.float32) for k in sc.GRADS}}
            assert _rejected(M.sga_judge, R, wrong, equality=False), (r, drop)
    print(name, "records on which each left-out term acts:", exercised)
    assert all(exercised.values()), exercised


@needs_models
@pytest.mark.parametrize("name", ["GANet11", "GANet_deep"])
def test_every_lga_record_rejects_a_wrong_result(port_oracle, name):
    train, infer = _recorded(port_oracle, name, "48x96")
    for r in [r for r in train + infer if r.kind == "OracleLgaChain"]:
        R = M.reference_of(r, port_oracle)
        got = M.lga_got(r)
        M.lga_judge(R, got)
        x, f, radius, passes = M._lga_inputs(r)
        gy = r.grad_out[0] if r.grad_out is not None else np.zeros_like(x)
        for k in got:
            assert _rejected(M.lga_judge, R, {**got, k: np.zeros_like(got[k])}), (r, k, "zeros pass")
            assert _rejected(M.lga_judge, R, _scaled(got, (k,))), (r, k, "scaled passes")
        for what in lga_ref64.MUTATIONS:
            mut = lga_ref64.mutated_chain(x, f, gy, radius, passes, what)
            for k in got:
                assert _rejected(M.lga_judge, R, {**got, k: mut[k].astype(np.float32)}), (r, k, what)


@needs_models
def test_the_absolute_bar_accepts_an_all_zero_lga2_data_gradient(port_oracle):
    """GANet_deep's first LGA2 ([1,49,48,96], r = 2) gets gradients of 4e-3 and returns a data gradient of 9e-5 at most: zeros
    are within parity_cases.TOL of it, and far outside the float64 bound"""
    train, _ = _recorded(port_oracle, "GANet_deep", "48x96")
    r = [r for r in train if r.kind == "OracleLgaChain"][0]
    R = M.reference_of(r, port_oracle)
    got = M.lga_got(r)
    zeros = np.zeros_like(got["gx"])
    assert 0 < np.abs(zeros - R["want"]["gx"]).max() <= pc.TOL and np.abs(got["gx"]).max() <= pc.TOL
    assert M.lga_ratios(R, {"gx": zeros})["gx"] > 1e3 * M.FACTOR


# ---- the recorder, on toy Functions -------------------------------------------------------------------------------------------
class ToyScale(torch.autograd.Function):
    """y = 2 x.  spoil: forward also writes x (which nothing declares); inplace: y overwrites x (declared below)"""

    @staticmethod
    def forward(ctx, x, inplace, spoil):
        if inplace:
            ctx.mark_dirty(x)
            return x.mul_(2)
        y = x * 2
        if spoil:
            x.add_(1)
        return y

    @staticmethod
    def backward(ctx, g):
        return g * 2, None, None


def test_recorder_reports_written_inputs_and_knows_declared_inplace_forms(monkeypatch):
    monkeypatch.setitem(M.DECLARED, "ToyScale", lambda r: {"arg0"} if r.args[1] else set())
    plain = ToyScale.forward
    with M.recording(monkeypatch, [ToyScale]) as records:
        a = torch.arange(4.0)
        y = ToyScale.apply(a.clone().requires_grad_(), False, False)
        y.backward(torch.ones(4))
        ToyScale.apply(a.clone(), False, True)
        b = a.clone().requires_grad_()
        z = ToyScale.apply(b * 1, True, False)
        z.sum().backward()
    assert ToyScale.forward is plain, "nothing stays patched"
    clean, spoilt, inplace = records
    assert np.array_equal(clean.args[0], [0, 1, 2, 3]) and np.array_equal(clean.outputs[0], [0, 2, 4, 6]) and clean.args[1:] == [False, False]
    assert np.array_equal(clean.grad_out[0], np.ones(4)) and np.array_equal(clean.grad_in[0], 2 * np.ones(4)) and clean.written == []
    assert spoilt.written == [("forward", "arg0")] and np.array_equal(spoilt.args[0], [0, 1, 2, 3]) and spoilt.grad_in is None
    assert inplace.written == [("forward", "arg0")] and np.array_equal(inplace.args[0], [0, 1, 2, 3])      # cloned BEFORE the call
    assert np.array_equal(inplace.after[0], [0, 2, 4, 6]) and np.array_equal(b.grad, 2 * np.ones(4))
    assert M.undeclared_writes(records) == [(1, "ToyScale", "forward", "arg0")]
    with pytest.raises(AssertionError, match="ToyScale"):
        M.check_all(records, None)                                  # a recorded kind without a checker
