"""The float64 yardsticks of tests/model_calls.py on MODEL data, without a GPU: the CPU-oracle twin of the reference models
(harness.steps.build_model + oracle.cpu_ops.route_cpu_through_oracle, as tests/test_model_harness_cpu.py builds it) and of the
stand-in network of tests/standin_net.py ("standin": needs no reference file, so these tests run wherever the suite runs)
runs one training step and one steps.predict under the recorder; every SGA and LGA record then goes through the checkers
with the ORACLE's own results as `got`.

  calibration  the reference stays inside FACTOR x the bounds on model-distributed data -- x half zeros, L1-normalised
               convolution output as guidance, gradients of 1e-2 .. 1e-4, a post-softmin volume with |gy| up to 26 -- at a
               48x96 crop (B = 1) and at 96x240 with B = 2, where the SGA volumes are [2,32,17,32,80] and [2,48,9,16,40]:
               N > 1 and a width that is no multiple of 16.  The largest error / bound per kind and key is printed.
  teeth        a comparison that cannot fail proves nothing: on every SGA and LGA record a result replaced by zeros, one with
               a term left out (sga_ref64.mutated; lga_ref64.mutated_chain: one tap dropped, zero padding instead of the
               centre value) and one scaled by 1 + 2^-12 must each be REJECTED.  The all-zero LGA2 data gradient of
               GANet_deep is the case parity_cases.TOL lets through at this scale: that is asserted too, so that the motive
               of these tests stays checked.
  recorder     on toy Functions: an input written during forward is reported, a declared in-place form is not.
  Disp tails   DispTail's and DispConv's checkers on records built by hand from the tensors the stand-in's CPU run hands to its
               two Disp and one DispAgg sites: calibration against a plain fp32 evaluation (disp_tail_ref64.Float32Model in both
               variants of lambda; a numpy fp32 accumulation of the convolution, and ATen's), and the same teeth plus every
               entry of the two MUTATIONS tables.
  stand-in     tied to the reference where that exists: the reference's SGABlock, Disp and DispAgg and the stand-in's, with one
               state_dict, give the same bits forward and backward, and every rebinder of harness.fuse counts the same sites."""
import collections
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import disp_conv_ref64  # noqa: E402
import disp_tail_ref64  # noqa: E402
import lga_ref64  # noqa: E402
import model_calls as M  # noqa: E402
import parity_cases as pc  # noqa: E402
import sga_ref64 as s64  # noqa: E402
import sga_ref64_cases as sc  # noqa: E402
import standin_net  # noqa: E402
from harness import refmodel, steps  # noqa: E402

needs_models = pytest.mark.skipif(not refmodel.available(), reason="no reference model code (GANET_REF_ROOT, "
                                  "/root/reference or oracle/_ref/pyref)")

MAX_DISP = 48
CROPS = {"48x96": (48, 96, 1), "96x240x2": (96, 240, 2)}
# SGA calls per forward (models/GANet11.py, models/GANet_deep.py; tests/standin_net.py: sga1, sga11, sga2, sga3); all call LGA2 twice
N_SGA = {"GANet11": 4, "GANet_deep": 7, "standin": 4}
_RUNS, _SITES = {}, {}


def _ref(*values):
    """a parameter set on a reference model: skipped where its files are missing.  The stand-in's never is."""
    return pytest.param(*values, marks=needs_models)


@pytest.fixture(scope="module", autouse=True)
def _release_the_runs():
    """the records and the float64 references kept on them (hundreds of MB) go when this module's tests are done"""
    yield
    _RUNS.clear()
    _SITES.clear()


def _recorded(oracle, name, crop):
    """-> (records of one training step, records of one steps.predict) of the CPU twin, recorded once per (model, crop)"""
    if (name, crop) not in _RUNS:
        from oracle.cpu_ops import route_cpu_through_oracle
        H, W, B = CROPS[crop]
        torch.manual_seed(0)
        if name == "standin":
            model = standin_net.build(MAX_DISP, "cpu")
            route_cpu_through_oracle(model, oracle)
            sites = _watch_the_disp_sites(model)
        else:
            model = steps.build_model(name, MAX_DISP, "cpu", hook=lambda m: route_cpu_through_oracle(m, oracle))
        left, right, target = steps.synthetic_batch(B, H, W, MAX_DISP, "cpu")
        with pytest.MonkeyPatch.context() as patch, M.recording(patch, *M.oracle_functions()) as records:
            model.train()
            outs = model(left, right)
            steps.loss_mix("GANet_deep" if name == "standin" else name, outs, target, target < MAX_DISP, steps.criterion(True)).backward()
            n_train = len(records)
            if name == "standin":
                _SITES[crop] = [_site_tensors(s) for s in sites]
                sites.clear()
            steps.predict(model, left, right)
            if name == "standin":
                _SITES[crop] += [_site_tensors(s) for s in sites]
        _RUNS[name, crop] = (records[:n_train], records[n_train:])
    return _RUNS[name, crop]


def _watch_the_disp_sites(model):
    """forward hooks on every Disp / DispAgg of the stand-in: what its conv32x1 was given and returned and, for a Disp, what the
    tail behind it returned -- kept WITH their gradients (retain_grad).  -> the list the calls are appended to"""
    sites = []
    for name, m in model.named_modules():
        if type(m).__name__ not in ("Disp", "DispAgg"):
            continue

        def conv_hook(conv, args, c, name=name, kind=type(m).__name__):
            if c.requires_grad:
                c.retain_grad()
            sites.append({"name": name, "kind": kind, "x": args[0], "w": conv.weight, "c": c, "out": None})

        def tail_hook(mod, args, out, name=name):
            if out.requires_grad:
                out.retain_grad()
            next(s for s in reversed(sites) if s["name"] == name)["out"] = out

        m.conv32x1.register_forward_hook(conv_hook)
        m.register_forward_hook(tail_hook)
    return sites


def _site_tensors(s):
    """host copies; g_c / g_out: the gradients that came in at the convolution's output resp. at the tail's (None: no_grad)"""
    np32 = lambda t: None if t is None else np.ascontiguousarray(t.detach().numpy(), np.float32)      # noqa: E731
    return {"name": s["name"], "kind": s["kind"], "x": np32(s["x"]), "w": np32(s["w"]), "c": np32(s["c"]), "out": np32(s["out"]),
            "g_c": np32(s["c"].grad), "g_out": np32(s["out"].grad), "maxdisp": MAX_DISP}


@pytest.mark.parametrize("name,crop", [_ref("GANet11", "48x96"), _ref("GANet_deep", "48x96"), _ref("GANet_deep", "96x240x2"),
                                       ("standin", "48x96"), ("standin", "96x240x2")])
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


@pytest.mark.parametrize("name", [_ref("GANet11"), _ref("GANet_deep"), "standin"])
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


@pytest.mark.parametrize("name", [_ref("GANet11"), _ref("GANet_deep"), "standin"])
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


# ---- DispTail's and DispConv's checkers on the stand-in's Disp sites -----------------------------------------------------------
def _record(kind, args, outputs, grad_out=None, grad_in=None):
    r = M.Record(kind, args, grad_out is not None)
    r.outputs, r.grad_out, r.grad_in = outputs, grad_out, grad_in
    return r


def _size(site):
    return (site["maxdisp"] + 1, 3 * site["x"].shape[3], 3 * site["x"].shape[4])


def _tail_record(site, variant):
    """what UpSoftminRegressionFunction would record at a Disp site, with disp_tail_ref64.Float32Model's results as the call's"""
    c4 = site["c"][:, 0]
    f32 = disp_tail_ref64.Float32Model(c4, _size(site), site["g_out"], variant)
    return _record("UpSoftminRegressionFunction", [site["c"], _size(site)], [f32.out], [site["g_out"]], [f32.grad_x[:, None], None])


def _conv_fp32(site, how):
    """{y, grad_x, grad_weight} of the convolution in plain fp32: "numpy" -- disp_conv_ref64's own loops on float32 arrays (an
    fp32 accumulation, tap by tap); "aten" -- F.conv3d and its autograd on the CPU"""
    x, w = site["x"], site["w"]
    gy = site["g_c"][:, 0] if site["g_c"] is not None else None
    if how == "numpy":
        w4 = w.reshape(w.shape[1], 3, 3, 3)
        res = {"y": disp_conv_ref64.forward(x, w4)}
        if gy is not None:
            res.update(grad_x=disp_conv_ref64.backward_data(gy, w4), grad_weight=disp_conv_ref64.backward_weight(x, gy))
        assert all(v.dtype == np.float32 for v in res.values())
        return res
    xt, wt = torch.from_numpy(x).requires_grad_(), torch.from_numpy(w).requires_grad_()
    y = torch.nn.functional.conv3d(xt, wt, None, 1, 1)
    res = {"y": y.detach().numpy()[:, 0]}
    if gy is not None:
        y.backward(torch.from_numpy(gy)[:, None])
        res.update(grad_x=xt.grad.numpy(), grad_weight=wt.grad.numpy()[0])
    return res


def _conv_record(site, how):
    res = _conv_fp32(site, how)
    if site["g_c"] is None:
        return _record("DispConvFunction", [site["x"], site["w"], ("forward", "data", "weight")], [res["y"][:, None]])
    return _record("DispConvFunction", [site["x"], site["w"], ("forward", "data", "weight")], [res["y"][:, None]], [site["g_c"]],
                   [res["grad_x"], res["grad_weight"][None], None])


def _sites(oracle, crop="48x96"):
    _recorded(oracle, "standin", crop)
    return _SITES[crop]


@pytest.mark.parametrize("crop", ["48x96", "96x240x2"])
def test_plain_fp32_stays_inside_the_bars_of_the_disp_tail_and_the_disp_conv(port_oracle, crop):
    """calibration: on the tensors the stand-in's CPU run hands to its Disp / DispAgg sites -- a convolution output of 1e-1,
    gradients of 1e-4 and below -- a plain fp32 evaluation of each op stays inside the checker's bar, and by how much is printed"""
    sites = _sites(port_oracle, crop)
    H, W, B = CROPS[crop]
    # training: two Disp and one DispAgg; steps.predict: the DispAgg alone, without a gradient
    assert [(s["kind"], s["g_c"] is not None) for s in sites] == [("Disp", True), ("Disp", True), ("DispAgg", True), ("DispAgg", False)]
    assert all(s["x"].shape == (B, standin_net.C, MAX_DISP // 3 + 1, H // 3, W // 3) for s in sites)
    worst = {}
    for s in sites:
        for how in ("numpy", "aten"):
            r = _conv_record(s, how)
            for k, v in M.check_disp_conv(r).items():
                worst["DispConv " + how, k] = max(worst.get(("DispConv " + how, k), 0.0), v)
        if s["kind"] == "Disp":
            assert float(np.abs(s["g_out"]).max()) < 1e-3 and float(np.abs(s["c"]).max()) < 10, "model-scale data"
            for variant in ("plain", "fma"):
                q = M.check_up_softmin_regression(_tail_record(s, variant))
                for k, v in q.items():
                    worst["DispTail " + variant, k] = max(worst.get(("DispTail " + variant, k), 0.0), v)
    print(f"stand-in {crop}: plain fp32 against the float64 statements, largest error / bar (bar: 1)\n" + M.fmt(worst))
    assert {k for _, k in worst} == {"y", "grad_x", "grad_weight", "out"} and max(worst.values()) <= 1.0
    if crop != "48x96":
        del _SITES[crop]


def test_every_disp_tail_record_rejects_a_wrong_result(port_oracle):
    exercised = dict.fromkeys(disp_tail_ref64.MUTATIONS, 0)
    records = [_tail_record(s, "plain") for s in _sites(port_oracle) if s["kind"] == "Disp"]
    assert len(records) == 2
    for r in records:
        S = M.reference_of(r, None)
        got = M.tail_got(r)
        assert set(got) == {"out", "grad_x"}
        M.tail_judge(S, got)                                        # the unspoilt record passes
        for k in got:
            assert _rejected(M.tail_judge, S, {**got, k: np.zeros_like(got[k])}), (r, k, "zeros pass")
            assert _rejected(M.tail_judge, S, _scaled(got, (k,))), (r, k, "scaled passes")
        c4, size = r.args[0][:, 0], r.args[1]
        for what in disp_tail_ref64.MUTATIONS:
            mut = disp_tail_ref64.mutant(c4, size, r.grad_out[0], what)
            if all(np.array_equal(mut[k], S.results()[k].astype(np.float32), equal_nan=True) for k in got):
                continue                                            # the wrong definition gives this record's results: counted
            exercised[what] += 1
            wrong = {k: mut[k] for k in got}
            assert _rejected(M.tail_judge, S, wrong), (r, what)
            for k in got:                                           # ... and each of the two results on its own
                if not np.array_equal(mut[k], S.results()[k].astype(np.float32), equal_nan=True):
                    assert _rejected(M.tail_judge, S, {**got, k: mut[k]}), (r, what, k)
        # "gc_skipped_unwritten" leaves NaN in the planes of the column workspace that no output reads.  A Disp site up-samples
        # D -> 3 (D - 1) + 1 planes: every plane is read, so that wrong definition IS the right one on every record a model
        # can produce (tests/test_sim_disp_tail.py has the down-sampling shapes on which it acts)
        assert not S.ad.unread().any()
    print("records on which each wrong definition changes the result:", exercised)
    assert all(n == len(records) for what, n in exercised.items() if what != "gc_skipped_unwritten"), exercised
    assert exercised["gc_skipped_unwritten"] == 0


def test_every_disp_conv_record_rejects_a_wrong_result(port_oracle):
    exercised = dict.fromkeys(disp_conv_ref64.MUTATIONS, 0)
    records = [_conv_record(s, "numpy") for s in _sites(port_oracle)]
    assert [r.grad_in is not None for r in records] == [True, True, True, False]
    for r in records:
        S = M.reference_of(r, None)
        got = M.conv_got(r)
        assert set(got) == ({"y", "grad_x", "grad_weight"} if r.grad_in is not None else {"y"})
        M.conv_judge(S, got)
        for k in got:
            assert _rejected(M.conv_judge, S, {**got, k: np.zeros_like(got[k])}), (r, k, "zeros pass")
            assert _rejected(M.conv_judge, S, _scaled(got, (k,))), (r, k, "scaled passes")
        gy = r.grad_out[0][:, 0] if r.grad_out is not None else np.zeros(r.outputs[0][:, 0].shape, np.float32)
        for what in disp_conv_ref64.MUTATIONS:
            mut = disp_conv_ref64.mutant(r.args[0], r.args[1], gy, what)
            changed = [k for k in got if not np.array_equal(mut[k], S.results()[k].astype(np.float32))]
            if not changed:
                continue
            exercised[what] += 1
            for k in changed:
                assert _rejected(M.conv_judge, S, {**got, k: mut[k]}), (r, what, k)
    print("records on which each wrong definition changes the result:", exercised)
    assert all(exercised.values()), exercised


# ---- the stand-in and the rebinders -------------------------------------------------------------------------------------------
_HELPERS = ("_fused_sga", "_fused_tail", "_fused_bn", "_fused_conv")


def _rebound(model):
    """name -> (the function its forward was rebound to, the types of its helpers), for every module that holds either"""
    res = {}
    for name, m in model.named_modules():
        held = {h: type(m.__dict__[h]).__name__ for h in _HELPERS if h in m.__dict__}
        fwd = m.__dict__.get("forward")
        if held or fwd is not None:
            res[name] = (getattr(fwd, "__func__", None), held)
    return res


def test_the_rebinders_give_the_same_sites_in_either_order():
    """ops -> bn -> tail -> conv and conv -> tail -> ops -> bn: every site holds a helper of the same type and the same forward,
    state_dict keys do not move.  (use_fused_bn replaces the tail use_fused_ops installs, so these two keep their order.)"""
    from ganet_amd.modules.fused import BnRelu, DispAggTail, DispConv, DispTail, GuidedSGA, GuidedSGABnRelu
    from harness import fuse
    models = []
    for order in (M.REBINDERS, ("use_fused_disp_conv", "use_fused_disp_tail", "use_fused_ops", "use_fused_bn")):
        m = standin_net.build(MAX_DISP)
        keys = list(m.state_dict())
        counts = {rb: getattr(fuse, rb)(m) for rb in order}
        assert list(m.state_dict()) == keys
        models.append((m, counts))
    (a, ca), (b, cb) = models
    assert _rebound(a) == _rebound(b)
    ca_, cb_ = a.cost_agg, b.cost_agg
    for agg in (ca_, cb_):
        assert all(isinstance(d._fused_tail, DispTail) and d.forward.__func__ is fuse._disp_tail_forward for d in (agg.disp0, agg.disp1))
        assert isinstance(agg.disp2._fused_tail, DispAggTail)
        assert all(isinstance(d.conv32x1._fused_conv, DispConv) for d in (agg.disp0, agg.disp1, agg.disp2))
        assert all(isinstance(getattr(agg, k)._fused_sga, GuidedSGABnRelu) for k in ("sga1", "sga11", "sga2")) and isinstance(agg.sga3._fused_sga, GuidedSGA)
        assert all(isinstance(getattr(agg, k)._fused_tail, BnRelu) for k in ("sga1", "sga11", "sga2", "sga3"))
        assert agg.sga3._fused_tail.bn is agg.sga3.bn and agg.sga1._fused_tail.bn is agg.sga1.conv_refine.bn
    # the census of tests/standin_net.py: 4 SGABlocks + 2 Disp + 1 DispAgg; 15 BasicConv with a BatchNorm + the 4 tails; 2 Disp; 3 conv32x1
    n_conv = sum(type(m).__name__ == "BasicConv" and m.use_bn for m in a.modules())
    assert n_conv == 15 and ca == {"use_fused_ops": 7, "use_fused_bn": n_conv + 4, "use_fused_disp_tail": 2, "use_fused_disp_conv": 3}
    # a Disp that already holds a DispTail is not a site of use_fused_ops any more
    assert cb == {**ca, "use_fused_ops": 5}


def _reference_blocks():
    cls = refmodel.model_class("GANet_deep")
    mod = sys.modules[cls.__module__]
    return mod.SGABlock, mod.Disp, mod.DispAgg


def _grads(out, leaves, seed):
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(seed))
    return [t.clone() for t in torch.autograd.grad(out, leaves, g, allow_unused=True)]


@needs_models
def test_the_stand_in_blocks_are_the_reference_blocks(port_oracle):
    """The stand-in stands for the reference: its SGABlock, Disp and DispAgg against the reference's own classes (imported, never
    copied), built with equal arguments and ONE state_dict, on the CPU through the oracle route -- the same bits forward, in
    training and in eval mode, and the same bits in every gradient; and every rebinder of harness.fuse finds the same number
    of sites on both."""
    from oracle.cpu_ops import route_cpu_through_oracle
    from harness import fuse
    RefSGABlock, RefDisp, RefDispAgg = _reference_blocks()
    gen = torch.Generator().manual_seed(5)
    rnd = lambda *shape: torch.randn(*shape, generator=gen)       # noqa: E731
    maxdisp = 6
    pairs = {
        "sga_refine": (RefSGABlock(channels=8, refine=True), standin_net.SGABlock(channels=8, refine=True), (rnd(2, 8, 5, 6, 7), rnd(2, 160, 6, 7))),
        "sga_plain": (RefSGABlock(channels=8, refine=False), standin_net.SGABlock(channels=8, refine=False), (rnd(2, 8, 5, 6, 7), rnd(2, 160, 6, 7))),
        # (the reference's tails are built for 32 channels)
        "disp": (RefDisp(maxdisp), standin_net.Disp(maxdisp, 32), (rnd(2, 32, 3, 4, 5),)),
        "dispagg": (RefDispAgg(maxdisp), standin_net.DispAgg(maxdisp, 32), (rnd(2, 32, 3, 4, 5), rnd(2, 75, 12, 15), rnd(2, 75, 12, 15))),
    }
    for name, (ref, mine, inputs) in pairs.items():
        standin_net.seed_batchnorms(ref, seed=3)
        assert list(mine.state_dict()) == list(ref.state_dict()), name
        mine.load_state_dict(ref.state_dict())
        for m in (ref, mine):
            assert route_cpu_through_oracle(m, port_oracle) > 0
        for mode in ("train", "eval"):
            res = []
            for m in (ref, mine):
                m.train(mode == "train")
                m.zero_grad()
                leaves = [t.clone().requires_grad_() for t in inputs]
                out = m(*leaves)
                res.append([out.detach().clone()] + _grads(out, leaves + list(m.parameters()), 7))
            for k, (x, y) in enumerate(zip(*res)):
                assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), (name, mode, k)
            assert float(res[0][0].abs().max()) > 0
        for x, y in zip(ref.buffers(), mine.buffers()):               # the running statistics moved alike
            assert torch.equal(x, y), name
    # the rebinders: one container of each kind, fresh per rebinder chain
    def container(kind):
        blocks = ((RefSGABlock, RefDisp, RefDispAgg) if kind == "ref" else
                  (standin_net.SGABlock, lambda d: standin_net.Disp(d, 32), lambda d: standin_net.DispAgg(d, 32)))
        net = torch.nn.Module()
        net.a, net.b = blocks[0](channels=8, refine=True), blocks[0](channels=8, refine=False)
        net.d, net.e = blocks[1](maxdisp), blocks[2](maxdisp)
        return net

    for chain in [(rb,) for rb in M.REBINDERS] + [M.REBINDERS, ("use_fused_disp_conv", "use_fused_disp_tail", "use_fused_ops", "use_fused_bn")]:
        ref, mine = container("ref"), container("mine")
        for rb in chain:
            assert getattr(fuse, rb)(ref) == getattr(fuse, rb)(mine), (chain, rb)
        assert _rebound(ref) == _rebound(mine), chain
        assert collections.Counter(type(m).__name__ for m in ref.modules() if "forward" in m.__dict__) == \
            collections.Counter(type(m).__name__ for m in mine.modules() if "forward" in m.__dict__)
