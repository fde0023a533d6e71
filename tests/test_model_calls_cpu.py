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
  the others   every other kind of model_calls.CHECKERS -- LgaRegress, cost volume, the regressions, L1 normalise, softmin,
               trilinear, ResidualRelu, BnApply, BnRelu, DisparityLoss, MyLoss2 -- on records built by hand from what the
               stand-in's CPU run hands to each site (hooks; both crops): a plain fp32 statement of the op stays inside the bar
               (by how much is printed), zeros and a factor 1 + 2^-12 on every compared array are rejected.
  the kink     LgaRegress's sgn(y): an fp32 pass with the other sign where float64 cannot decide is accepted, the same flip
               at decided elements is rejected, and so is every lga_ref64.MUTATIONS entry behind the regression.
  stand-in     tied to the reference where that exists: the reference's SGABlock, Disp and DispAgg and the stand-in's, with one
               state_dict, give the same bits forward and backward, and every rebinder of harness.fuse counts the same sites."""
import collections
import copy
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
import lga_regress_cases as lrc  # noqa: E402
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
_RUNS, _SITES, _OPS = {}, {}, {}


def _ref(*values):
    """a parameter set on a reference model: skipped where its files are missing.  The stand-in's never is."""
    return pytest.param(*values, marks=needs_models)


@pytest.fixture(scope="module", autouse=True)
def _release_the_runs():
    """the records and the float64 references kept on them (hundreds of MB) go when this module's tests are done"""
    yield
    _RUNS.clear()
    _SITES.clear()
    _OPS.clear()


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
            ops = _watch_the_op_sites(model)
        else:
            model = steps.build_model(name, MAX_DISP, "cpu", hook=lambda m: route_cpu_through_oracle(m, oracle))
        left, right, target = steps.synthetic_batch(B, H, W, MAX_DISP, "cpu")
        functions, plain = M.oracle_functions()
        if name == "standin":                                       # pure tensor arithmetic: the product's own Function runs on the CPU
            from ganet_amd.functions.GANet import MyLoss2Function
            functions = functions + [MyLoss2Function]
        with pytest.MonkeyPatch.context() as patch, M.recording(patch, functions, plain) as records:
            model.train()
            outs = model(left, right)
            steps.loss_mix("GANet_deep" if name == "standin" else name, outs, target, target < MAX_DISP, steps.criterion(True)).backward()
            if name == "standin":
                loss_record = records.pop(next(i for i, r in enumerate(records) if r.kind == "MyLoss2Function"))
            n_train = len(records)
            if name == "standin":
                _SITES[crop] = [_site_tensors(s) for s in sites]
                sites.clear()
                train_ops = _op_tensors(ops)
                ops.clear()
            steps.predict(model, left, right)
            if name == "standin":
                _SITES[crop] += [_site_tensors(s) for s in sites]
                _OPS[crop] = {"train": train_ops, "infer": _op_tensors(ops), "myloss2": loss_record, "target": _np32(target),
                              "preds": [_np32(o) for o in outs]}
                for part, recs in (("train", records[:n_train]), ("infer", records[n_train:])):
                    _OPS[crop][part]["lga"] = [_lga_site(r) for r in recs if r.kind == "OracleLgaChain"]
                    _OPS[crop][part]["sga"] = [_sga_site(r) for r in recs if r.kind == "OracleSga"]
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


def _np32(t):
    return None if t is None else np.ascontiguousarray(t.detach().numpy(), np.float32)


def _watch_the_op_sites(model):
    """forward hooks that keep what every OTHER op of model_calls.CHECKERS would be handed at its site in the stand-in (the
    inputs, cloned when they are met, and the gradient that later arrives at the site's output): the cost volume, the raw
    guidance and filter maps in front of the L1 normalisations, every BatchNorm (+ residual) (+ ReLU) site -- BasicConv, and
    the SGABlocks' tails with their residual.  -> the dict the calls are appended to"""
    ops = collections.defaultdict(list)
    met = {}

    def keep_grad(t, d):
        d["g"] = None
        if t.requires_grad:
            t.register_hook(lambda g: d.__setitem__("g", g.detach().clone()))

    def cv_hook(mod, args, out):
        d = {"x": args[0].detach().clone(), "y": args[1].detach().clone(), "Dn": out.shape[2]}
        keep_grad(out, d)
        ops["cv"].append(d)

    def bn_pre(mod, args):
        met[mod] = {"x": args[0].detach().clone(), "weight": mod.weight.detach().clone(), "bias": mod.bias.detach().clone(),
                    "running_mean": mod.running_mean.clone(), "running_var": mod.running_var.clone(), "momentum": mod.momentum,
                    "eps": mod.eps, "training": mod.training}

    def conv_hook(mod, args, out, name):
        d = {**met.pop(mod.bn), "name": name, "rem": None, "relu": bool(mod.relu)}
        keep_grad(out, d)
        ops["bn"].append(d)

    def block_hook(mod, args, out, name):
        d = {**met.pop(mod.conv_refine.bn if mod.refine else mod.bn), "name": name, "rem": args[0].detach().clone(), "relu": True}
        keep_grad(out, d)
        ops["bn"].append(d)

    model.cv.register_forward_hook(cv_hook)
    for key, conv in list(model.weight_sg.items()) + list(model.weight_lg.items()):
        conv.register_forward_hook(lambda mod, args, out, key=key: ops["raw"].append({"key": key, "x": out.detach().clone()}))
    refines = {m.conv_refine for m in model.modules() if type(m).__name__ == "SGABlock" and m.refine}
    for name, m in model.named_modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.register_forward_pre_hook(bn_pre)
        if type(m).__name__ == "BasicConv" and m.use_bn and m not in refines:
            m.register_forward_hook(lambda mod, args, out, name=name: conv_hook(mod, args, out, name))
        elif type(m).__name__ == "SGABlock":
            m.register_forward_hook(lambda mod, args, out, name=name: block_hook(mod, args, out, name))
    return ops


def _op_tensors(ops):
    """host copies of what _watch_the_op_sites has kept so far (after the backward: the gradients have arrived)"""
    conv = lambda v: _np32(v) if isinstance(v, torch.Tensor) else v      # noqa: E731
    return {k: [{kk: conv(v) for kk, v in d.items()} for d in calls] for k, calls in ops.items()}


def _lga_site(r):
    x, f, radius, passes = M._lga_inputs(r)
    g = r.grad_in is not None
    return {"x": x, "f": f, "radius": radius, "passes": passes, "y": r.outputs[0], "gy": r.grad_out[0] if g else None,
            "gx": r.grad_in[1] if g else None, "gf": r.grad_in[2] if g else None}


def _sga_site(r):
    """the four normalised guidance volumes an SGA call got and the gradients it returned for them"""
    return {"ks": list(r.args[2:6]), "gks": list(r.grad_in[2:6]) if r.grad_in is not None else None}


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
    if crop not in _SITES:
        _RUNS.pop(("standin", crop), None)
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


# ---- every other checker of model_calls.CHECKERS, on the stand-in's sites --------------------------------------------------------
# Records built by hand, as above: the inputs and the incoming gradient are what the stand-in's CPU run hands to the site, the
# results are a PLAIN fp32 statement of the op -- numpy with every intermediate float32, or ATen on the CPU where the op is
# ATen's own chain (softmin, trilinear, batch_norm) -- never the device's or the emulator's.  A checker whose bar plain fp32
# cannot meet is too tight and fails a correct kernel now and then; one that accepts zeros or a 2^-12 error checks nothing.
F32 = np.float32
OTHER_KINDS = ("LgaRegressFunction", "GetCostVolumeFunction", "DisparityRegressionFunction", "L1NormalizeGroupsFunction",
               "NormDisparityRegressionFunction", "SoftminFunction", "SoftminDisparityRegressionFunction", "TrilinearUpsampleFunction",
               "ResidualReluFunction", "BnApplyFunction", "BnReluFunction", "DisparityLossFunction", "MyLoss2Function")
COUNTS = ("undecided", "flipped")                       # keys of a checker's dict that are counts, not error / bar


def _ops(oracle, crop="48x96"):
    if crop not in _OPS or crop not in _SITES:
        _RUNS.pop(("standin", crop), None)
        _recorded(oracle, "standin", crop)
    return _OPS[crop], _SITES[crop]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _disp32(D):
    return np.arange(D, dtype=F32).reshape(1, D, 1, 1)


def _cost_volume_record(s):
    x, y, Dn, g = s["x"], s["y"], s["Dn"], s["g"]
    N, C, H, W = x.shape
    cost = np.zeros((N, 2 * C, Dn, H, W), F32)
    for i in range(min(Dn, W)):
        cost[:, :C, i, :, i:], cost[:, C:, i, :, i:] = x[..., i:], y[..., :W - i]
    if g is None:
        return _record("GetCostVolumeFunction", [x, y, Dn], [cost])
    gx, gy = np.zeros_like(x), np.zeros_like(y)
    for i in range(min(Dn, W)):                          # one fp32 addition per plane, in order
        gx[..., i:] += g[:, :C, i, :, i:]
        gy[..., :W - i] += g[:, C:, i, :, i:]
    return _record("GetCostVolumeFunction", [x, y, Dn], [cost], [g], [gx, gy, None])


def _regression_record(x, go):
    D = x.shape[1]
    out = (x * _disp32(D)).sum(1, dtype=F32)
    if go is None:
        return _record("DisparityRegressionFunction", [x, D], [out])
    return _record("DisparityRegressionFunction", [x, D], [out], [go], [go[:, None] * _disp32(D), None])


def _l1_record(x, G, C, K, gys):
    N, _, H, W = x.shape
    x6 = x.reshape(N, G, C, K, H, W)
    s = np.maximum(np.abs(x6).sum(3, keepdims=True, dtype=F32), F32(1e-12))
    y = x6 / s
    outs = [np.ascontiguousarray(y[:, g]) for g in range(G)]
    if gys is None:
        return _record("L1NormalizeGroupsFunction", [x, G, C, K], outs)
    gy = np.stack([g.reshape(N, C, K, H, W) for g in gys], 1)
    dot = (gy * y).sum(3, keepdims=True, dtype=F32)
    gx = ((gy - np.sign(x6) * dot) / s).astype(F32)
    return _record("L1NormalizeGroupsFunction", [x, G, C, K], outs, [g.reshape(N, C, K, H, W) for g in gys], [gx.reshape(x.shape), None, None, None])


def _norm_regression_record(x, go):
    D = x.shape[1]
    s = np.maximum(np.abs(x).sum(1, dtype=F32), F32(1e-12))
    out = (x * _disp32(D)).sum(1, dtype=F32) / s
    if go is None:
        return _record("NormDisparityRegressionFunction", [x, D], [out])
    gx = (go[:, None] * ((_disp32(D) - out[:, None] * np.sign(x)) / s[:, None])).astype(F32)
    return _record("NormDisparityRegressionFunction", [x, D], [out], [go], [gx, None])


def _softmin_record(x, gy):
    xt = _t(x).requires_grad_(gy is not None)
    y = torch.nn.functional.softmin(xt, dim=1)
    if gy is None:
        return _record("SoftminFunction", [x], [_np32(y)])
    return _record("SoftminFunction", [x], [_np32(y)], [gy], [_np32(torch.autograd.grad(y, xt, _t(gy))[0])])


def _softmin_regression_record(x, go):
    D = x.shape[1]
    xt = _t(x).requires_grad_()
    out = (torch.nn.functional.softmin(xt, dim=1) * _t(_disp32(D))).sum(1)
    return _record("SoftminDisparityRegressionFunction", [x, D], [_np32(out)], [go], [_np32(torch.autograd.grad(out, xt, _t(go))[0]), None])


def _upsampled(site, go=None):
    """the trilinear output of a Disp / DispAgg site (ATen, fp32) and, for a Disp, the gradient Softmin + regression hands back
    to it for the site's incoming `go`"""
    u = torch.nn.functional.interpolate(_t(site["c"]), list(_size(site)), mode="trilinear", align_corners=False)[:, 0]
    if go is None:
        return _np32(u), None
    u.requires_grad_()
    out = (torch.nn.functional.softmin(u, dim=1) * _t(_disp32(u.shape[1]))).sum(1)
    return _np32(u), _np32(torch.autograd.grad(out, u, _t(go))[0])


def _trilinear_record(site, gu):
    from misc_cases import _aten_trilinear
    x, size = site["c"], _size(site)
    if gu is None:
        y, _ = _aten_trilinear(x, np.zeros(x.shape[:2] + size, F32), size)
        return _record("TrilinearUpsampleFunction", [x, size], [y])
    y, gx = _aten_trilinear(x, np.ascontiguousarray(gu[:, None]), size)
    return _record("TrilinearUpsampleFunction", [x, size], [y], [np.ascontiguousarray(gu[:, None])], [gx, None])


def _folded(s):
    scale = (s["weight"].astype(F32) / np.sqrt(s["running_var"] + F32(s["eps"]), dtype=F32)).astype(F32)
    return scale, (s["bias"] - s["running_mean"] * scale).astype(F32)


def _affine_relu32(x, rem, scale, shift, relu):
    C = x.shape[1]
    b = lambda v: v.reshape((1, C) + (1,) * (x.ndim - 2))      # noqa: E731
    y = x if scale is None else b(scale) * x + b(shift)
    y = y if rem is None else y + rem
    assert y.dtype == F32
    return np.maximum(y, F32(0)) if relu else y


def _relu_grads32(y, gy, scale, relu):
    g = np.where(y > 0, gy, F32(0)) if relu else gy
    C = y.shape[1]
    return (g if scale is None else scale.reshape((1, C) + (1,) * (y.ndim - 2)) * g), g


def _bn_aten(s):
    """y and the four gradients of relu(batch_norm(x) [+ rem]) with batch statistics by ATen on the CPU, and the running
    statistics it leaves"""
    x, w, b = (_t(s[k]).requires_grad_() for k in ("x", "weight", "bias"))
    rem = None if s["rem"] is None else _t(s["rem"]).requires_grad_()
    rm, rv = _t(s["running_mean"].copy()), _t(s["running_var"].copy())
    y = torch.nn.functional.batch_norm(x, rm, rv, w, b, True, s["momentum"], s["eps"])
    y = y if rem is None else y + rem
    y = torch.relu(y) if s["relu"] else y
    leaves = [x, w, b] + ([rem] if rem is not None else [])
    gs = [_np32(g) for g in torch.autograd.grad(y, leaves, _t(s["g"]))]
    return _np32(y), gs[0], (gs[3] if rem is not None else None), gs[1], gs[2], _np32(rm), _np32(rv)


def _bn_model(s):
    """the same by bn_ref64.Float32Model: fp32 element by element, the per-channel sums in fp64 -- the arithmetic BnRelu's bars
    are derived for (ATen's fp32 sums do not reach them: measured, not asserted, in the calibration below)"""
    import bn_ref64
    N, C = s["x"].shape[:2]
    flat = lambda a: None if a is None else a.reshape(N, C, -1)      # noqa: E731
    m = bn_ref64.Float32Model(flat(s["x"]), flat(s["rem"]), flat(s["g"]), s["weight"], s["bias"], s["running_mean"], s["running_var"],
                              s["momentum"], s["eps"], s["relu"])
    shaped = lambda a: np.ascontiguousarray(a, F32).reshape(s["x"].shape)      # noqa: E731
    return (shaped(m.y), shaped(m.grad_x), shaped(m.grad_rem) if s["rem"] is not None else None, m.grad_weight, m.grad_bias,
            m.running_mean, m.running_var)


def _bn_relu_record(s, how="model"):
    y, gx, grem, gw, gb, rm, rv = (_bn_model if how == "model" else _bn_aten)(s)
    r = _record("BnReluFunction", [s["x"], s["rem"], s["weight"], s["bias"], s["running_mean"], s["running_var"], s["momentum"],
                                   s["eps"], s["relu"]], [y], [s["g"]], [gx, grem, gw, gb] + [None] * 5)
    r.after = {4: rm, 5: rv}
    return r


def _bn_apply_record(s, gy=None):
    scale, shift = _folded(s)
    y = _affine_relu32(s["x"], s["rem"], scale, shift, s["relu"])
    args = [s["x"], s["rem"], scale, shift, s["relu"], False]
    if gy is None:
        return _record("BnApplyFunction", args, [y])
    g_x, g_rem = _relu_grads32(y, gy, scale, s["relu"])
    return _record("BnApplyFunction", args, [y], [gy], [g_x, g_rem if s["rem"] is not None else None, None, None, None, None])


def _residual_relu_record(s, folded, gy=None):
    """an SGABlock's tail as ResidualReluFunction sees it: eval -- the BatchNorm folded; training -- relu(t + rem) on the
    framework's t = bn(.)"""
    if folded:
        t, (scale, shift) = s["x"], _folded(s)
    else:
        xt = _t(s["x"])
        t = _np32(torch.nn.functional.batch_norm(xt, _t(s["running_mean"].copy()), _t(s["running_var"].copy()), _t(s["weight"]), _t(s["bias"]),
                                                 True, s["momentum"], s["eps"]))
        scale = shift = None
    y = _affine_relu32(t, s["rem"], scale, shift, True)
    args = [t, s["rem"], scale, shift, False]
    if gy is None:
        return _record("ResidualReluFunction", args, [y])
    g_t, g_rem = _relu_grads32(y, gy, scale, True)
    return _record("ResidualReluFunction", args, [y], [gy], [g_t, g_rem, None, None, None])


def _rho32(v, kind, thresh=3, alpha=2):
    """loss_ref64.rho64 with every constant and operation fp32"""
    assert v.dtype == F32
    if kind == 0:
        return np.where(v < 1, F32(0.5) * v * v, v - F32(0.5))
    knee, span, far = F32(thresh), F32(alpha), F32(thresh) + F32(alpha)
    v = np.where(v < knee, v * v / knee, v)
    v = np.where((v >= knee) & (v <= far), F32(2) * v - (v - knee) ** 2 / (F32(2) * span) - knee, v)
    return np.where(v > far, v + span / F32(2), v).astype(F32)


def _disparity_loss_record(preds, target):
    """the fused criterion of the stand-in's training step (DisparityLoss.for_model("GANet_deep", MAX_DISP)): sums and means in
    fp32 numpy; the gradients by loss_ref64's own float32 statement -- the checker asks for its bits"""
    import loss_cases
    import loss_ref64
    from ganet_amd.modules.fused import DisparityLoss
    crit = DisparityLoss.for_model("GANet_deep", MAX_DISP)
    params = np.asarray(crit.values, F32)
    p = dict(zip(loss_ref64.PARAMS, params))
    ok = loss_ref64.valid(target, p["hi"], p["lo"], crit.mask_mode)
    n = F32(ok.sum())
    stats, loss = [n], F32(0)
    for k, (q, kind) in enumerate(zip(preds, crit.kinds)):
        v = np.abs(q - target)[ok]
        mean_rho = _rho32(v, kind, p["thresh"], p["alpha"]).sum(dtype=F32) / n
        stats += [mean_rho, v.sum(dtype=F32) / n, F32((v > p["rate"]).sum()) / n]
        loss = loss + p[f"w{k}"] * mean_rho
    c = loss_cases.Case("stand-in", target.shape, preds, target, crit.kinds, [p["w0"], p["w1"], p["w2"]], thresh=p["thresh"], alpha=p["alpha"],
                        mask_mode=crit.mask_mode, hi=p["hi"], lo=p["lo"], rate=p["rate"])
    grads = c.ref.grads(1.0, np.float32)
    return _record("DisparityLossFunction", [target, params, None, crit.kinds, crit.mask_mode] + list(preds), [np.asarray(loss, F32), np.asarray(stats, F32)],
                   [np.asarray(1.0, F32), None], [None] * 5 + grads)


def _lga_regress_site(ops, sites, part, oracle):
    """x: the first pass of the second LGA2 (the oracle's fp32) on the Softmin output, f: its filters, go: what arrives at the
    DispAgg's output"""
    lga = ops[part]["lga"][1]
    x = oracle.lga_forward(lga["x"], lga["f"], lga["radius"])
    go = next(s for s in sites if s["kind"] == "DispAgg" and (s["g_out"] is not None) == (part == "train"))["g_out"]
    return x, lga["f"], lga["radius"], go


def _lga_regress_record(x, f, r, go, y=None):
    return lrc.record(x, f, r, lrc.regress32(x, f, go, r, y), go)


def _other_records(oracle, crop, aten=None):
    """[(what, Record)] for every kind of OTHER_KINDS, training sites (with gradients) and steps.predict's (without).  aten: a
    list that gets the BnRelu records with ATen's results (measured only)"""
    ops, sites = _ops(oracle, crop)
    res, aten = [], [] if aten is None else aten
    add = lambda what, r: res.append((what, r))      # noqa: E731
    dispagg = {part: next(s for s in sites if s["kind"] == "DispAgg" and (s["g_out"] is not None) == (part == "train")) for part in ("train", "infer")}
    disps = [s for s in sites if s["kind"] == "Disp"]
    for part in ("train", "infer"):
        o, go = ops[part], dispagg[part]["g_out"]
        add(f"LgaRegress {part}", _lga_regress_record(*_lga_regress_site(ops, sites, part, oracle)))
        add(f"cost volume {part}", _cost_volume_record(o["cv"][0]))
        lga1, lga2 = o["lga"]
        add(f"softmin {part}", _softmin_record(lga1["y"], lga2["gx"]))
        add(f"normalised regression {part}", _norm_regression_record(lga2["y"], go))
        add(f"regression DispAgg {part}", _regression_record(_np32(torch.nn.functional.normalize(_t(lga2["y"]), p=1, dim=1)), go))
        add(f"trilinear DispAgg {part}", _trilinear_record(dispagg[part], lga1["gx"]))
        # the raw maps are the same in both passes' order: sg1, sg2, sg3, sg11, lg1, lg2 (ModuleDict); the SGA calls: sga1, sga11, sga2, sga3
        raw = {d["key"]: d["x"] for d in o["raw"]}
        for key, sga in zip(("sg1", "sg11", "sg2", "sg3"), o["sga"]):
            C = sga["ks"][0].shape[1]
            r = _l1_record(raw[key], 4, C, 5, sga["gks"])
            assert all(np.allclose(a, b, rtol=1e-6, atol=0) for a, b in zip(r.outputs, sga["ks"])), (key, "not this SGA call's guidance")
            add(f"L1 normalise {key} {part}", r)
        for key, lga in zip(("lg1", "lg2"), o["lga"]):
            r = _l1_record(raw[key], 1, 1, 75, None if lga["gf"] is None else [lga["gf"]])
            assert np.allclose(r.outputs[0][:, 0], lga["f"], rtol=1e-6, atol=0), (key, "not this LGA call's filters")
            add(f"L1 normalise {key} {part}", r)
    for k, s in enumerate(disps):
        u, gu = _upsampled(s, s["g_out"])
        add(f"softmin + regression Disp{k}", _softmin_regression_record(u, s["g_out"]))
        add(f"regression Disp{k}", _regression_record(_np32(torch.nn.functional.softmin(_t(u), dim=1)), s["g_out"]))
        add(f"trilinear Disp{k}", _trilinear_record(s, gu))
    train_bn, infer_bn = ops["train"]["bn"], ops["infer"]["bn"]
    assert [s["name"] for s in train_bn] == [s["name"] for s in infer_bn] and len(train_bn) == 13 + 4
    assert all(s["training"] and s["g"] is not None for s in train_bn) and not any(s["training"] or s["g"] is not None for s in infer_bn)
    for s, e in zip(train_bn, infer_bn):
        add(f"BnRelu {s['name']}", _bn_relu_record(s))
        aten.append((f"BnRelu {s['name']} by ATen", _bn_relu_record(s, "aten")))
        add(f"BnApply {e['name']}", _bn_apply_record(e))
        add(f"BnApply {e['name']} + the training step's gradient", _bn_apply_record(e, s["g"]))
        if s["rem"] is not None:
            add(f"ResidualRelu {s['name']} training", _residual_relu_record(s, False, s["g"]))
            add(f"ResidualRelu {e['name']} folded", _residual_relu_record(e, True))
            add(f"ResidualRelu {e['name']} folded + the training step's gradient", _residual_relu_record(e, True, s["g"]))
    add("DisparityLoss", _disparity_loss_record(_OPS[crop]["preds"], _OPS[crop]["target"]))
    add("MyLoss2", _OPS[crop]["myloss2"])
    assert {r.kind for _, r in res} == set(OTHER_KINDS)
    return res


@pytest.mark.parametrize("crop", ["48x96", "96x240x2"])
def test_plain_fp32_stays_inside_the_bars_of_every_other_checker(port_oracle, crop):
    """calibration, per kind of OTHER_KINDS: the plain fp32 statement is accepted, and the largest error / bar per kind and key
    is printed (profiles/r17a_checker_calibration.txt keeps the figures).  A kind above 0.5 of its bar is named: its bar leaves
    a correct kernel little room.  LgaRegress: the share of undecided elements on the stand-in's data, which the checker's
    cap is set from."""
    worst, report, aten = collections.OrderedDict(), [], []
    for what, r in _other_records(port_oracle, crop, aten):
        q = M.CHECKERS[r.kind](r, port_oracle)
        report.append(f"{what:60s} {r!r}: " + " ".join(f"{k}={v:.3g}" for k, v in q.items()))
        for k, v in q.items():
            worst[r.kind, k] = max(worst.get((r.kind, k), 0.0), v)
        if r.kind == "LgaRegressFunction":
            print(f"stand-in {crop} {what}: {int(q['undecided'])} of {r.args[0].size} elements undecided, share {q['undecided'] / r.args[0].size:.3g}")
    print("\n".join(report))
    print(f"stand-in {crop}: plain fp32 against the float64 statements, largest error / bar (bar: 1)\n" + M.fmt(worst))
    stock = {}
    for what, r in aten:
        for k, v in M.check_bn_relu(r, enforce=False).items():
            stock[k] = max(stock.get(k, 0.0), v)
    print("BnRelu by ATen's batch_norm (fp32 sums; measured, not asserted):", {k: round(v, 3) for k, v in stock.items() if k not in COUNTS})
    ratios = {k: v for k, v in worst.items() if k[1] not in COUNTS}
    print("above half of the bar:", {k: round(v, 3) for k, v in ratios.items() if v > 0.5})
    assert {k for k, _ in worst} == set(OTHER_KINDS) and max(ratios.values()) <= 1.0
    if crop != "48x96":                                             # nobody else uses the large crop
        del _OPS[crop], _SITES[crop]


def _slots(r):
    """every array of a record that its checker compares: (attribute, index)"""
    slots = [("outputs", i) for i, o in enumerate(r.outputs) if isinstance(o, np.ndarray)]
    if r.grad_in is not None:
        slots += [("grad_in", i) for i, g in enumerate(r.grad_in) if g is not None]
    slots += [("after", i) for i in r.after] + [("saved", k) for k in r.saved if k != "snorm"]      # (snorm is kept, not compared)
    return slots


def _spoilt(r, slot, fn):
    attr, i = slot
    s = copy.copy(r)
    held = copy.copy(getattr(r, attr))
    held[i] = fn(held[i])
    setattr(s, attr, held)
    s.reference = None
    return s


# (kind, slot) whose 1 + 2^-12 the checker CANNOT see on the stand-in's data, with the reason; asserted below, so that a bar that
# is tightened later shows up here
INVISIBLE = {}


def test_every_other_checker_rejects_a_wrong_result(port_oracle):
    """teeth, per kind of OTHER_KINDS and per compared array of each record: zeros and a factor 1 + 2^-12 are REJECTED"""
    seen, passed = collections.Counter(), collections.defaultdict(list)
    for what, r in _other_records(port_oracle, "48x96"):
        check = M.CHECKERS[r.kind]
        check(r, port_oracle)                                       # the unspoilt record passes
        for slot in _slots(r):
            a = getattr(r, slot[0])[slot[1]]
            if not np.any(a):
                continue                                            # (an all-zero gradient: nothing to spoil)
            seen[r.kind, slot[0]] += 1
            assert _rejected(check, _spoilt(r, slot, np.zeros_like), port_oracle), (what, slot, "zeros pass")
            if not _rejected(check, _spoilt(r, slot, lambda v: (v * F32(1 + 2.0 ** -12)).astype(v.dtype)), port_oracle):
                passed[r.kind, slot].append(what)
    print("spoilt arrays per kind:", dict(seen))
    print("a factor 1 + 2^-12 passes:", dict(passed))
    assert set(passed) == set(INVISIBLE), (set(passed) ^ set(INVISIBLE), "scaled results that pass / bars that see them now")
    assert {k for k, _ in seen} == set(OTHER_KINDS)
    assert all(seen[k, "grad_in"] for k in OTHER_KINDS), "a kind without a gradient to spoil"


# ---- LgaRegress: the LGA part, and the sign kink both ways -------------------------------------------------------------------------
def _kink_site(oracle):
    x, f, r, go = _lga_regress_site(*_ops(oracle), "train", oracle)
    y64, E_y, und = M.lga_regress_undecided(x, f, r)
    return x, f, r, go, y64, E_y, und


def test_lga_regress_rejects_a_wrong_lga_pass(port_oracle):
    """lga_ref64.MUTATIONS behind the regression: a dropped tap, zero padding -- in the whole op, and in each result alone"""
    x, f, r, go, y64, E_y, und = _kink_site(port_oracle)
    good = lrc.regress32(x, f, go, r)
    M.check_lga_regress(lrc.record(x, f, r, good, go))
    for what in lga_ref64.MUTATIONS:
        y = lga_ref64.lga_forward(x, f, r, what).astype(F32)
        bad = lrc.regress32(x, f, go, r, y)                          # the regression and its adjoint on the wrong pass ...
        gy = M.m64.norm_regression_adjoint(y64, go)
        bad["gx"], bad["gf"] = (g.astype(F32) for g in lga_ref64.lga_backward(x, f, gy, r, what))      # ... and the wrong adjoints of the right one
        assert _rejected(M.check_lga_regress, lrc.record(x, f, r, bad, go)), what
        for k in ("y", "out", "gx", "gf"):
            assert _rejected(M.check_lga_regress, lrc.record(x, f, r, {**good, k: bad[k]}, go)), (what, k)


def test_lga_regress_takes_the_calls_sign_where_float64_cannot_decide_and_nowhere_else(port_oracle):
    """The experiment behind check_lga_regress's treatment of sgn(y), kept: on the stand-in's LgaRegress site an fp32 pass whose y
    has the OTHER sign at the elements with |y64| <= chain_bound (no factor: -y64 is then within FACTOR x the bound of y64)
    is accepted -- with sgn taken from float64 its gx stood at 16 .. 42 x the bar, the failure a device run showed now and
    then.  The same flip at the decided elements nearest to the kink is rejected, by the name "sign"; and so is a backward
    that used the wrong sign at ONE decided element while its y is right."""
    x, f, r, go, y64, E_y, und = _kink_site(port_oracle)
    y = lrc.forward32(x, f, r)
    near = np.abs(y64) <= E_y / M.FACTOR
    assert near.sum() >= 2 and und[near].all(), int(near.sum())
    flipped = np.where(near, -y64, y).astype(F32)
    q = M.check_lga_regress(lrc.record(x, f, r, lrc.regress32(x, f, go, r, flipped), go))
    assert q["flipped"] == near.sum() and q["undecided"] == und.sum()
    print(f"{int(near.sum())} of {int(und.sum())} undecided elements flipped: accepted,", " ".join(f"{k}={v:.3g}" for k, v in q.items()))
    # decided elements, the nearest to the kink first
    margin = np.where(und, np.inf, np.abs(y64) / np.maximum(E_y, 1e-300))
    first = np.unravel_index(np.argsort(margin, axis=None)[:int(near.sum())], y64.shape)
    decided = np.zeros(y64.shape, bool)
    decided[first] = True
    assert not und[decided].any() and margin[decided].min() > 1
    wrong = np.where(decided, -y64, y).astype(F32)
    with pytest.raises(AssertionError, match="sign"):
        M.check_lga_regress(lrc.record(x, f, r, lrc.regress32(x, f, go, r, wrong), go))
    # the right y kept, the wrong sign used at one decided element -- one with a gradient to show for it
    good = lrc.regress32(x, f, go, r)
    lever = np.where(und, 0.0, np.abs(go[:, None] * good["out"][:, None] / good["snorm"][:, None]) * np.ones(y64.shape))
    one = np.zeros(y64.shape, bool)
    one[np.unravel_index(np.argmax(lever), y64.shape)] = True
    bad = lrc.regress32(x, f, go, r, np.where(one, -y, y))
    with pytest.raises(AssertionError, match="gx"):
        M.check_lga_regress(lrc.record(x, f, r, {**good, "gx": bad["gx"], "gf": bad["gf"]}, go))


# ---- the stand-in and the rebinders -------------------------------------------------------------------------------------------
_HELPERS =("_fused_sga", "_fused_tail", "_fused_bn", "_fused_conv")


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


# ---- the mixed-precision kinds: calibration on a numpy model, teeth, completeness ----------------------------------------------------
def _mixed_records(oracle, fmt):
    """[(what, Record)] of every kind of model_calls.MIXED_CHECKERS, built by tests/mixed_call_cases.py from what the stand-in's CPU
    run hands to each site at 48 x 96 (training: with the gradients that reached it; steps.predict: the inference forms)"""
    import mixed_call_cases as mcc
    ops, sites = _ops(oracle)
    tr, inf = ops["train"], ops["infer"]
    res = []
    for k, s in enumerate(x for x in sites if x["g_c"] is not None):
        res += [(f"cast {s['name']}", r) for r in mcc.cast_records(s["c"], s["g_c"], fmt)]
    res += [("cost volume", r) for r in mcc.cost_volume_records(tr["cv"][0], fmt)]
    raw = {d["key"]: d["x"] for d in tr["raw"]}
    for key, sga in zip(("sg1", "sg11", "sg2", "sg3"), tr["sga"]):
        res += [(f"guidance {key}", r) for r in mcc.l1_records(raw[key], 4, sga["ks"][0].shape[1], 5, sga["gks"], fmt,
                                                              "NormalizeGuidanceMixedFunction", "normalize_guidance_mixed")]
    for key, lga in zip(("lg1", "lg2"), tr["lga"]):
        res += [(f"filters {key}", r) for r in mcc.l1_records(raw[key], 1, 1, 75, [lga["gf"]], fmt,
                                                              "NormalizeFiltersMixedFunction", "normalize_filters_mixed")]
    for s, e in zip(tr["bn"], inf["bn"]):
        res.append((f"BatchNorm {s['name']}", mcc.bn_train_record(s, fmt)))
        res.append((f"folded BatchNorm {e['name']}", mcc.bn_apply_record(e, fmt)))
    assert {r.kind for _, r in res} == set(M.MIXED_CHECKERS)
    sites_seen = {r.site for _, r in res if r.kind == "MixedBnReluFunction"}
    assert sites_seen == {"conv", "pre-sga", "tail"}, sites_seen
    return res


@pytest.mark.parametrize("fmt", [2, 1], ids=["bf16", "f16"])
def test_the_numpy_model_stays_inside_the_bars_of_the_mixed_checkers_and_every_mutation_is_rejected(port_oracle, fmt):
    """calibration and teeth of every kind of model_calls.MIXED_CHECKERS, per format (fp16: gradients at 256 times their size, as
    under GradScaler(init_scale=256)): each table's statement -- fp32 on the up-cast, converted once -- is accepted with largest
    error / bar <= 1 (printed; profiles/r21a_mixed_calls.txt keeps the figures), and every mutation of tests/mixed_call_cases.py is
    REJECTED on every record it applies to."""
    import mixed_call_cases as mcc
    import mixed_cases as mxc
    assert fmt in mcc.FMTS
    worst, applied = collections.OrderedDict(), collections.Counter()
    for what, r in _mixed_records(port_oracle, fmt):
        check = M.CHECKERS[r.kind]
        q = check(r, port_oracle)
        for k, v in q.items():
            worst[r.kind, k] = max(worst.get((r.kind, k), 0.0), v)
        for name, slot, bad in mcc.mutations(r):
            applied[r.kind, name] += 1
            assert _rejected(check, bad, port_oracle), (what, r.kind, name, slot, "passes")
    print(f"numpy model {mxc.FMT_NAME[fmt]}, stand-in data 48x96: largest error / bar (bar: 1)\n" + M.fmt(worst))
    print("mutations rejected, per kind:", dict(applied))
    ratios = {k: v for k, v in worst.items() if k[1] not in COUNTS}
    assert max(ratios.values()) <= 1.0, {k: v for k, v in ratios.items() if v > 1.0}
    for kind in ("MixedBnReluFunction", "CostVolume16Function", "NormalizeGuidanceMixedFunction", "NormalizeFiltersMixedFunction", "CastFunction"):
        assert all(applied[kind, m] for m in ("zeros", "truncated", "twice", "x256")), (kind, dict(applied))
    assert all(applied[k, "one term"] for k in ("MixedBnReluFunction", "CostVolume16Function", "NormalizeGuidanceMixedFunction",
                                                "NormalizeFiltersMixedFunction"))
    assert all(applied[k, "zeros"] for k in M.MIXED_PLAIN) and all(applied[k, m] for k in ("cast", "bn_apply_mixed") for m in ("truncated", "twice"))


# a mixed-precision name that no checker applies to, with the reason
MIXED_NOT_APPLICABLE = {
    "_l1_groups": "the private launcher behind normalize_guidance_mixed and normalize_filters_mixed, its only callers: both are wrapped and checked",
    "TYPE_CODE": "a table of dtype codes, not an op",
}


def test_every_mixed_precision_op_is_recorded_and_has_a_checker():
    """completeness: every name of functions.mixed_train.__all__ and every function of functions/mixed.py that launches a kernel (its
    source calls into the native library) or is exported is wrapped by product_functions() AND has a checker, or stands in
    MIXED_NOT_APPLICABLE with its reason"""
    import inspect
    import ganet_amd.functions.mixed as fm
    import ganet_amd.functions.mixed_train as ft
    fns, plain = M.product_functions()
    wrapped = {f.__name__ for f in fns} | {name for _, name in plain}
    launching = {n for n, f in vars(fm).items() if inspect.isfunction(f) and f.__module__ == fm.__name__ and '.call("ganet_' in inspect.getsource(f)}
    assert {"cast", "bn_apply_mixed", "cost_volume_16", "_l1_groups"} <= launching
    names = set(ft.__all__) | set(fm.__all__) | launching
    assert len(ft.__all__) == 5 and set(M.MIXED_PLAIN) <= names
    for n in sorted(names):
        if n in MIXED_NOT_APPLICABLE:
            assert n not in M.CHECKERS and MIXED_NOT_APPLICABLE[n]
        else:
            assert n in wrapped and n in M.CHECKERS, (n, "not recorded or not checked")
    assert set(MIXED_NOT_APPLICABLE) <= names
    # the owners are EVERY module of the product that binds the name (all of its modules that hold op call sites are loaded first)
    import importlib
    for mod in ("ganet_amd.modules.GANet", "ganet_amd.modules.fused", "ganet_amd.modules.mixed", "harness.fuse", "harness.steps", "harness.predict",
                "harness.infer", "harness.train"):
        importlib.import_module(mod)
    for owners, name in plain:
        orig = getattr(owners[0], name)
        binders = {m.__name__ for m in sys.modules.values() if getattr(m, "__name__", "").split(".")[0] in ("ganet_amd", "harness")
                   and m.__dict__.get(name) is orig}
        assert binders == {o.__name__ for o in owners}, (name, binders)


def test_the_recorder_keeps_16_bit_tensors_as_bits():
    """model_calls._host on fp16 / bf16: the patterns with their tag, the up-cast exact, a changed bit noticed; fp32 and integer
    tensors as before"""
    import mixed_cases as mxc
    f = torch.tensor([1.0, -2.5, 3.1415927, 65504.0, 1e-8, float("nan")])
    for dt, fmt in ((torch.bfloat16, mxc.BF16), (torch.float16, mxc.F16)):
        t = f.to(dt)
        a = M._host(t)
        assert isinstance(a, M.Half) and a.fmt == fmt and a.dtype == np.uint16 and a.shape == (6,)
        assert np.array_equal(M.up(a)[:5], t.float().numpy()[:5]) and np.isnan(M.up(a)[5])
        assert np.array_equal(np.asarray(a)[:5], mxc.convert(f.numpy(), fmt)[:5])                    # (a NaN's payload aside)
        assert M._same(t, a) and np.zeros_like(a).fmt == fmt and a.reshape(2, 3).fmt == fmt
        assert not M._same(t.view(torch.float16 if dt == torch.bfloat16 else torch.bfloat16), a)     # the same bits under the other tag
        t[0] = 1.0078125                                                                             # one ulp of bf16 above 1
        assert not M._same(t, a)
    a = M._host(f)
    assert type(a) is np.ndarray and a.dtype == np.float32 and M.up(a) is a and M._same(f, a)
    i = torch.arange(4, dtype=torch.int32)
    assert M._host(i).dtype == np.int32 and M._same(i, M._host(i))
