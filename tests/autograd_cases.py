"""TEST INFRASTRUCTURE: one case table for the autograd layer (ganet_amd/functions/GANet.py, functions/fused.py and
modules/fused.py), used by tests/test_gpu_autograd.py.  One entry per op and host path:

  make(seed, family) -> Data    numpy inputs (the differentiable ones), constants, one incoming gradient per output --
                                at the smallest shapes that still reach the op's distinct host paths
  apply(torch, ins, consts)     the call through the autograd Function / module -> tuple of outputs (the first `ndiff`
                                are differentiable)
  check(data, outs, grads)      the yardstick: the oracle port or the float64 statements the suite already holds
                                (lga_ref64 / misc_ref64 / loss_ref64), with the bars of parity_cases / misc_cases / loss_cases
  env                           environment variables the Function reads (set around every run of the case)

The default inputs are EXACT families wherever the op has one (select / lga_inputs_exact / integers / dyadic): every
dispatch -- scalar twins, realigned copies, the inference path -- then returns the same bits, so the properties of
test_gpu_autograd.py ask for bit equality with the plain call and never for a bar."""
import contextlib
import os

import numpy as np

import lga_ref64
import loss_cases as lc
import misc_cases as mc
import misc_ref64 as r64
import parity_cases as pc

F32 = np.float32


class Data:
    def __init__(self, inputs, go, consts=()):
        self.inputs = [np.array(a, F32, order="C") for a in inputs]          # (np.array: a 0-d gradient stays 0-d)
        self.consts = [np.array(a, F32, order="C") for a in consts]
        self.go = [np.array(g, F32, order="C") for g in go]


class Case:
    ndiff = 1            # differentiable outputs (they come first)
    families = 1         # value families make() knows (graph replays rotate through them)
    env = {}
    inplace = False

    def __init__(self, id):
        self.id = id

    def __repr__(self):
        return self.id

    @contextlib.contextmanager
    def environ(self):
        old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)
        try:
            yield
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v


def _equal(name, got, want):
    return mc.Cmp(name, got, want, "equal")


def _close(name, got, want, rtol, atol, rel_only=None):
    return mc.Cmp(name, got, want, "close", rtol, atol, rel_only=rel_only)


# ---- SGA -------------------------------------------------------------------------------------------------------------------------
class Sga(Case):
    """SgaFunction on the select family (parity_cases.sga_inputs_select: equality with the oracle, gradients included);
    family 1 = dyadic, for the graph replays.  [1,2,9,4,16]: tiled workspace, row and column kernels; [1,2,9,5,7]: the
    scalar fallbacks.  D = 9 >= 6 and 64 / 35 pixels per slice: the tie floors of parity_cases.SGA_TIE_FLOORS hold."""
    families = 2

    def __init__(self, shape, save):
        super().__init__("sga-%s-%s" % ("x".join(map(str, shape)), save or "default"))
        self.shape, self.env = shape, {"GANET_SGA_SAVE": save}
        self.oracle = None                         # set by the test module (the session's port oracle)

    def make(self, seed=0, family=0):
        x, gs, go = (pc.sga_inputs_select, pc.sga_inputs_dyadic)[family](self.shape, 1000 + seed)
        return Data([x] + gs, [go])

    def apply(self, torch, ins, consts):
        from ganet_amd.functions.GANet import SgaFunction
        return (SgaFunction.apply(*ins),)

    def check(self, data, outs, grads):
        x, gs, go = data.inputs[0], data.inputs[1:], data.go[0]
        pc.assert_select_exact(x, gs, go)
        want = pc.oracle_sga_want(self.oracle, x, gs, go)
        pc.assert_sga_ties("select", [want[f"A{d}"] for d in range(4)])
        mc.check([_equal("out", outs[0], want["out"]), _equal("gx", grads[0], want["gx"])] +
                 [_equal(f"gw{d}", grads[1 + d], want[f"gw{d}"]) for d in range(4)])


# ---- LGA chains ------------------------------------------------------------------------------------------------------------------
class Lga(Case):
    """Lga / Lga2 / Lga3 and the 5-D forms on parity_cases.lga_inputs_exact: EQUAL to the float64 chain of lga_ref64."""

    def __init__(self, fn, passes, five_d, shape, r, env=None, tag=""):
        if five_d:
            shape = (1, 2) + tuple(shape[1:])
        super().__init__("%s-%s-r%d%s" % (fn, "x".join(map(str, shape)), r, tag))
        self.fn, self.passes, self.shape, self.r, self.env = fn, passes, shape, r, dict(env or {})

    def make(self, seed=0, family=0):
        x, f, gy = pc.lga_inputs_exact(self.shape, self.r, 2000 + seed)
        return Data([x, f], [gy])

    def apply(self, torch, ins, consts):
        import ganet_amd.functions.GANet as G
        return (getattr(G, self.fn).apply(ins[0], ins[1], self.r),)

    def check(self, data, outs, grads):
        x, f = data.inputs
        want = lga_ref64.assert_lga_exact(x, f, data.go[0], self.r, self.passes)
        mc.check([_equal("y", outs[0], want["y"]), _equal("gx", grads[0], want["gx"]), _equal("gf", grads[1], want["gf"])])


LGA_FORMS = [("LgaFunction", 1, False), ("Lga2Function", 2, False), ("Lga3Function", 3, False),
             ("Lga3dFunction", 1, True), ("Lga3d2Function", 2, True), ("Lga3d3Function", 3, True)]


def _lga_cases():
    forms = {name: (name, p, five) for name, p, five in LGA_FORMS}
    # r = 2, even W: the two-pass forms run paired.  Three passes: D = 4, so that the filter gradient (a sum over D of products
    # that carry two filter factors) stays on fp32's grid -- lga_ref64.assert_lga_exact
    cs = [Lga(*form, (1, 4, 3, 36) if form[1] == 3 else (1, 9, 3, 36), 2) for form in LGA_FORMS]
    for name in ("Lga2Function", "Lga3d2Function"):
        cs.append(Lga(*forms[name], (1, 9, 3, 36), 2, {"GANET_LGA_EDGES": "0"}, "-edges0"))
        cs.append(Lga(*forms[name], (1, 9, 3, 36), 2, {"GANET_LGA_PAIRED": "0"}, "-paired0"))
    for name in ("LgaFunction", "Lga2Function", "Lga3d2Function", "Lga3Function"):
        cs.append(Lga(*forms[name], (1, 5, 4, 7), 2, tag="-oddW"))                 # odd W: the planar fallback of the pair
    for name in ("LgaFunction", "Lga2Function", "Lga3d3Function"):
        cs.append(Lga(*forms[name], (1, 7, 4, 40), 1))
    for name in ("LgaFunction", "Lga2Function", "Lga3dFunction"):                  # (147 taps: three passes leave the grid)
        cs.append(Lga(*forms[name], (1, 5, 2, 36), 3))
    return cs


# ---- cost volume, regression ------------------------------------------------------------------------------------------------------
class CostVolume(Case):
    """integer x, y, gradient: copies forward, exact sums backward -- EQUAL to misc_ref64"""
    N, C, H, W, Dn = 1, 2, 3, 8, 5

    def make(self, seed=0, family=0):
        rng = np.random.default_rng(3000 + seed)
        x, y = (rng.integers(-3, 4, (self.N, self.C, self.H, self.W)) for _ in range(2))
        return Data([x, y], [rng.integers(-3, 4, (self.N, 2 * self.C, self.Dn, self.H, self.W))])

    def apply(self, torch, ins, consts):
        from ganet_amd.functions.GANet import GetCostVolumeFunction
        return (GetCostVolumeFunction.apply(ins[0], ins[1], self.Dn),)

    def check(self, data, outs, grads):
        wgx, wgy = r64.cost_volume_adjoint(data.go[0], self.C)
        mc.check([_equal("cost", outs[0], r64.cost_volume(*data.inputs, self.Dn)), _equal("gx", grads[0], wgx), _equal("gy", grads[1], wgy)])


class DispReg(Case):
    N, D, H, W = 2, 9, 3, 5

    def make(self, seed=0, family=0):
        rng = np.random.default_rng(3100 + seed)
        return Data([rng.integers(0, 9, (self.N, self.D, self.H, self.W))], [rng.integers(-4, 5, (self.N, self.H, self.W))])

    def apply(self, torch, ins, consts):
        from ganet_amd.functions.GANet import DisparityRegressionFunction
        return (DisparityRegressionFunction.apply(ins[0], self.D),)

    def check(self, data, outs, grads):
        mc.check([_equal("out", outs[0], r64.regression(data.inputs[0])), _equal("gx", grads[0], r64.regression_adjoint(data.go[0], self.D))])


# ---- the fused normalisations ------------------------------------------------------------------------------------------------------
class L1Norm(Case):
    """L1NormalizeGroupsFunction: G = 4, K = 5 (SGABlock's guidance) and G = 1 (LGA filters); misc_cases.l1norm's bars"""
    N, C, H, W = 2, 2, 3, 5

    def __init__(self, G, K):
        super().__init__(f"l1norm-G{G}-K{K}")
        self.G, self.K, self.ndiff = G, K, G
        if G == 1:
            self.C = 1

    def make(self, seed=0, family=0):
        rng = np.random.default_rng(3200 + seed)
        shape = (self.N, self.G, self.C, self.K, self.H, self.W)
        x = rng.standard_normal(shape) * (rng.random(shape) > 0.3)
        x[0, 0, 0, :, 0, 0] = 0.0                                        # an all-zero group: the clamped norm
        return Data([x.reshape(self.N, -1, self.H, self.W)], list(rng.standard_normal((self.G, self.N, self.C, self.K, self.H, self.W))))

    def apply(self, torch, ins, consts):
        from ganet_amd.functions.fused import L1NormalizeGroupsFunction
        return tuple(L1NormalizeGroupsFunction.apply(ins[0], self.G, self.C, self.K))

    def check(self, data, outs, grads):
        x = data.inputs[0].reshape(self.N, self.G, self.C, self.K, self.H, self.W)
        want, clamped = r64.l1_normalize(x, 3), r64.l1_clamped(x, 3)
        assert clamped.any() and not clamped.all()
        cmps = []
        for g in range(self.G):
            cmps += [_close(f"y{g}", outs[g], want[:, g], 1e-5, 1e-6, clamped[:, g]), mc.Cmp(f"y{g} zero set", outs[g], x[:, g] == 0, "zeros")]
        wgx = r64.l1_normalize_adjoint(x, np.stack(data.go, 1), 3)
        cmps.append(_close("gx", grads[0].reshape(x.shape), wgx, 1e-4, 1e-5, clamped))
        mc.check(cmps)


class NormReg(Case):
    """NormDisparityRegressionFunction on an exact family: integer x whose L1 norm over D is 32 at every pixel, integer
    gradient.  out = sum d x / 32 and gx = go (d - out sgn x) / 32 are then dyadic and small, so the 16-byte form of the
    backward ((go / s) * t) and its scalar twin (go * (t / s)) return the same bits -- EQUAL to misc_ref64.  (The clamped
    norm, where they may differ in the last bit, is misc_cases' business.)"""
    N, D, H, W = 1, 9, 2, 4

    def make(self, seed=0, family=0):
        rng = np.random.default_rng(3250 + seed)
        x = rng.integers(-3, 4, (self.N, self.D, self.H, self.W))
        x[0, 1::2, 0, 3] = 0                                                   # sgn(0) = 0
        x[:, self.D - 1] = (32 - np.abs(x[:, :self.D - 1]).sum(1)) * rng.choice([-1, 1], (self.N, self.H, self.W))
        assert (np.abs(x).sum(1) == 32).all()
        return Data([x], [rng.integers(-4, 5, (self.N, self.H, self.W))])

    def apply(self, torch, ins, consts):
        from ganet_amd.functions.fused import NormDisparityRegressionFunction
        return (NormDisparityRegressionFunction.apply(ins[0], self.D),)

    def check(self, data, outs, grads):
        x = data.inputs[0]
        wout, _ = r64.norm_regression(x)
        mc.check([_equal("out", outs[0], wout), _equal("gx", grads[0], r64.norm_regression_adjoint(x, data.go[0]))])


class Softmin(Case):
    """the backward is a function of the OUTPUT: compared with the float64 adjoint at the y the forward returned"""
    N, D, H, W = 1, 13, 3, 5

    def make(self, seed=0, family=0):
        """as misc_cases.softmin_inputs: 5 * randn and the columns +1e4 .. -1e4, constant, +300 .. -300"""
        rng = np.random.default_rng(3300 + seed)
        x = 5 * rng.standard_normal((self.N, self.D, self.H * self.W))
        x[0, :, 0], x[0, :, 1], x[0, :, 2] = np.linspace(1e4, -1e4, self.D), 7.25, np.linspace(300.0, -300.0, self.D)
        x = x.reshape(self.N, self.D, self.H, self.W)
        return Data([x], [rng.standard_normal(x.shape)])

    def apply(self, torch, ins, consts):
        from ganet_amd.functions.fused import SoftminFunction
        return (SoftminFunction.apply(ins[0]),)

    def check(self, data, outs, grads):
        mc.check([_close("y", outs[0], r64.softmin(data.inputs[0]), 2e-6, 1e-7),
                  _close("gx", grads[0], r64.softmin_adjoint(outs[0], data.go[0]), 1e-5, 1e-5)])


class SoftminReg(Softmin):
    def make(self, seed=0, family=0):
        d = super().make(seed, family)
        return Data(d.inputs, [np.random.default_rng(3350 + seed).standard_normal((self.N, self.H, self.W))])

    def apply(self, torch, ins, consts):
        from ganet_amd.functions.fused import SoftminDisparityRegressionFunction
        return (SoftminDisparityRegressionFunction.apply(ins[0], self.D),)

    def check(self, data, outs, grads):
        x = data.inputs[0]
        mc.check([_close("out", outs[0], r64.softmin_regression(x), 1e-5, 1e-4),
                  _close("gx", grads[0], r64.softmin_regression_adjoint(x, data.go[0]), 1e-4, 1e-4)])


class Trilinear(Case):
    """x2 on every axis: the weights are 1/4 and 3/4, so integer inputs make every product and sum exact -- EQUAL to ATen on
    the CPU (misc_ref64 has no float64 statement of this op, see there)"""
    ISZ, OSZ = (3, 4, 5), (6, 8, 10)

    def make(self, seed=0, family=0):
        rng = np.random.default_rng(3400 + seed)
        return Data([rng.integers(-8, 9, (1, 2) + self.ISZ)], [rng.integers(-8, 9, (1, 2) + self.OSZ)])

    def apply(self, torch, ins, consts):
        from ganet_amd.functions.fused import TrilinearUpsampleFunction
        return (TrilinearUpsampleFunction.apply(ins[0], self.OSZ),)

    def check(self, data, outs, grads):
        wy, wgx = mc._aten_trilinear(data.inputs[0], data.go[0], self.OSZ)
        for v in (wy, wgx):
            assert np.array_equal(v * 64, np.round(v * 64))
        mc.check([_equal("y", outs[0], wy), _equal("gx", grads[0], wgx)])


class LgaRegress(Case):
    """LgaRegressFunction: r = 2 runs the fused kernel, r = 3 its E_UNSUPPORTED fallback (two separate entries).  Exact family:
    x in {-1, +1}, filters with ONE tap of +-1 per pixel, D = 8, integer gradient -- every |y| is 1, so the L1 norm over D is 8
    at every pixel and the normalised regression and both adjoints stay dyadic (see NormReg).  EQUAL to lga_ref64's pass
    pushed through misc_ref64's normalised regression."""

    def __init__(self, shape, r):
        super().__init__("lgaregress-%s-r%d" % ("x".join(map(str, shape)), r))
        self.shape, self.r = shape, r
        assert shape[1] == 8

    def make(self, seed=0, family=0):
        rng = np.random.default_rng(3500 + seed)
        B, D, H, W = self.shape
        T = 3 * (2 * self.r + 1) ** 2
        x = rng.choice([-1.0, 1.0], self.shape)
        f = np.zeros((B, T, H, W))
        np.put_along_axis(f, rng.integers(0, T, (B, 1, H, W)), rng.choice([-1.0, 1.0], (B, 1, H, W)), axis=1)
        return Data([x, f], [rng.integers(-4, 5, (B, H, W))])

    def apply(self, torch, ins, consts):
        from ganet_amd.functions.fused import LgaRegressFunction
        return (LgaRegressFunction.apply(ins[0], ins[1], self.r, self.shape[1]),)

    def check(self, data, outs, grads):
        x, f = data.inputs
        y = lga_ref64.lga_forward(x, f, self.r)
        assert (np.abs(y) == 1).all()
        wout, _ = r64.norm_regression(y)
        wgx, wgf = lga_ref64.lga_backward(x, f, r64.norm_regression_adjoint(y, data.go[0]), self.r)
        mc.check([_equal("out", outs[0], wout), _equal("gx", grads[0], wgx), _equal("gf", grads[1], wgf)])


class Residual(Case):
    """ResidualReluFunction on dyadic values (misc_cases.residual): EQUAL to float64.  `inplace`: y overwrites t, which has to
    be a temporary -- autograd refuses the write to a leaf -- so apply() hands the Function a clone of the leaf."""
    SHAPE = (2, 3, 2, 3, 5)

    def __init__(self, scaled, inplace):
        super().__init__("residual-%s-%s" % ("scaled" if scaled else "unscaled", "inplace" if inplace else "outofplace"))
        self.scaled, self.inplace = scaled, inplace

    def make(self, seed=0, family=0):
        rng = np.random.default_rng(3600 + seed)
        t, rem, gy = (mc._dyadic(rng, self.SHAPE) for _ in range(3))
        consts = [mc._dyadic(rng, self.SHAPE[1]), mc._dyadic(rng, self.SHAPE[1])] if self.scaled else []
        return Data([t, rem], [gy], consts)

    def apply(self, torch, ins, consts):
        from ganet_amd.functions.fused import ResidualReluFunction
        t = ins[0].clone() if self.inplace else ins[0]
        return (ResidualReluFunction.apply(t, ins[1], *(consts if self.scaled else (None, None)), self.inplace),)

    def check(self, data, outs, grads):
        sc, sh = data.consts if self.scaled else (None, None)
        want = r64.residual_relu(*data.inputs, sc, sh)
        assert 0.2 < (want == 0).mean() < 0.8
        w_t, w_rem = r64.residual_relu_adjoint(want, data.go[0], sc)
        mc.check([_equal("y", outs[0], want), mc.Cmp("y zero set", outs[0], want == 0, "zeros"),
                  _equal("g_t", grads[0], w_t), _equal("g_rem", grads[1], w_rem)])


class Loss(Case):
    """DisparityLoss.ganet_deep through one module instance (its parameter tensor and workspace are created by the first
    call); yardstick and bars: loss_cases / loss_ref64.  outputs: (loss, stats), the statistics not differentiable."""
    SHAPE = (2, 4, 6)

    def __init__(self, id):
        super().__init__(id)
        self.module = None

    def make(self, seed=0, family=0):
        preds, t = lc.random_maps(3700 + seed, self.SHAPE, 3)
        return Data([p.reshape(self.SHAPE) for p in preds], [np.asarray(0.37 + seed, F32)], [t.reshape(self.SHAPE)])

    def new_module(self):
        from ganet_amd.modules.fused import DisparityLoss
        return DisparityLoss.ganet_deep(lc.HI, kitti=True)

    def apply(self, torch, ins, consts):
        if self.module is None:
            self.module = self.new_module()
        return tuple(self.module(list(ins), consts[0]))

    def as_loss_case(self, data):
        return lc.Case(self.id, self.SHAPE, data.inputs, data.consts[0], (0, 0, 1), lc.DEEP, thresh=3, alpha=2)

    def check(self, data, outs, grads):
        case = self.as_loss_case(data)
        assert 0 < case.ref.count < case.target.size
        lc.check_forward(case, outs[0], outs[1], verbose=False)
        lc.check_grads(case, grads, grad_loss=float(data.go[0]), want=(True,) * 3)


def _cases():
    cs = [Sga(shape, save) for shape in ((1, 2, 9, 4, 16), (1, 2, 9, 5, 7)) for save in ("", "recompute")]
    cs += _lga_cases()
    cs += [CostVolume("costvolume"), DispReg("dispreg"), L1Norm(4, 5), L1Norm(1, 5), NormReg("normreg"), Softmin("softmin"),
           SoftminReg("softminreg"), Trilinear("trilinear-x2"), LgaRegress((1, 8, 3, 36), 2), LgaRegress((1, 8, 2, 36), 3)]
    cs += [Residual(scaled, inplace) for scaled in (True, False) for inplace in (False, True)]
    cs.append(Loss("disparityloss-ganet_deep"))
    assert len({c.id for c in cs}) == len(cs)
    return cs


CASES = _cases()
