"""TEST INFRASTRUCTURE: the case table of the fused criterion (ganet_disparity_loss_workspace / _forward / _backward),
shared by tests/test_sim_loss.py (emulator build, guard pages) and tests/test_gpu_loss.py (gfx950 build, C ABI and module).
`run(api, dev, case)` drives the C ABI on either build; `check(case, got)` compares with tests/loss_ref64.py.

Bars (none of them taken from what the kernels return):
  sums (loss, mean rho, EPE)  relative 2^-18 against the float64 yardstick: at most 5 individually rounded fp32 operations
                              per term, amplified at most 2 far / knee <= 6 on the mixes used here, all terms non-negative
                              so the per-term bound carries over to the sum: 5 * 6 * 2^-24 = 1.8e-6, doubled for the final
                              rounding; the fp64 accumulation adds nothing visible.  `exact` cases: equality.
  count, error rate           stats[0] == count; rate == fl32(n / count), the one rounding of an exact quotient, which puts
                              rate * count within n * 2^-24 < 1/2 of the integer n
  gradients                   bit-equal to the float32 statement (sign of zero included; a NaN wherever that has one), and
                              within relative 2^-20 of the float64 statement
Both relative bars get the spacing of the fp32 subnormals, 2^-149, added: |r| = 2^-140 is in the table and its terms live
on that grid."""
import itertools

import numpy as np

import loss_ref64 as ref

F32 = np.float32
BLOCK, GRID_CAP = 256, 64          # ganet_amd/csrc/loss_kernels.h: LOSS_BLOCK, LOSS_MAX_BLOCKS
STRIDE = BLOCK * GRID_CAP          # lanes of one trip of the grid-stride loop
SUM_RTOL, GRAD_RTOL, TINY = 2.0 ** -18, 2.0 ** -20, 2.0 ** -149
HI, LO = 48.0, 0.001
DEEP, G11 = (0.2, 0.6, 1.0), (0.4, 1.2)


def ulp_step(x, k):
    """the fp32 value k steps of the fp32 grid away from x"""
    x = F32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, F32(np.inf if k > 0 else -np.inf))
    return x


class Case:
    def __init__(self, name, shape, preds, target, kinds, weights, thresh=3, alpha=2, mask_mode=0, offset=0, grad_loss=1.0,
                 want=None, exact=False, hi=HI, lo=LO, rate=3.0):
        self.name, self.shape, self.kinds, self.mask_mode, self.offset = name, tuple(shape), tuple(kinds), mask_mode, offset
        self.preds = [np.ascontiguousarray(p, F32).reshape(self.shape) for p in preds]
        self.target = np.ascontiguousarray(target, F32).reshape(self.shape)
        w = list(weights) + [0.0] * (3 - len(weights))
        self.params = dict(hi=hi, lo=lo, w0=w[0], w1=w[1], w2=w[2], thresh=thresh, alpha=alpha, rate=rate)
        self.grad_loss, self.exact = grad_loss, exact
        self.want = tuple(want) if want is not None else (True,) * len(preds)
        self._ref = None

    def __repr__(self):
        return self.name

    @property
    def ref(self):
        """computed once, shared by every test that runs the case"""
        if self._ref is None:
            self._ref = ref.Reference(self.preds, self.target, self.params, self.kinds, self.mask_mode)
        return self._ref

    def param_array(self):
        return np.asarray([self.params[k] for k in ref.PARAMS], F32)


def random_maps(seed, shape, P, sigma=3.0, hi=HI):
    """targets over [0, 1.2 hi) -- about one in six invalid -- with some exact zeros (below `lo`); residuals that reach
    every branch of both losses for (thresh, alpha) = (1, 2) and (3, 2)"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    t = rng.uniform(0, 1.2 * hi, n).astype(F32)
    t[::7] = 0.0
    t[-1] = 1.0                                    # the last element counts: a lane that never came round shows
    preds = [(t + rng.normal(0, sigma, n).astype(F32)).astype(F32) for _ in range(P)]
    return preds, t


def _random(name, shape, kinds, weights, seed, **kw):
    preds, t = random_maps(seed, shape, len(kinds))
    return Case(name, shape, preds, t, kinds, weights, **kw)


def boundary_residuals(thresh, alpha):
    knee, far = F32(thresh), F32(thresh) + F32(alpha)
    vs = [F32(0), F32(2.0 ** -140), F32(100)]
    for x in (knee, far, F32(1)):
        vs += [ulp_step(x, -1), x, ulp_step(x, +1)]
    return np.asarray([s * v for v in vs for s in (F32(1), F32(-1))], F32)


# the five values the issue states, float64 from the sequential chain: (thresh, alpha, v, value, slope)
SPOTS = [(1, 2, 2.9, 4.8975, 1.05), (1, 2, 4.0, 5.0, 2.0), (3, 2, 3.0, 3.0, 4.0 / 3.0), (3, 2, 4.9, 6.8975, 0.7), (3, 2, 5.1, 6.1, 2.0 / 3.0)]

# targets around both limits of the mask, and the ones no comparison accepts
EDGE_TARGETS = [ulp_step(HI, -1), F32(HI), ulp_step(LO, -1), F32(LO), F32(-2.5), F32(np.inf), F32(np.nan)]
EDGE_VALID = {0: [True, False, True, True, True, False, False], 1: [True, True, False, True, False, False, False]}


def _cases():
    cs = []
    # shapes: one pixel, around one block, N = 2, HW % 4 != 0 (scalar twin), 4-byte offset (scalar twin on a vector size),
    # more than one block of partials and the second trip of the grid-stride loop -- for both twins
    shapes = [("1", (1, 1, 1)), ("255", (1, 15, 17)), ("256", (1, 16, 16)), ("257", (1, 1, 257)), ("n2-scalar", (2, 3, 5)),
              ("n2-vec", (2, 4, 6)), ("vec-2blocks", (1, 4, BLOCK + 1)), ("scalar-stride2", (1, 1, STRIDE + 1)),
              ("vec-stride2", (1, 4, STRIDE + 1))]
    for i, (tag, shape) in enumerate(shapes):
        cs.append(_random(f"shape-{tag}", shape, (0, 0, 1), DEEP, 100 + i))
    cs.append(_random("shape-256-offset1", (1, 16, 16), (0, 0, 1), DEEP, 120, offset=1))
    cs.append(_random("shape-n2-vec-offset1", (2, 4, 6), (0, 1), G11, 121, offset=1))
    # P, kinds, mask modes, MyLoss2 parameters
    cs.append(_random("p1-sl1", (1, 9, 13), (0,), (1.0,), 130))
    cs.append(_random("p1-myloss2-eval", (1, 8, 12), (1,), (1.0,), 131, mask_mode=1))
    for j, kinds in enumerate(itertools.product((0, 1), repeat=2)):
        cs.append(_random(f"p2-kinds{kinds[0]}{kinds[1]}", (1, 10, 14), kinds, G11, 140 + j, thresh=1, alpha=2, mask_mode=j % 2))
    cs.append(_random("p3-eval-t1a2", (2, 7, 9), (1, 0, 1), DEEP, 150, thresh=1, alpha=2, mask_mode=1, grad_loss=-0.37))
    cs.append(_random("p3-wanted-101", (1, 12, 16), (0, 0, 1), DEEP, 151, want=(True, False, True), grad_loss=2.5))
    cs.append(_random("p3-wanted-010-offset1", (1, 5, 7), (0, 1, 1), DEEP, 152, want=(False, True, False), offset=1))
    # boundaries of every branch, both signs, target 0 so that fl32(p - t) IS the residual
    for thresh, alpha in ((1, 2), (3, 2)):
        r = boundary_residuals(thresh, alpha)
        cs.append(Case(f"boundary-t{thresh}a{alpha}", (1, 1, r.size), [r, r], np.zeros_like(r), (0, 1), (0.5, 1.0), thresh, alpha))
    for thresh, alpha, v, _, _ in SPOTS:
        cs.append(Case(f"spot-t{thresh}a{alpha}-v{v}", (1, 1, 1), [[v]], [0.0], (1,), (1.0,), thresh, alpha))
    for mode in (0, 1):
        t = np.asarray(EDGE_TARGETS, F32)
        p = np.asarray([40.0, 47.0, 1.5, 0.25, -1.0, 3.0, 2.0], F32)
        cs.append(Case(f"targets-mode{mode}", (1, 1, t.size), [p, p + F32(2)], t, (0, 1), G11, mask_mode=mode))
    # a NaN prediction at a VALID pixel propagates, as in torch
    preds, t = random_maps(160, (1, 4, 8), 2)
    t[5], preds[1][5] = 2.0, np.nan
    cs.append(Case("nan-at-valid", (1, 4, 8), preds, t, (0, 1), G11))
    # no valid pixel: everything zero, whatever the predictions hold
    preds, t = random_maps(161, (1, 6, 10), 3)
    preds[0][3], preds[2][7] = np.nan, np.inf
    for tag, off in (("", 0), ("-offset1", 1)):
        cs.append(Case("all-invalid" + tag, (1, 6, 10), preds, np.full_like(t, HI), (0, 0, 1), DEEP, offset=off))
    cs.append(Case("all-invalid-eval-nan-targets", (1, 6, 10), preds, np.full_like(t, np.nan), (0, 0, 1), DEEP, mask_mode=1))
    # exact: smooth-L1 only, residuals k / 8 with |r| <= 4, targets on the same grid, power-of-two count and weights: every
    # term, every sum and every quotient is representable, so loss and stats EQUAL the yardstick
    for tag, shape, off in (("256", (1, 16, 16), 0), ("256-offset1", (1, 16, 16), 1), ("2048", (2, 32, 32), 0)):
        rng = np.random.default_rng(170)
        n = int(np.prod(shape))
        t = (rng.integers(0, 8 * 40, n) / 8.0).astype(F32)
        preds = [(t + (rng.integers(-32, 33, n) / 8.0).astype(F32)).astype(F32) for _ in range(3)]
        cs.append(Case("exact-" + tag, shape, preds, t, (0, 0, 0), (0.5, 1.0, 2.0), exact=True, rate=1.0))
    return cs


CASES = _cases()


def poison_pair(seed=180, shape=(2, 6, 10), offset=0):
    """(clean, poisoned): the same maps, the poisoned ones with NaN / +inf / -inf predictions at EVERY invalid pixel"""
    preds, t = random_maps(seed, shape, 3)
    t[4] = np.nan
    bad = ~ref.valid(t, HI, LO, 0)
    vals = np.resize(np.asarray([np.nan, np.inf, -np.inf], F32), int(bad.sum()))
    dirty = []
    for k, p in enumerate(preds):
        q = p.copy()
        q[bad] = np.roll(vals, k)
        dirty.append(q)
    mk = lambda name, ps: Case(name, shape, ps, t, (0, 1, 1), DEEP, offset=offset)   # noqa: E731
    return mk("poison-clean", preds), mk("poison-dirty", dirty)


# ---- running a case through the C ABI on either build ---------------------------------------------------------------------

def run(api, dev, case, want=None):
    """forward + backward through the C ABI.  dev: parity_cases.NumpyDev (emulator) or test_gpu_parity.TorchDev.
    Outputs are poisoned first, so an element that is not written shows.  offset: every map starts 4 bytes behind a
    16-byte boundary."""
    want = case.want if want is None else want
    N, H, W = case.shape
    n, P, off = N * H * W, len(case.preds), case.offset
    keep = []

    def put(a):
        buf = dev.to(np.concatenate([np.full(off, 7.0, F32), np.asarray(a, F32).ravel()]))
        keep.append(buf)
        return dev.ptr(buf) + 4 * off

    pp = [put(p) for p in case.preds] + [None] * (3 - P)
    tp = put(case.target)
    params = dev.to(case.param_array())
    nws = api.query("ganet_disparity_loss_workspace", N, H, W)
    ws = dev.empty((2 * nws,), np.float32)             # fp64 scratch, NaN bit patterns all over
    loss, stats = dev.empty((1,)), dev.empty((1 + 3 * P,))
    kinds = list(case.kinds) + [0] * (3 - P)
    api.call("ganet_disparity_loss_forward", *pp, tp, dev.ptr(params), dev.ptr(ws), dev.ptr(loss), dev.ptr(stats),
             N, H, W, P, *kinds, case.mask_mode, dev.stream)
    gl = dev.to(np.asarray([case.grad_loss], F32))
    gbuf = [dev.empty((off + n,)) if w else None for w in want] + [None] * (3 - P)
    gp = [dev.ptr(g) + 4 * off if g is not None else None for g in gbuf]
    api.call("ganet_disparity_loss_backward", *pp, tp, dev.ptr(params), dev.ptr(stats), dev.ptr(gl), *gp,
             N, H, W, P, *kinds, case.mask_mode, dev.stream)
    dev.sync()
    grads = [np.array(dev.host(g))[off:].reshape(case.shape) if g is not None else None for g in gbuf[:P]]
    return {"loss": np.array(dev.host(loss))[0], "stats": np.array(dev.host(stats)), "grads": grads}


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def close(got, want, rtol):
    return abs(float(got) - float(want)) <= rtol * abs(float(want)) + TINY


def check_forward(case, loss, stats, verbose=True):
    r, P = case.ref, len(case.preds)
    assert stats.shape == (1 + 3 * P,)
    assert stats[0] == r.count, (stats[0], r.count)
    if r.count == 0:
        assert bits(loss) == 0 and not bits(stats).any(), "no valid pixel: loss and stats are +0"
        return
    for k in range(P):
        assert stats[3 + 3 * k] == r.rate[k], (k, stats[3 + 3 * k], r.rate[k])
        assert abs(float(stats[3 + 3 * k]) * r.count - r.nrate[k]) < 0.5
    pairs = [("loss", loss, r.loss)] + [(f"mean_rho{k}", stats[1 + 3 * k], r.mean_rho[k]) for k in range(P)] + \
            [(f"epe{k}", stats[2 + 3 * k], r.epe[k]) for k in range(P)]
    for what, got, want in pairs:
        if np.isnan(want):
            assert np.isnan(got), what
            continue
        if verbose and want:
            print(f"{case.name} {what}: got {float(got)!r} want {want!r} rel {abs(float(got) - want) / abs(want):.3e}")
        if case.exact:
            assert float(got) == want, (what, float(got), want)
        else:
            assert close(got, want, SUM_RTOL), (what, float(got), want)


def check_grads(case, grads, grad_loss=None, want=None):
    r = case.ref
    want = case.want if want is None else want
    gl = case.grad_loss if grad_loss is None else grad_loss
    g32, g64 = r.grads(gl, np.float32), r.grads(gl, np.float64)
    for k, g in enumerate(grads):
        if not want[k]:
            assert g is None
            continue
        nan = np.isnan(g32[k])
        assert np.array_equal(np.isnan(g), nan), f"map {k}: NaNs elsewhere than the float32 statement has them"
        same = bits(g)[~nan] == bits(g32[k])[~nan]
        assert same.all(), f"map {k}: {int((~same).sum())} of {g.size} elements differ from the float32 statement"
        err = np.abs(g.astype(np.float64) - g64[k])[~nan]
        assert (err <= GRAD_RTOL * np.abs(g64[k][~nan]) + TINY).all(), f"map {k}: off the float64 statement"
        assert not bits(g)[~r.ok].any(), f"map {k}: an invalid pixel's gradient is not +0"


def check(case, got):
    check_forward(case, got["loss"], got["stats"])
    check_grads(case, got["grads"])
