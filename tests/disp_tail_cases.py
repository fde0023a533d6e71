"""The cases of DispTail's kernels (ganet_amd/csrc/disp_tail_kernels.h: ganet_up_softmin_regression_forward / _backward), shared
by tests/test_sim_disp_tail.py (emulator build, numpy buffers behind guard pages) and tests/test_gpu_disp_tail.py (gfx950
build, device buffers).  A case takes the C ABI (`api`) and a device object with to / empty / host / ptr / sync / stream; every
output and the workspace start out as NaN (dev.empty), nothing is zero-filled.

Reference and bars: tests/disp_tail_ref64.py -- the float64 statement, and per element TWICE its first-order rounding bound
(`check` returns, per compared quantity, the worst |got - want| / bar).  Compared: out, mx, ssum, the column workspace gc
[N,Di,Ho,Wo] -- every plane of it -- and grad_x.  Kinds:
  "general"  the bars;
  "exact"    EQUALITY with the float64 statement on all five: zoom 2 and 4 in every axis (scale, src and l in {1/8 .. 7/8}
             are exact under any contraction), x dyadic and constant along d, Do in {8, 16}, dyadic grad_out -- then v is the
             same dyadic number at every od, mx = -v, ssum = Do, out = (Do - 1) / 2, and every product and sum of the
             adjoint is exact;
  "dyadic"   the same zooms on dyadic x that VARIES along d: v is exact, so mx must EQUAL the statement's; the rest by the bars.
The families (an id names what it reaches):
  model      [2,5,4,6] -> (13,12,18): the 3x zoom with Di = Do // 3 + 1
  depth65    the model's own depth axis, 65 -> 193, on a tiny image: lambda's ulp is 2^-18 at the far end, and at od = 96 src is
             32 but for its rounding, so a contracted and an uncontracted build read different plane pairs there
  Do<n>      depth against the chunk of 8: Do = 1, 7, 8, 9, 17
  Di1, HiWi1 a single input plane; a single input row and column
  DieqDo     no zoom along d
  down-skip  [1,9,3,3] -> (4,7,5): d0 jumps by more than one, planes between are never read and must come out +0
  down-tail  [1,12,2,2] -> (2,4,4): planes in front of the first d0 and behind the last d1
  slowloop   a W footprint of 12 outputs or more (stage 2's slow loop)
  stride2    one more pixel than one launch holds (the grid-stride loop's second trip), Do = 2, Di = 1
  fall, rise x falls resp. rises along d from +60 to -60: the running max rises up to the last plane and early terms
             underflow, resp. the first chunk holds it and every later term is rescaled against it
No 16-byte form exists in these kernels, so there is no 4-byte-offset family."""
import numpy as np

import disp_tail_ref64 as ref

F32 = np.float32
MAX_LANES = 4096 * 256            # ew_grid() in ganet_capi.hip: blocks are capped, the kernels loop
QUANTITIES = ("out", "mx", "ssum", "gc", "grad_x")


def _rng(*key):
    return np.random.default_rng([int(v) for v in key])


def _dyadic(rng, shape, lo=-64, hi=64, den=16.0):
    return (rng.integers(lo, hi + 1, shape) / den).astype(F32)


class Case:
    def __init__(self, id, shape, size, kind="general", fill="normal", model=True):
        self.id, self.shape, self.size, self.kind, self.fill, self.model = id, tuple(shape), tuple(size), kind, fill, model
        self._made = None

    def __repr__(self):
        return self.id

    def _make(self):
        N, Di, Hi, Wi = self.shape
        Do, Ho, Wo = self.size
        rng = _rng(12, *self.shape, *self.size)
        if self.fill == "normal":
            x = rng.standard_normal(self.shape).astype(F32)
            g = rng.standard_normal((N, Ho, Wo)).astype(F32)
        elif self.fill in ("fall", "rise"):
            ramp = np.linspace(60.0, -60.0, Di) if self.fill == "fall" else np.linspace(-60.0, 60.0, Di)
            x = (ramp[None, :, None, None] + 0.25 * rng.standard_normal(self.shape)).astype(F32)
            g = rng.standard_normal((N, Ho, Wo)).astype(F32)
        elif self.fill == "dyadic-const-d":
            x = np.broadcast_to(_dyadic(rng, (N, 1, Hi, Wi)), self.shape).copy()
            # multiples of 1/4 up to 2: gv is a multiple of 2^-7 below 1, the weights are multiples of 2^-3 per axis and a plane
            # has at most 4 readers per axis, so every partial sum of gc and grad_x fits 22 bits
            g = _dyadic(rng, (N, Ho, Wo), -8, 8, 4.0)
        else:
            assert self.fill == "dyadic"
            x = _dyadic(rng, self.shape)
            g = _dyadic(rng, (N, Ho, Wo))
        return x, g, ref.Statement(x, self.size, g)

    @property
    def made(self):
        """(x, grad_out, Statement): computed once, shared by every test, never written"""
        if self._made is None:
            self._made = self._make()
            for a in self._made[:2]:
                a.setflags(write=False)
        return self._made

    x = property(lambda self: self.made[0])
    grad_out = property(lambda self: self.made[1])
    ref = property(lambda self: self.made[2])


def run(api, dev, case):
    """both entries through the C ABI; the backward reads the forward's own out / mx / ssum, as the autograd Function does"""
    N, Di, Hi, Wi = case.shape
    Do, Ho, Wo = case.size
    x, g = dev.to(np.array(case.x)), dev.to(np.array(case.grad_out))            # (copies: the shared arrays are read-only)
    out, mx, ss = dev.empty((N, Ho, Wo)), dev.empty((N, Ho, Wo)), dev.empty((N, Ho, Wo))
    ws, gx = dev.empty((N, Di, Ho, Wo)), dev.empty(case.shape)
    dims = (N, Di, Hi, Wi, Do, Ho, Wo)
    api.call("ganet_up_softmin_regression_forward", dev.ptr(x), dev.ptr(out), dev.ptr(mx), dev.ptr(ss), *dims, dev.stream)
    api.call("ganet_up_softmin_regression_backward", dev.ptr(x), dev.ptr(out), dev.ptr(mx), dev.ptr(ss), dev.ptr(g), dev.ptr(ws),
             dev.ptr(gx), *dims, dev.stream)
    dev.sync()
    assert np.array_equal(np.asarray(dev.host(x)), case.x) and np.array_equal(np.asarray(dev.host(g)), case.grad_out), "inputs written"
    return {"out": np.array(dev.host(out)), "mx": np.array(dev.host(mx)), "ssum": np.array(dev.host(ss)),
            "gc": np.array(dev.host(ws)), "grad_x": np.array(dev.host(gx))}


def ratios(case, got, quantities=QUANTITIES):
    """per quantity: the worst |got - want| / (2 x bound); inf where got is not finite or misses a zero bar"""
    want, bound = case.ref.results(), case.ref.bounds()
    res = {}
    for q in quantities:
        g = np.asarray(got[q])
        assert g.dtype == F32 and g.shape == want[q].shape, (q, g.dtype, g.shape, want[q].shape)
        err, bar = np.abs(g.astype(np.float64) - want[q]), 2 * bound[q]
        with np.errstate(all="ignore"):
            r = np.where(err == 0, 0.0, err / bar)
        r = np.where(np.isfinite(g), r, np.inf)
        res[q] = float(r.max())
    return res


def check(case, got, quantities=QUANTITIES, verbose=True, limit=1.0):
    res = ratios(case, got, quantities)
    if verbose:
        print(f"{case.id}: worst error / bar  " + "  ".join(f"{q} {res[q]:.3f}" for q in res))
    want = case.ref.results()
    equal = quantities if case.kind == "exact" else ("mx",) if case.kind == "dyadic" else ()
    for q in quantities:
        if q in equal:
            bad = ~(np.asarray(got[q]).astype(np.float64) == want[q])
            assert not bad.any(), (case.id, q, f"{int(bad.sum())} of {bad.size} elements differ from the float64 statement")
        else:
            assert res[q] <= limit, (case.id, q, res[q])
    if case.kind == "exact":
        Do = case.size[0]
        assert np.all(got["ssum"] == Do) and np.all(got["out"] == (Do - 1) / 2.0)
    return res


def _cases():
    cs = [Case("model-2x5x4x6-to-13x12x18", (2, 5, 4, 6), (13, 12, 18)),
          Case("depth65-1x65x2x3-to-193x6x9", (1, 65, 2, 3), (193, 6, 9))]
    for Do in (1, 7, 8, 9, 17):
        cs.append(Case(f"Do{Do}-1x{Do // 3 + 1}x3x4-to-{Do}x7x9", (1, Do // 3 + 1, 3, 4), (Do, 7, 9)))
    cs += [Case("Di1-1x1x3x4-to-5x6x8", (1, 1, 3, 4), (5, 6, 8)),
           Case("HiWi1-2x4x1x1-to-10x3x3", (2, 4, 1, 1), (10, 3, 3)),
           Case("DieqDo-1x6x2x3-to-6x5x7", (1, 6, 2, 3), (6, 5, 7)),
           Case("down-skip-1x9x3x3-to-4x7x5", (1, 9, 3, 3), (4, 7, 5)),
           Case("down-tail-1x12x2x2-to-2x4x4", (1, 12, 2, 2), (2, 4, 4)),
           Case("slowloop-1x3x2x2-to-7x5x29", (1, 3, 2, 2), (7, 5, 29)),
           Case("stride2-1x1x6x20561-to-2x17x61681", (1, 1, 6, 20561), (2, 17, 61681)),
           Case("fall-1x7x2x3-to-19x5x7", (1, 7, 2, 3), (19, 5, 7), fill="fall"),
           Case("rise-1x7x2x3-to-19x5x7", (1, 7, 2, 3), (19, 5, 7), fill="rise")]
    for zoom in (2, 4):
        for Do in (8, 16):
            cs.append(Case(f"exact-zoom{zoom}-Do{Do}", (2, Do // zoom, 3, 5), (Do, 3 * zoom, 5 * zoom), kind="exact", fill="dyadic-const-d"))
        cs.append(Case(f"dyadic-zoom{zoom}", (1, 5, 3, 4), (5 * zoom, 3 * zoom, 4 * zoom), kind="dyadic", fill="dyadic"))
    return cs


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def check_bad_arguments(api, dev):
    """the neighbouring entries' checks, plus Do < 2^24; a refused call launches nothing"""
    from ganet_amd._native import GanetError
    x, o = dev.to(np.zeros((1, 1, 1, 1), F32)), dev.empty((1, 1, 1))
    p = dev.ptr
    good = (1, 1, 1, 1, 1, 1, 1)
    for k in range(7):
        for bad in (0, -1):
            dims = good[:k] + (bad,) + good[k + 1:]
            for call in (("ganet_up_softmin_regression_forward", p(x), p(o), p(o), p(o)),
                         ("ganet_up_softmin_regression_backward", p(x), p(o), p(o), p(o), p(o), p(x), p(x))):
                try:
                    api.call(*call, *dims, dev.stream)
                except GanetError as e:
                    assert "non-positive" in str(e)
                else:
                    raise AssertionError(dims)
    for call, n in (("ganet_up_softmin_regression_forward", 4), ("ganet_up_softmin_regression_backward", 7)):
        for k in range(n):
            ptrs = [p(x)] * n
            ptrs[k] = None
            try:
                api.call(call, *ptrs, *good, dev.stream)
            except GanetError as e:
                assert "null pointer" in str(e)
            else:
                raise AssertionError((call, k))
        try:
            api.call(call, *([p(x)] * n), 1, 1, 1, 1, 1 << 24, 1, 1, dev.stream)
        except GanetError as e:
            assert "2^24" in str(e)
        else:
            raise AssertionError(call)
    dev.sync()
    assert np.isnan(np.asarray(dev.host(o))).all()
