"""The cases of DispConv's kernels (ganet_amd/csrc/disp_conv_kernels.h: ganet_disp_conv_forward / _backward_data / _backward_weight),
shared by tests/test_sim_disp_conv.py (emulator build, numpy buffers behind guard pages) and tests/test_gpu_disp_conv.py (gfx950
build, device buffers).  A case takes the C ABI (`api`) and a device object with to / empty / host / ptr / sync / stream; every
output and the workspace start out as NaN (dev.empty), nothing is zero-filled.

Reference and bars: tests/disp_conv_ref64.py -- the float64 statement, and per element TWICE its first-order rounding bound
(`check` returns, per compared quantity, the worst |got - want| / bar).  Compared: y, grad_x, grad_weight.  Kinds:
  "general"  seeded randn inputs, the bars;
  "exact"    EQUALITY with the float64 statement on all three: x in multiples of 1/16 within +-2, weights in multiples of 1/8
             within +-1, grad_y in multiples of 1/8 within +-2 -- every product is a multiple of 2^-7 and every partial sum fits
             24 bits under any summation order (|y| <= 27 C 2, |gw| <= 4 N D H W: `premises` checks both).
Every shape runs in both kinds.  The shapes (an id names what it reaches; tests/test_sim_disp_conv.py asserts that it does).
A lane owns 4 consecutive w, a wave 64 such groups of the flattened (h, w / 4) plane, a workgroup's four waves split the
channels and march 8 planes; the weight gradient takes 4 channels per pass and writes one workspace row per workgroup:
  C1, C3, C32, C64   one wave with work and three without; a channel block that is not full; the model's count on the issue's
                     own [2,32,3,5,70]; four passes per wave
  D1, D2, H1, W1, one  single-element axes: both neighbours are padding
  Wsmall             W = 7: below one wave, no multiple of 4 (the last group is cut)
  W70, W130          no multiple of 4, and more than one workgroup along the plane (90 resp. 198 groups of 64 per block): a wave
                     runs over row ends
  W4                 16-byte form with a single group per row: no halo word on either side
  Hblocks            H carries the plane across a workgroup: 20 rows x 4 groups = 80 groups
  D9, D17            depth across the march of 8: two chunks (8 + 1) and three (8 + 8 + 1)
  N2                 batch strides
  aligned, offset    [2,4,9,5,68], W % 4 == 0: every base 16-byte aligned (the 16-byte kernels), and the same case with every
                     base 4 bytes into its buffer (the 4-byte kernels on data that would allow the others)
  row1, rows         the weight gradient's partial rows: exactly one workgroup (C1), resp. several
No grid is capped (sizes beyond the grid are refused), so there is no grid-stride case."""
import numpy as np

import disp_conv_ref64 as ref

F32 = np.float32
QUANTITIES = ("y", "grad_x", "grad_weight")
GROUPS_PER_BLOCK = 64


def _rng(*key):
    return np.random.default_rng([int(v) for v in key])


def _dyadic(rng, shape, bound, den):
    return (rng.integers(-bound * den, bound * den + 1, shape) / float(den)).astype(F32)


class Case:
    def __init__(self, name, shape, kind="general", offset=0):
        self.name, self.shape, self.kind, self.offset = name, tuple(shape), kind, offset
        self.id = f"{name}-{'x'.join(str(v) for v in shape)}-{kind}"
        self._made = None

    def __repr__(self):
        return self.id

    # what the kernels make of the shape (disp_conv_kernels.h)
    groups = property(lambda self: self.shape[3] * -(-self.shape[4] // ref.PX))
    blocks = property(lambda self: -(-self.groups // GROUPS_PER_BLOCK))
    chunks = property(lambda self: -(-self.shape[2] // ref.DEPTH))
    rows = property(lambda self: self.shape[0] * self.chunks * self.blocks)

    def _make(self):
        N, C, D, H, W = self.shape
        rng = _rng(13, *self.shape, self.kind == "exact")
        if self.kind == "general":
            x = rng.standard_normal(self.shape).astype(F32)
            w = (rng.standard_normal((1, C, 3, 3, 3)) / np.sqrt(27.0 * C)).astype(F32)
            g = rng.standard_normal((N, D, H, W)).astype(F32)
        else:
            x, w, g = _dyadic(rng, self.shape, 2, 16), _dyadic(rng, (1, C, 3, 3, 3), 1, 8), _dyadic(rng, (N, D, H, W), 2, 8)
        return x, w, g, ref.Statement(x, w, g)

    @property
    def made(self):
        """(x, weight, grad_y, Statement): computed once, shared by every test, never written"""
        if self._made is None:
            self._made = self._make()
            for a in self._made[:3]:
                a.setflags(write=False)
        return self._made

    x = property(lambda self: self.made[0])
    weight = property(lambda self: self.made[1])
    grad_y = property(lambda self: self.made[2])
    ref = property(lambda self: self.made[3])


class _Buf:
    """a flat device buffer whose tensor starts `off` floats in"""
    def __init__(self, dev, shape, off, init=None):
        self.shape, self.off = tuple(shape), off
        n = int(np.prod(shape))
        if init is None:
            self.buf = dev.empty((n + off,))
        else:
            self.buf = dev.to(np.concatenate([np.zeros(off, F32), np.asarray(init, F32).ravel()]))
        self.ptr = dev.ptr(self.buf) + 4 * off

    def host(self, dev):
        return np.array(dev.host(self.buf))[self.off:].reshape(self.shape)

    def front(self, dev):
        return np.array(dev.host(self.buf))[:self.off]


def run(api, dev, case):
    """the three entries through the C ABI, with the workspace sized by ganet_disp_conv_workspace"""
    N, C, D, H, W = case.shape
    off = case.offset
    x, w, g = _Buf(dev, case.shape, off, case.x), _Buf(dev, (1, C, 3, 3, 3), off, case.weight), _Buf(dev, (N, D, H, W), off, case.grad_y)
    y, gx, gw = _Buf(dev, (N, 1, D, H, W), off), _Buf(dev, case.shape, off), _Buf(dev, (1, C, 3, 3, 3), off)
    n_ws = api.query("ganet_disp_conv_workspace", *case.shape)
    assert n_ws == case.rows * 27 * C, (n_ws, case.rows)
    ws = _Buf(dev, (case.rows, 27 * C), off)
    for b in (x, g, y, gx):
        assert b.ptr % 16 == (4 * off) % 16, "the case's alignment"
    api.call("ganet_disp_conv_forward", x.ptr, w.ptr, y.ptr, *case.shape, dev.stream)
    api.call("ganet_disp_conv_backward_data", g.ptr, w.ptr, gx.ptr, *case.shape, dev.stream)
    api.call("ganet_disp_conv_backward_weight", x.ptr, g.ptr, ws.ptr, gw.ptr, *case.shape, dev.stream)
    dev.sync()
    for b, a in ((x, case.x), (w, case.weight), (g, case.grad_y)):
        assert np.array_equal(b.host(dev), a) and not b.front(dev).any(), "inputs written"
    for b in (y, gx, gw, ws):
        assert np.isnan(b.front(dev)).all(), "written in front of an output"
    rows = ws.host(dev)
    assert np.isfinite(rows).all(), "a workspace element was left unwritten"
    return {"y": y.host(dev).reshape(N, D, H, W), "grad_x": gx.host(dev), "grad_weight": gw.host(dev).reshape(C, 3, 3, 3)}


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
    for q in quantities:
        if case.kind == "exact":
            bad = ~(np.asarray(got[q]).astype(np.float64) == want[q])
            assert not bad.any(), (case.id, q, f"{int(bad.sum())} of {bad.size} elements differ from the float64 statement")
        else:
            assert res[q] <= limit, (case.id, q, res[q])
    return res


def premises(case):
    """the exact family's: grids, ranges, and every partial sum within 24 bits under any order"""
    assert case.kind == "exact"
    N, C, D, H, W = case.shape
    for a, den, bound in ((case.x, 16, 2), (case.weight, 8, 1), (case.grad_y, 8, 2)):
        assert np.array_equal(a * den, np.round(a * den)) and np.abs(a).max() <= bound
    # sums of multiples of 2^-7: |partial sum| * 2^7 <= (number of terms) * (largest product) * 2^7 < 2^24
    assert 27 * C * 2 * 128 < 2 ** 24 and N * D * H * W * 4 * 128 < 2 ** 24
    for a in case.ref.results().values():
        assert np.array_equal(a.astype(F32).astype(np.float64), a)


SHAPES = [("C1-row1", (1, 1, 3, 4, 9)),
          ("C3", (1, 3, 3, 4, 9)),
          ("C32-W70-N2-rows", (2, 32, 3, 5, 70)),
          ("C64", (1, 64, 2, 3, 8)),
          ("W130-N2", (2, 5, 4, 6, 130)),
          ("D1", (1, 2, 1, 4, 6)),
          ("D2", (1, 2, 2, 4, 6)),
          ("H1", (1, 2, 3, 1, 9)),
          ("W1", (1, 2, 3, 4, 1)),
          ("one", (1, 1, 1, 1, 1)),
          ("Wsmall", (1, 2, 2, 3, 7)),
          ("W4", (1, 2, 2, 3, 4)),
          ("Hblocks", (1, 2, 2, 20, 13)),
          ("D9", (1, 2, 9, 3, 8)),
          ("D17", (1, 1, 17, 2, 5)),
          ("N2", (2, 3, 2, 3, 5)),
          ("aligned", (2, 4, 9, 5, 68)),
          ("offset", (2, 4, 9, 5, 68))]


def _cases():
    cs = []
    for name, shape in SHAPES:
        for kind in ("general", "exact"):
            cs.append(Case(name, shape, kind, offset=1 if name == "offset" else 0))
    return cs


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def by_name(name, kind="general"):
    return next(c for c in CASES if c.name == name and c.kind == kind)


ENTRIES = (("ganet_disp_conv_forward", 3), ("ganet_disp_conv_backward_data", 3), ("ganet_disp_conv_backward_weight", 4))


BEYOND_WORKSPACE = (1, 64, 1024, 2048, 2048)         # inside the launch grid; rows * 27 * C = 2^21 * 1728 > 2^31 - 1


def check_bad_arguments(api, dev):
    """the neighbouring entries' checks, plus C <= 64; a refused call launches nothing"""
    from ganet_amd._native import E_INVALID, E_UNSUPPORTED, GanetError
    bufs = [dev.empty((27 * 65,)) for _ in range(4)]
    p = [dev.ptr(b) for b in bufs]
    good = (1, 1, 1, 1, 1)

    def refused(text, code, name, *args):
        try:
            (api.query if name.endswith("workspace") else api.call)(name, *args)
        except GanetError as e:
            assert text in str(e) and e.code == code, (name, args, str(e))
            # the library's own message names the entry that was called (the launchers behind the fp32 and the _16 entries are shared)
            assert str(e).startswith(f"{name} failed ({code}): {name}: "), (name, str(e))
        else:
            raise AssertionError((name, args))

    for k in range(5):
        for bad in (0, -1):
            dims = good[:k] + (bad,) + good[k + 1:]
            refused("non-positive", E_INVALID, "ganet_disp_conv_workspace", *dims)
            for name, n in ENTRIES:
                refused("non-positive", E_INVALID, name, *p[:n], *dims, dev.stream)
    for name, n in ENTRIES:
        for k in range(n):
            ptrs = list(p[:n])
            ptrs[k] = None
            refused("null pointer", E_INVALID, name, *ptrs, *good, dev.stream)
        refused("at most 64", E_UNSUPPORTED, name, *p[:n], 1, 65, 1, 1, 1, dev.stream)
        refused("alias", E_INVALID, name, *([p[0]] * n), *good, dev.stream)
        refused("beyond the launch grid", E_UNSUPPORTED, name, *p[:n], 65536, 1, 1, 1, 1, dev.stream)
    # 16384 x 128 blocks = 2^21 workspace rows of 27 * 64 floats: past what ganet_disp_conv_workspace can answer, refused before any launch
    refused("workspace is beyond ganet_disp_conv_workspace's answer", E_UNSUPPORTED, "ganet_disp_conv_backward_weight", *p[:4], *BEYOND_WORKSPACE, dev.stream)
    refused("do not fit the answer", E_UNSUPPORTED, "ganet_disp_conv_workspace", *BEYOND_WORKSPACE)
    refused("beyond the launch grid", E_UNSUPPORTED, "ganet_disp_conv_workspace", 65536, 1, 1, 1, 1)
    refused("at most 64", E_UNSUPPORTED, "ganet_disp_conv_workspace", 1, 65, 1, 1, 1)
    assert api.query("ganet_disp_conv_workspace", 1, 64, 1, 1, 1) == 27 * 64
    dev.sync()
    for b in bufs:
        assert np.isnan(np.asarray(dev.host(b))).all()
