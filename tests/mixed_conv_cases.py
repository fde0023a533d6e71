"""TEST INFRASTRUCTURE: the case table of conv32x1 on a 16-bit x (include/ganet_hip_conv16.h, ganet_amd/csrc/disp_conv_kernels.h on a 16-bit storage type:
ganet_disp_conv_forward_16 / _backward_data_16 / _backward_weight_16), run on the emulator behind guard pages by
tests/test_sim_mixed_conv.py and on the device by tests/test_gpu_mixed_conv.py through one `dev` (parity_cases.NumpyDev /
test_gpu_parity.TorchDev), in both 16-bit formats.

There is no tolerance anywhere.  For a 16-bit x (uint16 patterns), an fp32 weight and an fp32 grad_y:
    y_16, grad_weight_16  ==  the fp32 entry of the SAME build on up(x)                            bit for bit
    grad_x_16             ==  mixed_cases.convert(the fp32 entry's grad_x)                         bit for bit, NaN positions equal
and on the exact family additionally == the float64 statement of tests/disp_conv_ref64.py (every sum is exact there).
Value families:
  "exact"     disp_conv_cases' dyadic family: x multiples of 1/16 within +-2 (6 significant bits: both 16-bit formats hold them),
              weights multiples of 1/8 within +-1, grad_y multiples of 1/8 within +-2
  "general"   seeded randn: x rounded to the format, weight and grad_y fp32 (the weight has bits a 16-bit copy would lose)
  "rounding"  for grad_x's one rounding.  Channel 0's weight is the centre tap 1, channel 1's the centre tap -1: their grad_x is
              +-grad_y itself, exactly, and grad_y carries every tie of mixed_cases.tie_neighbours (both parities of the lower
              neighbour), values beyond the largest finite number of the format (overflow to +-inf), values in fp16's subnormal
              range, and one NaN in the far corner (it reaches only its 27 neighbours); the other channels have random weights.
              `rounding_premises` asserts what the family contains on the fp32 grad_x a run (or the statement) gives.
Shapes (a lane owns DCV_PX = 4 consecutive w, a wave 64 such groups of the flattened plane, a workgroup's four waves split the
channels and march DCV_DEPTH = 8 planes, the weight gradient takes DCV_CB = 4 channels per pass): W in {1, 3, 4, 5, 8} (twin and
VEC), H in {1, 3}, D in {1, 8, 9}, C in {1, 3, 4, 5, 33, 64}, N = 2, planes of more than 64 groups in both forms, and a 16-bit
base 2 bytes (twin on a W that would allow VEC) and 8 bytes (VEC, not 16-byte aligned) into its allocation.  Every output and the
workspace start out as NaN patterns; nothing is zero-filled."""
import numpy as np

import disp_conv_cases as dc
import disp_conv_ref64 as ref
import mixed_cases as mc

F32 = np.float32
FMTS = (mc.F16, mc.BF16)
QUANTITIES = ("y", "grad_x", "grad_weight")
ENTRIES16 = (("ganet_disp_conv_forward_16", 3), ("ganet_disp_conv_backward_data_16", 3), ("ganet_disp_conv_backward_weight_16", 4))


def _rng(*key):
    return np.random.default_rng([int(v) for v in key])


def tie_values(fmt):
    """fp32 values exactly half way between two neighbours of the format, with the pattern RNE must give"""
    h = mc.tie_neighbours(fmt)
    top = 0x7BFF if fmt == mc.F16 else 0x7F7F
    # (the overflow threshold stands on its own; bf16's subnormals are fp32's, and its largest values times a weight leave fp32:
    # neither is this family's subject)
    h = h[(h != top) & (h > 8)]
    v = mc.up(h, fmt)
    h = h[(v >= 1e-30) & (v <= 1e30)]
    lo, hi = mc.up(h, fmt).astype(np.float64), mc.up((h + 1).astype(np.uint16), fmt).astype(np.float64)
    mid = ((lo + hi) / 2).astype(F32)
    assert np.array_equal(mid.astype(np.float64), (lo + hi) / 2)
    assert (h & 1).any() and not (h & 1).all()                  # both parities of the lower neighbour
    want = np.where(h & 1, h + 1, h).astype(np.uint16)          # to even
    return mid, want


def specials(fmt):
    """the values the rounding family plants in grad_y (finite)"""
    mid, _ = tie_values(fmt)
    big = np.array([65520.0, 70000.0, 1e6] if fmt == mc.F16 else [3.4e38, 3.4028235e38, 3.39e38], F32)   # at / beyond the overflow threshold
    sub = np.array([2.0 ** -24, 3 * 2.0 ** -25, 2.0 ** -25, 5.1e-6, 6.0e-5, 2.0 ** -26], F32)            # fp16's subnormal range and below
    v = np.concatenate([mid, big, sub])
    return np.concatenate([v, -v]).astype(F32)


class Case:
    def __init__(self, name, shape, kind="general", off16=0):
        self.name, self.shape, self.kind, self.off16 = name, tuple(shape), kind, off16
        self.id = f"{name}-{'x'.join(str(v) for v in shape)}-{kind}"
        self._made = {}

    def __repr__(self):
        return self.id

    groups = property(lambda self: self.shape[3] * -(-self.shape[4] // ref.PX))
    blocks = property(lambda self: -(-self.groups // dc.GROUPS_PER_BLOCK))
    chunks = property(lambda self: -(-self.shape[2] // ref.DEPTH))
    rows = property(lambda self: self.shape[0] * self.chunks * self.blocks)
    vec = property(lambda self: self.shape[4] % 4 == 0 and (2 * self.off16) % 8 == 0)

    def _make(self, fmt):
        N, C, D, H, W = self.shape
        rng = _rng(22, *self.shape, ("general", "exact", "rounding").index(self.kind), fmt)
        if self.kind == "exact":
            x = dc._dyadic(rng, self.shape, 2, 16)
            w, g = dc._dyadic(rng, (1, C, 3, 3, 3), 1, 8), dc._dyadic(rng, (N, D, H, W), 2, 8)
        else:
            x = rng.standard_normal(self.shape).astype(F32)
            w = (rng.standard_normal((1, C, 3, 3, 3)) / np.sqrt(27.0 * C)).astype(F32)
            g = rng.standard_normal((N, D, H, W)).astype(F32)
        if self.kind == "rounding":
            assert C >= 3
            w[0, :2] = 0
            w[0, 0, 1, 1, 1], w[0, 1, 1, 1, 1] = 1.0, -1.0
            s = specials(fmt)
            flat = g.reshape(-1)
            assert 1 + 3 * s.size < flat.size - 64
            flat[1:1 + 3 * s.size:3] = s                        # (every third position: random values stay in between)
            assert not np.isin(g[N - 1, max(D - 2, 0):, max(H - 2, 0):, max(W - 2, 0):], s).any(), "a special next to the NaN"
            g[N - 1, D - 1, H - 1, W - 1] = np.nan
        x16 = mc.convert(x, fmt)
        assert np.array_equal(mc.convert(mc.up(x16, fmt), fmt), x16)
        if self.kind == "exact":
            assert np.array_equal(mc.up(x16, fmt), x)           # both formats hold the family
        for a in (x16, w, g):
            a.setflags(write=False)
        return x16, w, g

    def made(self, fmt):
        """(x16 patterns, weight, grad_y): computed once per format, shared by every test, never written"""
        if fmt not in self._made:
            self._made[fmt] = self._make(fmt)
        return self._made[fmt]

    def statement(self, fmt):
        key = ("statement", fmt)
        if key not in self._made:
            x16, w, g = self.made(fmt)
            with np.errstate(all="ignore"):
                self._made[key] = ref.Statement(mc.up(x16, fmt), w, g)
        return self._made[key]


def run(api, dev, case, fmt, which=("16", "32")):
    """{"16": the three new entries, "32": the fp32 entries on the up-cast x}, each {y, grad_x, grad_weight}; the 16-bit buffers
    (x and grad_x) sit case.off16 elements into their allocations"""
    N, C, D, H, W = case.shape
    x16, w, g = case.made(fmt)
    out = {}
    dw, dg = mc.Buf(dev, mc.F32, data=w), mc.Buf(dev, mc.F32, data=g)
    n_ws = api.query("ganet_disp_conv_workspace", *case.shape)
    assert n_ws == case.rows * 27 * C, (n_ws, case.rows)
    for arm in which:
        half = arm == "16"
        xf = fmt if half else mc.F32
        dx = mc.Buf(dev, xf, data=x16 if half else mc.up(x16, fmt), off=case.off16 if half else 0)
        y, gw, ws = mc.Buf(dev, mc.F32, n=N * D * H * W), mc.Buf(dev, mc.F32, n=27 * C), mc.Buf(dev, mc.F32, n=n_ws)
        gx = mc.Buf(dev, xf, n=x16.size, off=case.off16 if half else 0)
        if half:
            assert dx.ptr % 8 == gx.ptr % 8 == (2 * case.off16) % 8 and (case.off16 == 0 or dx.ptr % 16), "the case's alignment"
            api.call("ganet_disp_conv_forward_16", dx.ptr, dw.ptr, y.ptr, *case.shape, fmt, dev.stream)
            api.call("ganet_disp_conv_backward_data_16", dg.ptr, dw.ptr, gx.ptr, *case.shape, fmt, dev.stream)
            api.call("ganet_disp_conv_backward_weight_16", dx.ptr, dg.ptr, ws.ptr, gw.ptr, *case.shape, fmt, dev.stream)
        else:
            api.call("ganet_disp_conv_forward", dx.ptr, dw.ptr, y.ptr, *case.shape, dev.stream)
            api.call("ganet_disp_conv_backward_data", dg.ptr, dw.ptr, gx.ptr, *case.shape, dev.stream)
            api.call("ganet_disp_conv_backward_weight", dx.ptr, dg.ptr, ws.ptr, gw.ptr, *case.shape, dev.stream)
        dev.sync()
        assert np.array_equal(dx.host().view(np.uint8), np.ascontiguousarray(x16 if half else mc.up(x16, fmt)).ravel().view(np.uint8)), "x written"
        assert np.array_equal(dw.host().view(np.uint8), w.ravel().view(np.uint8)) and np.array_equal(dg.host().view(np.uint8), g.ravel().view(np.uint8))
        rows = ws.host()
        if case.kind != "rounding":
            assert np.isfinite(rows).all(), "a workspace element was left unwritten"
        out[arm] = {"y": y.host((N, D, H, W)), "grad_x": gx.host(case.shape), "grad_weight": gw.host((C, 3, 3, 3)), "fmt": xf}
    return out


def compare(case, fmt, got16, got32):
    """the contract: y and grad_weight equal the fp32 entry's bits, grad_x equals convert of the fp32 entry's"""
    for q in ("y", "grad_weight"):
        assert got16[q].dtype == F32
        mc.assert_same(got16[q], got32[q], mc.F32, f"{case.id} {mc.FMT_NAME[fmt]} {q}")
    assert got16["grad_x"].dtype == np.uint16 and got32["grad_x"].dtype == F32
    mc.assert_same(got16["grad_x"], mc.convert(got32["grad_x"], fmt), fmt, f"{case.id} {mc.FMT_NAME[fmt]} grad_x")


def compare_exact(case, fmt, got16):
    """the exact family against the float64 statement: equality on all three (grad_x: the statement's value, rounded once)"""
    want = case.statement(fmt).results()
    for q in ("y", "grad_weight"):
        bad = ~(got16[q].astype(np.float64) == want[q])
        assert not bad.any(), (case.id, q, f"{int(bad.sum())} of {bad.size} elements differ from the float64 statement")
    gx32 = want["grad_x"].astype(F32)
    assert np.array_equal(gx32.astype(np.float64), want["grad_x"])
    mc.assert_same(got16["grad_x"], mc.convert(gx32, fmt), fmt, f"{case.id} {mc.FMT_NAME[fmt]} grad_x against the statement")


def premises(case, fmt):
    """the exact family's: grids, ranges, every partial sum within 24 bits under any order (disp_conv_cases.premises)"""
    N, C, D, H, W = case.shape
    x16, w, g = case.made(fmt)
    for a, den, bound in ((mc.up(x16, fmt), 16, 2), (w, 8, 1), (g, 8, 2)):
        assert np.array_equal(a * den, np.round(a * den)) and np.abs(a).max() <= bound
    assert 27 * C * 2 * 128 < 2 ** 24 and N * D * H * W * 4 * 128 < 2 ** 24
    for a in case.statement(fmt).results().values():
        assert np.array_equal(a.astype(F32).astype(np.float64), a)


def truncate(f, fmt):
    """what a truncating store would write: the upper bits of the fp32 pattern (bf16), numpy's round-toward-zero (fp16)"""
    f = np.ascontiguousarray(f, F32)
    if fmt == mc.BF16:
        return (f.view(np.uint32) >> 16).astype(np.uint16)
    with np.errstate(all="ignore"):
        r = f.astype(np.float16)
        over = np.abs(r.astype(F32)) > np.abs(f)                 # rounded away from zero: step back
        bits = r.view(np.uint16)
        return np.where(over & ~np.isnan(f), bits - 1, bits).astype(np.uint16)


def rounding_premises(case, fmt, gx32):
    """what the rounding family contains, asserted on an fp32 grad_x of the case (a run's, or the statement's)"""
    assert case.kind == "rounding"
    gx32 = np.ascontiguousarray(gx32, F32)
    want = mc.convert(gx32, fmt)
    mid, even = tie_values(fmt)
    for sign, ch in ((1.0, 0), (-1.0, 1)):                       # every tie, both signs, in both centre-tap channels
        plane = gx32[:, ch].ravel()
        for m, e in zip(mid, even):
            for s in (1.0, -1.0):
                hit = np.flatnonzero(plane == F32(s * sign * m))
                assert hit.size, (case.id, float(m))
                got = want[:, ch].ravel()[hit[0]]
                assert got == (int(e) | (0x8000 if s * sign < 0 else 0)), (case.id, float(m), hex(int(got)))
        assert (np.array(even) & 1 == 0).all()
    inf = 0x7C00 if fmt == mc.F16 else 0x7F80
    finite = np.isfinite(gx32)
    assert ((want == inf) & finite).any() and ((want == (inf | 0x8000)) & finite).any(), "a finite value that overflows, both signs"
    if fmt == mc.F16:
        mag = want & 0x7FFF
        assert ((mag > 0) & (mag < 0x0400)).sum() >= 4, "fp16 subnormal results"
        assert ((mag == 0) & (gx32 != 0) & finite).any(), "an underflow to zero"
    nan = np.isnan(gx32)
    assert nan.any() and nan.sum() <= 27 * case.shape[1] and np.array_equal(mc.is_nan(want, fmt), nan)
    differs = (truncate(gx32, fmt) != want) & ~nan
    assert differs.mean() >= 0.25, (case.id, float(differs.mean()))
    return float(differs.mean())


SHAPES = [("C1-W1", (1, 1, 1, 1, 1)),
          ("C3-W3-H3-D8", (1, 3, 8, 3, 3)),
          ("C4-W4-H1-D9", (1, 4, 9, 1, 4)),
          ("C5-W5-H3-D1-N2", (2, 5, 1, 3, 5)),
          ("C33-W8-H3-D9-N2", (2, 33, 9, 3, 8)),
          ("C64-W8-H1", (1, 64, 2, 1, 8)),
          ("blocks-vec", (1, 2, 2, 9, 32)),
          ("blocks-twin", (1, 3, 2, 5, 53)),
          ("offset2", (2, 4, 9, 3, 16)),
          ("offset8", (2, 4, 9, 3, 16))]
OFF16 = {"offset2": 1, "offset8": 4}
ROUNDING = [("round-vec", (1, 4, 3, 6, 20)), ("round-twin", (1, 5, 3, 9, 19)), ("round-offset2", (1, 3, 3, 6, 20))]


def _cases():
    cs = []
    for name, shape in SHAPES:
        for kind in ("general", "exact"):
            cs.append(Case(name, shape, kind, OFF16.get(name, 0)))
    for name, shape in ROUNDING:
        cs.append(Case(name, shape, "rounding", 1 if name.endswith("offset2") else 0))
    return cs


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def by_name(name, kind="general"):
    return next(c for c in CASES if c.name == name and c.kind == kind)


def check_case(api, dev, case, fmt):
    got = run(api, dev, case, fmt)
    compare(case, fmt, got["16"], got["32"])
    if case.kind == "exact":
        compare_exact(case, fmt, got["16"])
    if case.kind == "rounding":
        print(f"{case.id} {mc.FMT_NAME[fmt]}: a truncating store would differ on {rounding_premises(case, fmt, got['32']['grad_x']):.3f} of grad_x")
    return got


def check_table():
    """the table reaches what its docstring names"""
    shapes = [c.shape for c in CASES if c.kind != "rounding"]
    assert {s[4] for s in shapes} >= {1, 3, 4, 5, 8} and {s[3] for s in shapes} >= {1, 3} and {s[2] for s in shapes} >= {1, 8, 9}
    assert {s[1] for s in shapes} >= {1, 3, 4, 5, 33, 64} and any(s[0] == 2 for s in shapes)
    assert (ref.PX, ref.WAVES, ref.DEPTH, ref.CB, ref.MAX_C) == (4, 4, 8, 4, 64)
    v, t = by_name("blocks-vec"), by_name("blocks-twin")
    assert v.vec and v.blocks == 2 and not t.vec and t.blocks == 2 and t.shape[4] % 4
    o2, o8 = by_name("offset2"), by_name("offset8")
    assert o2.shape == o8.shape and o2.shape[4] % 4 == 0 and (o2.off16, o8.off16) == (1, 4) and not o2.vec and o8.vec
    assert o8.chunks == 2 and o8.shape[0] == 2 and (2 * o8.off16) % 16 == 8
    assert any(c.vec for c in CASES if c.kind == "rounding") and any(not c.vec for c in CASES if c.kind == "rounding")
    assert by_name("C33-W8-H3-D9-N2").shape[1] % ref.CB == 1 and -(-33 // ref.WAVES) == 9      # a channel block of one; uneven wave split
    for c in CASES:
        assert c.shape[1] <= ref.MAX_C


def check_bad_arguments(api, dev):
    """the fp32 entries' refusals, and a type code that is not fp16 / bf16; a refused call launches nothing"""
    from ganet_amd._native import E_INVALID, E_UNSUPPORTED, GanetError
    bufs = [dev.empty((27 * 65,)) for _ in range(4)]
    p = [dev.ptr(b) for b in bufs]
    good = (1, 1, 1, 1, 1)

    def refused(text, code, name, *args):
        try:
            api.call(name, *args)
        except GanetError as e:
            assert text in str(e) and e.code == code, (name, args, str(e))
            # the library's own message names the entry that was called (the launchers behind the fp32 and the _16 entries are shared)
            assert str(e).startswith(f"{name} failed ({code}): {name}: "), (name, str(e))
        else:
            raise AssertionError((name, args))

    for name, n in ENTRIES16:
        for k in range(5):
            for bad in (0, -1):
                refused("non-positive", E_INVALID, name, *p[:n], *(good[:k] + (bad,) + good[k + 1:]), mc.BF16, dev.stream)
        for k in range(n):
            ptrs = list(p[:n])
            ptrs[k] = None
            refused("null pointer", E_INVALID, name, *ptrs, *good, mc.F16, dev.stream)
        refused("at most 64", E_UNSUPPORTED, name, *p[:n], 1, 65, 1, 1, 1, mc.F16, dev.stream)
        refused("alias", E_INVALID, name, *([p[0]] * n), *good, mc.BF16, dev.stream)
        for code in (mc.F32, 3, -1):
            refused("type code", E_INVALID, name, *p[:n], *good, code, dev.stream)
        refused("beyond the launch grid", E_UNSUPPORTED, name, *p[:n], 65536, 1, 1, 1, 1, mc.F16, dev.stream)
    refused("workspace is beyond ganet_disp_conv_workspace's answer", E_UNSUPPORTED, "ganet_disp_conv_backward_weight_16", *p[:4],
            *dc.BEYOND_WORKSPACE, mc.BF16, dev.stream)
    dev.sync()
    for b in bufs:
        assert np.isnan(np.asarray(dev.host(b))).all()
