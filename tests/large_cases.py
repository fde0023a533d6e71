"""TEST INFRASTRUCTURE: the large-offset cases -- every kernel family on an operand just past 2^31 elements -- shared by
tests/test_large_cases_cpu.py (the machinery, on the CPU, never skipped) and tests/test_gpu_large_offsets.py (gfx950 build,
C ABI).  DESIGN.md section 2 promises 64-bit element offsets everywhere; this table is what holds the kernels to it.

INPUTS: A REPLICATED POOL.  Every op here is independent per slice (n, (n, c) or b; BatchNorm's statistics and DispConv's weight
gradient reduce over slices and are dealt with in their cases).  A case names a small block shape for one slice and a
replication count R such that its largest operand ends within one slice past 2^31 elements.  Slice k holds pool block
k mod P, P = 3 seeded blocks; four slices hold blocks of their own: the first, the last, and the two that straddle elements
2^30 and 2^31 of the largest operand -- at most P + 4 distinct blocks.  Inputs are gathered from the pool on the device;
every output and workspace starts as NaN (integer outputs: a pattern the op cannot produce).

REFERENCE.  The family's own float64 statement (sga_ref64, misc_ref64, bn_ref64, disp_tail_ref64, disp_conv_ref64) or the
oracle where the family's bar is stated against it (SGA, LGA: forward bit-exact / 1e-4, parity_cases.TOL), evaluated on the
CPU on the distinct blocks only, at the family's existing bar.  No tolerance is introduced here.

CHECK (Checker).  (a) the first occurrence of every distinct block goes to the host and is held to the reference; (b) every
other slice is compared with its representative where the tensor lives -- equality where the family is bit-reproducible across
positions, max |a - b| <= bar for the SGA / LGA gradients, whose summation order may depend on the address; (c) a NaN or a
poison pattern fails (a) or (b) wherever it sits; inputs are compared with a fresh gather from the pool afterwards.

TEETH (assert_teeth, index arithmetic only).  For every operand and every distance a truncated offset could wrap by -- 2^31
and 2^32 elements, 2^31 and 2^32 bytes -- the element a wrapped access would land on differs in reference value from the true
element somewhere in the slice that straddles the distance and in the slice behind it.  The odd P, slice sizes that are no
powers of two and the special slices are there for that; the assertion shows it.

NOT APPLICABLE (NOT_APPLICABLE below names every exported entry that is not in the table, with the line that says why):
the criterion refuses 2^24 pixels or more (ganet_capi.hip: "counts are reported as floats"), the image front and back end
refuse planes above 2^24 / 2^28 pixels, the queries and self-tests take no tensor.  Three entries that refuse nothing are
marked NOT COVERED there with the reason (two need more than the 48 GiB a case may take, one has no bar that applies)."""
import math
import os
import re

import numpy as np

import mixed_cases as mc

P = 3
MARKS = (1 << 30, 1 << 31)
CAP_BYTES = 48 << 30
HEADROOM = 4 << 30
TEMP_BYTES = 2 << 30          # the checker's own chunks: a gathered chunk, a difference, a mask
CHUNK = 1 << 27               # elements per device-side comparison
MAX_SLICES = 65535
F32, F64 = np.float32, np.float64
POISON = {np.dtype(np.uint8): 113, np.dtype(np.uint16): 0x7FC1}     # mask is 0..3, kp < D, and 0x7FC1 is a NaN no convert() makes

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ganet_hip.h")


# ---- what a tensor of a case is -----------------------------------------------------------------------------------------------
class Spec:
    """one tensor [lead][R][per]: `kind` is the family's bar against the reference --
         "bits"            equal to the reference (cast to the tensor's type) bit for bit
         "equal"           IEEE-equal to the float64 value (exact families)
         ("abs", t)        max |got - want| <= t
         ("close", r, a)   |got - want| <= a + r |want|
         "bar"             |got - want| <= the per-element bar the reference returns beside the value
         None              no reference (a private workspace in a private layout): (b) alone
    `rep`: how slices are compared with their representative: "equal" or ("abs", t)."""

    def __init__(self, per, dtype=F32, lead=1, kind="bits", rep="equal", role="out", fmt=None):
        """fmt: the 16-bit float format (mixed_cases.F16 / BF16) of a uint16 tensor that is compared by value, not by pattern"""
        self.per, self.dtype, self.lead, self.kind, self.rep, self.role, self.fmt = int(per), np.dtype(dtype), lead, kind, rep, role, fmt

    @property
    def itemsize(self):
        return self.dtype.itemsize


def IN(per, dtype=F32, lead=1):
    return Spec(per, dtype, lead, kind="bits", role="in")


class Layout:
    """which block every slice holds"""

    def __init__(self, R, anchor_per, anchor_lead=1):
        self.R = R
        special = {0, R - 1}
        for m in MARKS:
            if m < anchor_lead * R * anchor_per:
                special.add((m // anchor_per) % R)
        self.special = sorted(special)
        self.block_of = np.arange(R, dtype=np.int64) % P
        for j, k in enumerate(self.special):
            self.block_of[k] = P + j
        self.nb = P + len(self.special)
        self.first = np.array([int(np.flatnonzero(self.block_of == b)[0]) for b in range(self.nb)])
        self.count = np.bincount(self.block_of, minlength=self.nb)


def ratio_of(got, want, kind, bar=None):
    """-> worst error / bar of one block (0 or inf for the exact kinds); raises nothing"""
    got = np.asarray(got)
    if kind == "bits":
        want = np.ascontiguousarray(np.asarray(want).astype(got.dtype))
        return 0.0 if np.array_equal(got.view(np.uint8), want.view(np.uint8)) else math.inf
    g, w = got.astype(F64), np.asarray(want, F64)
    if kind == "equal":
        return 0.0 if bool((g == w).all()) else math.inf
    if kind == "bar":
        b = np.asarray(bar, F64)
    elif kind[0] == "abs":
        b = np.full(w.shape, kind[1])
    else:
        b = kind[2] + kind[1] * np.abs(w)
    err = np.abs(g - w)
    with np.errstate(all="ignore"):
        r = np.where(err == 0, 0.0, err / b)
    r = np.where(np.isfinite(g), r, math.inf)
    return float(r.max())


class Checker:
    """(a) and (b) over a `store`: TorchStore below (device tensors) or test_large_cases_cpu's virtual numpy tensor.
    store.host(name, lead_index, slice) -> numpy [per];  store.worst_to_representative(name, spec, layout) -> the largest
    |slice - representative| over every slice (0.0 where all are equal, inf / nan where an element is NaN or differs under
    "equal")."""

    def __init__(self, case, store):
        self.case, self.store, self.ratios = case, store, {}

    def check(self, name):
        case, lay = self.case, self.case.layout
        spec = case.tensors[name]
        worst = 0.0
        if spec.kind is not None:
            want = case.want[name]
            bars = case.want.get(name + "/bar")
            for b in range(lay.nb):
                for l in range(spec.lead):
                    got = self.store.host(name, l, int(lay.first[b]))
                    if spec.fmt is not None:
                        got = mc.up(got, spec.fmt)
                    w = want[b].reshape(spec.lead, spec.per)[l]
                    r = ratio_of(got, w, spec.kind, None if bars is None else bars[b].reshape(spec.lead, spec.per)[l])
                    assert r <= 1.0, (case.name, name, f"block {b} (slice {int(lay.first[b])}, part {l}): error / bar = {r:.3g}")
                    worst = max(worst, r)
        d = self.store.worst_to_representative(name, spec, lay)
        tol = 0.0 if spec.rep == "equal" else spec.rep[1]
        assert d <= tol, (case.name, name, f"a slice differs from its representative by {d:.3g} (allowed {tol:.3g})")
        if tol:
            worst = max(worst, d / tol)
        self.ratios[name] = worst
        return worst


# ---- the teeth ------------------------------------------------------------------------------------------------------------------
def wrap_distances(itemsize):
    """in elements: 2^31 and 2^32 elements, 2^31 and 2^32 bytes"""
    return sorted({1 << 31, 1 << 32, (1 << 31) // itemsize, (1 << 32) // itemsize})


def value_at(values, spec, layout, flat_lo, flat_hi):
    """reference values of elements [flat_lo, flat_hi) of the tensor [lead][R][per], from the per-block values [nb, lead * per]"""
    i = np.arange(flat_lo, flat_hi, dtype=np.int64)
    q, e = i // spec.per, i % spec.per
    l, k = q // layout.R, q % layout.R
    return values[layout.block_of[k], l * spec.per + e]


def assert_teeth(case):
    """-> number of (tensor, distance, slice) triples examined"""
    lay, n = case.layout, 0
    for name, spec in case.tensors.items():
        values = case.inputs.get(name) if spec.role == "in" else case.want.get(name)
        if values is None:
            continue
        values = np.asarray(values).reshape(lay.nb, spec.lead * spec.per)
        total = spec.lead * lay.R * spec.per
        for w in wrap_distances(spec.itemsize):
            if w >= total:
                continue
            q = w // spec.per
            for s in (q, q + 1):
                lo, hi = max(s * spec.per, w), min((s + 1) * spec.per, total)
                if lo >= hi:
                    continue
                true, wrapped = value_at(values, spec, lay, lo, hi), value_at(values, spec, lay, lo - w, hi - w)
                differ = ~((true == wrapped) | ((true != true) & (wrapped != wrapped)))
                assert differ.any(), (case.name, name, f"a wrap by {w} elements is invisible in slice {s}")
                n += 1
    return n


# ---- a case -------------------------------------------------------------------------------------------------------------------
class Case:
    """name, family; `entries`: the ABI entries its script calls; dims: the block shape; tensors: name -> Spec; anchor: the
    tensor that must end just past `target` elements; data(case, nb) -> {input: [nb, ...]}; ref(case, inputs) -> {output:
    [nb, ...]} (+ "<name>/bar" for kind "bar"); script(ctx): the calls, written against a context (DryCtx for the peak,
    DeviceCtx on the device)."""

    def __init__(self, name, family, entries, dims, tensors, anchor, data, ref, script, target=1 << 31, seed=0):
        self.name, self.family, self.entries, self.dims, self.tensors = name, family, tuple(entries), tuple(dims), tensors
        self.anchor, self._data, self._ref, self.script, self.seed = anchor, data, ref, script, seed
        a = tensors[anchor]
        self.R = target // (a.lead * a.per) + 1
        self.layout = Layout(self.R, a.per, a.lead)
        self._made = None
        self._peak = None

    def __repr__(self):
        return self.name

    def largest(self):
        return max(s.lead * self.R * s.per for s in self.tensors.values())

    def rng(self):
        return np.random.default_rng([91, self.seed] + [int(v) for v in self.dims])

    @property
    def made(self):
        """(inputs, wants) on the distinct blocks: computed once, shared, read-only"""
        if self._made is None:
            inputs = {k: np.ascontiguousarray(v) for k, v in self._data(self, self.layout.nb).items()}
            want = self._ref(self, inputs)
            for a in list(inputs.values()) + [v for v in want.values() if isinstance(v, np.ndarray)]:
                a.setflags(write=False)
            self._made = (inputs, want)
        return self._made

    inputs = property(lambda self: self.made[0])
    want = property(lambda self: self.made[1])

    @property
    def peak(self):
        """peak device bytes, from the shapes: the script run against a context that only counts"""
        if self._peak is None:
            ctx = DryCtx(self)
            self.script(ctx)
            self._peak = ctx.peak + TEMP_BYTES
        return self._peak


class DryCtx:
    """runs a case's script without a device: counts bytes, records the entries called"""
    dry = True

    def __init__(self, case):
        self.case, self.R, self.dims = case, case.R, case.dims
        self.live, self.now, self.peak, self.called = {}, 0, 0, []

    def _add(self, name, nbytes):
        assert name not in self.live, name
        self.live[name] = nbytes
        self.now += nbytes
        self.peak = max(self.peak, self.now)
        return name

    def input(self, name):
        s = self.case.tensors[name]
        assert s.role == "in", name
        return self._add(name, s.lead * self.R * s.per * s.itemsize)

    def output(self, name):
        s = self.case.tensors[name]
        assert s.role != "in", name
        return self._add(name, s.lead * self.R * s.per * s.itemsize)

    def small(self, name, array=None, shape=None, dtype=F32, inout=False):
        n = np.asarray(array).size if array is not None else int(np.prod(shape))
        return self._add(name, n * np.dtype(dtype).itemsize)

    def free(self, *names):
        for n in names:
            self.now -= self.live.pop(n)

    def call(self, entry, *args):
        self.called.append(entry)

    def query(self, entry, *args):
        return 0

    def check(self, *names):
        pass

    def unchanged(self, *names):
        pass

    def same(self, a, b, tol=0.0):
        pass

    def host_small(self, name):
        return None

    def expect(self, cond, what=""):
        pass


# ---- the device side -----------------------------------------------------------------------------------------------------------
def _tdtype(torch, dtype):
    return {np.dtype(F32): torch.float32, np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.int16,
            np.dtype(F64): torch.float64}[np.dtype(dtype)]


def _as_torch_array(a):
    a = np.array(a)                                      # (a writable copy: the shared blocks are read-only)
    return a.view(np.int16) if a.dtype == np.uint16 else a


class TorchStore:
    def __init__(self, torch, tensors, idx):
        self.torch, self.t, self.idx = torch, tensors, idx

    def host(self, name, l, k):
        a = self.t[name][l, k].cpu().numpy()
        return a.view(np.uint16) if a.dtype == np.int16 else a

    def worst_to_representative(self, name, spec, lay):
        torch = self.torch
        t = self.t[name]
        first = torch.from_numpy(lay.first).to(t.device)
        rows = max(1, CHUNK // spec.per)
        worst = torch.zeros((), dtype=torch.float64, device=t.device)
        for l in range(spec.lead):
            rep = t[l].index_select(0, first)
            for a in range(0, lay.R, rows):
                got, exp = t[l, a:a + rows], rep.index_select(0, self.idx[a:a + rows])
                if spec.rep == "equal":
                    d = torch.where((got == exp).all(), 0.0, math.inf).to(torch.float64)
                else:
                    d = (got - exp).abs().max().to(torch.float64)
                worst = torch.where(torch.isnan(d) | (d > worst), d, worst)      # (a NaN stays)
                del got, exp, d
        v = float(worst.item())
        return math.inf if v != v else v


class DeviceCtx:
    """runs a case's script on the device through the C ABI"""
    dry = False

    def __init__(self, case, api, dev):
        self.case, self.api, self.dev, self.torch = case, api, dev, dev.torch
        self.R, self.dims = case.R, case.dims
        self.t, self.smalls, self.given = {}, {}, {}
        self.idx = self.torch.from_numpy(case.layout.block_of).to(dev.device)
        self.store = TorchStore(self.torch, self.t, self.idx)
        self.checker = Checker(case, self.store)
        self.called = []

    def _gather(self, name, out=None):
        s = self.case.tensors[name]
        pool = self.torch.from_numpy(_as_torch_array(self.case.inputs[name]).reshape(self.case.layout.nb, s.lead, s.per)).to(self.dev.device)
        t = self.torch.empty((s.lead, self.R, s.per), dtype=pool.dtype, device=self.dev.device) if out is None else out
        for l in range(s.lead):
            self.torch.index_select(pool[:, l], 0, self.idx, out=t[l])
        return t

    def input(self, name):
        assert self.case.tensors[name].role == "in" and name not in self.t
        self.t[name] = self._gather(name)
        return name                                      # (a name, not the tensor: a script's locals must not keep memory alive)

    def output(self, name):
        s = self.case.tensors[name]
        assert s.role != "in" and name not in self.t
        t = self.torch.empty((s.lead, self.R, s.per), dtype=_tdtype(self.torch, s.dtype), device=self.dev.device)
        if s.dtype == np.dtype(F32):
            t.fill_(float("nan"))
        else:
            p = POISON[s.dtype]
            t.fill_(p if s.dtype != np.dtype(np.uint16) else int(np.array(p, np.uint16).view(np.int16)))
        self.t[name] = t
        return name

    def small(self, name, array=None, shape=None, dtype=F32, inout=False):
        """a tensor that is not replicated (parameters, statistics, a workspace): given, or NaN-filled.  A given one must come
        back unchanged (checked against this copy when the script has run) unless it is `inout` (the running statistics)"""
        if array is not None:
            t = self.torch.from_numpy(np.array(array, dtype)).to(self.dev.device)
            if not inout:
                self.given[name] = (t, np.array(array, dtype))
        else:
            t = self.torch.full(tuple(shape), float("nan"), dtype=_tdtype(self.torch, dtype), device=self.dev.device)
        self.smalls[name] = t
        return name

    def host_small(self, name):
        self.torch.cuda.synchronize()
        return self.smalls[name].cpu().numpy()

    def free(self, *names):
        for n in names:
            if n in self.t:
                del self.t[n]
            else:
                del self.smalls[n]

    def _arg(self, a):
        if isinstance(a, str):
            return (self.t[a] if a in self.t else self.smalls[a]).data_ptr()
        return a

    def call(self, entry, *args):
        self.called.append(entry)
        self.api.call(entry, *[self._arg(a) for a in args], self.dev.stream)

    def query(self, entry, *args):
        return self.api.query(entry, *[self._arg(a) for a in args])

    def check(self, *names):
        self.torch.cuda.synchronize()
        for n in names:
            self.checker.check(n)

    def unchanged(self, *names):
        """inputs against a fresh gather from the pool"""
        self.torch.cuda.synchronize()
        for n in names:
            s = self.case.tensors[n]
            pool = self.torch.from_numpy(_as_torch_array(self.case.inputs[n]).reshape(self.case.layout.nb, s.lead, s.per)).to(self.dev.device)
            rows = max(1, CHUNK // s.per)
            ok = self.torch.ones((), dtype=self.torch.bool, device=self.dev.device)
            for l in range(s.lead):
                for a in range(0, self.R, rows):
                    ok = ok & (self.t[n][l, a:a + rows] == pool[:, l].index_select(0, self.idx[a:a + rows])).all()
            assert bool(ok.item()), (self.case.name, n, "an input was written")

    def same(self, a, b, tol=0.0):
        """two tensors of the run against each other, chunked: equal (tol 0) or within tol"""
        self.torch.cuda.synchronize()
        ta, tb = self.t[a].reshape(-1), self.t[b].reshape(-1)
        worst = 0.0
        for i in range(0, ta.numel(), CHUNK):
            x, y = ta[i:i + CHUNK], tb[i:i + CHUNK]
            if tol == 0.0:
                assert self.torch.equal(x, y), (self.case.name, a, b, "differ")
            else:
                d = float((x - y).abs().max().item())
                assert d <= tol, (self.case.name, a, b, d)
                worst = max(worst, d)
        self.checker.ratios[f"{a} against {b}"] = worst / tol if tol else 0.0

    def expect(self, cond, what=""):
        assert cond, (self.case.name, what)


def run_on_device(case, api, dev, skip):
    """-> {"peak": bytes, "seconds": wall time, "ratios": {tensor: worst error / bar}}; `skip(reason)` is pytest.skip"""
    import time
    torch = dev.torch
    free, total = torch.cuda.mem_get_info()
    if free < case.peak + HEADROOM:
        skip(f"{case.name}: {free} bytes free on the device, the case needs {case.peak + HEADROOM} (peak {case.peak} + {HEADROOM})")
    case.made                                           # (the references: outside the timed part)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    ctx = DeviceCtx(case, api, dev)
    try:
        case.script(ctx)
        torch.cuda.synchronize()
        for name, (t, a) in ctx.given.items():
            assert np.array_equal(t.cpu().numpy().view(np.uint8), a.view(np.uint8)), (case.name, name, "a parameter was written")
        called = set(ctx.called)
        assert called == set(case.entries), (case.name, "entries called", sorted(called ^ set(case.entries)))
        res = {"peak": case.peak, "measured_peak": int(torch.cuda.max_memory_allocated()), "seconds": time.perf_counter() - t0,
               "ratios": dict(ctx.checker.ratios)}
    finally:
        ctx.t.clear()
        ctx.smalls.clear()
        ctx.given.clear()
        del ctx
        torch.cuda.empty_cache()
    assert res["measured_peak"] <= case.peak, (case.name, "the peak computed from the shapes is too low", res)
    return res


# ---- references shared by several cases ---------------------------------------------------------------------------------------
def _oracle():
    from oracle.oracle import Oracle
    return Oracle("port")


def _l1(g, axis):
    return (g / np.abs(g).sum(axis, keepdims=True)).astype(F32)


def _flat(a, nb):
    return np.ascontiguousarray(a).reshape(nb, -1)


# =================================================================================================================================
# SGA
# =================================================================================================================================
TOL = 1e-4                       # parity_cases.TOL: the SGA / LGA gradient bar


def _sga_data(case, nb):
    D, H, W = case.dims
    rng = case.rng()
    d = {"x": rng.standard_normal((nb, D, H, W)).astype(F32), "go": rng.standard_normal((nb, D, H, W)).astype(F32)}
    for k in range(4):
        d[f"g{k}"] = _l1(rng.standard_normal((nb, 5, H, W)), 1)
    return d


def _sga_ref(case, inp):
    """the oracle on the distinct blocks as ONE tensor [1, nb, D, H, W]: slices (n, c) are independent"""
    nb = case.layout.nb
    o = _oracle()
    x, go = inp["x"][None], inp["go"][None]
    gs = [inp[f"g{k}"][None] for k in range(4)]
    out, tmp, mask = o.sga_forward(x, *gs)
    A = np.stack([o.sga_scan(x, gs[k], k)[0] for k in range(4)], 1)                      # [nb, 4, D, H, W]
    assert np.array_equal(A[:, 3], tmp[0])
    grads = o.sga_backward(x, *gs, tmp, mask, go)
    want = {"A": _flat(A, nb), "out": _flat(out, nb), "mask": _flat(mask.astype(np.uint8), nb),
            "kp": _flat(np.argmax(A, axis=2).astype(np.uint16), nb), "gx": _flat(grads[0], nb)}
    for k in range(4):
        want[f"gw{k}"] = _flat(grads[1 + k], nb)
    return want


def _sga_tensors(D, H, W):
    E, HW = D * H * W, H * W
    t = {"x": IN(E), "go": IN(E), "A": Spec(E, lead=4), "out": Spec(E), "mask": Spec(E, np.uint8), "kp": Spec(HW, np.uint16, lead=4),
         "G": Spec(E, lead=4, kind=None, rep=("abs", TOL), role="ws"), "gx": Spec(E, kind=("abs", TOL), rep=("abs", TOL)),
         # the steps once more, into buffers of their own (tiled case)
         "A2": Spec(E, lead=4), "G2": Spec(E, lead=4, kind=None, rep=("abs", TOL), role="ws"),
         "gx2": Spec(E, kind=("abs", TOL), rep=("abs", TOL))}
    for k in range(4):
        t[f"g{k}"] = IN(5 * HW)
        t[f"gw{k}"] = Spec(5 * HW, kind=("abs", TOL), rep=("abs", TOL))
        t[f"gw{k}b"] = Spec(5 * HW, kind=("abs", TOL), rep=("abs", TOL))
    return t


def _sga_composite(tiled, steps):
    def script(ctx):
        D, H, W = ctx.dims
        dims = (1, ctx.R, D, H, W)
        if not ctx.dry:
            ctx.expect(ctx.query("ganet_sga_workspace_layout", *dims) == tiled, "workspace layout")
        x, gs = ctx.input("x"), [ctx.input(f"g{k}") for k in range(4)]
        A, out, mask, kp = ctx.output("A"), ctx.output("out"), ctx.output("mask"), ctx.output("kp")
        ctx.call("ganet_sga_forward", x, *gs, A, out, mask, kp, *dims)
        ctx.check("A", "out", "mask", "kp")
        ctx.free("out")
        go, G, gx = ctx.input("go"), ctx.output("G"), ctx.output("gx")
        gw = [ctx.output(f"gw{k}") for k in range(4)]
        ctx.call("ganet_sga_backward", x, *gs, A, mask, kp, go, G, gx, *gw, *dims)
        ctx.check("gx", "gw0", "gw1", "gw2", "gw3", "G")
        if steps:
            # the composite entries are their steps, bit for bit (parity_cases.check_sga_forward_backward): here on the same sizes
            A2 = ctx.output("A2")
            for k in range(4):
                ctx.call("ganet_sga_scan_forward_ws", x, gs[k], A2, *dims, k)
            ctx.same("A2", "A")
            ctx.free("A2")
            G2 = ctx.output("G2")
            for k in range(4):
                ctx.call("ganet_sga_backward_scan_ws", gs[k], mask, kp, go, G2, *dims, k)
            ctx.same("G2", "G")
            ctx.free("G")
            gx2 = ctx.output("gx2")
            gwb = [ctx.output(f"gw{k}b") for k in range(4)]
            ctx.call("ganet_sga_backward_point", x, *gs, A, G2, gx2, *gwb, *dims)
            ctx.same("gx2", "gx")
            for k in range(4):
                ctx.same(f"gw{k}b", f"gw{k}")
        ctx.unchanged("x", "go", "g0", "g1", "g2", "g3")
    return script


def _sga_composite_ref(case, inp):
    want = _sga_ref(case, inp)
    want["A2"], want["gx2"] = want["A"], want["gx"]
    for k in range(4):
        want[f"gw{k}b"] = want[f"gw{k}"]
    return want


# ---- single scans: x itself past 2^31 ------------------------------------------------------------------------------------------
def _scan_data(case, nb):
    D, H, W = case.dims
    rng = case.rng()
    return {"x": rng.standard_normal((nb, D, H, W)).astype(F32), "g": _l1(rng.standard_normal((nb, 5, H, W)), 1),
            "go": rng.standard_normal((nb, D, H, W)).astype(F32), "mask": rng.integers(0, 4, (nb, D, H, W)).astype(np.uint8),
            "kpd": rng.integers(0, D, (nb, H, W)).astype(np.uint16)}


def _scan_ref(direction):
    def ref(case, inp):
        import sga_ref64
        nb = case.layout.nb
        x, g, go = inp["x"][None], inp["g"][None], inp["go"][None]
        A = _oracle().sga_scan(x, g, direction)
        # the adjoint scan of sga_ref64 on GIVEN selections (mask, kp): the kernel routes by what it is handed
        kp = np.broadcast_to(inp["kpd"][None, None].astype(np.int64), (4, 1) + inp["kpd"].shape)
        fwd = sga_ref64.forward(x, g, g, g, g, kp=kp, mask=inp["mask"][None])
        G = sga_ref64.backward(x, [g] * 4, go, fwd)[f"G{direction}"]
        return {"A": _flat(A, nb), "G": _flat(G, nb)}
    return ref


def _scan_script(direction):
    def script(ctx):
        D, H, W = ctx.dims
        dims = (1, ctx.R, D, H, W)
        x, g, A = ctx.input("x"), ctx.input("g"), ctx.output("A")
        ctx.call("ganet_sga_scan_forward", x, g, A, *dims, direction)
        ctx.check("A")
        ctx.unchanged("x")
        ctx.free("x", "A")
        mask, kp, go, G = ctx.input("mask"), ctx.input("kpd"), ctx.input("go"), ctx.output("G")
        ctx.call("ganet_sga_backward_scan", g, mask, kp, go, G, *dims, direction)
        ctx.check("G")
        ctx.unchanged("g", "mask", "kpd", "go")
    return script


def _scan_tensors(D, H, W):
    E, HW = D * H * W, H * W
    return {"x": IN(E), "g": IN(5 * HW), "go": IN(E), "mask": IN(E, np.uint8), "kpd": IN(HW, np.uint16), "A": Spec(E),
            "G": Spec(E, kind=("abs", TOL), rep=("abs", TOL))}


def _merge_data(case, nb):
    D, H, W = case.dims
    return {"A": case.rng().standard_normal((nb, 4, D, H, W)).astype(F32)}


def _merge_ref(case, inp):
    """sga_ref64.forward's last step: strict <, first arg-max"""
    A = inp["A"]
    out, m = A[:, 0].copy(), np.zeros(A[:, 0].shape, np.uint8)
    for d in (1, 2, 3):
        less = out < A[:, d]
        out[less], m[less] = A[:, d][less], d
    nb = case.layout.nb
    return {"out": _flat(out, nb), "mask": _flat(m, nb), "kp": _flat(np.argmax(A, axis=2).astype(np.uint16), nb)}


def _merge_script(ctx):
    D, H, W = ctx.dims
    A, out, mask, kp = ctx.input("A"), ctx.output("out"), ctx.output("mask"), ctx.output("kp")
    ctx.call("ganet_sga_merge", A, out, mask, kp, 1, ctx.R, D, H, W)
    ctx.check("out", "mask", "kp")
    ctx.unchanged("A")


INFER_SCALE, INFER_SHIFT = np.array([0.5], F32), np.array([-0.25], F32)     # a power of two: fmaf and multiply-add round alike


def _infer_ref(case, inp):
    import parity_cases as pc
    out, _, _ = _oracle().sga_forward(inp["x"][None], *[inp[f"g{k}"][None] for k in range(4)])
    y = pc.bn_relu_keep_nan(out.transpose(1, 0, 2, 3, 4), INFER_SCALE, INFER_SHIFT)      # [nb, 1, D, H, W]: one channel
    assert 0.05 < (y == 0).mean() < 0.95
    return {"out": _flat(y, case.layout.nb)}


def _infer_script(ctx):
    D, H, W = ctx.dims
    dims = (ctx.R, 1, D, H, W)
    x, gs, out = ctx.input("x"), [ctx.input(f"g{k}") for k in range(4)], ctx.output("out")
    sc, sh = ctx.small("scale", INFER_SCALE), ctx.small("shift", INFER_SHIFT)
    if not ctx.dry:
        ctx.expect(ctx.query("ganet_sga_forward_infer_scratch", x, *gs, out, *dims) == 0, "the fused form needs no scratch")
    ctx.call("ganet_sga_forward_infer", x, *gs, None, out, sc, sh, *dims)
    ctx.check("out")
    ctx.unchanged("x", "g0", "g1", "g2", "g3")


def _compat_ref(case, inp):
    """the reference buffer contract's forward: out, temp_out = A_left, a float-valued mask"""
    nb = case.layout.nb
    out, tmp, mask = _oracle().sga_forward(inp["x"][None], *[inp[f"g{k}"][None] for k in range(4)])
    return {"out": _flat(out, nb), "tmp": _flat(tmp, nb), "maskf": _flat(mask.astype(F32), nb)}


def _compat_script(ctx):
    D, H, W = ctx.dims
    x, gs = ctx.input("x"), [ctx.input(f"g{k}") for k in range(4)]
    tmp, out, maskf = ctx.output("tmp"), ctx.output("out"), ctx.output("maskf")
    ctx.call("ganet_sga_forward_compat", x, *gs, tmp, out, maskf, 1, ctx.R, D, H, W)
    ctx.check("out", "tmp", "maskf")
    ctx.unchanged("x", "g0", "g1", "g2", "g3")


# =================================================================================================================================
# LGA
# =================================================================================================================================
def _lga_data(case, nb):
    D, H, W = case.dims
    rng = case.rng()
    return {"x": rng.standard_normal((nb, D, H, W)).astype(F32), "f": _l1(rng.standard_normal((nb, 75, H, W)), 1),
            "gy": rng.standard_normal((nb, D, H, W)).astype(F32)}


def _lga_ref(case, inp):
    o, nb = _oracle(), case.layout.nb
    y = o.lga_forward(inp["x"], inp["f"], 2)
    gx, gf = o.lga_backward(inp["x"], inp["f"], inp["gy"], 2)
    return {"y": _flat(y, nb), "gx": _flat(gx, nb), "gf": _flat(gf, nb)}


def _lga_script(ctx):
    D, H, W = ctx.dims
    dims = (ctx.R, D, H, W, 2)
    x, f, y = ctx.input("x"), ctx.input("f"), ctx.output("y")
    ctx.call("ganet_lga_forward", x, f, y, *dims)
    ctx.check("y")
    ctx.free("y")
    gy, gx, gf = ctx.input("gy"), ctx.output("gx"), ctx.output("gf")
    ctx.call("ganet_lga_backward", x, f, gy, gx, gf, *dims, 0)
    ctx.check("gx", "gf")
    ctx.unchanged("x", "f", "gy")


def _lga2_ref(case, inp):
    import parity_cases as pc
    o, nb = _oracle(), case.layout.nb
    x, f, gy = inp["x"], inp["f"], inp["gy"]
    D, H, W = case.dims
    y, ins = o.lga_chain_forward(x, f, 2, 2)
    gt1, _ = o.lga_backward(ins[1], f, gy, 2)
    gx, gf = o.lga_chain_backward(ins, f, gy, 2)
    inside = np.zeros((25, H, W), bool)                      # the edge sums by their definition (parity_cases.check_lga2_paired)
    for a in range(-2, 3):
        for b in range(-2, 3):
            ii, jj = np.arange(H)[:, None] + a, np.arange(W)[None, :] + b
            inside[(a + 2) * 5 + (b + 2)] = (ii >= 0) & (ii < H) & (jj >= 0) & (jj < W)
    f3 = f.astype(F64).reshape(nb, 3, 25, H, W)
    edge = np.stack([(f3 * ~inside).sum((1, 2)), (f3[:, 0] * inside).sum(1), (f3[:, 2] * inside).sum(1)], 1)
    return {"t1p": _flat(pc.to_paired(ins[1]), nb), "y": _flat(y, nb), "gt1p": _flat(pc.to_paired(gt1), nb), "gx": _flat(gx, nb),
            "gf": _flat(gf, nb), "edge": _flat(edge, nb)}


def _lga2_script(ctx):
    """Lga2Function's call sequence with its private pair-interleaved intermediate and the edge-sum side channel"""
    D, H, W = ctx.dims
    dims = (ctx.R, D, H, W, 2)
    x, f, t1p, edge = ctx.input("x"), ctx.input("f"), ctx.output("t1p"), ctx.output("edge")
    ctx.call("ganet_lga_apply_paired_edges", x, f, t1p, edge, *dims, 0, 0, 1)
    ctx.check("t1p", "edge")
    y = ctx.output("y")
    ctx.call("ganet_lga_apply_paired", t1p, f, y, *dims, 0, 1, 0)
    ctx.check("y")
    ctx.free("y")
    gy, gf = ctx.input("gy"), ctx.output("gf")
    ctx.call("ganet_lga_filter_grad_paired", t1p, gy, gf, *dims, 0, 1, 0)
    ctx.free("t1p")
    gt1p = ctx.output("gt1p")
    ctx.call("ganet_lga_apply_paired_edges", gy, f, gt1p, edge, *dims, 1, 0, 1)
    ctx.check("gt1p")
    ctx.unchanged("gy")
    ctx.free("gy")
    ctx.call("ganet_lga_filter_grad_paired", x, gt1p, gf, *dims, 1, 0, 1)
    ctx.check("gf")
    ctx.unchanged("x")
    ctx.free("x")
    gx = ctx.output("gx")
    ctx.call("ganet_lga_apply_paired", gt1p, f, gx, *dims, 1, 1, 0)
    ctx.check("gx")
    ctx.unchanged("f")


def _lga_tensors(D, H, W):
    E, HW = D * H * W, H * W
    g = dict(kind=("abs", TOL), rep=("abs", TOL))
    return {"x": IN(E), "f": IN(75 * HW), "gy": IN(E), "y": Spec(E, kind=("abs", TOL)), "gx": Spec(E, **g), "gf": Spec(75 * HW, **g),
            "t1p": Spec((D + 1) // 2 * HW * 2, kind=("abs", TOL)), "gt1p": Spec((D + 1) // 2 * HW * 2, **g),
            "edge": Spec(3 * HW, kind=("abs", 1e-5))}


# =================================================================================================================================
# cost volume, cast
# =================================================================================================================================
def _cv_data(case, nb):
    C, Dn, H, W = case.dims
    rng = case.rng()
    d = {"x": rng.standard_normal((nb, C, H, W)).astype(F32), "y": rng.standard_normal((nb, C, H, W)).astype(F32),
         "gcost": rng.integers(-3, 4, (nb, 2 * C, Dn, H, W)).astype(F32)}
    d["x16"], d["y16"] = mc.convert(d["x"], mc.F16), mc.convert(d["y"], mc.F16)      # patterns: the forward copies them
    d["gcost_f16"], d["gcost_bf16"] = mc.convert(d["gcost"], mc.F16), mc.convert(d["gcost"], mc.BF16)
    return d


def _cv_ref(case, inp):
    import misc_ref64 as r64
    C, Dn, H, W = case.dims
    nb = case.layout.nb
    gx, gy = r64.cost_volume_adjoint(inp["gcost"], C)
    assert np.abs(inp["gcost"]).sum(2).max() < 2 ** 8               # every sum an integer that bf16 holds
    cost16 = r64.cost_volume(inp["x16"].astype(F64), inp["y16"].astype(F64), Dn).astype(np.uint16)   # zeros are pattern 0
    w = {"cost": _flat(r64.cost_volume(inp["x"], inp["y"], Dn), nb), "gx": _flat(gx, nb), "gy": _flat(gy, nb), "cost16": _flat(cost16, nb)}
    for tag, fmt in (("f16", mc.F16), ("bf16", mc.BF16)):
        w[f"gx_{tag}"] = _flat(mc.convert(gx.astype(F32), fmt), nb)
        w[f"gy_{tag}"] = _flat(mc.convert(gy.astype(F32), fmt), nb)
    return w


def _cv_tensors(C, Dn, H, W):
    big, sm = 2 * C * Dn * H * W, C * H * W
    t = {"x": IN(sm), "y": IN(sm), "gcost": IN(big), "cost": Spec(big), "gx": Spec(sm, kind="equal"), "gy": Spec(sm, kind="equal"),
         "x16": IN(sm, np.uint16), "y16": IN(sm, np.uint16), "cost16": Spec(big, np.uint16)}
    for tag in ("f16", "bf16"):
        t[f"gcost_{tag}"] = IN(big, np.uint16)
        t[f"gx_{tag}"], t[f"gy_{tag}"] = Spec(sm, np.uint16), Spec(sm, np.uint16)
    return t


def _cv_script(ctx):
    C, Dn, H, W = ctx.dims
    dims = (ctx.R, C, Dn, H, W)
    x, y, cost = ctx.input("x"), ctx.input("y"), ctx.output("cost")
    ctx.call("ganet_cost_volume_forward", x, y, cost, *dims)
    ctx.check("cost")
    ctx.unchanged("x", "y")
    ctx.free("cost", "x", "y")
    g, gx, gy = ctx.input("gcost"), ctx.output("gx"), ctx.output("gy")
    ctx.call("ganet_cost_volume_backward", g, gx, gy, *dims)
    ctx.check("gx", "gy")
    ctx.unchanged("gcost")
    ctx.free("gcost", "gx", "gy")


def _cv16_script(ctx):
    C, Dn, H, W = ctx.dims
    dims = (ctx.R, C, Dn, H, W)
    x, y, cost = ctx.input("x16"), ctx.input("y16"), ctx.output("cost16")
    ctx.call("ganet_cost_volume_forward_16", x, y, cost, *dims)
    ctx.check("cost16")
    ctx.unchanged("x16", "y16")
    ctx.free("cost16", "x16", "y16")
    for tag, fmt in (("f16", mc.F16), ("bf16", mc.BF16)):
        g, gx, gy = ctx.input(f"gcost_{tag}"), ctx.output(f"gx_{tag}"), ctx.output(f"gy_{tag}")
        ctx.call("ganet_cost_volume_backward_16", g, gx, gy, *dims, fmt)
        ctx.check(f"gx_{tag}", f"gy_{tag}")
        ctx.unchanged(f"gcost_{tag}")
        ctx.free(f"gcost_{tag}", f"gx_{tag}", f"gy_{tag}")


def _cast_data(case, nb):
    (E,) = case.dims
    rng = case.rng()
    a = rng.standard_normal((nb, E)).astype(F32)
    a[:, ::97] *= 1e-6                                       # fp16 subnormals
    a[:, 5::101] *= 1e6                                      # fp16 overflow
    return {"src32": a, "src16": rng.integers(0, 0x7C00, (nb, E)).astype(np.uint16) | (rng.integers(0, 2, (nb, E)).astype(np.uint16) << 15)}


def _cast_ref(case, inp):
    return {"dst_bf16": mc.convert(inp["src32"], mc.BF16), "dst_f16": mc.convert(inp["src32"], mc.F16), "dst32": mc.up(inp["src16"], mc.F16)}


def _cast_script(ctx):
    (E,) = ctx.dims
    n = mc.count_args(ctx.R * E)
    src = ctx.input("src32")
    for name, fmt in (("dst_bf16", mc.BF16), ("dst_f16", mc.F16)):
        dst = ctx.output(name)
        ctx.call("ganet_cast", src, dst, *n, mc.F32, fmt)
        ctx.check(name)
        ctx.free(name)
    ctx.unchanged("src32")
    ctx.free("src32")
    src, dst = ctx.input("src16"), ctx.output("dst32")
    ctx.call("ganet_cast", src, dst, *n, mc.F16, mc.F32)
    ctx.check("dst32")
    ctx.unchanged("src16")


# =================================================================================================================================
# streaming per-pixel ops (misc_kernels.h): bars of tests/misc_cases.py
# =================================================================================================================================
def _vol_data(case, nb):
    D, H, W = case.dims
    rng = case.rng()
    x = (5 * rng.standard_normal((nb, D, H, W))).astype(F32)
    import misc_ref64 as r64
    return {"x": x, "y32": r64.softmin(x).astype(F32), "gy": rng.standard_normal((nb, D, H, W)).astype(F32),
            "go": rng.standard_normal((nb, H, W)).astype(F32),
            "xd": (rng.integers(0, 1025, (nb, D, H, W)) / 1024.0).astype(F32), "god": (rng.integers(-1024, 1025, (nb, H, W)) / 1024.0).astype(F32)}


def _vol_tensors(D, H, W):
    E, HW = D * H * W, H * W
    return {"x": IN(E), "y32": IN(E), "gy": IN(E), "go": IN(HW), "xd": IN(E), "god": IN(HW),
            "y": Spec(E, kind=("close", 2e-6, 1e-7)), "gx": Spec(E, kind=("close", 1e-5, 1e-5)),
            "sr_out": Spec(HW, kind=("close", 1e-5, 1e-4)), "sr_mx": Spec(HW, kind="equal"), "sr_ss": Spec(HW, kind=None, role="ws"),
            "sr_gx": Spec(E, kind=("close", 1e-4, 1e-4)),
            "nr_out": Spec(HW, kind=("close", 1e-5, 1e-4)), "nr_sn": Spec(HW, kind=("close", 1e-5, 0.0)), "nr_gx": Spec(E, kind=("close", 1e-4, 1e-4)),
            "dr_out": Spec(HW, kind="equal"), "dr_gx": Spec(E, kind="equal")}


def _softmin_ref(case, inp):
    import misc_ref64 as r64
    nb = case.layout.nb
    return {"y": _flat(r64.softmin(inp["x"]), nb), "gx": _flat(r64.softmin_adjoint(inp["y32"], inp["gy"]), nb)}


def _softmin_script(ctx):
    D, H, W = ctx.dims
    dims = (ctx.R, D, H, W)
    x, y = ctx.input("x"), ctx.output("y")
    ctx.call("ganet_softmin_forward", x, y, *dims)
    ctx.check("y")
    ctx.unchanged("x")
    ctx.free("x", "y")
    y32, gy, gx = ctx.input("y32"), ctx.input("gy"), ctx.output("gx")
    ctx.call("ganet_softmin_backward", y32, gy, gx, *dims)
    ctx.check("gx")
    ctx.unchanged("y32", "gy")


def _reg_ref(case, inp):
    import misc_ref64 as r64
    nb = case.layout.nb
    x, go = inp["x"], inp["go"]
    nr_out, nr_sn = r64.norm_regression(x)
    assert not r64.l1_clamped(x, 1).any()
    want = r64.regression(inp["xd"])
    assert want.max() * 1024 < 2 ** 24
    return {"sr_out": _flat(r64.softmin_regression(x), nb), "sr_mx": _flat((-x.astype(F64)).max(1), nb),
            "sr_gx": _flat(r64.softmin_regression_adjoint(x, go), nb),
            "nr_out": _flat(nr_out, nb), "nr_sn": _flat(nr_sn, nb), "nr_gx": _flat(r64.norm_regression_adjoint(x, go), nb),
            "dr_out": _flat(want, nb), "dr_gx": _flat(r64.regression_adjoint(inp["god"], case.dims[0]), nb)}


def _reg_script(ctx):
    """the three regressions over one volume: softmin + regression, normalised regression, plain regression"""
    D, H, W = ctx.dims
    dims = (ctx.R, D, H, W)
    x, go = ctx.input("x"), ctx.input("go")
    out, mx, ss, gx = ctx.output("sr_out"), ctx.output("sr_mx"), ctx.output("sr_ss"), ctx.output("sr_gx")
    ctx.call("ganet_softmin_regression_forward", x, out, mx, ss, *dims)
    ctx.call("ganet_softmin_regression_backward", x, out, mx, ss, go, gx, *dims)
    ctx.check("sr_out", "sr_mx", "sr_ss", "sr_gx")
    ctx.free("sr_gx")
    out, sn, gx = ctx.output("nr_out"), ctx.output("nr_sn"), ctx.output("nr_gx")
    ctx.call("ganet_norm_disparity_regression_forward", x, out, sn, *dims)
    ctx.call("ganet_norm_disparity_regression_backward", x, out, sn, go, gx, *dims)
    ctx.check("nr_out", "nr_sn", "nr_gx")
    ctx.unchanged("x", "go")
    ctx.free("nr_gx", "x")
    xd, god, out, gx = ctx.input("xd"), ctx.input("god"), ctx.output("dr_out"), ctx.output("dr_gx")
    ctx.call("ganet_disparity_regression_forward", xd, out, *dims)
    ctx.call("ganet_disparity_regression_backward", god, gx, *dims)
    ctx.check("dr_out", "dr_gx")
    ctx.unchanged("xd", "god")


# ---- L1 normalise: fp32 and the mixed entries ---------------------------------------------------------------------------------
def _l1_case_parts(G, C, K, H, W, fmt):
    """x [N][G][C][K][H][W]; y_g [N][C][K][H][W]"""
    import mixed_train_cases as mtc
    import misc_ref64 as r64
    E, Eg = G * C * K * H * W, C * K * H * W

    def data(case, nb):
        rng = case.rng()
        x = rng.standard_normal((nb, G, C, K, H, W)).astype(F32)
        d = {"x": x, "x16": mc.convert(x, fmt)}
        for g in range(G):
            d[f"gy{g}"] = rng.standard_normal((nb, C, K, H, W)).astype(F32)
        return d

    def ref(case, inp):
        nb = case.layout.nb
        gys = np.stack([inp[f"gy{g}"] for g in range(G)], 1)
        xu = mc.up(inp["x16"], fmt).reshape(inp["x"].shape)
        y, yu = r64.l1_normalize(inp["x"], 3), r64.l1_normalize(xu, 3)
        assert not r64.l1_clamped(inp["x"], 3).any() and not r64.l1_clamped(xu, 3).any()
        gxu = r64.l1_normalize_adjoint(xu, gys, 3)
        w = {"gx": _flat(r64.l1_normalize_adjoint(inp["x"], gys, 3), nb), "gx16": _flat(gxu, nb),
             # the mixed backward is the fp32 backward's value rounded once to x's format: its bar plus half a unit in the last
             # place of that format (mixed_train_cases.half_ulp)
             "gx16/bar": _flat(1e-5 + 1e-4 * np.abs(gxu) + mtc.half_ulp(gxu, fmt), nb)}
        for g in range(G):
            w[f"y{g}"], w[f"ym{g}"] = _flat(y[:, g], nb), _flat(yu[:, g], nb)
        return w

    def script(ctx):
        dims = (ctx.R, G, C, K, H, W)
        x = ctx.input("x")
        ys = [ctx.output(f"y{g}") for g in range(G)] + [None] * (4 - G)
        ctx.call("ganet_l1_normalize_forward", x, *ys, *dims)
        ctx.check(*[f"y{g}" for g in range(G)])
        ctx.free(*[f"y{g}" for g in range(G)])
        gys = [ctx.input(f"gy{g}") for g in range(G)] + [None] * (4 - G)
        gx = ctx.output("gx")
        ctx.call("ganet_l1_normalize_backward", x, *gys, gx, *dims)
        ctx.check("gx")
        ctx.unchanged("x")
        ctx.free("gx", "x")
        x16 = ctx.input("x16")
        ys = [ctx.output(f"ym{g}") for g in range(G)] + [None] * (4 - G)
        ctx.call("ganet_l1_normalize_forward_mixed", x16, *ys, *dims, fmt)
        ctx.check(*[f"ym{g}" for g in range(G)])
        ctx.free(*[f"ym{g}" for g in range(G)])
        gx16 = ctx.output("gx16")
        ctx.call("ganet_l1_normalize_backward_mixed", x16, *gys, gx16, *dims, fmt)
        ctx.check("gx16")
        ctx.unchanged("x16", *[f"gy{g}" for g in range(G)])

    t = {"x": IN(E), "x16": IN(E, np.uint16), "gx": Spec(E, kind=("close", 1e-4, 1e-5)), "gx16": Spec(E, np.uint16, kind="bar", fmt=fmt)}
    for g in range(G):
        t[f"gy{g}"] = IN(Eg)
        t[f"y{g}"], t[f"ym{g}"] = Spec(Eg, kind=("close", 1e-5, 1e-6)), Spec(Eg, kind=("close", 1e-5, 1e-6))
    return t, data, ref, script


# ---- residual tail -------------------------------------------------------------------------------------------------------------
def _res_data(case, nb):
    C, D, H, W = case.dims
    rng = case.rng()
    dy = lambda shape: (rng.integers(-64, 65, shape) / 16.0).astype(F32)      # noqa: E731  (misc_cases._dyadic)
    return {"t": dy((nb, C, D, H, W)), "rem": dy((nb, C, D, H, W)), "gy": dy((nb, C, D, H, W))}


RES_SCALE, RES_SHIFT = np.array([0.5, -1.25, 2.0], F32), np.array([0.75, 0.0, -1.5], F32)


def _res_ref(case, inp):
    import misc_ref64 as r64
    nb = case.layout.nb
    y = r64.residual_relu(inp["t"], inp["rem"], RES_SCALE, RES_SHIFT)
    assert 0.2 < (y == 0).mean() < 0.8
    g_t, g_rem = r64.residual_relu_adjoint(y, inp["gy"], RES_SCALE)
    return {"y": _flat(y, nb), "g_t": _flat(g_t, nb), "g_rem": _flat(g_rem, nb)}


def _res_script(ctx):
    C, D, H, W = ctx.dims
    dims = (ctx.R, C, D, H, W)
    t, rem, y = ctx.input("t"), ctx.input("rem"), ctx.output("y")
    sc, sh = ctx.small("scale", RES_SCALE), ctx.small("shift", RES_SHIFT)
    ctx.call("ganet_residual_relu_forward", t, rem, sc, sh, y, *dims)
    ctx.check("y")
    ctx.unchanged("t", "rem")
    ctx.free("t", "rem")
    gy, g_t, g_rem = ctx.input("gy"), ctx.output("g_t"), ctx.output("g_rem")
    ctx.call("ganet_residual_relu_backward", y, gy, sc, g_t, g_rem, *dims)
    ctx.check("g_t", "g_rem")
    ctx.unchanged("gy")


def _res_tensors(C, D, H, W):
    E = C * D * H * W
    return {"t": IN(E), "rem": IN(E), "gy": IN(E), "y": Spec(E, kind="equal"), "g_t": Spec(E, kind="equal"), "g_rem": Spec(E, kind="equal")}


# ---- trilinear, and the fused tail -----------------------------------------------------------------------------------------------
def _tri_data(case, nb):
    isz, osz = case.dims[:3], case.dims[3:]
    rng = case.rng()
    return {"x": rng.standard_normal((nb,) + isz).astype(F32), "gy": rng.standard_normal((nb,) + osz).astype(F32)}


def _tri_ref(case, inp):
    import misc_cases
    nb = case.layout.nb
    y, gx = misc_cases._aten_trilinear(np.array(inp["x"][None]), np.array(inp["gy"][None]), case.dims[3:])     # ATen on the CPU: misc_cases' reference
    return {"y": _flat(y, nb), "gx": _flat(gx, nb)}


def _tri_script(ctx):
    x, y = ctx.input("x"), ctx.output("y")
    ctx.call("ganet_trilinear_upsample_forward", x, y, ctx.R, *ctx.dims)
    ctx.check("y")
    ctx.unchanged("x")
    ctx.free("x", "y")
    gy, gx = ctx.input("gy"), ctx.output("gx")
    ctx.call("ganet_trilinear_upsample_backward", gy, gx, ctx.R, *ctx.dims)
    ctx.check("gx")
    ctx.unchanged("gy")


def _tail_data(case, nb):
    Di, Hi, Wi, Do, Ho, Wo = case.dims
    rng = case.rng()
    return {"x": rng.standard_normal((nb, Di, Hi, Wi)).astype(F32), "go": rng.standard_normal((nb, Ho, Wo)).astype(F32)}


def _tail_ref(case, inp):
    import disp_tail_ref64 as ref
    nb = case.layout.nb
    st = ref.Statement(inp["x"], case.dims[3:], inp["go"])
    w = {}
    for q, v in st.results().items():
        w[q] = _flat(v, nb)
        w[q + "/bar"] = _flat(2 * st.bounds()[q], nb)            # disp_tail_cases: twice the first-order bound
    return w


def _tail_script(ctx):
    dims = (ctx.R,) + tuple(ctx.dims)
    x, go = ctx.input("x"), ctx.input("go")
    out, mx, ss, gc, gx = (ctx.output(n) for n in ("out", "mx", "ssum", "gc", "grad_x"))
    ctx.call("ganet_up_softmin_regression_forward", x, out, mx, ss, *dims)
    ctx.call("ganet_up_softmin_regression_backward", x, out, mx, ss, go, gc, gx, *dims)
    ctx.check("out", "mx", "ssum", "gc", "grad_x")
    ctx.unchanged("x", "go")


# =================================================================================================================================
# BatchNorm: statistics reduce over N -- every block is a permutation of ONE multiset per channel (mixed_train_cases' exact
# family: x = c0[c] + k / 4 with a symmetric set of k), so the replicated tensor's mean and variance are the block's exactly
# =================================================================================================================================
BN_C0 = np.array([1.0, -0.5, 2.0])
BN_W, BN_B = np.array([1.25, -0.75, 0.5], F32), np.array([0.3125, -0.4375, 0.1875], F32)
BN_RM, BN_RV = np.array([0.5, -1.0, 0.25], F32), np.array([1.5, 0.75, 1.0], F32)
BN_MOMENTUM, BN_EPS = 0.1, 1e-5


def _bn_data(case, nb):
    C, S = case.dims
    rng = case.rng()
    k = rng.integers(-8, 9, (C, S // 2))
    k = np.concatenate([k, -k] + ([np.zeros((C, 1), np.int64)] if S % 2 else []), axis=1)
    x = np.stack([BN_C0[:C, None] + rng.permuted(k, axis=1) / 4.0 for _ in range(nb)]).astype(F32)
    return {"x": x, "gy": (rng.integers(-4, 5, (nb, C, S)) / 8.0).astype(F32), "rem": (rng.integers(-4, 5, (nb, C, S)) / 2.0).astype(F32)}


class _BnRef:
    """bn_ref64.Reference on the distinct blocks, with every sum over the batch taken over the REPLICATED tensor: block b
    counts layout.count[b] times (the sums are of dyadic numbers: exact in float64 in any order)"""

    def __init__(self, case, inp, rem, relu):
        import bn_ref64
        C, S = case.dims
        cnt = case.layout.count.astype(F64)
        r = bn_ref64.Reference(inp["x"], inp["rem"] if rem else None, inp["gy"], BN_W[:C], BN_B[:C], BN_RM[:C], BN_RV[:C], BN_MOMENTUM, BN_EPS, relu)
        per_block = lambda a: a.sum(axis=2)                                                 # noqa: E731  [nb, C]
        M = F64(case.R * S)
        assert np.array_equal(per_block(r.x) / S, np.broadcast_to(r.mean, (case.layout.nb, C))), "a block's channel mean is off the grid"
        assert np.ptp(per_block(r.xm * r.xm), axis=0).max() == 0, "the blocks are not permutations of one multiset"
        assert not r.undecided().any(), "an element sits on the ReLU's kink"
        tot = lambda a: (cnt[:, None] * per_block(a)).sum(0)                                # noqa: E731
        r.M = case.R * S
        r.sum_g, r.sum_gxm = tot(r.g), tot(r.g * r.xm)
        r.sum_abs_g, r.sum_abs_gxm = tot(np.abs(r.g)), tot(np.abs(r.g * r.xm))
        r.grad_bias, r.grad_weight = r.sum_g, r.invstd * r.sum_gxm
        r.k1, r.q = r.sum_g / M, r.invstd ** 2 * r.sum_gxm / M
        b = lambda v: np.asarray(v)[None, :, None]                                          # noqa: E731
        r.grad_x = b(r.scale) * (r.g - b(r.k1) - r.xm * b(r.q))
        r.new_var = r.var * M / (M - 1.0)
        r.running_var = (1 - r.m) * r.old_var + r.m * r.new_var
        self.r = r


def _bn_ref(case, inp):
    import mixed_train_cases as mtc
    nb = case.layout.nb
    r = _BnRef(case, inp, True, True).r
    w = {"y": _flat(r.y, nb), "y/bar": _flat(r.bar_y(), nb), "gx": _flat(r.grad_x, nb), "gx/bar": _flat(r.bar_grad_x(), nb),
         "grem": _flat(r.g, nb), "_train": r}
    # the mixed twin at the tail site (x bf16, rem fp32, y / grad_y bf16): the same statement; a 16-bit store adds half a unit in
    # the last place of its format (mixed_train_cases.half_ulp) to the fp32 bar
    w["y16"], w["y16/bar"] = w["y"], _flat(r.bar_y() + mtc.half_ulp(r.y, mc.BF16), nb)
    w["gx16"], w["gx16/bar"] = w["gx"], _flat(r.bar_grad_x() + mtc.half_ulp(r.grad_x, mc.BF16), nb)
    w["grem16"] = w["grem"]
    # the eval form on dyadic parameters: exact
    import misc_ref64 as r64
    C, S = case.dims
    ya = r64.residual_relu(inp["x"][:, :, None, None, :], inp["rem"][:, :, None, None, :], RES_SCALE[:C], RES_SHIFT[:C])
    w["ya"] = _flat(ya, nb)
    w["ya16"] = _flat(mc.convert(ya.astype(F32), mc.BF16), nb)
    assert np.array_equal(mc.up(w["ya16"], mc.BF16).astype(F64).ravel(), ya.ravel()), "the eval form's result is not exact in bf16"
    return w


def _bn_small_checks(ctx, r, names):
    """statistics and parameter gradients against float64 at bn_cases' bars"""
    import bn_cases as bc
    sm, si, rm, rv, gw, gb = (ctx.host_small(n) for n in names)
    m = r.m
    rat = {"save_mean": bc.within("save_mean", sm, r.mean, 2.0 ** -23 * r.mean_abs_x, False),
           "save_invstd": bc.within("save_invstd", si, r.invstd, 2.0 ** -22 * r.invstd, False),
           "running_mean": bc.within("running_mean", rm, r.running_mean, 2.0 ** -22 * ((1 - m) * np.abs(r.old_mean) + m * np.abs(r.mean)), False),
           "running_var": bc.within("running_var", rv, r.running_var, 2.0 ** -22 * ((1 - m) * np.abs(r.old_var) + m * np.abs(r.new_var)), False),
           "grad_weight": bc.within("grad_weight", gw, r.grad_weight, 2.0 ** -22 * r.invstd * r.sum_abs_gxm, False),
           "grad_bias": bc.within("grad_bias", gb, r.grad_bias, 2.0 ** -22 * r.sum_abs_g, False)}
    assert np.array_equal(sm, r.mean.astype(F32)), "exact family: save_mean is the mean"
    ctx.checker.ratios.update({f"{names[0]}:{k}": v for k, v in rat.items()})


def _bn_script(ctx):
    import bn_cases as bc
    C, S = ctx.dims
    dims = (ctx.R, C, S)
    fb = bc.fbits
    x, rem = ctx.input("x"), ctx.input("rem")
    w, b = ctx.small("w", BN_W[:C]), ctx.small("b", BN_B[:C])
    nws = 1 if ctx.dry else ctx.query("ganet_bn_workspace", *dims)
    for tag, mixed in (("", False), ("16", True)):
        if mixed:
            ctx.free("x")
            x = ctx.input("x16")
        rm, rv = ctx.small("rm" + tag, BN_RM[:C], inout=True), ctx.small("rv" + tag, BN_RV[:C], inout=True)
        ws = ctx.small("ws" + tag, shape=(max(nws, 1),), dtype=F64)
        y, sm, si = ctx.output("y" + tag), ctx.small("sm" + tag, shape=(C,)), ctx.small("si" + tag, shape=(C,))
        types = (mc.BF16, mc.F32, mc.BF16) if mixed else ()
        ctx.call("ganet_bn_train_forward" + ("_mixed" if mixed else ""), x, rem, w, b, rm, rv, ws, y, sm, si, *dims, fb(BN_MOMENTUM), fb(BN_EPS), 1, *types)
        ctx.check("y" + tag)
        ctx.free("y" + tag)
        gy, gx, grem = ctx.input("gy" + tag), ctx.output("gx" + tag), ctx.output("grem" + tag)
        gw, gb = ctx.small("gw" + tag, shape=(C,)), ctx.small("gb" + tag, shape=(C,))
        ctx.call("ganet_bn_train_backward" + ("_mixed" if mixed else ""), x, rem, gy, w, b, sm, si, ws, gx, grem, gw, gb, *dims, 1, *types)
        ctx.check("gx" + tag, "grem" + tag)
        if not ctx.dry:
            _bn_small_checks(ctx, ctx.case.want["_train"], [n + tag for n in ("sm", "si", "rm", "rv", "gw", "gb")])
        ctx.unchanged("x" + tag, "gy" + tag)
        ctx.free("gy" + tag, "gx" + tag, "grem" + tag, "ws" + tag)
    # the eval form, fp32 and mixed (x bf16, no residual there: a 16-bit rem would have to be x's format)
    ctx.free("x16")
    x = ctx.input("x")
    sc, sh = ctx.small("scale", RES_SCALE[:C]), ctx.small("shift", RES_SHIFT[:C])
    ya = ctx.output("ya")
    ctx.call("ganet_bn_apply_forward", x, rem, sc, sh, ya, *dims, 1)
    ctx.check("ya")
    ctx.unchanged("x", "rem")
    ctx.free("ya", "x")
    x16, ya16 = ctx.input("x16"), ctx.output("ya16")
    ctx.call("ganet_bn_apply_forward_mixed", x16, rem, sc, sh, ya16, *dims, 1, mc.BF16, mc.F32, mc.BF16)
    ctx.check("ya16")
    ctx.unchanged("x16", "rem")


def _bn_data16(case, nb):
    d = _bn_data(case, nb)
    d["x16"], d["gy16"] = mc.convert(d["x"], mc.BF16), mc.convert(d["gy"], mc.BF16)
    assert np.array_equal(mc.up(d["x16"], mc.BF16).reshape(d["x"].shape), d["x"]) and np.array_equal(mc.up(d["gy16"], mc.BF16).reshape(d["gy"].shape), d["gy"])
    return d


def _bn_tensors(C, S):
    E = C * S
    return {"x": IN(E), "rem": IN(E), "gy": IN(E), "x16": IN(E, np.uint16), "gy16": IN(E, np.uint16),
            "y": Spec(E, kind="bar"), "gx": Spec(E, kind="bar"), "grem": Spec(E, kind="equal"),
            "y16": Spec(E, np.uint16, kind="bar", fmt=2), "gx16": Spec(E, np.uint16, kind="bar", fmt=2), "grem16": Spec(E, kind="equal"),
            "ya": Spec(E, kind="equal"), "ya16": Spec(E, np.uint16)}


# =================================================================================================================================
# DispConv: exact family of disp_conv_cases (x in 1/16, w in 1/8, grad_y in 1/8): y and grad_x EQUAL the float64 statement; the
# weight gradient sums over every slice -- per-workgroup partial sums are exact, the rows are added in fp64 and rounded once
# =================================================================================================================================
def _dc_data(case, nb):
    C, D, H, W = case.dims
    rng = case.rng()
    dy = lambda shape, bound, den: (rng.integers(-bound * den, bound * den + 1, shape) / float(den)).astype(F32)      # noqa: E731
    return {"x": dy((nb, C, D, H, W), 2, 16), "gy": dy((nb, D, H, W), 2, 8), "_w": dy((1, C, 3, 3, 3), 1, 8)}


def _dc_ref(case, inp):
    import disp_conv_ref64 as ref
    nb = case.layout.nb
    C, D, H, W = case.dims
    x64, g64, w64 = inp["x"].astype(F64), inp["gy"].astype(F64), inp["_w"].astype(F64).reshape(C, 3, 3, 3)
    assert 27 * C * 2 * 128 < 2 ** 24                                                      # disp_conv_cases.premises
    gw = sum(float(case.layout.count[b]) * ref.backward_weight(x64[b:b + 1], g64[b:b + 1]) for b in range(nb))
    assert np.abs(gw * 128).max() < 2 ** 53 and np.array_equal(gw * 128, np.round(gw * 128))   # multiples of 2^-7: the fp64 sum is exact
    return {"y": _flat(ref.forward(x64, w64), nb), "gx": _flat(ref.backward_data(g64, w64), nb), "_gw": gw.astype(F32)}


def _dc_script(ctx):
    C, D, H, W = ctx.dims
    dims = (ctx.R, C, D, H, W)
    x, y = ctx.input("x"), ctx.output("y")
    w = ctx.small("w", None if ctx.dry else ctx.case.inputs["_w"], shape=(1, C, 3, 3, 3))
    ctx.call("ganet_disp_conv_forward", x, w, y, *dims)
    ctx.check("y")
    ctx.free("y")
    gy = ctx.input("gy")
    n_ws = 27 * C * ctx.R * (-(-D // 8)) * (-(-(H * -(-W // 4)) // 64)) if ctx.dry else ctx.query("ganet_disp_conv_workspace", *dims)
    ws, gw = ctx.small("ws", shape=(n_ws,)), ctx.small("gw", shape=(C * 27,))
    ctx.call("ganet_disp_conv_backward_weight", x, gy, ws, gw, *dims)
    if not ctx.dry:
        got, want = ctx.host_small("gw").reshape(C, 3, 3, 3), ctx.case.want["_gw"]
        ctx.expect(np.array_equal(got, want), f"grad_weight: {int((got != want).sum())} of {got.size} differ from the float64 sum rounded once")
        ctx.expect(bool(ctx.torch.isfinite(ctx.smalls["ws"]).all().item()), "a workspace element was left unwritten")
    ctx.unchanged("x")
    ctx.free("x", "ws")
    gx = ctx.output("gx")
    ctx.call("ganet_disp_conv_backward_data", gy, w, gx, *dims)
    ctx.check("gx")
    ctx.unchanged("gy")


def _dc_tensors(C, D, H, W):
    return {"x": IN(C * D * H * W), "gy": IN(D * H * W), "y": Spec(D * H * W, kind="equal"), "gx": Spec(C * D * H * W, kind="equal")}


# =================================================================================================================================
# the table
# =================================================================================================================================
def _cases():
    cs = []
    sga_fb = ("ganet_sga_forward", "ganet_sga_backward")
    steps = ("ganet_sga_scan_forward_ws", "ganet_sga_backward_scan_ws", "ganet_sga_backward_point")
    # A_ws / G_ws [4][...] past 2^31 with x just past 2^29; tiled: W % 16 == 0 and H % 4 == 0
    cs.append(Case("sga-composite-tiled", "sga", sga_fb + steps, (33, 8, 48), _sga_tensors(33, 8, 48), "A", _sga_data, _sga_composite_ref,
                   _sga_composite(1, True)))
    cs.append(Case("sga-composite-api", "sga", sga_fb, (33, 7, 52), _sga_tensors(33, 7, 52), "A", _sga_data, _sga_composite_ref,
                   _sga_composite(0, False)))
    for tag, d in (("down-colblock", 0), ("right-rowwave", 2)):
        cs.append(Case(f"sga-scan-{tag}", "sga", ("ganet_sga_scan_forward", "ganet_sga_backward_scan"), (33, 20, 52), _scan_tensors(33, 20, 52),
                       "x", _scan_data, _scan_ref(d), _scan_script(d), seed=d))
    E = 33 * 20 * 52
    cs.append(Case("sga-merge", "sga", ("ganet_sga_merge",), (33, 20, 52),
                   {"A": IN(E, lead=4), "out": Spec(E), "mask": Spec(E, np.uint8), "kp": Spec(20 * 52, np.uint16, lead=4)}, "A",
                   _merge_data, _merge_ref, _merge_script))
    t = {k: v for k, v in _sga_tensors(33, 20, 52).items() if k in ("x", "g0", "g1", "g2", "g3", "out")}
    cs.append(Case("sga-infer-fused", "sga", ("ganet_sga_forward_infer",), (33, 20, 52), t, "out", _sga_data, _infer_ref, _infer_script))
    t = dict(t, tmp=Spec(E), maskf=Spec(E))
    cs.append(Case("sga-compat-forward", "sga", ("ganet_sga_forward_compat",), (33, 20, 52), t, "out", _sga_data, _compat_ref, _compat_script))
    # LGA: D well above 75 keeps the filters small
    lt = _lga_tensors(160, 12, 20)
    cs.append(Case("lga-api", "lga", ("ganet_lga_forward", "ganet_lga_backward"), (160, 12, 20),
                   {k: lt[k] for k in ("x", "f", "gy", "y", "gx", "gf")}, "x", _lga_data, _lga_ref, _lga_script))
    cs.append(Case("lga2-paired", "lga", ("ganet_lga_apply_paired_edges", "ganet_lga_apply_paired", "ganet_lga_filter_grad_paired"), (160, 12, 20),
                   lt, "x", _lga_data, _lga2_ref, _lga2_script))
    cv = _cv_tensors(2, 14, 12, 52)
    cs.append(Case("costvol", "misc", ("ganet_cost_volume_forward", "ganet_cost_volume_backward"), (2, 14, 12, 52),
                   {k: cv[k] for k in ("x", "y", "gcost", "cost", "gx", "gy")}, "cost", _cv_data, _cv_ref, _cv_script))
    cs.append(Case("costvol-16", "mixed", ("ganet_cost_volume_forward_16", "ganet_cost_volume_backward_16"), (2, 14, 12, 52),
                   {k: v for k, v in cv.items() if "16" in k}, "cost16", _cv_data, _cv_ref, _cv16_script))
    cs.append(Case("cast", "mixed", ("ganet_cast",), (34321,),
                   {"src32": IN(34321), "src16": IN(34321, np.uint16), "dst_bf16": Spec(34321, np.uint16), "dst_f16": Spec(34321, np.uint16),
                    "dst32": Spec(34321)}, "src32", _cast_data, _cast_ref, _cast_script))
    # streaming ops: H * W % 4 == 0 takes the 16-byte form, 19 x 55 the scalar one
    for tag, dims in (("vec4", (33, 20, 52)), ("scalar", (33, 19, 55))):
        vt = _vol_tensors(*dims)
        cs.append(Case(f"softmin-{tag}", "misc", ("ganet_softmin_forward", "ganet_softmin_backward"), dims,
                       {k: vt[k] for k in ("x", "y32", "gy", "y", "gx")}, "x", _vol_data, _softmin_ref, _softmin_script))
    vt = _vol_tensors(33, 20, 52)
    cs.append(Case("regressions-vec4", "misc", ("ganet_softmin_regression_forward", "ganet_softmin_regression_backward",
                                               "ganet_norm_disparity_regression_forward", "ganet_norm_disparity_regression_backward",
                                               "ganet_disparity_regression_forward", "ganet_disparity_regression_backward"), (33, 20, 52),
                   {k: v for k, v in vt.items() if k not in ("y32", "gy", "y", "gx")}, "x", _vol_data, _reg_ref, _reg_script))
    l1_entries = ("ganet_l1_normalize_forward", "ganet_l1_normalize_backward", "ganet_l1_normalize_forward_mixed", "ganet_l1_normalize_backward_mixed")
    for name, (G, C, K, H, W), fmt in (("l1norm-K5-G4-vec8", (4, 2, 5, 12, 72), mc.F16), ("l1norm-K75-G1-scalar", (1, 1, 75, 12, 41), mc.BF16)):
        t, data, ref, script = _l1_case_parts(G, C, K, H, W, fmt)
        cs.append(Case(name, "misc", l1_entries, (G, C, K, H, W), t, "x", data, ref, script))
    for tag, dims in (("vec4", (3, 11, 20, 52)), ("scalar", (3, 11, 19, 55))):
        cs.append(Case(f"residual-{tag}", "misc", ("ganet_residual_relu_forward", "ganet_residual_relu_backward"), dims, _res_tensors(*dims), "y",
                       _res_data, _res_ref, _res_script))
    cs.append(Case("trilinear", "misc", ("ganet_trilinear_upsample_forward", "ganet_trilinear_upsample_backward"), (6, 12, 18, 17, 36, 54),
                   {"x": IN(6 * 12 * 18), "gy": IN(17 * 36 * 54), "y": Spec(17 * 36 * 54, kind=("close", 1e-5, 1e-6)),
                    "gx": Spec(6 * 12 * 18, kind=("close", 1e-5, 1e-5))}, "y", _tri_data, _tri_ref, _tri_script))
    Di, Hi, Wi, Do, Ho, Wo = 17, 30, 66, 49, 33, 60           # Ho Wo == Hi Wi: the column workspace is as large as x
    cs.append(Case("up-softmin-regression", "disp_tail", ("ganet_up_softmin_regression_forward", "ganet_up_softmin_regression_backward"),
                   (Di, Hi, Wi, Do, Ho, Wo),
                   {"x": IN(Di * Hi * Wi), "go": IN(Ho * Wo), "out": Spec(Ho * Wo, kind="bar"), "mx": Spec(Ho * Wo, kind="bar"),
                    "ssum": Spec(Ho * Wo, kind="bar"), "gc": Spec(Di * Ho * Wo, kind="bar", role="ws"), "grad_x": Spec(Di * Hi * Wi, kind="bar")},
                   "x", _tail_data, _tail_ref, _tail_script))
    cs.append(Case("batchnorm", "bn", ("ganet_bn_train_forward", "ganet_bn_train_backward", "ganet_bn_apply_forward", "ganet_bn_train_forward_mixed",
                                       "ganet_bn_train_backward_mixed", "ganet_bn_apply_forward_mixed"), (3, 11440), _bn_tensors(3, 11440), "x",
                   _bn_data16, _bn_ref, _bn_script))
    cs.append(Case("disp-conv", "disp_conv", ("ganet_disp_conv_forward", "ganet_disp_conv_backward_data", "ganet_disp_conv_backward_weight"),
                   (32, 9, 10, 12), _dc_tensors(32, 9, 10, 12), "x", _dc_data, _dc_ref, _dc_script))
    return cs


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# every exported entry that no case calls, with the reason
NOT_APPLICABLE = {
    "ganet_disparity_loss_forward": "refuses N*H*W >= 2^24 pixels (ganet_capi.hip: 'counts are reported as floats, which holds below 2^24')",
    "ganet_disparity_loss_backward": "refuses N*H*W >= 2^24 pixels (ganet_capi.hip: '2^24 pixels or more')",
    "ganet_stereo_input_stats": "refuses H*W > 2^24 (include/ganet_hip.h: 'CP other than 3 | 4, H W > 2^24 ...: GANET_E_INVALID')",
    "ganet_stereo_input_apply": "refuses H*W > 2^24 (the same line)",
    "ganet_window_f32": "one image plane: below 2^28 pixels (the image front and back end)",
    "ganet_disparity_to_u16": "one image plane: below 2^28 pixels (the image front and back end)",
    "ganet_sga_backward_compat": "NOT COVERED, no refusal: the reference buffer contract's backward takes six volume-sized buffers and eight "
                                 "guidance-sized ones, 62 GB past 2^31 elements -- beyond the 48 GiB cap (its forward is sga-compat-forward)",
    "ganet_sga_backward_dir": "NOT COVERED, no refusal: adjoint scan + per-pixel kernel of ONE direction: both run in the table (ganet_sga_backward_scan past 2^31, the "
                              "per-pixel kernel through ganet_sga_backward_point); seven volume-sized buffers past 2^31 are 60 GB, beyond the cap",
    "ganet_lga_forward_regress": "NOT COVERED, no refusal: its op-level bars (tests/test_sim_fused.py: sdy within 2e-4 + 1e-5 |want|) are stated "
                                 "for D <= 31; at the D = 160 that keeps this table's filters small, sum_d d * y multiplies y's rounding by "
                                 "up to 12720, and tests/model_calls.py's check_lga_regress is a model-scale checker with planted kinks -- "
                                 "no existing bar applies.  Its volume pass is lga_apply_pp's, which lga-api and lga2-paired run",
    "ganet_abi_version": "no tensor", "ganet_last_error": "no tensor", "ganet_is_simulator": "no tensor",
    "ganet_set_option": "no tensor", "ganet_get_option": "no tensor",
    "ganet_sga_workspace_layout": "a query (asserted by the SGA cases)", "ganet_sga_forward_infer_scratch": "a query (asserted by sga-infer-fused)",
    "ganet_disp_conv_workspace": "a query (sizes disp-conv's workspace)", "ganet_bn_workspace": "a query (sizes batchnorm's workspace)",
    "ganet_disparity_loss_workspace": "a query", "ganet_stereo_input_workspace": "a query",
    "ganet_selftest_dpp": "a 64-lane probe", "ganet_selftest_dpp_wave": "a 64-lane probe",
}

# size refusals of ganet_capi.hip that no test can reach below 1 GB of operands (the reachable ones: tests/test_gpu_large_offsets.py)
UNREACHABLE_REFUSALS = {
    "H*W >= 2^28 (LGA paired / regress entries)": "one plane of 2^28 floats is 1 GiB by itself, and D planes of it are needed",
    "items >= 2^31 (ganet_lga_apply_paired / _filter_grad_paired: too many tiles)": "2^31 tiles of 32 x 2 pixels are 2^37 pixels",
    "check_dims5 (D*H*W > 2^29, N*C*H or N*C*W > 2^31)": "a slice of 2^29 floats is 2 GiB; 2^31 scanlines need as many elements",
}


def exported_entries():
    """every `int ganet_*(` / `const char *ganet_*(` of include/ganet_hip.h"""
    with open(HEADER) as fh:
        text = fh.read()
    return sorted(set(re.findall(r"^(?:int|const char \*)\s*(ganet_\w+)\(", text, re.M)))
