"""The machinery of tests/large_cases.py on the CPU (never skipped): the table's own premises, and the checker's teeth on a numpy
MODEL of two ops over a virtual replicated tensor whose offsets are computed in Python integers -- accepted as it is, rejected
once those offsets are wrapped to int32 elements, to uint32 bytes or to int32 bytes, or once the last slice is left unwritten.
This is the only place where a wrong offset is ever produced: no truncated kernel is built or run on the device (there a
wrapped offset is an out-of-bounds access)."""
import math

import numpy as np
import pytest

import large_cases as lc


# ---- the table ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lc.CASES, ids=repr)
def test_case_premises(case):
    spec = case.tensors[case.anchor]
    total = spec.lead * case.R * spec.per
    assert total == case.largest(), "the anchor is the largest operand"
    assert (1 << 31) < total <= (1 << 31) + spec.lead * spec.per, (case.name, total - (1 << 31))
    assert case.R <= lc.MAX_SLICES, "S / B above 65535 changes the kernel family (and LGA refuses it)"
    assert case.layout.nb <= lc.P + 4 and lc.P % 2 == 1
    assert all(s.per & (s.per - 1) for s in case.tensors.values()), "a slice size that is a power of two"
    assert np.array_equal(np.sort(np.unique(case.layout.block_of)), np.arange(case.layout.nb))
    assert case.peak <= lc.CAP_BYTES, (case.name, case.peak)
    dry = lc.DryCtx(case)
    case.script(dry)
    assert set(dry.called) == set(case.entries), sorted(set(dry.called) ^ set(case.entries))
    for name, s in case.tensors.items():                       # every input has data, every compared output a reference
        if s.role == "in":
            assert case.inputs[name].dtype == s.dtype and case.inputs[name].size == case.layout.nb * s.lead * s.per, name
        elif s.kind is not None:
            assert np.asarray(case.want[name]).size == case.layout.nb * s.lead * s.per, name
            assert np.isfinite(np.asarray(case.want[name], np.float64)).all() or s.dtype != np.float32, name
            assert (s.kind == "bar") == (name + "/bar" in case.want), name


@pytest.mark.parametrize("case", lc.CASES, ids=repr)
def test_wrapped_offsets_land_on_other_values(case):
    """the teeth of the arrangement: index arithmetic and reference values only"""
    assert lc.assert_teeth(case) >= 4


def test_teeth_assertion_notices_a_blind_arrangement():
    """the same layout over a pool whose blocks are all alike: no wrap can show, and the assertion says so"""
    from types import SimpleNamespace
    case = lc.BY_NAME["cast"]
    blind = SimpleNamespace(name="blind", tensors={"src32": case.tensors["src32"]}, layout=case.layout, want={},
                            inputs={"src32": np.broadcast_to(case.inputs["src32"][:1, :1], case.inputs["src32"].shape)})
    with pytest.raises(AssertionError, match="invisible"):
        lc.assert_teeth(blind)


def test_every_exported_entry_is_in_the_table_or_named_not_applicable():
    exported = set(lc.exported_entries())
    assert len(exported) > 60 and "ganet_sga_forward" in exported and "ganet_last_error" in exported
    from ganet_amd import _native
    assert exported == set(_native.EXPORTS), sorted(exported ^ set(_native.EXPORTS))
    covered = set(e for c in lc.CASES for e in c.entries)
    assert covered <= exported, sorted(covered - exported)
    assert not covered & set(lc.NOT_APPLICABLE), sorted(covered & set(lc.NOT_APPLICABLE))
    assert set(lc.NOT_APPLICABLE) <= exported, sorted(set(lc.NOT_APPLICABLE) - exported)
    unaccounted = exported - covered - set(lc.NOT_APPLICABLE)
    assert not unaccounted, f"entries that are neither in large_cases.CASES nor in NOT_APPLICABLE: {sorted(unaccounted)}"
    assert all(len(reason) > 5 for reason in lc.NOT_APPLICABLE.values())


def test_ratio_of_kinds():
    a = np.array([1.0, 2.0, -0.0], np.float32)
    assert lc.ratio_of(a, a.astype(np.float64), "bits") == 0 and lc.ratio_of(a, np.array([1.0, 2.0, 0.0]), "bits") == math.inf
    assert lc.ratio_of(a, np.array([1.0, 2.0, 0.0]), "equal") == 0
    assert lc.ratio_of(a, a + 1e-4, ("abs", 2e-4)) == pytest.approx(0.5, rel=1e-3)
    assert lc.ratio_of(np.array([np.nan], np.float32), np.array([0.0]), ("abs", 1.0)) == math.inf
    assert lc.ratio_of(np.array([np.nan], np.float32), np.array([0.0]), "equal") == math.inf
    assert lc.ratio_of(a, a, "bar", np.zeros(3)) == 0 and lc.ratio_of(a, a + 1e-3, "bar", np.zeros(3)) == math.inf


# ---- a numpy model of two ops over a virtual replicated tensor ------------------------------------------------------------------
M32 = (1 << 32) - 1


def _int32_elements(i, b):
    return ((i + (1 << 31)) & M32) - (1 << 31)


def _uint32_bytes(i, b):
    return ((i * b) & M32) // b


def _int32_bytes(i, b):
    t = (((i * b) + (1 << 31)) & M32) - (1 << 31)
    return np.where(t < 0, -1, t // b)


# (name, the offset a kernel with that truncation computes for the true element offset i -- negative: outside the tensor --,
#  the first element whose offset is wrong, the period of the wrap in elements)
CORRECT = ("exact 64-bit offsets", lambda i, b: i, lambda b: None, lambda b: None)
WRAPS = [("int32 elements", _int32_elements, lambda b: 1 << 31, lambda b: 1 << 32),
         ("uint32 bytes", _uint32_bytes, lambda b: (1 << 32) // b, lambda b: (1 << 32) // b),
         ("int32 bytes", _int32_bytes, lambda b: (1 << 31) // b, lambda b: (1 << 32) // b)]


def gather(values, spec, lay, idx, outside):
    """elements idx of the virtual tensor [lead][R][per] whose slice k holds values[block_of[k]]; `outside` where idx is not
    inside the tensor (foreign memory)"""
    total = spec.lead * lay.R * spec.per
    ok = (idx >= 0) & (idx < total)
    i = np.where(ok, idx, 0)
    q, e = i // spec.per, i % spec.per
    v = values.reshape(lay.nb, spec.lead * spec.per)[lay.block_of[q % lay.R], (q // lay.R) * spec.per + e]
    return np.where(ok, v, outside)


class ModelStore:
    """What large_cases.Checker reads, for a model whose arithmetic is right and whose offsets are `wrap`ped: slices that the
    truncation cannot touch are the correct values by construction (compared by identity: one block array per distinct
    block); the slices it can touch, the special slices, their neighbours and a seeded sample are evaluated element by
    element."""

    def __init__(self, case, out_name, kind, unwritten_tail=False):
        self.case, self.out, self.tail = case, out_name, unwritten_tail
        spec = case.tensors[out_name]
        _, fn, thr, period = kind
        self.wrap = lambda i: fn(i, spec.itemsize)
        self.thr, self.period = thr(spec.itemsize), period(spec.itemsize)
        self.total = spec.lead * case.R * spec.per

    # -- the two models --
    def _slice(self, spec, k):
        raise NotImplementedError

    def host(self, name, l, k):
        assert name == self.out and l == 0
        spec = self.case.tensors[name]
        a = self._slice(spec, k)
        if self.tail and k == self.case.R - 1:
            a = np.full_like(a, np.nan)
        return a

    def touched(self, spec):
        """slices a wrapped access can reach: where offsets wrap, and where wrapped accesses land"""
        if self.thr is None:
            return set()
        s = set(range(self.thr // spec.per, self.case.R))
        if self.period < self.total:
            s |= set(range(0, (self.total - self.period) // spec.per + 1))
        return s

    def worst_to_representative(self, name, spec, lay):
        rng = np.random.default_rng(5)
        look = set(lay.special) | {k + d for k in lay.special for d in (-1, 1) if 0 <= k + d < lay.R} | set(rng.integers(0, lay.R, 48).tolist())
        touched = self.touched(spec)
        worst = 0.0
        for k in sorted(touched, reverse=True) + sorted(look - touched):      # (where offsets wrap first: the first difference settles it)
            got, rep = self.host(name, 0, k), self.host(name, 0, int(lay.first[lay.block_of[k]]))
            if not np.array_equal(got, rep):
                return math.inf                            # (the first differing slice settles it; a NaN differs from itself)
        return worst


class CostVolumeModel(ModelStore):
    """writes wrapped: the element computed for true offset i is stored at wrap(i); x and y are small and read correctly"""

    def _slice(self, spec, k):
        lay = self.case.layout
        comp = np.asarray(self.case.want[self.out], np.float32)
        j = np.arange(k * spec.per, (k + 1) * spec.per, dtype=np.int64)
        if self.thr is None:
            return gather(comp, spec, lay, j, np.nan)
        out = np.where(self.wrap(j) == j, gather(comp, spec, lay, j, np.nan), np.float32(np.nan))       # the others' stores went elsewhere
        for m in (1, 2):                                                                               # wrapped stores that landed here, the later one last
            src = j + m * self.period
            lands = (src < self.total) & (self.wrap(np.minimum(src, self.total - 1)) == j)
            out = np.where(lands, gather(comp, spec, lay, src, np.nan), out)
        return out.astype(np.float32)


class SoftminModel(ModelStore):
    """reads wrapped: y[q, d, p] = softmin over d' of x at wrap(offset of (q, d', p)); a negative offset reads foreign memory
    (zeros); the output is written where it belongs"""

    def _slice(self, spec, k):
        import misc_ref64 as r64
        lay, case = self.case.layout, self.case
        D, H, W = case.dims
        if self.thr is None or (k + 1) * spec.per <= self.thr:
            return np.asarray(case.want[self.out], np.float32)[lay.block_of[k]]
        idx = self.wrap(np.arange(k * spec.per, (k + 1) * spec.per, dtype=np.int64))
        x = gather(case.inputs["x"], case.tensors["x"], lay, idx, np.float32(0)).reshape(1, D, H, W)
        return r64.softmin(x).astype(np.float32).ravel()


MODELS = {"costvol": (CostVolumeModel, "cost"), "softmin-vec4": (SoftminModel, "y")}


@pytest.mark.parametrize("case_name", sorted(MODELS))
def test_checker_accepts_the_model_with_exact_offsets(case_name):
    case = lc.BY_NAME[case_name]
    model, out = MODELS[case_name]
    checker = lc.Checker(case, model(case, out, CORRECT))
    assert checker.check(out) <= 1.0


@pytest.mark.parametrize("kind", WRAPS, ids=lambda k: k[0].replace(" ", "-"))
@pytest.mark.parametrize("case_name", sorted(MODELS))
def test_checker_rejects_wrapped_offsets(case_name, kind):
    case = lc.BY_NAME[case_name]
    model, out = MODELS[case_name]
    store = model(case, out, kind)
    spec = case.tensors[out]
    assert store.thr < store.total, "the tensor is large enough for this truncation to matter"
    with pytest.raises(AssertionError):
        lc.Checker(case, store).check(out)
    # (a) and (b) each notice on their own: a representative's comparison with the reference, and a slice's with its representative
    special_hit = [k for k in case.layout.special if (k + 1) * spec.per > store.thr]
    assert special_hit, "a special slice lies where offsets wrap"
    k = special_hit[0]
    b = case.layout.block_of[k]
    assert lc.ratio_of(store.host(out, 0, k), case.want[out][b], spec.kind) > 1.0
    # (b) notices wherever a slice that is not its own representative is touched; the last slice, the only one an int32 element
    # index reaches, is its own representative -- which is why it holds a block of its own and goes to the host
    ordinary = [k for k in store.touched(spec) if k * spec.per >= store.thr and k not in case.layout.special]
    assert not ordinary or store.worst_to_representative(out, spec, case.layout) == math.inf
    assert ordinary or kind[0] == "int32 elements"


@pytest.mark.parametrize("case_name", sorted(MODELS))
def test_checker_rejects_an_unwritten_last_slice(case_name):
    case = lc.BY_NAME[case_name]
    model, out = MODELS[case_name]
    with pytest.raises(AssertionError, match="block"):
        lc.Checker(case, model(case, out, CORRECT, unwritten_tail=True)).check(out)


def test_model_offsets_against_python_integers():
    """the three truncations against Python's own integers, around every threshold"""
    pts = [0, 1, (1 << 29) - 1, 1 << 29, (1 << 30) - 1, 1 << 30, (1 << 30) + 5, (1 << 30) + (1 << 29), (1 << 31) - 1, 1 << 31, (1 << 31) + 7]
    for name, fn, thr, period in WRAPS:
        for b in (2, 4):
            got = fn(np.array(pts, np.int64), b).tolist()
            for v, g in zip(pts, got):
                scale = 1 if name.endswith("elements") else b
                t = (v * scale) % (1 << 32)
                if name.startswith("int32") and t >= 1 << 31:
                    t -= 1 << 32
                assert (g < 0 and t < 0) or (t >= 0 and g == t // scale), (name, b, v, g, t)
                assert (g == v) == (v < thr(b)) or v >= thr(b), (name, b, v)
            assert fn(np.array([thr(b) - 1, thr(b)], np.int64), b).tolist()[0] == thr(b) - 1 and fn(np.array([thr(b)], np.int64), b)[0] != thr(b)
