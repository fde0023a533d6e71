"""The autograd layer as a training loop drives it: every entry of tests/autograd_cases.py (one per op and host path of
ganet_amd/functions/GANet.py, functions/fused.py, modules/fused.py) under every property below.

The ANCHOR of a case is the plain call -- contiguous tensors, every input requiring grad, torch.autograd.grad(out, inputs, go),
current stream -- computed once per case and shared.  Property A holds it to the case's yardstick (equality on the exact
families, otherwise the bar the op already has); B .. I then ask for the anchor's BITS: the kernels use no atomics, and the
exact families make scalar twins, realigned copies and the inference path return the same values.

  A  anchor against the reference
  B  backward twice (retain_graph), scratch-sized NaN allocations in between; saved tensors untouched
  C  awkward incoming gradients: stride-0 expanded, permuted view, contiguous slice 4 bytes into a buffer; never written
  D  partial requires_grad: each input alone, all but one, none (== no_grad)
  E  inputs are not written; inplace=True: t is the output, its version rose, rem unchanged
  F  accumulation into .grad: two backward() calls give exactly 2 x the anchor
  G  stream ordering: inputs become valid only on a busy side stream
  H  graph capture of forward + autograd.grad, replayed on new data
  I  one DisparityLoss instance serving several calls before their backwards run"""
import numpy as np
import pytest

import autograd_cases as ac
import loss_cases as lc

pytestmark = pytest.mark.gpu

DEVICE = "cuda"
# torch.cuda._sleep spins for this many ticks of the device's cycle counter.  Measured once on an MI355X with events around
# the call: _sleep(20_000_000) = 8.36 ms, _sleep(5_000_000) = 2.09 ms (0.418 ns per tick), so this is 50 ms -- against well
# under 2 ms that the host side of the longest case (SGA: five copies, forward, five-input backward) takes to return
SLEEP_TICKS = 120_000_000
CASES = pytest.mark.parametrize("case", ac.CASES, ids=repr)


@pytest.fixture(scope="module")
def torch_mod(port_oracle):
    import torch
    from ganet_amd import _native
    assert torch.cuda.is_available()
    lib = _native.lib()
    assert not lib.is_simulator, "GPU tests must run the gfx950 build"
    for c in ac.CASES:
        if isinstance(c, ac.Sga):
            c.oracle = port_oracle
    return torch


@pytest.fixture(scope="module", autouse=True)
def leave_no_trace():
    """These tests fill freed device memory with NaN on purpose (poison(), property G) and keep anchors, graphs' pools and
    side-stream blocks in the caching allocator.  Hand all of it back when the module is done, so that the files that run
    after this one meet the allocator they met before it existed."""
    yield
    import torch
    _ANCHORS.clear()
    for c in ac.CASES:
        if isinstance(c, ac.Loss):
            c.module = None
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def _np(t):
    return t.detach().cpu().numpy()


def same(torch, a, b):
    """the same dtype, shape and bits"""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return torch.equal(a.detach().contiguous().reshape(-1).view(torch.uint8), b.detach().contiguous().reshape(-1).view(torch.uint8))


class Run:
    def __init__(self, data, ins, consts, gos, outs, grads):
        self.data, self.ins, self.consts, self.gos, self.outs, self.grads = data, ins, consts, gos, outs, grads


def tensors(torch, data, requires=None):
    requires = [True] * len(data.inputs) if requires is None else requires
    ins = [torch.from_numpy(a).to(DEVICE).requires_grad_(bool(r)) for a, r in zip(data.inputs, requires)]
    return ins, [torch.from_numpy(a).to(DEVICE) for a in data.consts], [torch.from_numpy(g).to(DEVICE) for g in data.go]


def run(torch, case, data, requires=None, gos=None, grad_mode=True):
    """forward and torch.autograd.grad for the inputs that require grad -> Run (grads: one per input, None if not asked for)"""
    requires = [True] * len(data.inputs) if requires is None else list(requires)
    with case.environ(), torch.set_grad_enabled(grad_mode):
        ins, consts, own_gos = tensors(torch, data, requires)
        gos = own_gos if gos is None else gos
        outs = case.apply(torch, ins, consts)
        wanted = [t for t, r in zip(ins, requires) if r] if grad_mode else []
        got = iter(torch.autograd.grad(outs[:case.ndiff], wanted, gos) if wanted else ())
        grads = [next(got) if (r and grad_mode) else None for r in requires]
    return Run(data, ins, consts, gos, outs, grads)


_ANCHORS = {}


def anchor(torch, case):
    if case.id not in _ANCHORS:
        _ANCHORS[case.id] = run(torch, case, case.make())
    return _ANCHORS[case.id]


def assert_same_run(torch, got, want, what, outs=True):
    if outs:
        assert len(got.outs) == len(want.outs)
        for k, (a, b) in enumerate(zip(got.outs, want.outs)):
            assert same(torch, a, b), f"{what}: output {k} differs from the anchor"
    for k, (a, b) in enumerate(zip(got.grads, want.grads)):
        if a is not None:
            assert same(torch, a, b), f"{what}: gradient of input {k} differs from the anchor"


def function_node(out):
    """the custom Function's node (= its ctx) behind an output"""
    fn = out.grad_fn
    while fn is not None and not hasattr(fn, "saved_tensors"):
        fn = fn.next_functions[0][0]
    assert fn is not None
    return fn


def poison(torch, like):
    """allocate and free NaN-filled (0xFF for integer) tensors of the sizes in play, so that the next torch.empty of such a
    size starts out poisoned: a kernel that counts on what its scratch or its output held before shows"""
    sizes = sorted({t.numel() * t.element_size() for t in like} | {4 * like[0].numel() * like[0].element_size()})
    held = [torch.full(((n + 3) // 4,), float("nan"), device=DEVICE) for n in sizes for _ in range(3)]
    del held


# ---- A ---------------------------------------------------------------------------------------------------------------------------
@CASES
def test_a_anchor_against_reference(torch_mod, case):
    a = anchor(torch_mod, case)
    assert all(g is not None for g in a.grads) and all(o.requires_grad for o in a.outs[:case.ndiff])
    case.check(a.data, [_np(o) for o in a.outs], [_np(g) for g in a.grads])


# ---- B ---------------------------------------------------------------------------------------------------------------------------
@CASES
def test_b_backward_twice(torch_mod, case):
    """the context must be re-entrant: a backward may not use what forward saved as scratch, nor count on its own scratch"""
    torch = torch_mod
    a = anchor(torch, case)
    with case.environ():
        ins, consts, gos = tensors(torch, a.data)
        outs = case.apply(torch, ins, consts)
        ctx = function_node(outs[0])
        saved = [t.clone() for t in ctx.saved_tensors]
        for k in (1, 2):
            grads = torch.autograd.grad(outs[:case.ndiff], ins, gos, retain_graph=True)
            assert_same_run(torch, Run(a.data, ins, consts, gos, outs, list(grads)), a, f"backward {k}")
            now = ctx.saved_tensors
            assert len(now) == len(saved) and all(same(torch, s, t) for s, t in zip(now, saved)), f"backward {k} wrote a saved tensor"
            poison(torch, ins + list(outs) + saved)


# ---- C ---------------------------------------------------------------------------------------------------------------------------
def _expanded(torch, g):
    return torch.ones((), device=g.device).expand(g.shape)        # what out.sum().backward() delivers


def _permuted(torch, g):
    if g.dim() < 2:
        return g.clone()
    v = g.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert v.is_contiguous() == (min(g.shape[-2:]) == 1)
    return v


def _offset(torch, g):
    buf = torch.empty(g.numel() + 1, device=g.device)
    v = buf[1:].view(g.shape)
    v.copy_(g)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@CASES
@pytest.mark.parametrize("form", ["expanded", "permuted", "offset"])
def test_c_awkward_incoming_gradient(torch_mod, case, form):
    """(a 0-d gradient -- the loss -- has no non-contiguous form: its `permuted` is a fresh tensor of the same value)"""
    torch = torch_mod
    a = anchor(torch, case)
    gos = [{"expanded": _expanded, "permuted": _permuted, "offset": _offset}[form](torch, g) for g in a.gos]
    keep = [g.clone() for g in gos]
    want = a if form != "expanded" else run(torch, case, a.data, gos=[g.contiguous() for g in gos])
    got = run(torch, case, a.data, gos=gos)
    assert_same_run(torch, got, want, form)
    assert all(same(torch, g, k) for g, k in zip(gos, keep)), "the incoming gradient was written"


# ---- D ---------------------------------------------------------------------------------------------------------------------------
@CASES
def test_d_partial_requires_grad(torch_mod, case):
    torch = torch_mod
    a = anchor(torch, case)
    n = len(a.ins)
    subsets = {tuple(i == k for i in range(n)) for k in range(n)} | {tuple(i != k for i in range(n)) for k in range(n)}
    for req in sorted(subsets - {(False,) * n, (True,) * n}):
        got = run(torch, case, a.data, requires=req)
        assert [g is not None for g in got.grads] == list(req)
        assert_same_run(torch, got, a, f"requires_grad={req}")
    none = run(torch, case, a.data, requires=(False,) * n)
    no_grad = run(torch, case, a.data, grad_mode=False)
    assert not any(o.requires_grad for o in none.outs + no_grad.outs)
    assert_same_run(torch, none, a, "no input requires grad")
    assert_same_run(torch, no_grad, a, "no_grad")


# ---- E ---------------------------------------------------------------------------------------------------------------------------
@CASES
def test_e_inputs_are_not_written(torch_mod, case):
    torch = torch_mod
    a = anchor(torch, case)
    with case.environ():
        ins, consts, gos = tensors(torch, a.data)
        keep = [t.detach().clone() for t in ins + consts]
        outs = case.apply(torch, ins, consts)
        assert all(same(torch, t, k) for t, k in zip(ins + consts, keep)), "forward wrote an input"
        grads = torch.autograd.grad(outs[:case.ndiff], ins, gos)
        assert all(same(torch, t, k) for t, k in zip(ins + consts, keep)), "backward wrote an input"
    assert_same_run(torch, Run(a.data, ins, consts, gos, outs, list(grads)), a, "plain call")


@pytest.mark.parametrize("case", [c for c in ac.CASES if c.inplace], ids=repr)
def test_e_inplace_contract(torch_mod, case):
    """inplace=True: t IS the output and its version rose (mark_dirty), rem is untouched"""
    torch = torch_mod
    from ganet_amd.functions.fused import ResidualReluFunction
    a = anchor(torch, case)
    ins, consts, gos = tensors(torch, a.data)
    t = ins[0].clone()
    rem_keep, version = ins[1].detach().clone(), t._version
    y = ResidualReluFunction.apply(t, ins[1], *(consts if case.scaled else (None, None)), True)
    assert y is t and y.data_ptr() == t.data_ptr() and t._version > version
    assert same(torch, ins[1], rem_keep) and same(torch, y, a.outs[0])
    grads = torch.autograd.grad(y, ins, gos)
    assert same(torch, ins[1], rem_keep)
    assert_same_run(torch, Run(a.data, ins, consts, gos, (y,), list(grads)), a, "in place")


# ---- F ---------------------------------------------------------------------------------------------------------------------------
@CASES
def test_f_accumulation(torch_mod, case):
    torch = torch_mod
    a = anchor(torch, case)
    with case.environ():
        ins, consts, gos = tensors(torch, a.data)
        outs = case.apply(torch, ins, consts)
        torch.autograd.backward(outs[:case.ndiff], gos, retain_graph=True)
        first = [t.grad.clone() for t in ins]
        torch.autograd.backward(outs[:case.ndiff], gos)
    for k, (t, f, g) in enumerate(zip(ins, first, a.grads)):
        assert same(torch, f, g), f"input {k}: first backward()"
        assert same(torch, t.grad, g * 2), f"input {k}: .grad after two backward() calls is not 2 x the anchor"
    if isinstance(case, ac.Residual):
        # the unscaled backward hands ONE tensor object to both inputs: the two .grad must still be two buffers
        assert ins[0].grad.untyped_storage().data_ptr() != ins[1].grad.untyped_storage().data_ptr()


# ---- G ---------------------------------------------------------------------------------------------------------------------------
@CASES
def test_g_stream_ordering(torch_mod, case):
    """Inputs, constants and the incoming gradient are NaN until copies enqueued on a side stream -- behind a delay -- fill
    them in; forward and backward run under torch.cuda.stream(side).  A launch that goes to any other stream reads NaN.  The
    stream must still be busy when the host calls return, or the test has shown nothing (delay: SLEEP_TICKS above).
    Twice, on two streams created one after the other: the runtime spreads its streams over a few hardware queues, and a
    launch on the wrong stream that happens to share the side stream's queue still runs in order behind the copies (seen on
    the device: with every launch sent to stream 0, 8 of 39 single-stream runs passed)."""
    torch = torch_mod
    a = anchor(torch, case)
    real = [t.detach() for t in a.ins] + a.consts + a.gos
    n, nc = len(a.ins), len(a.consts)
    for side in (torch.cuda.Stream(), torch.cuda.Stream()):
        bufs = [torch.full_like(t, float("nan")) for t in real]
        torch.cuda.synchronize()
        with case.environ(), torch.cuda.stream(side):
            torch.cuda._sleep(SLEEP_TICKS)
            for b, r in zip(bufs, real):
                b.copy_(r)
            ins, consts, gos = [b.requires_grad_() for b in bufs[:n]], bufs[n:n + nc], bufs[n + nc:]
            outs = case.apply(torch, ins, consts)
            grads = torch.autograd.grad(outs[:case.ndiff], ins, gos)
        busy = not side.query()
        side.synchronize()
        assert busy, "the side stream had drained before the host calls returned: nothing was shown"
        assert_same_run(torch, Run(a.data, ins, consts, gos, outs, list(grads)), a, "side stream")


# ---- H ---------------------------------------------------------------------------------------------------------------------------
@CASES
def test_h_graph_capture_and_replay(torch_mod, case):
    """forward + autograd.grad captured once (single stream, after one warm-up on a side stream), replayed on three other data
    sets -- other seeds, and the op's second value family where it has one: each replay equals the eager run on that data.
    Fails on a host decision baked in at capture time, a hidden synchronisation, state created lazily after the first call."""
    torch = torch_mod
    datas = [case.make(seed=10 + k, family=(k + 1) % case.families) for k in range(3)]
    eager = [run(torch, case, d) for d in datas]
    with case.environ():
        ins, consts, gos = tensors(torch, case.make())
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            outs = case.apply(torch, ins, consts)
            torch.autograd.grad(outs[:case.ndiff], ins, gos)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = case.apply(torch, ins, consts)
            grads = torch.autograd.grad(outs[:case.ndiff], ins, gos)
    for k, e in enumerate(eager):
        with torch.no_grad():
            for dst, src in zip(ins + consts + gos, e.ins + e.consts + e.gos):
                dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert_same_run(torch, Run(e.data, ins, consts, gos, outs, list(grads)), e, f"replay {k}")


# ---- I ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shapes", [[(2, 4, 6), (2, 4, 6)], [(2, 4, 6), (1, 5, 7), (2, 4, 6), (1, 5, 7)]], ids=["one-shape", "two-shapes"])
def test_i_disparity_loss_instance_reuse(torch_mod, shapes):
    """one instance called on several (outputs, target) pairs BEFORE any of their backwards runs (its parameter tensor and
    fp64 workspace are shared between the calls), against one fresh instance per pair"""
    torch = torch_mod
    case = next(c for c in ac.CASES if isinstance(c, ac.Loss))
    calls = []
    for k, shape in enumerate(shapes):
        preds, t = lc.random_maps(3800 + k, shape, 3)
        calls.append(([torch.from_numpy(p.reshape(shape)).to(DEVICE).requires_grad_() for p in preds],
                      torch.from_numpy(t.reshape(shape)).to(DEVICE), torch.tensor(0.5 + k, device=DEVICE)))
    shared = case.new_module()
    results = [shared(preds, t) for preds, t, _ in calls]
    got = [torch.autograd.grad(loss, preds, go) for (loss, _), (preds, _, go) in zip(results, calls)]
    for k, (preds, t, go) in enumerate(calls):
        loss, stats = case.new_module()(preds, t)
        want = torch.autograd.grad(loss, preds, go)
        assert same(torch, results[k][0], loss) and same(torch, results[k][1], stats), f"call {k}: loss / stats"
        assert all(same(torch, g, w) for g, w in zip(got[k], want)), f"call {k}: gradients"
