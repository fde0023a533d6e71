"""The tails' conv32x1 = nn.Conv3d(32, 1, 3, 1, 1, bias=False) on its own: the stock path (MIOpen in find mode, the solver search
done before anything is timed and its duration reported) against ganet_amd.modules.fused.DispConv, at the shapes of a cfg4 step
([1,32,65,80,208]: 240x624 crop, one sample) and of a cfg5 step ([2,32,65,176,320]: 528x960, two samples per GPU): forward
alone, forward + both gradients, and each gradient alone.

    python scripts/bench_disp_conv.py                 timing: device events around an eager loop after warm-up, the two forms
                                                      alternating in one process, three rounds; each form's graph replay and
                                                      peak-memory rise over forward + backward beside it; whether two runs of
                                                      the weight gradient give the same bits, per form
    python scripts/bench_disp_conv.py --only fused --shape cfg4 --iters K --no-time
                                                      K bare iterations of forward + both gradients, for
                                                      `rocprofv3 --kernel-trace --stats -- python ...`
The bound beside each figure is the volume once at the copy rate bench.py's roofline measures (6.3 TB/s): read by the forward
and by the weight gradient, written by the data gradient (x plus the one-channel map: 142.7 MB at cfg4).
Prints one JSON object."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from harness.miopen_env import use_repo_miopen_cache  # noqa: E402

use_repo_miopen_cache()            # before torch loads MIOpen

import torch  # noqa: E402

from ganet_amd.functions.fused import disp_conv_grad_input, disp_conv_grad_weight  # noqa: E402
from ganet_amd.modules.fused import DispConv  # noqa: E402

SHAPES = {"cfg4": (1, 32, 65, 80, 208), "cfg5": (2, 32, 65, 176, 320)}
COPY_GBS = 6300.0
PARTS = ("fwd", "fwd_bwd", "grad_x", "grad_w")


def section(shape, dev):
    """{form: {part: callable}} on one input; the stock form first, so that its find passes can be timed"""
    N, C, D, H, W = shape
    g = torch.Generator().manual_seed(1)
    x = torch.randn(shape, generator=g).to(dev).requires_grad_()
    go = torch.randn((N, 1, D, H, W), generator=g).to(dev)
    torch.manual_seed(2)
    conv = torch.nn.Conv3d(C, 1, (3, 3, 3), (1, 1, 1), (1, 1, 1), bias=False).to(dev)
    forms = {}
    for name, op, native in (("stock", conv, False), ("fused", DispConv(conv), True)):
        # the gradients alone are plain calls under no_grad -- ATen's convolution_backward with one output asked for, resp. the
        # two entries DispConvFunction.backward calls: no autograd graph outlives a call (one kept alive across a graph capture
        # would tie the capture to the stream its AccumulateGrad nodes were made on)
        def grad_x(native=native):
            with torch.no_grad():
                return disp_conv_grad_input(go, conv.weight, x, native)

        def grad_w(native=native):
            with torch.no_grad():
                return disp_conv_grad_weight(x, go, conv.weight, native)

        forms[name] = {"fwd": lambda op=op: op(x),
                       "fwd_bwd": lambda op=op: torch.autograd.grad(op(x), [x, conv.weight], go),
                       "grad_x": grad_x, "grad_w": grad_w}
    return forms, conv


def eager_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def graph_ms(fn, iters):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn(); fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    g.replay()
    return eager_ms(g.replay, iters)


def peak_rise_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    r = fn()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    del r
    return round(rise / 1e6, 2)


def first_call_s(fn):
    """wall clock of a first call, synchronised: for the stock form in find mode this is MIOpen's solver search"""
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    del r
    return round(time.perf_counter() - t, 3)


def note(*words):
    """progress on stderr: the JSON object is printed at the very end"""
    print(*words, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["stock", "fused"])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--shape", choices=sorted(SHAPES), default=None)
    ap.add_argument("--no-time", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.backends.cudnn.benchmark = True          # MIOpen find mode (harness/miopen_env.py): the parent's path as the harness runs it
    out = {"what": "conv32x1 = Conv3d(32, 1, 3, 1, 1) alone, ms per iteration: stock (MIOpen, find mode) against DispConv",
           "device": torch.cuda.get_device_name(0)}
    r4 = lambda v: round(v, 4)   # noqa: E731
    for name in ([a.shape] if a.shape else list(SHAPES)):
        shape = SHAPES[name]
        forms, conv = section(shape, dev)
        if a.no_time:
            fn = forms[a.only or "fused"]["fwd_bwd"]
            for _ in range(a.iters):
                fn()
            torch.cuda.synchronize()
            out[name] = {"form": a.only or "fused", "iterations": a.iters}
            continue
        note(name, "first calls")
        # the first calls: MIOpen's find passes (forward, data gradient, weight gradient: three problems) resp. our library load
        first = {f: {"fwd": first_call_s(forms[f]["fwd"]), "grad_x": first_call_s(forms[f]["grad_x"]),
                     "grad_w": first_call_s(forms[f]["grad_w"])} for f in ("stock", "fused")}
        note(name, "first calls took", first, "; eager rounds")
        ys = {f: forms[f]["fwd"]().detach().clone() for f in forms}
        gs = {f: [t.clone() for t in forms[f]["fwd_bwd"]()] for f in forms}
        same_bits = {f: all(torch.equal(forms[f]["grad_w"](), gs[f][1]) for _ in range(3)) for f in forms}
        for f in forms:
            for p in PARTS:
                for _ in range(3):
                    forms[f][p]()
        rounds = [{f: {p: r4(eager_ms(forms[f][p], a.iters)) for p in PARTS} for f in ("stock", "fused")} for _ in range(3)]
        note(name, "eager ms, last round", rounds[-1], "; peak memory, graph replays")
        mem = {f: peak_rise_mb(forms[f]["fwd_bwd"]) for f in forms}
        graph = {}
        for f in forms:
            graph[f] = {}
            for p in ("fwd", "fwd_bwd"):
                graph[f][p] = r4(graph_ms(forms[f][p], a.iters))
                note(name, "graph replay", f, p, graph[f][p])
        N, C, D, H, W = shape
        vol_mb, map_mb = 4e-6 * N * C * D * H * W, 4e-6 * N * D * H * W
        bound = r4((vol_mb + map_mb) / COPY_GBS)
        out[name] = {"shape": list(shape),
                     "first_call_s": first,
                     "eager_ms": {f: {p: [r[f][p] for r in rounds] for p in PARTS} for f in ("stock", "fused")},
                     "fused_faster_in_all_rounds": {p: all(r["fused"][p] < r["stock"][p] for r in rounds) for p in PARTS},
                     "graph_ms": graph,
                     "peak_rise_fwd_bwd_MB": mem,
                     "MB": {"volume": r4(vol_mb), "one_channel_map": r4(map_mb)},
                     "bound_ms_per_direction": bound,
                     "fraction_of_copy_rate": {p: r4(bound / min(r["fused"][p] for r in rounds)) for p in ("fwd", "grad_x", "grad_w")},
                     "weight_gradient_same_bits_over_runs": same_bits,
                     "y_max_abs_diff": float((ys["fused"] - ys["stock"]).abs().max()),
                     "grad_x_max_rel_diff": float((gs["fused"][0] - gs["stock"][0]).abs().max() / gs["stock"][0].abs().max()),
                     "grad_w_max_rel_diff": float((gs["fused"][1] - gs["stock"][1]).abs().max() / gs["stock"][1].abs().max())}
        del forms, conv, ys, gs
        torch.cuda.empty_cache()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
