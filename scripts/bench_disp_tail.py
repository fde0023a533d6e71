"""The Disp tail of a training step on its own: behind conv32x1, the two-op chain use_fused_ops installs (TrilinearUpsample ->
SoftminDisparityRegression: the up-sampled volume is written, saved, re-read and mirrored by a gradient volume) against
ganet_amd.modules.fused.DispTail, forward and forward + backward, at the shapes of a cfg4 step (240x624 crop, one sample) and
of a cfg5 step (528x960, two samples per GPU).

    python scripts/bench_disp_tail.py                 timing: device events around an eager loop after warm-up, the two forms
                                                      alternating in one process, three rounds; each form's graph replay and
                                                      peak-memory rise over forward + backward beside it
    python scripts/bench_disp_tail.py --only fused --shape cfg4 --iters K --no-time
                                                      K bare iterations, for `rocprofv3 --kernel-trace --stats -- python ...`
The bound beside each figure is DispTail's traffic at the copy rate bench.py's roofline measures (6.3 TB/s): the input once
forward; over forward + backward the input plus the column workspace gc [N,Di,Ho,Wo] written and read (the input is
cache-resident for its re-reads, the input gradient is as small).
Prints one JSON object."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ganet_amd.modules.fused import DispTail, SoftminDisparityRegression, TrilinearUpsample  # noqa: E402

SHAPES = {"cfg4": ((1, 1, 65, 80, 208), (193, 240, 624)), "cfg5": ((2, 1, 65, 176, 320), (193, 528, 960))}
COPY_GBS = 6300.0


def section(shape, size, dev):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(shape, generator=g).to(dev).requires_grad_()
    go = torch.randn((shape[0],) + size[1:], generator=g).to(dev)
    up, reg, tail = TrilinearUpsample(), SoftminDisparityRegression(size[0] - 1), DispTail(size[0] - 1)

    def make(fwd):
        def forward():
            return fwd(x)

        def both():
            return torch.autograd.grad(fwd(x), [x], go)
        return forward, both

    return make(lambda c: reg(up(c, list(size)).squeeze(1))), make(tail)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["chain", "fused"])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--shape", choices=sorted(SHAPES), default=None)
    ap.add_argument("--no-time", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"what": "Disp tail behind conv32x1 (up-sampling + Softmin + regression), ms per iteration; fwd and fwd+bwd",
           "device": torch.cuda.get_device_name(0)}
    for name in ([a.shape] if a.shape else list(SHAPES)):
        shape, size = SHAPES[name]
        (c_fwd, c_both), (f_fwd, f_both) = section(shape, size, dev)
        if a.no_time:
            fn = c_both if a.only == "chain" else f_both
            for _ in range(a.iters):
                fn()
            torch.cuda.synchronize()
            out[name] = {"form": a.only, "iterations": a.iters}
            continue
        yc, yf = c_fwd().detach().clone(), f_fwd().detach().clone()
        (gc,), (gf,) = c_both(), f_both()
        for fn in (c_fwd, f_fwd, c_both, f_both):
            for _ in range(5):
                fn()
        r4 = lambda v: round(v, 4)   # noqa: E731
        rounds = [(r4(eager_ms(c_fwd, a.iters)), r4(eager_ms(f_fwd, a.iters)), r4(eager_ms(c_both, a.iters)), r4(eager_ms(f_both, a.iters)))
                  for _ in range(3)]
        mem = {"chain": peak_rise_mb(c_both), "fused": peak_rise_mb(f_both)}
        graph = {"chain": {"fwd": r4(graph_ms(c_fwd, a.iters)), "fwd_bwd": r4(graph_ms(c_both, a.iters))},
                 "fused": {"fwd": r4(graph_ms(f_fwd, a.iters)), "fwd_bwd": r4(graph_ms(f_both, a.iters))}}
        N, _, Di, Hi, Wi = shape
        x_mb, gc_mb, vol_mb = 4e-6 * N * Di * Hi * Wi, 4e-6 * N * Di * size[1] * size[2], 4e-6 * N * size[0] * size[1] * size[2]
        out[name] = {"shape": list(shape), "size": list(size),
                     "eager_fwd_ms": {"chain": [r[0] for r in rounds], "fused": [r[1] for r in rounds]},
                     "eager_fwd_bwd_ms": {"chain": [r[2] for r in rounds], "fused": [r[3] for r in rounds]},
                     "fused_faster_in_all_rounds": {"fwd": all(r[1] < r[0] for r in rounds), "fwd_bwd": all(r[3] < r[2] for r in rounds)},
                     "graph_ms": graph,
                     "peak_rise_fwd_bwd_MB": mem,
                     "MB": {"x": r4(x_mb), "gc_workspace": r4(gc_mb), "upsampled_volume": r4(vol_mb)},
                     "bound_ms": {"fwd_x": r4(x_mb / COPY_GBS), "fwd_bwd_x_plus_2gc": r4((x_mb + 2 * gc_mb) / COPY_GBS)},
                     "out_max_abs_diff": float((yf - yc).abs().max()),
                     "grad_max_rel_diff": float((gf - gc).abs().max() / gc.abs().max())}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
