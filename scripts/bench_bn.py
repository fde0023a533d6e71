"""BatchNorm + ReLU of a training step on its own: the stock chain F.relu_(bn(x)) (MIOpen's BatchNorm kernels, relu_ and
threshold_backward) against ganet_amd.modules.fused.BnRelu, forward and forward + backward, at the activation shapes of a cfg4
step of GANet_deep (240x624 crop): the 3-D volumes at 1/3, 1/6 and 1/12 resolution and two 2-D feature maps.

    python scripts/bench_bn.py                        timing: device events around an eager loop after warm-up, the two forms
                                                      alternating in one process, three rounds; each form's graph replay beside it
    python scripts/bench_bn.py --only fused --iters K --no-time
                                                      K bare iterations, for `rocprofv3 --kernel-trace --stats -- python ...`
The bound beside each figure: 3 volumes forward and 5 backward at the copy rate bench.py's roofline measures (6.3 TB/s).
Prints one JSON object."""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from ganet_amd.modules.fused import BnRelu  # noqa: E402

SHAPES = {"vol3": (1, 32, 65, 80, 208), "vol6": (1, 48, 33, 40, 104), "vol12": (1, 64, 17, 20, 52),
          "feat1": (1, 32, 240, 624), "feat3": (1, 32, 80, 208)}
COPY_GBS = 6300.0


def section(shape, dev):
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(shape, generator=g) * 1.5 + 0.3).to(dev).requires_grad_()
    gy = torch.randn(shape, generator=g).to(dev)
    bn_s = (torch.nn.BatchNorm3d if len(shape) == 5 else torch.nn.BatchNorm2d)(shape[1]).to(dev)
    bn_f = copy.deepcopy(bn_s)
    fused_mod = BnRelu(bn_f)

    def make(fwd, bn):
        def forward():
            return fwd(x)

        def both():
            return torch.autograd.grad(fwd(x), [x, bn.weight, bn.bias], gy)
        return forward, both

    return make(lambda t: F.relu_(bn_s(t)), bn_s), make(fused_mod, bn_f)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["stock", "fused"])
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--shape", choices=sorted(SHAPES), default=None)
    ap.add_argument("--no-time", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"what": "BatchNorm (training mode) + ReLU, ms per iteration; fwd and fwd+bwd", "device": torch.cuda.get_device_name(0)}
    for name in ([a.shape] if a.shape else list(SHAPES)):
        shape = SHAPES[name]
        (s_fwd, s_both), (f_fwd, f_both) = section(shape, dev)
        if a.no_time:
            fn = s_both if a.only == "stock" else f_both
            for _ in range(a.iters):
                fn()
            torch.cuda.synchronize()
            out[name] = {"form": a.only, "iterations": a.iters}
            continue
        ys, yf = s_fwd().detach().clone(), f_fwd().detach().clone()
        gs, gf = s_both(), f_both()
        for fn in (s_fwd, f_fwd, s_both, f_both):
            for _ in range(10):
                fn()
        r3 = lambda v: round(v, 4)   # noqa: E731
        rounds = [(r3(eager_ms(s_fwd, a.iters)), r3(eager_ms(f_fwd, a.iters)), r3(eager_ms(s_both, a.iters)), r3(eager_ms(f_both, a.iters)))
                  for _ in range(3)]
        vol_ms = 4e-6 * float(torch.tensor(shape).prod()) / COPY_GBS        # one volume at the copy rate
        graph_fused = {"fwd": r3(graph_ms(f_fwd, a.iters)), "fwd_bwd": r3(graph_ms(f_both, a.iters))}
        try:
            graph_stock = {"fwd": r3(graph_ms(s_fwd, a.iters)), "fwd_bwd": r3(graph_ms(s_both, a.iters))}
        except RuntimeError as e:                      # (a stock kernel that refuses capture: reported, not fatal)
            graph_stock = {"error": str(e).splitlines()[0][:200]}
        out[name] = {"shape": list(shape),
                     "eager_fwd_ms": {"stock": [r[0] for r in rounds], "fused": [r[1] for r in rounds]},
                     "eager_fwd_bwd_ms": {"stock": [r[2] for r in rounds], "fused": [r[3] for r in rounds]},
                     "graph_ms": {"stock": graph_stock, "fused": graph_fused},
                     "bound_ms": {"fwd_3V": r3(3 * vol_ms), "bwd_5V": r3(5 * vol_ms)},
                     "y_max_abs_diff": float((yf - ys).abs().max()),
                     "grad_max_rel_diff": max(float((p - q).abs().max() / q.abs().max()) for p, q in zip(gf, gs))}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
