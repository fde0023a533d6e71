"""The criterion section of a training step on its own (forward + backward over three disparity maps, KITTI mix):
harness.steps.loss_mix + the error read-out of train.py:126 on stock PyTorch ops against ganet_amd.modules.fused.DisparityLoss,
at the map sizes of cfg4 ([1,240,624]) and cfg5 ([2,528,960]).

    python scripts/bench_loss.py                      timing: device events around an EAGER loop after warm-up, the two forms
                                                      alternating, three rounds (the stock form cannot be captured -- its
                                                      boolean indexing synchronises -- so both are timed the way a step runs
                                                      them); the fused form's graph replay beside it
    python scripts/bench_loss.py --only fused --iters K --no-time
                                                      K bare iterations, for `rocprofv3 --kernel-trace --stats -- python ...`:
                                                      launches per iteration = (calls at K=5 - calls at K=1) / 4
Prints one JSON object."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ganet_amd.modules.fused import DisparityLoss  # noqa: E402
from harness import steps  # noqa: E402

SHAPES = {"cfg4": (1, 240, 624), "cfg5": (2, 528, 960)}
MAX_DISP = 192


def section(shape, dev):
    left, right, target = steps.synthetic_batch(shape[0], shape[1], shape[2], MAX_DISP, dev, seed=1)
    target = target * 1.2                                   # a tenth of the pixels at or above max_disp
    g = torch.Generator().manual_seed(2)
    outs = [(target + 4 * torch.randn(shape, generator=g).to(dev)).requires_grad_() for _ in range(3)]
    crit, fused = steps.criterion(True), DisparityLoss.ganet_deep(MAX_DISP, kitti=True)

    def stock():
        mask = (target < MAX_DISP).detach()
        loss = steps.loss_mix("GANet_deep", outs, target, mask, crit)
        err = torch.mean(torch.abs(outs[-1][mask] - target[mask])).detach()
        return loss, err, torch.autograd.grad(loss, outs)

    def fusedf():
        loss, stats = fused(outs, target)
        return loss, stats[fused.epe_index], torch.autograd.grad(loss, outs)

    return stock, fusedf


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
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--shape", choices=sorted(SHAPES), default=None)
    ap.add_argument("--no-time", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"what": "criterion section fwd+bwd, P=3, KITTI mix, ms per iteration", "device": torch.cuda.get_device_name(0)}
    for name in ([a.shape] if a.shape else sorted(SHAPES)):
        stock, fusedf = section(SHAPES[name], dev)
        if a.no_time:
            fn = stock if a.only == "stock" else fusedf
            for _ in range(a.iters):
                fn()
            torch.cuda.synchronize()
            out[name] = {"form": a.only, "iterations": a.iters}
            continue
        ls, es, gs = stock()
        lf, ef, gf = fusedf()
        for fn in (stock, fusedf):
            for _ in range(20):
                fn()
        rounds = [(round(eager_ms(stock, a.iters), 4), round(eager_ms(fusedf, a.iters), 4)) for _ in range(3)]
        out[name] = {"shape": list(SHAPES[name]), "eager_stock_ms": [r[0] for r in rounds], "eager_fused_ms": [r[1] for r in rounds],
                     "graph_fused_ms": round(graph_ms(fusedf, a.iters), 4),
                     "loss_stock_fused": [float(ls), float(lf)], "epe_stock_fused": [float(es), float(ef)],
                     "grad_max_rel_diff": max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(gf, gs))}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
