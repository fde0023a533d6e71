#!/usr/bin/env python
"""Mixed-precision TRAINING sites one by one at the model's shapes (GANet_deep at 240 x 624, max_disp 192): the 16-bit-storage
Function of ganet_amd.functions.mixed_train against the cast arm -- the existing fp32 op between ATen casts with autograd through
both, what harness.fuse.use_mixed_precision_training binds with kernels=False.

    python scripts/bench_mixed_train.py [--dtype bf16|fp16] [--reps 20] [--rounds 7] [--graph] [--out profiles/NAME.json]

Per site: ms per call (HIP events around `reps` back-to-back calls, the two arms alternating in one process, median over `rounds`
after a warm-up round), the bytes the site has to move (inputs read as often as the two launches read them, outputs written once,
computed from the shapes), the rate that gives and its fraction of the 6.3 TB/s device-to-device copy rate.  The three BatchNorm
sites forward and forward + backward, the cost-volume backward and the guidance-normalise backward.  The two arms are compared
first at the timed size, bit for bit, and the script stops where they differ: the BatchNorm sites run on dyadic inputs whose sums
are exact in any order (the exact tier of tests/mixed_train_cases.py), so their reductions owe the same bits too.  --graph times
graph replays of both arms: the device time without autograd's host work.  Peak memory of forward + backward per arm.  One JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

COPY_RATE = 6.3e12            # bytes / s


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(bits(a), bits(b)))


def dyadic(shape, unit, span, dev, centre=None):
    """integers in [-span, span] times `unit`, each channel's values a symmetric set around `centre[c]`: exact in both 16-bit
    formats, and every sum the BatchNorm forms over them is exact in any order (tests/mixed_train_cases.py: the exact tier), so
    the two arms owe each other the same bits"""
    N, C = shape[:2]
    S = 1
    for s in shape[2:]:
        S *= s
    assert N == 1 and S % 2 == 0
    k = torch.randint(-span, span + 1, (C, S // 2), device=dev)
    k = torch.cat([k, -k], 1)
    k = torch.gather(k, 1, torch.rand(C, S, device=dev).argsort(1)).float() * unit
    if centre is not None:
        k = k + centre[:, None]
    return k.reshape(shape)


def graphed(fn):
    """fn captured into a graph after a warm-up on a side stream: the replay leaves autograd's host work out of the timing"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn(), fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = fn()
    graph.keep = keep
    return graph.replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", choices=("bf16", "fp16"), default="bf16")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--graph", action="store_true", help="time graph replays of each arm instead of eager calls (device time without autograd's host work)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mixed_train needs a GPU"
    from ganet_amd import _native
    assert not _native.lib().is_simulator
    from ganet_amd.functions import fused, mixed_train
    from ganet_amd.modules.fused import BnRelu
    from ganet_amd.modules.GANet import GetCostVolume
    from ganet_amd.modules.mixed import MixedTrainBnRelu
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16}[args.dtype]
    torch.manual_seed(1)
    dev = torch.device("cuda:0")
    sites = []          # (name, bytes, kernel fn, cast-arm fn): each fn returns the tensors to compare

    def bn_sites(shape, tag):
        C, n = shape[1], 1
        for s in shape:
            n *= s
        bn = torch.nn.BatchNorm3d(C).to(dev).train()
        with torch.no_grad():
            bn.weight.uniform_(0.5, 1.5), bn.bias.normal_(0, 0.5)
        centre = torch.tensor([1.0, -0.5, 0.0, 2.0, -1.25], device=dev).repeat(C)[:C]
        x = dyadic(shape, 0.25, 8, dev, centre).to(dt).requires_grad_()
        rem = dyadic(shape, 0.5, 4, dev).requires_grad_()
        # (site, rem, out dtype, bytes forward: x twice + y [+ rem], bytes backward: x and gy twice + gx [+ rem twice + grem])
        for site, r, od, bf, bb in (("16->16", None, None, 6, 10), ("16->f32 (in front of SGA)", None, torch.float32, 8, 14),
                                    ("tail 16 + f32 rem -> 16", rem, None, 10, 22)):
            ydt = od or dt
            gy = dyadic(shape, 0.125, 4, dev).to(ydt)
            k_op, c_op = MixedTrainBnRelu(bn, out_dtype=od), BnRelu(bn)

            def k_fwd(k_op=k_op, r=r):
                return [k_op(x, r) if r is not None else k_op(x)]

            def c_fwd(c_op=c_op, r=r, ydt=ydt):
                return [c_op(x.float(), r).to(ydt)]

            def k_all(f=k_fwd, r=r, gy=gy):
                y = f()[0]
                return [y] + list(torch.autograd.grad(y, [x, bn.weight, bn.bias] + ([r] if r is not None else []), gy))

            def c_all(f=c_fwd, r=r, gy=gy):
                y = f()[0]
                return [y] + list(torch.autograd.grad(y, [x, bn.weight, bn.bias] + ([r] if r is not None else []), gy))

            sites.append((f"bn {site} forward {tag}", bf * n, k_fwd, c_fwd))
            sites.append((f"bn {site} forward + backward {tag}", (bf + bb) * n, k_all, c_all))

    bn_sites((1, 32, 65, 80, 208), "[1,32,65,80,208]")
    bn_sites((1, 48, 33, 40, 104), "[1,48,33,40,104]")

    g = torch.randn(1, 640, 80, 208, device=dev).to(dt).requires_grad_()
    ggs = [torch.randn(1, 32, 5, 80, 208, device=dev) for _ in range(4)]

    def k_guid():
        return list(torch.autograd.grad(mixed_train.NormalizeGuidanceMixedFunction.apply(g, 32), [g], ggs))

    def c_guid():
        return list(torch.autograd.grad(fused.normalize_guidance(g.float(), 32), [g], ggs))

    # forward: x + four outputs; backward: x, four gradients, gx
    sites.append(("guidance normalise forward + backward [1,640,80,208]", g.numel() * (2 + 4 + 2 + 4 + 2), k_guid, c_guid))

    fx = torch.randn(1, 32, 80, 208, device=dev).to(dt).requires_grad_()
    fy = torch.randn(1, 32, 80, 208, device=dev).to(dt).requires_grad_()
    gc = torch.randn(1, 64, 65, 80, 208, device=dev).to(dt)
    cv32 = GetCostVolume(64)

    def k_cv():
        return list(torch.autograd.grad(mixed_train.CostVolume16Function.apply(fx, fy, 65), [fx, fy], gc))

    def c_cv():
        return list(torch.autograd.grad(cv32(fx.float(), fy.float()).to(dt), [fx, fy], gc))

    sites.append(("cost volume forward + backward [1,64,65,80,208]", 2 * (2 * gc.numel() + 2 * fx.numel() * 2), k_cv, c_cv))

    rows = []
    for name, nbytes, k_fn, c_fn in sites:
        a, b = k_fn(), c_fn()
        if not all(same(u, v) for u, v in zip(a, b)):              # faster and different is not faster: nothing is timed
            raise SystemExit(f"{name}: the two arms differ at the timed size")
        del a, b
        peaks = []
        for fn in (k_fn, c_fn):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            peaks.append((torch.cuda.max_memory_allocated() - base) / 2 ** 20)
        if args.graph:
            k_fn, c_fn = graphed(k_fn), graphed(c_fn)
        timed(k_fn, 2), timed(c_fn, 2)
        ks, cs = [], []
        for _ in range(args.rounds):
            ks.append(timed(k_fn, args.reps))
            cs.append(timed(c_fn, args.reps))
        ks.sort(), cs.sort()
        k_ms, c_ms = ks[len(ks) // 2], cs[len(cs) // 2]
        rows.append({"site": name, "kernel_ms": round(k_ms, 4), "cast_arm_ms": round(c_ms, 4), "speedup": round(c_ms / k_ms, 2),
                     "bytes_needed_MB": round(nbytes / 1e6, 1), "kernel_fraction_of_copy_rate": round(nbytes / (k_ms * 1e-3) / COPY_RATE, 3),
                     "agree": "bit for bit", "timed": "graph replays" if args.graph else "eager calls",
                     "peak_rise_MiB_kernel": round(peaks[0], 1), "peak_rise_MiB_cast_arm": round(peaks[1], 1)})
        print(rows[-1], file=sys.stderr)
    line = {"what": "mixed-precision training sites, 16-bit-storage Functions against the cast arm", "dtype": args.dtype,
            "device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds, "copy_rate_TBps": COPY_RATE / 1e12,
            "rows": rows}
    print(json.dumps(line))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
