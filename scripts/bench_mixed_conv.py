#!/usr/bin/env python
"""conv32x1 under mixed precision at the model's shapes: what a 16-bit input to the tails' Conv3d(32, 1, 3, 1, 1) costs on three arms.

    python scripts/bench_mixed_conv.py [--dtype bf16|fp16] [--reps 20] [--rounds 7] [--out profiles/NAME.json]

  1  "autocast"   what the model does without use_mixed_disp_conv: the 16-bit F.conv3d under torch.autocast (MIOpen, find mode; the
                  weight rounded to 16 bits by autocast) and the up-cast of its small output by CastFunction, as
                  harness.fuse._conv32x1_f32 binds it.  The yardstick.
  2  "cast arm"   MixedDispConv(kernels=False): DispConvFunction on x.float() -- the fp32 kernels behind an up-cast pass, the data
                  gradient cast back by autograd
  3  "kernels"    MixedDispConv(kernels=True): DispConv16Function, the 16-bit siblings of the same kernels
Per shape ([1,32,65,80,208] and [1,32,65,128,416]) and run -- forward alone, forward + the data gradient, forward + the weight
gradient, forward + both -- eager calls and graph replays: ms per call (HIP events around `reps` back-to-back calls, the three
arms alternating in one process, median over `rounds` after a warm-up round), the bytes arm 3 has to move (computed from the
shapes) and the fraction of the 6.3 TB/s device-to-device copy rate that gives.  Arm 3 is compared with arm 2 first, at the timed
size, bit for bit -- y, grad_x and grad_weight -- and the script stops where they differ.  Arm 1 computes something else (a
16-bit weight, MIOpen's summation): how far it is from arm 3 is reported, not asserted.  One JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from harness.miopen_env import use_repo_miopen_cache  # noqa: E402

use_repo_miopen_cache()            # before torch loads MIOpen

import torch  # noqa: E402

COPY_RATE = 6.3e12            # bytes / s
SHAPES = [(1, 32, 65, 80, 208), (1, 32, 65, 128, 416)]


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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mixed_conv needs a GPU"
    from ganet_amd import _native
    assert not _native.lib().is_simulator
    from ganet_amd.functions import mixed_train
    from ganet_amd.modules.mixed_conv import MixedDispConv
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16}[args.dtype]
    torch.backends.cudnn.benchmark = True          # MIOpen find mode (harness/miopen_env.py): arm 1 as the harness runs it
    torch.manual_seed(1)
    dev = torch.device("cuda:0")
    rows = []
    for shape in SHAPES:
        N, C, D, H, W = shape
        conv = torch.nn.Conv3d(C, 1, (3, 3, 3), (1, 1, 1), (1, 1, 1), bias=False).to(dev)
        x = torch.randn(shape, device=dev).to(dt).requires_grad_()
        gy = torch.randn(N, 1, D, H, W, device=dev)
        k_op, c_op = MixedDispConv(conv, kernels=True), MixedDispConv(conv, kernels=False)

        def autocast_fwd():
            with torch.autocast("cuda", dtype=dt):
                c = conv(x)
            return mixed_train.CastFunction.apply(c.contiguous(), torch.float32)

        fwd = {"autocast": autocast_fwd, "cast arm": lambda: c_op(x), "kernels": lambda: k_op(x)}
        nx, ny = x.numel(), gy.numel()
        # bytes arm 3 needs: x (2 bytes) read once per direction that reads it, y / grad_y (4 bytes), grad_x (2 bytes) written once
        runs = [("forward", (), 2 * nx + 4 * ny),
                ("forward + data gradient", ("x",), 2 * nx + 4 * ny + 4 * ny + 2 * nx),
                ("forward + weight gradient", ("w",), 2 * nx + 4 * ny + 2 * nx + 4 * ny),
                ("forward + both gradients", ("x", "w"), 2 * nx + 4 * ny + 4 * ny + 2 * nx + 2 * nx + 4 * ny)]

        def make(arm, wrt):
            f = fwd[arm]
            targets = [t for k, t in (("x", x), ("w", conv.weight)) if k in wrt]
            if not targets:
                def run():
                    with torch.no_grad():
                        return [f()]
            else:
                def run():
                    y = f()
                    return [y] + list(torch.autograd.grad(y, targets, gy))
            return run

        # faster and different is not faster: arm 3 against arm 2, bit for bit, before anything is timed
        a, b, p = make("kernels", ("x", "w"))(), make("cast arm", ("x", "w"))(), make("autocast", ("x", "w"))()
        if not all(same(u, v) for u, v in zip(a, b)):
            raise SystemExit(f"{list(shape)}: the kernels and the cast arm differ at the timed size")
        far = [float((u.float() - v.float()).abs().max() / v.float().abs().max()) for u, v in zip(p, a)]
        del a, b, p
        for name, wrt, nbytes in runs:
            # a Function is told which gradients to compute by its inputs' requires_grad, not by what autograd.grad asks for
            x.requires_grad_("x" in wrt), conv.weight.requires_grad_("w" in wrt)
            for mode in ("eager calls", "graph replays"):
                fns = {arm: make(arm, wrt) for arm in fwd}
                if mode == "graph replays":
                    fns = {arm: graphed(fn) for arm, fn in fns.items()}
                ms = {arm: [] for arm in fns}
                for fn in fns.values():
                    timed(fn, 2)
                for _ in range(args.rounds):
                    for arm, fn in fns.items():
                        ms[arm].append(timed(fn, args.reps))
                med = {arm: sorted(v)[len(v) // 2] for arm, v in ms.items()}
                spread = {arm: (min(v), max(v)) for arm, v in ms.items()}
                rows.append({"shape": list(shape), "run": name, "timed": mode,
                             "autocast_ms": round(med["autocast"], 4), "cast_arm_ms": round(med["cast arm"], 4), "kernels_ms": round(med["kernels"], 4),
                             "min_max_ms": {arm: [round(lo, 4), round(hi, 4)] for arm, (lo, hi) in spread.items()},
                             "kernels_over_autocast_speedup": round(med["autocast"] / med["kernels"], 2),
                             "kernels_over_cast_arm_speedup": round(med["cast arm"] / med["kernels"], 2),
                             "bytes_needed_MB": round(nbytes / 1e6, 1), "kernels_fraction_of_copy_rate": round(nbytes / (med["kernels"] * 1e-3) / COPY_RATE, 3),
                             "kernels_against_cast_arm": "bit for bit",
                             "autocast_against_kernels_max_rel": {"y": far[0], "grad_x": far[1], "grad_weight": far[2]}})
                print(rows[-1], file=sys.stderr)
                del fns
    line = {"what": "conv32x1 on a 16-bit input: the 16-bit convolution under autocast + up-cast, the cast arm, the 16-bit kernels",
            "dtype": args.dtype, "device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds,
            "copy_rate_TBps": COPY_RATE / 1e12, "rows": rows}
    print(json.dumps(line))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
