#!/usr/bin/env python
"""BASELINE.json configs[2]: full GANet-deep inference (9 GA layers... 7 SGA + 2 LGA2) on a KITTI-2015-sized pair
(1248x384, max_disp 192) on one MI355X, the reference's model on this repository's ops.

    python -m harness.infer [--model GANet_deep] [--height 384] [--width 1248] [--max_disp 192] [--fused] [--fused_bn] [--fused_conv32] [--amp bf16|fp16 [--amp_cast_arm] [--amp_conv32]] [--channels_last] [--iters 5]

Prints one JSON line: ms per forward pass (median of --iters, HIP events), peak device memory, parameter count.
Random-init weights and synthetic standardised images (no checkpoint / dataset offline); predict.py:100-114 is the
step.  For the GA-op share of the pass run it under `rocprofv3 --kernel-trace --stats` and feed the kernel stats to
scripts/model_kernel_share.py."""
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

from harness import fuse, steps  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="GANet_deep")
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=1248)
    ap.add_argument("--max_disp", type=int, default=192)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--fused", action="store_true", help="ganet_amd.modules.fused op chains instead of the stock call forms")
    ap.add_argument("--fused_bn", action="store_true", help="BatchNorm + ReLU behind every BasicConv on ganet_amd.modules.fused.BnRelu")
    ap.add_argument("--fused_conv32", action="store_true", help="conv32x1 of every Disp / DispAgg on ganet_amd.modules.fused.DispConv (HIP kernels instead of MIOpen)")
    ap.add_argument("--amp", choices=("bf16", "fp16"), default=None,
                    help="mixed-precision inference: 16-bit convolutions under torch.autocast around the fp32 GA ops (harness.fuse.use_mixed_precision; implies --fused --fused_bn)")
    ap.add_argument("--amp_cast_arm", action="store_true", help="with --amp: the cast arm (fp32 ops between ATen casts) instead of the 16-bit-storage kernels")
    ap.add_argument("--amp_conv32", action="store_true", help="with --amp: conv32x1 of every Disp / DispAgg on ganet_amd.modules.mixed_conv.MixedDispConv (the HIP kernels on the 16-bit volume; with --amp_cast_arm its cast arm)")
    ap.add_argument("--channels_last", action="store_true",
                    help="the cost aggregation on channels_last_3d tensors (harness.fuse.use_channels_last; fp32 inference, implies --fused --fused_bn)")
    ap.add_argument("--no_miopen_find", dest="miopen_find", action="store_false",
                    help="MIOpen immediate mode (heuristic solver choice) instead of timing its solvers per shape")
    ap.add_argument("--kernel_share", action="store_true", help="add the per-group device-time table (torch.profiler over 2 extra passes)")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if args.amp_conv32 and args.amp is None:
        ap.error("--amp_conv32 needs --amp")
    if args.channels_last:
        if args.amp is not None:
            ap.error("--channels_last is fp32 only: it does not compose with --amp")
        from harness.miopen_env import suggest_channels_last
        suggest_channels_last()        # before torch's first convolution
    assert torch.cuda.is_available(), "harness.infer needs a GPU"
    from ganet_amd import _native
    assert not _native.lib().is_simulator
    dev = torch.device("cuda:0")
    torch.backends.cudnn.benchmark = bool(args.miopen_find)     # MIOpen find mode (harness/miopen_env.py)
    torch.manual_seed(123)
    model = steps.build_model(args.model, args.max_disp, dev)
    n_fused = fuse.use_fused_ops(model) if args.fused else 0
    n_fused_bn = fuse.use_fused_bn(model) if args.fused_bn else 0
    n_fused_conv32 = fuse.use_fused_disp_conv(model) if args.fused_conv32 else 0
    amp = {"bf16": torch.bfloat16, "fp16": torch.float16, None: None}[args.amp]
    n_mixed = fuse.use_mixed_precision(model, amp, kernels=not args.amp_cast_arm) if amp is not None else 0
    n_amp_conv32 = fuse.use_mixed_disp_conv(model, kernels=not args.amp_cast_arm) if args.amp_conv32 else 0
    n_cl = fuse.use_channels_last(model.eval()) if args.channels_last else 0
    left, right, _ = steps.synthetic_batch(args.batch, args.height, args.width, args.max_disp, dev)
    for _ in range(args.warmup):
        out = steps.predict(model, left, right, amp)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    times = []
    for _ in range(args.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = steps.predict(model, left, right, amp)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    times.sort()
    assert out.shape == (args.batch, args.height, args.width) and bool(torch.isfinite(out).all())
    share = None
    if args.kernel_share:
        from harness.kernel_share import profile_passes
        share = profile_passes(lambda: steps.predict(model, left, right, amp), 2)
    print(json.dumps({
        "what": "full-model inference, reference model on the drop-in ops", "model": args.model,
        "input": [args.batch, 3, args.height, args.width], "max_disp": args.max_disp,
        "ops": "ganet_amd.modules.fused (%d call sites)" % n_fused if args.fused else "drop-in call forms (libs/)",
        "fused_bn": "BnRelu (%d call sites)" % n_fused_bn if args.fused_bn else False,
        "fused_conv32": "DispConv (%d call sites)" % n_fused_conv32 if args.fused_conv32 else False,
        "ms_per_pair": round(times[len(times) // 2], 3), "ms_min": round(times[0], 3), "iters": args.iters,
        "peak_mem_GB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 3),
        "miopen_find": bool(args.miopen_find), "params": sum(p.numel() for p in model.parameters()),
        "amp": ("%s, %s (%d call sites)" % (args.amp, "cast arm" if args.amp_cast_arm else "16-bit-storage kernels", n_mixed)) if amp is not None else None,
        "amp_conv32": "MixedDispConv (%d call sites)" % n_amp_conv32 if args.amp_conv32 else False,
        "channels_last": "ClBnRelu / ClGetCostVolume (%d call sites), PYTORCH_MIOPEN_SUGGEST_NHWC=%s" % (n_cl, os.environ.get("PYTORCH_MIOPEN_SUGGEST_NHWC")) if args.channels_last else False,
        "dtype": ("%s convolutions under autocast, f32 guided aggregation and tails" % args.amp) if amp is not None else "f32", "weights": "random init",
        "disp_range": [round(float(out.min()), 3), round(float(out.max()), 3)],
        "device": torch.cuda.get_device_name(0), "kernel_share": share}))


if __name__ == "__main__":
    main()
