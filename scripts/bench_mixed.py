#!/usr/bin/env python
"""Mixed-precision sites one by one at the cfg3 shapes (GANet_deep at 1248x384, max_disp 192): the 16-bit-storage kernel of
ganet_amd.functions.mixed against the cast arm -- the existing fp32 op between ATen casts, what harness.fuse.use_mixed_precision
binds with kernels=False.

    python scripts/bench_mixed.py [--dtype bf16|fp16] [--reps 20] [--rounds 7] [--out profiles/NAME.json]

Per site: ms per call (HIP events around `reps` back-to-back calls, the two arms alternating, median over `rounds` after a
warm-up round), the bytes the site has to move (inputs read once, outputs written once, computed from the shapes), the rate
that gives and its fraction of the 6.3 TB/s device-to-device copy rate of MI355X_MICROARCH.md.  The two arms are compared bit
for bit at the timed size first: faster and different is not faster.  One JSON line."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", choices=("bf16", "fp16"), default="bf16")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mixed needs a GPU"
    from ganet_amd import _native
    assert not _native.lib().is_simulator
    from ganet_amd.functions import fused, mixed
    from ganet_amd.modules.fused import BnRelu
    from ganet_amd.modules.GANet import GetCostVolume
    from ganet_amd.modules.mixed import MixedBnRelu, MixedGetCostVolume
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16}[args.dtype]
    torch.manual_seed(1)
    dev = torch.device("cuda:0")
    sites = []

    def bn_sites(shape, tag):
        C = shape[1]
        bn = torch.nn.BatchNorm3d(C).to(dev).eval()
        with torch.no_grad():
            bn.running_mean.normal_()
            bn.running_var.uniform_(0.5, 1.5)
        x = torch.randn(shape, device=dev).to(dt)
        rem = torch.randn(shape, device=dev)
        n = x.numel()
        plain, plain_c = MixedBnRelu(bn, inplace=False), BnRelu(bn)
        to32 = MixedBnRelu(bn, out_dtype=torch.float32, inplace=False)
        sites.append((f"bn+relu 16->16 {tag}", 4 * n, lambda: plain(x), lambda: plain_c(x.float()).to(dt)))
        sites.append((f"bn+relu 16->f32 {tag} (in front of SGA)", 6 * n, lambda: to32(x), lambda: plain_c(x.float())))
        sites.append((f"bn+rem(f32)+relu 16->16 {tag} (SGABlock tail)", 8 * n, lambda: plain(x, rem), lambda: plain_c(x.float(), rem).to(dt)))

    bn_sites((1, 32, 65, 128, 416), "[1,32,65,128,416]")
    bn_sites((1, 48, 33, 64, 208), "[1,48,33,64,208]")
    g = torch.randn(1, 640, 128, 416, device=dev).to(dt)
    sites.append(("guidance L1 normalise [1,640,128,416] -> 4 x f32", 6 * g.numel(),
                  lambda: mixed.normalize_guidance_mixed(g, 32), lambda: fused.normalize_guidance(g.float(), 32)))
    fx, fy = (torch.randn(1, 32, 128, 416, device=dev).to(dt) for _ in range(2))
    cv, cv_c = MixedGetCostVolume(64), GetCostVolume(64)
    n_cost = 64 * 65 * 128 * 416
    sites.append(("cost volume -> [1,64,65,128,416]", 2 * n_cost + 4 * fx.numel(), lambda: cv(fx, fy), lambda: cv_c(fx.float(), fy.float()).to(dt)))
    v = torch.randn(1, 32, 65, 128, 416, device=dev)
    sites.append(("cast f32->16 [1,32,65,128,416] (ganet_cast against aten._to_copy)", 6 * v.numel(), lambda: mixed.cast(v, dt), lambda: v.to(dt)))

    rows = []
    with torch.no_grad():
        for name, nbytes, native, cast_arm in sites:
            a, b = native(), cast_arm()
            a, b = (a, b) if isinstance(a, (tuple, list)) else ((a,), (b,))
            equal = all(x.dtype == y.dtype and torch.equal(bits(x), bits(y)) for x, y in zip(a, b))
            del a, b
            timed(native, 2), timed(cast_arm, 2)                           # warm-up
            tn, tc = [], []
            for _ in range(args.rounds):                                   # alternating
                tn.append(timed(native, args.reps))
                tc.append(timed(cast_arm, args.reps))
            tn.sort(), tc.sort()
            ms_n, ms_c = tn[len(tn) // 2], tc[len(tc) // 2]
            rows.append({"site": name, "equal_bits": equal, "native_ms": round(ms_n, 4), "cast_arm_ms": round(ms_c, 4),
                         "speedup": round(ms_c / ms_n, 2), "native_ms_min_max": [round(tn[0], 4), round(tn[-1], 4)],
                         "cast_arm_ms_min_max": [round(tc[0], 4), round(tc[-1], 4)], "bytes_needed_MB": round(nbytes / 1e6, 1),
                         "native_TBs": round(nbytes / ms_n / 1e9, 3), "native_fraction_of_copy_rate": round(nbytes / (ms_n * 1e-3) / COPY_RATE, 3)})
            torch.cuda.empty_cache()
    res = {"what": "mixed-precision sites, 16-bit-storage kernel against the cast arm (fp32 op between ATen casts)", "dtype": args.dtype,
           "reps": args.reps, "rounds": args.rounds, "copy_rate_TBs": COPY_RATE / 1e12, "device": torch.cuda.get_device_name(0), "sites": rows}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
