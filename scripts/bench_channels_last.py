#!/usr/bin/env python
"""The channels-last inference path, measured at the cfg3 shapes (GANet_deep at 1248x384, max_disp 192).

    python scripts/bench_channels_last.py --what convs [--out profiles/NAME.json]     1. per convolution
    python scripts/bench_channels_last.py --what sites [--out ...]                    2. per site
    python scripts/bench_channels_last.py --what pass  [--out ...]                    3. whole pass

1. Every distinct 3-D convolution of the cost aggregation with planar against channels_last_3d operands (input and weight), in
   two processes of their own -- PYTORCH_MIOPEN_SUGGEST_NHWC unset and =1: the switch is read once per process -- in MIOpen's
   find mode: ms per call from replays of a captured graph, the output's memory format, the kernel names the torch profiler
   sees and whether a batched_transpose kernel is among them.
2. Every layout combination of ganet_bn_apply_forward_cl and the channels-last cost volume against what produces the same
   layouts today -- the planar entry plus ATen's .contiguous(memory_format=...) -- and against the planar entry alone; the
   results are compared bit for bit first.  ms from graph replays, the bytes the site has to move, the fraction of the
   6.3 TB/s copy rate.
3. python -m harness.infer --fused --fused_bn, with and without --channels_last, a process each, with the kernel-share table
   and the share of batched_transpose kernels; the stand-in network of tests/standin_net.py where the reference's model
   files are not reachable.
One JSON line per run."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

COPY_RATE = 6.3e12            # bytes / s
L0, L1, L2 = (65, 128, 416), (33, 64, 208), (17, 32, 104)
# (name, transposed, Cin, Cout, kernel, stride, input D,H,W, calls per GANet_deep pass)
CONVS = [
    ("64->32 k3 @65x128x416 (conv_start, deconv1a/1b.conv2)", False, 64, 32, (3, 3, 3), 1, L0, 3),
    ("32->32 k3 @65x128x416 (conv_refine of sga1-3)", False, 32, 32, (3, 3, 3), 1, L0, 3),
    ("32->48 k3 s2 @65x128x416 (conv1a, conv1b.conv1)", False, 32, 48, (3, 3, 3), 2, L0, 2),
    ("48->48 k3 @33x64x208 (conv_refine of sga11-14)", False, 48, 48, (3, 3, 3), 1, L1, 4),
    ("48->64 k3 s2 @33x64x208 (conv2a, conv2b.conv1)", False, 48, 64, (3, 3, 3), 2, L1, 2),
    ("96->48 k3 @33x64x208 (deconv2a/2b.conv2, conv1b.conv2)", False, 96, 48, (3, 3, 3), 1, L1, 3),
    ("128->64 k3 @17x32x104 (conv2b.conv2)", False, 128, 64, (3, 3, 3), 1, L2, 1),
    ("transposed 64->48 k3x4x4 s2 @17x32x104 (deconv2a/2b.conv1)", True, 64, 48, (3, 4, 4), 2, L2, 2),
    ("transposed 48->32 k3x4x4 s2 @33x64x208 (deconv1a/1b.conv1)", True, 48, 32, (3, 4, 4), 2, L1, 2),
]
SITE_SHAPES = [(1, 32, 65, 128, 416), (1, 48, 33, 64, 208), (1, 64, 17, 32, 104)]


def graph_ms(torch, fn, reps, rounds):
    """ms per call of fn from replays of one captured graph of `reps` calls: median of `rounds`"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(reps):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / reps)
    del graph
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def kernel_names(torch, fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {}
    for row in prof.key_averages():
        dt = float(getattr(row, "self_device_time_total", 0) or getattr(row, "self_cuda_time_total", 0) or 0)
        if dt > 0:
            out[row.key[:120]] = round(dt / 1e3, 4)
    return dict(sorted(out.items(), key=lambda kv: -kv[1]))


# ---- 1. per convolution ---------------------------------------------------------------------------------------------------------

def convs_child(args):
    import torch
    import torch.nn.functional as F
    torch.backends.cudnn.benchmark = True                                    # MIOpen find mode
    torch.manual_seed(1)
    dev = torch.device("cuda:0")
    rows = []
    with torch.no_grad():
        for name, transposed, cin, cout, k, stride, dhw, calls in CONVS:
            x = torch.randn((1, cin) + dhw, device=dev)
            w = torch.randn((cin, cout) + k if transposed else (cout, cin) + k, device=dev) * 0.05
            op = (lambda a, b: F.conv_transpose3d(a, b, stride=stride, padding=1)) if transposed else (lambda a, b: F.conv3d(a, b, stride=stride, padding=1))
            row = {"conv": name, "calls_per_pass": calls}
            outs = {}
            for layout in ("planar", "channels_last"):
                fmt = torch.channels_last_3d if layout == "channels_last" else torch.contiguous_format
                a, b = x.contiguous(memory_format=fmt), w.contiguous(memory_format=fmt)
                fn = lambda: op(a, b)                                        # noqa: E731
                y = fn()                                                     # find mode: the search happens here
                torch.cuda.synchronize()
                ms, lo, hi = graph_ms(torch, fn, args.reps, args.rounds)
                names = kernel_names(torch, fn)
                outs[layout] = y
                row[layout] = {"ms": round(ms, 4), "ms_min_max": [round(lo, 4), round(hi, 4)],
                               "output_channels_last": bool(y.is_contiguous(memory_format=torch.channels_last_3d)),
                               "batched_transpose": any("batched_transpose" in n for n in names),
                               "transpose_ms": round(sum(v for n, v in names.items() if "transpose" in n.lower()), 4), "kernels": names}
            row["max_abs_difference"] = float((outs["planar"] - outs["channels_last"]).abs().max())
            row["output_abs_max"] = float(outs["planar"].abs().max())
            rows.append(row)
            print(f"{name}: planar {row['planar']['ms']} ms, channels-last {row['channels_last']['ms']} ms", file=sys.stderr, flush=True)
            del outs, x, w
            torch.cuda.empty_cache()
    print(json.dumps({"switch": os.environ.get("PYTORCH_MIOPEN_SUGGEST_NHWC"), "torch": torch.__version__,
                      "device": torch.cuda.get_device_name(0), "convs": rows}))


def child(argv, env):
    """a fresh process; its last line of output is its JSON result.  A line on stderr every minute while it works (find mode is
    silent for minutes)"""
    import tempfile
    import time
    with tempfile.TemporaryFile("w+") as out:
        proc = subprocess.Popen([sys.executable] + argv, env=env, stdout=out, cwd=ROOT)
        t0 = time.time()
        while True:
            try:
                rc = proc.wait(timeout=60)
                break
            except subprocess.TimeoutExpired:
                print(f"... {' '.join(argv[-3:])}: {time.time() - t0:.0f} s", file=sys.stderr, flush=True)
        out.seek(0)
        text = out.read()
    if rc != 0:
        raise SystemExit(f"{' '.join(argv)} failed ({rc}):\n{text[-4000:]}")
    return json.loads(text.strip().splitlines()[-1])


def convs(args):
    arms = {}
    for tag, value in (("switch_unset", None), ("switch_1", "1")):
        env = {k: v for k, v in os.environ.items() if k != "PYTORCH_MIOPEN_SUGGEST_NHWC"}
        if value is not None:
            env["PYTORCH_MIOPEN_SUGGEST_NHWC"] = value
        arms[tag] = child([os.path.abspath(__file__), "--what", "convs_child", "--reps", str(args.reps), "--rounds", str(args.rounds)], env)
    total = {}
    for tag, arm in arms.items():
        for layout in ("planar", "channels_last"):
            total[f"{tag}/{layout}"] = {"ms_per_pass": round(sum(r[layout]["ms"] * r["calls_per_pass"] for r in arm["convs"]), 3),
                                        "transpose_ms_per_pass": round(sum(r[layout]["transpose_ms"] * r["calls_per_pass"] for r in arm["convs"]), 3)}
    return {"what": "every distinct 3-D convolution of a cfg3 GANet_deep pass, planar against channels_last_3d operands, find mode, graph replays",
            "reps": args.reps, "rounds": args.rounds, "sum_over_a_pass": total, "arms": arms}


# ---- 2. per site ------------------------------------------------------------------------------------------------------------------

def sites(args):
    import torch
    from ganet_amd.functions.channels_last import bn_apply_cl, cost_volume_cl
    from ganet_amd.functions.fused import BnApplyFunction
    from ganet_amd.functions.GANet import GetCostVolumeFunction
    torch.manual_seed(1)
    dev = torch.device("cuda:0")
    CL, PL = torch.channels_last_3d, torch.contiguous_format
    bits = lambda t: t.contiguous().view(torch.int32)                       # noqa: E731
    rows = []

    def measure(name, nbytes, new, today, planar_alone):
        a, b = new(), today()
        equal = bool(torch.equal(bits(a), bits(b)))
        del a, b
        ms = {}
        for tag, fn in (("new", new), ("planar_entry_plus_aten_copies", today), ("planar_entry_alone", planar_alone)):
            ms[tag] = graph_ms(torch, fn, args.reps, args.rounds)
        rows.append({"site": name, "equal_bits": equal, "bytes_needed_MB": round(nbytes / 1e6, 1),
                     **{f"{tag}_ms": round(v[0], 4) for tag, v in ms.items()},
                     **{f"{tag}_ms_min_max": [round(v[1], 4), round(v[2], 4)] for tag, v in ms.items()},
                     "new_TBs": round(nbytes / ms["new"][0] / 1e9, 3),
                     "new_fraction_of_copy_rate": round(nbytes / (ms["new"][0] * 1e-3) / COPY_RATE, 3),
                     "planar_entry_alone_fraction_of_copy_rate": round(nbytes / (ms["planar_entry_alone"][0] * 1e-3) / COPY_RATE, 3),
                     "new_against_today": round(ms["planar_entry_plus_aten_copies"][0] / ms["new"][0], 2),
                     "new_against_planar_entry_alone": round(ms["planar_entry_alone"][0] / ms["new"][0], 2)})
        torch.cuda.empty_cache()

    with torch.no_grad():
        for shape in SITE_SHAPES:
            C = shape[1]
            xp = torch.randn(shape, device=dev)
            xc = xp.contiguous(memory_format=CL)
            rem = torch.randn(shape, device=dev)
            scale, shift = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev)
            n, tag = xp.numel(), str(list(shape)).replace(" ", "")
            planar = lambda r=None: BnApplyFunction.apply(xp, r, scale, shift, True, False)     # noqa: E731
            forms = [
                ("cl -> cl", None, CL, lambda: BnApplyFunction.apply(xc.contiguous(), None, scale, shift, True, True).contiguous(memory_format=CL)),
                ("cl -> planar (in front of SGA)", None, PL, lambda: BnApplyFunction.apply(xc.contiguous(), None, scale, shift, True, True)),
                ("planar -> cl (behind SGA)", None, CL, lambda: planar().contiguous(memory_format=CL)),
                ("cl + rem planar -> cl (SGABlock tail)", rem, CL, lambda: BnApplyFunction.apply(xc.contiguous(), rem, scale, shift, True, True).contiguous(memory_format=CL)),
                ("cl + rem planar -> planar (last tail)", rem, PL, lambda: BnApplyFunction.apply(xc.contiguous(), rem, scale, shift, True, True)),
            ]
            for name, r, fmt, today in forms:
                src = xp if name.startswith("planar") else xc
                new = lambda src=src, r=r, fmt=fmt: bn_apply_cl(src, scale, shift, r, True, fmt, False)      # noqa: E731
                measure(f"bn+relu {name} {tag}", 4 * n * (3 if r is not None else 2), new, today, lambda r=r: planar(r))
            del xp, xc, rem
            torch.cuda.empty_cache()
        fx, fy = (torch.randn(1, 32, 128, 416, device=dev) for _ in range(2))
        n_cost = 64 * 65 * 128 * 416
        measure("cost volume C=32 Dn=65 128x416 -> [1,65,128,416,64]", 4 * n_cost + 8 * fx.numel(),
                lambda: cost_volume_cl(fx, fy, 65),
                lambda: GetCostVolumeFunction.apply(fx, fy, 65).contiguous(memory_format=CL),
                lambda: GetCostVolumeFunction.apply(fx, fy, 65))
    return {"what": "channels-last sites: the new kernel against the planar entry plus ATen's layout copies, and against the planar entry alone; graph replays",
            "reps": args.reps, "rounds": args.rounds, "copy_rate_TBs": COPY_RATE / 1e12, "device": torch.cuda.get_device_name(0), "sites": rows}


# ---- 3. whole pass ------------------------------------------------------------------------------------------------------------------

def standin_child(args):
    """the stand-in network at its largest size, both arms in one process (its convolutions are small: find mode is quick)"""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import standin_net as sn
    from harness import fuse, steps
    from harness.kernel_share import profile_passes
    torch.backends.cudnn.benchmark = True
    torch.manual_seed(1)
    first = sn.build(192, "cuda").eval()
    left, right, _ = steps.synthetic_batch(1, 384, 1248, 192, "cuda")
    res = {}
    outs = {}
    for arm in ("planar", "channels_last"):
        m = sn.build(192, "cuda").eval()
        m.load_state_dict(first.state_dict())
        fuse.use_fused_ops(m)
        fuse.use_fused_bn(m)
        if arm == "channels_last":
            fuse.use_channels_last(m)
        fn = lambda m=m: steps.predict(m, left, right)                       # noqa: E731
        for _ in range(3):
            outs[arm] = fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        times.sort()
        res[arm] = {"ms_per_pair": round(times[len(times) // 2], 3), "kernel_share": profile_passes(fn, 2)}
    res["max_abs_difference_of_the_disparity"] = float((outs["planar"] - outs["channels_last"]).abs().max())
    print(json.dumps(res))


def whole_pass(args):
    from harness import refmodel
    env = {k: v for k, v in os.environ.items() if k != "PYTORCH_MIOPEN_SUGGEST_NHWC"}
    if not refmodel.available():
        res = child([os.path.abspath(__file__), "--what", "standin_child", "--rounds", str(args.rounds)], dict(env, PYTORCH_MIOPEN_SUGGEST_NHWC="1"))
        return {"what": "whole pass: the stand-in network of tests/standin_net.py at 1248x384, max_disp 192 (no reference model files here)", **res}
    base = ["-m", "harness.infer", "--fused", "--fused_bn", "--kernel_share", "--iters", str(args.rounds)]
    arms = {"planar": child(base, env), "channels_last": child(base + ["--channels_last"], env)}
    return {"what": "whole pass: python -m harness.infer --fused --fused_bn, with and without --channels_last, a process each", "arms": arms,
            "ms_per_pair": {k: v["ms_per_pair"] for k, v in arms.items()},
            "batched_transpose": {k: (v.get("kernel_share") or {}).get("watched") for k, v in arms.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", required=True, choices=("convs", "sites", "pass", "convs_child", "standin_child"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.what == "convs_child":
        return convs_child(args)
    if args.what == "standin_child":
        return standin_child(args)
    res = {"convs": convs, "sites": sites, "pass": whole_pass}[args.what](args)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
