"""The streaming kernels around the guided-aggregation ops (misc_kernels.h, their 16-bit readers of mixed_kernels.h, the SGA
inference merge) at the model's shapes through the C ABI: ms per call.  Every entry twice: 16-byte aligned tensors (the
vector kernels) and the same tensors one element further on (`+1`: their scalar twins).

  python scripts/bench_misc.py [--lib PATH ...] [--rounds N] [--out FILE]

With several --lib the builds alternate inside each round of one process on the same buffers (an older build is bound with
strict=False); an entry is timed over at least 0.1 s of calls.  Prints one JSON document: ms[entry][lib] = one value per round."""
import argparse, json, math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from ganet_amd import _native

ap = argparse.ArgumentParser()
ap.add_argument("--lib", action="append", help="libganet_hip.so to time (default: this tree's)")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out")
args = ap.parse_args()

dev = torch.device("cuda:0")
paths = args.lib or [_native.lib_path()]
libs = [_native.CApi(p, strict=False) for p in paths]
st = torch.cuda.current_stream().cuda_stream
F16, BF16 = 1, 2      # include/ganet_hip.h: GANET_F16, GANET_BF16


def timed(fn, min_s=0.1):
    """ms per call over at least min_s of calls (20 calls of a 0.1 ms kernel are 2 ms: too short for device events)"""
    def run(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record(); e1.synchronize()
        return e0.elapsed_time(e1) / iters
    fn(); torch.cuda.synchronize()
    return run(max(20, math.ceil(min_s * 1e3 / max(run(20), 1e-3))))


def buf(shape, k, dtype=torch.float32, fill="randn"):
    """a tensor that starts k elements behind a 16-byte boundary"""
    n = math.prod(shape)
    flat = torch.empty(n + k, device=dev, dtype=dtype)
    v = flat[k:].view(shape)
    if fill == "randn":
        v.copy_(torch.randn(shape, device=dev))
    elif fill == "rand":
        v.copy_(torch.rand(shape, device=dev))
    return v


def entries(k):
    """name -> fn(lib), on tensors offset by k elements"""
    tag = "+1" if k else ""
    P = lambda *ts: [None if t is None else t.data_ptr() for t in ts]
    out = {}
    for W in (208, 206):      # W = 206: the scalar cost volume at aligned pointers too
        N, C, Dn, H = 1, 32, 65, 80
        x, y = buf((N, C, H, W), k), buf((N, C, H, W), k)
        cost, gc = buf((N, 2 * C, Dn, H, W), k, fill=None), buf((N, 2 * C, Dn, H, W), k)
        gx, gy = buf((N, C, H, W), k, fill=None), buf((N, C, H, W), k, fill=None)
        x16, y16 = (buf((N, C, H, W), 2 * k, torch.bfloat16) for _ in range(2))
        c16 = buf((N, 2 * C, Dn, H, W), 2 * k, torch.bfloat16, fill=None)
        dims = (N, C, Dn, H, W, st)
        out[f"cost_volume_fwd_W{W}{tag}"] = lambda l, a=P(x, y, cost), d=dims: l.call("ganet_cost_volume_forward", *a, *d)
        out[f"cost_volume_fwd16_W{W}{tag}"] = lambda l, a=P(x16, y16, c16), d=dims: l.call("ganet_cost_volume_forward_16", *a, *d)
        if W == 208:
            out[f"cost_volume_bwd{tag}"] = lambda l, a=P(gc, gx, gy), d=dims: l.call("ganet_cost_volume_backward", *a, *d)
    N, Dn, H, W = 1, 193, 240, 624
    dims = (N, Dn, H, W, st)
    p, gp, sy = buf((N, Dn, H, W), k, fill="rand"), buf((N, Dn, H, W), k, fill=None), buf((N, Dn, H, W), k, fill=None)
    o, go, sn, mx, ss = (buf((N, H, W), k) for _ in range(5))
    out["disp_regression_fwd" + tag] = lambda l, a=P(p, o): l.call("ganet_disparity_regression_forward", *a, *dims)
    out["disp_regression_bwd" + tag] = lambda l, a=P(go, gp): l.call("ganet_disparity_regression_backward", *a, *dims)
    out["norm_regression_fwd" + tag] = lambda l, a=P(p, o, sn): l.call("ganet_norm_disparity_regression_forward", *a, *dims)
    out["norm_regression_bwd" + tag] = lambda l, a=P(p, o, sn, go, gp): l.call("ganet_norm_disparity_regression_backward", *a, *dims)
    out["softmin_fwd" + tag] = lambda l, a=P(p, sy): l.call("ganet_softmin_forward", *a, *dims)
    out["softmin_bwd" + tag] = lambda l, a=P(sy, p, gp): l.call("ganet_softmin_backward", *a, *dims)
    out["softmin_regression_fwd" + tag] = lambda l, a=P(p, o, mx, ss): l.call("ganet_softmin_regression_forward", *a, *dims)
    out["softmin_regression_bwd" + tag] = lambda l, a=P(p, o, mx, ss, go, gp): l.call("ganet_softmin_regression_backward", *a, *dims)
    # the guidance split [1,640,80,208] (G = 4, K = 5) and the LGA filters [1,75,240,624]: fp32 and bf16 readers
    for name, (N, G, C, K, H, W) in (("guidance", (1, 4, 32, 5, 80, 208)), ("filter", (1, 1, 1, 75, 240, 624))):
        g = buf((N, G * C * K, H, W), k)
        g16 = buf((N, G * C * K, H, W), 2 * k, torch.bfloat16)
        ys = [buf((N, C, K, H, W), k, fill=None) if i < G else None for i in range(4)]
        gg = buf((N, G * C * K, H, W), k, fill=None)
        dims_n = (N, G, C, K, H, W)
        out[f"{name}_normalize_fwd{tag}"] = lambda l, a=P(g, *ys), d=dims_n: l.call("ganet_l1_normalize_forward", *a, *d, st)
        out[f"{name}_normalize_fwd_bf16{tag}"] = lambda l, a=P(g16, *ys), d=dims_n: l.call("ganet_l1_normalize_forward_mixed", *a, *d, BF16, st)
        out[f"{name}_normalize_bwd{tag}"] = lambda l, a=P(g, *ys, gg), d=dims_n: l.call("ganet_l1_normalize_backward", *a, *d, st)
    # SGABlock's residual tail and the inference merge (ROWWAVE off: four scans into A_ws, then sga_merge_infer -- the scans are
    # most of that time) at [1,32,65,80,208]
    N, C, D, H, W = 1, 32, 65, 80, 208
    shape = (N, C, D, H, W)
    t, rem, yv, gt = buf(shape, k), buf(shape, k), buf(shape, k, fill=None), buf(shape, k, fill=None)
    sc, sh = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev)
    dims5 = (N, C, D, H, W, st)
    out["residual_relu_fwd" + tag] = lambda l, a=P(t, rem, sc, sh, yv): l.call("ganet_residual_relu_forward", *a, *dims5)
    out["residual_relu_bwd" + tag] = lambda l, a=P(yv, rem, sc, gt, t): l.call("ganet_residual_relu_backward", *a, *dims5)
    gs = [torch.nn.functional.normalize(buf((N, C, 5, H, W), k), p=1, dim=2) for _ in range(4)]
    gsk = [buf((N, C, 5, H, W), k, fill=None).copy_(g) for g in gs]
    ws = buf((4,) + shape, k, fill=None)

    def merge(l, a=P(t, *gsk, ws, yv, sc, sh)):
        l.set_option("GANET_SGA_ROWWAVE", 0)
        try:
            l.call("ganet_sga_forward_infer", *a, *dims5)
        finally:
            l.set_option("GANET_SGA_ROWWAVE", 1)
    out["sga_infer_scans_and_merge" + tag] = merge
    return out


ms = {}
for k in (0, 1):
    es = entries(k)
    for name, fn in es.items():
        ms[name] = {p: [] for p in paths}
    for _ in range(args.rounds):
        for name, fn in es.items():
            for p, l in zip(paths, libs):
                ms[name][p].append(round(timed(lambda: fn(l)), 5))
    del es
    torch.cuda.empty_cache()
doc = json.dumps({"libs": paths, "rounds": args.rounds, "ms": ms}, indent=1)
print(doc)
if args.out:
    open(args.out, "w").write(doc + "\n")
