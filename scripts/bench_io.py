"""The image front and back end of one KITTI-sized pair (375 x 1242 -> 384 x 1248) on its own, two forms alternating in one
process:
  host    predict.py's order of work: numpy standardisation and padding on the host, two fp32 uploads (`.cuda()`); the fp32 map
          downloaded (`.cpu()`), un-padded and converted with astype on the host
  fused   the uint8 images uploaded as they are, ganet_amd.modules.fused.StereoInput (2 launches) and DisparityOutput (1 launch),
          the uint16 image downloaded

    python scripts/bench_io.py [--iters 20] [--height 375 --width 1242 --crop_height 384 --crop_width 1248]
    python scripts/bench_io.py --profile K            K bare launches of each kernel form, nothing timed, for
                                                      `rocprofv3 --kernel-trace --stats -- python ...` (the eager event figures
                                                      are launch-bound: the kernels' own durations come from the trace)

Figures: wall clock around a synchronise after warm-up (front and back separately, per form, three rounds); the three kernels'
device time by events (the table form and the direct form of the apply pass); the fused form's graph replay (3 launches, no
copies).  The bound beside them: uint8 in (read twice) and fp32 out at the copy rate bench.py's roofline measures.
Prints one JSON object."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ganet_amd.functions.fused import disparity_to_u16, stereo_input  # noqa: E402
from ganet_amd.modules.fused import DisparityOutput, StereoInput  # noqa: E402
from harness.predict import host_back, host_front  # noqa: E402

COPY_GBS = 6300.0


def wall_ms(fn, iters):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
        torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t) / iters


def event_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--height", type=int, default=375)
    ap.add_argument("--width", type=int, default=1242)
    ap.add_argument("--crop_height", type=int, default=384)
    ap.add_argument("--crop_width", type=int, default=1248)
    ap.add_argument("--profile", type=int, default=0)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    left, right = (rng.integers(0, 256, (a.height, a.width, 3)).astype(np.uint8) for _ in range(2))
    crop = (a.crop_height, a.crop_width)
    front, back = StereoInput(*crop), DisparityOutput()
    pred = (torch.rand((1,) + crop, device=dev) * 190).contiguous()
    hw = (a.height, a.width)

    def host_f():
        l, r, _ = host_front(left, right, crop)
        return torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()

    def fused_f():
        l, r, _ = front(torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda())
        return l, r

    def host_b():
        return host_back(pred.cpu().numpy(), hw)

    def fused_b():
        return back(pred, hw).cpu().numpy()

    (hl, hr), (fl, fr) = host_f(), fused_f()
    same_front = bool(torch.equal(hl, fl) and torch.equal(hr, fr))
    same_back = bool(np.array_equal(host_b(), fused_b()))
    for fn in (host_f, fused_f, host_b, fused_b):
        for _ in range(3):
            fn()
    r3 = lambda v: round(v, 4)   # noqa: E731
    rounds = [[r3(wall_ms(fn, a.iters)) for fn in (host_f, fused_f, host_b, fused_b)] for _ in range(3)]

    # the kernels alone: images and map resident on the device
    dl, dr = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
    ol, orr = (torch.empty((3,) + crop, device=dev) for _ in range(2))
    oy, ox = a.height - a.crop_height, a.width - a.crop_width
    table = lambda: stereo_input(dl, dr, crop, oy, ox, ox, ol, orr, form=0)     # noqa: E731
    direct = lambda: stereo_input(dl, dr, crop, oy, ox, ox, ol, orr, form=1)    # noqa: E731
    u16 = lambda: disparity_to_u16(pred[0], hw, -oy, -ox)                        # noqa: E731

    def three():
        table()
        u16()

    if a.profile:
        for fn in (table, direct, u16):
            for _ in range(a.profile):
                fn()
        torch.cuda.synchronize()
        print(json.dumps({"profile": a.profile, "forms": ["table", "direct", "u16"]}))
        return
    table()
    t_bits = ol.clone()
    direct()
    same_forms = bool(torch.equal(t_bits.view(torch.int32), ol.view(torch.int32)))
    for fn in (table, direct, u16, three):
        for _ in range(10):
            fn()
    kern = {"front_table": [r3(event_ms(table, 200)) for _ in range(3)], "front_direct": [r3(event_ms(direct, 200)) for _ in range(3)],
            "back_u16": [r3(event_ms(u16, 200)) for _ in range(3)]}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        three()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        three()
    g.replay()
    graph = [r3(event_ms(g.replay, 200)) for _ in range(3)]
    n_in, n_out = a.height * a.width * 3, 3 * a.crop_height * a.crop_width * 4
    print(json.dumps({
        "what": "image front and back end of one stereo pair, ms per pair", "device": torch.cuda.get_device_name(0),
        "image": [a.height, a.width, 3], "crop": list(crop), "iters": a.iters,
        "wall_ms_rounds": {"front_host": [r[0] for r in rounds], "front_fused": [r[1] for r in rounds],
                           "back_host": [r[2] for r in rounds], "back_fused": [r[3] for r in rounds]},
        "kernels_event_ms": kern, "graph_replay_3_launches_ms": graph,
        "bound_ms": {"front": r3(1e-6 * (2 * 2 * n_in + 2 * n_out) / COPY_GBS), "copy_GBs": COPY_GBS,
                     "bytes": {"uint8_in_per_pass": 2 * n_in, "passes_over_input": 2, "fp32_out": 2 * n_out}},
        "upload_bytes": {"host": 2 * n_out, "fused": 2 * n_in},
        "equal": {"front_host_vs_fused": same_front, "back_host_vs_fused": same_back, "table_vs_direct": same_forms}}, indent=1))


if __name__ == "__main__":
    main()
