#!/usr/bin/env python
"""predict.py of the reference for one stereo pair: two image files in, the 16-bit disparity image out.

    python -m harness.predict --left L --right R --out O [--crop_height 384] [--crop_width 1248] [--max_disp 192]
                              [--model GANet_deep] [--resume CKPT] [--fused] [--fused_bn] [--host_io]

L, R: anything PIL reads (KITTI's PNGs), or .npy arrays uint8 [H, W, 3 | 4].  O: a 16-bit PNG (mode I;16, disparity x 256 as
predict.py:138 saves it) or .npy (uint16 [h, w]).  The uint8 images go to the device as they are; standardisation, padding /
centre crop, the un-padding and the conversion to 16 bit run there (ganet_amd.modules.fused.StereoInput / DisparityOutput,
harness.steps.predict_images): no numpy on the pixel path.  --host_io runs the reference's order of work instead (numpy on
the host, fp32 upload, fp32 download, astype), for comparison.  The two differ where the reference is undefined: a constant
channel (NaN there, 0 here) and disparities outside [0, 256) (wrapped there, saturated here).

Prints one JSON line like harness.infer's, plus ms_io_front / ms_io_back (wall clock around a synchronise).  The model code is
the reference's ($GANET_REF_ROOT, harness/refmodel.py); the I/O ops need nothing of it.  Without --resume the weights are
random: the output is then a smoke signal, not a disparity map."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--left", required=True)
    ap.add_argument("--right", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--crop_height", type=int, default=384)
    ap.add_argument("--crop_width", type=int, default=1248)
    ap.add_argument("--max_disp", type=int, default=192)
    ap.add_argument("--model", default="GANet_deep")
    ap.add_argument("--resume", default="", help="a checkpoint of the reference's train.py ({'state_dict': ...})")
    ap.add_argument("--fused", action="store_true", help="ganet_amd.modules.fused op chains instead of the stock call forms")
    ap.add_argument("--fused_bn", action="store_true", help="BatchNorm + ReLU behind every BasicConv on ganet_amd.modules.fused.BnRelu")
    ap.add_argument("--host_io", action="store_true", help="the reference's host-side numpy front and back end instead of the kernels")
    ap.add_argument("--amp", choices=("bf16", "fp16"), default=None,
                    help="mixed-precision inference: 16-bit convolutions under torch.autocast around the fp32 GA ops (harness.fuse.use_mixed_precision)")
    ap.add_argument("--channels_last", action="store_true",
                    help="the cost aggregation on channels_last_3d tensors (harness.fuse.use_channels_last; fp32 inference, implies --fused --fused_bn)")
    ap.add_argument("--amp_cast_arm", action="store_true", help="with --amp: the cast arm (fp32 ops between ATen casts) instead of the 16-bit-storage kernels")
    ap.add_argument("--amp_conv32", action="store_true", help="with --amp: conv32x1 of every Disp / DispAgg on ganet_amd.modules.mixed_conv.MixedDispConv (the HIP kernels on the 16-bit volume; with --amp_cast_arm its cast arm)")
    args = ap.parse_args(argv)
    if args.amp_conv32 and args.amp is None:
        ap.error("--amp_conv32 needs --amp")
    if args.crop_height <= 0 or args.crop_width <= 0 or args.max_disp <= 0:
        ap.error("--crop_height, --crop_width and --max_disp are positive")
    return args


def read_image(path):
    """uint8 [H, W, 3 | 4] from an image file (PIL) or a .npy array"""
    import numpy as np
    if path.lower().endswith(".npy"):
        a = np.load(path)
    else:
        from PIL import Image
        with Image.open(path) as im:
            if im.mode not in ("RGB", "RGBA"):
                im = im.convert("RGB")
            a = np.asarray(im)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (3, 4):
        raise ValueError(f"{path}: expected uint8 [H, W, 3 | 4], got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a)


def write_disparity(path, u16):
    """uint16 [h, w] -> a 16-bit greyscale PNG (I;16) or a .npy array"""
    import numpy as np
    u16 = np.ascontiguousarray(u16)
    if u16.dtype != np.uint16 or u16.ndim != 2:
        raise ValueError(f"expected uint16 [h, w], got {u16.dtype} {u16.shape}")
    if path.lower().endswith(".npy"):
        np.save(path, u16)
        return
    from PIL import Image
    Image.frombytes("I;16", (u16.shape[1], u16.shape[0]), u16.astype("<u2").tobytes()).save(path)


def read_disparity(path):
    """what write_disparity wrote, back as uint16 [h, w]"""
    import numpy as np
    if path.lower().endswith(".npy"):
        return np.load(path)
    from PIL import Image
    with Image.open(path) as im:
        assert im.mode in ("I;16", "I;16L", "I"), im.mode
        return np.asarray(im).astype(np.uint16)


def host_front(left, right, crop_hw):
    """the numpy restatement of predict.py:92-114 and :75-90: fp32 [1, 3, Hc, Wc] twice and the image's size"""
    import numpy as np
    from ganet_amd.modules.fused import predict_offsets
    Hc, Wc = crop_hw
    h, w = left.shape[:2]
    oy, ox = predict_offsets(h, w, Hc, Wc)
    outs = []
    for img in (left, right):
        planes = np.zeros((3, Hc, Wc), np.float32)
        for c in range(3):
            ch = img[:, :, c]
            std = (ch - np.mean(ch)) / np.std(ch)
            if h <= Hc and w <= Wc:
                planes[c, -oy:, -ox:] = std
            else:
                planes[c] = std[oy:oy + Hc, ox:ox + Wc]
        outs.append(planes[None])
    return outs[0], outs[1], (h, w)


def host_back(pred, hw):
    """predict.py:132-138 on the downloaded fp32 map [1, Hc, Wc]"""
    Hc, Wc = pred.shape[1:]
    h, w = hw
    temp = pred[0, Hc - h:, Wc - w:] if h <= Hc and w <= Wc else pred[0]
    return (temp * 256).astype("uint16")


def main(argv=None):
    args = parse_args(argv)
    from harness.miopen_env import use_repo_miopen_cache
    use_repo_miopen_cache()            # before torch loads MIOpen
    if args.channels_last:
        if args.amp is not None:
            raise SystemExit("--channels_last is fp32 only: it does not compose with --amp")
        from harness.miopen_env import suggest_channels_last
        suggest_channels_last()        # before torch's first convolution
    import torch
    from harness import fuse, steps
    assert torch.cuda.is_available(), "harness.predict needs a GPU"
    from ganet_amd import _native
    assert not _native.lib().is_simulator
    dev = torch.device("cuda:0")
    torch.manual_seed(123)
    left, right = read_image(args.left), read_image(args.right)
    if left.shape != right.shape:
        raise ValueError(f"the two images differ in shape: {left.shape} and {right.shape}")
    crop = (args.crop_height, args.crop_width)
    model = steps.build_model(args.model, args.max_disp, dev)
    if args.resume:
        steps.load_checkpoint(args.resume, model)
    n_fused = fuse.use_fused_ops(model) if args.fused else 0
    n_fused_bn = fuse.use_fused_bn(model) if args.fused_bn else 0
    amp = {"bf16": torch.bfloat16, "fp16": torch.float16, None: None}[args.amp]
    n_mixed = fuse.use_mixed_precision(model, amp, kernels=not args.amp_cast_arm) if amp is not None else 0
    n_amp_conv32 = fuse.use_mixed_disp_conv(model, kernels=not args.amp_cast_arm) if getattr(args, "amp_conv32", False) else 0
    n_cl = fuse.use_channels_last(model.eval()) if args.channels_last else 0

    def clock():
        torch.cuda.synchronize()
        return time.perf_counter()

    t0 = clock()
    if args.host_io:
        l, r, hw = host_front(left, right, crop)
        l, r = torch.from_numpy(l).to(dev), torch.from_numpy(r).to(dev)
    else:
        from ganet_amd.modules.fused import DisparityOutput, StereoInput
        l, r, hw = StereoInput(*crop)(torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev))
    t1 = clock()
    pred = steps.predict(model, l, r, amp)
    t2 = clock()
    if args.host_io:
        u16 = host_back(pred.cpu().numpy(), hw)
    else:
        u16 = DisparityOutput()(pred, hw).cpu().numpy()
    t3 = time.perf_counter()
    write_disparity(args.out, u16)
    print(json.dumps({
        "what": "one stereo pair, image files to 16-bit disparity image", "model": args.model, "image": list(left.shape),
        "crop": list(crop), "max_disp": args.max_disp, "out": args.out, "out_shape": list(u16.shape),
        "io": "host numpy (predict.py's order of work)" if args.host_io else "ganet_amd.modules.fused.StereoInput / DisparityOutput",
        "ops": "ganet_amd.modules.fused (%d call sites)" % n_fused if args.fused else "drop-in call forms (libs/)",
        "fused_bn": "BnRelu (%d call sites)" % n_fused_bn if args.fused_bn else False,
        "amp": ("%s, %s (%d call sites)" % (args.amp, "cast arm" if args.amp_cast_arm else "16-bit-storage kernels", n_mixed)) if amp is not None else None,
        "amp_conv32": "MixedDispConv (%d call sites)" % n_amp_conv32 if n_amp_conv32 else False,
        "channels_last": "ClBnRelu / ClGetCostVolume (%d call sites)" % n_cl if n_cl else False,
        "dtype": ("%s convolutions under autocast, f32 guided aggregation and tails" % args.amp) if amp is not None else "f32",
        "ms_io_front": round(1e3 * (t1 - t0), 3), "ms_model_first_call": round(1e3 * (t2 - t1), 3), "ms_io_back": round(1e3 * (t3 - t2), 3),
        "weights": args.resume or "random init", "disp_u16_range": [int(u16.min()), int(u16.max())],
        "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
