"""TEST INFRASTRUCTURE: the image front and back end (ganet_amd/csrc/io_kernels.h: ganet_stereo_input_* / ganet_window_f32 /
ganet_disparity_to_u16) stated three times over.

(a) THE STATEMENT: the procedure of io_kernels.h's header in Python integers and numpy float64 -- integer sums, the variance's
    numerator N S2 - S1^2 as an integer, mean and std from one fp64 operation each, the 256 results of a channel rounded to
    float32 once.  The kernels are held to it bit for bit.
(b) THE HOST CHAIN: what the reference does on the host, restated from scratch: predict.py:92-114 (each of the six channels
    `(r - np.mean(r)) / np.std(r)`, float64 temporaries stored into a float32 array), :75-90 (pad to the bottom-right, else
    centre-crop), :132-138 (un-pad, `(temp * 256).astype('uint16')`) and dataloader/dataset.py:48-92 (the training crop on the
    padded arrays, the target filled with 1000 and lowered by shift_x).  It differs from (a) in two places, both deliberate:
    a constant channel is NaN here (0 / 0) and 0 in (a); values outside [0, 65536) wrap in astype and saturate in (a).
(c) margin: (a) and (b) share the mean (an exact integer sum over N in both) and differ in std by a few fp64 ulps (numpy sums
    the squared deviations in float64, (a) takes the square root of an exact quotient).  A relative change of std of 2^-50 moves
    a quotient q by 2^-50 |q|; it changes float32(q) only if q lies that close to a rounding boundary of float32.  margin()
    is the smallest relative distance of an occurring quotient from such a boundary: above 2^-40 the float32 results of (a),
    (b) and of any kernel whose std is within a thousand ulps are EQUAL, and the tests ask for equality."""
import numpy as np

F32, F64 = np.float32, np.float64
MARGIN = 2.0 ** -40


# ---- (a) the statement ------------------------------------------------------------------------------------------------------

def sums(img):
    """N, S1[3], S2[3] as Python integers; img uint8 [H, W, CP], the first three bytes of a pixel are its channels"""
    a = np.asarray(img)[..., :3].reshape(-1, 3).astype(np.int64)
    return a.shape[0], [int(v) for v in a.sum(axis=0)], [int(v) for v in (a * a).sum(axis=0)]


def quotients(N, S1, S2):
    """the 256 float64 quotients of one channel, or None for a constant channel"""
    num = N * S2 - S1 * S1
    assert 0 <= num < 2 ** 64 and N <= 2 ** 24
    if num == 0:
        return None
    mean = F64(S1) / F64(N)
    std = np.sqrt(F64(num) / (F64(N) * F64(N)))
    return (np.arange(256, dtype=F64) - mean) / std


def table(img):
    """[3, 256] float32: the result for every byte value, per channel"""
    N, S1, S2 = sums(img)
    out = np.zeros((3, 256), F32)
    for c in range(3):
        q = quotients(N, S1[c], S2[c])
        if q is not None:
            out[c] = q.astype(F32)
    return out


def standardise(img):
    """[3, H, W] float32"""
    t = table(img)
    a = np.asarray(img)
    return np.stack([t[c][a[..., c]] for c in range(3)])


def place(planes, Hc, Wc, oy, ox, fill=0.0):
    """out[..., y, x] = planes[..., y + oy, x + ox] where that lies inside, else fill"""
    planes = np.asarray(planes)
    H, W = planes.shape[-2:]
    out = np.full(planes.shape[:-2] + (Hc, Wc), fill, planes.dtype)
    y0, y1, x0, x1 = max(0, -oy), min(Hc, H - oy), max(0, -ox), min(Wc, W - ox)
    if y0 < y1 and x0 < x1:
        out[..., y0:y1, x0:x1] = planes[..., y0 + oy:y1 + oy, x0 + ox:x1 + ox]
    return out


def stereo_input(left, right, Hc, Wc, oy, ox_left, ox_right):
    return place(standardise(left), Hc, Wc, oy, ox_left), place(standardise(right), Hc, Wc, oy, ox_right)


def predict_offsets(h, w, Hc, Wc):
    """(oy, ox) of predict.py:75-90: an image no larger than the crop goes to the bottom-right corner, one larger both ways is
    centre-cropped; the reference's slice arithmetic breaks on any other mix"""
    if h <= Hc and w <= Wc:
        return h - Hc, w - Wc
    if h > Hc and w > Wc:
        return int((h - Hc) / 2), int((w - Wc) / 2)
    raise ValueError("image larger than the crop one way and not the other")


def window_f32(src, Hc, Wc, oy, ox, sub, fill):
    src = np.asarray(src, F32)
    return place(src - F32(sub), Hc, Wc, oy, ox, F32(fill))


def disparity_u16(disp, h, w, oy, ox, scale):
    with np.errstate(all="ignore"):
        p = np.asarray(disp, F32)[oy:oy + h, ox:ox + w] * F32(scale)
        out = np.zeros(p.shape, np.uint16)
        mid = (p >= 0) & (p < 65536)
        out[mid] = np.trunc(p[mid]).astype(np.uint16)
        out[p >= 65536] = 65535
    return out


# ---- (b) the host chain -----------------------------------------------------------------------------------------------------

def host_load(left, right):
    """predict.py:92-114: [6, H, W] float32"""
    H, W = np.shape(left)[:2]
    data = np.zeros([6, H, W], "float32")
    with np.errstate(all="ignore"):
        for k, img in enumerate((np.asarray(left), np.asarray(right))):
            for c in range(3):
                ch = img[:, :, c]
                data[3 * k + c] = (ch - np.mean(ch)) / np.std(ch)
    return data


def host_test_transform(data, Hc, Wc):
    """predict.py:75-90: left, right [1, 3, Hc, Wc] float32 and the image's size"""
    h, w = data.shape[1:]
    if h <= Hc and w <= Wc:
        canvas = np.zeros([6, Hc, Wc], "float32")
        canvas[:, Hc - h:, Wc - w:] = data
    else:
        x0, y0 = int((w - Wc) / 2), int((h - Hc) / 2)
        canvas = data[:, y0:y0 + Hc, x0:x0 + Wc]
    return canvas[None, 0:3].copy(), canvas[None, 3:6].copy(), h, w


def host_output(pred, h, w, scale=256):
    """predict.py:132-138: pred [1, Hc, Wc] float32 -> uint16 [h, w] (or the whole map where the image was cropped)"""
    Hc, Wc = pred.shape[1:]
    temp = pred[0, Hc - h:, Wc - w:] if h <= Hc and w <= Wc else pred[0]
    with np.errstate(all="ignore"):
        return (temp * scale).astype("uint16")


def host_train_crop(data, target, Hc, Wc, shift, start_y, start_x, shift_x):
    """dataloader/dataset.py:58-74 for an image no larger than the crop and shift > 0, the three random draws given: the six
    channels and the target are padded to [Hc + shift, Wc + shift] (bottom-right, the target with 1000), then cropped -- the
    left image and the target shift_x further right -- and the target lowered by shift_x"""
    h, w = data.shape[1:]
    canvas = np.zeros([7, Hc + shift, Wc + shift], "float32")
    canvas[6] = 1000
    canvas[:6, Hc + shift - h:, Wc + shift - w:] = data
    canvas[6, Hc + shift - h:, Wc + shift - w:] = target
    ys, xr, xl = slice(start_y, start_y + Hc), slice(start_x, start_x + Wc), slice(start_x + shift_x, start_x + shift_x + Wc)
    return canvas[0:3, ys, xl], canvas[3:6, ys, xr], canvas[6:7, ys, xl] - shift_x


# ---- (c) the margin ---------------------------------------------------------------------------------------------------------

def margin(*images):
    """the smallest relative distance of an occurring quotient (every byte value that occurs in a channel of one of the images)
    from a rounding boundary of float32 -- the midpoint of two neighbouring float32 values.  A quotient of exactly 0 stays 0
    whatever std is and does not count; constant channels have no quotients."""
    worst = np.inf
    for img in images:
        N, S1, S2 = sums(img)
        for c in range(3):
            q = quotients(N, S1[c], S2[c])
            if q is None:
                continue
            q = q[np.unique(np.asarray(img)[..., c])]
            q = q[q != 0]
            f = q.astype(F32)
            lo = (f.astype(F64) + np.nextafter(f, F32(-np.inf)).astype(F64)) / 2
            hi = (f.astype(F64) + np.nextafter(f, F32(np.inf)).astype(F64)) / 2
            assert (lo <= q).all() and (q <= hi).all()
            d = np.minimum(q - lo, hi - q) / np.abs(q)
            worst = min(worst, float(d.min(initial=np.inf)))
    return worst
