"""TEST INFRASTRUCTURE: the case table of the image front and back end (ganet_stereo_input_workspace / _stats / _apply,
ganet_window_f32, ganet_disparity_to_u16), shared by tests/test_sim_io.py (emulator build, guard pages) and tests/test_gpu_io.py
(gfx950 build, C ABI and modules).  `run_*(api, dev, case)` drive the C ABI on either build; `check_*` compare with the
statement (a) of tests/io_ref64.py -- bit for bit: every image of the table keeps its quotients at least io_ref64.MARGIN away
from a rounding boundary of float32 (`ImageCase` draws again until they do, tests/test_sim_io.py asserts that none is left), so
neither the few fp64 ulps between two ways of computing std nor anything smaller can excuse a differing bit.

Every device buffer is a byte buffer; tensors sit in it at a byte offset.  Emulator, guard="end": the tensor ENDS at the
inaccessible page (its front padding is what that takes, (-size) % 16 bytes, so the 16-byte forms run where the size is a
multiple of 16); guard="start" and the device: the tensor begins `misalign` bytes behind a 16-byte boundary."""
import numpy as np

import io_ref64 as ref

F32, U8 = np.float32, np.uint8
# ganet_amd/csrc/io_kernels.h: IO_BLOCK, IO_MAX_ROWS, IO_PIX_PER_BLOCK, IO_ROW, IO_MAX_BLOCKS
BLOCK, MAX_ROWS, PIX_PER_BLOCK, ROW, MAX_BLOCKS = 256, 64, 4096, 8, 256


def rows(pixels):
    """rows (blocks) per image as the launcher chooses them (ganet_capi.hip: io_rows)"""
    return min(MAX_ROWS, -(-pixels // PIX_PER_BLOCK))


def blocks(units):
    """ganet_capi.hip: io_blocks"""
    return max(1, min(MAX_BLOCKS, -(-units // BLOCK)))


def trips(units, nblocks):
    """trips of a grid-stride loop over `units` that the busiest lane makes"""
    return -(-units // (nblocks * BLOCK))


def fbits(v):
    return int(F32(v).view(np.int32))


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---- the front end's cases --------------------------------------------------------------------------------------------------

def _values(kind, rng, H, W):
    if kind == "uniform":
        return rng.integers(0, 256, (H, W, 3))
    if kind == "levels4":
        return rng.choice([3, 77, 130, 251], (H, W, 3))
    if kind == "two":
        return rng.choice([0, 255], (H, W, 3))
    if kind == "low":                                   # low contrast: 100 ... 103
        return rng.integers(100, 104, (H, W, 3))
    if kind == "zeros":
        return np.zeros((H, W, 3), np.int64)
    if kind == "ones":
        return np.full((H, W, 3), 255)
    if kind == "const1":                                # one channel constant beside two that are not
        a = rng.integers(0, 256, (H, W, 3))
        a[..., 1] = 91
        return a
    raise KeyError(kind)


class ImageCase:
    def __init__(self, name, hw, crop, offsets=None, CP=3, kind="uniform", misalign=(0, 0), out_misalign=0, seed=0):
        """offsets: (oy, ox_left, ox_right), default: the rule of predict.py:75-90.  misalign: bytes, per image; out_misalign:
        bytes, both outputs"""
        H, W = hw
        self.name, self.H, self.W, self.CP, self.kind = name, H, W, CP, kind
        self.Hc, self.Wc = crop
        if offsets is None:
            oy, ox = ref.predict_offsets(H, W, *crop)
            offsets = (oy, ox, ox)
        self.oy, self.ox_left, self.ox_right = offsets
        self.misalign, self.out_misalign = misalign, out_misalign
        self.tries = 0
        for k in range(16):                             # draw again until no quotient sits at a rounding boundary
            rng = np.random.default_rng(1000 * k + seed)
            imgs = []
            for _ in range(2):
                a = np.zeros((H, W, CP), U8)
                a[..., :3] = _values(kind, rng, H, W)
                if CP == 4:
                    a[..., 3] = rng.integers(0, 256, (H, W))    # a fourth byte nobody may look at
                imgs.append(a)
            self.left, self.right = imgs
            self.tries = k + 1
            if ref.margin(self.left, self.right) >= ref.MARGIN:
                break
        self._ref = None

    def __repr__(self):
        return self.name

    @property
    def ref(self):
        """(left_out, right_out) of the statement, computed once, shared by every test that runs the case"""
        if self._ref is None:
            self._ref = ref.stereo_input(self.left, self.right, self.Hc, self.Wc, self.oy, self.ox_left, self.ox_right)
        return self._ref

    @property
    def vec_out(self):
        return self.Wc % 4 == 0 and self.out_misalign % 16 == 0

    def apply_trips(self, vec=None):
        vec = self.vec_out if vec is None else vec
        units = self.Hc * (self.Wc // 4 if vec else self.Wc)
        return trips(units, blocks(units))

    def stats_trips(self, wide):
        n = self.H * self.W
        return trips(n // 16 if wide else n, rows(n))

    def poisoned(self, img, ox):
        """the image with every pixel outside the window inverted (and every fourth byte): the apply pass may not care"""
        a = img.copy()
        keep = np.zeros((self.H, self.W), bool)
        keep[max(0, self.oy):max(0, self.oy + self.Hc), max(0, ox):max(0, ox + self.Wc)] = True
        a[~keep] ^= 0xFF
        if self.CP == 4:
            a[..., 3] ^= 0x5A
        return a


def _image_cases():
    cs = []
    seed = [10]

    def add(name, hw, crop, offsets=None, **kw):
        seed[0] += 1
        cs.append(ImageCase(name, hw, crop, offsets, seed=seed[0], **kw))

    # constant channels: one pixel, two equal pixels, all 0, all 255
    add("1x1", (1, 1), (3, 5))
    add("1x2-same", (1, 2), (1, 2), kind="ones")
    add("zeros-5x7", (5, 7), (8, 8), kind="zeros")
    add("ones-5x7-cp4", (5, 7), (5, 7), kind="ones", CP=4)
    add("const1-33x65", (33, 65), (40, 68), kind="const1")
    # the two pixel strides, the 16-byte forms and their twins.  5x7 and 33x65: no row, no image a multiple of 16 bytes
    add("pad-5x7-cp3", (5, 7), (8, 12))
    add("pad-5x7-cp4", (5, 7), (8, 12), CP=4)
    add("pad-33x65-cp3", (33, 65), (40, 68))
    add("pad-33x65-cp4", (33, 65), (40, 68), CP=4)
    add("exact-6x6-cp4", (6, 6), (6, 6), CP=4)                    # 144 bytes: 2 units of 16 pixels and a tail of 4
    add("exact-16x16-cp3", (16, 16), (16, 16))                    # 768 bytes: whole units
    add("exact-8x16-cp4", (8, 16), (8, 16), CP=4)
    for k in (1, 2, 3):
        add(f"base+{k}-33x65", (33, 65), (40, 68), misalign=(k, 0) if k != 2 else (0, 2))
    add("base+3+1-5x7-cp4", (5, 7), (8, 8), CP=4, misalign=(3, 1))
    add("out+4-33x65", (33, 65), (40, 68), out_misalign=4)        # a slice of a batch tensor one float behind a boundary
    add("odd-crop-33x65", (33, 65), (37, 67))                     # Wc % 4 != 0: the scalar stores
    # windows
    add("centre-crop-odd-33x65", (33, 65), (16, 32))              # (33 - 16) / 2 = 8.5, (65 - 32) / 2 = 16.5
    add("centre-crop-odd-cp4", (33, 65), (20, 36), CP=4)
    add("shifted-33x65", (33, 65), (16, 32), (5, 9, 2))           # ox_left != ox_right, inside
    for name, off in (("above", (-50, 3, 3)), ("below", (40, 3, 3)), ("left", (3, -70, -70)), ("right", (3, 70, 70)),
                      ("top-left", (-4, -6, -2)), ("bottom-right", (25, 50, 57)), ("left-out-right-in", (2, -40, 10))):
        add("window-" + name, (33, 65), (16, 32), off)
    # values
    add("two-level-33x65", (33, 65), (40, 68), kind="two")
    add("four-level-33x65-cp4", (33, 65), (40, 68), kind="levels4", CP=4)
    add("low-contrast-33x65", (33, 65), (40, 68), kind="low")
    # second trips.  statistics: the byte-wise twin beyond rows x 256 pixels (33x65 above: 1 row), the wide form beyond 64 rows x
    # 4,096 pixels; apply: more than 256 blocks x 256 lanes of output, which is also far more blocks than the image has pixels
    add("stats-trip2-513x512", (513, 512), (8, 8), (250, 250, 251))
    add("apply-trip2-scalar-257x257", (5, 7), (257, 257))
    add("apply-trip2-vec-257x1024", (33, 65), (257, 1024), CP=4)
    return cs


IMAGE_CASES = _image_cases()
IMAGES = {c.name: c for c in IMAGE_CASES}


# ---- buffers ----------------------------------------------------------------------------------------------------------------

FRONT = 0xA5


def _front(dev, nbytes, misalign):
    return (-nbytes) % 16 if getattr(dev, "guard", None) == "end" else misalign


def put(dev, a, misalign=0):
    """(buffer, address, bytes in front) of a copy of `a`"""
    raw = np.ascontiguousarray(a).view(U8).ravel()
    front = _front(dev, raw.size, misalign)
    buf = dev.to(np.concatenate([np.full(front, FRONT, U8), raw]))
    return buf, dev.ptr(buf) + front, front


def out(dev, nbytes, misalign=0):
    """a poisoned output buffer (every byte 113)"""
    front = _front(dev, nbytes, misalign)
    buf = dev.empty((front + nbytes,), U8)
    return buf, dev.ptr(buf) + front, front


def fetch(dev, buf, front, dtype, shape, what):
    raw = np.array(dev.host(buf)).view(U8)
    assert (raw[:front] == (113 if what.startswith("out") else FRONT)).all(), f"{what}: written in front of the tensor"
    return raw[front:].view(dtype).reshape(shape).copy()


def workspace(api, dev, case):
    n = api.query("ganet_stereo_input_workspace", case.H, case.W, case.CP)
    assert n == 2 * MAX_ROWS * ROW
    return out(dev, 8 * n)


def run_image(api, dev, case, form=0, poison=True):
    """statistics, then the apply pass -- on copies of the images whose pixels outside the window are inverted (poison): the
    output may depend on them through the statistics only"""
    lb, lp, lf = put(dev, case.left, case.misalign[0])
    rb, rp, rf = put(dev, case.right, case.misalign[1])
    wb, wp, _ = workspace(api, dev, case)
    api.call("ganet_stereo_input_stats", lp, rp, wp, case.H, case.W, case.CP, dev.stream)
    if poison:
        lb2, lp2, _ = put(dev, case.poisoned(case.left, case.ox_left), case.misalign[0])
        rb2, rp2, _ = put(dev, case.poisoned(case.right, case.ox_right), case.misalign[1])
    else:
        lp2, rp2 = lp, rp
    n = 3 * case.Hc * case.Wc
    lob, lop, lof = out(dev, 4 * n, case.out_misalign)
    rob, rop, rof = out(dev, 4 * n, case.out_misalign)
    api.call("ganet_stereo_input_apply", lp2, rp2, wp, lop, rop, case.H, case.W, case.CP, case.Hc, case.Wc, case.oy, case.ox_left,
             case.ox_right, form, dev.stream)
    dev.sync()
    shape = (3, case.Hc, case.Wc)
    got = {"left": fetch(dev, lob, lof, F32, shape, "out left"), "right": fetch(dev, rob, rof, F32, shape, "out right"),
           "ws": fetch(dev, wb, 0, np.uint64, (2 * MAX_ROWS, ROW), "out workspace"),
           "wide": tuple((p % 16) == 0 for p in (lp, rp)), "vec": case.Wc % 4 == 0 and lop % 16 == 0 and rop % 16 == 0}
    assert np.array_equal(fetch(dev, lb, lf, U8, case.left.shape, "left"), case.left), "the left image was written"
    assert np.array_equal(fetch(dev, rb, rf, U8, case.right.shape, "right"), case.right), "the right image was written"
    return got


def check_image(case, got):
    """the workspace rows add up to the integer sums; both outputs equal the statement bit for bit"""
    R = rows(case.H * case.W)
    for k, img in enumerate((case.left, case.right)):
        _, S1, S2 = ref.sums(img)
        tot = [int(v) for v in got["ws"][k * R:(k + 1) * R, :6].astype(object).sum(axis=0)]
        assert tot == S1 + S2, (case.name, k, tot, S1 + S2)
    for key, want in zip(("left", "right"), case.ref):
        diff = bits(got[key]) != bits(want)
        assert not diff.any(), f"{case.name} {key}: {int(diff.sum())} of {diff.size} differ, first at {np.argwhere(diff)[0]}"


# ---- the float window -------------------------------------------------------------------------------------------------------

class WindowCase:
    def __init__(self, name, hw, crop, oy, ox, sub=0.0, fill=1000.0, misalign=0, seed=0):
        self.name, self.Hc, self.Wc, self.oy, self.ox, self.sub, self.fill, self.misalign = name, crop[0], crop[1], oy, ox, sub, fill, misalign
        self.src = (np.random.default_rng(seed).uniform(0, 192, hw)).astype(F32)
        self.ref = ref.window_f32(self.src, self.Hc, self.Wc, oy, ox, sub, fill)

    def __repr__(self):
        return self.name


WINDOW_CASES = [
    WindowCase("pad-5x7", (5, 7), (8, 12), -3, -5, seed=1),
    WindowCase("inside-sub-33x65", (33, 65), (16, 32), 5, 9, sub=7.0, fill=993.0, seed=2),
    WindowCase("partly-out-sub-33x65", (33, 65), (16, 32), 25, -6, sub=-3.0, fill=1003.0, seed=3),
    WindowCase("outside-33x65", (33, 65), (16, 32), 3, 70, seed=4),
    WindowCase("odd-33x65", (33, 65), (37, 67), -4, -2, sub=0.5, seed=5),
    WindowCase("dst+4-33x65", (33, 65), (40, 68), -7, -3, misalign=4, seed=6),
    WindowCase("trip2-scalar-257x257", (5, 7), (257, 257), -252, -250, sub=1.0, seed=7),
    WindowCase("trip2-vec-257x1024", (33, 65), (257, 1024), -10, -900, sub=2.0, seed=8),
]


def run_window(api, dev, c):
    sb, sp, sf = put(dev, c.src)
    ob, op, of = out(dev, 4 * c.Hc * c.Wc, c.misalign)
    api.call("ganet_window_f32", sp, op, c.src.shape[0], c.src.shape[1], c.Hc, c.Wc, c.oy, c.ox, fbits(c.sub), fbits(c.fill), dev.stream)
    dev.sync()
    assert np.array_equal(bits(fetch(dev, sb, sf, F32, c.src.shape, "src")), bits(c.src))
    return fetch(dev, ob, of, F32, (c.Hc, c.Wc), "out window")


def check_window(c, got):
    assert np.array_equal(bits(got), bits(c.ref)), c.name


# ---- the back end -----------------------------------------------------------------------------------------------------------

SPECIAL = [0.0, -0.0, float(np.nextafter(F32(1 / 256), F32(0))), 1 / 256, 3 / 256, 255 / 256, 1.0, 100.5, 191.99609375,
           65535 / 256, float(np.nextafter(F32(256), F32(0))), 256.0, 300.0, -0.5, -1e-30, -3.0, float("nan"), float("inf"), float("-inf")]


class DispCase:
    def __init__(self, name, map_hw, hw, oy, ox, misalign=0, scale=256.0, seed=0):
        self.name, self.h, self.w, self.oy, self.ox, self.misalign, self.scale = name, hw[0], hw[1], oy, ox, misalign, scale
        rng = np.random.default_rng(seed)
        d = rng.uniform(0, 192, map_hw).astype(F32)
        idx = rng.permutation(self.h * self.w)[:len(SPECIAL)]
        for i, v in zip(idx, SPECIAL):                           # the special values inside the window, wherever they fall
            d[oy + i // self.w, ox + i % self.w] = v
        self.disp = d
        self.ref = ref.disparity_u16(d, self.h, self.w, oy, ox, scale)

    def __repr__(self):
        return self.name


DISP_CASES = [
    DispCase("whole-5x7", (5, 7), (5, 7), 0, 0, seed=1),                      # 35 values: 4 packs of 8 and a tail of 3
    DispCase("unpad-odd-w-40x68", (40, 68), (33, 65), 7, 3, seed=2),
    DispCase("out+2-40x68", (40, 68), (33, 65), 7, 3, misalign=2, seed=3),    # a 2-byte offset: the scalar stores
    DispCase("crop-offsets-40x68", (40, 68), (16, 24), 11, 19, seed=4),
    DispCase("tiny-1x1", (3, 3), (1, 1), 1, 2, seed=5),
    DispCase("scale-1-9x9", (9, 9), (9, 9), 0, 0, scale=1.0, seed=6),
    DispCase("trip2-scalar-257x257", (257, 259), (257, 257), 0, 2, misalign=2, seed=7),
    DispCase("trip2-vec-513x1025", (515, 1030), (513, 1025), 2, 5, seed=8),
]


def run_disp(api, dev, c):
    db, dp, df = put(dev, c.disp)
    ob, op, of = out(dev, 2 * c.h * c.w, c.misalign)
    api.call("ganet_disparity_to_u16", dp, op, c.disp.shape[0], c.disp.shape[1], c.h, c.w, c.oy, c.ox, fbits(c.scale), dev.stream)
    dev.sync()
    assert np.array_equal(bits(fetch(dev, db, df, F32, c.disp.shape, "disp")), bits(c.disp))
    return fetch(dev, ob, of, np.uint16, (c.h, c.w), "out u16")


def check_disp(c, got):
    assert np.array_equal(got, c.ref), (c.name, np.argwhere(got != c.ref)[:4])


# ---- argument errors --------------------------------------------------------------------------------------------------------

def check_bad_arguments(api, dev):
    import pytest
    from ganet_amd._native import E_INVALID, GanetError
    c = IMAGES["pad-5x7-cp3"]
    (_, lp, _), (_, rp, _), (_, wp, _) = keep = put(dev, c.left), put(dev, c.right), workspace(api, dev, c)
    n = 3 * c.Hc * c.Wc
    (_, lop, _), (_, rop, _) = keep2 = out(dev, 4 * n), out(dev, 4 * n)

    def stats(l=lp, r=rp, w=wp, dims=(c.H, c.W, c.CP)):
        api.call("ganet_stereo_input_stats", l, r, w, *dims, dev.stream)

    def apply(l=lp, r=rp, w=wp, lo=lop, ro=rop, dims=(c.H, c.W, c.CP), crop=(c.Hc, c.Wc), form=0):
        api.call("ganet_stereo_input_apply", l, r, w, lo, ro, *dims, *crop, c.oy, c.ox_left, c.ox_right, form, dev.stream)

    stats()
    apply()
    bad_dims = [(c.H, c.W, 2), (c.H, c.W, 5), (0, c.W, 3), (c.H, -1, 3), (4097, 4096, 3)]
    for call, kws in ((stats, [dict(l=None), dict(r=None), dict(w=None)] + [dict(dims=d) for d in bad_dims]),
                      (apply, [dict(l=None), dict(r=None), dict(w=None), dict(lo=None), dict(ro=None), dict(crop=(0, 4)),
                               dict(crop=(4, -4)), dict(form=2)] + [dict(dims=d) for d in bad_dims])):
        for kw in kws:
            with pytest.raises(GanetError) as e:
                call(**kw)
            assert e.value.code == E_INVALID and "ganet_stereo_input" in str(e.value), kw
    for dims in bad_dims:
        with pytest.raises(GanetError) as e:
            api.query("ganet_stereo_input_workspace", *dims)
        assert e.value.code == E_INVALID
    assert api.query("ganet_stereo_input_workspace", 4096, 4096, 4) == 2 * MAX_ROWS * ROW
    w = WINDOW_CASES[0]
    (_, sp, _), (_, op, _) = keep3 = put(dev, w.src), out(dev, 4 * w.Hc * w.Wc)
    for args in ((None, op, 5, 7, 8, 12), (sp, None, 5, 7, 8, 12), (sp, sp, 5, 7, 8, 12), (sp, op, 0, 7, 8, 12), (sp, op, 5, 7, 8, 0)):
        with pytest.raises(GanetError) as e:
            api.call("ganet_window_f32", *args, 0, 0, fbits(0), fbits(0), dev.stream)
        assert e.value.code == E_INVALID and "ganet_window_f32" in api.last_error()
    d = DISP_CASES[0]
    (_, dp, _), (_, up, _) = keep4 = put(dev, d.disp), out(dev, 2 * d.h * d.w)
    for args in ((None, up, 5, 7, 5, 7, 0, 0), (dp, None, 5, 7, 5, 7, 0, 0), (dp, up, 5, 7, 5, 7, 1, 0), (dp, up, 5, 7, 5, 7, 0, 1),
                 (dp, up, 5, 7, 5, 7, -1, 0), (dp, up, 5, 7, 0, 7, 0, 0), (dp, up, 5, 7, 6, 7, 0, 0)):
        with pytest.raises(GanetError) as e:
            api.call("ganet_disparity_to_u16", *args, fbits(256), dev.stream)
        assert e.value.code == E_INVALID and "ganet_disparity_to_u16" in api.last_error()
    dev.sync()
    del keep, keep2, keep3, keep4
