"""The image front and back end (ganet_amd/csrc/io_kernels.h: ganet_stereo_input_workspace / _stats / _apply, ganet_window_f32,
ganet_disparity_to_u16) on the CPU emulator build: the case table of tests/io_cases.py (tests/test_gpu_io.py runs the same table
on the device), every case in both guard modes -- each tensor ENDS at an inaccessible page, resp. BEGINS right behind one --
against the statement of tests/io_ref64.py, which the first tests here tie to the reference's host chain restated in numpy."""
import os

import numpy as np
import pytest

import io_cases as ic
import io_ref64 as ref
import parity_cases as pc

F32 = np.float32


@pytest.fixture(scope="module")
def sim():
    from sim_util import sim_api
    return sim_api()


@pytest.fixture(params=["end", "start"])
def dev(request):
    return pc.NumpyDev(request.param)


# ---- the yardstick and the table ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ic.IMAGE_CASES, ids=repr)
def test_table_keeps_its_margin(case):
    """no quotient of the table within 2^-40 (relative) of a float32 rounding boundary: equality is the bar everywhere"""
    assert ref.margin(case.left, case.right) >= ref.MARGIN and case.tries <= 4, (case.name, case.tries)


@pytest.mark.parametrize("case", ic.IMAGE_CASES, ids=repr)
def test_statement_equals_the_host_chain(case):
    """(a) against (b): the reference's numpy standardisation, windowed, is the statement bit for bit -- except on a constant
    channel, where the host chain has NaN (0 / 0) wherever the image lands and the statement 0: the first deviation"""
    data = ref.host_load(case.left, case.right)
    for k, (img, ox, want) in enumerate(zip((case.left, case.right), (case.ox_left, case.ox_right), case.ref)):
        host = ref.place(data[3 * k:3 * k + 3], case.Hc, case.Wc, case.oy, ox)
        covered = ref.place(np.ones((1, case.H, case.W), bool), case.Hc, case.Wc, case.oy, ox, False)[0]
        N, S1, S2 = ref.sums(img)
        for c in range(3):
            if N * S2[c] == S1[c] ** 2:
                assert np.isnan(host[c][covered]).all() and not host[c][~covered].any() and not want[c].any()
            else:
                assert np.array_equal(ic.bits(host[c]), ic.bits(want[c])), (case.name, k, c)


@pytest.mark.parametrize("hw,crop", [((5, 7), (8, 12)), ((33, 65), (40, 68)), ((33, 65), (33, 65)), ((33, 65), (16, 32)), ((34, 66), (17, 31))])
def test_offsets_are_the_references_transform(hw, crop):
    """predict.py:75-90 on the host chain against the statement's (oy, ox); :132-138 un-pads with the same pair"""
    rng = np.random.default_rng(3)
    left, right = (rng.integers(0, 256, hw + (3,)).astype(np.uint8) for _ in range(2))
    hl, hr, h, w = ref.host_test_transform(ref.host_load(left, right), *crop)
    oy, ox = ref.predict_offsets(*hw, *crop)
    sl, sr = ref.stereo_input(left, right, *crop, oy, ox, ox)
    assert (h, w) == hw and np.array_equal(ic.bits(hl[0]), ic.bits(sl)) and np.array_equal(ic.bits(hr[0]), ic.bits(sr))
    pred = rng.uniform(0, 192, (1,) + crop).astype(F32)
    if h <= crop[0]:
        assert np.array_equal(ref.host_output(pred, h, w), ref.disparity_u16(pred[0], h, w, -oy, -ox, 256.0))
    else:
        assert np.array_equal(ref.host_output(pred, h, w), ref.disparity_u16(pred[0], *crop, 0, 0, 256.0))
    for bad in ((50, 60), (30, 70)):
        with pytest.raises(ValueError):
            ref.predict_offsets(*bad, 40, 68)


@pytest.mark.parametrize("shift_x", [-2, 0, 1])
def test_training_crop_is_a_window(shift_x):
    """dataloader/dataset.py:58-74: the crop of the padded arrays is the window (start_y - pad_y, start_x - pad_x [+ shift_x]) of
    the images, and `target - shift_x` on the 1000-filled target is sub = shift_x, fill = 1000 - shift_x"""
    rng = np.random.default_rng(4)
    h, w, Hc, Wc, shift, sy, sx = 9, 14, 12, 16, 3, 1, 2      # 0 <= sx + shift_x <= shift: dataset.py:67 keeps shift_x
    left, right = (rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(2))
    target = rng.uniform(0, 192, (h, w)).astype(F32)
    hl, hr, ht = ref.host_train_crop(ref.host_load(left, right), target, Hc, Wc, shift, sy, sx, shift_x)
    oy, ox = sy - (Hc + shift - h), sx - (Wc + shift - w)
    sl, sr = ref.stereo_input(left, right, Hc, Wc, oy, ox + shift_x, ox)
    assert np.array_equal(ic.bits(hl), ic.bits(sl)) and np.array_equal(ic.bits(hr), ic.bits(sr))
    assert np.array_equal(ic.bits(ht[0]), ic.bits(ref.window_f32(target, Hc, Wc, oy, ox + shift_x, shift_x, 1000 - shift_x)))


def test_back_end_deviates_only_outside_the_16_bit_range():
    """(temp * 256).astype('uint16') against the statement: equal for 0 <= p < 65536; below, above and on NaN the statement
    saturates (0 / 65535 / 0) -- the second deviation"""
    for c in ic.DISP_CASES:
        with np.errstate(all="ignore"):
            win = c.disp[c.oy:c.oy + c.h, c.ox:c.ox + c.w]
            p = win * F32(c.scale)
            inside = (p > -1) & (p < 65536)
            assert np.array_equal((win * c.scale).astype("uint16")[inside], c.ref[inside])
        assert (c.ref[p >= 65536] == 65535).all() and not c.ref[~(p > -1)].any()
    c = ic.DISP_CASES[0]
    assert {0, 1, 3, 255, 256, 65535}.issubset(set(c.ref.ravel().tolist())) and int((c.ref == 65535).sum()) >= 4
    assert ref.disparity_u16(np.array([[np.nextafter(F32(1 / 256), F32(0))]], F32), 1, 1, 0, 0, 256.0)[0, 0] == 0


def test_integer_variance_keeps_what_float64_loses():
    """4096 x 4096, all 255 but one pixel of 254: N S2 - S1^2 = N - 1 exactly; sum v^2 / N - mean^2 in float64 is off by 2^-24
    of the variance, 2^-25 of std: half an ulp of float32, enough to move a rounded result"""
    N = 2 ** 24
    S1, S2 = 255 * N - 1, 65025 * N - 509
    assert N * S2 - S1 * S1 == N - 1 and N * S2 < 2 ** 64
    q = ref.quotients(N, S1, S2)
    var64 = np.float64(S2) / N - (np.float64(S1) / N) ** 2
    assert abs(var64 * N * N / (N - 1) - 1) > 2.0 ** -25 and abs(q[254] + 4096) < 1e-3 and abs(q[255] - 2.0 ** -12) < 1e-9


def test_case_table_reaches_what_it_claims():
    by = ic.IMAGES
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ganet_amd", "csrc", "io_kernels.h")).read()
    for k, v in (("IO_BLOCK", ic.BLOCK), ("IO_MAX_ROWS", ic.MAX_ROWS), ("IO_PIX_PER_BLOCK", ic.PIX_PER_BLOCK), ("IO_ROW", ic.ROW),
                 ("IO_MAX_BLOCKS", ic.MAX_BLOCKS)):
        assert f"constexpr int {k} = {v};" in hdr
    # second trips of every grid-stride loop
    assert by["pad-33x65-cp3"].stats_trips(wide=False) >= 2 and by["stats-trip2-513x512"].stats_trips(wide=True) >= 2
    assert ic.rows(513 * 512) == ic.MAX_ROWS and 513 * 512 * 3 % 16 == 0 and 513 * 512 % 16 == 0
    c = by["apply-trip2-scalar-257x257"]
    assert not c.vec_out and c.apply_trips() >= 2 and ic.blocks(c.Hc * c.Wc) > c.H * c.W        # more blocks than pixels
    c = by["apply-trip2-vec-257x1024"]
    assert c.vec_out and c.apply_trips() >= 2
    w = {c.name: c for c in ic.WINDOW_CASES}
    assert ic.trips(257 * 257, ic.blocks(257 * 257)) >= 2 and ic.trips(257 * 256, ic.blocks(257 * 256)) >= 2
    assert w["trip2-vec-257x1024"].Wc % 4 == 0 and w["trip2-scalar-257x257"].Wc % 4
    d = {c.name: c for c in ic.DISP_CASES}
    assert ic.trips(513 * 1025 // 8, ic.blocks(513 * 1025 // 8)) >= 2 and 513 * 1025 % 8 and d["trip2-scalar-257x257"].misalign == 2
    # 16-byte forms and their tails, also where the tensor ends at the guard page (sizes that are multiples of 16)
    for name, tail in (("exact-6x6-cp4", 4), ("exact-16x16-cp3", 0), ("exact-8x16-cp4", 0), ("stats-trip2-513x512", 0)):
        c = by[name]
        assert c.H * c.W * c.CP % 16 == 0 and c.H * c.W % 16 == tail
    assert 33 * 65 % 16 == 1 and 33 * 65 * 3 % 16 and 65 * 3 % 16 and 7 * 3 % 16 and 7 * 4 % 16      # tails; no row a multiple of 16 bytes
    # constant channels, and one beside two that are not
    for name in ("1x1", "1x2-same", "zeros-5x7", "ones-5x7-cp4"):
        assert not any(r.any() for r in by[name].ref)
    c = by["const1-33x65"]
    assert not c.ref[0][1].any() and c.ref[0][0].any() and c.ref[0][2].any()
    # windows: wholly outside on each side, partly outside, different offsets for the two images
    for name in ("window-above", "window-below", "window-left", "window-right"):
        assert not any(r.any() for r in by[name].ref)
    for name in ("window-top-left", "window-bottom-right"):
        r = by[name].ref[0][0]
        assert (r == 0).all(axis=1).any() and (r == 0).all(axis=0).any() and r.any()
    c = by["window-left-out-right-in"]
    assert c.ox_left != c.ox_right and not c.ref[0].any() and c.ref[1].any()
    assert by["shifted-33x65"].ox_left != by["shifted-33x65"].ox_right
    assert ref.predict_offsets(33, 65, 16, 32) == (8, 16) and (33 - 16) % 2 and (65 - 32) % 2
    assert set(np.unique(by["low-contrast-33x65"].left[..., :3])) == {100, 101, 102, 103}
    assert set(np.unique(by["two-level-33x65"].left)) == {0, 255}


# ---- the kernels ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ic.IMAGE_CASES, ids=repr)
def test_image_case(sim, dev, case):
    ic.check_image(case, ic.run_image(sim, dev, case))


@pytest.mark.parametrize("name", ["pad-33x65-cp3", "pad-5x7-cp4", "odd-crop-33x65", "const1-33x65", "window-top-left"])
def test_direct_form_gives_the_same_bits(sim, dev, name):
    ic.check_image(ic.IMAGES[name], ic.run_image(sim, dev, ic.IMAGES[name], form=1))


def test_both_forms_of_every_kernel_ran(sim):
    """the table reaches the 16-byte form and the twin of the statistics and of the apply pass in each guard mode"""
    seen = {"end": set(), "start": set()}
    for guard in seen:
        for name in ("exact-6x6-cp4", "exact-16x16-cp3", "pad-33x65-cp3", "base+1-33x65", "odd-crop-33x65"):
            got = ic.run_image(sim, pc.NumpyDev(guard), ic.IMAGES[name])
            seen[guard] |= {("wide", w) for w in got["wide"]} | {("vec", got["vec"])}
    for guard, s in seen.items():
        assert s == {("wide", True), ("wide", False), ("vec", True), ("vec", False)}, (guard, s)


@pytest.mark.parametrize("case", ic.WINDOW_CASES, ids=repr)
def test_window_case(sim, dev, case):
    ic.check_window(case, ic.run_window(sim, dev, case))


@pytest.mark.parametrize("case", ic.DISP_CASES, ids=repr)
def test_disp_case(sim, dev, case):
    ic.check_disp(case, ic.run_disp(sim, dev, case))


def test_bad_arguments(sim):
    ic.check_bad_arguments(sim, pc.NumpyDev())
