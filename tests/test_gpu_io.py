"""The image front and back end on the gfx950 build: the case table of tests/io_cases.py through the C ABI (tests/test_sim_io.py
runs it on the emulator) -- same inputs, same statement, equality as the bar -- and, device only: through the functions and
modules of ganet_amd (StereoInput, DisparityOutput), the integer sums at the edge of 64 bits on 4096 x 4096 images, graph
capture, no host synchronisation, a side stream, and harness.steps.predict_images on a stand-in model against the host
pipeline of the reference restated in tests/io_ref64.py."""
import numpy as np
import pytest

import io_cases as ic
import io_ref64 as ref
from test_gpu_parity import TorchDev

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def api():
    from ganet_amd import _native
    lib = _native.lib()
    assert not lib.is_simulator, "GPU tests must run the gfx950 build"
    assert lib.path.endswith("ganet_amd/libganet_hip.so")
    return lib


@pytest.fixture(scope="module")
def dev():
    return TorchDev()


def host(t):
    return t.detach().cpu().numpy()


# ---- C ABI: the shared table ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ic.IMAGE_CASES, ids=repr)
def test_image_case(api, dev, case):
    got = ic.run_image(api, dev, case)
    assert got["wide"] == tuple(m % 16 == 0 for m in case.misalign) and got["vec"] == case.vec_out
    ic.check_image(case, got)


@pytest.mark.parametrize("name", ["pad-33x65-cp3", "pad-5x7-cp4", "odd-crop-33x65", "const1-33x65", "window-top-left"])
def test_direct_form_gives_the_same_bits(api, dev, name):
    ic.check_image(ic.IMAGES[name], ic.run_image(api, dev, ic.IMAGES[name], form=1))


@pytest.mark.parametrize("case", ic.WINDOW_CASES, ids=repr)
def test_window_case(api, dev, case):
    ic.check_window(case, ic.run_window(api, dev, case))


@pytest.mark.parametrize("case", ic.DISP_CASES, ids=repr)
def test_disp_case(api, dev, case):
    ic.check_disp(case, ic.run_disp(api, dev, case))


def test_bad_arguments(api, dev):
    ic.check_bad_arguments(api, dev)


def test_sums_at_the_edge_of_64_bits(api, dev):
    """4096 x 4096 = 2^24 pixels, the limit.  Left: all 255 but one pixel of 254 -- N S2 and S1^2 just under 2^64, their
    difference N - 1, a variance that sum v^2 / N - mean^2 in float64 gets wrong by half a float32 ulp of std.  Right: half 0,
    half 255 -- N S2 - S1^2 = 2^62 (255 / 2)^2 ... the largest numerator there is.  Both equal to the statement."""
    import torch
    n, N = 4096, 2 ** 24
    left = torch.full((n, n, 3), 255, dtype=torch.uint8, device=dev.device)
    left[1234, 2345, :] = 254
    right = torch.zeros((n, n, 4), dtype=torch.uint8, device=dev.device)
    right[n // 2:, :, :3] = 255
    right = right[:, :, :3].contiguous()
    sums = {"left": ([255 * N - 1] * 3, [65025 * N - 509] * 3), "right": ([255 * N // 2] * 3, [65025 * N // 2] * 3)}
    assert N * sums["left"][1][0] - sums["left"][0][0] ** 2 == N - 1 and N * sums["left"][1][0] > 2 ** 63
    nws = api.query("ganet_stereo_input_workspace", n, n, 3)
    ws = torch.zeros(nws, dtype=torch.int64, device=dev.device)
    Hc, Wc, oy, oxl, oxr = 8, 12, 1230, 2340, 2341
    lo, ro = (torch.full((3, Hc, Wc), float("nan"), device=dev.device) for _ in range(2))
    st = torch.cuda.current_stream().cuda_stream
    api.call("ganet_stereo_input_stats", left.data_ptr(), right.data_ptr(), ws.data_ptr(), n, n, 3, st)
    api.call("ganet_stereo_input_apply", left.data_ptr(), right.data_ptr(), ws.data_ptr(), lo.data_ptr(), ro.data_ptr(), n, n, 3,
             Hc, Wc, oy, oxl, oxr, 0, st)
    lo2, ro2 = (torch.full((3, Hc, Wc), float("nan"), device=dev.device) for _ in range(2))
    api.call("ganet_stereo_input_apply", left.data_ptr(), right.data_ptr(), ws.data_ptr(), lo2.data_ptr(), ro2.data_ptr(), n, n, 3,
             Hc, Wc, 2044, oxl, oxr, 0, st)                         # the right image's window across its 0 / 255 edge
    torch.cuda.synchronize()
    rows = host(ws).view(np.uint64).reshape(2 * ic.MAX_ROWS, ic.ROW)
    for k, key in enumerate(("left", "right")):
        tot = [int(v) for v in rows[k * ic.MAX_ROWS:(k + 1) * ic.MAX_ROWS, :6].astype(object).sum(axis=0)]
        assert tot == sums[key][0] + sums[key][1], (key, tot)
    tl = ref.quotients(N, sums["left"][0][0], sums["left"][1][0]).astype(F32)
    tr = ref.quotients(N, sums["right"][0][0], sums["right"][1][0]).astype(F32)
    assert tr[0] == -1 and tr[255] == 1 and tl[254] < -4095
    want = np.full((3, Hc, Wc), tl[255], F32)
    want[:, 1234 - oy, 2345 - oxl] = tl[254]
    assert np.array_equal(ic.bits(host(lo)), ic.bits(want))
    assert np.array_equal(ic.bits(host(ro)), ic.bits(np.full((3, Hc, Wc), tr[0], F32)))
    want = np.full((3, Hc, Wc), tr[255], F32)
    want[:, :4] = tr[0]
    assert np.array_equal(ic.bits(host(ro2)), ic.bits(want))
    assert np.array_equal(ic.bits(host(lo2)), ic.bits(np.full((3, Hc, Wc), tl[255], F32)))


# ---- functions and modules ------------------------------------------------------------------------------------------------

def _u8(dev, img, misalign=0):
    """the image on the device, `misalign` bytes behind an allocation's boundary"""
    flat = dev.to(np.concatenate([np.zeros(misalign, np.uint8), img.ravel()]))
    return flat[misalign:].view(img.shape)


@pytest.mark.parametrize("case", [c for c in ic.IMAGE_CASES if c.out_misalign == 0 and "trip2" not in c.name], ids=repr)
def test_stereo_input_module(api, dev, case):
    import torch
    from ganet_amd.modules.fused import StereoInput, predict_offsets
    m = StereoInput(case.Hc, case.Wc)
    left, right = _u8(dev, case.left, case.misalign[0]), _u8(dev, case.right, case.misalign[1])
    batch_l, batch_r = (torch.full((3, 3, case.Hc, case.Wc), float("nan"), device=dev.device) for _ in range(2))
    a, b = m.window(left, right, case.oy, case.ox_left, case.ox_right, out_left=batch_l[1], out_right=batch_r[2])
    assert a.data_ptr() == batch_l[1].data_ptr() and b.data_ptr() == batch_r[2].data_ptr()
    for got, want in zip((a, b), case.ref):
        assert np.array_equal(ic.bits(host(got)), ic.bits(want)), case.name
    assert bool(torch.isnan(batch_l[0]).all()) and bool(torch.isnan(batch_l[2]).all()) and bool(torch.isnan(batch_r[:2]).all())
    try:
        rule = predict_offsets(case.H, case.W, case.Hc, case.Wc)
    except ValueError:
        return
    if (case.oy, case.ox_left, case.ox_right) == rule + rule[1:]:
        l4, r4, hw = m(left, right)
        assert hw == (case.H, case.W) and l4.shape == (1, 3, case.Hc, case.Wc)
        assert np.array_equal(ic.bits(host(l4[0])), ic.bits(case.ref[0])) and np.array_equal(ic.bits(host(r4[0])), ic.bits(case.ref[1]))


@pytest.mark.parametrize("case", ic.WINDOW_CASES[:6], ids=repr)
def test_target_window_module(api, dev, case):
    from ganet_amd.modules.fused import StereoInput
    got = StereoInput(case.Hc, case.Wc).target_window(dev.to(case.src), case.oy, case.ox, case.sub, case.fill)
    ic.check_window(case, host(got))


@pytest.mark.parametrize("case", ic.DISP_CASES[:6], ids=repr)
def test_disparity_output(api, dev, case):
    import torch
    from ganet_amd.functions.fused import disparity_to_u16
    from ganet_amd.modules.fused import DisparityOutput
    d = dev.to(case.disp)
    got = disparity_to_u16(d, (case.h, case.w), case.oy, case.ox, case.scale)
    assert got.dtype == torch.uint16 and np.array_equal(host(got), case.ref)
    Hd, Wd = case.disp.shape
    if (case.oy, case.ox) == (Hd - case.h, Wd - case.w):           # the un-padding rule of predict.py:134-137
        assert np.array_equal(host(DisparityOutput(case.scale)(d[None], (case.h, case.w))), case.ref)
    whole = DisparityOutput(case.scale)(d, (Hd + 1, Wd + 1))         # a cropped image keeps the whole map
    assert np.array_equal(host(whole), ref.disparity_u16(case.disp, Hd, Wd, 0, 0, case.scale))


def test_tensors_that_are_not_uint8_on_the_device_raise(api, dev):
    import torch
    from ganet_amd.modules.fused import DisparityOutput, StereoInput
    c = ic.IMAGES["pad-5x7-cp3"]
    m = StereoInput(c.Hc, c.Wc)
    left, right = dev.to(c.left), dev.to(c.right)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(left.cpu(), right.cpu())
    with pytest.raises(TypeError):
        m(left.float(), right.float())
    with pytest.raises(ValueError):
        m(left, right[:, :5])
    with pytest.raises(ValueError):
        m(left[:, :5], right[:, :5])                                 # not contiguous
    with pytest.raises(ValueError):
        m.window(left, right, 0, 0, 0, out_left=torch.empty(3, c.Hc, c.Wc + 1, device=dev.device))
    with pytest.raises(RuntimeError, match="no CPU path"):
        DisparityOutput()(torch.zeros(4, 4), (4, 4))
    with pytest.raises(TypeError):
        DisparityOutput()(torch.zeros(4, 4, device=dev.device).double(), (4, 4))


def _front_and_back(m, o, left, right):
    l4, r4, hw = m(left, right)
    return l4, r4, o((l4[0, 0] * 40 + r4[0, 1] * 30 + 90), hw)


def test_no_host_synchronisation(api, dev):
    import torch
    from ganet_amd.modules.fused import DisparityOutput, StereoInput
    c = ic.IMAGES["pad-33x65-cp3"]
    m, o = StereoInput(c.Hc, c.Wc), DisparityOutput()
    left, right = dev.to(c.left), dev.to(c.right)
    _front_and_back(m, o, left, right)                              # first use: library load, allocator warm-up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        l4, r4, u16 = _front_and_back(m, o, left, right)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert np.array_equal(ic.bits(host(l4[0])), ic.bits(c.ref[0])) and np.array_equal(ic.bits(host(r4[0])), ic.bits(c.ref[1]))
    want = ref.disparity_u16((c.ref[0][0] * F32(40) + c.ref[1][1] * F32(30)) + F32(90), c.H, c.W, c.Hc - c.H, c.Wc - c.W, 256.0)
    assert u16.shape == (c.H, c.W) and np.array_equal(host(u16), want)


def test_graph_capture_replayed_on_new_data_and_a_side_stream(api, dev):
    """front end, a pointwise stand-in and the back end captured once on a side stream and replayed on other images: equal to
    the statement of each"""
    import torch
    from ganet_amd.modules.fused import DisparityOutput, StereoInput
    cases = [ic.IMAGES[n] for n in ("pad-33x65-cp3", "two-level-33x65", "low-contrast-33x65")]
    c0 = cases[0]
    m, o = StereoInput(c0.Hc, c0.Wc), DisparityOutput()
    left, right = dev.to(c0.left), dev.to(c0.right)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            l4, r4, u16 = _front_and_back(m, o, left, right)
    side.synchronize()
    assert np.array_equal(ic.bits(host(l4[0])), ic.bits(c0.ref[0]))          # the side stream's eager result
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        l4, r4, u16 = _front_and_back(m, o, left, right)
    for c in cases[1:] + cases[:1]:
        left.copy_(dev.to(c.left)), right.copy_(dev.to(c.right))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(ic.bits(host(l4[0])), ic.bits(c.ref[0])) and np.array_equal(ic.bits(host(r4[0])), ic.bits(c.ref[1])), c.name
        want = ref.disparity_u16((c.ref[0][0] * F32(40) + c.ref[1][1] * F32(30)) + F32(90), c.H, c.W, c.Hc - c.H, c.Wc - c.W, 256.0)
        assert np.array_equal(host(u16), want), c.name


@pytest.mark.parametrize("name", ["pad-33x65-cp3", "centre-crop-odd-33x65", "pad-33x65-cp4"])
def test_predict_images_equals_the_host_pipeline(api, dev, name):
    """harness.steps.predict_images on a stand-in model of pointwise ops against predict.py's own order of work: numpy
    standardisation and padding on the host, upload, the same model, download, (temp * 256).astype('uint16') -- bit for bit,
    the un-padded uint16 map included"""
    import torch
    from harness import steps

    class StandIn(torch.nn.Module):
        def forward(self, left, right):
            return (left[:, 0] * 25 - right[:, 1] * 17 + left[:, 2] * right[:, 0] * 3).abs() + 0.25

    c = ic.IMAGES[name]
    model = StandIn().to(dev.device)
    got = steps.predict_images(model, dev.to(c.left), dev.to(c.right), (c.Hc, c.Wc))
    hl, hr, h, w = ref.host_test_transform(ref.host_load(c.left, c.right), c.Hc, c.Wc)
    with torch.no_grad():
        pred = model(torch.from_numpy(hl).to(dev.device), torch.from_numpy(hr).to(dev.device))
    want = ref.host_output(host(pred), h, w)
    assert got.dtype == torch.uint16 and got.shape == want.shape and np.array_equal(host(got), want)
    assert want.max() > 256 and len(np.unique(want)) > 100
