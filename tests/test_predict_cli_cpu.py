"""harness.predict and the host side of StereoInput / DisparityOutput without a GPU: argument parsing, the reader and the
writer (a 16-bit PNG and a .npy written and read back equal), the host restatement behind --host_io against tests/io_ref64.py,
the ValueError on an image larger than the crop one way only, and the refusal of anything but device tensors."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import io_ref64 as ref  # noqa: E402
from harness import predict as cli  # noqa: E402


def test_argument_parsing():
    a = cli.parse_args(["--left", "l.png", "--right", "r.png", "--out", "o.png"])
    assert (a.crop_height, a.crop_width, a.max_disp, a.model, a.resume) == (384, 1248, 192, "GANet_deep", "")
    assert not (a.fused or a.fused_bn or a.host_io)
    a = cli.parse_args("--left l --right r --out o.npy --crop_height 240 --crop_width 624 --max_disp 96 --resume ck.pth --fused "
                       "--fused_bn --host_io --model GANet11".split())
    assert (a.crop_height, a.crop_width, a.max_disp, a.model, a.resume) == (240, 624, 96, "GANet11", "ck.pth")
    assert a.fused and a.fused_bn and a.host_io
    for bad in (["--left", "l", "--right", "r"], ["--left", "l", "--right", "r", "--out", "o", "--crop_height", "0"],
                ["--left", "l", "--right", "r", "--out", "o", "--no_such_flag"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)


@pytest.mark.parametrize("ext", [".png", ".npy"])
def test_disparity_image_round_trip(tmp_path, ext):
    rng = np.random.default_rng(1)
    u16 = rng.integers(0, 65536, (37, 53)).astype(np.uint16)
    u16[0, :4] = (0, 1, 255, 65535)
    path = str(tmp_path / ("disp" + ext))
    cli.write_disparity(path, u16)
    back = cli.read_disparity(path)
    assert back.dtype == np.uint16 and np.array_equal(back, u16)
    if ext == ".png":
        from PIL import Image
        with Image.open(path) as im:
            assert im.mode.startswith("I;16") and im.size == (53, 37)
    with pytest.raises(ValueError):
        cli.write_disparity(path, u16.astype(np.float32))


def test_image_reader(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(2)
    rgb = rng.integers(0, 256, (9, 14, 3)).astype(np.uint8)
    rgba = rng.integers(0, 256, (9, 14, 4)).astype(np.uint8)
    Image.fromarray(rgb).save(tmp_path / "rgb.png")
    Image.fromarray(rgba).save(tmp_path / "rgba.png")
    Image.fromarray(rgb[..., 0]).save(tmp_path / "grey.png")
    np.save(tmp_path / "rgb.npy", rgb)
    np.save(tmp_path / "bad.npy", rgb.astype(np.float32))
    assert np.array_equal(cli.read_image(str(tmp_path / "rgb.png")), rgb)
    assert np.array_equal(cli.read_image(str(tmp_path / "rgba.png")), rgba)
    assert np.array_equal(cli.read_image(str(tmp_path / "rgb.npy")), rgb)
    grey = cli.read_image(str(tmp_path / "grey.png"))
    assert grey.shape == (9, 14, 3) and all(np.array_equal(grey[..., c], rgb[..., 0]) for c in range(3))
    with pytest.raises(ValueError):
        cli.read_image(str(tmp_path / "bad.npy"))


@pytest.mark.parametrize("hw,crop", [((9, 14), (12, 16)), ((9, 14), (9, 14)), ((9, 14), (4, 7)), ((9, 14), (8, 13))])
def test_host_io_is_the_reference_chain(hw, crop):
    """--host_io's restatement against the one the kernels' tests use (tests/io_ref64.py (b))"""
    rng = np.random.default_rng(3)
    left, right = (rng.integers(0, 256, hw + (3,)).astype(np.uint8) for _ in range(2))
    l, r, got_hw = cli.host_front(left, right, crop)
    hl, hr, h, w = ref.host_test_transform(ref.host_load(left, right), *crop)
    assert got_hw == (h, w) and np.array_equal(l.view(np.uint32), hl.view(np.uint32)) and np.array_equal(r.view(np.uint32), hr.view(np.uint32))
    pred = rng.uniform(0, 192, (1,) + crop).astype(np.float32)
    assert np.array_equal(cli.host_back(pred, got_hw), ref.host_output(pred, h, w))


def test_mixed_sizes_raise():
    import torch
    from ganet_amd.modules.fused import DisparityOutput, StereoInput, predict_offsets
    assert predict_offsets(375, 1242, 384, 1248) == (-9, -6) and predict_offsets(400, 1300, 384, 1248) == (8, 26)
    assert predict_offsets(384, 1248, 384, 1248) == (0, 0) and predict_offsets(33, 65, 16, 32) == ref.predict_offsets(33, 65, 16, 32)
    m = StereoInput(384, 1248)
    for hw in ((400, 1242), (375, 1300), (385, 1248)):
        with pytest.raises(ValueError, match="one way"):
            predict_offsets(*hw, 384, 1248)
        img = torch.zeros(hw + (3,), dtype=torch.uint8)
        with pytest.raises(ValueError, match="one way"):
            m(img, img)
        with pytest.raises(ValueError):
            cli.host_front(img.numpy(), img.numpy(), (384, 1248))
    img = torch.zeros((5, 7, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):                 # no CPU path, as everywhere in the package
        m(img, img)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.target_window(torch.zeros(5, 7), 0, 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        DisparityOutput()(torch.zeros(1, 8, 8), (5, 7))


def test_abi_14_names_the_new_entries():
    from ganet_amd import _native
    assert _native.ABI_VERSION == 14
    for name in ("ganet_stereo_input_workspace", "ganet_stereo_input_stats", "ganet_stereo_input_apply", "ganet_window_f32",
                 "ganet_disparity_to_u16"):
        assert name in _native.EXPORTS
    from harness import steps
    assert callable(steps.predict_images)
