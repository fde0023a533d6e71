"""GPU parity tests (pytest -m gpu, run on a real MI355X through gpurun): the gfx950 build of
libganet_hip.so driven through its C ABI, against the committed golden fixtures (generated from
the reference's own kernel bodies) and the CPU oracle on the same seeded inputs.
Bar: direction mask / forward volumes bit-exact, fp32 gradients within 1e-4 max-abs."""
import os

import numpy as np
import pytest

import parity_cases as pc
from golden_util import lga_case_names, load, sga_case_names

pytestmark = pytest.mark.gpu


class TorchDev:
    def __init__(self):
        import torch
        self.torch = torch
        assert torch.cuda.is_available()
        self.device = torch.device("cuda:0")
        self.stream = torch.cuda.current_stream().cuda_stream

    def to(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def _dt(self, dtype):
        return {np.float32: self.torch.float32, np.uint8: self.torch.uint8, np.int32: self.torch.int32,
                np.uint16: self.torch.int16}[dtype]

    def empty(self, shape, dtype=np.float32):
        # poison so that an element the kernel fails to write is noticed
        t = self.torch.empty(tuple(shape), dtype=self._dt(dtype), device=self.device)
        return t.fill_(float("nan")) if dtype == np.float32 else t.fill_(113)

    def zeros(self, shape, dtype=np.float32):
        return self.torch.zeros(tuple(shape), dtype=self._dt(dtype), device=self.device)

    def ptr(self, t):
        return t.data_ptr()

    def host(self, t):
        a = t.cpu().numpy()
        return a.view(np.uint16) if a.dtype == np.int16 else a

    def sync(self):
        self.torch.cuda.synchronize()

    def release(self):
        """buffers are torch tensors: freed by reference count (the raw-hipMalloc device of test_gpu_bounds.py frees here)"""
        self.sync()


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


def test_dpp_lane_patterns(api, dev):
    scratch = dev.zeros((8 * 64,), np.int32)
    host = np.zeros(8 * 64, np.int32)
    api.call("ganet_selftest_dpp", scratch.data_ptr(), host.ctypes.data, dev.stream)
    api.call("ganet_selftest_dpp_wave", scratch.data_ptr(), host.ctypes.data, dev.stream)     # wave_shl / wave_shr / readlane


@pytest.mark.parametrize("name", sga_case_names())
def test_sga_golden(api, dev, name):
    z = load("sga_golden.npz")
    x, go = z[f"{name}.x"], z[f"{name}.go"]
    gs = [z[f"{name}.g{d}"] for d in range(4)]
    want = {"out": z[f"{name}.out"], "mask": z[f"{name}.mask"], "tmp": z[f"{name}.tmp"], "gx": z[f"{name}.gx"]}
    for d in range(4):
        want[f"A{d}"] = z[f"{name}.A{d}"]
        want[f"gw{d}"] = z[f"{name}.gw{d}"]
    pc.check_sga_forward_backward(api, dev, x, gs, go, want)
    pc.check_sga_compat(api, dev, x, gs, go, want)


def test_sga_cfg1_golden_forward(api, dev):
    """BASELINE.json configs[0]: 1x48x48x48 (C=1) forward."""
    z = load("sga_cfg1_golden.npz")
    _, _, _, out, mask, _ = pc.run_sga_forward(api, dev, z["x"], [z[f"g{d}"] for d in range(4)])
    assert np.array_equal(dev.host(out), z["out"])
    assert np.array_equal(dev.host(mask), z["mask"])


def _oracle_want(oracle, x, gs, go):
    out, tmp, mask = oracle.sga_forward(x, *gs)
    grads = oracle.sga_backward(x, *gs, tmp, mask, go)
    want = {"out": out, "mask": mask.astype(np.uint8), "tmp": tmp, "gx": grads[0]}
    for d in range(4):
        want[f"gw{d}"] = grads[1 + d]
    return want


@pytest.mark.parametrize("shape", [(1, 3, 65, 20, 52), (2, 2, 33, 40, 104), (1, 2, 48, 17, 30), (1, 1, 193, 6, 12),
                                   (1, 5, 9, 64, 8), (3, 1, 2, 7, 260)])
def test_sga_random_vs_oracle(api, dev, port_oracle, shape):
    x, gs, go = pc.sga_inputs(shape, seed=sum(shape))
    pc.check_sga_forward_backward(api, dev, x, gs, go, _oracle_want(port_oracle, x, gs, go))


def test_sga_horizontal_depth_over_wavefront_boundaries(api, dev, port_oracle):
    """Every boundary of the row kernels' dispatch between the wavefront-wide depth axis (D <= 40, 48, 64, 72) and the
    mirrored 16-lane DPP row (sga_row_tu.hip), rows of several batches with partial ones, forward bit-exact / gradients at 1e-4."""
    for D in (1, 2, 39, 40, 41, 47, 49, 57, 64, 66, 71, 72, 73):
        shape = (1, 2, D, 3, 104)
        x, gs, go = pc.sga_inputs(shape, seed=100 + D)
        pc.check_sga_forward_backward(api, dev, x, gs, go, _oracle_want(port_oracle, x, gs, go))
    # the last depth of a range of disparities per lane whose kernel another family's makes unreachable (tests/test_sim_sga.py,
    # _LAUNCHER_ARMS): rows at 48, 80, 81; columns at 144, 208 with the wide families off; W % 16 and W % 4 only, H % 4
    no_wide = {"GANET_SGA_WIDE_SCAN": 0, "GANET_SGA_WIDE_COL": 0}
    for D in (48, 80, 81, 144, 208):
        for name, value in (no_wide if D >= 96 else {}).items():
            api.set_option(name, value)
        try:
            for W in (16, 20):
                x, gs, go = pc.sga_inputs((1, 1, D, 4, W), seed=100 + D + W)
                pc.check_sga_forward_backward(api, dev, x, gs, go, _oracle_want(port_oracle, x, gs, go))
        finally:
            for name in no_wide:
                api.set_option(name, 1)


@pytest.mark.parametrize("rowwave", [0, 1])
def test_sga_horizontal_kernel_families(api, dev, port_oracle, rowwave):
    """float4-per-lane segments vs one-wavefront-per-row LDS-staged kernels (right / left)."""
    api.set_option("GANET_SGA_ROWWAVE", rowwave)
    try:
        for shape in [(1, 2, 65, 9, 48), (2, 1, 33, 5, 104), (1, 1, 130, 3, 24), (1, 3, 7, 4, 20)]:
            x, gs, go = pc.sga_inputs(shape, seed=17 + rowwave)
            pc.check_sga_forward_backward(api, dev, x, gs, go, _oracle_want(port_oracle, x, gs, go))
    finally:
        api.set_option("GANET_SGA_ROWWAVE", 1)


@pytest.mark.parametrize("name", lga_case_names())
def test_lga_golden(api, dev, name):
    z = load("lga_golden.npz")
    r, passes = (int(v) for v in z[f"{name}.meta"])
    want = {"y": z[f"{name}.y"], "gx": z[f"{name}.gx"], "gf": z[f"{name}.gf"]}
    pc.check_lga_chain(api, dev, z[f"{name}.x"], z[f"{name}.f"], z[f"{name}.gy"], r, passes, want)


@pytest.mark.parametrize("shape,r,passes", [((1, 193, 24, 72), 2, 2), ((2, 33, 41, 67), 2, 1), ((1, 7, 64, 128), 1, 3),
                                            ((1, 12, 19, 33), 3, 1), ((2, 3, 17, 9, 40), 2, 2),
                                            # W % 4 == 0, radius 2: the API-layout operands are staged planar by 16-byte copies and read
                                            # with ds_read2_b32 (a path the CPU emulator does not execute) -- images narrower than a tile
                                            # and than its staged row, odd and even depth, one to three passes
                                            ((1, 9, 5, 8), 2, 2), ((2, 7, 9, 12), 2, 2), ((1, 1, 1, 4), 2, 1), ((1, 4, 3, 36), 2, 3),
                                            ((1, 2, 67, 100), 2, 1)])
def test_lga_random_vs_oracle(api, dev, port_oracle, shape, r, passes):
    rng = np.random.default_rng(sum(shape) + r)
    fs = list(shape)
    fs[-3] = 3 * (2 * r + 1) ** 2
    x = rng.standard_normal(shape).astype(np.float32)
    f = pc.l1norm(rng.standard_normal(fs), -3)
    gy = rng.standard_normal(shape).astype(np.float32)
    y, ins = port_oracle.lga_chain_forward(x, f, r, passes)
    gx, gf = port_oracle.lga_chain_backward(ins, f, gy, r)
    pc.check_lga_chain(api, dev, x, f, gy, r, passes, {"y": y, "gx": gx, "gf": gf})


def test_full_size_cfg2_against_oracle(api, dev, port_oracle):
    """BASELINE.json configs[1] at full size: SGA [1,32,65,80,208] and LGA2 [1,193,240,624]."""
    x, gs, go = pc.sga_inputs((1, 32, 65, 80, 208), seed=123)
    err = pc.check_sga_forward_backward(api, dev, x, gs, go, _oracle_want(port_oracle, x, gs, go))
    print("cfg2 SGA max-abs errors:", err)
    rng = np.random.default_rng(123)
    shape = (1, 193, 240, 624)
    xl = rng.standard_normal(shape).astype(np.float32)
    f = pc.l1norm(rng.standard_normal((1, 75, 240, 624)), 1)
    gy = rng.standard_normal(shape).astype(np.float32)
    y, ins = port_oracle.lga_chain_forward(xl, f, 2, 2)
    gx, gf = port_oracle.lga_chain_backward(ins, f, gy, 2)
    err = pc.check_lga_chain(api, dev, xl, f, gy, 2, 2, {"y": y, "gx": gx, "gf": gf})
    print("cfg2 LGA2 max-abs errors:", err)


@pytest.mark.parametrize("name", ["sga_cfg2", "sga_b", "sga_cfg3"])
def test_sga_full_size_forward_matches_reference_digests(api, dev, name):
    """The bit-exact outputs of SGA's forward at the full model shapes -- out, the direction mask, the four directional volumes,
    A_left under the reference's name temp_out -- hashed on the host and compared with the sha256 the REFERENCE's own kernel bodies
    produced on the same seeded inputs (tests/golden/digests.json, made here from oracle/_ref by make_golden.py --digests).  The
    GPU box has no /root/reference: this is its direct link to the reference at BASELINE configs[1]'s size, past the restatement."""
    import golden_util as gu
    want = gu.load_digests()[name]
    shape, seed = tuple(want["shape"]), want["seed"]
    x, gs, _ = gu.sga_digest_inputs(shape, seed)
    assert gu.sha(x) == want["sha256"]["in.x"] and all(gu.sha(gs[k]) == want["sha256"][f"in.g{k}"] for k in range(4))
    _, _, A, out, mask, _ = pc.run_sga_forward(api, dev, x, gs)
    hA = dev.host(A)
    got = {"out": gu.sha(dev.host(out)), "mask_u8": gu.sha(dev.host(mask)), "temp_out": gu.sha(hA[3]),
           **{f"A{k}": gu.sha(hA[k]) for k in range(4)}}
    assert got == {k: want["sha256"][k] for k in got}, [k for k in got if got[k] != want["sha256"][k]]


@pytest.mark.parametrize("tiled", [0, 1])
@pytest.mark.parametrize("shape", [(1, 32, 65, 80, 208), (1, 4, 33, 8, 48), (2, 3, 48, 12, 80), (1, 2, 9, 4, 16)])
def test_sga_tiled_private_workspace(api, dev, port_oracle, shape, tiled):
    """GANET_SGA_TILED (sga_col_kernels.h): the vertical directions' ADJOINT volumes of ganet_sga_backward's private workspace
    tiled [slice][W/16][H/4][D][4][16] -- written by the column adjoint scans as contiguous bursts, read by
    sga_bwd_point<.., TG>.  Both settings: same gradients (within 1e-4 of the oracle), and the tiled volume itself, un-tiled by
    the checker, equals what ganet_sga_backward_scan writes in the API layout.  Shapes: several row batches, one to five column
    blocks, depths that do and do not fill their lanes (GPU: the full cfg2 size as well)."""
    was = api.get_option("GANET_SGA_TILED")
    api.set_option("GANET_SGA_TILED", tiled)
    try:
        N, C, D, H, W = shape
        assert api.query("ganet_sga_workspace_layout", N, C, D, H, W) == tiled
        x, gs, go = pc.sga_inputs(shape, seed=7 + tiled)
        err = pc.check_sga_forward_backward(api, dev, x, gs, go, _oracle_want(port_oracle, x, gs, go))
        assert max(err.values()) <= pc.TOL, err
    finally:
        api.set_option("GANET_SGA_TILED", was)


@pytest.mark.parametrize("shape", [(1, 4, 33, 8, 48), (1, 2, 9, 4, 16)])
def test_sga_backward_with_a_4_byte_aligned_gradient_on_a_tiled_shape(api, dev, port_oracle, shape):
    """where the private adjoint workspace is tiled, a contiguous gradient at a 4-byte aligned address takes the API
    layout and the generic scans (ganet_sga_backward decides the layout once, alignment included) instead of failing."""
    N, C, D, H, W = shape
    assert api.query("ganet_sga_workspace_layout", N, C, D, H, W) == 1
    x, gs, go = pc.sga_inputs(shape, seed=11)
    got = pc.run_sga_backward_only(api, dev, x, gs, go, go_offset=1)
    out, tmp, mask = port_oracle.sga_forward(x, *gs)
    grads = port_oracle.sga_backward(x, *gs, tmp, mask, go)
    assert np.abs(got["gx"] - grads[0]).max() <= pc.TOL
    for d in range(4):
        assert np.abs(got[f"gw{d}"] - grads[1 + d]).max() <= pc.TOL


def test_full_size_properties(api, dev):
    """Size-independent properties at the full cfg2 shapes (no oracle involved):
    SGA is positively homogeneous -- scaling x by 2 scales every volume by exactly 2 and leaves
    the direction mask unchanged; LGA is bilinear, so <y, gy> == <x, gX> == <f, gF>."""
    torch = dev.torch
    x, gs, _ = pc.sga_inputs((1, 32, 65, 80, 208), seed=5)
    _, _, _, out1, mask1, _ = pc.run_sga_forward(api, dev, x, gs)
    _, _, _, out2, mask2, _ = pc.run_sga_forward(api, dev, 2.0 * x, gs)
    assert torch.equal(out2, 2.0 * out1) and torch.equal(mask1, mask2)
    g = torch.Generator(device="cuda").manual_seed(9)
    B, D, H, W = 1, 193, 240, 624
    xl = torch.randn((B, D, H, W), device="cuda", generator=g)
    f = torch.nn.functional.normalize(torch.randn((B, 75, H, W), device="cuda", generator=g), p=1, dim=1)
    gy = torch.randn((B, D, H, W), device="cuda", generator=g)
    y, gx, gf = torch.empty_like(xl), torch.empty_like(xl), torch.empty_like(f)
    api.call("ganet_lga_forward", xl.data_ptr(), f.data_ptr(), y.data_ptr(), B, D, H, W, 2, dev.stream)
    api.call("ganet_lga_backward", xl.data_ptr(), f.data_ptr(), gy.data_ptr(), gx.data_ptr(), gf.data_ptr(),
             B, D, H, W, 2, 0, dev.stream)
    torch.cuda.synchronize()
    a = (y.double() * gy.double()).sum().item()
    b = (xl.double() * gx.double()).sum().item()
    c = (f.double() * gf.double()).sum().item()
    scale = (y.double().abs() * gy.double().abs()).sum().item()
    assert abs(a - b) <= 1e-6 * scale and abs(a - c) <= 1e-6 * scale, (a, b, c, scale)


@pytest.mark.parametrize("shape", [(1, 48, 33, 40, 104), (2, 32, 65, 176, 320), (1, 32, 65, 128, 416)])
def test_sga_model_shapes_fast_path_vs_compat_path(api, dev, shape):
    """The other SGA shapes of BASELINE configs 2-5 (1/6-resolution volumes, SceneFlow 960x528 at
    2 samples per GPU, KITTI 1248x384): the fast path (column-block / row-per-wave kernels, uint8
    mask, saved volumes) and the reference-buffer-contract path (segment scans, float mask,
    recomputed volumes) are different kernel families and must agree -- forward bit-exact,
    gradients to fp32 rounding -- with no oracle in the loop."""
    torch = dev.torch
    N, C, D, H, W = shape
    g = torch.Generator(device="cuda").manual_seed(sum(shape))
    x = torch.randn(shape, device="cuda", generator=g)
    gs = [torch.nn.functional.normalize(torch.randn((N, C, 5, H, W), device="cuda", generator=g), p=1, dim=2)
          for _ in range(4)]
    go = torch.randn(shape, device="cuda", generator=g)
    st = dev.stream
    A = torch.empty((4,) + shape, device="cuda")
    out, gx = torch.empty_like(x), torch.empty_like(x)
    mask = torch.empty(shape, dtype=torch.uint8, device="cuda")
    kp = torch.empty((4, N, C, H, W), dtype=torch.int16, device="cuda")
    gw = [torch.empty_like(t) for t in gs]
    api.call("ganet_sga_forward", x.data_ptr(), *[t.data_ptr() for t in gs], A.data_ptr(), out.data_ptr(),
             mask.data_ptr(), kp.data_ptr(), N, C, D, H, W, st)
    G = torch.empty_like(A)
    api.call("ganet_sga_backward", x.data_ptr(), *[t.data_ptr() for t in gs], A.data_ptr(), mask.data_ptr(),
             kp.data_ptr(), go.data_ptr(), G.data_ptr(), gx.data_ptr(), *[t.data_ptr() for t in gw], N, C, D, H, W, st)
    del G
    tmp, out2, maskf = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
    api.call("ganet_sga_forward_compat", x.data_ptr(), *[t.data_ptr() for t in gs], tmp.data_ptr(), out2.data_ptr(),
             maskf.data_ptr(), N, C, D, H, W, st)
    assert torch.equal(out, out2) and torch.equal(mask.float(), maskf) and torch.equal(tmp, A[3])
    gx2 = torch.zeros_like(x)
    gw2 = [torch.zeros_like(t) for t in gs]
    tgrad = torch.empty_like(x)
    idx = torch.empty((N, C, H, W), device="cuda")
    api.call("ganet_sga_backward_compat", x.data_ptr(), *[t.data_ptr() for t in gs], tmp.data_ptr(), maskf.data_ptr(),
             idx.data_ptr(), go.data_ptr(), tgrad.data_ptr(), gx2.data_ptr(), *[t.data_ptr() for t in gw2],
             N, C, D, H, W, st)
    torch.cuda.synchronize()
    assert (gx - gx2).abs().max().item() <= pc.TOL
    for a, b in zip(gw, gw2):
        assert (a - b).abs().max().item() <= pc.TOL


def test_cost_volume_and_regression(api, dev, port_oracle):
    torch = dev.torch
    rng = np.random.default_rng(11)
    N, C, H, W, maxdisp = 2, 32, 20, 52, 64
    Dn = maxdisp + 1
    x = rng.standard_normal((N, C, H, W)).astype(np.float32)
    y = rng.standard_normal((N, C, H, W)).astype(np.float32)
    dx, dy = dev.to(x), dev.to(y)
    cost = dev.empty((N, 2 * C, Dn, H, W))
    api.call("ganet_cost_volume_forward", dx.data_ptr(), dy.data_ptr(), cost.data_ptr(), N, C, Dn, H, W, dev.stream)
    assert np.array_equal(dev.host(cost), port_oracle.cost_volume(x, y, maxdisp))
    p = rng.random((N, 193, H, W)).astype(np.float32)
    out = dev.empty((N, H, W))
    api.call("ganet_disparity_regression_forward", dev.to(p).data_ptr(), out.data_ptr(), N, 193, H, W, dev.stream)
    np.testing.assert_allclose(dev.host(out), port_oracle.disparity_regression(p, 192), rtol=1e-5, atol=1e-4)
    assert torch.cuda.is_available()


@pytest.mark.parametrize("shape", [(1, 193, 384, 1248), (2, 193, 528, 960), (1, 193, 241, 624)])
def test_lga_model_shapes_wave_kernels_vs_block_kernels(api, dev, shape):
    """The LGA shapes of BASELINE configs 3 and 5 (KITTI 1248x384; SceneFlow 960x528, 2 samples per GPU) and an odd
    height: the plane-pair kernels (default, GANET_LGA_WAVE=2; 1 = all of them on one-wave rings) and the 256-thread tile kernels (0, the general fallback) are different
    kernel families and must agree to fp32 rounding, forward, data gradient and filter gradient; the bilinear identity
    <y, gy> == <x, gX> == <f, gF> holds for both -- no oracle in the loop."""
    torch = dev.torch
    B, D, H, W = shape
    g = torch.Generator(device="cuda").manual_seed(sum(shape))
    xl = torch.randn(shape, device="cuda", generator=g)
    f = torch.nn.functional.normalize(torch.randn((B, 75, H, W), device="cuda", generator=g), p=1, dim=1)
    gy = torch.randn(shape, device="cuda", generator=g)
    res = {}
    try:
        for mode in (2, 0):
            api.set_option("GANET_LGA_WAVE", mode)
            y, gx, gf = torch.empty_like(xl), torch.empty_like(xl), torch.empty_like(f)
            api.call("ganet_lga_forward", xl.data_ptr(), f.data_ptr(), y.data_ptr(), B, D, H, W, 2, dev.stream)
            api.call("ganet_lga_backward", xl.data_ptr(), f.data_ptr(), gy.data_ptr(), gx.data_ptr(), gf.data_ptr(),
                     B, D, H, W, 2, 0, dev.stream)
            torch.cuda.synchronize()
            res[mode] = (y, gx, gf)
    finally:
        api.set_option("GANET_LGA_WAVE", 2)
    for a, b in zip(res[2], res[0]):
        assert (a - b).abs().max().item() <= pc.TOL, (a - b).abs().max().item()
    y, gx, gf = res[2]
    a = (y.double() * gy.double()).sum().item()
    b = (xl.double() * gx.double()).sum().item()
    c = (f.double() * gf.double()).sum().item()
    scale = (y.double().abs() * gy.double().abs()).sum().item()
    assert abs(a - b) <= 1e-6 * scale and abs(a - c) <= 1e-6 * scale, (a, b, c, scale)


def test_random_shape_fuzz_against_oracle(api, dev, port_oracle):
    """40 seeded random shapes (odd sizes, W % 4 != 0, W % 16 != 0, D = 1, H = 1, tiny and ragged tiles) through every
    dispatch branch (row-per-wave / column-block / segment scans, four-pixel / one-pixel merge, LDS-DMA / block LGA
    kernels): SGA forward bit-exact, all gradients and LGA within 1e-4 of the oracle."""
    rng = np.random.default_rng(2024)
    for case in range(24):
        N, C = int(rng.integers(1, 3)), int(rng.integers(1, 4))
        D = int(rng.choice([1, 2, 5, 16, 33, 48, 65, 70]))
        H = int(rng.integers(1, 14))
        W = int(rng.choice([1, 3, 4, 8, 12, 16, 20, 28, 32, 36, 48, 52, 64]))
        x, gs, go = pc.sga_inputs((N, C, D, H, W), seed=1000 + case)
        err = pc.check_sga_forward_backward(api, dev, x, gs, go, _oracle_want(port_oracle, x, gs, go))
        assert max(err.values()) <= pc.TOL, ((N, C, D, H, W), err)
    for case in range(16):
        B = int(rng.integers(1, 3))
        D = int(rng.choice([1, 2, 3, 9, 17, 40]))
        H = int(rng.integers(1, 12))
        W = int(rng.choice([1, 2, 5, 8, 16, 31, 32, 36, 40, 64, 68]))
        r = int(rng.choice([1, 2, 2, 3]))
        passes = int(rng.integers(1, 3))
        shape = (B, D, H, W)
        x = rng.standard_normal(shape).astype(np.float32)
        f = pc.l1norm(rng.standard_normal((B, 3 * (2 * r + 1) ** 2, H, W)), 1)
        gy = rng.standard_normal(shape).astype(np.float32)
        y, ins = port_oracle.lga_chain_forward(x, f, r, passes)
        gx, gf = port_oracle.lga_chain_backward(ins, f, gy, r)
        pc.check_lga_chain(api, dev, x, f, gy, r, passes, {"y": y, "gx": gx, "gf": gf})


# ---- every model shape of BASELINE configs 2-5 against the ORACLE (not only family vs family) -------------------------

@pytest.mark.parametrize("shape", [(1, 48, 33, 40, 104), (1, 32, 65, 128, 416), (1, 48, 33, 64, 208),
                                   (2, 32, 65, 176, 320), (2, 48, 33, 88, 160)])
def test_sga_model_shapes_vs_oracle(api, dev, port_oracle, shape):
    """The SGA volumes GANet-deep feeds the op at cfg2/4 (1/6-res), cfg3 (KITTI 1248x384: 1/3- and 1/6-res) and cfg5
    (SceneFlow 960x528, two samples per GPU): forward volumes / mask / arg-max bit-exact, gradients within 1e-4 of
    the CPU oracle on the same seeded inputs."""
    x, gs, go = pc.sga_inputs(shape, seed=sum(shape))
    err = pc.check_sga_forward_backward(api, dev, x, gs, go, _oracle_want(port_oracle, x, gs, go), per_dir=False)
    print("SGA", shape, "max-abs errors:", err)


@pytest.mark.parametrize("shape", [(1, 2, 240, 12, 24), (1, 1, 209, 6, 16), (1, 1, 272, 5, 20)])
def test_sga_deep_volumes_segment_fallback_vs_oracle(api, dev, port_oracle, shape):
    """D > 208 leaves the LDS-staged scans' range: the segment kernels take over for D in (208, 272] -- same bar
    against the oracle."""
    x, gs, go = pc.sga_inputs(shape, seed=sum(shape))
    pc.check_sga_forward_backward(api, dev, x, gs, go, _oracle_want(port_oracle, x, gs, go))


def _lga_vs_oracle(api, dev, oracle, x, f, gy, r, passes):
    y, ins = oracle.lga_chain_forward(x, f, r, passes)
    gx, gf = oracle.lga_chain_backward(ins, f, gy, r)
    return pc.check_lga_chain(api, dev, x, f, gy, r, passes, {"y": y, "gx": gx, "gf": gf})


@pytest.mark.parametrize("shape", [(1, 193, 240, 624), (1, 193, 384, 1248), (2, 193, 528, 960), (3, 12, 240, 624), (2, 21, 57, 130)])
def test_lga_model_shapes_vs_oracle(api, dev, port_oracle, shape):
    """LGA2 (radius 2, two chained passes) at the cfg2, cfg3 and cfg5 shapes (and a batch of three with an even D, an odd D on
    a ragged plane) against the oracle, y, gX, gF within 1e-4, both ways Lga2Function can run it: one-pass entries on the API
    layout (mixed item list: the default), and the pair-interleaved private intermediate (the default of the Function)."""
    rng = np.random.default_rng(sum(shape))
    x = rng.standard_normal(shape).astype(np.float32)
    f = pc.l1norm(rng.standard_normal((shape[0], 75) + shape[2:]), 1)
    gy = rng.standard_normal(shape).astype(np.float32)
    y, ins = port_oracle.lga_chain_forward(x, f, 2, 2)
    gx, gf = port_oracle.lga_chain_backward(ins, f, gy, 2)
    want = {"y": y, "gx": gx, "gf": gf}
    print("LGA2", shape, "max-abs errors:", pc.check_lga_chain(api, dev, x, f, gy, 2, 2, want),
          "paired:", pc.check_lga2_paired(api, dev, x, f, gy, 2, 2, want))


def test_lga_post_softmin_input_full_size_vs_oracle(api, dev, port_oracle):
    """SURVEY 8d's second LGA input: pass-2-like x = softmax(-randn) over the disparity axis (what DispAgg feeds the
    second LGA2 after nn.Softmin, models/GANet_deep.py:244-245), full cfg2 size."""
    rng = np.random.default_rng(77)
    shape = (1, 193, 240, 624)
    z = -rng.standard_normal(shape)
    z = np.exp(z - z.max(1, keepdims=True))
    x = (z / z.sum(1, keepdims=True)).astype(np.float32)
    f = pc.l1norm(rng.standard_normal((1, 75, 240, 624)), 1)
    gy = rng.standard_normal(shape).astype(np.float32)
    print("LGA2 post-softmin max-abs errors:", _lga_vs_oracle(api, dev, port_oracle, x, f, gy, 2, 2))


def test_cost_volume_and_regression_cfg2_size(api, dev, port_oracle):
    """GetCostVolume [1,32,80,208] x2 -> [1,64,65,80,208] forward (bit-exact: pure copies) and backward (sums of up to
    65 terms: 1e-4), DisparityRegression [1,193,240,624] forward and backward, against the oracle / its adjoint."""
    rng = np.random.default_rng(5)
    N, C, H, W, maxdisp = 1, 32, 80, 208, 64
    Dn = maxdisp + 1
    x = rng.standard_normal((N, C, H, W)).astype(np.float32)
    y = rng.standard_normal((N, C, H, W)).astype(np.float32)
    dx, dy = dev.to(x), dev.to(y)
    cost = dev.empty((N, 2 * C, Dn, H, W))
    api.call("ganet_cost_volume_forward", dx.data_ptr(), dy.data_ptr(), cost.data_ptr(), N, C, Dn, H, W, dev.stream)
    want = port_oracle.cost_volume(x, y, maxdisp)
    assert np.array_equal(dev.host(cost), want)
    gc = rng.standard_normal(want.shape).astype(np.float32)
    gx, gy = dev.empty((N, C, H, W)), dev.empty((N, C, H, W))
    api.call("ganet_cost_volume_backward", dev.to(gc).data_ptr(), gx.data_ptr(), gy.data_ptr(), N, C, Dn, H, W, dev.stream)
    # adjoint of the copies (modules/GANet.py:125-131): x feeds cost[:, :C, i, :, i:], y feeds cost[:, C:, i, :, i:] shifted by i
    wx = np.zeros((N, C, H, W), np.float64)
    wy = np.zeros((N, C, H, W), np.float64)
    for i in range(Dn):
        wx[..., i:] += gc[:, :C, i, :, i:]
        wy[..., :W - i] += gc[:, C:, i, :, i:]
    assert np.abs(dev.host(gx) - wx).max() <= pc.TOL and np.abs(dev.host(gy) - wy).max() <= pc.TOL
    p = rng.random((1, 193, 240, 624)).astype(np.float32)
    p /= p.sum(1, keepdims=True)
    out = dev.empty((1, 240, 624))
    api.call("ganet_disparity_regression_forward", dev.to(p).data_ptr(), out.data_ptr(), 1, 193, 240, 624, dev.stream)
    np.testing.assert_allclose(dev.host(out), port_oracle.disparity_regression(p, 192), rtol=1e-5, atol=1e-4)
    go = rng.standard_normal((1, 240, 624)).astype(np.float32)
    gp = dev.empty(p.shape)
    api.call("ganet_disparity_regression_backward", dev.to(go).data_ptr(), gp.data_ptr(), 1, 193, 240, 624, dev.stream)
    assert np.array_equal(dev.host(gp), go[:, None] * np.arange(193, dtype=np.float32)[None, :, None, None])


@pytest.mark.parametrize("shape,segs", [((1, 193, 240, 624), 0), ((1, 33, 7, 36), 2), ((2, 9, 3, 64), 3), ((1, 5, 66, 132), 0),
                                        ((1, 64, 13, 100), 2), ((1, 2, 2, 4), 0)])
def test_lga_plane_pair_item_lists_reproducible(api, dev, port_oracle, shape, segs):
    """The plane-pair kernels stage their planes with hand-counted waits (copies through immediate offsets on ONE M0 value):
    a miscounted wait or a misplaced copy reads a stale or foreign ring slot -- an O(1), run-to-run varying difference.  Whole
    tiles, the mixed item list (default) and forced depth segments (d_lo > 0) must each be bit-reproducible over repeated
    runs and agree with each other to fp32 rounding (and with the oracle where it is quick)."""
    torch = dev.torch
    B, D, H, W = shape
    g = torch.Generator(device="cuda").manual_seed(sum(shape) + segs)
    x = torch.randn(shape, device="cuda", generator=g)
    f = torch.nn.functional.normalize(torch.randn((B, 75, H, W), device="cuda", generator=g), p=1, dim=1)
    gy = torch.randn(shape, device="cuda", generator=g)
    res = {}
    try:
        for tag, mix, sg in (("whole", 0, 0), ("mix", 1, 0), ("segs", 0, segs if segs else 2)):
            api.set_option("GANET_LGA_MIX", mix)
            api.set_option("GANET_LGA_SEGS", sg)
            outs = []
            for rep in range(3):           # repeated: a race would not be deterministic
                y, gx, gf = torch.full_like(x, float("nan")), torch.full_like(x, float("nan")), torch.full_like(f, float("nan"))
                api.call("ganet_lga_forward", x.data_ptr(), f.data_ptr(), y.data_ptr(), B, D, H, W, 2, dev.stream)
                api.call("ganet_lga_backward", x.data_ptr(), f.data_ptr(), gy.data_ptr(), gx.data_ptr(), gf.data_ptr(),
                         B, D, H, W, 2, 0, dev.stream)
                torch.cuda.synchronize()
                outs.append((y, gx, gf))
            for o in outs[1:]:
                assert all(torch.equal(a, b) for a, b in zip(o, outs[0])), (tag, "not reproducible")
            res[tag] = outs[0]
    finally:
        api.set_option("GANET_LGA_MIX", 1)
        api.set_option("GANET_LGA_SEGS", 0)
    for tag in ("mix", "segs"):
        for a, b in zip(res["whole"], res[tag]):
            assert (a - b).abs().max().item() <= pc.TOL, tag
    if x.numel() <= 4_000_000:
        y, ins = port_oracle.lga_chain_forward(x.cpu().numpy(), f.cpu().numpy(), 2, 1)
        ogx, ogf = port_oracle.lga_chain_backward(ins, f.cpu().numpy(), gy.cpu().numpy(), 2)
        for got, want in zip(res["mix"], (y, ogx, ogf)):
            assert np.abs(got.cpu().numpy() - want).max() <= pc.TOL


@pytest.mark.parametrize("shape,wide", [((1, 1, 300, 5, 12), 1), ((1, 2, 577, 3, 8), 1), ((1, 2, 65, 9, 24), 2), ((1, 1, 193, 4, 20), 2),
                                        ((1, 1, 192, 240, 624), 1)])
def test_sga_wave_wide_scanlines_vs_oracle(api, dev, port_oracle, shape, wide):
    """Scans with the whole wavefront on one scanline (GANET_SGA_WIDE_SCAN): D beyond the 16-lane limit of 272, forced
    on ordinary volumes, and chosen automatically for SURVEY 8d's literal stress shape [1,1,192,240,624] (one slice: 624
    columns / 240 rows).  Same bar as everywhere: forward / mask / arg-max bit-exact, gradients within 1e-4."""
    x, gs, go = pc.sga_inputs(shape, seed=sum(shape))
    api.set_option("GANET_SGA_WIDE_SCAN", wide)
    try:
        err = pc.check_sga_forward_backward(api, dev, x, gs, go, _oracle_want(port_oracle, x, gs, go), per_dir=shape[3] < 100)
    finally:
        api.set_option("GANET_SGA_WIDE_SCAN", 1)
    print("wide scan", shape, err)


@pytest.mark.parametrize("shape,mode", [((1, 32, 65, 80, 208), 2), ((1, 2, 65, 7, 20), 2), ((2, 1, 7, 9, 8), 2), ((1, 1, 150, 3, 12), 2),
                                        ((1, 1, 191, 2, 40), 2), ((1, 1, 192, 240, 624), 1)])
def test_sga_wide_column_blocks_vs_oracle(api, dev, port_oracle, shape, mode):
    """Vertical scans with one wavefront per column (sga_col_fwd_wide / sga_col_bwdg_wide, 1,024-thread blocks): forced
    (GANET_SGA_WIDE_COL=2) on the full cfg2 volume and on small volumes with partial column blocks, H not a multiple of the
    4-row batch and D not a multiple of 3, and chosen automatically (1, the default) for SURVEY 8d's literal stress shape
    [1,1,192,240,624].  Same bar as everywhere: forward / mask / arg-max bit-exact, gradients within 1e-4 of the oracle."""
    x, gs, go = pc.sga_inputs(shape, seed=sum(shape))
    api.set_option("GANET_SGA_WIDE_COL", mode)
    try:
        err = pc.check_sga_forward_backward(api, dev, x, gs, go, _oracle_want(port_oracle, x, gs, go), per_dir=shape[3] < 100)
    finally:
        api.set_option("GANET_SGA_WIDE_COL", 1)
    print("wide column blocks", shape, err)


@pytest.mark.parametrize("N,C,H,W,maxdisp,Dr,Hr,Wr", [(1, 32, 128, 416, 64, 193, 384, 1248), (2, 32, 176, 320, 64, 193, 528, 960)])
def test_cost_volume_and_regression_cfg3_cfg5_sizes(api, dev, port_oracle, N, C, H, W, maxdisp, Dr, Hr, Wr):
    """GetCostVolume / DisparityRegression at the sizes of BASELINE configs 3 and 5: cost volumes [1,64,65,128,416] (886 MB)
    and [2,64,65,176,320] (1.87 GB: element offsets beyond 2^31 bytes inside one tensor), regression on [1,193,384,1248] and
    [2,193,528,960]; forward against the oracle (bit-exact copies / 1e-4), backward against the adjoint of the copies."""
    rng = np.random.default_rng(N + H)
    Dn = maxdisp + 1
    x = rng.standard_normal((N, C, H, W)).astype(np.float32)
    y = rng.standard_normal((N, C, H, W)).astype(np.float32)
    dx, dy = dev.to(x), dev.to(y)
    cost = dev.empty((N, 2 * C, Dn, H, W))
    api.call("ganet_cost_volume_forward", dx.data_ptr(), dy.data_ptr(), cost.data_ptr(), N, C, Dn, H, W, dev.stream)
    want = port_oracle.cost_volume(x, y, maxdisp)
    assert np.array_equal(dev.host(cost), want)
    del want
    # backward: a gradient volume of small integers makes every sum exact in fp32 (up to 65 terms) -- equality, not a tolerance
    gc = dev.torch.randint(-3, 4, (N, 2 * C, Dn, H, W), device="cuda", generator=dev.torch.Generator(device="cuda").manual_seed(5)).float()
    gx, gy = dev.empty((N, C, H, W)), dev.empty((N, C, H, W))
    api.call("ganet_cost_volume_backward", gc.data_ptr(), gx.data_ptr(), gy.data_ptr(), N, C, Dn, H, W, dev.stream)
    wx, wy = dev.torch.zeros_like(gx), dev.torch.zeros_like(gy)
    for i in range(Dn):                      # adjoint of the slice copies (modules/GANet.py:125-131), with torch on the device
        wx[..., i:] += gc[:, :C, i, :, i:]
        wy[..., :W - i] += gc[:, C:, i, :, i:]
    assert dev.torch.equal(gx, wx) and dev.torch.equal(gy, wy)
    del gc, cost, wx, wy
    p = rng.random((N, Dr, Hr, Wr)).astype(np.float32)
    p /= p.sum(1, keepdims=True)
    out = dev.empty((N, Hr, Wr))
    api.call("ganet_disparity_regression_forward", dev.to(p).data_ptr(), out.data_ptr(), N, Dr, Hr, Wr, dev.stream)
    np.testing.assert_allclose(dev.host(out), port_oracle.disparity_regression(p, Dr - 1), rtol=1e-5, atol=1e-4)
    go = rng.standard_normal((N, Hr, Wr)).astype(np.float32)
    gp = dev.empty(p.shape)
    api.call("ganet_disparity_regression_backward", dev.to(go).data_ptr(), gp.data_ptr(), N, Dr, Hr, Wr, dev.stream)
    assert np.array_equal(dev.host(gp), go[:, None] * np.arange(Dr, dtype=np.float32)[None, :, None, None])


@pytest.mark.parametrize("shape", [(1, 48, 240, 624), (1, 33, 7, 36), (2, 9, 3, 64), (1, 5, 66, 132), (1, 64, 13, 100), (1, 2, 2, 4),
                                   (1, 21, 61, 96)])
@pytest.mark.parametrize("paired", [0, 1])
def test_lga_workgroup_ring_matches_default_kernels(api, dev, port_oracle, shape, paired):
    """GANET_LGA_WAVE=2 (default) against 1 (the fallback): the four forward / data-backward launches of a two-pass chain with one
    LDS ring per 256-thread workgroup (32 x 8 tiles; lga_apply_pp_wx / _wxo / _wpi, a barrier per plane pair) and with one ring
    per wave (32 x 2 tiles).  Same arithmetic per pixel: results must agree to fp32 rounding on whole tiles, be bit-reproducible
    over repeated runs (the hand-off between the four waves is one counted wait + one barrier per plane pair: a race would not
    be deterministic), and agree with the oracle; then once more with the item lists each form chooses for itself."""
    torch = dev.torch
    B, D, H, W = shape
    g = torch.Generator(device="cuda").manual_seed(sum(shape))
    x = torch.randn(shape, device="cuda", generator=g)
    f = torch.nn.functional.normalize(torch.randn((B, 75, H, W), device="cuda", generator=g), p=1, dim=1)
    gy = torch.randn(shape, device="cuda", generator=g)
    xn, fn, gyn = x.cpu().numpy(), f.cpu().numpy(), gy.cpu().numpy()
    want = None
    if x.numel() <= 4_000_000:
        y, ins = port_oracle.lga_chain_forward(xn, fn, 2, 2)
        ogx, ogf = port_oracle.lga_chain_backward(ins, fn, gyn, 2)
        want = {"y": y, "gx": ogx, "gf": ogf}
    chain = pc.check_lga2_paired if paired else pc.check_lga_chain
    res = {}
    try:
        for mix, segs in ((0, 1), (1, 0)):
            api.set_option("GANET_LGA_MIX", mix)
            api.set_option("GANET_LGA_SEGS", segs)
            for wg in (0, 1, 1):
                api.set_option("GANET_LGA_WAVE", 1 + wg)
                got = {}
                chain(api, dev, xn, fn, gyn, 2, 2, want, out=got)
                if (mix, wg) in res:
                    assert all(np.array_equal(got[k], res[mix, wg][k]) for k in got), "workgroup ring: not reproducible"
                res[mix, wg] = got
                dev.release()
    finally:
        api.set_option("GANET_LGA_WAVE", 2)
        api.set_option("GANET_LGA_MIX", 1)
        api.set_option("GANET_LGA_SEGS", 0)
    # (bit for bit under the emulator, tests/test_sim_bounds.py; here the two forms are separate instantiations compiled for the
    # device, where the prologue's plain C++ sums may be contracted differently: fp32 rounding is the bar, a stale ring slot is O(1))
    for k in res[0, 0]:
        assert np.abs(res[0, 0][k] - res[0, 1][k]).max() <= pc.TOL, (k, float(np.abs(res[0, 0][k] - res[0, 1][k]).max()))
        assert np.abs(res[1, 0][k] - res[1, 1][k]).max() <= pc.TOL, k
