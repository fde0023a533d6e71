"""SGA on the gfx950 build against the float64 statement of its definition (tests/sga_ref64.py; the cases of
tests/sga_ref64_cases.py, which the emulator runs in tests/test_sim_sga_ref64.py): on the exact *select* family volumes, out,
mask, arg-max, the adjoint volumes and the five gradients EQUAL the definition's; on stable randn inputs every one of them lies
within 2 x the per-element first-order rounding bound of the exact value.  Small volumes only -- the smallest that reach each
kernel family -- because float64 is the slow side.  Each randn case prints its largest error / bound per result."""
import pytest

import parity_cases as pc
import sga_ref64_cases as sc
import value_cases as vc
from test_gpu_parity import TorchDev

pytestmark = pytest.mark.gpu


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


def _both(api, dev, oracle, shape, what, seed=None):
    sc.run_select(api, dev, shape, seed=seed, per_dir=True)
    q = sc.run_randn(api, dev, oracle, shape, per_dir=True)
    print("device randn", what, shape, "error / bound:", sc.fmt(q))
    return q


@pytest.mark.parametrize("shape", vc.SGA_DEFAULT_SHAPES)
def test_sga_default_dispatch(api, dev, port_oracle, shape):
    _both(api, dev, port_oracle, shape, "default")


@pytest.mark.parametrize("tiled", [0, 1])
@pytest.mark.parametrize("shape", vc.SGA_TILED_SHAPES)
def test_sga_tiled_workspace(api, dev, port_oracle, shape, tiled):
    with vc.option(api, "GANET_SGA_TILED", tiled):
        assert api.query("ganet_sga_workspace_layout", *shape) == tiled
        _both(api, dev, port_oracle, shape, f"tiled={tiled}", seed=vc.seed_of(shape, 1 + tiled))


@pytest.mark.parametrize("shape", sc.ROW_DEPTH_SHAPES, ids=[f"D{s[2]}" for s in sc.ROW_DEPTH_SHAPES])
def test_sga_row_kernels_depth_boundaries(api, dev, port_oracle, shape):
    _both(api, dev, port_oracle, shape, "row depth")


@pytest.mark.parametrize("shape", [vc.SGA_SEGMENT_FALLBACK_SHAPE, sc.WIDE_SCAN_DEEP_SHAPE], ids=["segment_fallback", "wide_scan_D300"])
def test_sga_deep_volumes(api, dev, port_oracle, shape):
    """D in (208, 272]: the 16-lane segment kernels; D > 272: the whole wavefront on one scanline"""
    _both(api, dev, port_oracle, shape, "deep")


@pytest.mark.parametrize("opt,value,restore,shapes", vc.SGA_FORCED, ids=[o[0] for o in vc.SGA_FORCED])
def test_sga_forced_kernel_families(api, dev, port_oracle, opt, value, restore, shapes):
    with vc.option(api, opt, value, restore):
        for shape in shapes:
            _both(api, dev, port_oracle, shape, f"{opt}={value}")


@pytest.mark.parametrize("shape", vc.SGA_COMPAT_SHAPES)
def test_sga_reference_buffer_contract(api, dev, shape):
    x, gs, go, ref, want = sc.select_case(shape, seed=vc.seed_of(shape, 5))
    pc.check_sga_compat(api, dev, x, gs, go, want)


@pytest.mark.parametrize("with_bn", [False, True])
@pytest.mark.parametrize("shape", vc.SGA_INFER_SHAPES)
def test_sga_forward_infer(api, dev, shape, with_bn):
    sc.run_select_infer(api, dev, shape, with_bn)
