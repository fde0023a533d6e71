"""Every kernel family on an operand just past 2^31 elements, through the C ABI of the gfx950 build (tests/large_cases.py: the
table, the replicated pool, the checker; tests/test_large_cases_cpu.py shows on the CPU that the checker rejects wrapped
offsets).  Beside it: SGA with more slices than gridDim.y holds, and the launchers' size refusals that less than 1 GB reaches.

Each case takes a few seconds: about 10 GB are allocated and gathered, the launches and the comparisons run on the device, the
CPU reference sees at most seven small blocks.  A case skips only if the device has less free memory than its peak plus 4 GiB
(both numbers in the reason); on an idle MI355X none does.  One line per case goes to stdout: peak bytes, wall time, the worst
error / bar of every compared tensor (profiles/ keeps the record of one run)."""
import ctypes
import json

import numpy as np
import pytest

import large_cases as lc
import parity_cases as pc
from test_gpu_parity import api, dev  # noqa: F401  (the fixtures)

pytestmark = pytest.mark.gpu
E_INVALID, E_UNSUPPORTED = -1, -2


@pytest.mark.parametrize("case", lc.CASES, ids=repr)
def test_large_offsets(api, dev, case):
    assert api.get_option("GANET_LGA_WAVE") == 2 and api.get_option("GANET_SGA_ROWWAVE") == 1 and api.get_option("GANET_SGA_COLBLOCK") == 1
    assert api.get_option("GANET_SGA_TILED") == 1, "the default kernel families"
    res = lc.run_on_device(case, api, dev, pytest.skip)
    assert res["ratios"] and max(res["ratios"].values()) <= 1.0, res
    print("LARGE " + json.dumps({"case": case.name, "peak_bytes": res["peak"], "allocated_peak_bytes": res["measured_peak"],
                                 "seconds": round(res["seconds"], 2), "worst_ratio": {k: round(v, 4) for k, v in res["ratios"].items()}}))


def test_checker_notices_one_element_on_the_device(api, dev):
    """The device side of the checker, without a wrong kernel: after the cast case has run and passed, ONE element of its
    output is changed from the host side -- in the last slice (its own representative: the comparison with the reference must
    notice) and in an ordinary slice behind element 2^30 (the comparison with its representative must)."""
    case = lc.BY_NAME["cast"]
    torch = dev.torch
    ctx = lc.DeviceCtx(case, api, dev)
    try:
        case.script(ctx)                                   # leaves dst32 (checked: it passed) and src16 alive
        t, spec = ctx.t["dst32"], case.tensors["dst32"]
        ordinary = (1 << 30) // spec.per + 2
        assert ordinary not in case.layout.special and case.R - 1 in case.layout.special
        for k, what in ((case.R - 1, "block"), (ordinary, "representative")):
            e = spec.per - 1
            assert (k * spec.per + e >= (1 << 31)) == (k == case.R - 1)
            keep = t[0, k, e].clone()
            t[0, k, e] = keep + 1.0
            with pytest.raises(AssertionError, match=what):
                ctx.check("dst32")
            t[0, k, e] = float("nan")
            with pytest.raises(AssertionError, match=what):
                ctx.check("dst32")
            t[0, k, e] = keep
        ctx.check("dst32")
    finally:
        ctx.t.clear()
        ctx.smalls.clear()
        ctx.given.clear()
        del ctx
        torch.cuda.empty_cache()


# ---- SGA with S = N * C > 65535: the column-block family and the tiled workspace are dropped (S is gridDim.y) -------------------
MANY = (1, 65537, 5, 4, 16)


def _expand(blocks, block_of):
    """{key: [1, nb, ...]} -> the same over every slice"""
    return {k: np.ascontiguousarray(v[:, block_of]) for k, v in blocks.items()}


def test_sga_more_slices_than_grid_y(api, dev, port_oracle):
    """[1, 65537, 5, 4, 16] (W % 16 == 0, H % 4 == 0: tiled at S = 65535, not here), forward and backward with their steps
    against the oracle on randn at parity_cases' bars, and EQUAL to sga_ref64 on the select family.  The references see the
    distinct blocks of a replicated pool (large_cases.Layout: P blocks, the first and the last slice their own) -- sga_ref64 on
    all 65537 slices takes over a minute.  Device only: the emulator pays per launched block, and a dozen launches of 65537
    blocks and more are minutes there (as misc_cases' residual-gridy)."""
    import sga_ref64_cases as sc
    N, C, D, H, W = MANY
    assert api.query("ganet_sga_workspace_layout", *MANY) == 0
    assert api.query("ganet_sga_workspace_layout", 1, 65535, D, H, W) == 1
    lay = lc.Layout(C, D * H * W)
    small = (1, lay.nb, D, H, W)
    # randn against the oracle
    x, gs, go = pc.sga_inputs(small, seed=65537)
    want = _expand(pc.oracle_sga_want(port_oracle, x, gs, go), lay.block_of)
    ex = lambda a: np.ascontiguousarray(a[:, lay.block_of])                  # noqa: E731
    err = pc.check_sga_forward_backward(api, dev, ex(x), [ex(g) for g in gs], ex(go), want, per_dir=True)
    assert max(err.values()) <= pc.TOL, err
    # select against the float64 statement: equality, gradients and adjoint-free volumes alike
    x, gs, go = pc.sga_inputs_select(small, seed=65538)
    pc.assert_select_exact(x, gs, go)
    ref = sc.ref64(x, gs, go)
    want = sc.to_fp32(ref, sc.FWD + sc.GRADS)
    want["mask"] = ref["mask"]
    want = _expand(want, lay.block_of)
    res = {}
    pc.check_sga_forward_backward(api, dev, ex(x), [ex(g) for g in gs], ex(go), want, per_dir=False, results=res)
    sc.assert_equal(res, want, sc.GRADS, "select, 65537 slices")
    dev.release()
    dev.torch.cuda.empty_cache()


# ---- the launchers' size refusals ---------------------------------------------------------------------------------------------
def _hip_last_error():
    """hipGetLastError of the runtime this process has mapped (the calling thread's)"""
    with open("/proc/self/maps") as fh:
        paths = sorted({line.split()[-1] for line in fh if "libamdhip64" in line})
    assert len(paths) == 1, paths
    fn = ctypes.CDLL(paths[0]).hipGetLastError
    fn.restype = ctypes.c_int
    return fn()


def _refused(api, dev, code, entry, outputs, *args):
    """the call answers `code`, leaves every output as it was (NaN / poison) and the runtime's error state clean"""
    torch = dev.torch
    torch.cuda.synchronize()
    assert _hip_last_error() == 0, "an earlier error was pending"
    rc = getattr(api._lib, entry)(*[a.data_ptr() if hasattr(a, "data_ptr") else a for a in args], dev.stream)
    assert rc == code, (entry, rc, api.last_error())
    assert api.last_error(), entry
    torch.cuda.synchronize()
    for t in outputs:
        assert bool((torch.isnan(t) if t.dtype.is_floating_point else (t == 113)).all().item()), (entry, "a refused call wrote an output")
    assert _hip_last_error() == 0, (entry, "left an error behind")


def test_size_refusals(api, dev):
    """Every size refusal of ganet_capi.hip that operands below 1 GB reach: LGA with B > 65535 on the general entries (B is
    grid.z), SGA with D > 65535 (kp is uint16), the fused tail with Do >= 2^24 (the disparity index must be exact in float).
    The others need operands no test can hold: large_cases.UNREACHABLE_REFUSALS names them with the reason."""
    assert len(lc.UNREACHABLE_REFUSALS) == 3
    e, z = dev.empty, dev.zeros
    # LGA: B = 65536 slices of [2, 3, 4]
    B, D, H, W = 65536, 2, 3, 4
    x, f, gy = z((B, D, H, W)), z((B, 75, H, W)), z((B, D, H, W))
    y, gx, gf = e((B, D, H, W)), e((B, D, H, W)), e((B, 75, H, W))
    _refused(api, dev, E_UNSUPPORTED, "ganet_lga_forward", [y], x, f, y, B, D, H, W, 2)
    _refused(api, dev, E_UNSUPPORTED, "ganet_lga_backward", [gx, gf], x, f, gy, gx, gf, B, D, H, W, 2, 0)
    del x, f, gy, y, gx, gf
    # SGA: D = 65536 on one scanline of four pixels
    N, C, D, H, W = 1, 1, 65536, 1, 4
    x, gs = z((N, C, D, H, W)), [z((N, C, 5, H, W)) for _ in range(4)]
    A, out, mask, kp = e((4, N, C, D, H, W)), e((N, C, D, H, W)), e((N, C, D, H, W), np.uint8), e((4, N, C, H, W), np.uint16)
    _refused(api, dev, E_UNSUPPORTED, "ganet_sga_forward", [A, out, mask, kp], x, *gs, A, out, mask, kp, N, C, D, H, W)
    A0 = z((4, N, C, D, H, W))
    _refused(api, dev, E_UNSUPPORTED, "ganet_sga_merge", [out, mask, kp], A0, out, mask, kp, N, C, D, H, W)
    tmp, maskf, idx, go, tg = z((N, C, D, H, W)), z((N, C, D, H, W)), e((N, C, H, W)), z((N, C, D, H, W)), e((N, C, D, H, W))
    gxc, gws = e((N, C, D, H, W)), [e((N, C, 5, H, W)) for _ in range(4)]
    _refused(api, dev, E_UNSUPPORTED, "ganet_sga_backward_compat", [idx, tg, gxc] + gws, x, *gs, tmp, maskf, idx, go, tg, gxc, *gws, N, C, D, H, W)
    # the fused tail: Do = 2^24 (nothing of that size is allocated: the up-sampled volume is never materialised)
    x1, g1 = z((1, 1, 1, 1)), z((1, 1, 1))
    o, mx, ss, gc, gx1 = e((1, 1, 1)), e((1, 1, 1)), e((1, 1, 1)), e((1, 1, 1, 1)), e((1, 1, 1, 1))
    dims = (1, 1, 1, 1, 1 << 24, 1, 1)
    _refused(api, dev, E_INVALID, "ganet_up_softmin_regression_forward", [o, mx, ss], x1, o, mx, ss, *dims)
    _refused(api, dev, E_INVALID, "ganet_up_softmin_regression_backward", [gc, gx1], x1, z((1, 1, 1)), z((1, 1, 1)), z((1, 1, 1)) + 1, g1, gc, gx1, *dims)
