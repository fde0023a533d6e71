"""TEST INFRASTRUCTURE: the large-offset cases of conv32x1 on a 16-bit x (include/ganet_hip_conv16.h) -- x and grad_x just past
2^31 ELEMENTS (4 GiB of 16-bit storage each) -- in the replicated-pool arrangement of tests/large_cases.py, whose Layout, Spec,
Case, contexts, Checker and teeth are used as they are.  One case per format.  An exact family (x in 1/16, w in 1/8, grad_y in
1/64): y EQUALS the float64 statement, grad_x EQUALS it rounded once to the format (multiples of 2^-9 up to 54: the rounding is
at work in both formats, asserted), and grad_weight -- the sum over every slice -- EQUALS the float64 sum rounded once.
tests/test_mixed_conv_cpu.py holds the cases to large_cases' premises and teeth and shows on a numpy model that wrapped offsets
are rejected; tests/test_gpu_large_offsets_conv16.py runs them on the device."""
import numpy as np

import large_cases as lc
import mixed_cases as mc

F32, F64 = lc.F32, lc.F64
ENTRIES = ("ganet_disp_conv_forward_16", "ganet_disp_conv_backward_data_16", "ganet_disp_conv_backward_weight_16")
DIMS = (32, 9, 10, 12)            # large_cases' disp-conv block: the model's channel count, two depth chunks, W % 4 == 0


def _fmt(case):
    return mc.F16 if case.name.endswith("f16") and not case.name.endswith("bf16") else mc.BF16


def _data(case, nb):
    C, D, H, W = case.dims
    rng = case.rng()
    dy = lambda shape, bound, den: (rng.integers(-bound * den, bound * den + 1, shape) / float(den)).astype(F32)      # noqa: E731
    x = dy((nb, C, D, H, W), 2, 16)
    x16 = mc.convert(x, _fmt(case))
    assert np.array_equal(mc.up(x16, _fmt(case)), x)                   # both formats hold the family
    return {"x16": x16, "gy": dy((nb, D, H, W), 2, 64), "_w": dy((1, C, 3, 3, 3), 1, 8)}


def _ref(case, inp):
    import disp_conv_ref64 as ref
    nb, fmt = case.layout.nb, _fmt(case)
    C, D, H, W = case.dims
    x64, g64, w64 = mc.up(inp["x16"], fmt).astype(F64), inp["gy"].astype(F64), inp["_w"].astype(F64).reshape(C, 3, 3, 3)
    # products are multiples of 2^-10 (x gy) resp. 2^-9 (w gy): y as in disp_conv_cases.premises; a workgroup's weight-gradient row
    # sums 64 lanes x 4 pixels x 8 planes of |x gy| <= 4; grad_x sums 27 taps of |w gy| <= 2 -- all below 2^24 units
    assert 27 * C * 2 * 128 < 2 ** 24 and 64 * 4 * 8 * 4 * 1024 <= 2 ** 24 and 27 * 2 * 512 < 2 ** 24
    gw = sum(float(case.layout.count[b]) * ref.backward_weight(x64[b:b + 1], g64[b:b + 1]) for b in range(nb))
    assert np.abs(gw * 1024).max() < 2 ** 53 and np.array_equal(gw * 1024, np.round(gw * 1024))   # multiples of 2^-10: the fp64 sum is exact
    gx = ref.backward_data(g64, w64)
    gx32 = gx.astype(F32)
    assert np.array_equal(gx32.astype(F64), gx)
    gx16 = mc.convert(gx32, fmt)
    assert (mc.up(gx16, fmt) != gx32).mean() > 0.05, "the rounding is at work on a share of the elements that a wrong store cannot hide in"
    return {"y": lc._flat(ref.forward(x64, w64), nb), "gx16": lc._flat(mc.up(gx16, fmt).astype(F64), nb), "_gw": gw.astype(F32)}


def _script(ctx):
    C, D, H, W = ctx.dims
    dims = (ctx.R, C, D, H, W)
    fmt = _fmt(ctx.case)
    x, y = ctx.input("x16"), ctx.output("y")
    w = ctx.small("w", None if ctx.dry else ctx.case.inputs["_w"], shape=(1, C, 3, 3, 3))
    ctx.call(ENTRIES[0], x, w, y, *dims, fmt)
    ctx.check("y")
    ctx.free("y")
    gy = ctx.input("gy")
    n_ws = 27 * C * ctx.R * (-(-D // 8)) * (-(-(H * -(-W // 4)) // 64)) if ctx.dry else ctx.query("ganet_disp_conv_workspace", *dims)
    ws, gw = ctx.small("ws", shape=(n_ws,)), ctx.small("gw", shape=(C * 27,))
    ctx.call(ENTRIES[2], x, gy, ws, gw, *dims, fmt)
    if not ctx.dry:
        got, want = ctx.host_small("gw").reshape(C, 3, 3, 3), ctx.case.want["_gw"]
        ctx.expect(np.array_equal(got, want), f"grad_weight: {int((got != want).sum())} of {got.size} differ from the float64 sum rounded once")
        ctx.expect(bool(ctx.torch.isfinite(ctx.smalls["ws"]).all().item()), "a workspace element was left unwritten")
    ctx.unchanged("x16")
    ctx.free("x16", "ws")
    gx = ctx.output("gx16")
    ctx.call(ENTRIES[1], gy, w, gx, *dims, fmt)
    ctx.check("gx16")
    ctx.unchanged("gy")


def _tensors(C, D, H, W, fmt):
    E = C * D * H * W
    return {"x16": lc.IN(E, np.uint16), "gy": lc.IN(D * H * W), "y": lc.Spec(D * H * W, kind="equal"),
            "gx16": lc.Spec(E, np.uint16, kind="equal", fmt=fmt)}


CASES = [lc.Case(f"disp-conv16-{mc.FMT_NAME[fmt]}", "disp_conv16", ENTRIES, DIMS, _tensors(*DIMS, fmt), "x16", _data, _ref, _script, seed=fmt)
         for fmt in (mc.BF16, mc.F16)]
BY_NAME = {c.name: c for c in CASES}
