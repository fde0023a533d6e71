"""TEST INFRASTRUCTURE: the large-offset cases of the channels-last BatchNorm site (include/ganet_hip_cl.h) -- x and y just past
2^31 ELEMENTS, one case per direction of the layout change (channels-last -> planar, planar -> channels-last) -- in the
replicated-pool arrangement of tests/large_cases.py, whose Layout, Spec, Case, contexts, Checker and teeth are used as they are.
The slice axis is N: slice n of a planar tensor is [C][S], of a channels-last one [S][C], both contiguous.  Representatives are
held to the numpy statement of tests/cl_cases.py bit for bit, every other slice to its representative on the device.
tests/test_cl_cpu.py holds the cases to large_cases' premises and teeth; tests/test_gpu_large_offsets_cl.py runs them."""
import numpy as np

import cl_cases as cc
import large_cases as lc

F32 = lc.F32
ENTRIES = ("ganet_bn_apply_forward_cl",)
DIMS = (32, 1040)                 # C (the model's; 16-byte requests), S = 8 tiles of CL_T and a rest of 16: N = 64529 slices
FORMS = {"bn-cl-to-planar": (cc.CL, cc.PLANAR), "bn-planar-to-cl": (cc.PLANAR, cc.CL)}


def _data(case, nb):
    C, S = case.dims
    rng = case.rng()
    x = (rng.normal(0, 1.5, (nb, C, S)) + rng.normal(0, 1, (1, C, 1))).astype(F32)
    scale = (rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C)).astype(F32)
    shift = rng.normal(0, 0.5, C).astype(F32)
    return {"x": lc._flat(cc.image(x, FORMS[case.name][0]), nb), "_scale": scale, "_shift": shift}


def _ref(case, inp):
    C, S = case.dims
    nb = case.layout.nb
    xl, yl = FORMS[case.name]
    x = cc.values(inp["x"].reshape(-1), xl, nb, C, S)
    y = cc.bn_statement(x, None, inp["_scale"], inp["_shift"], 1)
    assert (y == 0).mean() > 0.1 and (y > 0).mean() > 0.1            # the ReLU is at work on both sides
    return {"y": lc._flat(cc.image(y, yl), nb)}


def _script(ctx):
    C, S = ctx.dims
    xl, yl = FORMS[ctx.case.name]
    x, y = ctx.input("x"), ctx.output("y")
    sc = ctx.small("scale", None if ctx.dry else ctx.case.inputs["_scale"], shape=(C,))
    sh = ctx.small("shift", None if ctx.dry else ctx.case.inputs["_shift"], shape=(C,))
    ctx.call(ENTRIES[0], x, None, sc, sh, y, ctx.R, C, S, 1, xl, cc.PLANAR, yl)
    ctx.check("y")
    ctx.unchanged("x")


def _tensors(C, S):
    return {"x": lc.IN(C * S), "y": lc.Spec(C * S, kind="bits")}


CASES = [lc.Case(name, "bn_cl", ENTRIES, DIMS, _tensors(*DIMS), "x", _data, _ref, _script, seed=i) for i, name in enumerate(FORMS)]
BY_NAME = {c.name: c for c in CASES}
