"""SGA against its float64 definition (tests/sga_ref64.py): the cases shared by tests/test_sim_sga_ref64.py (oracle and emulator
build) and tests/test_gpu_sga_ref64.py (gfx950 build).

*select* (parity_cases.sga_inputs_select): every result is an integer below 2^24, so the definition fixes every bit -- ties,
merge order and integer gradients included -- and the comparison is EQUALITY.
*randn* (parity_cases.sga_inputs): the comparison is |got - float64| <= FACTOR * bound per element, with sga_ref64's
first-order bound; FACTOR = 2 is for the second-order terms that analysis drops.  It applies only where fp32 and float64 make
the same selections: RANDN_SEEDS holds, per shape, a seed for which sga_ref64.unstable() == 0 over the whole volume (searched
on the CPU; asserted by randn_case before anything is compared).
*sparse* (exact ties, values that are not exact): the selections are taken from the fp32 side and only then is float64
evaluated -- sparse_case."""
import functools

import numpy as np

import parity_cases as pc
import sga_ref64 as r64
import value_cases as vc

FACTOR = 2
FWD = ("A0", "A1", "A2", "A3", "out", "tmp")
GRADS = ("gx", "gw0", "gw1", "gw2", "gw3")
ADJOINTS = ("G0", "G1", "G2", "G3")
BOUND_OF = {"tmp": "E_A3"}                               # every other key k: E_k

WIDE_SCAN_DEEP_SHAPE = (1, 1, 300, 3, 12)                # D > 272: the whole wavefront on one scanline by default
ROW_DEPTH_SHAPES = [(1, 1, D, 2, 40) for D in vc.SGA_ROW_DEPTHS]
FORCED_SHAPES = [s for o in vc.SGA_FORCED for s in o[3]]
ALL_SHAPES = list(dict.fromkeys(vc.SGA_DEFAULT_SHAPES + vc.SGA_TILED_SHAPES + FORCED_SHAPES + vc.SGA_COMPAT_SHAPES
                                + vc.SGA_INFER_SHAPES + ROW_DEPTH_SHAPES + [vc.SGA_SEGMENT_FALLBACK_SHAPE, WIDE_SCAN_DEEP_SHAPE]))
SMALL_SHAPES = [s for s in ALL_SHAPES if s not in ROW_DEPTH_SHAPES and s[2] <= 100]      # what the emulator runs

# shape -> the first seed >= value_cases.seed_of(shape) whose randn inputs are stable (no selection within the bounds of a tie)
RANDN_SEEDS = {
    (2, 1, 20, 9, 20): 52, (1, 1, 9, 6, 14): 31, (1, 2, 6, 5, 7): 21, (1, 1, 33, 8, 32): 76, (1, 1, 65, 4, 48): 119,
    (1, 2, 33, 3, 20): 59, (1, 1, 65, 5, 20): 92, (1, 1, 100, 5, 20): 127, (1, 1, 65, 7, 12): 86, (1, 1, 65, 5, 12): 84,
    (1, 1, 300, 3, 12): 317, (1, 2, 33, 8, 32): 76, (1, 1, 49, 5, 7): 63, (1, 3, 33, 4, 12): 53, (2, 2, 9, 5, 7): 25,
    (1, 1, 39, 2, 40): 83, (1, 1, 40, 2, 40): 84, (1, 1, 41, 2, 40): 85, (1, 1, 48, 2, 40): 92, (1, 1, 49, 2, 40): 93,
    (1, 1, 64, 2, 40): 108, (1, 1, 65, 2, 40): 111, (1, 1, 72, 2, 40): 116, (1, 1, 73, 2, 40): 118, (1, 1, 240, 4, 12): 258,
}


def ref64(x, gs, go, kp=None, mask=None):
    """forward and backward of the definition in one dict (values float64, bounds E_*)"""
    fwd = r64.forward(x, *gs, kp=kp, mask=mask)
    return {**fwd, **r64.backward(x, gs, go, fwd)}


def _freeze(*dicts):
    """shared between tests (lru_cache): nobody writes to a reference"""
    for v in dicts:
        for a in v.values():
            a.setflags(write=False)


def to_fp32(ref, keys):
    """the float64 results as fp32, asserted to be representable (the *select* family)"""
    want = {}
    for k in keys:
        want[k] = ref[k].astype(np.float32)
        assert np.array_equal(want[k].astype(np.float64), ref[k]), k
    return want


@functools.lru_cache(maxsize=None)
def select_case(shape, seed=None):
    """-> x, gs, go, ref (float64), want (the same as fp32 / uint8, in the form parity_cases' checks take)"""
    x, gs, go = pc.sga_inputs_select(shape, vc.seed_of(shape) if seed is None else seed)
    pc.assert_select_exact(x, gs, go)
    ref = ref64(x, gs, go)
    pc.assert_sga_ties("select", [ref[f"A{d}"] for d in range(4)])
    want = to_fp32(ref, FWD + GRADS + ADJOINTS)
    want["mask"] = ref["mask"]
    for k in GRADS + ADJOINTS:
        assert np.array_equal(ref[k], np.round(ref[k])), k
    _freeze(ref, want)
    return x, gs, go, ref, want


@functools.lru_cache(maxsize=None)
def randn_case(shape):
    x, gs, go = pc.sga_inputs(shape, RANDN_SEEDS[shape])
    ref = ref64(x, gs, go)
    assert r64.unstable(ref) == 0, (shape, RANDN_SEEDS[shape], r64.unstable(ref), r64.selection_gaps(ref))
    _freeze(ref)
    return x, gs, go, ref


def sparse_case(oracle, shape):
    """-> x, gs, go, the oracle's results, and float64 on the ORACLE's selections (its mask, the first arg-max of its volumes)"""
    x, gs, go, want = vc.sga_case(oracle, "sparse", shape)
    kp = np.stack([np.argmax(want[f"A{d}"], 2) for d in range(4)])
    return x, gs, go, want, ref64(x, gs, go, kp=kp, mask=want["mask"])


def ratios(got, ref, keys):
    """key -> largest |got - float64| / bound over the elements (an element whose bound is 0 must be met exactly)"""
    out = {}
    for k in keys:
        err = np.abs(got[k].astype(np.float64) - ref[k])
        bound = ref[BOUND_OF.get(k, "E_" + k)]
        assert err.shape == bound.shape, k
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0, 0.0, err / bound)              # err > 0 on a zero bound: inf
        out[k] = float(q.max())
    return out


def assert_within_bound(got, ref, keys, what=""):
    q = ratios(got, ref, keys)
    assert max(q.values()) <= FACTOR, (what, {k: v for k, v in q.items() if v > FACTOR})
    return q


def assert_equal(got, ref, keys, what=""):
    for k in keys:
        assert got[k].shape == ref[k].shape, k
        assert np.array_equal(got[k], ref[k]), (what, k, int((got[k] != ref[k]).sum()), float(np.abs(got[k] - ref[k]).max()))


def assert_selections_equal(got, ref, what=""):
    assert np.array_equal(got["mask"].astype(np.uint8), ref["mask"]), (what, "mask")
    if "kp" in got:
        assert np.array_equal(np.asarray(got["kp"], np.int64), ref["kp"]), (what, "kp")


def oracle_results(oracle, x, gs, go):
    """parity_cases.oracle_sga_want plus the first arg-max of the oracle's volumes"""
    want = pc.oracle_sga_want(oracle, x, gs, go)
    want["kp"] = np.stack([np.argmax(want[f"A{d}"], 2) for d in range(4)])
    return want


def device_volumes(api, dev, x, gs, go):
    """forward, then the adjoint volume of each direction from ganet_sga_backward_scan (API layout):
    -> A0..A3, out, tmp, mask, kp, G0..G3 as host arrays"""
    N, C, D, H, W = x.shape
    dx, dg, A, out, mask, kp = pc.run_sga_forward(api, dev, x, gs)
    hA = np.array(dev.host(A))
    got = {f"A{d}": hA[d] for d in range(4)}
    got.update(out=np.array(dev.host(out)), tmp=hA[3], mask=np.array(dev.host(mask)), kp=np.array(dev.host(kp)))
    dgo = dev.to(go)
    for d in range(4):
        G = dev.empty(x.shape)
        api.call("ganet_sga_backward_scan", dev.ptr(dg[d]), dev.ptr(mask), dev.ptr(kp) + 2 * d * (N * C * H * W), dev.ptr(dgo),
                 dev.ptr(G), N, C, D, H, W, d, dev.stream)
        dev.sync()
        got[f"G{d}"] = np.array(dev.host(G))
    return got


def run_select(api, dev, shape, seed=None, per_dir=True, compat=False):
    """the library on *select* with the float64 results (as fp32) as `want`: volumes, out, mask, arg-max, the adjoint volumes
    and all five gradients EQUAL the definition's"""
    x, gs, go, ref, want = select_case(shape, seed)
    res = {}
    pc.check_sga_forward_backward(api, dev, x, gs, go, want, per_dir=per_dir, results=res)
    assert_equal(res, want, GRADS, "select")
    got = device_volumes(api, dev, x, gs, go)
    assert_selections_equal(got, ref, "select")
    assert_equal(got, want, FWD + ADJOINTS, "select")
    if compat:
        pc.check_sga_compat(api, dev, x, gs, go, want)


def run_randn(api, dev, oracle, shape, per_dir=False):
    """the library on a stable randn case: parity_cases' check against the oracle as everywhere else, then volumes, adjoint
    volumes and gradients within FACTOR * bound of float64.  -> key -> largest error / bound"""
    x, gs, go, ref = randn_case(shape)
    res = {}
    pc.check_sga_forward_backward(api, dev, x, gs, go, oracle_results(oracle, x, gs, go), per_dir=per_dir, results=res)
    got = device_volumes(api, dev, x, gs, go)
    assert_selections_equal(got, ref, "randn")
    q = assert_within_bound(got, ref, FWD + ADJOINTS, ("randn", shape))
    q.update(assert_within_bound(res, ref, GRADS, ("randn", shape)))
    return q


def run_select_infer(api, dev, shape, with_bn):
    """ganet_sga_forward_infer on *select*: `out` (through the BN + ReLU epilogue too) equal to the definition's"""
    x, gs, go, ref, want = select_case(shape)
    vc.check_sga_infer(api, dev, x, gs, want["out"], with_bn)


def fmt(q):
    return " ".join(f"{k}={v:.3f}" for k, v in q.items())
