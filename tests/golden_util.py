"""Helpers to read the committed golden fixtures (tests/golden/*.npz)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    return np.load(os.path.join(GOLDEN, name))


def sga_case_names():
    z = load("sga_golden.npz")
    return sorted({k.split(".")[0] for k in z.files})


def lga_case_names():
    z = load("lga_golden.npz")
    return sorted({k.split(".")[0] for k in z.files})


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bit_equal(a, b, what=""):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = bits(a) != bits(b)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} words differ, max abs {np.abs(a - b).max()}"


# ---- full-size digests (tests/golden/digests.json, made by tests/golden/make_golden.py --digests from oracle/_ref) -------------
def _l1norm(g, axis):
    return (g / np.abs(g).sum(axis, keepdims=True)).astype(np.float32)


def load_digests():
    import json
    with open(os.path.join(GOLDEN, "digests.json")) as fh:
        return json.load(fh)


# The inputs are the seeded ones of tests/test_gpu_parity.py (test_full_size_cfg2_against_oracle, test_sga_model_shapes_vs_oracle,
# test_lga_model_shapes_vs_oracle): numpy's default_rng (PCG64) is a documented stable stream, and the digests of the INPUTS are
# stored too, so a change of the generator would be noticed as such.
SGA_DIGEST_CASES = [  # (name, shape, seed)
    ("sga_cfg2", (1, 32, 65, 80, 208), 123),                       # BASELINE configs[1]
    ("sga_b", (1, 48, 33, 40, 104), 1 + 48 + 33 + 40 + 104),        # the 1/6-resolution volumes of cfg2 / cfg4
    ("sga_cfg3", (1, 32, 65, 128, 416), 1 + 32 + 65 + 128 + 416),   # KITTI 1248x384
]
LGA_DIGEST_CASES = [  # (name, shape, seed): Lga2Function, radius 2
    ("lga2_cfg2", (1, 193, 240, 624), 123),
    ("lga2_cfg3", (1, 193, 384, 1248), 1 + 193 + 384 + 1248),
]


def sha(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def sga_digest_inputs(shape, seed):
    """= tests/parity_cases.sga_inputs"""
    rng = np.random.default_rng(seed)
    N, C, D, H, W = shape
    x = rng.standard_normal(shape).astype(np.float32)
    gs = [_l1norm(rng.standard_normal((N, C, 5, H, W)), 2) for _ in range(4)]
    go = rng.standard_normal(shape).astype(np.float32)
    return x, gs, go


def lga_digest_inputs(shape, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape).astype(np.float32)
    f = _l1norm(rng.standard_normal((shape[0], 75) + tuple(shape[2:])), 1)
    gy = rng.standard_normal(shape).astype(np.float32)
    return x, f, gy


def sga_digests(ora, shape, seed, inputs=None, canon=False):
    """every array SgaFunction produces, forward and backward, as the oracle `ora` computes it -> {name: sha256}
    (`inputs`: another seeded input family; `canon`: float arrays hashed with -0 turned into +0, see canon_zero)"""
    x, gs, go = (inputs or sga_digest_inputs)(shape, seed)
    d = {"in.x": sha(x), "in.go": sha(go), **{f"in.g{k}": sha(gs[k]) for k in range(4)}}
    c = canon_zero if canon else (lambda a: a)
    out, tmp, mask = ora.sga_forward(x, *gs)
    d.update({"out": sha(c(out)), "temp_out": sha(c(tmp)), "mask_u8": sha(mask.astype(np.uint8))})
    for k in range(4):
        d[f"A{k}"] = sha(c(ora.sga_scan(x, gs[k], k)))
    for n, g in zip(("gx", "gw0", "gw1", "gw2", "gw3"), ora.sga_backward(x, *gs, tmp, mask, go)):
        d[n] = sha(c(g))
    return d


def lga_digests(ora, shape, seed, inputs=None, canon=False):
    x, f, gy = (inputs or lga_digest_inputs)(shape, seed)
    d = {"in.x": sha(x), "in.f": sha(f), "in.gy": sha(gy)}
    y, ins = ora.lga_chain_forward(x, f, 2, 2)
    gx, gf = ora.lga_chain_backward(ins, f, gy, 2)
    c = canon_zero if canon else (lambda a: a)
    d.update({"t1": sha(c(ins[1])), "y": sha(c(y)), "gx": sha(c(gx)), "gf": sha(c(gf))})
    return d


# ---- the value families (tests/parity_cases.py: sga_inputs_select / _dyadic / _sparse, lga_inputs_exact) pinned to the
# reference: small fixtures (make_golden.py --values -> sga_values*_golden.npz, lga_values_golden.npz) and two full-size digest
# entries (make_golden.py --value-digests, ADDED to digests.json).  On these two families every result is exactly
# representable and so independent of the order of the sums: the GRADIENT digests hold for the device build too.
VALUES_SGA_SHAPES = [("s33", (1, 2, 33, 8, 32)), ("s65", (1, 1, 65, 4, 48))]          # case name: f"{family}_{tag}"
VALUES_SGA_FAMILIES = ["select", "dyadic", "sparse"]
VALUES_SGA_FILES = [("sga_values_golden.npz", ("select", "dyadic")), ("sga_values_sparse_golden.npz", ("sparse",))]
VALUES_LGA_CASES = [("exact_r2", (1, 9, 7, 12), 2, 2), ("exact_r3", (1, 12, 19, 33), 3, 1), ("exact_5d", (2, 3, 9, 5, 8), 2, 2)]
SGA_SELECT_DIGEST = ("sga_cfg2_select", (1, 32, 65, 80, 208), 123)
LGA_EXACT_DIGEST = ("lga2_cfg2_exact", (1, 193, 240, 624), 123)


def canon_zero(a):
    """-0 -> +0 (IEEE addition): a zero's sign depends on which zero product a sum starts from, and would change the hash"""
    return np.asarray(a, np.float32) + np.float32(0)


def values_sga_case_names():
    return [f"{fam}_{tag}" for fam in VALUES_SGA_FAMILIES for tag, _ in VALUES_SGA_SHAPES]


def load_values_sga(name):
    """the fixture file that holds case `name` (f"{family}_{tag}")"""
    return load(next(fn for fn, fams in VALUES_SGA_FILES if name.split("_")[0] in fams))


def lga_exact_digest_inputs(shape, seed):
    import parity_cases as pc
    return pc.lga_inputs_exact(shape, 2, seed)


def sga_select_digest_inputs(shape, seed):
    import parity_cases as pc
    return pc.sga_inputs_select(shape, seed)




# ---- the restatement against the reference on awkward shapes (tests/test_oracle_vs_ref.py <- tests/golden/vs_ref_golden.npz,
# made by make_golden.py --vs-ref from oracle/_ref: inputs and every output of the reference, so the test needs no oracle/_ref) ---
VS_REF_SGA_SHAPES = [(1, 2, 5, 4, 3), (2, 2, 16, 7, 5), (1, 3, 34, 9, 17), (1, 1, 3, 2, 33)]
VS_REF_LGA_CASES = [((1, 6, 5, 7), 1), ((2, 9, 6, 11), 2), ((1, 2, 4, 3, 9), 2), ((1, 4, 3, 3), 3)]   # (shape, radius)


def vs_ref_key(op, shape, r=None):
    return op + "_" + "x".join(map(str, shape)) + ("" if r is None else f"_r{r}")


def vs_ref_sga_inputs(shape):
    rng = np.random.default_rng(sum(shape))
    N, C, D, H, W = shape
    x = rng.standard_normal(shape).astype(np.float32)
    gs = [_l1norm(rng.standard_normal((N, C, 5, H, W)), 2) for _ in range(4)]
    go = rng.standard_normal(shape).astype(np.float32)
    return x, gs, go


def vs_ref_lga_inputs(shape, r):
    rng = np.random.default_rng(sum(shape) + r)
    fs = list(shape)
    fs[-3] = 3 * (2 * r + 1) ** 2
    x = rng.standard_normal(shape).astype(np.float32)
    f = _l1norm(rng.standard_normal(fs), -3)
    gy = rng.standard_normal(shape).astype(np.float32)
    return x, f, gy
