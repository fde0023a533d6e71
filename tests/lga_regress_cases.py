"""TEST INFRASTRUCTURE: one float64 case table for LgaRegress -- one LGA pass with the normalised regression in its epilogue, and
the backward chain behind it (ganet_lga_forward_regress, or radius 3's fallback ganet_lga_forward +
ganet_norm_disparity_regression_forward; ganet_norm_disparity_regression_backward; ganet_lga_backward) -- run unchanged by
tests/test_sim_fused.py (the emulator build, the three ABI entries called directly) and tests/test_gpu_fused.py (the device,
through LgaRegressFunction under the recorder of tests/model_calls.py).  Every case is judged by model_calls.check_lga_regress
on a Record: the checker that judges the op inside a model run is the one that is exercised here, at the kink it has to
know about.

Until now the fused pass was held to float64 only where every |y| is 1 (autograd_cases.LgaRegress) and by its two sums.

Shapes (the smallest that reach each arm): radius 1, 2 and 3 (3: no fused kernel, E_UNSUPPORTED, asserted); N = 2; widths
that are no multiple of the LGA tile and odd (9, 11, 37; 37 and 40 are wider than one 32-column tile); H W % 4 == 0 (36, 200:
norm_disp_regression_bwd4) and != 0 (170, 66, 185: norm_disp_regression_bwd).

Families, all on model-like values -- x a softmin volume, signed L1-normalised filters, go of 1e-4:
  general   as drawn.  No element is expected near the kink: the checker's cap on undecided elements holds as in a model run.
  planted   the same inputs with y PUT at the kink on a sparse lattice.  y[p] is linear in x[p], with the coefficient
            c = f_centre + the taps that leave the volume at p (they read the centre value): x[p] <- fl32(x[p] - y64[p] / c)
            leaves y64[p] = c * (the rounding of x[p]), of order u |c x[p]|, below E_y = gamma_75 sum |f| |v| which holds that
            very term.  Lattice: every 3rd d, every (2r+3)-th row and column -- no lattice element reads another -- and only
            where |c| >= 1 / T (the mean |f|: x stays of its magnitude).  Asserted on the CPU before anything is compared:
            every planted element is undecided; the undecided set is the planted set plus at most the checker's cap (both
            inside check_lga_regress, `planted`); and a plain fp32 numpy pass (forward32) gives at least one planted element
            the sign float64 does not -- the seeds below were chosen on the CPU for that and are pinned.
            This is the deterministic form of a failure a model run showed now and then: gx at 32 x its bar, from a
            reference that took sgn(y) from float64 where the device's fp32 y had the other sign.
  clamped   x exactly zero on a patch of 2r+2 rows (all rows, where H is smaller) and 2r+3 columns over every d of sample
            0: the pixels whose whole window lies inside have y == 0 -- sgn(0) = 0, the norm clamped to eps, out = 0 -- and go is
            zero there (go d / eps would otherwise dominate the absolute part of every other element's bar).  Asserted: such
            pixels exist, and the call's out and snorm say so.

With and without autograd: the call that keeps no volume (y = NULL; under no_grad) returns the same bits in `out`."""
import numpy as np

import lga_ref64
import misc_ref64 as m64
import model_calls as M

F32 = np.float32
SHAPES = [((1, 5, 4, 9), 1), ((2, 6, 5, 34), 2), ((2, 9, 6, 11), 2), ((1, 4, 5, 40), 3), ((2, 9, 5, 37), 2)]
FAMILIES = ("general", "planted", "clamped")
# per (shape, radius): the first seed whose planted family has an element with the other sign in forward32 (chosen by
# `python tests/lga_regress_cases.py`, which prints this table)
SEEDS = {((1, 5, 4, 9), 1): 0, ((2, 6, 5, 34), 2): 0, ((2, 9, 6, 11), 2): 0, ((1, 4, 5, 40), 3): 0, ((2, 9, 5, 37), 2): 0}
CASES = [(shape, r, fam) for shape, r in SHAPES for fam in FAMILIES]


def case_id(case):
    shape, r, fam = case
    return "%s-r%d-%s" % ("x".join(map(str, shape)), r, fam)


# ---- a plain fp32 statement of the op: numpy, tap by tap, every intermediate float32 ----------------------------------------------
def _tap_values(x, dst, src):
    v = x.copy()                                      # outside: the centre value
    v[(slice(None),) + dst] = x[(slice(None),) + src]
    return v


def forward32(x, f, r):
    assert x.dtype == F32 and f.dtype == F32
    y = np.zeros_like(x)
    for t, dst, src in lga_ref64._taps(r, *x.shape[1:]):
        y += f[:, t][:, None] * _tap_values(x, dst, src)
    return y


def backward32(x, f, g, r):
    assert x.dtype == F32 and f.dtype == F32 and g.dtype == F32
    D, H, W = x.shape[1:]
    gx, gf = np.zeros_like(x), np.zeros_like(f)
    for t, dst, src in lga_ref64._taps(r, D, H, W):
        gf[:, t] = (g * _tap_values(x, dst, src)).sum(1, dtype=F32)
        c = f[:, t][:, None] * g
        inside = np.zeros((D, H, W), bool)
        inside[dst] = True
        gx += np.where(inside, F32(0), c)
        gx[(slice(None),) + src] += c[(slice(None),) + dst]
    return gx, gf


def regress32(x, f, go, r, y=None):
    """-> dict(y, snorm, out, gx, gf) in fp32.  y: a volume to go on from instead of forward32's (a test that spoils it)"""
    D = x.shape[1]
    d = np.arange(D, dtype=F32).reshape(1, D, 1, 1)
    y = forward32(x, f, r) if y is None else y
    assert y.dtype == F32
    raw = np.abs(y).sum(1, dtype=F32)
    snorm = np.maximum(raw, F32(m64.EPS))
    out = (y * d).sum(1, dtype=F32) / snorm
    res = {"y": y, "snorm": snorm, "out": out}
    if go is not None:
        ov = np.where(raw < F32(m64.EPS), F32(0), out)
        gy = (go[:, None] * ((d - ov[:, None] * np.sign(y)) / snorm[:, None])).astype(F32)
        res["gx"], res["gf"] = backward32(x, f, gy, r)
    return res


def record(x, f, r, res, go=None):
    """what the recorder of model_calls keeps of one LgaRegressFunction call with these results"""
    rec = M.Record("LgaRegressFunction", [x, f, r, x.shape[1]], go is not None)
    rec.outputs = [res["out"]]
    if go is not None:
        rec.grad_out, rec.grad_in = [go], [res["gx"], res["gf"], None, None]
        rec.saved = {"y": res["y"], "snorm": res["snorm"]}
    return rec


# ---- the inputs --------------------------------------------------------------------------------------------------------------------
def model_like(shape, r, seed):
    B, D, H, W = shape
    rng = np.random.default_rng(seed)
    x = m64.softmin(rng.standard_normal(shape) * 3).astype(F32)
    f = rng.standard_normal((B, 3 * (2 * r + 1) ** 2, H, W))
    f = (f / np.abs(f).sum(1, keepdims=True)).astype(F32)
    go = (rng.standard_normal((B, H, W)) * 1e-4).astype(F32)
    return x, f, go


def own_coefficient(f, r, D, H, W):
    """dy[b,d,i,j] / dx[b,d,i,j]: the centre tap and every tap that leaves the volume at (d, i, j)"""
    f = f.astype(np.float64)
    c = np.zeros((f.shape[0], D, H, W))
    for t, dst, _ in lga_ref64._taps(r, D, H, W):
        inside = np.zeros((D, H, W), bool)
        inside[dst] = True
        c += np.where(inside, 0.0, f[:, t][:, None])
    ws = 2 * r + 1
    return c + f[:, ws * ws + r * ws + r][:, None]


def plant(x, f, r):
    """-> (x with y put at the kink on the lattice, the mask of those elements)"""
    B, D, H, W = x.shape
    c = own_coefficient(f, r, D, H, W)
    lattice = np.zeros(x.shape, bool)
    lattice[:, 1::3, 1::2 * r + 3, 2::2 * r + 3] = True
    lattice &= np.abs(c) >= 1.0 / f.shape[1]
    y = lga_ref64.lga_forward(x, f, r)
    xp = np.where(lattice, (x.astype(np.float64) - y / np.where(lattice, c, 1.0)).astype(F32), x)
    return xp, lattice


def make(case, seed=None):
    """-> x, f, go, planted (a mask, or None), after the family's conditions on the CPU"""
    shape, r, fam = case
    B, D, H, W = shape
    x, f, go = model_like(shape, r, SEEDS[shape, r] if seed is None else seed)
    planted = None
    if fam == "planted":
        x, planted = plant(x, f, r)
        assert planted.sum() >= 2, (case, int(planted.sum()))
        y64, E_y, und = M.lga_regress_undecided(x, f, r)
        assert und[planted].all() and (np.abs(y64[planted]) <= E_y[planted] / (M.FACTOR * 8)).all(), case      # far inside, not at the edge
        assert float(np.abs(x).max()) < 64, (case, float(np.abs(x).max()))
        assert other_signs(x, f, r, planted) >= 1, (case, "no planted element changes sign in fp32: choose another seed")
    elif fam == "clamped":
        rows, cols = slice(0, min(H, 2 * r + 2)), slice(1, 1 + 2 * r + 3)
        assert W >= 2 + 2 * r + 3
        x[0, :, rows, cols] = 0
        dead = (np.abs(lga_ref64.lga_forward(x, f, r)).sum(1) == 0)
        assert dead[0].sum() >= 1 and not dead[1:].any(), (case, "the patch is not reached")
        go[dead] = 0
        assert np.count_nonzero(go) >= go.size // 2
    return x, f, go, planted


def other_signs(x, f, r, planted):
    """planted elements to which forward32 gives another sign than float64"""
    return int((np.sign(forward32(x, f, r).astype(np.float64)) != np.sign(lga_ref64.lga_forward(x, f, r)))[planted].sum())


# ---- one case --------------------------------------------------------------------------------------------------------------------
def run(case, call):
    """call(x, f, go, r) -> dict(out, y, snorm, gx, gf, fused) of the call that keeps its volume; call(x, f, None, r) ->
    dict(out, fused) of the one that does not.  -> check_lga_regress's ratios (printed)"""
    shape, r, fam = case
    x, f, go, planted = make(case)
    res = call(x, f, go, r)
    bare = call(x, f, None, r)
    assert res["fused"] == bare["fused"] == (r <= 2), (case, "radius 1 and 2 have the fused pass, radius 3 answers E_UNSUPPORTED")
    assert np.array_equal(res["out"].view(np.uint32), bare["out"].view(np.uint32)), (case, "out differs without the volume")
    if fam == "clamped":
        dead = np.abs(lga_ref64.lga_forward(x, f, r)).sum(1) == 0
        assert (res["snorm"][dead] == F32(m64.EPS)).all() and not res["out"][dead].any() and not res["y"][np.broadcast_to(dead[:, None], shape)].any()
    q = M.check_lga_regress(record(x, f, r, res, go), planted=planted)
    M.check_lga_regress(record(x, f, r, bare), planted=planted)
    if fam == "planted":
        flipped_here = int((np.sign(res["y"].astype(np.float64)) != np.sign(lga_ref64.lga_forward(x, f, r)))[planted].sum())
        q["planted"], q["flipped_in_call"] = float(planted.sum()), float(flipped_here)
    print(case_id(case), " ".join(f"{k}={v:.3g}" for k, v in q.items()))
    return q


if __name__ == "__main__":
    table = {}
    for shape, r in SHAPES:
        for seed in range(64):
            x, f, _ = model_like(shape, r, seed)
            xp, planted = plant(x, f, r)
            if planted.sum() >= 2 and other_signs(xp, f, r, planted) >= 1:
                table[shape, r] = seed
                print(shape, r, "seed", seed, "planted", int(planted.sum()), "other signs in fp32", other_signs(xp, f, r, planted))
                break
    print("SEEDS =", table)
