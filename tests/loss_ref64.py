"""TEST INFRASTRUCTURE: the yardstick of the fused criterion (ganet_disparity_loss_*, ganet_amd/csrc/loss_kernels.h).

The residual is fl32(p - t), as in the kernels and in the stock fp32 path; everything behind it is float64 numpy.  MyLoss2 is
written stage by stage -- the reference's three masked updates of one buffer, each condition seeing what the previous update
left (libs/GANet/functions/GANet.py:264-289; ganet_amd/functions/GANet.py `_piecewise`) -- for the value and, separately, for
the slope table.  `slope` is generic over the dtype: in float64 it is the yardstick, in float32 (every constant and every
operation fp32, individually rounded) it is the statement the kernels' gradients must equal bit for bit.
tests/test_sim_loss.py ties `loss` to harness.steps.loss_mix on float64 CPU tensors."""
import numpy as np

F32, F64 = np.float32, np.float64
PARAMS = ("hi", "lo", "w0", "w1", "w2", "thresh", "alpha", "rate")


def _chain(v, *stages):
    for cond, repl in stages:
        v = np.where(cond(v), repl(v), v)
    return v


def valid(t, hi, lo, mask_mode):
    """fp32 comparisons; a NaN target fails every one of them"""
    t = np.asarray(t, F32)
    with np.errstate(invalid="ignore"):
        return t < F32(hi) if mask_mode == 0 else (F32(lo) <= t) & (t <= F32(hi))


def rho64(v, kind, thresh, alpha):
    v = np.asarray(v, F64)
    if kind == 0:
        return np.where(v < 1, 0.5 * v * v, v - 0.5)
    knee, span, far = F64(F32(thresh)), F64(F32(alpha)), F64(F32(thresh) + F32(alpha))
    return _chain(v,
                  (lambda v: v < knee, lambda v: v * v / knee),
                  (lambda v: (v >= knee) & (v <= far), lambda v: 2 * v - (v - knee) ** 2 / (2.0 * span) - knee),
                  (lambda v: v > far, lambda v: v + span / 2.0))


def slope(v, kind, thresh, alpha, dtype):
    """the reference's slope table; every constant is of `dtype`, so with float32 every operation is an fp32 one"""
    T = dtype
    v = np.asarray(v, T)
    one, two = T(1), T(2)
    if kind == 0:
        return np.where(v >= one, one, v)          # (a NaN stays a NaN, as in torch's smooth_l1 backward)
    knee, span, far = T(F32(thresh)), T(F32(alpha)), T(F32(thresh) + F32(alpha))
    return _chain(v,
                  (lambda v: v > far, lambda v: np.full_like(v, one)),
                  (lambda v: (v >= knee) & (v <= far), lambda v: two - (v - knee) / span),
                  (lambda v: v < knee, lambda v: two * v / knee))


class Reference:
    """Everything the tests compare with, for preds (list of fp32 arrays), an fp32 target and params (dict over PARAMS)."""

    def __init__(self, preds, target, params, kinds, mask_mode):
        with np.errstate(all="ignore"):
            p = {k: F32(params[k]) for k in PARAMS}
            self.p, self.kinds = p, kinds
            self.weights = [F64(p[f"w{k}"]) for k in range(len(preds))]
            t = np.asarray(target, F32)
            self.ok = valid(t, p["hi"], p["lo"], mask_mode)
            self.count = int(self.ok.sum())
            self.r = [np.asarray(q, F32) - t for q in preds]            # fl32(p - t)
            v = [np.abs(r).astype(F64) for r in self.r]
            n = max(self.count, 1)
            self.sum_rho = [float(np.where(self.ok, rho64(v[k], kinds[k], p["thresh"], p["alpha"]), 0.0).sum()) for k in range(len(preds))]
            self.mean_rho = [s / n for s in self.sum_rho]
            self.epe = [float(np.where(self.ok, v[k], 0.0).sum()) / n for k in range(len(preds))]
            self.nrate = [int((self.ok & (v[k] > F64(p["rate"]))).sum()) for k in range(len(preds))]
            self.rate = [F32(F64(m) / F64(n)) for m in self.nrate]       # the one rounding of an exact quotient
            self.loss = float(sum(w * m for w, m in zip(self.weights, self.mean_rho)))

    def grads(self, grad_loss, dtype):
        """g_k = valid ? (sign(r) * slope) * c_k : +0, c_k = w_k * grad_loss / count in float64 -- rounded to fp32 once for the
        float32 statement; grad_loss is the fp32 value the backward reads."""
        out = []
        with np.errstate(all="ignore"):
            for k, r in enumerate(self.r):
                c = self.weights[k] * F64(F32(grad_loss)) / F64(max(self.count, 1))
                c = dtype(F32(c)) if dtype is F32 else c
                rr = r.astype(dtype)
                sg = np.where(rr > 0, dtype(1), np.where(rr < 0, dtype(-1), dtype(0)))
                g = sg * slope(np.abs(rr), self.kinds[k], self.p["thresh"], self.p["alpha"], dtype) * c
                out.append(np.where(self.ok & (self.count > 0), g, dtype(0)).astype(dtype))
        return out
