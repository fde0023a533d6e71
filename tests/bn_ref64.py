"""TEST INFRASTRUCTURE: the float64 statement of the fused training-mode BatchNorm + residual + ReLU
(ganet_bn_train_forward / _backward, ganet_amd/csrc/bn_kernels.h), and its float32 twin.

x [N, C, S] and every other input are the fp32 values the kernels read; everything behind them is float64 numpy:
  mean = sum x / M, var = mean((x - mean)^2) (biased; the two-pass form, which float64 carries without cancellation),
  invstd = 1 / sqrt(var + eps), scale = weight invstd, z = (x - mean) scale + bias [+ rem], y = relu ? (z <= 0 ? 0 : z) : z
  g = relu and z <= 0 ? 0 : grad_y, grad_bias = sum g, grad_weight = invstd sum g (x - mean), grad_rem = g
  grad_x = scale (g - sum g / M - (x - mean) invstd^2 sum g (x - mean) / M)
  running_mean = (1 - m) running_mean + m mean,  running_var = (1 - m) running_var + m var M / (M - 1)
`Float32Model` is the arithmetic of bn_kernels.h operation by operation (fp64 sums, mean and invstd rounded once, fmaf where
the kernel has one): the bars of tests/bn_cases.py are derived for it, and tests/test_sim_bn.py checks that it stays inside
half of them -- the bars come from the arithmetic, not from what the kernels return."""
import numpy as np

F32, F64 = np.float32, np.float64


def _per_channel(a):
    return a.sum(axis=(0, 2))


def _b(v):
    """[C] -> [1, C, 1]"""
    return np.asarray(v)[None, :, None]


class Reference:
    def __init__(self, x, rem, grad_y, weight, bias, running_mean, running_var, momentum, eps, relu, relu_positive=None):
        """relu_positive (recorded data, which nobody can nudge away from the kink): a boolean array that decides the ReLU at
        the elements where float64 cannot speak for fp32 -- undecided(), |z| <= 4 B_y; everywhere else z decides as always"""
        with np.errstate(all="ignore"):
            x = np.asarray(x, F32)
            N, C, S = x.shape
            self.N, self.C, self.S, self.M = N, C, S, N * S
            self.relu, self.has_rem = bool(relu), rem is not None
            M = F64(self.M)
            self.x = x.astype(F64)
            self.rem = np.zeros_like(self.x) if rem is None else np.asarray(rem, F32).astype(F64)
            self.gy = np.asarray(grad_y, F32).astype(F64)
            self.weight = np.ones(C, F64) if weight is None else np.asarray(weight, F32).astype(F64)
            self.bias = np.zeros(C, F64) if bias is None else np.asarray(bias, F32).astype(F64)
            self.eps, self.m = F64(F32(eps)), F64(F32(momentum))
            self.mean = _per_channel(self.x) / M
            self.xm = self.x - _b(self.mean)
            self.var = _per_channel(self.xm * self.xm) / M
            self.invstd = 1.0 / np.sqrt(self.var + self.eps)
            self.scale = self.weight * self.invstd
            self.z = self.xm * _b(self.scale) + _b(self.bias) + self.rem
            off = self.z <= 0
            if self.relu and relu_positive is not None:
                off = np.where(self.undecided(), ~np.asarray(relu_positive, bool).reshape(x.shape), off)
            self.y = np.where(off, 0.0, self.z) if self.relu else self.z
            self.g = np.where(off, 0.0, self.gy) if self.relu else self.gy
            self.sum_g = _per_channel(self.g)
            self.sum_gxm = _per_channel(self.g * self.xm)
            self.sum_abs_g = _per_channel(np.abs(self.g))
            self.sum_abs_gxm = _per_channel(np.abs(self.g * self.xm))
            self.grad_bias = self.sum_g
            self.grad_weight = self.invstd * self.sum_gxm
            self.k1 = self.sum_g / M
            self.q = self.invstd ** 2 * self.sum_gxm / M
            self.grad_x = _b(self.scale) * (self.g - _b(self.k1) - self.xm * _b(self.q))
            self.grad_rem = self.g
            self.mean_abs_x = _per_channel(np.abs(self.x)) / M
            if running_mean is not None:
                self.old_mean, self.old_var = np.asarray(running_mean, F32).astype(F64), np.asarray(running_var, F32).astype(F64)
                self.new_var = self.var * M / (M - 1.0)
                self.running_mean = (1 - self.m) * self.old_mean + self.m * self.mean
                self.running_var = (1 - self.m) * self.old_var + self.m * self.new_var
            else:
                self.running_mean = self.running_var = None

    # ---- the bars (tests/bn_cases.py) ----
    def bar_y(self):
        return 2.0 ** -21 * ((np.abs(self.x) + _b(np.abs(self.mean))) * _b(np.abs(self.scale)) + _b(np.abs(self.bias)) + np.abs(self.rem))

    def bar_grad_x(self, mean_term=False):
        """mean_term (bn_cases: the far-mean cases and recorded model data): the rounding of the saved mean, 2^-24 |mean|, also
        sits in sum g (x - mean) and so in q -- |xhat| invstd |k1| times it, with the factor 4 of the bars' other terms"""
        xhat = self.xm * _b(self.invstd)
        qt = self.grad_weight / F64(self.M)
        bar = _b(np.abs(self.scale)) * (2.0 ** -20 * (np.abs(self.g) + _b(np.abs(self.k1)) + np.abs(xhat * _b(qt))) +
                                        2.0 ** -23 * _b(np.abs(self.mean) * self.invstd * np.abs(qt)))
        if mean_term:
            bar = bar + _b(np.abs(self.scale)) * 2.0 ** -22 * np.abs(xhat) * _b(np.abs(self.mean) * self.invstd * np.abs(self.k1))
        return bar

    def undecided(self):
        """elements whose ReLU mask the fp32 arithmetic may decide the other way: |z| <= 4 B_y.  (A z that is exactly zero
        with a zero bar -- scale = 0, bias = 0, no residual -- is zero in fp32 as well: decided.)"""
        if not self.relu:
            return np.zeros(self.x.shape, bool)
        by = self.bar_y()
        with np.errstate(invalid="ignore"):
            return (np.abs(self.z) <= 4 * by) & (by > 0)


def _fma32(a, b, c):
    """fmaf on fp32 arrays: the product of two fp32 values is exact in float64, the sum is rounded to 53 bits and then to
    24 -- double rounding can differ from fmaf by one ulp in about 1 case in 2^29, which the half-of-the-bar check absorbs"""
    return (np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64) + np.asarray(c, F32).astype(F64)).astype(F32)


class Float32Model:
    """bn_kernels.h, operation by operation, on numpy"""

    def __init__(self, x, rem, grad_y, weight, bias, running_mean, running_var, momentum, eps, relu):
        with np.errstate(all="ignore"):
            x = np.asarray(x, F32)
            N, C, S = x.shape
            M = F64(N * S)
            x64 = x.astype(F64)
            x0 = x64[0, :, 0]
            d = x64 - _b(x0)
            dm = _per_channel(d) / M
            mean = x0 + dm
            var = np.maximum(_per_channel(d * d) / M - dm * dm, 0.0)
            self.save_mean = mean.astype(F32)
            self.save_invstd = (1.0 / np.sqrt(var + F64(F32(eps)))).astype(F32)
            w = np.ones(C, F32) if weight is None else np.asarray(weight, F32)
            b = np.zeros(C, F32) if bias is None else np.asarray(bias, F32)
            scale = (w * self.save_invstd).astype(F32)
            shift = _fma32(-self.save_mean, scale, b)
            z = _fma32(x, _b(scale), _b(shift))
            if rem is not None:
                z = (z + np.asarray(rem, F32)).astype(F32)
            self.y = np.where(z <= 0, F32(0), z) if relu else z
            gy = np.asarray(grad_y, F32)
            g = np.where(z <= 0, F32(0), gy) if relu else gy
            sg = _per_channel(g.astype(F64))
            sgx = _per_channel(g.astype(F64) * (x64 - _b(self.save_mean.astype(F64))))
            inv = self.save_invstd.astype(F64)
            self.grad_bias, self.grad_weight = sg.astype(F32), (inv * sgx).astype(F32)
            k1, q = (sg / M).astype(F32), (inv * inv * sgx / M).astype(F32)
            xm = (x - _b(self.save_mean)).astype(F32)
            t = (g - _b(k1)).astype(F32)
            t = (t - (xm * _b(q)).astype(F32)).astype(F32)
            self.grad_x = (_b(scale) * t).astype(F32)
            self.grad_rem = g
            if running_mean is not None:
                m = F64(F32(momentum))
                self.running_mean = ((1 - m) * np.asarray(running_mean, F32).astype(F64) + m * mean).astype(F32)
                self.running_var = ((1 - m) * np.asarray(running_var, F32).astype(F64) + m * (var * M / (M - 1.0))).astype(F32)
