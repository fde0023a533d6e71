"""Plain float64 numpy statements of the streaming and fused operations of ganet_amd/csrc/misc_kernels.h, written from the
operations' definitions (libs/GANet/modules/GANet.py:114-148, models/GANet_deep.py:217-277), one short function each with
its adjoint.  Inputs are taken as they are (fp32 arrays are widened, never rounded); nothing here is rounded to fp32.

Trilinear interpolation has no statement here on purpose: ATen computes the source index and the weights in fp32, and a
float64 restatement differs from it by ~1e-5 at 33 -> 100.  Its reference stays F.interpolate on the CPU in fp32."""
import numpy as np

EPS = 1e-12           # F.normalize's default eps: x / max(||x||_1, eps)


def _f64(a):
    return np.asarray(a, np.float64)


# ---- GetCostVolume -----------------------------------------------------------------------------------------------------------
def cost_volume(x, y, Dn):
    """x, y [N,C,H,W] -> [N,2C,Dn,H,W]: cost[n,c,i,h,w] = x[n,c,h,w] | y[n,c-C,h,w-i] for w >= i, else 0"""
    x, y = _f64(x), _f64(y)
    N, C, H, W = x.shape
    cost = np.zeros((N, 2 * C, Dn, H, W))
    for i in range(min(Dn, W)):
        cost[:, :C, i, :, i:] = x[..., i:]
        cost[:, C:, i, :, i:] = y[..., :W - i]
    return cost


def cost_volume_adjoint(g, C):
    """g [N,2C,Dn,H,W] -> (gx, gy) [N,C,H,W]: gx[..w] = sum_{i<=w} g[:C, i, w];  gy[..w] = sum_{i: w+i<W} g[C:, i, w+i]"""
    g = _f64(g)
    N, _, Dn, H, W = g.shape
    gx, gy = np.zeros((N, C, H, W)), np.zeros((N, C, H, W))
    for i in range(min(Dn, W)):
        gx[..., i:] += g[:, :C, i, :, i:]
        gy[..., :W - i] += g[:, C:, i, :, i:]
    return gx, gy


# ---- DisparityRegression -----------------------------------------------------------------------------------------------------
def _disp(Dn):
    return np.arange(Dn, dtype=np.float64).reshape(1, Dn, 1, 1)


def regression(x):
    """x [N,D,H,W] -> [N,H,W]: sum_d d * x[n,d,h,w]"""
    x = _f64(x)
    return (x * _disp(x.shape[1])).sum(1)


def regression_adjoint(gout, Dn):
    return _f64(gout)[:, None] * _disp(Dn)


# ---- F.normalize(p=1) --------------------------------------------------------------------------------------------------------
def sgn(x):
    return np.sign(_f64(x))                               # sgn(0) = 0


def l1_normalize(x, axis):
    x = _f64(x)
    return x / np.maximum(np.abs(x).sum(axis, keepdims=True), EPS)


def l1_clamped(x, axis):
    """where the norm sits below eps (broadcast to x's shape)"""
    x = _f64(x)
    return np.broadcast_to(np.abs(x).sum(axis, keepdims=True) < EPS, x.shape)


def l1_normalize_adjoint(x, gy, axis):
    """y = x / s, s = sum |x|:  gx_t = (gy_t - sgn(x_t) * sum_u gy_u y_u) / s;  gy_t / eps where the norm is clamped (the
    clamp passes no gradient to the norm)"""
    x, gy = _f64(x), _f64(gy)
    s = np.abs(x).sum(axis, keepdims=True)
    clamped = s < EPS
    sden = np.maximum(s, EPS)
    dot = np.where(clamped, 0.0, (gy * (x / sden)).sum(axis, keepdims=True))
    return (gy - sgn(x) * dot) / sden


def norm_regression(x):
    """-> (out, snorm): out = sum_d d * x_d / max(sum_d |x_d|, eps), snorm = that denominator"""
    x = _f64(x)
    snorm = np.maximum(np.abs(x).sum(1), EPS)
    return regression(x) / snorm, snorm


def norm_regression_adjoint(x, gout, sign=None):
    """gx_d = gout * (d - out * sgn(x_d)) / s;  gout * d / eps where the norm is clamped.  sign: used in place of sgn(x) (a
    caller whose x is itself a computed quantity, and who knows where float64 cannot decide its sign for fp32)"""
    x, gout = _f64(x), _f64(gout)
    s = np.abs(x).sum(1)
    out, sden = norm_regression(x)
    ov = np.where(s < EPS, 0.0, out)
    return gout[:, None] * (_disp(x.shape[1]) - ov[:, None] * (sgn(x) if sign is None else _f64(sign))) / sden[:, None]


# ---- Softmin(dim=1) ----------------------------------------------------------------------------------------------------------
def softmin(x):
    x = _f64(x)
    e = np.exp(-(x - x.min(1, keepdims=True)))
    return e / e.sum(1, keepdims=True)


def softmin_adjoint(y, gy):
    """in terms of the OUTPUT y, as the kernel (and autograd's softmax backward) has it: gx = -y * (gy - sum_d gy_d y_d)"""
    y, gy = _f64(y), _f64(gy)
    return -y * (gy - (gy * y).sum(1, keepdims=True))


def softmin_regression(x):
    return regression(softmin(x))


def softmin_regression_adjoint(x, gout):
    """gx_d = -gout * p_d * (d - out), p = softmin(x)"""
    p = softmin(x)
    out = regression(p)
    return -_f64(gout)[:, None] * p * (_disp(p.shape[1]) - out[:, None])


# ---- SGABlock's residual tail ------------------------------------------------------------------------------------------------
def _per_channel(v, C):
    return _f64(v).reshape(1, C, 1, 1, 1)


def residual_relu(t, rem, scale=None, shift=None):
    """t, rem [N,C,D,H,W]: relu(scale[c] * t + shift[c] + rem)  (scale None: relu(t + rem))"""
    t, rem = _f64(t), _f64(rem)
    C = t.shape[1]
    pre = t + rem if scale is None else _per_channel(scale, C) * t + _per_channel(shift, C) + rem
    return np.maximum(pre, 0.0)


def residual_relu_adjoint(y, gy, scale=None):
    """-> (g_t, g_rem): g = gy where y > 0, else 0;  g_rem = g, g_t = scale[c] * g"""
    g = np.where(_f64(y) > 0, _f64(gy), 0.0)
    return (g if scale is None else _per_channel(scale, g.shape[1]) * g), g
