"""A plain float64 numpy statement of LGA and its adjoints, written from the operation's definition (not from the oracle's C):

    y[b, d, i, j] = sum over taps (dd, a, b') of f[b, t, i, j] * x[b, d+dd, i+a, j+b']
                    dd in {-1, 0, 1}, a, b' in [-r, r], t = (dd+1) * K + (a+r) * (2r+1) + (b'+r), K = (2r+1)^2,

where a tap whose index leaves the volume in depth, row or column reads the CENTRE value x[b, d, i, j] instead.
4-D [B,D,H,W] with filters [B,3K,H,W], or 5-D [N,C,D,H,W] with filters [N,C,3K,H,W] (N*C folded)."""
import numpy as np


def _fold(x, f):
    H, W = x.shape[-2:]
    return x.reshape(-1, x.shape[-3], H, W).astype(np.float64), f.reshape(-1, f.shape[-3], H, W).astype(np.float64)


def _taps(r, D, H, W):
    """(tap index, dd, a, b, slices of the positions whose tap stays inside, slices of what they read)"""
    ws = 2 * r + 1
    for dd in (-1, 0, 1):
        for a in range(-r, r + 1):
            for b in range(-r, r + 1):
                t = (dd + 1) * ws * ws + (a + r) * ws + (b + r)
                dst, src = [], []
                for off, n in ((dd, D), (a, H), (b, W)):
                    lo, hi = max(0, -off), min(n, n - off)
                    hi = max(hi, lo)
                    dst.append(slice(lo, hi))
                    src.append(slice(lo + off, hi + off))
                yield t, tuple(dst), tuple(src)


MUTATIONS = ("drop_tap", "zero_pad")                    # private switches of lga_forward / lga_backward: see mutated_chain()


def _dropped(t, r, _mut):
    """"drop_tap" leaves out the tap (dd, a, b') = (0, 0, +1): the centre plane's right-hand neighbour"""
    ws = 2 * r + 1
    return _mut == "drop_tap" and t == ws * ws + r * ws + r + 1


def lga_forward(x, f, r, _mut=None):
    assert _mut is None or _mut in MUTATIONS
    xs, fs = _fold(x, f)
    B, D, H, W = xs.shape
    y = np.zeros_like(xs)
    for t, dst, src in _taps(r, D, H, W):
        if _dropped(t, r, _mut):
            continue
        v = np.zeros_like(xs) if _mut == "zero_pad" else xs.copy()      # outside: the centre value
        v[(slice(None),) + dst] = xs[(slice(None),) + src]
        y += fs[:, t][:, None] * v
    return y.reshape(x.shape)


def lga_backward(x, f, gy, r, _mut=None):
    """-> (gx, gf): the adjoints of lga_forward in x and in f"""
    assert _mut is None or _mut in MUTATIONS
    xs, fs = _fold(x, f)
    gs = gy.reshape(xs.shape).astype(np.float64)
    B, D, H, W = xs.shape
    gx, gf = np.zeros_like(xs), np.zeros_like(fs)
    for t, dst, src in _taps(r, D, H, W):
        if _dropped(t, r, _mut):
            continue
        v = np.zeros_like(xs) if _mut == "zero_pad" else xs.copy()
        v[(slice(None),) + dst] = xs[(slice(None),) + src]
        gf[:, t] = (gs * v).sum(1)
        c = fs[:, t][:, None] * gs                        # what each output position hands to the element it read
        if _mut != "zero_pad":
            inside = np.zeros((D, H, W), bool)
            inside[dst] = True
            gx += np.where(inside, 0.0, c)                # ... the centre, where the tap left the volume
        gx[(slice(None),) + src] += c[(slice(None),) + dst]
    return gx.reshape(x.shape), gf.reshape(f.shape)


def lga_chain(x, f, gy, r, passes, _mut=None):
    """`passes` chained passes with one filter tensor and their backward: -> dict(y, gx, gf, ins=[input of each pass])"""
    ins = [np.asarray(x, np.float64)]
    for _ in range(passes):
        ins.append(lga_forward(ins[-1], f, r, _mut))
    g, gf = np.asarray(gy, np.float64), 0.0
    for xin in reversed(ins[:-1]):
        g, gfk = lga_backward(xin, f, g, r, _mut)
        gf = gf + gfk
    return {"y": ins[-1], "gx": g, "gf": gf, "ins": ins[:-1]}


def mutated_chain(x, f, gy, r, passes, what):
    """lga_chain with one thing wrong, for the tests that show that a comparison notices:  "drop_tap" -- every pass and its
    adjoints lack one of the 3(2r+1)^2 taps;  "zero_pad" -- a tap that leaves the volume reads 0 instead of the centre value."""
    assert what in MUTATIONS
    return lga_chain(x, f, gy, r, passes, what)


U = 2.0 ** -24


def _gamma(n):
    return n * U / (1.0 - n * U)


def chain_bound(x, f, gy, r, passes, backward=True):
    """A first-order rounding-error bound, per element, for an fp32 evaluation of lga_chain: -> dict(y, gx, gf) of bounds, and
    `want`, the float64 chain they belong to.  Whoever compares allows a factor 2 for the second-order terms, as with SGA.
    backward=False (a call that got no gradient): the forward chain and the bound of y alone -- the same y and the same bound,
    without the adjoint passes, which are most of the cost.

    u = 2^-24.  A sum of n rounded products, accumulated in any order (fused or not, split over lanes or not), differs from
    the exact sum of the same terms by at most gamma_n sum|terms|, gamma_n = n u / (1 - n u) (every term passes through at
    most n roundings: its product and at most n - 1 additions).  To first order the error of a computed quantity is what its
    inputs' errors contribute through the exact (linear) formula, plus that.  x, f and gy are exact fp32 inputs.

      forward   x_0 = x, x_{k+1}[p] = sum_t f_t[p] v_t(x_k)[p], T = 3(2r+1)^2 terms (v_t: the tap, or the centre value):
                    E_0 = 0,   E_{k+1} = sum_t |f_t| v_t(E_k) + gamma_T sum_t |f_t| |v_t(x_k)|
                -- the previous pass's bound pushed through |f|, plus gamma_T times the absolute-value sum of the element's
                own accumulation.  Both are lga_forward on absolute values.
      data      g_P = gy, g_k = adjoint of pass k applied to g_{k+1}.  An element q receives one term f_t[q-o] g[q-o] from
      adjoint   every tap whose reader q - o lies inside the volume, and one term f_t[q] g[q] from every tap of its OWN pixel
                that leaves the volume at q + o; the tap set is symmetric (o <-> -o), so these are T terms altogether:
                    G_P = 0,   G_k = adj(|f|, G_{k+1}) + gamma_T adj(|f|, |g_{k+1}|)
                (a kernel that first sums the out-of-range filters of a pixel and multiplies once stays inside: T - 1 roundings).
      filter    gf_t[p] = sum_k sum_d g_{k+1}[d,p] v_t(x_k)[d,p]: per pass D products, and the passes' results added up --
      gradient  n = D + passes roundings at most on any term's way; both factors carry their own bounds:
                    E = sum_k sum_d (G_{k+1} |v_t(x_k)| + |g_{k+1}| v_t(E_k)) + gamma_n sum_k sum_d |g_{k+1} v_t(x_k)|
                Each of the three sums is the filter gradient of lga_backward on absolute values.

    Everything is computed from the float64 chain beside it, from the inputs alone."""
    fa = np.abs(np.asarray(f, np.float64))
    T, D = f.shape[-3], x.shape[-3]
    if backward:
        want = lga_chain(x, f, gy, r, passes)
    else:
        ins = [np.asarray(x, np.float64)]
        for _ in range(passes):
            ins.append(lga_forward(ins[-1], f, r))
        want = {"y": ins[-1], "ins": ins[:-1]}
    gT, gN = _gamma(T), _gamma(D + passes)
    E = [np.zeros(x.shape)]
    for k in range(passes):
        # (E_0 = 0 pushes nothing through: the pass over it is skipped, its result is 0 exactly)
        E.append((lga_forward(E[k], fa, r) if k else 0.0) + gT * lga_forward(np.abs(want["ins"][k]), fa, r))
    if not backward:
        return {"y": E[passes], "want": want}
    g, G, egf = np.asarray(gy, np.float64), np.zeros(x.shape), 0.0
    for k in reversed(range(passes)):
        xk = np.abs(want["ins"][k])
        own = lga_backward(xk, fa, np.abs(g), r)
        through = lga_backward(xk, fa, G, r) if k < passes - 1 else (0.0, 0.0)      # (G_P = 0, E_0 = 0: exact zeros, skipped)
        egf = egf + through[1] + (lga_backward(E[k], fa, np.abs(g), r)[1] if k else 0.0) + gN * own[1]
        G = through[0] + gT * own[0]
        g = lga_backward(want["ins"][k], f, g, r)[0]
    return {"y": E[passes], "gx": G, "gf": egf, "want": want}


def assert_lga_exact_by_norms(x, f, gy, r, passes):
    """The same condition from norms alone, for volumes too large to push through the float64 chain: a forward pass
    multiplies max|.| by at most F = max over pixels of sum_t |f_t|; a data-backward pass by at most S = 2 T max|f| (an
    element is read through at most T taps of its neighbours, one each, and through at most T out-of-range taps of its
    own pixel); a filter gradient is a sum over D products of an input and a gradient of its pass.  Grids: 1/8 per filter
    factor (y, gx: `passes` factors; each term of gf: `passes` - 1)."""
    for v in (x, gy, 8 * f):
        assert np.array_equal(v, np.round(v))
    T, D = f.shape[-3], x.shape[-3]
    F = float(np.abs(f).sum(-3).max())
    S = 2.0 * T * float(np.abs(f).max())
    mx, mg = float(np.abs(x).max()), float(np.abs(gy).max())
    ins = [mx * F ** k for k in range(passes)]                   # max|input of pass k|
    gs = [mg * S ** k for k in range(passes)]                    # max|gradient of the output of pass (passes-1-k)|
    bounds = {"y": mx * F ** passes * 8.0 ** passes, "gx": mg * S ** passes * 8.0 ** passes,
              "gf": sum(D * ins[passes - 1 - k] * gs[k] for k in range(passes)) * 8.0 ** (passes - 1)}
    assert max(bounds.values()) < 2 ** 24, bounds
    return bounds


def assert_lga_exact(x, f, gy, r, passes):
    """Exactness condition of the exact LGA family: the float64 chain on the ABSOLUTE values of the inputs bounds every
    partial sum of every result in any order; in units of the result's grid (filters are multiples of 1/8: 1/8 per filter
    factor -- y and gx carry `passes` factors, gf up to `passes` - 1 and the data) it must stay below 2^24, the range
    in which fp32 holds every multiple of the grid exactly.  -> the float64 results on the real inputs."""
    for v in (x, gy, 8 * f):
        assert np.array_equal(v, np.round(v))
    bound = lga_chain(np.abs(x), np.abs(f), np.abs(gy), r, passes)
    grid = 8.0 ** passes
    for k in ("y", "gx", "gf"):
        assert np.abs(bound[k]).max() * grid < 2 ** 24, (k, float(np.abs(bound[k]).max()), grid)
    for v in bound["ins"]:
        assert np.abs(v).max() * grid < 2 ** 24
    want = lga_chain(x, f, gy, r, passes)
    for k in ("y", "gx", "gf"):
        assert np.array_equal(want[k], want[k].astype(np.float32).astype(np.float64)), k     # representable in fp32 at all
    return want
