"""A plain float64 numpy statement of SGA, its backward pass as the reference defines it, the true adjoint of its forward,
and a running first-order rounding-error bound for an fp32 evaluation -- written from SURVEY Appendix A.1 / A.2 (not from
the oracle's C).  Layouts: x, out, grad_out [N,C,D,H,W]; guidance of one direction [N,C,5,H,W]; directions 0 = down (rows
0 -> H-1), 1 = up, 2 = right (columns 0 -> W-1), 3 = left.

THE OPERATION.  For fixed (n, c) and orthogonal coordinate, a direction visits the positions p = 0 .. L-1 of its scanline;
w_t[p] (t = 0..4) is the guidance of that pixel, x[p][d] the input:

    A[0][d] = x[0][d] * (w0 + w1 + w2 + w3 + w4)[0]
    A[p][d] = x[p][d] w0[p] + A[p-1][d] w1[p] + T2 w2[p] + T3 w3[p] + A[p-1][k_{p-1}] w4[p]
              T2 = A[p-1][d-1] (d >= 1), T3 = A[p-1][d+1] (d+1 < D); a tap that is not available reads x[p][d]
              k_p = the FIRST arg-max over d of A[p][.]
    out = A_down, mask = 0; then for dir in (up, right, left): if out < A_dir: out = A_dir, mask = dir      (strict <)
    tmp = A_left, kp[dir] = k of every pixel

backward() is A.2: with G = [mask == dir] * grad_out propagated against the scan,

    G[p][d]     += G[p+1][d] w1[p+1] + [d+1 < D] G[p+1][d+1] w2[p+1] + [d >= 1] G[p+1][d-1] w3[p+1]         (p + 1 < L)
    G[p][k_p]   += t,   t = sum_d G[p+1][d] w4[p+1]                                                        (p + 1 < L)
    gradX[p][d]  = G[p][d] w0[p] + [d == 0] G[p][0] w2[p] + [d == D-1] G[p][D-1] w3[p]                     (EVERY p)
    gw0[p] = sum_d G x[p];  for p >= 1: gw_t[p] = sum_d G[p][d] * (tap t of the forward);  gw1..gw4[0] = 0

summed over the four directions for gradX.  true_backward() is the adjoint of forward() with the selections (k, mask) held
fixed.  It differs at the FIRST scan position of each direction only, where all five taps read x[0][d]:

    gradX[0][d] = G[0][d] (w0 + w1 + w2 + w3 + w4)[0],      gw_t[0] = sum_d G[0][d] x[0][d]   for every t

(the reference leaves these terms out: SURVEY F4).

THE ERROR BOUND.  u = 2^-24 is the unit roundoff of fp32.  A rounded operation returns its exact result times (1 + e), |e| <= u;
to first order in u the error of a computed quantity is what its inputs' errors contribute through the exact formula plus u
times the magnitude of every intermediate that is rounded.  A sum of n rounded products, in any order, has n product roundings
and n-1 additions whose partial sums are bounded by the sum of the |terms|: at most n u sum|terms|.  Second-order terms
(error times error, u^2) are dropped; whoever compares with the bound allows a factor 2 for them.

  forward   five products and five additions per step (an fma build performs fewer), counted as 10 roundings of at most the
            sum of the |terms|; x and w are exact fp32 inputs, and with equal selections tap t carries the previous
            position's error:
                E_A[p][d] = sum_t |w_t| E_A(tap t) + 10 u sum_t |w_t P_t|,       E_A(x) = 0
            E_out is E_A of the winning direction.
  adjoint   G[p][d] is a sum of at most five terms -- grad_out (exact), three products, and t at d = k_p -- and t a sum of D
            products:
                E_t       = sum_d |w4| E_G[p+1][d] + D u sum_d |G[p+1][d] w4|
                E_G[p][d] = |w1| E_G[p+1][d] + |w2| E_G[p+1][d+1] + |w3| E_G[p+1][d-1] + [d == k_p] E_t
                            + 5 u (|grad_out| + |three products| + [d == k_p] sum_d |G[p+1][d] w4|)
  gradX     a sum of at most 12 products (three per direction):  E = sum_terms |w| E_G + 12 u sum_terms |G w|
  gw_t[p]   a sum of D products G V with V = x (exact) or a forward tap (E_V = E_A of that tap):
                E = sum_d (E_G |V| + |G| E_V) + D u sum_d |G V|

Every bound is computed from the float64 values beside them, per output element, from the inputs alone."""
import numpy as np

U = 2.0 ** -24
DIRS = (0, 1, 2, 3)
DROPS = ("gx_last", "w4_routing", "last_argmax")      # private switches of backward(): see mutated()


def _to_scan(v, direction):
    """[N,C,K,H,W] -> [L,N,C,O,K]: scan position first (in scan order), the K axis (depth or tap) last"""
    t = v.transpose(3, 0, 1, 4, 2) if direction < 2 else v.transpose(4, 0, 1, 3, 2)
    return t[::-1] if direction in (1, 3) else t


def _from_scan(t, direction):
    t = t[::-1] if direction in (1, 3) else t
    return np.ascontiguousarray(t.transpose(1, 2, 4, 0, 3) if direction < 2 else t.transpose(1, 2, 4, 3, 0))


def _shift_up(a, fill):
    """element d <- a[d-1]; d = 0 <- fill"""
    return np.concatenate([fill, a[..., :-1]], -1)


def _shift_down(a, fill):
    """element d <- a[d+1]; d = D-1 <- fill"""
    return np.concatenate([a[..., 1:], fill], -1)


def _taps(x, a, e, k):
    """the five taps of one step and their error bounds: x [.., D] of this position; a, e, k of the previous one"""
    zero = np.zeros_like(x[..., :1])
    best = np.broadcast_to(np.take_along_axis(a, k, -1), x.shape)
    ebest = np.broadcast_to(np.take_along_axis(e, k, -1), x.shape)
    return ([x, a, _shift_up(a, x[..., :1]), _shift_down(a, x[..., -1:]), best],
            [np.zeros_like(x), e, _shift_up(e, zero), _shift_down(e, zero), ebest])


def _scan(xs, ws, ks=None):
    """xs [L,..,D], ws [L,..,5] (scan layout) -> A, E_A [L,..,D], k [L,..,1]; ks: selections to use instead of the arg-max"""
    L = xs.shape[0]
    A, E = np.empty_like(xs), np.empty_like(xs)
    K = np.empty(xs.shape[:-1] + (1,), np.int64)
    for p in range(L):
        w = [ws[p][..., t:t + 1] for t in range(5)]
        if p == 0:
            taps, errs = [xs[0]] * 5, [np.zeros_like(xs[0])] * 5
        else:
            taps, errs = _taps(xs[p], A[p - 1], E[p - 1], K[p - 1])
        acc, mag, err = 0.0, 0.0, 0.0
        for t in range(5):
            acc = acc + taps[t] * w[t]
            mag = mag + np.abs(taps[t] * w[t])
            err = err + np.abs(w[t]) * errs[t]
        A[p], E[p] = acc, err + 10 * U * mag
        K[p] = np.argmax(A[p], -1)[..., None] if ks is None else ks[p]
    return A, E, K


def _f64(a):
    return np.asarray(a, np.float64)


def scan(x, g, direction):
    """A_dir of one direction (A.1)"""
    return _from_scan(_scan(_to_scan(_f64(x), direction), _to_scan(_f64(g), direction))[0], direction)


def forward(x, g0, g1, g2, g3, kp=None, mask=None):
    """-> dict: A0..A3, out, mask (uint8), tmp (= A_left), kp [4,N,C,H,W] (first arg-max over d), and the bounds E_A0..E_A3,
    E_out.  kp / mask given: the selections are taken from there (inputs with exact ties, where fp32 decides them)."""
    x = _f64(x)
    r = {}
    kps = []
    for d, g in enumerate((g0, g1, g2, g3)):
        ks = None if kp is None else _to_scan(np.asarray(kp[d], np.int64)[:, :, None], d)
        A, E, K = _scan(_to_scan(x, d), _to_scan(_f64(g), d), ks)
        r[f"A{d}"], r[f"E_A{d}"] = _from_scan(A, d), _from_scan(E, d)
        kps.append(_from_scan(K, d)[:, :, 0])
    r["kp"] = np.stack(kps)
    if mask is None:
        out, m = r["A0"].copy(), np.zeros(x.shape, np.uint8)
        for d in (1, 2, 3):
            less = out < r[f"A{d}"]
            out[less], m[less] = r[f"A{d}"][less], d
    else:
        m = np.asarray(mask).astype(np.uint8)
        out = np.choose(m, [r[f"A{d}"] for d in DIRS])
    r["out"], r["mask"], r["tmp"] = out, m, r["A3"]
    r["E_out"] = np.choose(m, [r[f"E_A{d}"] for d in DIRS])
    return r


def _backward(x, gs, go, fwd, first_position, drop):
    assert drop is None or drop in DROPS
    x, go = _f64(x), _f64(go)
    N, C, D, H, W = x.shape
    r = {"gx": 0.0}
    e_gx, m_gx = 0.0, 0.0
    depth = np.arange(D)
    for d in DIRS:
        xs, ws = _to_scan(x, d), _to_scan(_f64(gs[d]), d)
        As, Es = _to_scan(fwd[f"A{d}"], d), _to_scan(fwd[f"E_A{d}"], d)
        ks = _to_scan(fwd["kp"][d][:, :, None], d)
        if drop == "last_argmax":
            ks = D - 1 - np.argmax(As[..., ::-1], -1)[..., None]
        L = xs.shape[0]
        w = [ws[..., t:t + 1] for t in range(5)]
        G = _to_scan(np.where(fwd["mask"] == d, go, 0.0), d).copy()
        EG = np.zeros_like(G)
        zero = np.zeros_like(G[0][..., :1])
        for p in range(L - 2, -1, -1):
            gn, en = G[p + 1], EG[p + 1]
            w1, w2, w3, w4 = (w[t][p + 1] for t in (1, 2, 3, 4))
            t1, t2, t3 = gn * w1, _shift_down(gn, zero) * w2, _shift_up(gn, zero) * w3
            at_k = depth == ks[p]
            tt, tmag = (gn * w4).sum(-1, keepdims=True), np.abs(gn * w4).sum(-1, keepdims=True)
            et = (np.abs(w4) * en).sum(-1, keepdims=True) + D * U * tmag
            if drop == "w4_routing":
                tt = tt * 0.0
            mag = np.abs(G[p]) + np.abs(t1) + np.abs(t2) + np.abs(t3) + at_k * tmag
            EG[p] = (np.abs(w1) * en + np.abs(w2) * _shift_down(en, zero) + np.abs(w3) * _shift_up(en, zero)
                     + at_k * et + 5 * U * mag)
            G[p] = G[p] + t1 + t2 + t3 + at_k * tt
        # gradX of this direction: G w0, and what the unavailable depth taps (they read x[p][d]) hand back
        first, last = depth == 0, depth == D - 1
        if drop == "gx_last":
            last = last & False
        terms = [(G, EG, w[0]), (G * first, EG * first, w[2]), (G * last, EG * last, w[3])]
        gx = sum(g * wt for g, _, wt in terms)
        if first_position:
            gx[0] = G[0] * (w[0][0] + w[1][0] + w[2][0] + w[3][0] + w[4][0])
        e_gx = e_gx + _from_scan(sum(e * np.abs(wt) for _, e, wt in terms), d)
        m_gx = m_gx + _from_scan(sum(np.abs(g * wt) for g, _, wt in terms), d)
        r[f"gx_dir{d}"] = _from_scan(gx, d)
        r["gx"] = r["gx"] + r[f"gx_dir{d}"]
        # guidance gradients: tap t of position p >= 1 as the forward read it
        gw, egw = np.zeros_like(ws), np.zeros_like(ws)
        gw[..., 0] = (G * xs).sum(-1)
        egw[..., 0] = (EG * np.abs(xs)).sum(-1) + D * U * np.abs(G * xs).sum(-1)
        for p in range(1, L):
            taps, errs = _taps(xs[p], As[p - 1], Es[p - 1], ks[p - 1])
            for t in range(1, 5):
                gw[p][..., t] = (G[p] * taps[t]).sum(-1)
                egw[p][..., t] = ((EG[p] * np.abs(taps[t]) + np.abs(G[p]) * errs[t]).sum(-1)
                                  + D * U * np.abs(G[p] * taps[t]).sum(-1))
        if first_position:
            gw[0][..., 1:] = gw[0][..., :1]
        r[f"G{d}"], r[f"E_G{d}"] = _from_scan(G, d), _from_scan(EG, d)
        r[f"gw{d}"], r[f"E_gw{d}"] = _from_scan(gw, d), _from_scan(egw, d)
    r["E_gx"] = e_gx + 12 * U * m_gx
    return r


def backward(x, gs, go, fwd, _drop=None):
    """A.2 on the selections of `fwd` (a forward() result) -> dict: the adjoint volumes G0..G3 (API layout), gx, gw0..gw3,
    gx_dir0..3 (each direction's share of gx), and the bounds E_G*, E_gx, E_gw*."""
    return _backward(x, gs, go, fwd, False, _drop)


def true_backward(x, gs, go, fwd):
    """the exact adjoint of forward() with the selections of `fwd` held fixed (same keys as backward(); the bounds are those
    of backward() and do not apply)"""
    return _backward(x, gs, go, fwd, True, None)


def mutated(x, gs, go, fwd, drop):
    """backward() with one term wrong, for the tests that show that a comparison notices:  "gx_last" -- gradX lacks the
    d == D-1 boundary term;  "w4_routing" -- t is not routed to k_p;  "last_argmax" -- k_p is the LAST arg-max."""
    return _backward(x, gs, go, fwd, False, drop)


def _top_two_gap(v, axis):
    if v.shape[axis] < 2:
        return np.full(np.delete(v.shape, axis), np.inf)
    s = np.sort(v, axis)
    return np.take(s, -1, axis) - np.take(s, -2, axis)


def selection_gaps(fwd):
    """(smallest gap between the two largest entries over d of any pixel and direction, smallest gap between the two largest
    directions of any element)"""
    return (min(float(_top_two_gap(fwd[f"A{d}"], 2).min()) for d in DIRS),
            float(_top_two_gap(np.stack([fwd[f"A{d}"] for d in DIRS]), 0).min()))


def unstable(fwd):
    """Number of selections that an fp32 evaluation within the bounds could make differently: pixels (per direction) whose
    two largest entries over d are not more than 2 max_d E_A apart, plus elements where some direction comes within the sum
    of the two bounds of the winning one.  0: fp32 and float64 select alike, everywhere."""
    n = 0
    for d in DIRS:
        n += int((_top_two_gap(fwd[f"A{d}"], 2) <= 2 * fwd[f"E_A{d}"].max(2)).sum())
    for d in DIRS:
        lost = fwd["mask"] != d
        n += int((lost & (fwd["out"] - fwd[f"A{d}"] <= fwd["E_out"] + fwd[f"E_A{d}"])).sum())
    return n


def stable(fwd):
    return unstable(fwd) == 0
