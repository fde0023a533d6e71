"""TEST INFRASTRUCTURE: the float64 statement of DispTail (ganet_up_softmin_regression_forward / _backward,
ganet_amd/csrc/disp_tail_kernels.h), its first-order rounding bounds, and a float32 model of the kernels' arithmetic.

THE STATEMENT.  x [N, Di, Hi, Wi] holds the fp32 values the kernels read.  Per axis, (i0, i1, l) are up_src's
(ganet_amd/csrc/misc_kernels.h) restated in numpy float32 -- PyTorch's align_corners=False rule, and the float32 evaluation is
part of the definition: scale = (float)in / out, src = max(scale * (o + 0.5) - 0.5, 0), i0 = min(int(src), in - 1),
i1 = min(i0 + 1, in - 1), l = src - i0.  Everything behind that is float64:
  a(d,h,.) = (1-lw) x[d,h,w0] + lw x[d,h,w1];  c[d] = (1-lh) a(d,h0) + lh a(d,h1);  v[od] = (1-ld) c[d0] + ld c[d1]
  m = max_od(-v), s = sum e^(-v-m), out = sum od e^(-v-m) / s, p_od = e^(-v_od-m) / s
  gv[od] = -gout p_od (od - out);  gc[id] = sum_od w_d(od,id) gv[od];  gx[id,ih,iw] = sum_(oh,ow) w_h w_w gc[id,oh,ow]

THE BOUNDS (u = 2^-24; first order in u; per element; the bar of tests/disp_tail_cases.py is twice the bound).
  v   Each of the three blends rounds 1-l, two products and one sum: 3u of |1-l||p| + l|q|, and passes its inputs' errors on
      with weights that sum to one: 9u A, A = the same interpolation of |x|.  A contraction to fused multiply-adds only removes
      roundings.  l ITSELF: `scale * (o + 0.5) - 0.5` may or may not be contracted by either build, which moves src -- and l,
      since src - i0 is exact -- by up to one ulp of the product, dl = spacing(src + 0.5) (2^-18 at od ~ 190), times the
      slope |q - p| of the blend.  Where src sits within dl of an integer the two evaluations may even choose neighbouring
      (i0, i1) with l ~ 1 resp. ~ 0: the value is continuous there and moves by dl times the slope of one of the two
      segments, so the slope taken is the largest of the segment's and its two neighbours'.  The W and H terms pass through
      the blends behind them:   ev = 9u A + W_d W_h (dl_w slope_w) + W_d (dl_h slope_h) + dl_d slope_d.
  e   e_od = e^(-v_od - m) as the kernel forms it: the error of v (absolute in the exponent = relative in e); the rounding of
      the exponents, which along the chain of chunk maxima telescope to u |-v_od - m|; one expf (within 1 ulp = 2u), and per
      LATER chunk one more expf and one product for the rescale: eta_od = ev_od + u (|-v_od - m| + 2 + 3 (K - 1 - od // 8)),
      K = ceil(Do / 8).
  out = t / s.  A relative error common to all e cancels; what is left is sum p |od - out| eta.  The two running sums round
      once per term (t by fmaf): u times the sum of their partial sums, S_run and T_run (data dependent: far below the
      worst case (Do - 1) s when the mass sits late), and the division once:
      b_out = sum p |od - out| eta + u (T_run + out S_run) / s + u out.
      (At Do = 193 on unit-normal x the two running-sum terms are about three quarters of b_out: a worst-case statement about 193
      roundings that all point the same way.  Measured errors sit at a few hundredths of the bar there; the wrong
      definitions of the calibration still exceed it by factors of 400 to 40000.)
  mx  |max a - max b| <= max |a - b|: b_mx = max_od ev.    ssum  b_ss = sum E eta + u S_run + s b_mx (it is relative to m).
  gv  p_od is recomputed as expf(-v - m) / ssum from the SAVED m and ssum (m cancels): relative error
      rho_od = ev_od + u (|-v_od - m| + 2) + (sum E eta + u S_run) / s;  gout / ssum, two products and od - out round once
      each, and out carries b_out:   b_gv = |gout| p_od (|od - out| (rho_od + 5u) + b_out).
  gc  = sum_od w_d gv: the errors of gv with their weights; dl_d |gv| onto every plane from i0 - 1 to i1 + 1 (a weight that
      moves, see v); 1-l, and one rounding per accumulated term and for the final g0 + g1: (3 + n_id) u sum w_d |gv|, n_id the
      number of od that read plane id.
  gx  = sum w_h w_w gc (trilinear_up_bwd on depth 1 -> 1, whose depth weight is exactly 1): the same three kinds of term on
      the two remaining axes, (n_ih + n_iw + 6) u for the weights' own roundings and the two fmaf chains.
`Float32Model` is the kernels' arithmetic operation by operation in numpy float32 -- the chunks of 8, the running-max rescale,
fmaf where the kernels have one -- in both variants of l; tests/test_sim_disp_tail.py checks that it stays inside HALF of every
bar: the bars come from the arithmetic, not from what the kernels return.  The same file checks that the comparison
discriminates: `mutant()` restates five wrong definitions, and each must exceed the bar."""
import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
CHUNK = 8                      # disp_tail_kernels.h: od marches in chunks of 8


class Axis:
    """(i0, i1, lam) of up_src for every output index, in float32.  variant: "plain" (product and difference rounded
    separately), "fma" (one rounding), "align_corners" (the other rule: a wrong definition, for the calibration)"""

    def __init__(self, n_in, n_out, variant="plain"):
        self.n_in, self.n_out = n_in, n_out
        o = np.arange(n_out)
        of = o.astype(F32) + F32(0.5)
        scale = F32(n_in) / F32(n_out)
        if variant == "plain":
            src = (scale * of).astype(F32) - F32(0.5)
        elif variant == "fma":
            src = (F64(scale) * of.astype(F64) - 0.5).astype(F32)
        else:
            assert variant == "align_corners"
            src = (o * (F64(n_in - 1) / F64(n_out - 1) if n_out > 1 else 0.0)).astype(F32)
        src = np.where(src < 0, F32(0), src).astype(F32)
        self.src = src
        i0 = np.minimum(src.astype(np.int64), n_in - 1)
        self.i0, self.i1 = i0, i0 + (i0 < n_in - 1)
        self.lam = np.clip((src - i0.astype(F32)).astype(F32), F32(0), F32(1))
        self.dlam = np.spacing(src + F32(0.5)).astype(F64)
        self.lam64 = self.lam.astype(F64)

    def up(self, arr, axis, lam=None):
        """interpolate along `axis` (input extent -> output extent)"""
        lam = self.lam64 if lam is None else lam
        arr = np.moveaxis(arr, axis, -1)
        return np.moveaxis((1.0 - lam) * arr[..., self.i0] + lam * arr[..., self.i1], -1, axis)

    def _scatter(self, arr, pairs):
        """sum over (idx, w) of: out[..., idx[o]] += w[o] * arr[..., o]"""
        out = np.zeros(arr.shape[:-1] + (self.n_in,))
        for idx, w in pairs:
            np.add.at(out, (Ellipsis, idx), arr * w)
        return out

    def down(self, arr, axis, lam=None):
        """the adjoint of up (output extent -> input extent)"""
        lam = self.lam64 if lam is None else lam
        arr = np.moveaxis(arr, axis, -1)
        return np.moveaxis(self._scatter(arr, [(self.i0, 1.0 - lam), (self.i1, lam)]), -1, axis)

    def down_moved(self, arr, axis):
        """dlam * arr onto every input from i0 - 1 to i1 + 1 (where a weight may move to), each once"""
        arr = np.moveaxis(arr, axis, -1)
        lo, hi = np.maximum(self.i0 - 1, 0), np.minimum(self.i1 + 1, self.n_in - 1)
        pairs = [(lo, self.dlam), (self.i0, self.dlam * (self.i0 != lo)), (self.i1, self.dlam * (self.i1 != self.i0)),
                 (hi, self.dlam * (hi != self.i1))]
        return np.moveaxis(self._scatter(arr, pairs), -1, axis)

    def reader_lists(self):
        """per input: the outputs that read it with a non-zero weight, ascending"""
        lists = [[] for _ in range(self.n_in)]
        for o in range(self.n_out):
            if self.i1[o] == self.i0[o] or self.lam[o] != 1:
                lists[self.i0[o]].append(o)
            if self.i1[o] != self.i0[o] and self.lam[o] != 0:
                lists[self.i1[o]].append(o)
        return lists

    def readers(self):
        """[in]: how many outputs read each input (at least 1)"""
        return np.maximum(np.array([len(q) for q in self.reader_lists()]), 1)

    def unread(self):
        """[in] bool: inputs that no output reads"""
        return np.array([len(q) == 0 for q in self.reader_lists()])

    def slope_term(self, arr, axis):
        """arr has the INPUT extent along `axis`; -> the output extent: dlam[o] * the largest |arr[k+1] - arr[k]| over the
        segments k = i0 - 1, i0, i0 + 1"""
        arr = np.moveaxis(arr, axis, -1)
        D = np.abs(np.diff(arr, axis=-1))
        Dp = np.concatenate([np.zeros(arr.shape[:-1] + (1,)), D, np.zeros(arr.shape[:-1] + (2,))], axis=-1)
        s = np.maximum(np.maximum(Dp[..., self.i0], Dp[..., self.i0 + 1]), Dp[..., self.i0 + 2]) * self.dlam
        return np.moveaxis(s, -1, axis)


class Statement:
    def __init__(self, x, size, gout, variant="plain", mutation=None):
        x = np.asarray(x, F32)
        assert x.ndim == 4 and np.asarray(gout).dtype == F32
        N, Di, Hi, Wi = x.shape
        Do, Ho, Wo = size
        var = "align_corners" if mutation == "align_corners" else variant
        ad, ah, aw = Axis(Di, Do, var), Axis(Hi, Ho, var), Axis(Wi, Wo, var)
        self.ad, self.ah, self.aw = ad, ah, aw
        ld = 1.0 - ad.lam64 if mutation == "swap_lambda_d" else ad.lam64
        x64, g = x.astype(F64), np.asarray(gout).astype(F64)
        a = aw.up(x64, 3)
        c = ah.up(a, 2)
        v = ad.up(c, 1, ld)
        od = (np.arange(Do, dtype=F64) + (1.0 if mutation == "od_plus_1" else 0.0))[None, :, None, None]
        nv = -v
        m = nv.max(1)
        E = np.exp(nv - m[:, None])
        s = E.sum(1)
        out = (od * E).sum(1) / s
        p = E / s[:, None]
        dev_ = od - (0.0 if mutation == "gv_no_out" else out[:, None])
        gv = -g[:, None] * p * dev_
        gc = ad.down(gv, 1, ld)
        if mutation == "gc_skipped_unwritten":
            # what a column pass that writes only the planes it visits leaves behind a poisoned workspace
            gc = np.where(ad.unread()[None, :, None, None], np.nan, gc)
        gx = aw.down(ah.down(gc, 2), 3)
        self.v, self.mx, self.ssum, self.out, self.gv, self.gc, self.grad_x = v, m, s, out, gv, gc, gx
        if mutation is not None:
            return
        # ---- the bounds ----
        A = ad.up(ah.up(aw.up(np.abs(x64), 3), 2), 1)
        ev = 9 * U * A + ad.up(ah.up(aw.slope_term(x64, 3), 2), 1) + ad.up(ah.slope_term(a, 2), 1) + ad.slope_term(c, 1)
        K = -(-Do // CHUNK)
        later = (K - 1 - np.arange(Do) // CHUNK)[None, :, None, None]
        expo = np.abs(nv - m[:, None])
        eta = ev + U * (expo + 2 + 3 * later)
        S_run = np.cumsum(E, 1).sum(1)
        T_run = np.cumsum(od * E, 1).sum(1)
        self.ev = ev
        self.b_out = (p * np.abs(od - out[:, None]) * eta).sum(1) + U * (T_run + out * S_run) / s + U * out
        self.b_mx = ev.max(1)
        s_rel = ((E * eta).sum(1) + U * S_run) / s
        self.b_ssum = s * (s_rel + self.b_mx)
        rho = ev + U * (expo + 2) + s_rel[:, None]
        b_gv = np.abs(g)[:, None] * p * (np.abs(od - out[:, None]) * (rho + 5 * U) + self.b_out[:, None])
        nd = ad.readers()[None, :, None, None]
        agv = np.abs(gv)
        self.b_gc = ad.down(b_gv, 1) + ad.down_moved(agv, 1) + (3 + nd) * U * ad.down(agv, 1)
        agc = np.abs(gc)
        nh, nw = ah.readers()[None, None, :, None], aw.readers()[None, None, None, :]
        self.b_grad_x = (aw.down(ah.down(self.b_gc, 2), 3) + aw.down(ah.down_moved(agc, 2), 3) + aw.down_moved(ah.down(agc, 2), 3)
                         + (nh + nw + 6) * U * aw.down(ah.down(agc, 2), 3))

    def results(self):
        return {"out": self.out, "mx": self.mx, "ssum": self.ssum, "gc": self.gc, "grad_x": self.grad_x}

    def bounds(self):
        return {"out": self.b_out, "mx": self.b_mx, "ssum": self.b_ssum, "gc": self.b_gc, "grad_x": self.b_grad_x}


MUTATIONS = ("align_corners", "swap_lambda_d", "od_plus_1", "gv_no_out", "gc_skipped_unwritten")


def mutant(x, size, gout, mutation):
    """the results of a WRONG definition, as fp32 arrays"""
    assert mutation in MUTATIONS
    return {k: v.astype(F32) for k, v in Statement(x, size, gout, mutation=mutation).results().items()}


def _fma32(a, b, c):
    """fmaf on fp32 arrays: the product of two fp32 values is exact in float64; the sum is rounded to 53 bits and then to 24
    (double rounding differs from fmaf by one ulp in about 1 case in 2^29: the half-of-the-bar check absorbs it)"""
    return (np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64) + np.asarray(c, F32).astype(F64)).astype(F32)


def _weight32(ax, o, i):
    """up_weight: (i0 == i ? 1 - l : 0) + (i1 == i ? l : 0) in float32, for arrays o, i"""
    l = ax.lam[o]
    return (np.where(ax.i0[o] == i, F32(1) - l, F32(0)) + np.where(ax.i1[o] == i, l, F32(0))).astype(F32)


class Float32Model:
    """disp_tail_kernels.h (and stage 2, trilinear_up_bwd) operation by operation on numpy float32, vectorised over pixels"""

    def __init__(self, x, size, gout, variant):
        with np.errstate(all="ignore"):
            x, g = np.asarray(x, F32), np.asarray(gout, F32)
            N, Di, Hi, Wi = x.shape
            Do, Ho, Wo = size
            ad, ah, aw = Axis(Di, Do, variant), Axis(Hi, Ho, variant), Axis(Wi, Wo, variant)
            one = F32(1)
            lw, lh = aw.lam[None, None, None, :], ah.lam[None, None, :, None]
            a = (one - lw) * x[..., aw.i0] + lw * x[..., aw.i1]                       # [N,Di,Hi,Wo]
            c = (one - lh) * a[:, :, ah.i0, :] + lh * a[:, :, ah.i1, :]              # [N,Di,Ho,Wo]
            assert a.dtype == F32 and c.dtype == F32
            nv = [-((one - ad.lam[o]) * c[:, ad.i0[o]] + ad.lam[o] * c[:, ad.i1[o]]) for o in range(Do)]
            m = np.full((N, Ho, Wo), -np.inf, F32)
            s, t = np.zeros((N, Ho, Wo), F32), np.zeros((N, Ho, Wo), F32)
            for o0 in range(0, Do, CHUNK):
                chunk = range(o0, min(o0 + CHUNK, Do))
                mc = m
                for o in chunk:
                    mc = np.maximum(mc, nv[o])
                resc = np.exp(m - mc)
                s, t = s * resc, t * resc
                for o in chunk:
                    e = np.exp(nv[o] - mc)
                    s = s + e
                    t = _fma32(e, F32(o), t)
                m = mc
            assert s.dtype == F32 and resc.dtype == F32
            self.out, self.mx, self.ssum = t / s, m, s
            # the column pass: per plane one accumulator in od order; the last plane's d1 == d0 readers use two
            gs = -g / self.ssum
            acc, acc1 = np.zeros((N, Di, Ho, Wo), F32), np.zeros((N, Di, Ho, Wo), F32)
            for o in range(Do):
                gv = (gs * np.exp(nv[o] - m)).astype(F32) * (F32(o) - self.out)
                d0, d1 = ad.i0[o], ad.i1[o]
                acc[:, d0] = _fma32(one - ad.lam[o], gv, acc[:, d0])
                if d1 != d0:
                    acc[:, d1] = _fma32(ad.lam[o], gv, acc[:, d1])
                else:
                    acc1[:, d0] = _fma32(ad.lam[o], gv, acc1[:, d0])
            self.gc = acc + acc1
            # stage 2: t = fmaf chain over the ow that read iw (ascending), acc = fmaf(w_h, t, acc) over the oh that read ih
            tw = np.zeros((N, Di, Ho, Wi), F32)
            iw = np.arange(Wi)
            readers = aw.reader_lists()
            for r in range(max(len(q) for q in readers)):
                ow = np.array([q[r] if r < len(q) else q[-1] if len(q) else 0 for q in readers])
                w = np.where(np.array([r < len(q) for q in readers]), _weight32(aw, ow, iw), F32(0)).astype(F32)
                tw = _fma32(w, self.gc[..., ow], tw)
            gx = np.zeros((N, Di, Hi, Wi), F32)
            ih = np.arange(Hi)
            readers = ah.reader_lists()
            for r in range(max(len(q) for q in readers)):
                oh = np.array([q[r] if r < len(q) else q[-1] if len(q) else 0 for q in readers])
                w = np.where(np.array([r < len(q) for q in readers]), _weight32(ah, oh, ih), F32(0)).astype(F32)
                gx = _fma32(w[None, None, :, None], tw[:, :, oh, :], gx)
            self.grad_x = gx

    def results(self):
        return {"out": self.out, "mx": self.mx, "ssum": self.ssum, "gc": self.gc, "grad_x": self.grad_x}
