// disp_tail_kernels.h -- Disp.forward behind its conv32x1 (models/GANet_deep.py:214-219) without the up-sampled volume:
//   v   = F.interpolate(x, [Do, Ho, Wo], mode='trilinear', align_corners=False)     x [N,Di,Hi,Wi] -> [N,Do,Ho,Wo]
//   out = DisparityRegression(Softmin(dim=1)(v))                                    -> [N,Ho,Wo]
// Trilinear interpolation is separable and the softmin-regression reduces along the axis it expands: one lane per OUTPUT
// PIXEL interpolates its column c[d] (the H-then-W part of ATen's chain, a function of d alone) once per input plane, blends
// v[od] = (1-ld) c[d0] + ld c[d1] in registers and feeds it to softmin_regression_fwd's running max / rescaled sums.
// Nothing of size Do*Ho*Wo exists in either direction:
//   forward    x -> out, mx, ssum                                                   (up_softmin_regression_fwd)
//   backward   gv[od] = -gout p_od (od - out), p recomputed from x, mx, ssum;  gc[id] = sum_od w_d(od,id) gv[od] goes to a
//              workspace [N,Di,Ho,Wo] (up_softmin_regression_bwd_cols), and trilinear_up_bwd on N*Di slices of depth 1 -> 1
//              (weight exactly 1) gathers gx[id,ih,iw] = sum_(oh,ow) w_h w_w gc[id,oh,ow]: deterministic, no atomics.
// Per axis (i0, i1, l) are up_src's (misc_kernels.h): PyTorch's align_corners=False rule evaluated in float32.
#pragma once
#include "misc_kernels.h"

namespace ga {

// The column c[d] of one output pixel (oh, ow) of slice n, and the march of od over it.  d0 never decreases with od (up_src
// is monotone), so the lane keeps c[d0], c[d1] and fetches the four values of a plane only when d0 advances; a new d0 that
// is the old d1 reuses its value.  d0 may jump (Di > Do) and d1 may equal d0 (last plane, Di == 1).
struct UpColumn {
  const float *xs;      // slice n of x
  i64 plane;            // Hi * Wi
  i64 r0, r1;           // h0 * Wi, h1 * Wi
  int w0, w1;
  float lh, lw;
  int d0, d1;           // planes held (-1: none yet)
  float c0, c1;

  GA_DEV void init(const float *xs_, const UpAxis &ah, const UpAxis &aw, int oh, int ow)
  {
    int h0, h1;
    up_src(ah, oh, h0, h1, lh);
    up_src(aw, ow, w0, w1, lw);
    xs = xs_;
    plane = (i64)ah.in * aw.in;
    r0 = (i64)h0 * aw.in; r1 = (i64)h1 * aw.in;
    d0 = d1 = -1;
    c0 = c1 = 0.f;
  }
  // ATen's order: (1-lh) * ((1-lw) a + lw b) + lh * ((1-lw) c + lw d)
  GA_DEV float fetch(int d) const
  {
    const float *p = xs + (i64)d * plane;
    const float a0 = (1.f - lw) * p[r0 + w0] + lw * p[r0 + w1];
    const float a1 = (1.f - lw) * p[r1 + w0] + lw * p[r1 + w1];
    return (1.f - lh) * a0 + lh * a1;
  }
  // v[od]; n0, n1, ld = up_src(ad, od)
  GA_DEV float at(int n0, int n1, float ld)
  {
    if (n0 != d0) {
      c0 = n0 == d1 ? c1 : fetch(n0);
      c1 = n1 == n0 ? c0 : fetch(n1);
      d0 = n0; d1 = n1;
    }
    return (1.f - ld) * c0 + ld * c1;
  }
};

// one lane per output pixel, ow fastest; od marches upwards in chunks of 8 like softmin_regression_fwd: running max m of -v
// with rescaled sums s = sum e^(-v-m), t = sum od e^(-v-m); the tail of the last chunk repeats od = Do - 1 and is masked
static __global__ void __launch_bounds__(256)
up_softmin_regression_fwd(const float *__restrict__ x, float *__restrict__ out, float *__restrict__ mx,
                          float *__restrict__ ssum, i64 N, UpAxis ad, UpAxis ah, UpAxis aw)
{
  const i64 HWo = (i64)ah.out * aw.out;
  const i64 total = N * HWo;
  const i64 stride = (i64)gridDim.x * blockDim.x;
  for (i64 o = (i64)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += stride) {
    const int ow = (int)(o % aw.out);
    const i64 r = o / aw.out;
    const int oh = (int)(r % ah.out);
    const i64 n = r / ah.out;
    UpColumn col;
    col.init(x + n * ad.in * ah.in * aw.in, ah, aw, oh, ow);
    float m = -INFINITY, s_ = 0.f, t_ = 0.f;
    for (int od0 = 0; od0 < ad.out; od0 += 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; u++) {
        int n0, n1; float ld;
        up_src(ad, od0 + u < ad.out ? od0 + u : ad.out - 1, n0, n1, ld);
        v[u] = -col.at(n0, n1, ld);
      }
      float mc = m;
#pragma unroll
      for (int u = 0; u < 8; u++)
        if (od0 + u < ad.out) mc = fmaxf(mc, v[u]);
      const float resc = expf(m - mc);          // (exp(-inf) = 0 on the first chunk)
      s_ *= resc; t_ *= resc;
#pragma unroll
      for (int u = 0; u < 8; u++)
        if (od0 + u < ad.out) { const float e = expf(v[u] - mc); s_ += e; t_ = fmaf(e, (float)(od0 + u), t_); }
      m = mc;
    }
    out[o] = t_ / s_;
    mx[o] = m;
    ssum[o] = s_;
  }
}

// The same march.  gv[od] is split between the two planes od reads: g0 collects what goes to plane d0, g1 what goes to d1.
// When d0 advances, plane d0 is complete and is written; a new d0 that is the old d1 carries g1 over, otherwise d1 is
// written as well and every plane the march jumps over gets +0.  EVERY plane of gc [N,Di,Ho,Wo] is written: the ones in
// front of the first d0 and behind the last d1 too (nobody zero-fills the workspace).
static __global__ void __launch_bounds__(256)
up_softmin_regression_bwd_cols(const float *__restrict__ x, const float *__restrict__ out, const float *__restrict__ mx,
                               const float *__restrict__ ssum, const float *__restrict__ gout, float *__restrict__ gc,
                               i64 N, UpAxis ad, UpAxis ah, UpAxis aw)
{
  const i64 HWo = (i64)ah.out * aw.out;
  const i64 total = N * HWo;
  const i64 stride = (i64)gridDim.x * blockDim.x;
  for (i64 o = (i64)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += stride) {
    const int ow = (int)(o % aw.out);
    const i64 r = o / aw.out;
    const int oh = (int)(r % ah.out);
    const i64 n = r / ah.out;
    UpColumn col;
    col.init(x + n * ad.in * ah.in * aw.in, ah, aw, oh, ow);
    float *gp = gc + n * ad.in * HWo + (o - n * HWo);        // plane id of this pixel: gp[id * HWo]
    const float m = mx[o], ov = out[o];
    const float gs = -gout[o] / ssum[o];
    int p0 = -1, p1 = -1;                                     // the planes g0, g1 belong to
    float g0 = 0.f, g1 = 0.f;
    for (int od = 0; od < ad.out; od++) {
      int n0, n1; float ld;
      up_src(ad, od, n0, n1, ld);
      if (n0 != p0) {
        if (p0 >= 0) gp[(i64)p0 * HWo] = p1 == p0 ? g0 + g1 : g0;
        if (n0 == p1 && p1 != p0) {
          g0 = g1;
        } else {
          if (p1 > p0) gp[(i64)p1 * HWo] = g1;
          for (int z = p1 + 1; z < n0; z++) gp[(i64)z * HWo] = 0.f;
          g0 = 0.f;
        }
        g1 = 0.f;
        p0 = n0; p1 = n1;
      }
      const float v = -col.at(n0, n1, ld);
      const float gv = gs * expf(v - m) * ((float)od - ov);
      g0 = fmaf(1.f - ld, gv, g0);
      g1 = fmaf(ld, gv, g1);
    }
    gp[(i64)p0 * HWo] = p1 == p0 ? g0 + g1 : g0;
    if (p1 > p0) gp[(i64)p1 * HWo] = g1;
    for (int z = p1 + 1; z < ad.in; z++) gp[(i64)z * HWo] = 0.f;
  }
}

}  // namespace ga
