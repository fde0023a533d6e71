// mixed_train_kernels.h -- the adjoint of the 16-bit cost volume, which a TRAINING step under torch.autocast needs beside
// mixed_kernels.h, for gfx950, and the apply pass of the 16-bit BatchNorm site's forward.  (Its batch statistics and its backward are
// bn_kernels.h's kernels on 16-bit storage types; the backward of the 16-bit L1 normalisation is misc_kernels.h's
// l1norm_bwd<KT, Tx>.)  16-bit STORAGE (ga_common.h: st_f16 / st_bf16), fp32 and fp64 arithmetic: every operand is up-cast exactly, every
// 16-bit result is rounded ONCE on its store.
//
// cost_volume_bwd16: misc_kernels.h's cost_volume_bwd on 16-bit gcost / gx / gy; fp32 sums over i ascending, masked adds.
#pragma once
#include "mixed_kernels.h"

namespace ga {

// ---- BatchNorm forward, the apply pass on a 16-bit x -------------------------------------------------------------------------

// bn_kernels.h's bn_train_apply term for term, with x (Tx, 16-bit) and y (Ty) on storage types and __restrict__ on both: x is
// saved for the backward, so there is no in-place form.  A sibling, not one template with the fp32 kernel: that one's text (no
// __restrict__ on x and y, the loop in bn_apply_share) costs these instantiations 1 to 3 instructions, and on the smallest
// BatchNorm site of the model that form measured 2.2 % over the parent where 2 % is allowed (DESIGN.md;
// profiles/r24a_bn_train_apply_timing.txt).  The statistics in front of it and both backward passes are bn_kernels.h's own kernels.
template <typename Tx, typename Ty, int V>
__global__ void __launch_bounds__(BN_BLOCK)
bn_train_apply_mixed(const typename Tx::T *__restrict__ x, const float *__restrict__ rem, const float *__restrict__ weight,
                     const float *__restrict__ bias, float *running_mean, float *running_var, const double *__restrict__ ws,
                     typename Ty::T *__restrict__ y, float *save_mean, float *save_invstd, BnGeom g, float momentum, float eps,
                     int relu)
{
  __shared__ double rows[2 * BN_MAX_ROWS];
  const int c = (int)blockIdx.y;
  double s1, s2;
  bn_sum_rows(ws, c, g.Rs * g.Rn, rows, s1, s2);
  const double M = (double)g.N * (double)g.S;
  const double dm = s1 / M, mean = (double)Tx::get(x[(i64)c * g.S]) + dm;
  double var = s2 / M - dm * dm;
  var = var < 0.0 ? 0.0 : var;                      // (rounding only; a NaN stays)
  const float mean_f = (float)mean, invstd_f = (float)(1.0 / sqrt(var + (double)eps));
  float scale, shift;
  bn_scale_shift(weight ? weight[c] : 1.f, bias ? bias[c] : 0.f, mean_f, invstd_f, scale, shift);
  if (blockIdx.x == 0 && threadIdx.x == 0) {        // once per channel
    save_mean[c] = mean_f;
    save_invstd[c] = invstd_f;
    if (running_mean) {
      const double m = (double)momentum;
      running_mean[c] = (float)((1.0 - m) * (double)running_mean[c] + m * mean);
      running_var[c] = (float)((1.0 - m) * (double)running_var[c] + m * (var * M / (M - 1.0)));
    }
  }
  const int rs = (int)blockIdx.x % g.Rs, rn = (int)blockIdx.x / g.Rs;
  const i64 SV = g.S / V, stride = (i64)g.Rs * BN_BLOCK;
  const bool has_rem = rem != nullptr;
  for (int n = rn; n < g.N; n += g.Rn) {
    const i64 base = ((i64)n * g.C + c) * g.S;
    for (i64 i = (i64)rs * BN_BLOCK + threadIdx.x; i < SV; i += stride) {
      float a[V], r[V], o[V];
      st_load<Tx, V>(x + base + i * V, a);
      if (has_rem) st_load<st_f32, V>(rem + base + i * V, r);
#pragma unroll
      for (int j = 0; j < V; j++) {
        const float z = bn_z(a[j], scale, shift, has_rem ? r[j] : 0.f, has_rem);
        o[j] = relu ? relu_keep_nan(z) : z;
      }
      st_store<Ty, V>(y + base + i * V, o);
    }
  }
}

// ---- cost volume adjoint -----------------------------------------------------------------------------------------------------

// gx[n,c,h,w] = sum_{i<=w} g[n,c,i,h,w];  gy[n,c,h,w] = sum_{i: w+i<W} g[n,C+c,i,h,w+i]  on 16-bit storage: cost_volume_bwd's
// sums -- fp32, i ascending, unconditional loads (column clamped into the row) with masked adds -- rounded once on the store.
// V = 8: eight consecutive columns per lane (W % 8 == 0, 16-byte aligned buffers): the left half is one 16-byte load per
// disparity, the shifted right half eight 2-byte loads at any alignment, U = 4 disparities (36 requests) in flight;
// V = 1: the scalar twin, U = 8 as in the fp32 kernel.
template <typename T16, int V>
__global__ void __launch_bounds__(256)
cost_volume_bwd16(const uint16_t *__restrict__ gcost, uint16_t *__restrict__ gx, uint16_t *__restrict__ gy,
                  int N, int C, int Dn, int H, int W)
{
  constexpr int U = V == 1 ? 8 : 4;
  const int WV = W / V;
  const i64 total = (i64)N * C * H * WV;
  const i64 HW = (i64)H * W;
  const i64 stride = (i64)gridDim.x * blockDim.x;
  for (i64 q = (i64)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += stride) {
    const int w = (int)(q % WV) * V;
    i64 r = q / WV;
    const int h = (int)(r % H); r /= H;
    const int c = (int)(r % C);
    const int n = (int)(r / C);
    const uint16_t *gl = gcost + (((i64)n * 2 * C + c) * Dn) * HW + (i64)h * W;
    const uint16_t *gr = gcost + (((i64)n * 2 * C + C + c) * Dn) * HW + (i64)h * W;
    float sx[V], sy[V];
#pragma unroll
    for (int j = 0; j < V; j++) sx[j] = sy[j] = 0.f;
    for (int i0 = 0; i0 < Dn; i0 += U) {
      float a[U][V];
      uint16_t b[U][V];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int i = i0 + u < Dn ? i0 + u : Dn - 1;
        st_load<T16, V>(gl + (i64)i * HW + w, a[u]);
#pragma unroll
        for (int j = 0; j < V; j++) {
          const int wr = w + j + i < W ? w + j + i : W - 1;
          b[u][j] = gr[(i64)i * HW + wr];
        }
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int i = i0 + u;
#pragma unroll
        for (int j = 0; j < V; j++) {
          if (i < Dn && i <= w + j) sx[j] += a[u][j];
          if (i < Dn && w + j + i < W) sy[j] += T16::get(b[u][j]);
        }
      }
    }
    st_store<T16, V>(gx + q * V, sx);
    st_store<T16, V>(gy + q * V, sy);
  }
}

}  // namespace ga
