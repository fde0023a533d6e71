// bn_kernels.h -- training-mode BatchNorm + (residual) + ReLU as streaming kernels for gfx950.
// Reference: models/GANet_deep.py:35-41 (BasicConv.forward: conv -> bn -> F.relu(inplace=True), 64 call sites) and :270-277
// (SGABlock's tail: conv_refine's BatchNorm3d, `x += rem`, relu).  Stock PyTorch moves about 5 volumes forward (statistics,
// normalise, relu_) and 8 backward (threshold_backward, the reduction and the apply pass of the BatchNorm backward); here
// 3 forward (x for the sums, x again, y) and 5 backward (x and grad_y for the sums, both again, grad_x): the backward
// recomputes the ReLU mask from x, the output is never read back.
//
// Tensors [N, C, S] (S = D*H*W or H*W, contiguous slices), 64-bit offsets.  Two launches each way, no atomics:
//   partial sums   grid (R, C): block (r, c) sums its share of channel c into fp64 row r of the caller's workspace
//                  (per-thread fp64 accumulators, a fixed-order tree through LDS)
//   apply          the same grid; every block re-sums its channel's R rows in index order (so two runs are bit-identical),
//                  finishes the statistics in fp64 and streams its share; block r = 0 of the channel also writes the saved
//                  statistics and the running buffers (forward) / grad_weight and grad_bias (backward), exactly once.
// R = Rs * Rn rows: Rs blocks along a slice (at most one trip of BN_BLOCK lanes each before the cap), Rn over the N slices
// of the channel, R <= min(BN_MAX_ROWS, BN_TARGET_BLOCKS / C): about 2048 blocks on 256 CUs and at most 64 rows to re-sum.
// V = 4: 16-byte requests (S % 4 == 0 and 16-byte aligned bases); V = 1: the scalar twin.
//
// One kernel text for the statistics and for both backward passes; the STORAGE types of the volumes (st_f32 / st_f16 / st_bf16
// of ga_common.h) are template parameters: Tx of x and gx, Ty of gy; rem and grem are fp32.  All fp32 is the instantiation st_f32
// at V = 4 | 1.  Under torch.autocast x is 16-bit and gy is x's type, or fp32 in front of an SGABlock (no residual there);
// statistics, gw and gb stay fp32.  A 16-bit operand is up-cast exactly, the arithmetic below is the same fp32 / fp64 term for
// term, and a 16-bit result is rounded ONCE on its store; there V = 8 | 1: 16-byte requests of 16-bit storage (S % 8 == 0).  The
// lanes of V = 8 cover other elements than the lanes of V = 4 do, so the fp64 sums of a mixed call agree with the fp32 entry's to
// rounding, and bit for bit where every partial sum is exact (tests/mixed_train_cases.py).  The two apply kernels of the forward
// are fp32 only: their 16-bit forms are siblings (mixed_train_kernels.h: bn_train_apply_mixed, mixed_kernels.h:
// bn_affine_apply_mixed), which say why.
//
// Arithmetic (tests/bn_ref64.py states it in float64):
//   mean = sum x / M, var = sum x^2 / M - mean^2 (biased), invstd = 1 / sqrt(var + eps), all fp64, M = N * S -- with both
//   sums taken over d = x - x0, x0 = the channel's first value (exact in fp64; mean = x0 + sum d / M): the same quantities,
//   but a channel that sits far from zero (x = 1000 +- 0.01) no longer loses its variance to the rounding of sum x^2 / M,
//   which at 1e6 is as large as the 2^-22 the tests allow on invstd;
//   mean and invstd rounded to fp32 once;  scale = weight * invstd (fp32), shift = fmaf(-mean, scale, bias)
//   running_mean = (1 - m) running_mean + m mean,  running_var = (1 - m) running_var + m var M / (M - 1): fp64, rounded once
//   z = fmaf(x, scale, shift) [+ rem],  y = relu ? relu_keep_nan(z) : z
//   g = relu && z <= 0 ? 0 : grad_y   (z recomputed by the same expression: the mask is the forward's, bit for bit)
//   grad_bias = sum g, grad_weight = invstd * sum g (x - mean)          (fp64 sums, (x - mean) formed before the product)
//   grad_x = scale * (g - k1 - (x - mean) * q),  k1 = sum g / M, q = invstd^2 * sum g (x - mean) / M, each rounded to fp32 once
//   grad_rem = g
// Every fp32 operation is rounded on its own (no contraction beyond the two fmaf written out).
#pragma once
#include "ga_common.h"

#if defined(GA_HIPSIM)
#define BN_FP_STRICT
#else
#define BN_FP_STRICT _Pragma("clang fp contract(off)")
#endif

namespace ga {

constexpr int BN_BLOCK = 256;           // threads per block
constexpr int BN_MAX_ROWS = 64;         // rows (blocks) per channel at most
constexpr int BN_TARGET_BLOCKS = 2048;  // blocks per launch aimed at: 256 CUs x 8

struct BnGeom {
  int N, C;
  i64 S;
  int Rs, Rn;   // blocks along a slice x blocks over the slices of one channel; R = Rs * Rn rows of 2 doubles per channel
};

// the pre-activation, the one expression forward and backward share
GA_DEV float bn_z(float x, float scale, float shift, float rem, bool has_rem)
{
  BN_FP_STRICT
  const float z = fmaf(x, scale, shift);
  return has_rem ? z + rem : z;
}

GA_DEV void bn_scale_shift(float weight, float bias, float mean, float invstd, float &scale, float &shift)
{
  BN_FP_STRICT
  scale = weight * invstd;
  shift = fmaf(-mean, scale, bias);
}

// block-wide sums of two fp64 values in a fixed order; thread 0 stores row (c, r)
GA_DEV void bn_store_row(double a, double b, double *red, double *__restrict__ ws, int R)
{
  const int t = (int)threadIdx.x;
  red[t] = a;
  red[BN_BLOCK + t] = b;
  __syncthreads();
  for (int s = BN_BLOCK / 2; s > 0; s >>= 1) {
    if (t < s) {
      red[t] += red[t + s];
      red[BN_BLOCK + t] += red[BN_BLOCK + t + s];
    }
    __syncthreads();
  }
  if (t == 0) {
    const i64 row = (i64)blockIdx.y * R + blockIdx.x;
    ws[2 * row] = red[0];
    ws[2 * row + 1] = red[BN_BLOCK];
  }
}

// the channel's two sums from its R <= BN_MAX_ROWS rows, in index order: thread r fetches row r (one 16-byte request per lane,
// one trip to the L2), the rows go through LDS and every thread adds them up by row number -- a loop of dependent loads
// from one address after the other would cost every block R memory latencies before its first store
GA_DEV void bn_sum_rows(const double *__restrict__ ws, int c, int R, double *rows /* LDS, 2 * BN_MAX_ROWS */, double &a, double &b)
{
  const int t = (int)threadIdx.x;
  if (t < R) {
    rows[2 * t] = ws[2 * ((i64)c * R + t)];
    rows[2 * t + 1] = ws[2 * ((i64)c * R + t) + 1];
  }
  __syncthreads();
  a = 0.0;
  b = 0.0;
  for (int r = 0; r < R; r++) {
    a += rows[2 * r];
    b += rows[2 * r + 1];
  }
}

// ---- forward -------------------------------------------------------------------------------------------------------------

template <typename Tx, int V>
__global__ void __launch_bounds__(BN_BLOCK)
bn_stat_partials(const typename Tx::T *__restrict__ x, double *__restrict__ ws, BnGeom g)
{
  __shared__ double red[2 * BN_BLOCK];
  const int c = (int)blockIdx.y, rs = (int)blockIdx.x % g.Rs, rn = (int)blockIdx.x / g.Rs;
  const i64 SV = g.S / V, stride = (i64)g.Rs * BN_BLOCK;
  const double x0 = (double)Tx::get(x[(i64)c * g.S]);       // the channel's first value: the origin of both sums
  double s1 = 0.0, s2 = 0.0;
  for (int n = rn; n < g.N; n += g.Rn) {
    const typename Tx::T *xs = x + ((i64)n * g.C + c) * g.S;
    for (i64 i = (i64)rs * BN_BLOCK + threadIdx.x; i < SV; i += stride) {
      float a[V];
      st_load<Tx, V>(xs + i * V, a);
#pragma unroll
      for (int j = 0; j < V; j++) {
        const double d = (double)a[j] - x0;
        s1 += d;
        s2 += d * d;
      }
    }
  }
  bn_store_row(s1, s2, red, ws, g.Rs * g.Rn);
}

// x and y carry no __restrict__: in the eval form y may BE x
template <int V>
GA_DEV void bn_apply_share(const float *x, const float *__restrict__ rem, float *y, const BnGeom &g, int c, float scale,
                           float shift, int relu)
{
  const int rs = (int)blockIdx.x % g.Rs, rn = (int)blockIdx.x / g.Rs;
  const i64 SV = g.S / V, stride = (i64)g.Rs * BN_BLOCK;
  const bool has_rem = rem != nullptr;
  for (int n = rn; n < g.N; n += g.Rn) {
    const i64 base = ((i64)n * g.C + c) * g.S;
    for (i64 i = (i64)rs * BN_BLOCK + threadIdx.x; i < SV; i += stride) {
      float a[V], r[V], o[V];
      st_load<st_f32, V>(x + base + i * V, a);
      if (has_rem) st_load<st_f32, V>(rem + base + i * V, r);
#pragma unroll
      for (int j = 0; j < V; j++) {
        const float z = bn_z(a[j], scale, shift, has_rem ? r[j] : 0.f, has_rem);
        o[j] = relu ? relu_keep_nan(z) : z;
      }
      st_store<st_f32, V>(y + base + i * V, o);
    }
  }
}

template <int V>
__global__ void __launch_bounds__(BN_BLOCK)
bn_train_apply(const float *x, const float *__restrict__ rem, const float *__restrict__ weight, const float *__restrict__ bias,
               float *running_mean, float *running_var, const double *__restrict__ ws, float *y, float *save_mean,
               float *save_invstd, BnGeom g, float momentum, float eps, int relu)
{
  __shared__ double rows[2 * BN_MAX_ROWS];
  const int c = (int)blockIdx.y;
  double s1, s2;
  bn_sum_rows(ws, c, g.Rs * g.Rn, rows, s1, s2);
  const double M = (double)g.N * (double)g.S;
  const double dm = s1 / M, mean = (double)x[(i64)c * g.S] + dm;   // (sums over x - x0, see bn_stat_partials)
  double var = s2 / M - dm * dm;
  var = var < 0.0 ? 0.0 : var;                      // (rounding only: the exact value is never negative; a NaN stays)
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
  bn_apply_share<V>(x, rem, y, g, c, scale, shift, relu);
}

// eval mode: y = relu(scale[c] * x + shift[c] [+ rem]) with the BatchNorm folded from its running statistics
template <int V>
__global__ void __launch_bounds__(BN_BLOCK)
bn_affine_apply(const float *x, const float *__restrict__ rem, const float *__restrict__ scale, const float *__restrict__ shift,
                float *y, BnGeom g, int relu)
{
  const int c = (int)blockIdx.y;
  bn_apply_share<V>(x, rem, y, g, c, scale[c], shift[c], relu);
}

// ---- backward ------------------------------------------------------------------------------------------------------------

template <typename Tx, typename Ty, int V>
__global__ void __launch_bounds__(BN_BLOCK)
bn_bwd_partials(const typename Tx::T *__restrict__ x, const float *__restrict__ rem, const typename Ty::T *__restrict__ gy,
                const float *__restrict__ weight, const float *__restrict__ bias, const float *__restrict__ save_mean,
                const float *__restrict__ save_invstd, double *__restrict__ ws, BnGeom g, int relu)
{
  __shared__ double red[2 * BN_BLOCK];
  const int c = (int)blockIdx.y, rs = (int)blockIdx.x % g.Rs, rn = (int)blockIdx.x / g.Rs;
  const i64 SV = g.S / V, stride = (i64)g.Rs * BN_BLOCK;
  const bool has_rem = rem != nullptr;
  const float mean = save_mean[c];
  float scale, shift;
  bn_scale_shift(weight ? weight[c] : 1.f, bias ? bias[c] : 0.f, mean, save_invstd[c], scale, shift);
  double s1 = 0.0, s2 = 0.0;
  for (int n = rn; n < g.N; n += g.Rn) {
    const i64 base = ((i64)n * g.C + c) * g.S;
    for (i64 i = (i64)rs * BN_BLOCK + threadIdx.x; i < SV; i += stride) {
      float a[V], r[V], d[V];
      st_load<Tx, V>(x + base + i * V, a);
      st_load<Ty, V>(gy + base + i * V, d);
      if (relu && has_rem) st_load<st_f32, V>(rem + base + i * V, r);
#pragma unroll
      for (int j = 0; j < V; j++) {
        float gj = d[j];
        if (relu) gj = bn_z(a[j], scale, shift, has_rem ? r[j] : 0.f, has_rem) <= 0.f ? 0.f : gj;
        s1 += (double)gj;
        s2 += (double)gj * ((double)a[j] - (double)mean);
      }
    }
  }
  bn_store_row(s1, s2, red, ws, g.Rs * g.Rn);
}

// gx / grem / gw / gb: nullptr = not wanted.  With neither gx nor grem the launch is one block per channel (the parameter
// gradients only) and `g` still names the rows the partial sums wrote.
template <typename Tx, typename Ty, int V>
__global__ void __launch_bounds__(BN_BLOCK)
bn_bwd_apply(const typename Tx::T *__restrict__ x, const float *__restrict__ rem, const typename Ty::T *__restrict__ gy,
             const float *__restrict__ weight, const float *__restrict__ bias, const float *__restrict__ save_mean,
             const float *__restrict__ save_invstd, const double *__restrict__ ws, typename Tx::T *__restrict__ gx,
             float *__restrict__ grem, float *__restrict__ gw, float *__restrict__ gb, BnGeom g, int relu)
{
  BN_FP_STRICT
  __shared__ double rows[2 * BN_MAX_ROWS];
  const int c = (int)blockIdx.y;
  double sg, sgx;
  bn_sum_rows(ws, c, g.Rs * g.Rn, rows, sg, sgx);
  const double M = (double)g.N * (double)g.S;
  const float mean = save_mean[c], invstd = save_invstd[c];
  const float k1 = (float)(sg / M), q = (float)((double)invstd * (double)invstd * sgx / M);
  float scale, shift;
  bn_scale_shift(weight ? weight[c] : 1.f, bias ? bias[c] : 0.f, mean, invstd, scale, shift);
  if (blockIdx.x == 0 && threadIdx.x == 0) {        // once per channel
    if (gw) gw[c] = (float)((double)invstd * sgx);
    if (gb) gb[c] = (float)sg;
  }
  if (!gx && !grem) return;
  const int rs = (int)blockIdx.x % g.Rs, rn = (int)blockIdx.x / g.Rs;
  const i64 SV = g.S / V, stride = (i64)g.Rs * BN_BLOCK;
  const bool has_rem = rem != nullptr;
  for (int n = rn; n < g.N; n += g.Rn) {
    const i64 base = ((i64)n * g.C + c) * g.S;
    for (i64 i = (i64)rs * BN_BLOCK + threadIdx.x; i < SV; i += stride) {
      float a[V], r[V], d[V], o[V];
      st_load<Tx, V>(x + base + i * V, a);
      st_load<Ty, V>(gy + base + i * V, d);
      if (relu && has_rem) st_load<st_f32, V>(rem + base + i * V, r);
#pragma unroll
      for (int j = 0; j < V; j++) {
        if (relu) d[j] = bn_z(a[j], scale, shift, has_rem ? r[j] : 0.f, has_rem) <= 0.f ? 0.f : d[j];
        o[j] = scale * (d[j] - k1 - (a[j] - mean) * q);
      }
      if (gx) st_store<Tx, V>(gx + base + i * V, o);
      if (grem) st_store<st_f32, V>(grem + base + i * V, d);
    }
  }
}

}  // namespace ga
