// loss_kernels.h -- the training criterion and the error read-out in one pass for gfx950.
// Reference: train.py:100-126 (valid-pixel mask, the weighted mix of smooth-L1 / MyLoss2 terms over up to three disparity
// maps, the mean absolute error of the last one), libs/GANet/functions/GANet.py:264-289 (MyLoss2Function) and
// evaluation.py:199-202 (end-point error and threshold error rate).  There every `d[mask]` is a nonzero + gather with a
// device-to-host copy behind it and every term a dozen element-wise launches; here: two launches forward, one backward,
// fixed shapes, no host round trip, no atomics (the result is bit-reproducible from run to run).
//
// Per pixel, all in fp32 with every operation rounded on its own (GA_FP_STRICT: no fma contraction, true division -- the
// emulator build and the device build compute the same terms):
//   valid   mask_mode 0: t < hi (train.py:100)      1: lo <= t && t <= hi (evaluation.py:199).  A NaN target is invalid.
//   r = p - t, v = |r|
//   kind 0  smooth-L1, beta = 1:  rho = v < 1 ? 0.5 v v : v - 0.5,  slope = v < 1 ? v : 1
//   kind 1  MyLoss2(thresh, alpha): the reference's three masked updates of ONE buffer, applied one after the other -- each
//           condition sees the value the previous update left (a mid-range value lifted above thresh + alpha by the second
//           update also takes the third).  The slope table is a chain of its own, in the reference's order.
// An invalid pixel contributes through a SELECT, never through a product with 0: a NaN / inf prediction there leaves every
// sum finite.  A NaN at a valid pixel propagates, as in torch.
// count == 0 gives loss = 0, all stats 0 and all-zero gradient maps -- NOT the NaN stock torch returns for the mean of an
// empty selection: it is what a rank with an empty shard needs (harness/steps.py), and it keeps the op capturable.
#pragma once
#include "ga_common.h"

#if defined(GA_HIPSIM)
#define GA_FP_STRICT
#else
#define GA_FP_STRICT _Pragma("clang fp contract(off)")
#endif

namespace ga {

constexpr int LOSS_BLOCK = 256;      // threads per block of the partial sums
constexpr int LOSS_MAX_BLOCKS = 64;  // grid cap of the partial sums = rows of the workspace
constexpr int LOSS_ROW = 10;         // doubles per row: count, then per map sum rho, sum |r|, #{|r| > rate_thresh}
enum { LOSS_HI, LOSS_LO, LOSS_W0, LOSS_W1, LOSS_W2, LOSS_THRESH, LOSS_ALPHA, LOSS_RATE };   // params[8]

struct LossMaps {
  const float *p[3];   // predictions
  float *g[3];         // their gradients (backward; nullptr: not wanted)
  int kind[3];
};

GA_DEV bool loss_valid(float t, float hi, float lo, int mask_mode)
{
  return mask_mode == 0 ? t < hi : (lo <= t && t <= hi);
}

GA_DEV float loss_rho(float v, int kind, float knee, float span, float far)
{
  GA_FP_STRICT
  if (kind == 0) return v < 1.f ? 0.5f * v * v : v - 0.5f;
  if (v < knee) v = v * v / knee;
  if (v >= knee && v <= far) { const float d = v - knee; v = 2.f * v - d * d / (2.f * span) - knee; }
  if (v > far) v = v + span / 2.f;
  return v;
}

GA_DEV float loss_slope(float v, int kind, float knee, float span, float far)
{
  GA_FP_STRICT
  if (kind == 0) return v >= 1.f ? 1.f : v;      // (a NaN stays a NaN)
  if (v > far) v = 1.f;
  if (v >= knee && v <= far) v = 2.f - (v - knee) / span;
  if (v < knee) v = 2.f * v / knee;
  return v;
}

// Launch 1: V (1 or 4: 16-byte loads) pixels per lane and trip, fp64 accumulators per thread, a fixed-order tree through
// LDS, one row of 1 + 3P partial sums per block.
template <int V>
__global__ void __launch_bounds__(LOSS_BLOCK)
loss_partials(LossMaps m, const float *__restrict__ target, const float *__restrict__ params, double *__restrict__ ws,
              i64 total, int P, int mask_mode)
{
  __shared__ double red[LOSS_BLOCK];
  const float hi = params[LOSS_HI], lo = params[LOSS_LO], knee = params[LOSS_THRESH], span = params[LOSS_ALPHA];
  const float far = knee + span, rate = params[LOSS_RATE];
  double acc[LOSS_ROW];
#pragma unroll
  for (int a = 0; a < LOSS_ROW; a++) acc[a] = 0.0;
  const i64 stride = (i64)gridDim.x * blockDim.x;
  for (i64 q = (i64)blockIdx.x * blockDim.x + threadIdx.x; q < total / V; q += stride) {
    float t[V], p[V];
    bool ok[V];
    st_load<st_f32, V>(target + q * V, t);
#pragma unroll
    for (int j = 0; j < V; j++) {
      ok[j] = loss_valid(t[j], hi, lo, mask_mode);
      acc[0] += ok[j] ? 1.0 : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
      if (k < P) {
        st_load<st_f32, V>(m.p[k] + q * V, p);
#pragma unroll
        for (int j = 0; j < V; j++) {
          const float v = fabsf(p[j] - t[j]);
          acc[1 + 3 * k] += ok[j] ? (double)loss_rho(v, m.kind[k], knee, span, far) : 0.0;
          acc[2 + 3 * k] += ok[j] ? (double)v : 0.0;
          acc[3 + 3 * k] += (ok[j] && v > rate) ? 1.0 : 0.0;
        }
      }
    }
  }
#pragma unroll
  for (int a = 0; a < LOSS_ROW; a++) {
    if (a < 1 + 3 * P) {                          // (uniform: every thread of the block meets the same barriers)
      red[threadIdx.x] = acc[a];
      __syncthreads();
      for (int s = LOSS_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
      }
      if (threadIdx.x == 0) ws[(i64)blockIdx.x * LOSS_ROW + a] = red[0];
      __syncthreads();
    }
  }
}

// Launch 2: one block; thread a sums column a of the rows in index order, thread 0 finishes in fp64 and rounds once.
// stats[0] = count; per map k: stats[1 + 3k] = mean rho, [2 + 3k] = mean |r| (EPE), [3 + 3k] = fraction with |r| > rate_thresh.
static __global__ void __launch_bounds__(64)
loss_finish(const double *__restrict__ ws, int rows, const float *__restrict__ params, int P, float *__restrict__ loss,
            float *__restrict__ stats)
{
  GA_FP_STRICT
  __shared__ double tot[LOSS_ROW];
  const int a = (int)threadIdx.x;
  if (a < 1 + 3 * P) {
    double s = 0.0;
    for (int b = 0; b < rows; b++) s += ws[(i64)b * LOSS_ROW + a];
    tot[a] = s;
  }
  __syncthreads();
  if (a == 0) {
    const double count = tot[0];
    double l = 0.0;
    stats[0] = (float)count;
    for (int k = 0; k < P; k++) {
      for (int j = 1; j <= 3; j++) stats[3 * k + j] = count > 0.0 ? (float)(tot[3 * k + j] / count) : 0.f;
      l += count > 0.0 ? (double)params[LOSS_W0 + k] * (tot[1 + 3 * k] / count) : 0.0;
    }
    loss[0] = (float)l;
  }
}

// Backward: g_k = valid ? (sign(r) * slope_k) * c_k : +0,  c_k = (float)(w_k * grad_loss / count) with the quotient in fp64;
// sign(0) = 0; grad_loss and count (stats[0] of the forward) are read from device memory.  Every element of every
// requested map is written.
template <int V>
__global__ void __launch_bounds__(256)
loss_bwd(LossMaps m, const float *__restrict__ target, const float *__restrict__ params, const float *__restrict__ stats,
         const float *__restrict__ grad_loss, i64 total, int P, int mask_mode)
{
  GA_FP_STRICT
  const float hi = params[LOSS_HI], lo = params[LOSS_LO], knee = params[LOSS_THRESH], span = params[LOSS_ALPHA];
  const float far = knee + span;
  const double count = (double)stats[0], gl = (double)grad_loss[0];
  float c[3];
#pragma unroll
  for (int k = 0; k < 3; k++) c[k] = (k < P && count > 0.0) ? (float)((double)params[LOSS_W0 + k] * gl / count) : 0.f;
  const i64 stride = (i64)gridDim.x * blockDim.x;
  for (i64 q = (i64)blockIdx.x * blockDim.x + threadIdx.x; q < total / V; q += stride) {
    float t[V], p[V], g[V];
    bool ok[V];
    st_load<st_f32, V>(target + q * V, t);
#pragma unroll
    for (int j = 0; j < V; j++) ok[j] = count > 0.0 && loss_valid(t[j], hi, lo, mask_mode);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      if (k < P && m.g[k]) {
        st_load<st_f32, V>(m.p[k] + q * V, p);
#pragma unroll
        for (int j = 0; j < V; j++) {
          const float r = p[j] - t[j];
          const float sg = r > 0.f ? 1.f : (r < 0.f ? -1.f : 0.f);
          const float gv = sg * loss_slope(fabsf(r), m.kind[k], knee, span, far) * c[k];
          g[j] = ok[j] ? gv : 0.f;
        }
        st_store<st_f32, V>(m.g[k] + q * V, g);
      }
    }
  }
}

}  // namespace ga
