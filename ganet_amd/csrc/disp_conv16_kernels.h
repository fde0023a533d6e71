// disp_conv16_kernels.h -- the 16-bit siblings of disp_conv_kernels.h: the tails' conv32x1 under mixed precision, where the big
// volume (x, and its gradient) is stored as fp16 / bf16 and everything the fp32 tails touch stays fp32:
//   forward          x 16-bit, weight fp32 -> y fp32                                             (disp_conv16_fwd)
//   data gradient    grad_y fp32, weight fp32 -> grad_x 16-bit, rounded ONCE on the store        (disp_conv16_bwd_data)
//   weight gradient  x 16-bit, grad_y fp32 -> fp32 workspace rows -> disp_conv_bwd_weight_sum    (disp_conv16_bwd_weight_partials)
// The contract is EQUALITY with the fp32 kernels on the exactly up-cast x (include/ganet_hip_conv16.h), so nothing of the
// arithmetic is new: the lane geometry (DCV_PX, DCV_WAVES, DCV_DEPTH, DCV_CB, dcv_lane), the accumulators and their order, the
// LDS hand-over and its merge (r0 + r1) + (r2 + r3), the wave reduction and the second-stage sum are those of
// disp_conv_kernels.h, and the fp32 operands go through its dcv_row6 / dcv_plane / dcv_store4 / dcv_fma9.  Only the loads of x
// and the store of grad_x are templated on the storage type ST (st_f16 / st_bf16 of ga_common.h): ST::get is the exact up-cast,
// ST::put / ST::pack2 the mixed contract's convert (round to nearest even, overflow to +-inf, fp16 subnormals, one quiet NaN).
// VEC: one 8-byte request for a lane's four 16-bit words (W % 4 == 0 and an 8-byte aligned 16-bit base) beside the 16-byte
// requests of the fp32 operand; halo words are 2-byte loads.  Otherwise the 2-byte / 4-byte twin, every word predicated on its
// own.  Nothing outside a tensor is read, every output element is written exactly once, 64-bit element offsets throughout.
#pragma once
#include "disp_conv_kernels.h"

namespace ga {

// the lane's four 16-bit words at p (8-byte aligned), up-cast
template <typename ST> GA_DEV void dcv16_load4(const uint16_t *p, float (&o)[DCV_PX])
{
  const uint2 a = *reinterpret_cast<const uint2 *>(p);
  o[0] = ST::get((uint16_t)(a.x & 0xffffu));
  o[1] = ST::get((uint16_t)(a.x >> 16));
  o[2] = ST::get((uint16_t)(a.y & 0xffffu));
  o[3] = ST::get((uint16_t)(a.y >> 16));
}

// dcv_row6 on a 16-bit plane, v[j] = [plane[h, w0 - 1 + j]], j = 0 .. 5, in two steps, so that the nine requests of a channel's
// three rows are all issued before the first conversion waits for one of them (a conversion right behind its load costs a
// memory round trip per request: nine waits per channel and plane in that form, four in this one): the patterns as they were
// loaded -- 0x0000, zero in both formats, where nothing is read -- and their up-cast afterwards.
struct Dcv16Row {
  uint2 own;            // VEC: the lane's four words
  uint16_t w[6];        // VEC: w[0] and w[5], the halo words; twin: all six
};

template <bool VEC>
GA_DEV void dcv16_row6_fetch(const uint16_t *__restrict__ plane, bool ok, int h, int w0, int H, int W, Dcv16Row &r)
{
  ok = ok && h >= 0 && h < H;
  r.own.x = 0u; r.own.y = 0u;
#pragma unroll
  for (int j = 0; j < 6; j++) r.w[j] = 0;
  if (!ok) return;
  const uint16_t *row = plane + (i64)h * W;
  if constexpr (VEC) {                  // (w0 % 4 == 0 and W % 4 == 0: the four words are inside)
    r.own = *reinterpret_cast<const uint2 *>(row + w0);
    if (w0 > 0) r.w[0] = row[w0 - 1];
    if (w0 + DCV_PX < W) r.w[5] = row[w0 + DCV_PX];
  } else {
#pragma unroll
    for (int j = 0; j < 6; j++) {
      const int w = w0 - 1 + j;
      if (w >= 0 && w < W) r.w[j] = row[w];
    }
  }
}

template <typename ST, bool VEC> GA_DEV void dcv16_row6_up(const Dcv16Row &r, float (&v)[6])
{
  if constexpr (VEC) {
    v[0] = ST::get(r.w[0]);
    v[1] = ST::get((uint16_t)(r.own.x & 0xffffu));
    v[2] = ST::get((uint16_t)(r.own.x >> 16));
    v[3] = ST::get((uint16_t)(r.own.y & 0xffffu));
    v[4] = ST::get((uint16_t)(r.own.y >> 16));
    v[5] = ST::get(r.w[5]);
  } else {
#pragma unroll
    for (int j = 0; j < 6; j++) v[j] = ST::get(r.w[j]);
  }
}

// the lane's own four words of x at p, without halo (weight gradient)
template <typename ST, bool VEC> GA_DEV void dcv16_own4(const uint16_t *p, int w0, int W, float (&o)[DCV_PX])
{
  if constexpr (VEC) {
    dcv16_load4<ST>(p, o);
  } else {
#pragma unroll
    for (int k = 0; k < DCV_PX; k++)
      if (w0 + k < W) o[k] = ST::get(p[k]);
  }
}

// dcv_store4 with the one rounding of the data gradient
template <typename ST, bool VEC> GA_DEV void dcv16_store4(uint16_t *p, int w0, int W, const float (&a)[DCV_PX])
{
  if constexpr (VEC) {
    uint2 o;
    o.x = ST::pack2(a[0], a[1]);
    o.y = ST::pack2(a[2], a[3]);
    *reinterpret_cast<uint2 *>(p) = o;
  } else {
#pragma unroll
    for (int k = 0; k < DCV_PX; k++)
      if (w0 + k < W) p[k] = ST::put(a[k]);
  }
}

// ---- forward: disp_conv_fwd with x read through dcv16_row6_fetch / _up -------------------------------------------------------------------

template <typename ST, bool VEC>
static __global__ void __launch_bounds__(64 * DCV_WAVES)
disp_conv16_fwd(const uint16_t *__restrict__ x, const float *__restrict__ wgt, float *__restrict__ y, DispConvGeom g)
{
  __shared__ f4 red[2][DCV_WAVES][64];
  const int lane = (int)threadIdx.x & 63, wave = GA_UNIFORM_I((int)threadIdx.x >> 6);
  const DcvLane L = dcv_lane(g);
  const int n = (int)blockIdx.z, d0 = (int)blockIdx.y * DCV_DEPTH, d1 = d0 + DCV_DEPTH < g.D ? d0 + DCV_DEPTH : g.D;
  const int CG = (g.C + DCV_WAVES - 1) / DCV_WAVES, c0 = wave * CG, c1 = c0 + CG < g.C ? c0 + CG : g.C;
  const i64 HW = (i64)g.H * g.W;
  float A[3][DCV_PX];                   // A[kd]: the wave's part of y[z + 1 - kd]
#pragma unroll
  for (int k = 0; k < 3; k++)
#pragma unroll
    for (int p = 0; p < DCV_PX; p++) A[k][p] = 0.f;
  for (int z = d0 - 1; z <= d1; z++) {
    if (z >= 0 && z < g.D) {
      const bool k0 = z + 1 < d1, k1 = z >= d0 && z < d1, k2 = z - 1 >= d0;
      for (int c = c0; c < c1; c++) {
        const uint16_t *xs = x + (((i64)n * g.C + c) * g.D + z) * HW;
        const float *wc = wgt + c * 27;
        Dcv16Row r[3];
        float v[3][6];
#pragma unroll
        for (int i = 0; i < 3; i++) dcv16_row6_fetch<VEC>(xs, L.ok, L.h - 1 + i, L.w0, g.H, g.W, r[i]);
#pragma unroll
        for (int i = 0; i < 3; i++) dcv16_row6_up<ST, VEC>(r[i], v[i]);
        if (k0) dcv_fma9(wc, v, A[0]);
        if (k1) dcv_fma9(wc + 9, v, A[1]);
        if (k2) dcv_fma9(wc + 18, v, A[2]);
      }
    }
    const int d = z - 1;                // complete in every wave now (d < d1 as z <= d1)
    if (d >= d0) {
      const int b = (d - d0) & 1;
      f4 o; o.x = A[2][0]; o.y = A[2][1]; o.z = A[2][2]; o.w = A[2][3];
      red[b][wave][lane] = o;
      GA_LDS_BARRIER();
      // (the buffer is written again two planes on, behind the next barrier: as in disp_conv_fwd)
      if (wave == ((d - d0) & (DCV_WAVES - 1)) && L.ok) {
        const f4 r0 = red[b][0][lane], r1 = red[b][1][lane], r2 = red[b][2][lane], r3 = red[b][3][lane];
        float s[DCV_PX];
        s[0] = (r0.x + r1.x) + (r2.x + r3.x);
        s[1] = (r0.y + r1.y) + (r2.y + r3.y);
        s[2] = (r0.z + r1.z) + (r2.z + r3.z);
        s[3] = (r0.w + r1.w) + (r2.w + r3.w);
        dcv_store4<VEC>(y + ((i64)n * g.D + d) * HW + (i64)L.h * g.W + L.w0, L.w0, g.W, s);
      }
    }
#pragma unroll
    for (int p = 0; p < DCV_PX; p++) { A[2][p] = A[1][p]; A[1][p] = A[0][p]; A[0][p] = 0.f; }
  }
}

// ---- data gradient: disp_conv_bwd_data with the store rounding to ST -------------------------------------------------------------

template <typename ST, bool VEC>
static __global__ void __launch_bounds__(64 * DCV_WAVES)
disp_conv16_bwd_data(const float *__restrict__ gy, const float *__restrict__ wgt, uint16_t *__restrict__ gx, DispConvGeom g)
{
  const int wave = GA_UNIFORM_I((int)threadIdx.x >> 6);
  const DcvLane L = dcv_lane(g);
  const int n = (int)blockIdx.z, d0 = (int)blockIdx.y * DCV_DEPTH, d1 = d0 + DCV_DEPTH < g.D ? d0 + DCV_DEPTH : g.D;
  const int CG = (g.C + DCV_WAVES - 1) / DCV_WAVES, c0 = wave * CG, c1 = c0 + CG < g.C ? c0 + CG : g.C;
  const i64 HW = (i64)g.H * g.W;
  const float *gys = gy + (i64)n * g.D * HW;
  float P[3][3][6];
  dcv_plane<VEC>(gys, HW, L.ok, d0 - 1, g.D, L.h, L.w0, g.H, g.W, P[0]);
  dcv_plane<VEC>(gys, HW, L.ok, d0, g.D, L.h, L.w0, g.H, g.W, P[1]);
  for (int z = d0; z < d1; z++) {
    dcv_plane<VEC>(gys, HW, L.ok, z + 1, g.D, L.h, L.w0, g.H, g.W, P[2]);
    for (int c = c0; c < c1; c++) {
      const float *wc = wgt + c * 27;
      float a[DCV_PX];
#pragma unroll
      for (int p = 0; p < DCV_PX; p++) a[p] = 0.f;
#pragma unroll
      for (int kd = 0; kd < 3; kd++)
#pragma unroll
        for (int kh = 0; kh < 3; kh++)
#pragma unroll
          for (int kw = 0; kw < 3; kw++) {
            const float t = wc[kd * 9 + kh * 3 + kw];
#pragma unroll
            for (int p = 0; p < DCV_PX; p++) a[p] = fmaf(t, P[2 - kd][2 - kh][p + 2 - kw], a[p]);
          }
      if (L.ok) dcv16_store4<ST, VEC>(gx + (((i64)n * g.C + c) * g.D + z) * HW + (i64)L.h * g.W + L.w0, L.w0, g.W, a);
    }
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 6; j++) { P[0][i][j] = P[1][i][j]; P[1][i][j] = P[2][i][j]; }
  }
}

// ---- weight gradient: disp_conv_bwd_weight_partials with x read through dcv16_own4 -----------------------------------------------

template <typename ST, bool VEC>
static __global__ void __launch_bounds__(64 * DCV_WAVES)
disp_conv16_bwd_weight_partials(const uint16_t *__restrict__ x, const float *__restrict__ gy, float *__restrict__ ws, DispConvGeom g)
{
  const int lane = (int)threadIdx.x & 63, wave = GA_UNIFORM_I((int)threadIdx.x >> 6);
  const DcvLane L = dcv_lane(g);
  const int n = (int)blockIdx.z, d0 = (int)blockIdx.y * DCV_DEPTH, d1 = d0 + DCV_DEPTH < g.D ? d0 + DCV_DEPTH : g.D;
  const i64 HW = (i64)g.H * g.W;
  const float *gys = gy + (i64)n * g.D * HW;
  const i64 row = ((i64)n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  float *wsr = ws + row * 27 * g.C;
  const int nblk = (g.C + DCV_CB - 1) / DCV_CB;
  for (int cb = wave; cb < nblk; cb += DCV_WAVES) {
    float acc[DCV_CB][27];
#pragma unroll
    for (int j = 0; j < DCV_CB; j++)
#pragma unroll
      for (int t = 0; t < 27; t++) acc[j][t] = 0.f;
    float P[3][3][6];
    dcv_plane<VEC>(gys, HW, L.ok, d0 - 1, g.D, L.h, L.w0, g.H, g.W, P[0]);
    dcv_plane<VEC>(gys, HW, L.ok, d0, g.D, L.h, L.w0, g.H, g.W, P[1]);
    for (int z = d0; z < d1; z++) {
      dcv_plane<VEC>(gys, HW, L.ok, z + 1, g.D, L.h, L.w0, g.H, g.W, P[2]);
#pragma unroll
      for (int j = 0; j < DCV_CB; j++) {
        const int c = cb * DCV_CB + j;
        if (c < g.C) {
          float xv[DCV_PX];
#pragma unroll
          for (int p = 0; p < DCV_PX; p++) xv[p] = 0.f;
          if (L.ok) dcv16_own4<ST, VEC>(x + (((i64)n * g.C + c) * g.D + z) * HW + (i64)L.h * g.W + L.w0, L.w0, g.W, xv);
#pragma unroll
          for (int kd = 0; kd < 3; kd++)
#pragma unroll
            for (int kh = 0; kh < 3; kh++)
#pragma unroll
              for (int kw = 0; kw < 3; kw++)
#pragma unroll
                for (int p = 0; p < DCV_PX; p++)
                  acc[j][kd * 9 + kh * 3 + kw] = fmaf(xv[p], P[2 - kd][2 - kh][p + 2 - kw], acc[j][kd * 9 + kh * 3 + kw]);
        }
      }
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 6; j++) { P[0][i][j] = P[1][i][j]; P[1][i][j] = P[2][i][j]; }
    }
    // (every lane of the wave is here: the reduction runs on the full wave; c < C is uniform)
#pragma unroll
    for (int j = 0; j < DCV_CB; j++) {
      const int c = cb * DCV_CB + j;
#pragma unroll
      for (int t = 0; t < 27; t++) {
        const float s = seg_allsum<64>(acc[j][t]);
        if (lane == 0 && c < g.C) wsr[c * 27 + t] = s;
      }
    }
  }
}

}  // namespace ga
