// disp_conv_kernels.h -- the tails' conv32x1 = nn.Conv3d(C, 1, (3,3,3), (1,1,1), (1,1,1), bias=False) (models/GANet_deep.py:212, 232)
// as streaming kernels: a reduction over C * 27 taps into ONE output channel, not a GEMM.  x [N,C,D,H,W], y and gy [N,1,D,H,W],
// weight [1,C,3,3,3], all contiguous; [.] is zero outside the volume (padding by predication: nothing outside a tensor is read):
//   forward          y[n,d,h,w]      = sum_c sum_(kd,kh,kw) wgt[c,kd,kh,kw] [x[n,c,d+kd-1,h+kh-1,w+kw-1]]      (disp_conv_fwd)
//   data gradient    gx[n,c,z,y,x]   = sum_(kd,kh,kw) wgt[c,kd,kh,kw] [gy[n,z-kd+1,y-kh+1,x-kw+1]]              (disp_conv_bwd_data)
//   weight gradient  gw[c,kd,kh,kw]  = sum_(n,d,h,w) gy[n,d,h,w] [x[n,c,d+kd-1,h+kh-1,w+kw-1]]                  (disp_conv_bwd_weight_partials
//                                                                                                              + disp_conv_bwd_weight_sum)
// One shape for all three.  A lane owns DCV_PX = 4 consecutive w of one row h; the 64 lanes of a wave own 64 consecutive such
// groups of the plane, rows flattened (no tile edge in H or W: a wave simply runs on into the next row).  A workgroup is
// DCV_WAVES = 4 waves ON THE SAME 64 GROUPS that split the CHANNELS, and it marches DCV_DEPTH = 8 planes along d
// (grid: groups / 64 x depth chunks x N).  The 27 taps of a channel are wave-uniform: read through uniform (scalar) loads.
//   forward          per input plane z and channel c a lane fetches rows h-1, h, h+1 (16 bytes + two halo words each) ONCE and
//                    feeds all 27 taps from them: three running accumulators serve y[z+1], y[z], y[z-1].  When a plane of y is
//                    complete in a wave's channel group the four waves hand their parts over through LDS (double-buffered, one
//                    barrier per plane) and one of them adds them in wave order and stores.
//   data gradient    the 3 x 3 x 6 neighbourhood of gy lives in registers as a ring of three planes (18 words fetched per
//                    plane); per channel 27 FMAs per pixel and one 16-byte store.  No LDS, no barrier.
//   weight gradient  the same ring of gy; a lane owns the x position, so the big volume is read exactly once, 16 bytes per lane,
//                    without halo.  A wave takes DCV_CB = 4 channels per pass (4 x 27 accumulators per lane), reduces each
//                    across the wave (seg_allsum<64>) and lane 0 writes the workgroup's row [27 C] of the workspace: every
//                    channel belongs to one wave, so there is no cross-wave step.  A second small launch adds the rows in index
//                    order in fp64 and rounds once (as bn_kernels.h does its statistics): no atomics, two runs give the same bits.
// VEC: 16-byte requests (W % 4 == 0 and 16-byte aligned bases); otherwise the 4-byte twin, every word predicated on its own.
// Every element of y, gx, the workspace rows and gw is written exactly once.  64-bit element offsets throughout.
//
// ST, the storage type of the BIG volume (st_f32 / st_f16 / st_bf16 of ga_common.h), is a template parameter of all three: x of
// the forward and of the weight gradient, gx of the data gradient.  Everything else -- y, gy, the weight, the workspace rows,
// gw -- is fp32 whatever ST is, and so is all arithmetic: one kernel text per direction, so the 16-bit entries
// (include/ganet_hip_conv16.h) EQUAL the fp32 entries on the exactly up-cast x by construction.  ST::get is the exact up-cast;
// ST::put / ST::pack2 round gx ONCE on its store (to nearest even, overflow to +-inf, fp16 subnormals, one quiet NaN).  A 16-bit
// operand's VEC is one 8-byte request for a lane's four words (W % 4 == 0 and an 8-byte aligned base), its halo words 2-byte
// loads; its twin predicates every 2-byte word on its own.
//
// fp32 roundings on the longest path of one term (tests/disp_conv_ref64.py takes its bound from these; tests/test_sim_disp_conv.py
// reads them here):
//   forward          a wave's FMA chain over its ceil(C / DCV_WAVES) channels x 27 taps, then (r0 + r1) + (r2 + r3): 2 adds
//   data gradient    the FMA chain over the 27 taps
//   weight gradient  the lane's FMA chain over DCV_PX pixels x DCV_DEPTH planes, 6 steps of the wave reduction, and the
//                    rounding of the fp64 total
#pragma once
#include "ga_common.h"

namespace ga {

constexpr int DCV_WAVES = 4;       // waves per workgroup: they split the channels
constexpr int DCV_PX = 4;          // consecutive w per lane
constexpr int DCV_DEPTH = 8;       // planes a workgroup marches
constexpr int DCV_CB = 4;          // channels per pass of the weight gradient
constexpr int DCV_MAX_C = 64;
constexpr int DCV_SUM_COLS = 16;   // second stage: columns x row slices per 256-thread block
constexpr int DCV_SUM_SLICES = 16;

constexpr int DCV_L_FWD_PER_CHANNEL = 27;   // L_forward = DCV_L_FWD_PER_CHANNEL * ceil(C / DCV_WAVES) + DCV_L_FWD_MERGE
constexpr int DCV_L_FWD_MERGE = 2;
constexpr int DCV_L_BWD_DATA = 27;
constexpr int DCV_L_BWD_WEIGHT = DCV_PX * DCV_DEPTH + 6 + 1;

struct DispConvGeom {
  int N, C, D, H, W;
  int W4;       // groups of DCV_PX along a row: ceil(W / 4)
  i64 groups;   // H * W4: lanes a plane needs
};

struct DcvLane {
  bool ok;      // the lane owns a group of the plane
  int h, w0;
};

GA_DEV DcvLane dcv_lane(const DispConvGeom &g)
{
  const i64 idx = (i64)blockIdx.x * 64 + ((int)threadIdx.x & 63);
  DcvLane l;
  l.ok = idx < g.groups;
  l.h = (int)(idx / g.W4);
  l.w0 = (int)(idx % g.W4) * DCV_PX;
  return l;
}

// v[j] = [plane[h, w0 - 1 + j]], j = 0 .. 5: the lane's four words and one halo word on either side
template <bool VEC>
GA_DEV void dcv_row6(const float *__restrict__ plane, bool ok, int h, int w0, int H, int W, float (&v)[6])
{
  ok = ok && h >= 0 && h < H;
#pragma unroll
  for (int j = 0; j < 6; j++) v[j] = 0.f;
  if (!ok) return;
  const float *row = plane + (i64)h * W;
  if constexpr (VEC) {                  // (w0 % 4 == 0 and W % 4 == 0: the four words are inside)
    const f4 a = *reinterpret_cast<const f4 *>(row + w0);
    v[1] = a.x; v[2] = a.y; v[3] = a.z; v[4] = a.w;
    if (w0 > 0) v[0] = row[w0 - 1];
    if (w0 + DCV_PX < W) v[5] = row[w0 + DCV_PX];
  } else {
#pragma unroll
    for (int j = 0; j < 6; j++) {
      const int w = w0 - 1 + j;
      if (w >= 0 && w < W) v[j] = row[w];
    }
  }
}

// dcv_row6 on a 16-bit plane in two steps, so that the nine requests of a channel's three rows are all issued before the first
// conversion waits for one of them (a conversion right behind its load costs a memory round trip per request: nine waits per
// channel and plane in that form, four in this one): the patterns as they were loaded -- 0x0000, zero in both formats, where
// nothing is read -- and their up-cast afterwards.
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

// p[i] = row h - 1 + i of plane z of the volume `vol` [D,H,W]; all zero for a plane outside it
template <bool VEC>
GA_DEV void dcv_plane(const float *__restrict__ vol, i64 HW, bool ok, int z, int D, int h, int w0, int H, int W, float (&p)[3][6])
{
  ok = ok && z >= 0 && z < D;
  const float *plane = vol + (ok ? (i64)z * HW : 0);
#pragma unroll
  for (int i = 0; i < 3; i++) dcv_row6<VEC>(plane, ok, h - 1 + i, w0, H, W, p[i]);
}

// o = the lane's own four words of an ST volume at p, up-cast, without halo (p + 0 .. 3 inside the row for VEC: one 16- or 8-byte
// request; else each word w0 + k < W on its own, the others stay as they are)
template <typename ST, bool VEC> GA_DEV void dcv_own4(const typename ST::T *p, int w0, int W, float (&o)[DCV_PX])
{
  if constexpr (!VEC) {
#pragma unroll
    for (int k = 0; k < DCV_PX; k++)
      if (w0 + k < W) o[k] = ST::get(p[k]);
  } else if constexpr (sizeof(typename ST::T) == 4) {
    const f4 a = *reinterpret_cast<const f4 *>(p);
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w;
  } else {
    const uint2 a = *reinterpret_cast<const uint2 *>(p);
    o[0] = ST::get((uint16_t)(a.x & 0xffffu));
    o[1] = ST::get((uint16_t)(a.x >> 16));
    o[2] = ST::get((uint16_t)(a.y & 0xffffu));
    o[3] = ST::get((uint16_t)(a.y >> 16));
  }
}

// the lane's four words to an ST volume at p, under the same conditions; a 16-bit ST rounds here, once
template <typename ST, bool VEC> GA_DEV void dcv_store4(typename ST::T *p, int w0, int W, const float (&a)[DCV_PX])
{
  if constexpr (sizeof(typename ST::T) == 4) {
    if constexpr (VEC) {
      f4 o; o.x = a[0]; o.y = a[1]; o.z = a[2]; o.w = a[3];
      *reinterpret_cast<f4 *>(p) = o;
    } else {
#pragma unroll
      for (int k = 0; k < DCV_PX; k++)
        if (w0 + k < W) p[k] = a[k];
    }
  } else {
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
}

// ---- forward ---------------------------------------------------------------------------------------------------------------

// nine taps wk[kh * 3 + kw] of one kd on the rows v: a[p] += wk * x[h + kh - 1, w0 + p + kw - 1]
GA_DEV void dcv_fma9(const float *__restrict__ wk, const float (&v)[3][6], float (&a)[DCV_PX])
{
#pragma unroll
  for (int kh = 0; kh < 3; kh++)
#pragma unroll
    for (int kw = 0; kw < 3; kw++) {
      const float t = wk[kh * 3 + kw];
#pragma unroll
      for (int p = 0; p < DCV_PX; p++) a[p] = fmaf(t, v[kh][p + kw], a[p]);
    }
}

template <typename ST, bool VEC>
static __global__ void __launch_bounds__(64 * DCV_WAVES)
disp_conv_fwd(const typename ST::T *__restrict__ x, const float *__restrict__ wgt, float *__restrict__ y, DispConvGeom g)
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
      // the planes of y inside the chunk that plane z of x feeds
      const bool k0 = z + 1 < d1, k1 = z >= d0 && z < d1, k2 = z - 1 >= d0;
      for (int c = c0; c < c1; c++) {
        const typename ST::T *xs = x + (((i64)n * g.C + c) * g.D + z) * HW;
        const float *wc = wgt + c * 27;
        float v[3][6];
        // (this branch stays in the kernel body: behind a helper the compiler schedules every instantiation differently)
        if constexpr (sizeof(typename ST::T) == 4) {
#pragma unroll
          for (int i = 0; i < 3; i++) dcv_row6<VEC>(xs, L.ok, L.h - 1 + i, L.w0, g.H, g.W, v[i]);
        } else {
          Dcv16Row r[3];
#pragma unroll
          for (int i = 0; i < 3; i++) dcv16_row6_fetch<VEC>(xs, L.ok, L.h - 1 + i, L.w0, g.H, g.W, r[i]);
#pragma unroll
          for (int i = 0; i < 3; i++) dcv16_row6_up<ST, VEC>(r[i], v[i]);
        }
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
      // the buffer is written again two planes on, behind the next barrier, which this wave reaches only with its reads done
      if (wave == ((d - d0) & (DCV_WAVES - 1)) && L.ok) {
        const f4 r0 = red[b][0][lane], r1 = red[b][1][lane], r2 = red[b][2][lane], r3 = red[b][3][lane];
        float s[DCV_PX];
        s[0] = (r0.x + r1.x) + (r2.x + r3.x);
        s[1] = (r0.y + r1.y) + (r2.y + r3.y);
        s[2] = (r0.z + r1.z) + (r2.z + r3.z);
        s[3] = (r0.w + r1.w) + (r2.w + r3.w);
        dcv_store4<st_f32, VEC>(y + ((i64)n * g.D + d) * HW + (i64)L.h * g.W + L.w0, L.w0, g.W, s);
      }
    }
#pragma unroll
    for (int p = 0; p < DCV_PX; p++) { A[2][p] = A[1][p]; A[1][p] = A[0][p]; A[0][p] = 0.f; }
  }
}

// ---- data gradient ---------------------------------------------------------------------------------------------------------

// P[j] = plane z - 1 + j of gy around the lane.  Tap (kd, kh, kw) of pixel p reads gy[z - kd + 1, h - kh + 1, w0 + p - kw + 1]
// = P[2 - kd][2 - kh][p + 2 - kw].
template <typename ST, bool VEC>
static __global__ void __launch_bounds__(64 * DCV_WAVES)
disp_conv_bwd_data(const float *__restrict__ gy, const float *__restrict__ wgt, typename ST::T *__restrict__ gx, DispConvGeom g)
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
      if (L.ok) dcv_store4<ST, VEC>(gx + (((i64)n * g.C + c) * g.D + z) * HW + (i64)L.h * g.W + L.w0, L.w0, g.W, a);
    }
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 6; j++) { P[0][i][j] = P[1][i][j]; P[1][i][j] = P[2][i][j]; }
  }
}

// ---- weight gradient -------------------------------------------------------------------------------------------------------

// Row (n, depth chunk, group block) of ws [rows, 27 C]: this workgroup's sums over its 64 groups x DCV_DEPTH planes.  The lane
// owns the x position: gw[c, kd, kh, kw] += x[c, z, h, w0 + p] gy[z - kd + 1, h - kh + 1, w0 + p - kw + 1], the ring of gy as above.
template <typename ST, bool VEC>
static __global__ void __launch_bounds__(64 * DCV_WAVES)
disp_conv_bwd_weight_partials(const typename ST::T *__restrict__ x, const float *__restrict__ gy, float *__restrict__ ws, DispConvGeom g)
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
          if (L.ok) dcv_own4<ST, VEC>(x + (((i64)n * g.C + c) * g.D + z) * HW + (i64)L.h * g.W + L.w0, L.w0, g.W, xv);
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

// gw[k] = the sum of column k over the R rows of ws [R, K]: slice s of a block adds rows s, s + 16, ... in fp64, thread (0, k)
// adds the 16 slices in index order and rounds once
static __global__ void __launch_bounds__(DCV_SUM_COLS * DCV_SUM_SLICES)
disp_conv_bwd_weight_sum(const float *__restrict__ ws, float *__restrict__ gw, int K, i64 R)
{
  __shared__ double red[DCV_SUM_SLICES][DCV_SUM_COLS];
  const int t = (int)threadIdx.x, k = t % DCV_SUM_COLS, s = t / DCV_SUM_COLS;
  const int col = (int)blockIdx.x * DCV_SUM_COLS + k;
  double a = 0.0;
  if (col < K)
    for (i64 r = s; r < R; r += DCV_SUM_SLICES) a += (double)ws[r * K + col];
  red[s][k] = a;
  __syncthreads();
  if (s == 0 && col < K) {
    double b = 0.0;
    for (int i = 0; i < DCV_SUM_SLICES; i++) b += red[i][k];
    gw[col] = (float)b;
  }
}

}  // namespace ga
