// cl_kernels.h -- the channels-last inference path (include/ganet_hip_cl.h): the folded BatchNorm + (residual) + ReLU sites and
// the cost volume on tensors whose memory layout is [N, S, C] (S = D*H*W; torch.channels_last_3d), beside the planar [N, C, S]
// the rest of the library computes in.  The convolution library computes in channels-last and repacks planar operands around
// every 3-D convolution; SGA stays planar (its C slices are independent scans).  So the layout changes INSIDE these streaming
// kernels: the site in front of an SGABlock reads [N,S,C] and writes [N,C,S], the one behind SGA the other way, the tail reads
// both -- no extra pass over a volume anywhere.
//
// Per element the arithmetic is bn_kernels.h's apply form, through the same device function (bn_z), then relu_keep_nan:
//   z = fmaf(x, scale[c], shift[c]) [+ rem],  y = relu ? (z <= 0 ? 0 : z) : z          (a NaN passes through)
//
//   cl_bn_stream<V>                     x cl -> y cl, no rem: a plain stream with c = index % C; y may BE x
//   cl_bn_transpose<SRC_CL, MODE, VC, VP>  every form in which one operand changes layout.  A tile of CL_CB channels x CL_T
//                                       positions of that operand is staged RAW through LDS in its own layout's lane order and
//                                       consumed in y's lane order, where the other operand (if any) is loaded directly:
//       SRC_CL = 1, MODE 0   x cl -> y planar                 staged x
//       SRC_CL = 1, MODE 1   x cl, rem planar -> y planar     staged x,   direct rem
//       SRC_CL = 0, MODE 0   x planar -> y cl                 staged x
//       SRC_CL = 0, MODE 2   x cl, rem planar -> y cl         staged rem, direct x (y may BE x: one lane reads, then writes, an address)
//       SRC_CL = 0, MODE 3   x planar, rem planar -> y cl     both read by the planar lanes, the RESULT staged (a convolution
//                                                             that answered in planar where channels-last was expected)
//     Both global sides are coalesced: channels-last lanes run over the tile's elements in memory order (for C <= CL_CB a
//     tile is ONE contiguous range of CL_T * C floats), planar lanes along S.  VC = 4 / VP = 4: 16-byte requests on the
//     channels-last side (C % 4 == 0) / the planar side (S % 4 == 0) with 16-byte aligned bases; 1: scalar requests.
//     The channel axis is blocked by CL_CB (any C; the host refuses C > 65535), tiles are taken grid-stride, 64-bit offsets.
//
// The LDS image.  Element (c, s) of a tile sits at  cl_row(c) + cl_col(s):
//     cl_row(c) = c * CL_LD + 2 * (c / 32),  CL_LD = 133 (odd)
//     cl_col(s) = (s % 4) * 33 + s / 4   where the planar side moves four positions per lane (VP = 4),  s otherwise
//   every access is a 4-byte one (ds_read_b32 / ds_write_b32: 32 banks, lanes conflict within a half-wave of 32).
//   planar side, VP = 4: lane q of a channel holds positions 4q .. 4q+3 and its j-th access is column j * 33 + q: the 32 lanes
//     of a half-wave are 32 consecutive q of ONE channel (CL_T / 4 = 32) -> 32 consecutive banks.  VP = 1: consecutive s.
//   channels-last side, VC = 4: lane l of a half-wave holds channels 4k .. 4k+3 (k = l % (C/4)) of position s0 + l / (C/4), its
//     j-th access is row 4k + j.  bank = (4k + j) * 133 + 2 * ((4k + j) / 32) + col(s)  (mod 32)  =  4 * (5k mod 8) + const(j) + 2 * (k / 8) + col(s):
//       C = 32: k = 0..7 and four positions of one aligned group of 4, col(s) = s % 4 + const -> 8 x 4 distinct banks
//       C = 64: k = 0..15 and two positions: k and k + 8 differ by the 2 of cl_row, the two positions by 1 -> 32 distinct banks
//       C = 48: 12 lanes per position, a half-wave spans parts of up to four positions that need not share s / 4: two lanes can
//               meet on a bank (2-way, on some half-waves).  On ds_write_b32 a 2-way conflict is hidden behind the
//               instruction's own issue cycles; the consuming side of that form (planar) is conflict-free.  In the forms that
//               READ in channels-last order (y cl) such a half-wave pays one extra LDS cycle.
//
// Cost volume, channels-last: x, y planar [N,C,H,W] -> cost [N,Dn,H,W,2C], the values of cost_volume_fwd permuted:
//   cost[n,d,h,w,c] = w >= d ? x[n,c,h,w] : +0,  cost[n,d,h,w,C+c] = w >= d ? y[n,c,h,w-d] : +0  (copies of bits).
//   A block takes (n, h, CV_TW columns, CV_CB channels, CV_DB disparities): the x tile and the y window of CV_TW + CV_DB - 1
//   columns are transposed through LDS once and reused for every d of the chunk; the stores run over (d, half, w, c) in memory
//   order, 16 bytes per lane where C % 4 == 0 and the cost base is 16-byte aligned.
#pragma once
#include "bn_kernels.h"

namespace ga {

constexpr int CL_BLOCK = 256;        // threads per block
constexpr int CL_T = 128;            // positions per tile
constexpr int CL_CB = 64;            // channels per tile
constexpr int CL_LD = 133;           // floats between two channel rows of the LDS image
constexpr int CL_QS = CL_T / 4 + 1;  // floats between the four position phases of a row (VP = 4)
constexpr int CL_MAX_BLOCKS = 2048;  // blocks per launch at most (256 CUs x 8): the tiles / groups beyond are a second trip
static_assert(3 * CL_QS + CL_T / 4 - 1 + 2 * ((CL_CB - 1) >> 5) < CL_LD && CL_LD % 2 == 1, "a row of the LDS image fits its stride");

struct ClGeom {
  int N, C;
  i64 S;
  i64 nst;      // tiles along S
  int ncb;      // channel blocks
  i64 ntiles;   // N * nst * ncb
};

GA_DEV int cl_row(int c) { return c * CL_LD + 2 * (c >> 5); }
template <int VP> GA_DEV int cl_col(int s) { return VP == 4 ? (s & 3) * CL_QS + (s >> 2) : s; }

GA_DEV float cl_bn_one(float x, float scale, float shift, float rem, bool has_rem, int relu)
{
  const float z = bn_z(x, scale, shift, rem, has_rem);
  return relu ? relu_keep_nan(z) : z;
}

// x and y carry no __restrict__: y may BE x
template <int V>
__global__ void __launch_bounds__(CL_BLOCK)
cl_bn_stream(const float *x, const float *__restrict__ scale, const float *__restrict__ shift, float *y, i64 groups, int C, int relu)
{
  const i64 stride = (i64)gridDim.x * CL_BLOCK, first = (i64)blockIdx.x * CL_BLOCK + threadIdx.x;
  // the channel of a lane's first element, then stepped: one 64-bit remainder per lane instead of one per trip
  const int step = (int)((stride * V) % C);
  int c = (int)((first * V) % C) - step;
  for (i64 i = first; i < groups; i += stride) {
    c += step;
    c = c >= C ? c - C : c;
    float a[V], o[V];
    st_load<st_f32, V>(x + i * V, a);
#pragma unroll
    for (int j = 0; j < V; j++) o[j] = cl_bn_one(a[j], scale[c + j], shift[c + j], 0.f, false, relu);
    st_store<st_f32, V>(y + i * V, o);
  }
}

// direct and y carry no __restrict__: in MODE 2 y may BE x (= direct)
template <bool SRC_CL, int MODE, int VC, int VP>
__global__ void __launch_bounds__(CL_BLOCK)
cl_bn_transpose(const float *__restrict__ staged, const float *direct, const float *__restrict__ scale,
                const float *__restrict__ shift, float *y, ClGeom g, int relu)
{
  static_assert(SRC_CL ? (MODE == 0 || MODE == 1) : (MODE == 0 || MODE == 2 || MODE == 3), "cl_bn_transpose: no such form");
  __shared__ float tile[CL_CB * CL_LD];
  const int tid = (int)threadIdx.x;
  for (i64 t = blockIdx.x; t < g.ntiles; t += gridDim.x) {
    const int cb = (int)(t % g.ncb);
    const i64 r = t / g.ncb;
    const i64 s0 = (r % g.nst) * CL_T;
    const i64 n = r / g.nst;
    const int c0 = cb * CL_CB;
    const int cw = g.C - c0 < CL_CB ? g.C - c0 : CL_CB;
    const int tw = (int)(g.S - s0 < CL_T ? g.S - s0 : CL_T);
    const int ne = tw * cw;        // channels-last lanes: elements of the tile in memory order (s, c); cw % VC == 0
    const int nq = tw / VP;        // planar lanes: groups of VP positions per channel; tw % VP == 0
    const i64 cl0 = (n * g.S + s0) * g.C + c0;          // (position s0, channel c0) in a channels-last tensor
    const i64 pl0 = (n * g.C + c0) * g.S + s0;          // the same in a planar one
    if constexpr (SRC_CL) {
      for (int e = tid * VC; e < ne; e += CL_BLOCK * VC) {
        const int s = e / cw, c = e - s * cw;
        float v[VC];
        st_load<st_f32, VC>(staged + cl0 + (i64)s * g.C + c, v);
#pragma unroll
        for (int j = 0; j < VC; j++) tile[cl_row(c + j) + cl_col<VP>(s)] = v[j];
      }
    } else {
      for (int i = tid; i < cw * nq; i += CL_BLOCK) {
        const int c = i / nq, q = i - c * nq;
        const i64 at = pl0 + (i64)c * g.S + q * VP;
        float v[VP];
        st_load<st_f32, VP>(staged + at, v);
        if constexpr (MODE == 3) {
          const float sc = scale[c0 + c], sh = shift[c0 + c];
          float rm[VP];
          st_load<st_f32, VP>(direct + at, rm);
#pragma unroll
          for (int j = 0; j < VP; j++) v[j] = cl_bn_one(v[j], sc, sh, rm[j], true, relu);
        }
#pragma unroll
        for (int j = 0; j < VP; j++) tile[cl_row(c) + cl_col<VP>(q * VP + j)] = v[j];
      }
    }
    __syncthreads();
    if constexpr (SRC_CL) {        // y planar: staged is x, direct (MODE 1) the planar rem
      for (int i = tid; i < cw * nq; i += CL_BLOCK) {
        const int c = i / nq, q = i - c * nq;
        const i64 at = pl0 + (i64)c * g.S + q * VP;
        const float sc = scale[c0 + c], sh = shift[c0 + c];
        float rm[VP], o[VP];
        if constexpr (MODE == 1) st_load<st_f32, VP>(direct + at, rm);
#pragma unroll
        for (int j = 0; j < VP; j++)
          o[j] = cl_bn_one(tile[cl_row(c) + cl_col<VP>(q * VP + j)], sc, sh, MODE == 1 ? rm[j] : 0.f, MODE == 1, relu);
        st_store<st_f32, VP>(y + at, o);
      }
    } else {                       // y channels-last: staged is x (MODE 0), the planar rem beside a direct x (MODE 2), the result (MODE 3)
      for (int e = tid * VC; e < ne; e += CL_BLOCK * VC) {
        const int s = e / cw, c = e - s * cw;
        const i64 at = cl0 + (i64)s * g.C + c;
        float xv[VC], o[VC];
        if constexpr (MODE == 2) st_load<st_f32, VC>(direct + at, xv);
#pragma unroll
        for (int j = 0; j < VC; j++) {
          const float st = tile[cl_row(c + j) + cl_col<VP>(s)];
          if constexpr (MODE == 3) o[j] = st;
          else o[j] = cl_bn_one(MODE == 2 ? xv[j] : st, scale[c0 + c + j], shift[c0 + c + j], MODE == 2 ? st : 0.f, MODE == 2, relu);
        }
        st_store<st_f32, VC>(y + at, o);
      }
    }
    __syncthreads();               // the next tile overwrites the image
  }
}

// ---- cost volume ----------------------------------------------------------------------------------------------------------

constexpr int CV_TW = 64;                      // columns per tile
constexpr int CV_DB = 32;                      // disparities per tile
constexpr int CV_CB = 32;                      // channels (of C) per tile
constexpr int CV_LDX = CV_TW + 1;              // odd row strides: the channels-last lanes read down the channel axis
constexpr int CV_LDY = CV_TW + CV_DB - 1;
static_assert(CV_LDX % 2 == 1 && CV_LDY % 2 == 1, "odd row strides");

struct CvClGeom {
  int N, C, Dn, H, W;
  int nwb, ndb, ncb;   // column blocks, disparity chunks, channel blocks
  i64 ntiles;          // N * H * nwb * ndb * ncb
};

template <int V>
__global__ void __launch_bounds__(CL_BLOCK)
cost_volume_cl(const float *__restrict__ x, const float *__restrict__ y, float *__restrict__ cost, CvClGeom g)
{
  __shared__ float xs[CV_CB * CV_LDX];
  __shared__ float ys[CV_CB * CV_LDY];
  const int tid = (int)threadIdx.x;
  for (i64 t = blockIdx.x; t < g.ntiles; t += gridDim.x) {
    const int cb = (int)(t % g.ncb);
    i64 r = t / g.ncb;
    const int db = (int)(r % g.ndb); r /= g.ndb;
    const int wb = (int)(r % g.nwb); r /= g.nwb;
    const int h = (int)(r % g.H);
    const i64 n = r / g.H;
    const int c0 = cb * CV_CB, d0 = db * CV_DB, w0 = wb * CV_TW;
    const int cw = g.C - c0 < CV_CB ? g.C - c0 : CV_CB;
    const int dw = g.Dn - d0 < CV_DB ? g.Dn - d0 : CV_DB;
    const int tw = g.W - w0 < CV_TW ? g.W - w0 : CV_TW;
    const int yw = tw + dw - 1;                  // the y window: columns w0 - (d0 + dw - 1) .. w0 + tw - 1 - d0
    const int yw0 = w0 - (d0 + dw - 1);          // (columns left of the image are never selected: w >= d there means w - d >= 0)
    const i64 row0 = ((n * g.C + c0) * g.H + h) * g.W;      // (n, c0, h, 0) of x and y
    const i64 plane = (i64)g.H * g.W;
    for (int i = tid; i < cw * tw; i += CL_BLOCK) {
      const int c = i / tw, w = i - c * tw;
      xs[c * CV_LDX + w] = x[row0 + c * plane + w0 + w];
    }
    for (int i = tid; i < cw * yw; i += CL_BLOCK) {
      const int c = i / yw, u = i - c * yw;
      const int col = yw0 + u;
      ys[c * CV_LDY + u] = col >= 0 ? y[row0 + c * plane + col] : 0.f;
    }
    __syncthreads();
    const int nev = tw * cw / V;                 // lane items of one (d, half): cw % V == 0
    for (int i = tid; i < dw * 2 * nev; i += CL_BLOCK) {
      const int dh = i / nev, e = (i - dh * nev) * V;
      const int d = d0 + (dh >> 1), half = dh & 1;
      const int w = e / cw, c = e - w * cw;
      const int gw = w0 + w;
      const float *src = half ? ys + c * CV_LDY + (gw - d - yw0) : xs + c * CV_LDX + w;
      const int ld = half ? CV_LDY : CV_LDX;
      float v[V];
#pragma unroll
      for (int j = 0; j < V; j++) v[j] = gw >= d ? src[j * ld] : 0.f;
      st_store<st_f32, V>(cost + ((((n * g.Dn + d) * g.H + h) * g.W + gw) * 2 + half) * g.C + c0 + c, v);
    }
    __syncthreads();
  }
}

}  // namespace ga
