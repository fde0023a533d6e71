// io_kernels.h -- the image front and back end around the model as streaming kernels for gfx950.
// Reference: predict.py:92-114 (load_data: per-channel `(r - np.mean(r)) / np.std(r)` on the six uint8 channels of a stereo pair,
// float64 temporaries, stored as float32), :75-90 (test_transform: pad to the bottom-right or centre-crop), :132-138 (un-pad,
// `(temp * 256).astype('uint16')`) and dataloader/dataset.py:48-92 (train_transform: the training crop with the left / right
// shift and the target filled with 1000).  The host form standardises in numpy and ships 3 x 4 bytes per pixel and image; here
// the uint8 images go up as they are (CP bytes per pixel) and three launches produce the model's fp32 input.
//
// Images: uint8 [H, W, CP], interleaved, CP = 3 | 4, the first three bytes of a pixel are its channels (a fourth is skipped).
// 64-bit offsets, no atomics.
//   io_stats       grid (R, 2): block (r, image) adds its share of the image's pixels into six integer sums (sum v and sum v^2
//                  per channel, unsigned long long: exact and independent of the order, so two runs are bit-identical by
//                  construction) and stores row (image, r) of the caller's workspace, IO_ROW words each.
//                  R = min(IO_MAX_ROWS, ceil(H W / IO_PIX_PER_BLOCK)).  Wide form: a lane takes 16 pixels as CP 16-byte requests
//                  (16-byte aligned base; the H W % 16 pixels of the tail byte by byte); the byte-wise twin takes any address.
//   io_apply       grid (B, 2): every block re-adds its image's R rows in index order, finishes the statistics in fp64, builds
//                  the 3 x 256 table of results in LDS (a channel has only 256 of them: the streaming loop does not divide) and
//                  streams its share of the output window.  TABLE = false is the direct form, the same expression per element:
//                  the same bits (tests), kept for the comparison on the device (scripts/bench_io.py).
//                  V = 4: 16-byte stores (Wc % 4 == 0, 16-byte aligned outputs); V = 1: the scalar twin.
//   io_window_f32  dst[Hc, Wc] = inside ? src[y + oy, x + ox] - sub : fill          (the training target, dataset.py:53-74)
//   io_disp_u16    out[h, w] = sat(trunc(disp[y + oy, x + ox] * scale))             (predict.py:134-138)
//
// Arithmetic (tests/io_ref64.py states it in Python integers and float64), per channel, N = H W <= 2^24, S1 = sum v, S2 = sum v^2:
//   mean = double(S1) / double(N)
//   std  = sqrt(double(N S2 - S1 S1) / (double(N) double(N)))      the numerator in 64-bit integers: N S2 < 2^24 2^24 2^16, exact
//                                                                  where sum v^2 / N - mean^2 in fp64 loses a small variance
//   out  = float32((double(v) - mean) / std)                       every fp64 operation rounded on its own
//   N S2 == S1 S1 (a constant channel): out = 0 everywhere         (the reference divides by zero there and returns NaN)
//   out[c, y, x] = pixel (y + oy, x + ox_image) of the image, 0 where that pixel lies outside; no byte outside the image is read
//   u16: p = disp * scale, one fp32 multiplication; p < 0 or NaN -> 0, p >= 65536 (+Inf) -> 65535, else truncation toward zero
//        (the reference's astype wraps or is undefined outside [0, 65536))
#pragma once
#include "ga_common.h"

#if defined(GA_HIPSIM)
#define IO_FP_STRICT
#else
#define IO_FP_STRICT _Pragma("clang fp contract(off)")
#endif

namespace ga {

typedef unsigned long long u64;

constexpr int IO_BLOCK = 256;             // threads per block
constexpr int IO_MAX_ROWS = 64;           // rows (blocks) per image at most
constexpr int IO_PIX_PER_BLOCK = 4096;    // pixels of one trip of a block in the wide form: IO_BLOCK lanes x 16 pixels
constexpr int IO_ROW = 8;                 // words per workspace row: S1[3], S2[3], two unused (64-byte rows)
constexpr int IO_MAX_BLOCKS = 256;        // blocks per image (apply) / per launch (window, u16) at most

struct IoImage {
  const uint8_t *left, *right;
  int H, W, CP;
  int R;               // rows per image
  int wide;            // bit i: image i takes the wide form of io_stats
};

struct IoWindow {
  float *left_out, *right_out;
  int Hc, Wc, oy, ox_left, ox_right;
};

// ---- statistics -------------------------------------------------------------------------------------------------------------

GA_DEV void io_add_pixel(const uint8_t *p, u64 (&s1)[3], u64 (&s2)[3])
{
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const unsigned v = p[c];
    s1[c] += v;
    s2[c] += v * v;
  }
}

// 16 pixels = CP 16-byte requests; the byte at position j of the 16 CP bytes belongs to channel j % CP (a compile-time index:
// the twelve partial sums stay in registers)
template <int CP> GA_DEV void io_add_16_pixels(const uint8_t *p, u64 (&s1)[3], u64 (&s2)[3])
{
  unsigned a1[3] = {0, 0, 0}, a2[3] = {0, 0, 0};      // 16 x 255^2 < 2^21
#pragma unroll
  for (int q = 0; q < CP; q++) {
    const uint4 w = *reinterpret_cast<const uint4 *>(p + 16 * q);
    const unsigned word[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const int c = (16 * q + j) % CP;
      if (c < 3) {
        const unsigned v = (word[j / 4] >> (8 * (j % 4))) & 255u;
        a1[c] += v;
        a2[c] += v * v;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 3; c++) {
    s1[c] += a1[c];
    s2[c] += a2[c];
  }
}

template <int CP> GA_DEV void io_stats_wide(const uint8_t *img, i64 N, int R, u64 (&s1)[3], u64 (&s2)[3])
{
  const i64 units = N / 16, stride = (i64)R * IO_BLOCK;
  for (i64 u = (i64)blockIdx.x * IO_BLOCK + threadIdx.x; u < units; u += stride) io_add_16_pixels<CP>(img + u * 16 * CP, s1, s2);
  if (blockIdx.x == 0) {                               // the tail: fewer than 16 pixels
    const i64 i = units * 16 + threadIdx.x;
    if (i < N) io_add_pixel(img + i * CP, s1, s2);
  }
}

GA_DEV void io_stats_bytes(const uint8_t *img, i64 N, int CP, int R, u64 (&s1)[3], u64 (&s2)[3])
{
  const i64 stride = (i64)R * IO_BLOCK;
  for (i64 i = (i64)blockIdx.x * IO_BLOCK + threadIdx.x; i < N; i += stride) io_add_pixel(img + i * CP, s1, s2);
}

__global__ void __launch_bounds__(IO_BLOCK)
io_stats(IoImage g, u64 *__restrict__ ws)
{
  __shared__ u64 red[6 * IO_BLOCK];
  const int image = (int)blockIdx.y, t = (int)threadIdx.x;
  const uint8_t *img = image ? g.right : g.left;
  const i64 N = (i64)g.H * g.W;
  u64 s1[3] = {0, 0, 0}, s2[3] = {0, 0, 0};
  if ((g.wide >> image) & 1) {
    if (g.CP == 3) io_stats_wide<3>(img, N, g.R, s1, s2);
    else io_stats_wide<4>(img, N, g.R, s1, s2);
  } else {
    io_stats_bytes(img, N, g.CP, g.R, s1, s2);
  }
#pragma unroll
  for (int c = 0; c < 3; c++) {
    red[c * IO_BLOCK + t] = s1[c];
    red[(3 + c) * IO_BLOCK + t] = s2[c];
  }
  __syncthreads();
  for (int s = IO_BLOCK / 2; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int k = 0; k < 6; k++) red[k * IO_BLOCK + t] += red[k * IO_BLOCK + t + s];
    }
    __syncthreads();
  }
  if (t < IO_ROW) ws[((i64)image * g.R + blockIdx.x) * IO_ROW + t] = t < 6 ? red[t * IO_BLOCK] : 0;
}

// ---- standardise + place ----------------------------------------------------------------------------------------------------

struct IoChannel {
  double mean, std;
  bool constant;
};

GA_DEV float io_entry(unsigned v, const IoChannel &ch)
{
  IO_FP_STRICT
  return ch.constant ? 0.f : (float)(((double)v - ch.mean) / ch.std);
}

// the image's six sums from its R <= IO_MAX_ROWS rows, in index order; `tot` is LDS, 6 words
GA_DEV void io_sum_rows(const u64 *__restrict__ ws, int image, int R, u64 *rows /* LDS, 6 * IO_MAX_ROWS */, u64 *tot)
{
  const int t = (int)threadIdx.x;
  for (int i = t; i < 6 * R; i += IO_BLOCK) rows[i] = ws[((i64)image * R + i / 6) * IO_ROW + i % 6];
  __syncthreads();
  if (t < 6) {
    u64 s = 0;
    for (int r = 0; r < R; r++) s += rows[6 * r + t];
    tot[t] = s;
  }
  __syncthreads();
}

GA_DEV IoChannel io_channel(u64 S1, u64 S2, u64 N)
{
  IO_FP_STRICT
  IoChannel ch;
  const u64 num = N * S2 - S1 * S1;                    // N <= 2^24: both products below 2^64; never negative (Cauchy-Schwarz)
  ch.constant = num == 0;
  ch.mean = (double)S1 / (double)N;
  ch.std = sqrt((double)num / ((double)N * (double)N));
  return ch;
}

template <int V, bool TABLE>
__global__ void __launch_bounds__(IO_BLOCK)
io_apply(IoImage g, IoWindow w, const u64 *__restrict__ ws)
{
  __shared__ u64 rows[6 * IO_MAX_ROWS];
  __shared__ u64 tot[6];
  __shared__ float tab[TABLE ? 3 * 256 : 1];
  const int image = (int)blockIdx.y, t = (int)threadIdx.x;
  const uint8_t *img = image ? g.right : g.left;
  float *out = image ? w.right_out : w.left_out;
  const int ox = image ? w.ox_right : w.ox_left;
  io_sum_rows(ws, image, g.R, rows, tot);
  IoChannel ch[3];
#pragma unroll
  for (int c = 0; c < 3; c++) ch[c] = io_channel(tot[c], tot[3 + c], (u64)g.H * (u64)g.W);
  if constexpr (TABLE) {
    static_assert(IO_BLOCK == 256, "one table entry per lane and channel");
#pragma unroll
    for (int c = 0; c < 3; c++) tab[c * 256 + t] = io_entry((unsigned)t, ch[c]);   // IO_BLOCK == 256: one value per lane
    __syncthreads();
  }
  const i64 plane = (i64)w.Hc * w.Wc, upr = w.Wc / V, units = (i64)w.Hc * upr, stride = (i64)gridDim.x * IO_BLOCK;
  for (i64 u = (i64)blockIdx.x * IO_BLOCK + t; u < units; u += stride) {
    const i64 y = u / upr, x = (u % upr) * V, sy = y + w.oy;
    float o[3][V];
#pragma unroll
    for (int j = 0; j < V; j++) {
      const i64 sx = x + j + ox;
      const bool inside = sy >= 0 && sy < g.H && sx >= 0 && sx < g.W;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        float r = 0.f;
        if (inside) {
          const unsigned v = img[(sy * g.W + sx) * g.CP + c];
          if constexpr (TABLE) r = tab[c * 256 + v];
          else r = io_entry(v, ch[c]);
        }
        o[c][j] = r;
      }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
      float *q = out + c * plane + y * w.Wc + x;
      if constexpr (V == 4) {
        f4 a; a.x = o[c][0]; a.y = o[c][1]; a.z = o[c][2]; a.w = o[c][3];
        *reinterpret_cast<f4 *>(q) = a;
      } else {
        *q = o[c][0];
      }
    }
  }
}

// ---- float window (the training target) -------------------------------------------------------------------------------------

template <int V>
__global__ void __launch_bounds__(IO_BLOCK)
io_window_f32(const float *__restrict__ src, float *__restrict__ dst, int H, int W, int Hc, int Wc, int oy, int ox, float sub,
              float fill)
{
  IO_FP_STRICT
  const i64 upr = Wc / V, units = (i64)Hc * upr, stride = (i64)gridDim.x * IO_BLOCK;
  for (i64 u = (i64)blockIdx.x * IO_BLOCK + threadIdx.x; u < units; u += stride) {
    const i64 y = u / upr, x = (u % upr) * V, sy = y + oy;
    float o[V];
#pragma unroll
    for (int j = 0; j < V; j++) {
      const i64 sx = x + j + ox;
      const bool inside = sy >= 0 && sy < H && sx >= 0 && sx < W;
      o[j] = inside ? src[sy * W + sx] - sub : fill;
    }
    float *q = dst + y * Wc + x;
    if constexpr (V == 4) {
      f4 a; a.x = o[0]; a.y = o[1]; a.z = o[2]; a.w = o[3];
      *reinterpret_cast<f4 *>(q) = a;
    } else {
      *q = o[0];
    }
  }
}

// ---- disparity to 16 bit ----------------------------------------------------------------------------------------------------

GA_DEV unsigned io_u16(float d, float scale)
{
  IO_FP_STRICT
  const float p = d * scale;
  if (!(p >= 0.f)) return 0u;               // below zero, NaN
  if (p >= 65536.f) return 65535u;          // +Inf included
  return (unsigned)p;                       // toward zero
}

// the [h, w] result as one run of h w values: V = 8 packs eight into a 16-byte store (16-byte aligned `out`), the h w % 8 of the
// tail one by one; V = 1 the scalar twin
template <int V>
__global__ void __launch_bounds__(IO_BLOCK)
io_disp_u16(const float *__restrict__ disp, uint16_t *__restrict__ out, int Wd, int h, int w, int oy, int ox, float scale)
{
  const i64 n = (i64)h * w, units = n / V, stride = (i64)gridDim.x * IO_BLOCK;
  const i64 first = (i64)blockIdx.x * IO_BLOCK + threadIdx.x;
  for (i64 u = first; u < units; u += stride) {
    unsigned r[V];
#pragma unroll
    for (int j = 0; j < V; j++) {
      const i64 i = u * V + j, y = i / w, x = i % w;
      r[j] = io_u16(disp[(y + oy) * Wd + x + ox], scale);
    }
    if constexpr (V == 8) {
      uint4 a;
      a.x = r[0] | (r[1] << 16); a.y = r[2] | (r[3] << 16); a.z = r[4] | (r[5] << 16); a.w = r[6] | (r[7] << 16);
      *reinterpret_cast<uint4 *>(out + u * 8) = a;
    } else {
      out[u] = (uint16_t)r[0];
    }
  }
  if constexpr (V == 8) {
    const i64 i = units * 8 + first;
    if (i < n) out[i] = (uint16_t)io_u16(disp[(i / w + oy) * Wd + i % w + ox], scale);
  }
}

}  // namespace ga
