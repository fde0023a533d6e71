// mixed_kernels.h -- the streaming kernels that sit between a 16-bit convolution and an fp32 guided-aggregation op, for gfx950.
// Under torch.autocast MIOpen's convolutions read and write fp16 / bf16; SGA, LGA and the tails stay fp32.  These kernels read
// and write 16-bit STORAGE (ga_common.h: st_f16 / st_bf16, uint16_t patterns) and compute in fp32, so that no cast pass stands
// between a convolution and one of our ops.
//
// The contract (tests/mixed_cases.py): with 16-bit inputs a16, ...
//     op_mixed(a16, ...) == convert(op_fp32(upcast(a16), ...), out_type)            bit for bit, NaN positions equal
// where op_fp32 is the fp32 kernel of the same name: the up-cast is exact, the arithmetic is that kernel's own expression
// (bn_z and relu_keep_nan of bn_kernels.h, the summation order of l1norm_fwd), and the result is rounded ONCE on the store.
//
//   bn_affine_apply_mixed   y = relu?(fmaf(x, scale[c], shift[c]) [+ rem]) on [N, C, S]; x 16-bit, rem none | f32 | 16-bit,
//                           y 16-bit | f32; also x f32, rem none | f32, y 16-bit (behind an op autocast keeps in fp32).
//                           bn_affine_apply's grid and slice loop (BnGeom) with eight elements per lane.
//                           y may BE x where both have one width: a lane reads its eight elements before it writes them.
//                           A sibling of bn_affine_apply, not one template with it: folded into bn_apply_share's form its
//                           V = 8 instantiations need one more SGPR each (profiles/r24a_kernel_resources.txt).
//                           The TRAINING forms of the 16-bit site are bn_kernels.h's own kernels on 16-bit storage types.
//   cost_volume_fwd16       GetCostVolume on 2-byte elements: a copy with zeros, and 0x0000 is zero in both formats -- no type.
//                           Its scalar twin is misc_kernels.h's cost_volume_fwd<uint16_t>.
//   l1norm_fwd<KT, Tx>      misc_kernels.h's kernel itself, reading a 16-bit x; fp32 outputs.
//   cast_kernel             element-wise conversion between any two of f32 / f16 / bf16; the same type is a copy of patterns.
// Lanes along the fastest axis, 64-bit offsets, grid-stride.  V = 8: 16-byte requests (sizes a multiple of 8 and 16-byte
// aligned bases, decided on the host); V = 1: the scalar twin.
#pragma once
#include "bn_kernels.h"
#include "misc_kernels.h"

namespace ga {

constexpr int MX_V = 8;     // elements per lane of the vector paths: one 16-byte request of 16-bit storage

// x and y carry no __restrict__: y may BE x
template <typename Tx, typename Tr, typename Ty, int V>
__global__ void __launch_bounds__(BN_BLOCK)
bn_affine_apply_mixed(const typename Tx::T *x, const typename Tr::T *__restrict__ rem, const float *__restrict__ scale,
                      const float *__restrict__ shift, typename Ty::T *y, BnGeom g, int relu)
{
  const int c = (int)blockIdx.y, rs = (int)blockIdx.x % g.Rs, rn = (int)blockIdx.x / g.Rs;
  const i64 SV = g.S / V, stride = (i64)g.Rs * BN_BLOCK;
  const bool has_rem = rem != nullptr;
  const float sc = scale[c], sh = shift[c];
  for (int n = rn; n < g.N; n += g.Rn) {
    const i64 base = ((i64)n * g.C + c) * g.S;
    for (i64 i = (i64)rs * BN_BLOCK + threadIdx.x; i < SV; i += stride) {
      float a[V], r[V], o[V];
      st_load<Tx, V>(x + base + i * V, a);
      if (has_rem) st_load<Tr, V>(rem + base + i * V, r);
#pragma unroll
      for (int j = 0; j < V; j++) {
        const float z = bn_z(a[j], sc, sh, has_rem ? r[j] : 0.f, has_rem);
        o[j] = relu ? relu_keep_nan(z) : z;
      }
      st_store<Ty, V>(y + base + i * V, o);
    }
  }
}

// eight consecutive columns per lane (W % 8 == 0, x and cost 16-byte aligned): the left image is one 16-byte load, the shifted
// right-image samples are eight 2-byte loads at any alignment (the counterpart of cost_volume_fwd4), the store is 16 bytes
static __global__ void __launch_bounds__(256)
cost_volume_fwd16(const uint16_t *__restrict__ x, const uint16_t *__restrict__ y, uint16_t *__restrict__ cost,
                  int N, int C, int Dn, int H, int W)
{
  const int W8 = W >> 3;
  const i64 total = (i64)N * 2 * C * Dn * H * W8;
  const i64 stride = (i64)gridDim.x * blockDim.x;
  for (i64 q = (i64)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += stride) {
    const int w = (int)(q % W8) << 3;
    i64 r = q / W8;
    const int h = (int)(r % H); r /= H;
    const int i = (int)(r % Dn); r /= Dn;
    const int c = (int)(r % (2 * C));
    const int n = (int)(r / (2 * C));
    uint32_t e[8];
    if (c < C) {
      const u4 a = *reinterpret_cast<const u4 *>(x + (((i64)n * C + c) * H + h) * W + w);
      const uint32_t p[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
      for (int j = 0; j < 8; j++) e[j] = w + j < i ? 0u : (p[j >> 1] >> (16 * (j & 1))) & 0xffffu;
    } else {
      const uint16_t *yr = y + (((i64)n * C + (c - C)) * H + h) * W;
      const int s0 = w - i;                        // source column of the first element (may be negative)
      uint32_t t[8];
#pragma unroll
      for (int j = 0; j < 8; j++) t[j] = yr[s0 + j > 0 ? s0 + j : 0];
#pragma unroll
      for (int j = 0; j < 8; j++) e[j] = s0 + j >= 0 ? t[j] : 0u;
    }
    u4 v;
    v.x = e[0] | (e[1] << 16); v.y = e[2] | (e[3] << 16); v.z = e[4] | (e[5] << 16); v.w = e[6] | (e[7] << 16);
    *reinterpret_cast<u4 *>(cost + (q << 3)) = v;
  }
}

// dst[i] = convert(src[i]), i < n: groups of V first, then the n % V elements behind them one per lane
template <typename Ts, typename Td, int V>
__global__ void __launch_bounds__(256)
cast_kernel(const typename Ts::T *__restrict__ src, typename Td::T *__restrict__ dst, i64 n)
{
  const i64 groups = n / V, tail = n - groups * V;
  const i64 stride = (i64)gridDim.x * blockDim.x, first = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  for (i64 q = first; q < groups; q += stride) {
    float a[V];
    st_load<Ts, V>(src + q * V, a);
    st_store<Td, V>(dst + q * V, a);
  }
  if (V > 1 && first < tail) {
    float a[1];
    st_load<Ts, 1>(src + groups * V + first, a);
    st_store<Td, 1>(dst + groups * V + first, a);
  }
}

}  // namespace ga
