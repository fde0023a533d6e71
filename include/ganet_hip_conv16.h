/*
 * ganet_hip_conv16.h -- C ABI of libganet_hip.so, additions to ABI v14 (GANET_ABI_VERSION stays 14; every entry of
 * ganet_hip.h is unchanged): the tails' conv32x1 = nn.Conv3d(C, 1, (3,3,3), (1,1,1), (1,1,1), bias=False)
 * (models/GANet_deep.py:212, 232) on a 16-bit x, so that torch.autocast keeps the streaming kernels of ganet_disp_conv_*
 * instead of the library's 16-bit one-column GEMM (ganet_amd/csrc/disp_conv_kernels.h, instantiated on a 16-bit storage type).
 *
 * The conventions are ganet_hip.h's: device pointers to contiguous buffers, `stream` a hipStream_t passed as void *, 0 or a
 * negative GANET_E_* with a message in ganet_last_error().  fp16 and bf16 values are uint16_t patterns; x_type / gx_type is
 * GANET_F16 or GANET_BF16.
 *
 *   forward          x 16-bit [N,C,D,H,W], weight fp32 [1,C,3,3,3] -> y fp32 [N,1,D,H,W]
 *   data gradient    grad_y fp32 [N,1,D,H,W], weight fp32 -> grad_x 16-bit [N,C,D,H,W]
 *   weight gradient  x 16-bit, grad_y fp32 -> workspace rows (fp32), then grad_weight fp32 [1,C,3,3,3]
 *
 * The contract is EQUALITY with the fp32 entries of the same build on the exactly up-cast input, bit for bit:
 *   ganet_disp_conv_forward_16(x16, w)            == ganet_disp_conv_forward(upcast(x16), w)
 *   ganet_disp_conv_backward_weight_16(x16, gy)   == ganet_disp_conv_backward_weight(upcast(x16), gy)
 *   ganet_disp_conv_backward_data_16(gy, w)       == convert(ganet_disp_conv_backward_data(gy, w), gx_type)
 * with `convert` of ganet_hip.h's mixed contract: round to nearest even, the sign of zero kept, overflow to +-inf, fp16
 * subnormals, every NaN the one quiet NaN 0x7E00 / 0x7FC0.  The sums are fp32 in the fp32 entries' FMA order over the fp32
 * entries' lane geometry; the data gradient is rounded once, on the store.  The weight is the fp32 parameter itself, never a
 * 16-bit copy of it.  No atomics, no host synchronisation (graph-capturable); two runs of the weight gradient give the same
 * bits.  Nothing outside a tensor is read, every output element is written exactly once, 64-bit element offsets.
 *
 * workspace: ganet_disp_conv_workspace(N, C, D, H, W) floats, as for the fp32 entry.
 * 8-byte requests for four 16-bit words (beside 16-byte requests of the fp32 operand) where W % 4 == 0, the 16-bit base is
 * 8-byte aligned and the fp32 bases are 16-byte aligned; 2-byte / 4-byte requests otherwise.
 * The argument checks and size refusals are the fp32 entries': NULL, non-positive sizes, an output that aliases an input:
 * GANET_E_INVALID; C > 64, sizes beyond the launch grid or the workspace's answer: GANET_E_UNSUPPORTED.  A type code other
 * than GANET_F16 / GANET_BF16 (GANET_F32 included: that is the fp32 entry's case): GANET_E_INVALID.
 * Replaces: under torch.autocast, models/GANet_deep.py:212, 232 (conv32x1 as a 16-bit convolution, the up-cast of its output
 *           in front of the fp32 tail) with their autograd backward.
 */
#ifndef GANET_HIP_CONV16_H
#define GANET_HIP_CONV16_H

#include "ganet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int ganet_disp_conv_forward_16(const void *x, const float *weight, float *y, int N, int C, int D, int H, int W, int x_type, void *stream);
int ganet_disp_conv_backward_data_16(const float *grad_y, const float *weight, void *grad_x, int N, int C, int D, int H, int W, int gx_type, void *stream);
int ganet_disp_conv_backward_weight_16(const void *x, const float *grad_y, float *workspace, float *grad_weight, int N, int C, int D, int H, int W, int x_type, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GANET_HIP_CONV16_H */
