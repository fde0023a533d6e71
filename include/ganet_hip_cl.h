/*
 * ganet_hip_cl.h -- C ABI of libganet_hip.so, additions to ABI v14 (GANET_ABI_VERSION stays 14; every entry of ganet_hip.h
 * is unchanged): the channels-last inference path (ganet_amd/csrc/cl_kernels.h).  The 3-D convolutions of the cost
 * aggregation compute in [N,D,H,W,C]; these entries let every site between two of them read and write that layout, and
 * change layout where a planar op (SGA, the tails) is the neighbour, without a pass of their own.
 *
 * The conventions are ganet_hip.h's: device pointers to dense fp32 buffers, `stream` a hipStream_t passed as void *, 0 or a
 * negative GANET_E_* with a message in ganet_last_error().  S = D*H*W (or H*W).  A layout code says how a [N,C,S] tensor
 * lies in memory:
 *   GANET_LAYOUT_PLANAR  [N,C,S] contiguous
 *   GANET_LAYOUT_CL      [N,S,C] contiguous (torch.channels_last_3d / channels_last)
 *
 * ganet_bn_apply_forward_cl: y = relu(scale[c] * x + shift[c] [+ rem]), ganet_bn_apply_forward's arithmetic through the same
 * device function.  The contract is EQUALITY of bits with ganet_bn_apply_forward of the same build on the permuted operands,
 * permuted back.  Compiled layout combinations (x, rem, y):
 *   cl,     none,   cl       a plain stream; y may alias x
 *   cl,     none,   planar   the site in front of a planar op
 *   planar, none,   cl       the site behind a planar op
 *   cl,     planar, cl       the residual tail; y may alias x
 *   cl,     planar, planar   the residual tail in front of a planar op
 *   planar, planar, cl       the residual tail behind a convolution that answered in planar
 * The transposing forms stage one operand through LDS; both global sides are coalesced, with 16-byte requests on the
 * channels-last side where C % 4 == 0 and on the planar side where S % 4 == 0 and the bases on that side are 16-byte
 * aligned, 4-byte requests otherwise.  Any C up to 65535, 64-bit element offsets, no atomics, no host synchronisation
 * (graph-capturable); nothing outside a tensor is read, every output element is written exactly once.
 *   GANET_E_INVALID      a NULL x / scale / shift / y, a non-positive size, a layout code other than the two, y == rem, y == x
 *                        where the two layouts differ
 *   GANET_E_UNSUPPORTED  all operands planar (that is ganet_bn_apply_forward's case); a channels-last rem; C > 65535
 *
 * ganet_cost_volume_forward_cl: x, y planar [N,C,H,W] -> cost [N,Dn,H,W,2C]:
 *   cost[n,d,h,w,c] = w >= d ? x[n,c,h,w] : 0,   cost[n,d,h,w,C+c] = w >= d ? y[n,c,h,w-d] : 0
 * -- the values of ganet_cost_volume_forward, permuted; copies of bits, the zeros +0.  Each (h, block of columns) tile of x
 * and y is transposed through LDS once per chunk of disparities.  16-byte stores where C % 4 == 0 and cost is 16-byte aligned.
 *   GANET_E_INVALID      a NULL pointer, a non-positive size, cost == x or cost == y
 * Replaces: models/GANet_deep.py:35-41, 270-277 and libs/GANet/modules/GANet.py:114-134 in an inference pass whose 3-D
 *           convolutions run on channels_last_3d tensors.
 */
#ifndef GANET_HIP_CL_H
#define GANET_HIP_CL_H

#include "ganet_hip.h"

#define GANET_LAYOUT_PLANAR 0
#define GANET_LAYOUT_CL 1

#ifdef __cplusplus
extern "C" {
#endif

int ganet_bn_apply_forward_cl(const float *x, const float *rem, const float *scale, const float *shift, float *y, int N, int C, int S, int relu, int x_layout, int rem_layout, int y_layout, void *stream);
int ganet_cost_volume_forward_cl(const float *x, const float *y, float *cost, int N, int C, int Dn, int H, int W, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* GANET_HIP_CL_H */
