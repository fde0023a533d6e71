/*
 * ganet_hip.h -- C ABI of libganet_hip.so: GA-Net's guided-aggregation hot path
 * (SGA, LGA, GetCostVolume, DisparityRegression) as hand-written HIP kernels for
 * AMD Instinct MI355X (gfx950 / CDNA4).
 *
 * This is the drop-in boundary for the reference's native layer: every entry
 * point below names the reference interface it replaces (paths relative to the
 * reference repository root).  Plain pointers and sizes only -- no torch types.
 *
 * Conventions
 *   - All pointers are DEVICE pointers to contiguous fp32 (or uint8 where stated)
 *     buffers owned by the caller; the library never allocates tensor storage.
 *   - Volumes are [N,C,D,H,W]; guidance [N,C,5,H,W] (taps w0..w4, L1-normalised by
 *     the caller as in models/GANet_deep.py:264-268); LGA input [B,D,H,W] with
 *     filters [B,3*(2r+1)^2,H,W] (B = N for the 4-D ops, N*C for the "3d" ops).
 *   - dir: 0 down, 1 up, 2 right, 3 left (the reference's mask values,
 *     libs/GANet/src/GANet_kernel.cu:964-994).
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream).
 *     Work is enqueued asynchronously; nothing here synchronises the device.
 *   - Return value: 0 on success, negative on error (GANET_E_*); a message is
 *     available from ganet_last_error() (thread-local).  The reference returns 1
 *     unconditionally and never checks the runtime (GANet_cuda.cpp:5-64).
 */
#ifndef GANET_HIP_H
#define GANET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GANET_OK 0
#define GANET_E_INVALID (-1)      /* null pointer, non-positive size, bad dir      */
#define GANET_E_UNSUPPORTED (-2)  /* shape outside the compiled kernel set         */
#define GANET_E_RUNTIME (-3)      /* HIP runtime / launch error                    */

#define GANET_ABI_VERSION 14      /* v14 = v13 + ganet_stereo_input_workspace / _stats / _apply, ganet_window_f32, ganet_disparity_to_u16 (image front and back end); v14 also holds ganet_up_softmin_regression_forward / _backward and ganet_disp_conv_workspace / _forward / _backward_data / _backward_weight (additions only: every earlier entry is unchanged) */
int ganet_abi_version(void);
const char *ganet_last_error(void);
/* 1 if this build runs the lockstep CPU emulator (tests only), 0 for the gfx950 build */
int ganet_is_simulator(void);

/* ---------------------------------------------------------------- SGA ------------ */

/* One directional volume A_dir = scan_dir(x, g).
 * Replaces: memcpy + sga_{down,up,right,left}_forward<<<>>>
 *           (libs/GANet/src/GANet_kernel.cu:66-127, 285-346, 507-565, 720-778). */
int ganet_sga_scan_forward(const float *x, const float *g, float *A,
                           int N, int C, int D, int H, int W, int dir, void *stream);

/* Fast-path forward used by ganet_amd's SgaFunction: the four directional volumes
 * are written to A_ws ([4][N*C*D*H*W] floats, caller-allocated; kept for backward),
 * out = element-wise max in reference order, mask = winning direction (uint8), and
 * kp ([4][N*C*H*W] uint16) = first-argmax over d of every directional volume.
 * Replaces: sga_kernel_forward (GANet_kernel.cu:935-998) incl. the three `Max`
 * launches (:23-36) and five device memcpys; kp is what MaxDepth (:50-64) recomputes
 * four times in the reference's backward. */
int ganet_sga_forward(const float *x, const float *g0, const float *g1, const float *g2,
                      const float *g3, float *A_ws, float *out, uint8_t *mask, uint16_t *kp,
                      int N, int C, int D, int H, int W, void *stream);

/* The steps of ganet_sga_forward / ganet_sga_backward as they run inside those calls: direction `dir`'s scan into its place in
 * the op's PRIVATE workspace (A_ws / G_ws: [4][N*C*D*H*W] floats; kp: the whole [4][N*C*H*W] array).  A_ws holds the four
 * directional volumes in the API layout.  G_ws is not in the API layout in general: ganet_sga_workspace_layout() returns 1 if
 * the two vertical directions' adjoint volumes are tiled for these dimensions (element (s, d, h, w) of G_ws[dir < 2] at
 * ((((s * W/16 + w/16) * H/4 + h/4) * D + d) * 4 + h%4) * 16 + w%16), 0 if everything has the API layout.
 * ganet_sga_backward_scan (above) always writes the API layout.
 * Replaces: the same reference code as ganet_sga_scan_forward / ganet_sga_backward_scan. */
int ganet_sga_scan_forward_ws(const float *x, const float *g, float *A_ws,
                              int N, int C, int D, int H, int W, int dir, void *stream);
int ganet_sga_backward_scan_ws(const float *g, const uint8_t *mask, const uint16_t *kp, const float *grad_out, float *G_ws,
                               int N, int C, int D, int H, int W, int dir, void *stream);
int ganet_sga_workspace_layout(int N, int C, int D, int H, int W);

/* The last step of ganet_sga_forward on its own: out / mask / kp from the four directional volumes in A_ws (same buffers, same
 * layouts).  ganet_sga_forward == 4 x ganet_sga_scan_forward_ws + this; exported so that a caller (bench.py) can time it in place.  A_ws as ganet_sga_scan_forward_ws leaves it.
 * Replaces: the three `Max` launches (GANet_kernel.cu:23-36, 964-994) and the four MaxDepth launches of the backward (:50-64). */
int ganet_sga_merge(const float *A_ws, float *out, uint8_t *mask, uint16_t *kp,
                    int N, int C, int D, int H, int W, void *stream);

/* Inference-only forward: out = relu(bn_scale[c] * max_dir A_dir + bn_shift[c]) (bn_scale = bn_shift = NULL:
 * plain max).  No mask / arg-max is produced; A_ws ([4][N*C*D*H*W]) is scratch and stays untouched when the scans can take
 * the running maximum themselves (the usual case: W % 4 == 0, D <= 208, 16-byte aligned buffers).
 * Replaces: sga_kernel_forward (GANet_kernel.cu:935-998) followed by the eval-mode BatchNorm3d + ReLU of
 * SGABlock.forward (models/GANet_deep.py:269-271: `x = self.SGA(...); x = self.bn_relu(x)`), with
 * bn_scale = weight / sqrt(running_var + eps), bn_shift = bias - running_mean * bn_scale. */
int ganet_sga_forward_infer(const float *x, const float *g0, const float *g1, const float *g2,
                            const float *g3, float *A_ws, float *out, const float *bn_scale,
                            const float *bn_shift, int N, int C, int D, int H, int W, void *stream);
/* How many volume-sized ([N*C*D*H*W] floats) scratch buffers ganet_sga_forward_infer needs behind A_ws for these
 * arguments: 0 (the scans take the running maximum themselves; A_ws may then be NULL) or 4.  Negative on error. */
int ganet_sga_forward_infer_scratch(const float *x, const float *g0, const float *g1, const float *g2,
                                    const float *g3, const float *out, int N, int C, int D, int H, int W);

/* Reverse-scan adjoint of one direction: G = [mask == dir] * grad_out propagated through the
 * recurrence with first-argmax routing (kp_dir: [N*C*H*W] uint16 of that direction).
 * Replaces: cudaMemset + get_temp_grad (:38-48) + the top_diff part of
 *           sga_*_data_backward (:144-181 & mirrors). */
int ganet_sga_backward_scan(const float *g, const uint8_t *mask, const uint16_t *kp_dir,
                            const float *grad_out, float *G,
                            int N, int C, int D, int H, int W, int dir, void *stream);

/* One direction of the backward pass: adjoint scan into G_ws ([N*C*D*H*W] scratch) followed by
 * the per-pixel gradient kernel.  grad_x: written (accumulate = 0) or accumulated into
 * (accumulate = 1); gw ([N,C,5,H,W]) is written.
 * Replaces: cudaMemset + get_temp_grad + MaxDepth + sga_*_data_backward (:129-208 & mirrors)
 *           + sga_*_weight_backward (:210-281 & mirrors). */
int ganet_sga_backward_dir(const float *x, const float *g, const float *A, const uint8_t *mask,
                           const uint16_t *kp_dir, const float *grad_out, float *G_ws,
                           float *grad_x, float *gw,
                           int N, int C, int D, int H, int W, int dir, int accumulate,
                           void *stream);

/* Fast-path backward: four adjoint scans into G_ws ([4][N*C*D*H*W] scratch) + ONE per-pixel
 * kernel for all gradients, from the volumes / mask / kp saved by ganet_sga_forward.
 * grad_x and gw0..gw3 are fully overwritten.
 * Replaces: sga_kernel_backward (GANet_kernel.cu:1000-1129). */
int ganet_sga_backward(const float *x, const float *g0, const float *g1, const float *g2,
                       const float *g3, const float *A_ws, const uint8_t *mask, const uint16_t *kp,
                       const float *grad_out, float *G_ws, float *grad_x, float *gw0, float *gw1,
                       float *gw2, float *gw3, int N, int C, int D, int H, int W, void *stream);

/* The last step of ganet_sga_backward on its own: every gradient from the four adjoint volumes in G_ws (written by
 * ganet_sga_backward_scan_ws, in the layout ganet_sga_workspace_layout reports for these dimensions -- NOT by
 * ganet_sga_backward_scan, whose G has the API layout) and the forward volumes in A_ws.  On 16-byte aligned volumes
 * ganet_sga_backward == 4 x ganet_sga_backward_scan_ws + this; ganet_sga_backward itself also accepts a contiguous gradient /
 * guidance at a 4-byte aligned address (it then keeps the API layout internally), the _ws entries return GANET_E_UNSUPPORTED
 * for that on a tiled shape.
 * Replaces: the bottom_diff part of sga_*_data_backward (:182-207 & mirrors) + sga_*_weight_backward (:210-281 & mirrors). */
int ganet_sga_backward_point(const float *x, const float *g0, const float *g1, const float *g2, const float *g3,
                             const float *A_ws, const float *G_ws, float *grad_x, float *gw0, float *gw1,
                             float *gw2, float *gw3, int N, int C, int D, int H, int W, void *stream);

/* Reference-compatible buffer contract, for callers that keep the reference's
 * libs/GANet/functions/GANet.py unchanged:
 *   sga_cuda_forward(input, g0..g3, temp_out, output, mask)      GANet_cuda.cpp:39-48
 *   sga_cuda_backward(input, g0..g3, temp_out, mask, max_idx, gradOutput, temp_grad,
 *                     gradInput, grad0..grad3)                    GANet_cuda.cpp:50-64
 * mask is float-valued; temp_out ends the forward holding A_left and is reused as
 * scratch by the backward (which recomputes the other three volumes); temp_grad and
 * max_idx are scratch (adjoint volume / per-pixel arg-max, as in the reference);
 * gradInput is ACCUMULATED into (the caller zero-fills it, functions/GANet.py:33);
 * grad0..3 are written. */
int ganet_sga_forward_compat(const float *x, const float *g0, const float *g1, const float *g2,
                             const float *g3, float *temp_out, float *out, float *mask_f32,
                             int N, int C, int D, int H, int W, void *stream);
int ganet_sga_backward_compat(const float *x, const float *g0, const float *g1, const float *g2,
                              const float *g3, float *temp_out, const float *mask_f32,
                              float *max_idx, const float *grad_out, float *temp_grad,
                              float *grad_x, float *gw0, float *gw1, float *gw2, float *gw3,
                              int N, int C, int D, int H, int W, void *stream);

/* ---------------------------------------------------------------- LGA ------------ */

/* One LGA pass, y fully overwritten.  radius in {1,2,3}.
 * Replaces: lga_cuda_forward / lga3d_cuda_forward (GANet_cuda.cpp:14-37) ->
 *           lga_filtering_forward (GANet_kernel.cu:1131-1175).  The reference
 *           accumulates into a zero-filled output; here the zero-fill is not needed. */
int ganet_lga_forward(const float *x, const float *f, float *y,
                      int B, int D, int H, int W, int radius, void *stream);

/* One LGA pass that also reduces its output over the disparity axis: snorm [B,H,W] = sum_d |y|, sdy [B,H,W] = sum_d d * y,
 * so that F.normalize(y, p=1, dim=1) followed by DisparityRegression (the end of DispAgg.forward, models/GANet_deep.py:246-247)
 * is sdy / max(snorm, 1e-12) -- a per-pixel finish instead of two more passes over the volume.  y may be NULL (inference:
 * the volume itself is not needed); with y given it is written as by ganet_lga_forward (training keeps it for the backward,
 * ganet_norm_disparity_regression_backward takes it together with out and snorm).  GANET_E_UNSUPPORTED where the fused kernel
 * does not apply (radius 3, planes of 2^28 pixels or more): run the two separate entries instead. */
int ganet_lga_forward_regress(const float *x, const float *f, float *y, float *snorm, float *sdy,
                              int B, int D, int H, int W, int radius, void *stream);

/* ABI v7.  One LGA pass (transposed = 0: as ganet_lga_forward) or its data-backward (transposed = 1: x is the output gradient,
 * y the input gradient, as the second half of ganet_lga_backward) on volumes in the PAIR-INTERLEAVED layout
 * [B][ceil(D/2)][H][W][2] -- planes 2m and 2m+1 of a pixel adjacent; for odd D the odd half of the last pair is zero (written
 * so by this entry when y is interleaved; required of x when x is interleaved).  x_paired / y_paired select the layout of
 * either side; at most one of them (neither: the API-layout pass or data-backward on its own).  The layout is for volumes that never cross the operator API: the
 * intermediate between the two passes of an LGA2 (functions/GANet.py:176-187) and its gradient -- a consumer stages a plane
 * pair with two 16-byte copies per lane instead of seven 4-byte ones, a producer stores a pair with one 8-byte store.
 * radius 2 only, W even, 16-byte aligned volumes; GANET_E_UNSUPPORTED otherwise (use the API-layout entries). */
int ganet_lga_apply_paired(const float *x, const float *f, float *y, int B, int D, int H, int W, int radius,
                           int transposed, int x_paired, int y_paired, void *stream);
/* The same with the per-pixel EDGE SUMS of the filters as a side channel, edge: [B][3][H][W] floats (caller-allocated, private to
 * the op): the centre coefficient of the spatially replaced taps and the in-range sums of the two outer depth slabs, which
 * depend on f only.  transposed == 0 (a forward pass): WRITTEN as a by-product (the pass gathers those taps anyway);
 * transposed == 1 (the data-backward of the same filters): READ, instead of gathering 50 - 75 own taps per pixel for them.
 * Lga2Function's forward fills it once, its two data-backward launches use it. */
int ganet_lga_apply_paired_edges(const float *x, const float *f, float *y, float *edge, int B, int D, int H, int W, int radius,
                                 int transposed, int x_paired, int y_paired, void *stream);

/* ABI v7.  The filter gradient of one LGA pass (the first half of ganet_lga_backward: lga_filter_backward,
 * GANet_kernel.cu:1177-1216) with x OR gy in the pair-interleaved layout (see ganet_lga_apply_paired; at most one of
 * x_paired / gy_paired, neither: the API layout); gf keeps the API layout and is written (accumulate_gf = 0) or accumulated
 * into.  radius 2 only, W even, 16-byte aligned volumes. */
int ganet_lga_filter_grad_paired(const float *x, const float *gy, float *gf, int B, int D, int H, int W, int radius,
                                 int accumulate_gf, int x_paired, int gy_paired, void *stream);

/* One LGA pass backward: gx fully overwritten; gf written (accumulate_gf = 0) or
 * accumulated into (accumulate_gf = 1, what chained LGA2/LGA3 rely on,
 * functions/GANet.py:197-199).  gx may alias x (the reference's chained
 * backward does); it must not alias gy.
 * Replaces: lga_cuda_backward / lga3d_cuda_backward (GANet_cuda.cpp:5-28) ->
 *           lga_filter_backward (:1177-1216) + cudaMemset + lga_data_backward
 *           (:1218-1269). */
int ganet_lga_backward(const float *x, const float *f, const float *gy, float *gx, float *gf,
                       int B, int D, int H, int W, int radius, int accumulate_gf, void *stream);

/* ------------------------------------------- GetCostVolume / DisparityRegression -- */

/* cost [N,2C,Dn,H,W] from x,y [N,C,H,W]; Dn = maxdisp + 1.
 * Replaces: GetCostVolume.forward (libs/GANet/modules/GANet.py:119-134) and its
 * autograd-derived backward. */
int ganet_cost_volume_forward(const float *x, const float *y, float *cost,
                              int N, int C, int Dn, int H, int W, void *stream);
int ganet_cost_volume_backward(const float *grad_cost, float *grad_x, float *grad_y,
                               int N, int C, int Dn, int H, int W, void *stream);

/* out [N,H,W] = sum_d d * x[N,Dn,H,W].
 * Replaces: DisparityRegression.forward (libs/GANet/modules/GANet.py:142-148). */
int ganet_disparity_regression_forward(const float *x, float *out,
                                       int N, int Dn, int H, int W, void *stream);
int ganet_disparity_regression_backward(const float *grad_out, float *grad_x,
                                        int N, int Dn, int H, int W, void *stream);

/* ------------------------------------------------- callers' normalisations ---- */

/* L1 normalisation over a strided channel axis, F.normalize(x, p=1, dim) = x / max(sum|x|, 1e-12).
 * x [N][G][C][K][H][W]  ->  y_g [N][C][K][H][W] for g < G (G <= 4; unused outputs may be NULL).
 * G = 4, K = 5 replaces SGABlock's torch.split + view + 4 x F.normalize(p=1, dim=2) of the guidance
 * (models/GANet_deep.py:263-268; ~16 stock kernels); G = C = 1, K = 3(2r+1)^2 replaces
 * F.normalize(g, p=1, dim=1) of the LGA filters (models/GANet_deep.py:235).
 * backward: grad_x [N][G][C][K][H][W] from x and the G gradients wrt y_g (autograd of the same ops). */
int ganet_l1_normalize_forward(const float *x, float *y0, float *y1, float *y2, float *y3,
                               int N, int G, int C, int K, int H, int W, void *stream);
int ganet_l1_normalize_backward(const float *x, const float *gy0, const float *gy1,
                                const float *gy2, const float *gy3, float *grad_x,
                                int N, int G, int C, int K, int H, int W, void *stream);

/* out [N,H,W] = sum_d d * x[N,Dn,H,W] / s,  s = snorm [N,H,W] = max(sum_d |x|, 1e-12).
 * Replaces: F.normalize(x, p=1, dim=1) followed by DisparityRegression at the end of DispAgg.forward
 * (models/GANet_deep.py:246-247): one pass over the volume instead of five.  backward needs x, out, snorm. */
int ganet_norm_disparity_regression_forward(const float *x, float *out, float *snorm,
                                            int N, int Dn, int H, int W, void *stream);
int ganet_norm_disparity_regression_backward(const float *x, const float *out, const float *snorm,
                                             const float *grad_out, float *grad_x,
                                             int N, int Dn, int H, int W, void *stream);

/* y = softmax over the Dn axis of -x, x [N,Dn,H,W]  (nn.Softmin(dim=1) between the two LGA calls of DispAgg.forward,
 * models/GANet_deep.py:244); backward from y and grad_y. */
int ganet_softmin_forward(const float *x, float *y, int N, int Dn, int H, int W, void *stream);
int ganet_softmin_backward(const float *y, const float *grad_y, float *grad_x,
                           int N, int Dn, int H, int W, void *stream);

/* out [N,H,W] = sum_d d * softmin_d(x), x [N,Dn,H,W]: Softmin(dim=1) followed by DisparityRegression as in Disp.forward
 * (models/GANet_deep.py:217-219) without materialising the probabilities; mx, ssum [N,H,W] (running max of -x and
 * the sum of exponentials) are kept for the backward, which recomputes them from x. */
int ganet_softmin_regression_forward(const float *x, float *out, float *mx, float *ssum,
                                     int N, int Dn, int H, int W, void *stream);
int ganet_softmin_regression_backward(const float *x, const float *out, const float *mx, const float *ssum,
                                      const float *grad_out, float *grad_x,
                                      int N, int Dn, int H, int W, void *stream);

/* y [S,Do,Ho,Wo] = F.interpolate(x [S,Di,Hi,Wi], size=[Do,Ho,Wo], mode='trilinear', align_corners=False) per slice
 * (S = N * C), and its adjoint.  Replaces: the up-sampling of the cost volume in Disp.forward / DispAgg.forward
 * (models/GANet_deep.py:212, 240), i.e. ATen's upsample_trilinear3d and -- the point -- upsample_trilinear3d_backward,
 * which scatters with eight atomicAdds per output element; the backward here is a gather per input voxel. */
int ganet_trilinear_upsample_forward(const float *x, float *y, int S, int Di, int Hi, int Wi,
                                     int Do, int Ho, int Wo, void *stream);
int ganet_trilinear_upsample_backward(const float *grad_y, float *grad_x, int S, int Di, int Hi, int Wi,
                                      int Do, int Ho, int Wo, void *stream);

/* Disp.forward behind its conv32x1 (models/GANet_deep.py:214-219) in one pass, without the up-sampled volume:
 *   v = F.interpolate(x [N,Di,Hi,Wi], size=[Do,Ho,Wo], mode='trilinear', align_corners=False),  out [N,Ho,Wo] = sum_od od *
 *   softmin_od(v).  Per axis the source index and weight are those of ganet_trilinear_upsample_forward (PyTorch's rule
 *   evaluated in float32), the association is ATen's (W, then H, then D).  mx, ssum [N,Ho,Wo] are kept for the backward,
 *   which recomputes v and the probabilities from x: it writes the depth-reduced gradient columns to gcol_ws [N,Di,Ho,Wo]
 *   (every element is written; the caller provides the memory, contents irrelevant) and gathers grad_x [N,Di,Hi,Wi] from
 *   them: deterministic, no atomics.  Any sizes (down-sampling included); Do < 2^24. */
int ganet_up_softmin_regression_forward(const float *x, float *out, float *mx, float *ssum,
                                        int N, int Di, int Hi, int Wi, int Do, int Ho, int Wo, void *stream);
int ganet_up_softmin_regression_backward(const float *x, const float *out, const float *mx, const float *ssum,
                                         const float *grad_out, float *gcol_ws /* [N,Di,Ho,Wo] */, float *grad_x,
                                         int N, int Di, int Hi, int Wi, int Do, int Ho, int Wo, void *stream);

/* The tails' conv32x1 = nn.Conv3d(C, 1, (3,3,3), (1,1,1), (1,1,1), bias=False) as streaming kernels (disp_conv_kernels.h): fp32,
 * x [N,C,D,H,W], y and grad_y [N,1,D,H,W], weight and grad_weight [1,C,3,3,3] as ATen holds them, all contiguous; stride 1,
 * padding 1, no dilation, no bias; [.] is zero outside the volume (predicated: nothing outside a tensor is read):
 *   forward          y[n,d,h,w]               = sum_c sum_(kd,kh,kw) weight[c,kd,kh,kw] [x[n,c,d+kd-1,h+kh-1,w+kw-1]]
 *   backward_data    grad_x[n,c,z,y,x]        = sum_(kd,kh,kw) weight[c,kd,kh,kw] [grad_y[n,z-kd+1,y-kh+1,x-kw+1]]
 *   backward_weight  grad_weight[c,kd,kh,kw]  = sum_(n,d,h,w) grad_y[n,d,h,w] [x[n,c,d+kd-1,h+kh-1,w+kw-1]]
 * backward_weight runs two launches: per-workgroup partial sums go to rows of `workspace` in a fixed order, a second launch
 * adds the rows in index order in fp64 and rounds once.  No atomics anywhere: two runs give identical bits.
 * workspace: ganet_disp_conv_workspace(N, C, D, H, W) floats, private to the call until it has run; contents irrelevant, every
 * element of it and of every output is written exactly once.  Outputs must not alias inputs.  No host synchronisation,
 * capturable.  16-byte requests where W % 4 == 0 and the volumes' bases are 16-byte aligned, 4-byte ones otherwise.
 * 64-bit element offsets.  NULL pointer, non-positive size: GANET_E_INVALID.  C > 64, more than 65535 * 8 planes, N > 65535, a
 * workspace of 2^31 elements or more: GANET_E_UNSUPPORTED.  A refused call launches nothing.
 * Replaces: self.conv32x1(x) in Disp.forward and DispAgg.forward (models/GANet_deep.py:212, 232) -- MIOpen's implicit GEMM
 *           with one output column, its transposes, and its weight gradient, which accumulates with atomics. */
int ganet_disp_conv_workspace(int N, int C, int D, int H, int W);
int ganet_disp_conv_forward(const float *x, const float *weight, float *y, int N, int C, int D, int H, int W, void *stream);
int ganet_disp_conv_backward_data(const float *grad_y, const float *weight, float *grad_x,
                                  int N, int C, int D, int H, int W, void *stream);
int ganet_disp_conv_backward_weight(const float *x, const float *grad_y, float *workspace, float *grad_weight,
                                    int N, int C, int D, int H, int W, void *stream);

/* The end of SGABlock.forward (models/GANet_deep.py:270-277): behind `conv_refine` (Conv3d + BatchNorm3d, no ReLU) the
 * block adds its input back and applies ReLU,  `x += rem; return relu(x)`.  One pass:
 *   y[n,c,d,h,w] = relu(bn_scale[c] * t + bn_shift[c] + rem)     t = the convolution's output, (bn_scale, bn_shift) = the
 *                  BatchNorm3d folded from its running statistics (eval mode);
 *   bn_scale == bn_shift == NULL:  y = relu(t + rem)             t = bn(conv(..)) as the framework computed it (training).
 * y may alias t (the reference adds in place too).  relu as ATen's: [v <= 0] ? 0 : v (a NaN passes).
 * Backward: g = [y <= 0] ? 0 : grad_y;  grad_rem = g;  grad_t = bn_scale[c] * g (bn_scale NULL: = g; grad_t NULL with
 * bn_scale NULL: not written -- both inputs take grad_rem).
 * Replaces: batch_norm (eval) + add_ + relu_ and their backward nodes -- 7 volume passes forward in stock PyTorch, 3 here. */
int ganet_residual_relu_forward(const float *t, const float *rem, const float *bn_scale, const float *bn_shift,
                                float *y, int N, int C, int D, int H, int W, void *stream);
int ganet_residual_relu_backward(const float *y, const float *grad_y, const float *bn_scale, float *grad_t,
                                 float *grad_rem, int N, int C, int D, int H, int W, void *stream);

/* ---------------------------------------------------------------- criterion ------ */

/* ABI v12.  The training criterion and the error read-out over up to three disparity maps p_k [N,H,W] (unused ones NULL)
 * against one target [N,H,W], in two launches forward and one backward, without a host round trip and without atomics
 * (bit-reproducible).  params: DEVICE array of 8 floats {hi, lo, w0, w1, w2, thresh, alpha, rate_thresh}.
 *   valid pixel  mask_mode 0: target < hi (train.py:100);  1: lo <= target && target <= hi (evaluation.py:199).  NaN: invalid.
 *   r = p - t    kind 0: smooth-L1 (beta = 1);  kind 1: MyLoss2(thresh, alpha) as the reference applies it -- three masked
 *                updates of one buffer in sequence, for the value and, separately, for its slope table
 *                (libs/GANet/functions/GANet.py:264-289).  Every fp32 operation is rounded on its own.
 *   loss [1]     = sum_k w_k * mean_valid rho_k(|r_k|)
 *   stats [1+3P] = count, then per map: mean rho, mean |r| (end-point error), fraction with |r| > rate_thresh
 *   g_k          = valid ? sign(r_k) * slope_k(|r_k|) * (float)(w_k * grad_loss / count) : +0;  grad_loss: DEVICE scalar,
 *                count: stats[0] of the forward.  A NULL g_k: that map is not wanted.
 * count == 0 gives loss 0, stats 0 and all-zero gradient maps -- deliberately not the NaN that the mean over an empty
 * selection is in stock PyTorch.  Invalid pixels are left out by a select: a NaN / inf prediction there harms nothing.
 * workspace: ganet_disparity_loss_workspace(N, H, W) doubles (the size for P = 3), private to the call until it has run.
 * N * H * W >= 2^24: GANET_E_UNSUPPORTED (counts are reported as floats).  Bad P / kind / mask_mode: GANET_E_INVALID.
 * Replaces: train.py:100-118 (mask, `d[mask]` gathers, F.smooth_l1_loss / MyLoss2 terms and their weighted sum) with its
 *           autograd backward and MyLoss2Function.backward, train.py:126 and evaluation.py:199-202 (error, rate). */
int ganet_disparity_loss_workspace(int N, int H, int W);
int ganet_disparity_loss_forward(const float *p0, const float *p1, const float *p2, const float *target,
                                 const float *params, double *workspace, float *loss, float *stats,
                                 int N, int H, int W, int P, int kind0, int kind1, int kind2, int mask_mode, void *stream);
int ganet_disparity_loss_backward(const float *p0, const float *p1, const float *p2, const float *target,
                                  const float *params, const float *stats, const float *grad_loss,
                                  float *g0, float *g1, float *g2,
                                  int N, int H, int W, int P, int kind0, int kind1, int kind2, int mask_mode, void *stream);

/* ---------------------------------------------------------------- batch norm ----- */

/* ABI v13.  Training-mode BatchNorm + optional residual + optional ReLU on fp32 [N, C, S] (S = D*H*W or H*W, contiguous
 * slices), two launches each way, no atomics, no host round trip; two runs are bit-identical.
 *   statistics   per channel over M = N*S values, sums in fp64: mean, biased var, invstd = 1/sqrt(var + eps); mean and invstd
 *                rounded to fp32 once (save_mean, save_invstd [C]);  scale = weight * invstd, shift = fmaf(-mean, scale, bias)
 *                (weight / bias NULL: 1 / 0)
 *   running      running_mean = (1-m) running_mean + m mean, running_var = (1-m) running_var + m var M/(M-1), in fp64 from the
 *                unrounded statistics, written exactly once per channel; both NULL: no update
 *   forward      z = fmaf(x, scale, shift) [+ rem],  y = relu ? (z <= 0 ? 0 : z) : z   (a NaN passes through)
 *   backward     g = relu && z <= 0 ? 0 : grad_y, the mask recomputed from x (and rem): y is never read;
 *                grad_bias = sum g, grad_weight = invstd * sum g (x - mean), grad_rem = g,
 *                grad_x = scale * (g - k1 - (x - mean) q), k1 = sum g / M, q = invstd^2 sum g (x - mean) / M.
 *                A NULL output is not computed.
 * momentum_bits / eps_bits: the two fp32 values as their bit patterns (the ABI's scalars are ints).  relu: 0 | 1.
 * workspace: ganet_bn_workspace(N, C, S) doubles, private to the call until it has run; forward and backward may share one.
 * y, grad_x and grad_rem must not alias an input.  16-byte requests where S % 4 == 0 and every base is 16-byte aligned.
 * M = 1, NULL x, non-positive sizes: GANET_E_INVALID.  C > 65535: GANET_E_UNSUPPORTED.  M up to 2^40 and beyond (64-bit offsets).
 * ganet_bn_apply_forward is the eval form: y = relu(scale[c] x + shift[c] [+ rem]) with the BatchNorm folded from its running
 * statistics into (scale, shift) [C]; here y may alias x.
 * Replaces: models/GANet_deep.py:35-41 (BasicConv.forward: `bn` and F.relu(inplace=True) behind the convolution) and
 *           :270-277 (SGABlock's tail: conv_refine's BatchNorm3d, `x += rem`, relu), with their autograd backward. */
int ganet_bn_workspace(int N, int C, int S);
int ganet_bn_train_forward(const float *x, const float *rem, const float *weight, const float *bias,
                           float *running_mean, float *running_var, double *workspace, float *y,
                           float *save_mean, float *save_invstd,
                           int N, int C, int S, int momentum_bits, int eps_bits, int relu, void *stream);
int ganet_bn_train_backward(const float *x, const float *rem, const float *grad_y, const float *weight, const float *bias,
                            const float *save_mean, const float *save_invstd, double *workspace,
                            float *grad_x, float *grad_rem, float *grad_weight, float *grad_bias,
                            int N, int C, int S, int relu, void *stream);
int ganet_bn_apply_forward(const float *x, const float *rem, const float *scale, const float *shift, float *y,
                           int N, int C, int S, int relu, void *stream);

/* ---------------------------------------------------------------- mixed precision - */

/* ABI v14 (additions).  Inference with 16-bit convolutions around fp32 guided aggregation: the streaming ops between a
 * convolution and a GA op on 16-bit STORAGE, fp32 arithmetic inside (ganet_amd/csrc/mixed_kernels.h).  fp16 and bf16 values
 * are uint16_t patterns; a *_type argument names the format of one buffer. */
#define GANET_F32 0
#define GANET_F16 1
#define GANET_BF16 2
/* The contract: with 16-bit inputs, op_mixed(a16, ..) == convert(op_fp32(upcast(a16), ..), out_type) bit for bit, where op_fp32
 * is ganet_bn_apply_forward / ganet_cost_volume_forward / ganet_l1_normalize_forward of the same build: the up-cast is exact,
 * the arithmetic is the fp32 kernel's expression, the result is rounded once.
 *   convert      32 -> 16 rounds to nearest even, keeps the sign of zero, overflows to +-inf, produces fp16 subnormals; every NaN
 *                becomes the one quiet NaN 0x7E00 (fp16) / 0x7FC0 (bf16).  16 -> 32 is exact.
 *   cast         dst[i] = convert(src[i]) for i < n = n_hi * 2^31 + n_lo (the ABI's scalars are ints; 0 <= n_lo), between any two
 *                of the three types; the same type is a copy of patterns.  dst must not alias src.
 *   bn apply     y = relu(scale[c] x + shift[c] [+ rem]) on [N, C, S] as ganet_bn_apply_forward; x fp16 | bf16; rem NULL, fp32 or
 *                x's format; y fp32 or x's format.  Also an fp32 x (rem NULL or fp32) with a 16-bit y: behind an op that autocast
 *                runs in fp32.  y may alias x where both have one width and never otherwise, and never rem.
 *   cost volume  ganet_cost_volume_forward on 2-byte elements: a copy of patterns with zeros (0x0000 is zero in both formats).
 *   l1 normalize ganet_l1_normalize_forward with an fp16 | bf16 x and fp32 outputs.
 * 16-byte requests (eight 16-bit elements) where the inner size is a multiple of 8 and the bases are 16-byte aligned, scalar
 * ones otherwise.  NULL, non-positive sizes, an unknown type code, a forbidden alias: GANET_E_INVALID.  A type combination that
 * is not compiled (fp32 x and y, an fp32 x with a 16-bit rem, two different 16-bit formats in one call): GANET_E_UNSUPPORTED. */
int ganet_cast(const void *src, void *dst, int n_hi, int n_lo, int src_type, int dst_type, void *stream);
int ganet_bn_apply_forward_mixed(const void *x, const void *rem, const float *scale, const float *shift, void *y,
                                 int N, int C, int S, int relu, int x_type, int rem_type, int y_type, void *stream);
int ganet_cost_volume_forward_16(const void *x, const void *y, void *cost, int N, int C, int Dn, int H, int W, void *stream);
int ganet_l1_normalize_forward_mixed(const void *x, float *y0, float *y1, float *y2, float *y3,
                                     int N, int G, int C, int K, int H, int W, int x_type, void *stream);

/* ABI v14 (additions).  Training under autocast: batch statistics on 16-bit storage and the backwards the inference entries
 * above left out (ganet_amd/csrc/bn_kernels.h on 16-bit storage types, mixed_train_kernels.h for the cost volume's adjoint).
 * fp32 / fp64 arithmetic on the exactly up-cast operands, one rounding on each 16-bit store.
 *   bn train     ganet_bn_train_forward / _backward with a 16-bit x: their arithmetic term for term, their two launches each way
 *                over the same rows (ganet_bn_workspace is reused), no atomics, two runs bit-identical.  Three combinations:
 *                    x 16-bit, rem NULL, y and grad_y x's format   (every BasicConv)
 *                    x 16-bit, rem NULL, y and grad_y fp32         (the BasicConv in front of an SGABlock)
 *                    x 16-bit, rem fp32, y and grad_y x's format   (the SGABlock tail)
 *                grad_x has x's format, grad_rem is fp32, the statistics, running buffers, grad_weight and grad_bias are fp32.
 *                y, grad_x and grad_rem must not alias an input (x is saved for the backward: no in-place form).  A NULL output
 *                is not computed; with neither grad_x nor grad_rem the second launch is one block per channel.
 *                The statistics are reductions whose lanes cover other elements than the fp32 entry's: they agree with it to
 *                rounding, and bit for bit where every partial sum is exact; y is the fp32 expression of the RETURNED statistics,
 *                rounded once.
 *   cost volume  ganet_cost_volume_backward on fp16 | bf16 grad_cost, grad_x and grad_y (`type` names the one format): fp32 sums
 *                over the disparity ascending, == convert(ganet_cost_volume_backward(upcast(grad_cost))) bit for bit.
 *   l1 normalize ganet_l1_normalize_backward with an fp16 | bf16 x, fp32 incoming gradients and a grad_x of x's format:
 *                == convert(ganet_l1_normalize_backward(upcast(x), ..)) bit for bit.
 * 16-byte requests where the inner size is a multiple of 8 and the bases are 16-byte aligned, scalar ones otherwise.  NULL,
 * non-positive sizes, M = N*S = 1, an unknown type code, a forbidden alias: GANET_E_INVALID.  A combination that is not compiled
 * (an fp32 x, a 16-bit rem, a residual with an fp32 y, two different 16-bit formats in one call): GANET_E_UNSUPPORTED.
 * Replaces: under torch.autocast, models/GANet_deep.py:35-41 and :270-277 (BatchNorm, `x += rem`, relu behind a 16-bit
 *           convolution, with their autograd backward and the casts around them), libs/GANet/modules/GANet.py:114-134
 *           (GetCostVolume's backward) and the backward of models/GANet_deep.py:263-268 / :235 (F.normalize of the guidance
 *           and of the LGA filters). */
int ganet_bn_train_forward_mixed(const void *x, const float *rem, const float *weight, const float *bias,
                                 float *running_mean, float *running_var, double *workspace, void *y,
                                 float *save_mean, float *save_invstd, int N, int C, int S, int momentum_bits, int eps_bits,
                                 int relu, int x_type, int rem_type, int y_type, void *stream);
int ganet_bn_train_backward_mixed(const void *x, const float *rem, const void *grad_y, const float *weight, const float *bias,
                                  const float *save_mean, const float *save_invstd, double *workspace,
                                  void *grad_x, float *grad_rem, float *grad_weight, float *grad_bias,
                                  int N, int C, int S, int relu, int x_type, int rem_type, int gy_type, void *stream);
int ganet_cost_volume_backward_16(const void *grad_cost, void *grad_x, void *grad_y, int N, int C, int Dn, int H, int W,
                                  int type, void *stream);
int ganet_l1_normalize_backward_mixed(const void *x, const float *gy0, const float *gy1, const float *gy2, const float *gy3,
                                      void *grad_x, int N, int G, int C, int K, int H, int W, int x_type, void *stream);

/* ---------------------------------------------------------------- image I/O ------ */

/* ABI v14.  The two ends around the model: a stereo pair of uint8 images becomes the model's standardised fp32 input, the
 * disparity map becomes the 16-bit image the reference saves (ganet_amd/csrc/io_kernels.h; tests/io_ref64.py states the
 * arithmetic in Python integers and float64).
 *
 * Images: uint8 [H, W, CP], interleaved, CP = 3 | 4; the first three bytes of a pixel are its channels.  N = H W <= 2^24.
 *   statistics   per image and channel S1 = sum v, S2 = sum v^2 in 64-bit integers (exact, order-independent: two runs are
 *                bit-identical), one workspace row per block, plain stores, no atomics
 *   apply        mean = double(S1) / double(N), std = sqrt(double(N S2 - S1 S1) / (double(N) double(N))), the numerator in
 *                64-bit integers; out = float32((double(v) - mean) / std), every fp64 operation rounded on its own.
 *                DEVIATION: a constant channel (N S2 == S1 S1) gives 0 everywhere; the reference divides by zero and
 *                returns NaN (Inf for nothing: v - mean is 0 there).
 *                left_out / right_out: fp32 [3, Hc, Wc] each (two pointers: they may be slices of batch tensors);
 *                out[c, y, x] = channel c of pixel (y + oy, x + ox_left) of the left image, resp. (y + oy, x + ox_right) of
 *                the right one, 0 where that pixel lies outside the image.  No byte outside the images is read.
 *                form: 0 the 3 x 256 table of results built once per block (a channel has only 256), 1 the same expression per
 *                element (same bits; kept for measurement).
 * workspace: ganet_stereo_input_workspace(H, W, CP) 8-byte words, private to the pair of calls until both have run.
 * _stats takes 16-byte requests from an image whose base is 16-byte aligned and single bytes from any other address; _apply
 * stores 16 bytes where Wc % 4 == 0 and both outputs are 16-byte aligned.
 * CP other than 3 | 4, H W > 2^24, a NULL pointer, non-positive sizes: GANET_E_INVALID.
 * Replaces: predict.py:92-114 (load_data: `(r - np.mean(r)) / np.std(r)` per channel, float64 temporaries, float32 result) and
 *           :75-90 (test_transform: oy = H - Hc, ox = W - Wc pads to the bottom-right, int((W - Wc) / 2) centre-crops);
 *           dataloader/dataset.py:64-92 (train_transform: the random crop, the left image shifted by shift_x). */
int ganet_stereo_input_workspace(int H, int W, int CP);
int ganet_stereo_input_stats(const uint8_t *left, const uint8_t *right, uint64_t *workspace,
                             int H, int W, int CP, void *stream);
int ganet_stereo_input_apply(const uint8_t *left, const uint8_t *right, const uint64_t *workspace,
                             float *left_out, float *right_out, int H, int W, int CP, int Hc, int Wc,
                             int oy, int ox_left, int ox_right, int form, void *stream);

/* dst[Hc, Wc] = inside ? src[y + oy, x + ox] - sub : fill on fp32 maps, src [H, W]; sub_bits / fill_bits: the two fp32 values
 * as their bit patterns.  dst must not alias src.
 * Replaces: dataloader/dataset.py:53-74 (train_transform: the target padded with 1000, cropped, `target - shift_x`) and
 *           :100-104 (test_transform's padded target). */
int ganet_window_f32(const float *src, float *dst, int H, int W, int Hc, int Wc, int oy, int ox,
                     int sub_bits, int fill_bits, void *stream);

/* out[h, w] (uint16, contiguous) = sat(trunc(disp[y + oy, x + ox] * scale)), disp fp32 [Hd, Wd]; the window must lie inside
 * the map.  The product is one fp32 multiplication, truncation is toward zero.
 * DEVIATION: values below 0 and NaN give 0, values >= 65536 and +Inf give 65535; the reference's astype('uint16') wraps or is
 * undefined there.  16-byte stores where `out` is 16-byte aligned.
 * Replaces: predict.py:132-138 (un-pad with oy = Hd - h, ox = Wd - w, `(temp * 256).astype('uint16')`). */
int ganet_disparity_to_u16(const float *disp, uint16_t *out, int Hd, int Wd, int h, int w, int oy, int ox,
                           int scale_bits, void *stream);

/* ---------------------------------------------------------------- diagnostics ---- */

/* Runs a 64-lane probe of every DPP pattern the kernels rely on and compares with
 * the documented lane maps.  scratch: device buffer of >= 8*64 ints.  host_out
 * (host memory, >= 8*64 ints) receives the raw lane values.  Synchronises `stream`.
 * Returns 0 if all patterns match. */
int ganet_selftest_dpp(int *scratch_dev, int *host_out, void *stream);
/* The same for the whole-wavefront patterns of the 64-lanes-per-scanline scans (wave_shl:1, wave_shr:1, the wave-wide
 * maximum and sum); scratch / host_out: >= 4*64 ints. */
int ganet_selftest_dpp_wave(int *scratch_dev, int *host_out, void *stream);

/* Knobs (also read from the environment at first use).  One default path per operator plus its general fallback; the knobs
 * exist so that tests can reach the fallbacks and the forced modes:
 *   GANET_SGA_ROWWAVE / GANET_SGA_COLBLOCK = 0|1  LDS-staged row-per-wave / column-block scans (default 1; 0: the 16-lane
 *                         segment kernels, which are also the fallback for W % 4 != 0 and D > 208)
 *   GANET_SGA_WIDE_SCAN=0|1|2  scans with the whole wavefront on one scanline: never | for inputs with few scanlines and for
 *                         D > 272 (default) | whenever D > 48 (tests).  D up to 1088
 *   GANET_SGA_WIDE_COL=0|1|2  vertical scans on LDS-staged column blocks with one wavefront per column (1,024-thread blocks,
 *                         D <= 192): never | for inputs with few column blocks and D >= 96 (default; measured on
 *                         [1,1,192,240,624]: forward 0.33 -> 0.21 ms, adjoint 0.52 -> 0.40) | whenever the kernel applies (tests)
 *   GANET_SGA_TILED = 0|1 ganet_sga_backward's private workspace: the vertical directions' adjoint volumes G_down / G_up in the API
 *                         layout | tiled [slice][W/16][H/4][D][4][16] where W % 16 == 0, H % 4 == 0 and the 16-column kernels run
 *                         (default; whole step -1.1 %; see ganet_sga_workspace_layout)
 *   GANET_LGA_WAVE=0|1|2  LGA kernel family (radius <= 2): 256-thread tiles (any radius; the general fallback) | wave-autonomous
 *                         plane-pair kernels, LDS-DMA staging, FMAs packed along plane pairs, one ring per wave on 32 x 2 pixel
 *                         tiles | the same with the forward / data-backward kernels on ONE ring per 256-thread workgroup (32 x 8
 *                         tiles: the halo'd tile staged once for four waves, 12 rows fetched for 8 instead of 24; a barrier per
 *                         plane pair).  Default 2 (whole step -1.4 ... -3.5 % in five A/Bs on four boxes against 1, profiles/r8*_ab_step*).
 *                         The filter gradient: under 2, where its x is pair-interleaved (an LGA2's second pass), the 75 taps of a 32 x 2
 *                         tile are split over a wave pair that shares the x and gy rings (five waves per SIMD instead of three: its launch
 *                         -7 %, profiles/r9k_*, r9l_*); with an API-layout x one ring per wave in both (the wave-pair form lost there,
 *                         the four-wave ring form of round 5 was no gain: removed)
 *   GANET_LGA_SEGS = n    depth segments per tile for the plane-pair forward / data-backward (0 = automatic)
 *   GANET_LGA_MIX=0|1|n   the same kernels with a MIXED item list: whole tiles first (a whole number per SIMD), the remaining
 *                         tiles cut into depth segments, at most one segment per SIMD -- the waves of a SIMD share one VALU, so
 *                         a pass lasts as long as the SIMD with the most tiles (3 of 2.34 on average at 240x624).  Default 1
 *                         (measured: forward pass 0.103 -> 0.0955 ms); n > 1: n SIMDs assumed (tests)
 * Read by ganet_amd.functions.GANet, not by this library: GANET_LGA_PAIRED=0 keeps the intermediate volume of a two-pass
 * chain in the API layout instead of pair-interleaved (ganet_lga_apply_paired; default on, measured -7 % on Lga2Function
 * fwd+bwd); GANET_SGA_SAVE=recompute selects the reference's memory profile.  GANET_TRACE_DISPATCH=1 prints which LGA kernel
 * a call took.  Unknown names -> GANET_E_INVALID. */
int ganet_set_option(const char *name, int value);
/* current value of a library option (>= 0), GANET_E_INVALID for an unknown name */
int ganet_get_option(const char *name);

#ifdef __cplusplus
}
#endif
#endif /* GANET_HIP_H */
