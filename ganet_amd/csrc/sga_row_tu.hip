// sga_row_tu.hip -- the horizontal scan kernels (forward and adjoint) in a translation unit of their own.
// Reason: compiler flags.  With hipcc's SLP vectoriser on, neighbouring scalar FMAs of the recurrence
// are packed into v_pk_fma_f32 and paid for with v_mov shuffles (12 per scan position in the forward scan,
// 0.098 -> 0.082 ms without it; the adjoint with its lane-uniform range tests spills 24 registers with it);
// the vertical scans in ganet_capi.hip are a few per cent faster WITH it.  A row kernel is bound by its
// instruction count per position -- scalar instructions included (profiles/r5d_*) -- so that is what is
// kept small here.  build.py compiles this file with -fno-slp-vectorize and links both objects into
// libganet_hip.so.
#include "ga_launch.h"

#ifndef GA_ROW_GD64
#define GA_ROW_GD64 1        // forward: depth axis over the whole wavefront for the models' depths
#endif
#ifndef GA_ROW_BWDG_GD64
#define GA_ROW_BWDG_GD64 1   // the same for the adjoint
#endif

namespace ga {

// The wave-wide kernels below take every D <= 72 before with_row_dpl sees it, so a 16-lane kernel with fewer than five
// disparities per lane (D <= 48) has a caller only in a build that switches them off or runs several rows per wavefront.
constexpr bool row16_fwd_reached(int dpl) { return dpl >= 5 || !GA_ROW_GD64 || ROW_LN_F != 1; }
constexpr bool row16_bwdg_reached(int dpl) { return dpl >= 5 || !GA_ROW_BWDG_GD64 || ROW_LN_B != 1; }

// D <= 72 with the depth axis over the whole wavefront: one disparity per lane up to 64, two up to 72.  f(int_c<P>, int_c<NP>):
// NP = staged pieces per lane = ceil(D_max / 8) of the range: the models' 33 / 48 / 65 get exactly what they need, the ranges in
// between share an instantiation (12 / 16 pieces for D <= 96 / 128 spill at these register caps: those depths keep the 16-lane kernels)
template <class F>
static bool with_row_gd64(int D, F &&f)
{
  if (D <= 40) f(int_c<1>{}, int_c<5>{});
  else if (D <= 48) f(int_c<1>{}, int_c<6>{});
  else if (D <= 64) f(int_c<1>{}, int_c<8>{});
  else if (D <= 72) f(int_c<2>{}, int_c<9>{});
  else return false;
  return true;
}

static RowGeom row_geom(int S, int D, int H, int W, int out_mode, int C, const float *scale, const float *shift)
{
  RowGeom geo;
  geo.D = D; geo.H = H; geo.W = W; geo.HW = (i64)H * W; geo.total_rows = S * H;
  geo.out_mode = out_mode; geo.C = C > 0 ? C : 1; geo.scale = scale; geo.shift = shift;
  return geo;
}

void launch_row_fwd(const float *x, const float *g, float *A, int S, int D, int H, int W, int dir, hipStream_t st,
                    int out_mode, int C, const float *scale, const float *shift)
{
  const RowGeom geo = row_geom(S, D, H, W, out_mode, C, scale, shift);
  const int dpl = row_dpl(D);
  const bool full = dpl > 0 && D % dpl == 0;     // lanes wholly inside / outside [0, D): leaner recurrence
  const size_t smem = row_smem_fwd(D);
  const dim3 grid((S * H + ROW_LN_F - 1) / ROW_LN_F), block(64);
  // `left` (3) visits w descending
#if GA_ROW_GD64
  if (ROW_LN_F == 1 && with_row_gd64(D, [&](auto P, auto NP) {
        with_flags([&](auto desc, auto fl) {
          if constexpr (decltype(fl)::value || decltype(P)::value > 1)      // (one disparity per lane is always full)
            GA_LAUNCH_SMEM((sga_row_fwd<decltype(P)::value, ROW_SBH_F, ROW_PAD_F, 1, decltype(desc)::value, decltype(fl)::value, 64, decltype(NP)::value>), grid, block, smem, st, x, g, A, geo);
        }, dir == 3, D % decltype(P)::value == 0);
      }))
    return;
#endif
  with_row_dpl(dpl, [&](auto P) {
    with_flags([&](auto desc, auto fl) {
      if constexpr (row16_fwd_reached(decltype(P)::value))
        GA_LAUNCH_SMEM((sga_row_fwd<decltype(P)::value, ROW_SBH_F, ROW_PAD_F, ROW_LN_F, decltype(desc)::value, decltype(fl)::value>), grid, block, smem, st, x, g, A, geo);
    }, dir == 3, full);
  });
}

void launch_row_bwdg(const float *g, const uint8_t *mask, const uint16_t *kp, const float *gout, float *G,
                     int S, int D, int H, int W, int dir, hipStream_t st)
{
  const RowGeom geo = row_geom(S, D, H, W, 0, 1, nullptr, nullptr);
  const int dpl = row_dpl(D);
  const size_t smem = row_smem_bwdg(D);
  const dim3 grid((S * H + ROW_LN_B - 1) / ROW_LN_B), block(64);
  // the adjoint of `right` (2) walks w downwards, of `left` (3) upwards.  Lanes wholly inside / outside [0, D): the leaner
  // recurrence of bwdg_step<FULL>, instantiated for the depths the models use (33 and 48 at three, 65 at five per lane)
  const bool full = dpl > 0 && D % dpl == 0;
#if GA_ROW_BWDG_GD64
  if (ROW_LN_B == 1 && with_row_gd64(D, [&](auto P, auto NP) {
        with_flags([&](auto desc, auto fl) {
          if constexpr (decltype(fl)::value || decltype(P)::value > 1)      // (one disparity per lane is always full)
            GA_LAUNCH_SMEM((sga_row_bwdg<decltype(P)::value, ROW_SBH_B, ROW_PAD_B, 1, decltype(desc)::value, decltype(fl)::value, 64, decltype(NP)::value>), grid, block, smem, st, g, mask, kp, gout, G, geo, dir);
        }, dir == 2, D % decltype(P)::value == 0);
      }))
    return;
#endif
  with_row_dpl(dpl, [&](auto P) {
    with_flags([&](auto desc, auto fl) {
      constexpr bool FL = decltype(fl)::value && (decltype(P)::value == 3 || decltype(P)::value == 5);
      if constexpr (row16_bwdg_reached(decltype(P)::value))
        GA_LAUNCH_SMEM((sga_row_bwdg<decltype(P)::value, ROW_SBH_B, ROW_PAD_B, ROW_LN_B, decltype(desc)::value, FL>), grid, block, smem, st, g, mask, kp, gout, G, geo, dir);
    }, dir == 2, full);
  });
}

}  // namespace ga
