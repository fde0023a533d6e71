// ganet_capi.hip -- host side of libganet_hip.so: the C ABI declared in
// include/ganet_hip.h, argument validation, kernel selection and launch.
// Compiled by hipcc for gfx950 (product) and by g++ -DGA_HIPSIM (CPU test emulator).
#include "ga_common.h"
#include "bn_kernels.h"
#include "io_kernels.h"
#include "lga_kernels.h"
#include "loss_kernels.h"
#include "misc_kernels.h"
#include "disp_tail_kernels.h"
#include "disp_conv_kernels.h"
#include "cl_kernels.h"
#include "mixed_kernels.h"
#include "mixed_train_kernels.h"
#include "sga_kernels.h"
#include "sga_row_kernels.h"
#include "sga_col_kernels.h"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>

#include "../../include/ganet_hip.h"
#include "../../include/ganet_hip_conv16.h"
#include "../../include/ganet_hip_cl.h"

#include "ga_launch.h"

namespace {

using namespace ga;

thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...)
{
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int check_launch(const char *what)
{
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(GANET_E_RUNTIME, "%s: %s", what, hipGetErrorString(e));
  return GANET_OK;
}

// the argument checks the entries share: one helper per message form
template <class... P> int check_ptrs(const char *who, const P *...p)
{
  return ((p == nullptr) || ...) ? fail(GANET_E_INVALID, "%s: null pointer", who) : GANET_OK;
}
template <class... I> int check_positive(const char *who, I... n)
{
  return ((n <= 0) || ...) ? fail(GANET_E_INVALID, "%s: non-positive size", who) : GANET_OK;
}
int check_ncdhw(const char *who, int N, int C, int D, int H, int W)
{
  if (N > 0 && C > 0 && D > 0 && H > 0 && W > 0) return GANET_OK;
  return fail(GANET_E_INVALID, "%s: non-positive size N=%d C=%d D=%d H=%d W=%d", who, N, C, D, H, W);
}
int check_dir(const char *who, int dir) { return dir < 0 || dir > 3 ? fail(GANET_E_INVALID, "%s: dir %d", who, dir) : GANET_OK; }

#define GA_TRY(expr)                         \
  do {                                       \
    const int rc_ = (expr);                  \
    if (rc_ != GANET_OK) return rc_;         \
  } while (0)

#define GA_HIP(expr)                                                                   \
  do {                                                                                 \
    const hipError_t e_ = (expr);                                                      \
    if (e_ != hipSuccess) return fail(GANET_E_RUNTIME, #expr ": %s", hipGetErrorString(e_)); \
  } while (0)

// ---- options ------------------------------------------------------------------
// One default path per operator (measured on MI355X, profiles/) plus its general fallback; the knobs exist so that tests can
// reach the fallbacks and the forced modes.  Fields are atomics: ganet_set_option() may race with launches on other threads
// (each launcher reads a field once).
#ifndef GA_SGA_TILED_DEFAULT
#define GA_SGA_TILED_DEFAULT 1
#endif
struct Options {
  std::atomic<int> sga_tiled{GA_SGA_TILED_DEFAULT};  // SGA backward: the vertical directions' adjoint volumes G_down / G_up in the private tiled layout
                                    // of sga_col_kernels.h (1; where W % 16 == 0 and H % 4 == 0) or in the API layout (0)
  std::atomic<int> lga_wave{2};     // LGA kernel family (radius <= 2): 2 plane-pair kernels, the forward / data-backward with ONE x ring per 256-thread workgroup on 32 x 8 tiles and a barrier per plane pair (lga_apply_pp_w*; default: whole step -1.4 ... -3.5 % over five boxes against 1, profiles/r8*_ab_step*; where W % 4 != 0 on API-layout x: as 1), 1 plane-pair kernels with one ring per wave on 32 x 2 tiles (lga_apply_pp_* / lga_filter_grad_pp_*).  The filter gradient under 2: where x is pair-interleaved (the second pass of an LGA2) the taps of a 32 x 2 tile are split over a WAVE PAIR that shares the rings (lga_filter_grad_pair_xp: five waves per SIMD instead of three, the launch -7 %, round 6 profiles/r9k_*, r9l_*); with an API-layout x it runs the one-wave kernel in both settings (its wave-pair form lost +3 %, its four-wave ring form of round 5 was no gain: both removed).  0 the 256-thread tile kernels (any radius; the general fallback)
  std::atomic<int> lga_mix{1};      // plane-pair forward / data-backward: mixed item list (whole tiles + segments of the rest); 0 off, 1 on (measured: forward pass 0.103 -> 0.0955 ms, profiles/r3a_*), n > 1: n SIMDs assumed (tests)
  std::atomic<int> lga_segs{0};     // depth segments per tile for the plane-pair forward / data-backward (0 = automatic)
  std::atomic<int> wide_col{1};     // vertical scans: LDS-staged column blocks with one wavefront per column (1,024-thread blocks): 1 for inputs with few column blocks and D >= 96 (measured on [1,1,192,240,624]: forward 0.33 -> 0.21 ms, adjoint 0.52 -> 0.40, profiles/r3a_check_wide_col.txt), 0 never, 2 whenever the kernel applies (tests)
  std::atomic<int> wide_scan{1};    // SGA scans with the whole wavefront on one scanline: 1 for inputs with few scanlines (and D > 272), 0 never, 2 whenever D > 48 (tests)
  std::atomic<int> rowwave{1};      // horizontal scans: one wavefront per row, LDS-staged (sga_row_kernels.h); 0 = segment kernels (the fallback)
  std::atomic<int> colblock{1};     // vertical scans: 16-column blocks, LDS-staged (sga_col_kernels.h); 0 = segment kernels (the fallback)
};
Options g_opt;
std::once_flag g_opt_once;

// the one list of options: ganet_set_option, ganet_get_option and the environment go through it, and `norm` is the one place a
// value is normalised (GANET_LGA_WAVE=-1 from the environment used to be stored as is, truthy, and reported as -1)
int norm_tri(int v) { return v < 0 ? 0 : (v > 2 ? 2 : v); }
int norm_flag(int v) { return v ? 1 : 0; }
int norm_count(int v) { return v < 0 ? 0 : v; }
const struct OptionDesc {
  const char *name;
  std::atomic<int> Options::*field;
  int (*norm)(int);
} g_option_table[] = {
    {"GANET_LGA_WAVE", &Options::lga_wave, norm_tri},
    {"GANET_SGA_TILED", &Options::sga_tiled, norm_flag},
    {"GANET_LGA_MIX", &Options::lga_mix, norm_count},      // 1: S = SIMDs of the device; n > 1: S = n (tests)
    {"GANET_LGA_SEGS", &Options::lga_segs, norm_count},
    {"GANET_SGA_WIDE_SCAN", &Options::wide_scan, norm_tri},
    {"GANET_SGA_WIDE_COL", &Options::wide_col, norm_tri},
    {"GANET_SGA_ROWWAVE", &Options::rowwave, norm_flag},
    {"GANET_SGA_COLBLOCK", &Options::colblock, norm_flag},
};

const OptionDesc *find_option(const char *name)
{
  for (const OptionDesc &o : g_option_table)
    if (!strcmp(name, o.name)) return &o;
  return nullptr;
}

bool store_option(const char *name, int value)
{
  const OptionDesc *o = find_option(name);
  if (o) g_opt.*o->field = o->norm(value);
  return o != nullptr;
}

void load_env_options()
{
  for (const OptionDesc &o : g_option_table) {
    const char *v = getenv(o.name);
    if (v && *v) store_option(o.name, atoi(v));
  }
}
const Options &opts()
{
  std::call_once(g_opt_once, load_env_options);
  return g_opt;
}

// ---- SGA kernel selection -----------------------------------------------------------
// (lanes per scanline GD, disparities per lane DPL) pairs compiled in.
// GD = 64: the whole wavefront owns one scanline (D up to 1,088; 4x the waves of GD = 16 for inputs with few scanlines)
#define GA_SGA_PAIRS(X) \
  X(16, 1) X(16, 2) X(16, 3) X(16, 5) X(16, 9) X(16, 13) X(16, 17) \
  X(64, 3) X(64, 5) X(64, 9) X(64, 17)

constexpr int fwd_sb(int dpl) { return dpl <= 3 ? 8 : dpl <= 5 ? 4 : dpl <= 9 ? 2 : 1; }
constexpr int fwd_nv(int dpl) { return dpl <= 5 ? 2 : 1; }
constexpr int bwd_sb(int dpl) { return dpl <= 3 ? 8 : dpl <= 5 ? 4 : dpl <= 9 ? 2 : 1; }
constexpr int bwd_nv(int dpl) { return dpl <= 5 ? 2 : 1; }

bool pick_pair(int D, int want_gd, int *gd, int *dpl)
{
  int best_gd = 0, best_dpl = 0;
#define X(G, P)                                                                    \
  if ((G) == want_gd && (G) * (P) >= D && (best_gd == 0 || (P) < best_dpl)) {      \
    best_gd = (G);                                                                 \
    best_dpl = (P);                                                                \
  }
  GA_SGA_PAIRS(X)
#undef X
  if (best_gd == 0 && want_gd == 16) return pick_pair(D, 64, gd, dpl);      // D > 272: wave-wide scanlines
  if (best_gd == 0) return false;
  *gd = best_gd;
  *dpl = best_dpl;
  return true;
}

// f(int_c<GD>, int_c<DPL>) for the compiled pair that equals (gd, dpl)
template <class F> bool with_sga_pair(int gd, int dpl, F &&f)
{
#define X(G, P) if (gd == (G) && dpl == (P)) { f(int_c<G>{}, int_c<P>{}); return true; }
  GA_SGA_PAIRS(X)
#undef X
  return false;
}

// blocks of `per_block` items for `count` of them, at least one and at most `cap`
int clamp_grid(i64 count, int per_block, i64 cap)
{
  const i64 g = (count + per_block - 1) / per_block;
  return (int)(g < 1 ? 1 : (g < cap ? g : cap));
}
int px_grid(i64 npix) { return clamp_grid(npix, 256, 256 * 32); }
int ew_grid(i64 n) { return clamp_grid(n, 256, 256 * 16); }

int device_cus();

ScanGeom make_geom(int S, int D, int H, int W, int dir, bool backward)
{
  ScanGeom g;
  g.D = D; g.H = H; g.W = W;
  g.HW = (i64)H * W;
  const bool vertical = dir < 2;
  g.L = vertical ? H : W;
  g.Q = vertical ? W : H;
  g.total_lines = S * g.Q;
  g.line_stride = vertical ? 1 : W;
  const i64 unit = vertical ? W : 1;
  // forward visit order: down/right ascending, up/left descending; backward reverses it
  const bool ascending = ((dir == 0 || dir == 2) != backward);
  g.step_stride = ascending ? unit : -unit;
  g.start = ascending ? 0 : (i64)(g.L - 1) * unit;
  return g;
}

template <int GD, int DPL>
int launch_scan_fwd(const float *x, const float *g, float *A, int S, int D, int H, int W, int dir,
                    hipStream_t st)
{
  ScanGeom geo = make_geom(S, D, H, W, dir, false);
  const bool rowvec = DPL <= 17 && dir >= 2 && (W % 4 == 0) && aligned16(x, g, A);
  const int block = dir < 2 ? 128 : 64;      // (measured defaults of round 1, profiles/r1_tune_sga.txt)
  const int lpb = block / GD;
  const int grid = (geo.total_lines + lpb - 1) / lpb;
  if (rowvec) {
    if constexpr (DPL <= 17)
      GA_LAUNCH((sga_fwd_rowvec<GD, DPL, fwd_nv(DPL)>), dim3(grid), dim3(block), st, x, g, A, geo,
                dir == 3 ? 1 : 0);
  } else {
    GA_LAUNCH((sga_fwd_strided<GD, DPL, fwd_sb(DPL)>), dim3(grid), dim3(block), st, x, g, A, geo);
  }
  return check_launch("sga scan forward");
}

template <int GD, int DPL>
int launch_scan_bwdg(const float *g, const uint8_t *mask, const uint16_t *kp, const float *gout,
                     float *G, int S, int D, int H, int W, int dir, hipStream_t st)
{
  ScanGeom geo = make_geom(S, D, H, W, dir, true);
  const bool rowvec = DPL <= 17 && dir >= 2 && (W % 4 == 0) && aligned16(g, gout, G) && aligned4(mask) && aligned8(kp);
  const int block = dir < 2 ? 128 : 64;      // (measured defaults of round 1, profiles/r1_tune_sga.txt)
  const int lpb = block / GD;
  const int grid = (geo.total_lines + lpb - 1) / lpb;
  if (rowvec) {
    // the adjoint of `right` (2) visits w descending, of `left` (3) ascending
    if constexpr (DPL <= 17)
      GA_LAUNCH((sga_bwdg_rowvec<GD, DPL, bwd_nv(DPL)>), dim3(grid), dim3(block), st, g, mask, kp, gout,
                G, geo, dir, dir == 2 ? 1 : 0);
  } else {
    GA_LAUNCH((sga_bwdg_strided<GD, DPL, bwd_sb(DPL), uint8_t>), dim3(grid), dim3(block), st, g, mask,
              kp, gout, G, geo, dir);
  }
  return check_launch("sga adjoint scan");
}

// float-valued mask (reference buffer contract): element-strided traversal, GD = 16 family (64 for D > 272)
template <int GD, int DPL>
int launch_scan_bwdg_f32mask(const float *g, const float *mask, const uint16_t *kp, const float *gout,
                             float *G, int S, int D, int H, int W, int dir, hipStream_t st)
{
  ScanGeom geo = make_geom(S, D, H, W, dir, true);
  const int block = 64, lpb = block / GD;
  const int grid = (geo.total_lines + lpb - 1) / lpb;
  // (scan_bwdg_f32mask asks pick_pair for 16 lanes and gets 64 only past the last 16-lane pair: no 64-lane pair that small)
  if constexpr (GD == 16 || GD * DPL > 16 * 17)
    GA_LAUNCH((sga_bwdg_strided<GD, DPL, bwd_sb(DPL), float>), dim3(grid), dim3(block), st, g, mask, kp,
              gout, G, geo, dir);
  return check_launch("sga adjoint scan (f32 mask)");
}

int check_dims5(const char *who, int N, int C, int D, int H, int W)
{
  GA_TRY(check_ncdhw(who, N, C, D, H, W));
  if ((i64)D * H * W > 0x7fffffffLL / 4 || (i64)N * C * H > 0x7fffffffLL || (i64)N * C * W > 0x7fffffffLL)
    return fail(GANET_E_UNSUPPORTED, "%s: slice too large for 32-bit line indexing", who);
  return GANET_OK;
}

// ---- horizontal scans, one wavefront per row (sga_row_kernels.h) --------------------------

bool rowwave_ok(int D, int W, int dir, size_t smem)
{
  return opts().rowwave && dir >= 2 && W % 4 == 0 && D <= 16 * 13 && smem <= ROW_SMEM_MAX;
}

int row_fwd(const float *x, const float *g, float *A, int S, int D, int H, int W, int dir, hipStream_t st,
            int out_mode = 0, int C = 1, const float *scale = nullptr, const float *shift = nullptr)
{
  launch_row_fwd(x, g, A, S, D, H, W, dir, st, out_mode, C, scale, shift);   // sga_row_tu.hip (own translation unit, own flags)
  return check_launch("sga row forward");
}

// ---- vertical scans over LDS-staged 16-column blocks (sga_col_kernels.h) ----------------------------
constexpr size_t col_smem_fwd(int D) { return sizeof(float) * ((size_t)2 * COL_NC * D * COL_SBV + COL_NC * 5 * COL_SBV); }
constexpr size_t col_smem_bwdg(int D)
{
  return sizeof(float) * ((size_t)2 * COL_NC * D * COL_SBV + COL_NC * 5 * COL_SBV + COL_NC * COL_SBV) +
         (size_t)D * COL_SBV * 16;
}
bool colblock_ok(int D, int W, int dir, size_t smem)
{
  return opts().colblock && dir < 2 && W % 4 == 0 && D <= 16 * 13 && smem <= ROW_SMEM_MAX;
}
// disparities per lane the column blocks are compiled for: what the LDS cap lets through (forward D <= 125, adjoint less),
// and every caller of col_fwd / col_bwdg has asked colblock_ok
constexpr bool col_dpl_fits(int dpl) { return dpl <= 9; }
static_assert(col_smem_fwd(16 * 9 + 1) > ROW_SMEM_MAX && col_smem_bwdg(16 * 9 + 1) > ROW_SMEM_MAX, "col_dpl_fits: D = 145 fits now");

ColGeom col_geom(int D, int H, int W, int out_mode, int tiled)
{
  ColGeom geo;
  geo.D = D; geo.H = H; geo.W = W; geo.HW = (i64)H * W; geo.out_mode = out_mode; geo.tiled = tiled;
  return geo;
}

int col_fwd(const float *x, const float *g, float *A, int S, int D, int H, int W, int dir, hipStream_t st,
            int out_mode = 0)
{
  const ColGeom geo = col_geom(D, H, W, out_mode, 0);
  const int dpl = row_dpl(D);
  const bool full = dpl > 0 && D % dpl == 0;
  const size_t smem = col_smem_fwd(D);
  const dim3 grid((W + COL_NC - 1) / COL_NC, S), block(256);
  with_row_dpl(dpl, [&](auto P) {
    with_flags([&](auto asc, auto fl) {
      if constexpr (col_dpl_fits(decltype(P)::value) && (decltype(fl)::value || decltype(P)::value > 1))      // (one disparity per lane is always full)
        GA_LAUNCH_SMEM((sga_col_fwd<decltype(P)::value, decltype(asc)::value, decltype(fl)::value>), grid, block, smem, st, x, g, A, geo);
    }, dir == 0, full);
  });
  return check_launch("sga column-block forward");
}

// ---- the same column blocks with one WAVEFRONT per column (sga_col_fwd_wide / sga_col_bwdg_wide; GANET_SGA_WIDE_COL) -----
// For inputs with few column blocks (SURVEY 8d's stress shape [1,1,192,240,624]: 39 blocks) and many disparities: 16 waves
// per block instead of 4, 3-5 disparities of serial work per lane instead of 12-13, and -- unlike the register-only wide
// segment kernels -- the same 64-byte global pieces as the 16-lane column blocks.  D <= 192; up to 112 KB of LDS per block.
constexpr size_t COL_WIDE_SMEM_MAX = 152 * 1024;
int col_wide_dpl(int D) { return D <= 64 * 3 ? 3 : 0; }      // (5 disparities per lane spill at the 128 registers a 1,024-thread block leaves)
bool col_wide_ok(int D, int W, int dir, size_t smem, int S)
{
  const int mode = opts().wide_col;
  if (!mode || dir >= 2 || W % 4 != 0 || col_wide_dpl(D) <= 0 || smem > COL_WIDE_SMEM_MAX || S > 65535) return false;
  if (mode >= 2) return true;
  // automatic: fewer 16-column blocks than half the compute units (the 16-lane blocks would leave most SIMDs idle, each with
  // 12-13 disparities of serial work per lane) -- the literal stress shape [1,1,192,240,624] has 39
  return D >= 96 && (i64)S * ((W + COL_NC - 1) / COL_NC) * 2 <= device_cus();
}

int col_fwd_wide(const float *x, const float *g, float *A, int S, int D, int H, int W, int dir, hipStream_t st)
{
  const ColGeom geo = col_geom(D, H, W, 0, 0);
  const int dpl = col_wide_dpl(D);
  const bool full = D % dpl == 0;
  const size_t smem = col_smem_fwd(D);
  const dim3 grid((W + COL_NC - 1) / COL_NC, S), block(1024);
  with_int<3>(dpl, [&](auto P) {
    with_flags([&](auto asc, auto fl) {
      GA_LAUNCH_SMEM_BIG((sga_col_fwd_wide<decltype(P)::value, decltype(asc)::value, decltype(fl)::value>), grid, block, smem, st, x, g, A, geo);
    }, dir == 0, full);
  });
  static const bool trace = getenv("GANET_TRACE_DISPATCH") != nullptr;
  if (trace) fprintf(stderr, "[ganet] sga_col_fwd_wide DPL=%d dir=%d D=%d smem=%zu\n", dpl, dir, D, smem);
  return check_launch("sga wide column-block forward");
}

int col_bwdg_wide(const float *g, const uint8_t *mask, const uint16_t *kp, const float *gout, float *G,
                  int S, int D, int H, int W, int dir, hipStream_t st)
{
  const ColGeom geo = col_geom(D, H, W, 0, 0);
  const int dpl = col_wide_dpl(D);
  const size_t smem = col_smem_bwdg(D);
  const dim3 grid((W + COL_NC - 1) / COL_NC, S), block(1024);
  const bool m16 = W % 16 == 0 && aligned16(mask);
  with_int<3>(dpl, [&](auto P) {
    with_flags([&](auto asc, auto m) {
      GA_LAUNCH_SMEM_BIG((sga_col_bwdg_wide<decltype(P)::value, decltype(asc)::value, decltype(m)::value, false>), grid, block, smem, st, g, mask, kp, gout, G, geo, dir);
    }, dir == 1, m16);
  });
  static const bool trace = getenv("GANET_TRACE_DISPATCH") != nullptr;
  if (trace) fprintf(stderr, "[ganet] sga_col_bwdg_wide DPL=%d dir=%d D=%d smem=%zu\n", dpl, dir, D, smem);
  return check_launch("sga wide column-block adjoint scan");
}

int col_bwdg(const float *g, const uint8_t *mask, const uint16_t *kp, const float *gout, float *G,
             int S, int D, int H, int W, int dir, hipStream_t st, int tiled = 0)
{
  const ColGeom geo = col_geom(D, H, W, 0, tiled);
  const int dpl = row_dpl(D);
  const size_t smem = col_smem_bwdg(D);
  const dim3 grid((W + COL_NC - 1) / COL_NC, S), block(256);
  // the adjoint of `down` (0) walks rows upwards (H-1..0), of `up` (1) downwards
  const bool m16 = W % 16 == 0 && aligned16(mask);
  // (lanes wholly inside / outside [0, D): the leaner recurrence of bwdg_step<FULL>, instantiated for the depths the models use
  //  -- 33 and 48 at three, 65 at five disparities per lane)
  const bool full = D % dpl == 0;
  with_row_dpl(dpl, [&](auto P) {
    with_flags([&](auto asc, auto m, auto fl) {
      constexpr bool FL = decltype(fl)::value && (decltype(P)::value == 3 || decltype(P)::value == 5);
      if constexpr (col_dpl_fits(decltype(P)::value))
        GA_LAUNCH_SMEM((sga_col_bwdg<decltype(P)::value, decltype(asc)::value, decltype(m)::value, FL>), grid, block, smem, st, g, mask, kp, gout, G, geo, dir);
    }, dir == 1, m16, full);
  });
  return check_launch("sga column-block adjoint scan");
}

int row_bwdg(const float *g, const uint8_t *mask, const uint16_t *kp, const float *gout, float *G,
             int S, int D, int H, int W, int dir, hipStream_t st)
{
  launch_row_bwdg(g, mask, kp, gout, G, S, D, H, W, dir, st);       // sga_row_tu.hip
  return check_launch("sga row adjoint scan");
}

// Inputs with few scanlines (a single slice at full resolution: SURVEY 8d's literal stress shape [1,1,192,240,624] has 624
// columns / 240 rows) leave most of the 1,024 SIMDs without a wave when a scanline is 16 lanes wide (156 / 240 waves): the
// segment kernels with the whole wavefront on one scanline give 4x the waves and a quarter of the serial work per position.
// Measured on that shape (profiles/r2n_sga_wide_scan_stress_shape.txt): horizontal scans 0.25 -> 0.10 ms forward and
// 0.31 -> 0.21 ms adjoint; VERTICAL scans do not gain (0.33 -> 0.32, adjoint 0.49 -> 0.54-0.64 ms): with one column per wave
// every lane of a load touches a different plane (64 cache lines for 256 bytes), which the LDS-staged column blocks avoid.
// So the automatic mode widens horizontal scans only; D > 272 takes the wide kernels in every direction (pick_pair).
bool few_lines(int N, int C, int D, int H, int W, int dir)
{
  if (opts().wide_scan == 0) return false;
  if (opts().wide_scan == 2) return D > 48;
  if (dir < 2) return false;
  const i64 lines = (i64)N * C * H;
  return D >= 96 && lines * 16 < (i64)4 * device_cus() * 64 * 2;      // fewer 16-lane segments than two waves per SIMD hold
}

// ---- the one place that chooses the kernel family of an SGA scan ------------------------------------------------------------
// In order of preference: wide column blocks, wide segments (GD = 64), row waves, column blocks, segments.
enum ScanFamily { SCAN_COL_WIDE, SCAN_SEG_WIDE, SCAN_ROW_WAVE, SCAN_COL_BLOCK, SCAN_SEGMENT, SCAN_NONE };
struct ScanQuery {
  int N, C, D, H, W, dir;
  bool adjoint;                         // the pass: forward scan | adjoint scan
  bool vol16, mask4 = true, kp8 = true; // alignment facts: every volume 16 bytes, the mask 4, kp 8 (a forward scan has neither)
};
struct ScanChoice { ScanFamily family; int gd, dpl; };      // (gd, dpl): the segment kernels' pair

// does this family's kernel apply to the scan?  (options, shape, LDS need and alignment; not: whether a better one does too)
bool scan_family_ok(ScanFamily f, const ScanQuery &q)
{
  const int S = q.N * q.C, D = q.D;
  switch (f) {
    case SCAN_COL_WIDE: return col_wide_ok(D, q.W, q.dir, q.adjoint ? col_smem_bwdg(D) : col_smem_fwd(D), S) && q.vol16 && q.mask4;
    case SCAN_SEG_WIDE: return few_lines(q.N, q.C, D, q.H, q.W, q.dir);
    case SCAN_ROW_WAVE: return rowwave_ok(D, q.W, q.dir, q.adjoint ? row_smem_bwdg(D) : row_smem_fwd(D)) && q.vol16 && q.mask4 && q.kp8;
    case SCAN_COL_BLOCK: return colblock_ok(D, q.W, q.dir, q.adjoint ? col_smem_bwdg(D) : col_smem_fwd(D)) && q.vol16 && q.mask4 && S <= 65535;
    default: return f == SCAN_SEGMENT;
  }
}

ScanChoice choose_scan(const ScanQuery &q)
{
  int gd = 0, dpl = 0;
  if (scan_family_ok(SCAN_COL_WIDE, q)) return {SCAN_COL_WIDE, 0, 0};
  if (scan_family_ok(SCAN_SEG_WIDE, q) && pick_pair(q.D, 64, &gd, &dpl)) return {SCAN_SEGMENT, gd, dpl};
  if (scan_family_ok(SCAN_ROW_WAVE, q)) return {SCAN_ROW_WAVE, 0, 0};
  if (scan_family_ok(SCAN_COL_BLOCK, q)) return {SCAN_COL_BLOCK, 0, 0};
  if (!pick_pair(q.D, 16, &gd, &dpl)) return {SCAN_NONE, 0, 0};
  return {SCAN_SEGMENT, gd, dpl};
}

int no_scan_kernel(const ScanChoice &c, int D)
{
  if (c.family == SCAN_NONE) return fail(GANET_E_UNSUPPORTED, "SGA: D=%d exceeds the compiled maximum (1088)", D);
  return fail(GANET_E_UNSUPPORTED, "SGA: no kernel for GD=%d DPL=%d", c.gd, c.dpl);
}

// 1 if ganet_sga_backward keeps G_down / G_up in the tiled layout of sga_col_kernels.h for these dimensions: where the 16-lane
// column-block adjoint kernel runs (not the wide one), W % 16 == 0, H % 4 == 0.  Decided from the dimensions and GANET_SGA_TILED,
// and from the alignment of what the tiled column kernels touch where the caller knows it.
int sga_ws_tiled(int N, int C, int D, int H, int W, bool vol16 = true, bool mask4 = true)
{
  if (!opts().sga_tiled || W % 16 != 0 || H % 4 != 0 || N * C > 65535 || opts().wide_scan == 2) return 0;
  const ScanQuery q = {N, C, D, H, W, 0, true, vol16, mask4};
  return (!scan_family_ok(SCAN_COL_WIDE, q) && scan_family_ok(SCAN_COL_BLOCK, q)) ? 1 : 0;
}

int scan_fwd(const float *x, const float *g, float *A, int N, int C, int D, int H, int W, int dir,
             hipStream_t st)
{
  const ScanChoice c = choose_scan({N, C, D, H, W, dir, false, aligned16(x, g, A)});
  if (c.family == SCAN_COL_WIDE) return col_fwd_wide(x, g, A, N * C, D, H, W, dir, st);
  if (c.family == SCAN_ROW_WAVE) return row_fwd(x, g, A, N * C, D, H, W, dir, st);
  if (c.family == SCAN_COL_BLOCK) return col_fwd(x, g, A, N * C, D, H, W, dir, st);
  int rc;
  if (with_sga_pair(c.gd, c.dpl, [&](auto G, auto P) {
        rc = launch_scan_fwd<decltype(G)::value, decltype(P)::value>(x, g, A, N * C, D, H, W, dir, st);
      }))
    return rc;
  return no_scan_kernel(c, D);
}

int scan_bwdg(const float *g, const uint8_t *mask, const uint16_t *kp, const float *gout, float *G,
              int N, int C, int D, int H, int W, int dir, hipStream_t st, int tiled = 0)
{
  const bool vol16 = aligned16(g, gout, G);
  if (tiled) {
    if (!(vol16 && aligned4(mask))) return fail(GANET_E_UNSUPPORTED, "SGA: tiled workspace needs 16-byte aligned volumes");
    return col_bwdg(g, mask, kp, gout, G, N * C, D, H, W, dir, st, 1);
  }
  const ScanChoice c = choose_scan({N, C, D, H, W, dir, true, vol16, aligned4(mask), aligned8(kp)});
  if (c.family == SCAN_COL_WIDE) return col_bwdg_wide(g, mask, kp, gout, G, N * C, D, H, W, dir, st);
  if (c.family == SCAN_ROW_WAVE) return row_bwdg(g, mask, kp, gout, G, N * C, D, H, W, dir, st);
  if (c.family == SCAN_COL_BLOCK) return col_bwdg(g, mask, kp, gout, G, N * C, D, H, W, dir, st);
  int rc;
  if (with_sga_pair(c.gd, c.dpl, [&](auto GD, auto P) {
        rc = launch_scan_bwdg<decltype(GD)::value, decltype(P)::value>(g, mask, kp, gout, G, N * C, D, H, W, dir, st);
      }))
    return rc;
  return no_scan_kernel(c, D);
}

int scan_bwdg_f32mask(const float *g, const float *mask, const uint16_t *kp, const float *gout, float *G,
                      int N, int C, int D, int H, int W, int dir, hipStream_t st)
{
  int gd, dpl, rc;
  if (!pick_pair(D, 16, &gd, &dpl)) return fail(GANET_E_UNSUPPORTED, "SGA: D=%d exceeds the compiled maximum (1088)", D);
  if (with_sga_pair(gd, dpl, [&](auto GD, auto P) {
        rc = launch_scan_bwdg_f32mask<decltype(GD)::value, decltype(P)::value>(g, mask, kp, gout, G, N * C, D, H, W, dir, st);
      }))
    return rc;
  return fail(GANET_E_UNSUPPORTED, "SGA: no kernel for DPL=%d", dpl);
}

// per-pixel gradients for `ndir` (1 or 4) directions
int bwd_point(const float *x, float *gx, const PointArgs &pa, int ndir, int N, int C, int D, int H, int W,
              int accumulate, hipStream_t st, int tiled = 0)
{
  const i64 npix = (i64)N * C * H * W;
  const int pb = 256;      // (64 / 128 measured equal)
  const dim3 grid(clamp_grid(npix, pb, (i64)256 * 32 * (256 / pb)));
  // (every four-direction caller overwrites grad_x; the tiled layout of G_down / G_up exists for that form alone: sga_bwd_point<4, false, true>)
  with_flags([&](auto four, auto acc, auto til) {
    constexpr int ND = decltype(four)::value ? 4 : 1;
    constexpr bool ACC = decltype(acc)::value, TG = decltype(til)::value;
    if constexpr (ND == 4 ? !ACC : !TG)
      GA_LAUNCH((sga_bwd_point<ND, ACC, TG>), grid, dim3(pb), st, x, gx, pa, D, H, W, npix);
  }, ndir == 4, accumulate != 0, ndir == 4 && !accumulate && tiled);
  return check_launch("sga per-pixel gradients");
}

// compute units of the current device (256 on MI355X); the emulator build reports 256
int device_cus()
{
#if defined(GA_HIPSIM)
  return 256;
#else
  static int cus[16] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return 256;
  if (cus[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cus[dev] = n;
  }
  return cus[dev];
#endif
}

// ---- LGA dispatch -------------------------------------------------------------------
// Work items of the plane-pair forward / data-backward (LgaSegMix).  Every item re-gathers its pixels' filter taps (75 loads per
// lane; for the data-backward from 25 neighbouring pixels) and fills its ring, 0.038 ms of a 0.107 ms pass
// (profiles/r2f_lga_pp_ablation.txt), so whole tiles are best (profiles/r2e_ab_lga_plane_pairs_v2.txt) unless there are too few
// of them to fill the wave slots; with a whole number q < 3 of tiles per SIMD plus a remainder, the remainder is cut into
// segments, at most one per SIMD (the mixed list).  `whole_only`: the pass carries a per-pixel reduction over all of D.
// `wg`: items of the workgroup kernels (32 x 8 tiles, four waves each: the unit that takes an item is a CU, not a SIMD).
LgaSegMix lga_items(int W, int H, int B, int D, bool whole_only, i64 *items, bool wg = false)
{
  LgaSegMix mx;
  const int th = wg ? 8 : LGAW_TH, units = (wg ? 1 : 4) * device_cus();
  mx.tiles_x = (W + LGA_TW - 1) / LGA_TW;
  mx.tiles_y = (H + th - 1) / th;
  const i64 tiles = (i64)mx.tiles_x * mx.tiles_y * B;
  mx.n_whole = (int)(tiles < (1ll << 30) ? tiles : (1ll << 30));
  mx.nsub = 1;
  mx.sub_len = (D + 1) & ~1;
  *items = tiles;
  if (whole_only || tiles >= (1ll << 30)) return mx;
  const i64 slots = (i64)LGA_WAVES_PER_SIMD * units;
  int nseg = opts().lga_segs;
  if (nseg <= 0) {
    nseg = tiles * 2 > slots ? 1 : (int)((slots + tiles - 1) / tiles);
    if (nseg > D / 16) nseg = D / 16 > 1 ? D / 16 : 1;
  }
  if (nseg > D) nseg = D;
  if (nseg > 1) {                                   // every tile cut into equal segments
    mx.n_whole = 0;
    mx.sub_len = ((D + nseg - 1) / nseg + 1) & ~1;
    mx.nsub = (D + mx.sub_len - 1) / mx.sub_len;
    *items = tiles * mx.nsub;
    return mx;
  }
  const int mixo = opts().lga_mix;
  const i64 S = mixo > 1 ? (i64)mixo : (i64)units;
  if (mixo && opts().lga_segs <= 0 && tiles / S < LGA_WAVES_PER_SIMD && tiles % S != 0) {
    const i64 r = tiles % S;
    int nsub = (int)(S / r);
    if (nsub > D / 16) nsub = D / 16;
    if (nsub >= 2) {
      mx.n_whole = (int)(tiles - r);
      mx.sub_len = ((D + nsub - 1) / nsub + 1) & ~1;
      mx.nsub = (D + mx.sub_len - 1) / mx.sub_len;
      *items = mx.n_whole + r * mx.nsub;
    }
  }
  return mx;
}

#ifndef GA_LGA_PLANAR
#ifndef GA_FGP_DEFAULT
#define GA_FGP_DEFAULT 1  // (0: a build whose GANET_LGA_WAVE=2 keeps the one-wave filter gradient -- same-box A/B builds, scripts/build_variants.py)
#endif
#ifndef GA_FGP_WPS
#define GA_FGP_WPS 5      // waves per SIMD the wave-pair filter gradient is compiled for
#endif
#define GA_LGA_PLANAR 1     // API-layout operands of the plane-pair kernels staged planar by 16-byte copies where W % 4 == 0
#endif
// API-layout operand of the plane-pair kernels staged planar by 16-byte copies (radius 2 alone)
template <int R> bool lga_planar(int W, const float *x) { return R == 2 && GA_LGA_PLANAR && W % 4 == 0 && aligned16(x); }

LgaGeom lga_geom(int D, int H, int W)
{
  LgaGeom geo;
  geo.D = D; geo.H = H; geo.W = W; geo.HW = (i64)H * W;
  return geo;
}

// the items of a pass that takes whole 32 x 2 tiles, one depth segment each
LgaSeg lga_whole_tiles(int W, int H, int B, int D, i64 *items)
{
  LgaSeg sg;
  sg.tiles_x = (W + LGA_TW - 1) / LGA_TW;
  sg.tiles_y = (H + LGAW_TH - 1) / LGAW_TH;
  sg.nseg = 1; sg.seg_len = D;
  *items = (i64)sg.tiles_x * sg.tiles_y * B;
  return sg;
}

template <int R>
int launch_lga_fwd(const float *x, const float *f, float *y, int B, int D, int H, int W,
                   bool transposed, hipStream_t st)
{
  const LgaGeom geo = lga_geom(D, H, W);
  if constexpr (R <= 2) {
    const int family = opts().lga_wave;
    if (family && (i64)H * W < (1ll << 28)) {
      i64 items;
      const bool planar = lga_planar<R>(W, x);
      if constexpr (R == 2) {
        if (planar && family == 2) {                      // one ring per 256-thread workgroup (32 x 8 tiles)
          const LgaSegMix wx = lga_items(W, H, B, D, false, &items, true);
          if (items < (1ll << 31)) {
            with_flags([&](auto t) { GA_LAUNCH((lga_apply_pp_wx<2, decltype(t)::value>), dim3((unsigned)items), dim3(256), st, x, f, y, geo, wx); }, transposed);
            return check_launch("lga apply (plane pairs, workgroup ring)");
          }
        }
      }
      const LgaSegMix mx = lga_items(W, H, B, D, false, &items);
      if (items < (1ll << 31)) {
        with_flags([&](auto t, auto pl) {      // (planar: R == 2 alone)
          if constexpr (!decltype(pl)::value) GA_LAUNCH((lga_apply_pp<R, decltype(t)::value>), dim3((unsigned)items), dim3(64), st, x, f, y, geo, mx);
          else if constexpr (R == 2) GA_LAUNCH((lga_apply_pp_x<2, decltype(t)::value>), dim3((unsigned)items), dim3(64), st, x, f, y, geo, mx);
        }, transposed, planar);
        static const bool trace = getenv("GANET_TRACE_DISPATCH") != nullptr;      // (development: which LGA kernel ran)
        if (trace) fprintf(stderr, "[ganet] lga_apply_pp R=%d T=%d items=%lld: %d whole tiles + segments of %d planes x %d\n", R, (int)transposed, (long long)items, mx.n_whole, mx.sub_len, mx.nsub);
        return check_launch("lga apply (plane pairs)");
      }
    }
  }
  const dim3 grid((W + LGA_TW - 1) / LGA_TW, (H + LGA_TH - 1) / LGA_TH, B);
  with_flags([&](auto t) { GA_LAUNCH((lga_apply<R, decltype(t)::value>), grid, dim3(LGA_NT), st, x, f, y, geo); }, transposed);
  return check_launch("lga apply");
}

// one LGA pass / data-backward with one side in the pair-interleaved layout (lga_apply_pp_pi / lga_apply_pp_po / lga_apply_pp_xo)
int launch_lga_paired(const float *x, const float *f, float *y, int B, int D, int H, int W, bool transposed, bool x_paired,
                      hipStream_t st, float *edge = nullptr)
{
  if ((i64)H * W >= (1ll << 28) || W % 2 != 0 || !aligned16(x) || !aligned16(y))
    return fail(GANET_E_UNSUPPORTED, "ganet_lga_apply_paired: needs W even, planes below 2^28 pixels and 16-byte aligned volumes");
  const LgaGeom geo = lga_geom(D, H, W);
  i64 items;
  float *const none = nullptr;
  const bool wg_ring = opts().lga_wave == 2;
  const bool planar = GA_LGA_PLANAR && W % 4 == 0;      // API-layout input staged planar, two 16-byte copies per plane pair
  if (wg_ring && (x_paired || planar)) {                // one ring per 256-thread workgroup (32 x 8 tiles)
    const LgaSegMix wx = lga_items(W, H, B, D, false, &items, true);
    if (items < (1ll << 31)) {
      const dim3 grid((unsigned)items), block(256);
      with_flags([&](auto t, auto xp) {
        constexpr bool T = decltype(t)::value;
        if constexpr (decltype(xp)::value) GA_LAUNCH((lga_apply_pp_wpi<2, T>), grid, block, st, x, f, y, geo, wx, none, none, edge);
        else GA_LAUNCH((lga_apply_pp_wxo<2, T>), grid, block, st, x, f, y, geo, wx, none, none, edge);
      }, transposed, x_paired);
      return check_launch(x_paired ? "lga apply (plane pairs, interleaved input, workgroup ring)"
                                   : "lga apply (plane pairs, interleaved volume, workgroup ring)");
    }
  }
  const LgaSegMix sg = lga_items(W, H, B, D, false, &items);
  if (items >= (1ll << 31)) return fail(GANET_E_UNSUPPORTED, "ganet_lga_apply_paired: too many tiles");
  const dim3 grid((unsigned)items), block(64);
  with_flags([&](auto t, auto xp, auto pl) {
    constexpr bool T = decltype(t)::value;
    if constexpr (decltype(xp)::value) GA_LAUNCH((lga_apply_pp_pi<2, T>), grid, block, st, x, f, y, geo, sg, none, none, edge);
    else if constexpr (decltype(pl)::value) GA_LAUNCH((lga_apply_pp_xo<2, T>), grid, block, st, x, f, y, geo, sg, none, none, edge);
    else GA_LAUNCH((lga_apply_pp_po<2, T>), grid, block, st, x, f, y, geo, sg, none, none, edge);
  }, transposed, x_paired, planar);
  return check_launch("lga apply (plane pairs, interleaved volume)");
}

int launch_lga_gf_paired(const float *x, const float *gy, float *gf, int B, int D, int H, int W, int acc, bool x_paired,
                         hipStream_t st)
{
  if ((i64)H * W >= (1ll << 28) || W % 2 != 0 || !aligned16(x) || !aligned16(gy))
    return fail(GANET_E_UNSUPPORTED, "ganet_lga_filter_grad_paired: needs W even, planes below 2^28 pixels and 16-byte aligned volumes");
  const LgaGeom geo = lga_geom(D, H, W);
  i64 items;
  const LgaSeg sg = lga_whole_tiles(W, H, B, D, &items);
  if (items >= (1ll << 31)) return fail(GANET_E_UNSUPPORTED, "ganet_lga_filter_grad_paired: too many tiles");
  const bool fg_pair = GA_FGP_DEFAULT && opts().lga_wave >= 2;      // the workgroup forms: here the taps of a tile split over a wave pair (lga_filter_grad_pair.inc)
  if (x_paired && fg_pair) GA_LAUNCH((lga_filter_grad_pair_xp<GA_FGP_WPS>), dim3((unsigned)items), dim3(128), st, x, gy, gf, geo, sg, acc);
  else if (x_paired) GA_LAUNCH((lga_filter_grad_pp_xp<2, 3, 0>), dim3((unsigned)items), dim3(64), st, x, gy, gf, geo, sg, acc);
  else if (GA_LGA_PLANAR && W % 4 == 0) GA_LAUNCH((lga_filter_grad_pp_gypx<2, 3, 0>), dim3((unsigned)items), dim3(64), st, x, gy, gf, geo, sg, acc);
  else GA_LAUNCH((lga_filter_grad_pp_gyp<2, 3, 0>), dim3((unsigned)items), dim3(64), st, x, gy, gf, geo, sg, acc);
  return check_launch("lga filter grad (plane pairs, interleaved volume)");
}

// one LGA pass whose output is also reduced over d per pixel (plane-pair kernel, one depth segment per tile)
template <int R>
int launch_lga_fwd_regress(const float *x, const float *f, float *y, float *snorm, float *sdy, int B, int D, int H, int W,
                           hipStream_t st)
{
  if constexpr (R <= 2) {
    if ((i64)H * W < (1ll << 28)) {
      const LgaGeom geo = lga_geom(D, H, W);
      i64 items;
      const LgaSegMix sg = lga_items(W, H, B, D, true, &items);      // (the epilogue reduces over all of D: whole tiles only)
      if (items < (1ll << 31)) {
        with_flags([&](auto pl) {
          if constexpr (!decltype(pl)::value) GA_LAUNCH((lga_apply_pp<R, false, true>), dim3((unsigned)items), dim3(64), st, x, f, y, geo, sg, snorm, sdy);
          else if constexpr (R == 2) GA_LAUNCH((lga_apply_pp_x<2, false, true>), dim3((unsigned)items), dim3(64), st, x, f, y, geo, sg, snorm, sdy);
        }, lga_planar<R>(W, x));
        return check_launch("lga apply + regression epilogue (plane pairs)");
      }
    }
  }
  return fail(GANET_E_UNSUPPORTED, "ganet_lga_forward_regress: no fused kernel for this shape / radius: run ganet_lga_forward "
                                   "and ganet_norm_disparity_regression_forward instead");
}

template <int R>
int launch_lga_gf(const float *x, const float *gy, float *gf, int B, int D, int H, int W, int acc,
                  hipStream_t st)
{
  const LgaGeom geo = lga_geom(D, H, W);
  if constexpr (R <= 2) {
    if (opts().lga_wave && (i64)H * W < (1ll << 28)) {
      i64 items;
      const LgaSeg sg = lga_whole_tiles(W, H, B, D, &items);
      if (items < (1ll << 31)) {
        with_flags([&](auto pl) {
          if constexpr (!decltype(pl)::value) GA_LAUNCH((lga_filter_grad_pp<R, 3, 0>), dim3((unsigned)items), dim3(64), st, x, gy, gf, geo, sg, acc);
          else if constexpr (R == 2) GA_LAUNCH((lga_filter_grad_pp_x<2, 3, 0>), dim3((unsigned)items), dim3(64), st, x, gy, gf, geo, sg, acc);
        }, lga_planar<R>(W, x));
        return check_launch("lga filter grad (plane pairs)");
      }
    }
  }
  const dim3 grid((W + LGA_TW - 1) / LGA_TW, (H + LGA_TH - 1) / LGA_TH, B);
  GA_LAUNCH((lga_filter_grad<R>), grid, dim3(LGA_NT), st, x, gy, gf, geo, acc);
  return check_launch("lga filter grad");
}

int check_lga(const char *who, int B, int D, int H, int W, int radius)
{
  if (B <= 0 || D <= 0 || H <= 0 || W <= 0) return fail(GANET_E_INVALID, "%s: non-positive size B=%d D=%d H=%d W=%d", who, B, D, H, W);
  if (radius < 1 || radius > 3) return fail(GANET_E_UNSUPPORTED, "%s: radius %d not in the compiled set {1,2,3}", who, radius);
  if (B > 65535) return fail(GANET_E_UNSUPPORTED, "%s: batch %d > 65535 (grid.z)", who, B);
  return GANET_OK;
}

__global__ void dpp_probe(int *out)
{
  const int lane = threadIdx.x;
  out[0 * 64 + lane] = dpp_i<DPP_QP_XOR1>(-1, lane);
  out[1 * 64 + lane] = dpp_i<DPP_QP_XOR2>(-1, lane);
  out[2 * 64 + lane] = dpp_i<DPP_ROW_SHL1>(-1, lane);
  out[3 * 64 + lane] = dpp_i<DPP_ROW_SHR1>(-1, lane);
  out[4 * 64 + lane] = dpp_i<DPP_ROW_MIRROR>(-1, lane);
  out[5 * 64 + lane] = dpp_i<DPP_ROW_HALF_MIRROR>(-1, lane);
  float v = (float)((lane * 37) % 64);
  int k = lane;
  seg_argmax<16>(v, k);
  out[6 * 64 + lane] = k;
  out[7 * 64 + lane] = (int)seg_allsum<16>((float)lane);
}

// whole-wavefront patterns of the 64-lanes-per-scanline scans
__global__ void dpp_probe_wave(int *out)
{
  const int lane = threadIdx.x;
  out[0 * 64 + lane] = dpp_i<DPP_WAVE_SHL1>(-1, lane);
  out[1 * 64 + lane] = dpp_i<DPP_WAVE_SHR1>(-1, lane);
  out[2 * 64 + lane] = (int)seg_allmax<64>((float)((lane * 37) % 64));
  out[3 * 64 + lane] = (int)seg_allsum<64>((float)lane);
}

}  // namespace

// =====================================================================================
GA_EXPORT int ganet_abi_version(void) { return GANET_ABI_VERSION; }
GA_EXPORT const char *ganet_last_error(void) { return g_err; }
GA_EXPORT int ganet_is_simulator(void)
{
#if defined(GA_HIPSIM)
  return 1;
#else
  return 0;
#endif
}

GA_EXPORT int ganet_get_option(const char *name)
{
  const char *who = "ganet_get_option";
  opts();
  if (!name) return fail(GANET_E_INVALID, "%s: null name", who);
  if (const OptionDesc *o = find_option(name)) return g_opt.*o->field;
  return fail(GANET_E_INVALID, "%s: unknown option %s", who, name);
}

GA_EXPORT int ganet_set_option(const char *name, int value)
{
  const char *who = "ganet_set_option";
  opts();
  if (!name) return fail(GANET_E_INVALID, "%s: null name", who);
  if (store_option(name, value)) {}      // a library option, normalised
#if defined(GA_HIPSIM)
  else if (!strcmp(name, "HIPSIM_LATE_DMA")) hipsim::S().late_dma = value != 0;   // emulator only: see tests/hipsim/hipsim.h
  else if (!strcmp(name, "HIPSIM_LANE_ORDER")) hipsim::S().lane_order = value ? 1 : 0;
  else if (!strcmp(name, "HIPSIM_WAVE_GREEDY")) hipsim::S().wave_greedy = value ? 1 : 0;   // one wavefront runs as far as its synchronisation lets it
  else if (!strcmp(name, "HIPSIM_LATE_LDS")) hipsim::S().late_lds = value != 0;
  else if (!strcmp(name, "HIPSIM_LGKM_SLACK")) hipsim::S().lgkm_slack = value;     // tests: every counted LDS wait loosened by `value`
  else if (!strcmp(name, "HIPSIM_VMCNT_SLACK")) hipsim::S().vm_slack = value;      // tests: every counted copy wait loosened by `value`
#endif
  else {
    // names retired in ABI 7 / 10 (their kernels were removed, became the only path, or the switch moved into another option:
    // GANET_LGA_WG -> GANET_LGA_WAVE = 2 | 1): accepted and ignored, so that a caller written against an older ABI keeps running;
    // one note per process
    static const char *const retired[] = {"GANET_LGA_BWD_STREAMS", "GANET_LGA_FG_WPS", "GANET_LGA_SPLIT", "GANET_LGA_VMCNT_SAFE",
                                          "GANET_SGA_BLOCK_H", "GANET_SGA_BLOCK_V", "GANET_SGA_GD", "GANET_SGA_GD_H", "GANET_SGA_GD_V",
                                          "GANET_SGA_INFER_FUSED", "GANET_SGA_MERGE4", "GANET_SGA_POINT_BLOCK", "GANET_SGA_STREAMS",
                                          "GANET_LGA_WG", "GANET_SGA_POINT_Q4"};
    for (const char *r : retired)
      if (!strcmp(name, r)) {
        static std::atomic<int> noted{0};
        if (!noted.exchange(1)) fprintf(stderr, "[ganet] ganet_set_option: %s is retired (no effect); see INTEGRATION.md\n", name);
        return GANET_OK;
      }
    return fail(GANET_E_INVALID, "%s: unknown option %s", who, name);
  }
  return GANET_OK;
}

GA_EXPORT int ganet_sga_scan_forward(const float *x, const float *g, float *A, int N, int C, int D,
                                     int H, int W, int dir, void *stream)
{
  const char *who = "ganet_sga_scan_forward";
  GA_TRY(check_ptrs(who, x, g, A));
  GA_TRY(check_dir(who, dir));
  GA_TRY(check_dims5(who, N, C, D, H, W));
  return scan_fwd(x, g, A, N, C, D, H, W, dir, (hipStream_t)stream);
}

GA_EXPORT int ganet_sga_scan_forward_ws(const float *x, const float *g, float *A_ws, int N, int C, int D, int H, int W, int dir,
                                         void *stream)
{
  const char *who = "ganet_sga_scan_forward_ws";
  GA_TRY(check_ptrs(who, x, g, A_ws));
  GA_TRY(check_dir(who, dir));
  GA_TRY(check_dims5(who, N, C, D, H, W));
  const i64 n = (i64)N * C * D * H * W;
  return scan_fwd(x, g, A_ws + dir * n, N, C, D, H, W, dir, (hipStream_t)stream);
}

GA_EXPORT int ganet_sga_backward_scan_ws(const float *g, const uint8_t *mask, const uint16_t *kp, const float *grad_out, float *G_ws,
                                          int N, int C, int D, int H, int W, int dir, void *stream)
{
  const char *who = "ganet_sga_backward_scan_ws";
  GA_TRY(check_ptrs(who, g, mask, kp, grad_out, G_ws));
  GA_TRY(check_dir(who, dir));
  GA_TRY(check_dims5(who, N, C, D, H, W));
  const i64 n = (i64)N * C * D * H * W, npix = (i64)N * C * H * W;
  return scan_bwdg(g, mask, kp + dir * npix, grad_out, G_ws + dir * n, N, C, D, H, W, dir, (hipStream_t)stream,
                   dir < 2 && sga_ws_tiled(N, C, D, H, W));
}

GA_EXPORT int ganet_sga_workspace_layout(int N, int C, int D, int H, int W)
{
  if (check_dims5("ganet_sga_workspace_layout", N, C, D, H, W) != GANET_OK) return GANET_E_INVALID;
  return sga_ws_tiled(N, C, D, H, W);
}

GA_EXPORT int ganet_sga_merge(const float *A_ws, float *out, uint8_t *mask, uint16_t *kp, int N, int C, int D, int H, int W,
                               void *stream)
{
  const char *who = "ganet_sga_merge";
  GA_TRY(check_ptrs(who, A_ws, out, mask, kp));
  GA_TRY(check_dims5(who, N, C, D, H, W));
  if (D > 65535) return fail(GANET_E_UNSUPPORTED, "%s: D > 65535", who);
  const i64 n = (i64)N * C * D * H * W;
  const i64 npix = (i64)N * C * H * W;
  hipStream_t st = (hipStream_t)stream;
  const i64 HWl = (i64)H * W;
  const bool al = aligned16(A_ws, out) && aligned4(mask) && aligned8(kp);
  if (HWl % 4 == 0 && al && npix / 4 / 64 + 1 < (1ll << 31)) {
    GA_LAUNCH(sga_merge_px4, dim3((unsigned)((npix / 4 + 63) / 64)), dim3(64), st, A_ws, A_ws + n, A_ws + 2 * n,
              A_ws + 3 * n, out, mask, kp, D, HWl, npix);
    return check_launch("sga merge (4 px / lane)");
  }
  GA_LAUNCH((sga_merge_px<uint8_t>), dim3(px_grid(npix)), dim3(256), st, A_ws, A_ws + n, A_ws + 2 * n,
            A_ws + 3 * n, out, mask, kp, D, HWl, npix);
  return check_launch("sga merge");
}

GA_EXPORT int ganet_sga_forward(const float *x, const float *g0, const float *g1, const float *g2,
                                const float *g3, float *A_ws, float *out, uint8_t *mask,
                                uint16_t *kp, int N, int C, int D, int H, int W, void *stream)
{
  const char *who = "ganet_sga_forward";
  GA_TRY(check_ptrs(who, x, g0, g1, g2, g3, A_ws, out, mask, kp));
  GA_TRY(check_dims5(who, N, C, D, H, W));
  if (D > 65535) return fail(GANET_E_UNSUPPORTED, "%s: D > 65535", who);
  const i64 n = (i64)N * C * D * H * W;
  hipStream_t st = (hipStream_t)stream;
  const float *gs[4] = {g0, g1, g2, g3};
  // (the four scans on four streams were measured twice and dropped: 0.596 vs 0.606 ms)
  for (int d = 0; d < 4; d++) GA_TRY(scan_fwd(x, gs[d], A_ws + d * n, N, C, D, H, W, d, st));
  return ganet_sga_merge(A_ws, out, mask, kp, N, C, D, H, W, stream);
}

namespace {
bool infer_fused_ok(const float *x, const float *g0, const float *g1, const float *g2, const float *g3, const float *out,
                    int N, int C, int D, int W)
{
  // (H does not enter either family's test)
  const bool all_al = aligned16(x, out, g0, g1, g2, g3);
  return scan_family_ok(SCAN_ROW_WAVE, {N, C, D, 0, W, 2, false, all_al}) &&
         scan_family_ok(SCAN_COL_BLOCK, {N, C, D, 0, W, 0, false, all_al});
}
}  // namespace

GA_EXPORT int ganet_sga_forward_infer_scratch(const float *x, const float *g0, const float *g1, const float *g2,
                                              const float *g3, const float *out, int N, int C, int D, int H, int W)
{
  const char *who = "ganet_sga_forward_infer_scratch";
  GA_TRY(check_ptrs(who, x, g0, g1, g2, g3, out));
  GA_TRY(check_dims5(who, N, C, D, H, W));
  return infer_fused_ok(x, g0, g1, g2, g3, out, N, C, D, W) ? 0 : 4;
}

GA_EXPORT int ganet_sga_forward_infer(const float *x, const float *g0, const float *g1, const float *g2,
                                      const float *g3, float *A_ws, float *out, const float *bn_scale,
                                      const float *bn_shift, int N, int C, int D, int H, int W,
                                      void *stream)
{
  const char *who = "ganet_sga_forward_infer";
  GA_TRY(check_ptrs(who, x, g0, g1, g2, g3, out));
  if ((bn_scale == nullptr) != (bn_shift == nullptr)) return fail(GANET_E_INVALID, "%s: bn_scale and bn_shift go together", who);
  GA_TRY(check_dims5(who, N, C, D, H, W));
  const i64 n = (i64)N * C * D * H * W;
  const i64 slice = (i64)D * H * W;
  hipStream_t st = (hipStream_t)stream;
  const float *gs[4] = {g0, g1, g2, g3};
  // Fast form: no directional volume is kept.  `down` writes the output volume, `up` / `right` / `left` take the running
  // maximum in the copy-out of their tiles, `left` also applies the BatchNorm affine + ReLU: 11 V of traffic and four
  // launches instead of 13 V and five (A_ws is not touched).
  if (infer_fused_ok(x, g0, g1, g2, g3, out, N, C, D, W)) {
    GA_TRY(col_fwd(x, g0, out, N * C, D, H, W, 0, st, 0));
    GA_TRY(col_fwd(x, g1, out, N * C, D, H, W, 1, st, 1));
    GA_TRY(row_fwd(x, g2, out, N * C, D, H, W, 2, st, 1));
    return row_fwd(x, g3, out, N * C, D, H, W, 3, st, bn_scale ? 2 : 1, C, bn_scale, bn_shift);
  }
  if (!A_ws) return fail(GANET_E_INVALID, "%s: this shape needs the A_ws scratch (see ganet_sga_forward_infer_scratch)", who);
  for (int d = 0; d < 4; d++) GA_TRY(scan_fwd(x, gs[d], A_ws + d * n, N, C, D, H, W, d, st));
  const bool vec = slice % 4 == 0 && aligned16(A_ws, out);
  with_width<4>(vec, [&](auto v) {
    GA_LAUNCH((sga_merge_infer<decltype(v)::value>), dim3(ew_grid(vec ? n / 4 : n)), dim3(256), st, A_ws, A_ws + n, A_ws + 2 * n,
              A_ws + 3 * n, out, bn_scale, bn_shift, C, slice, n);
  });
  return check_launch("sga merge (inference)");
}

GA_EXPORT int ganet_sga_backward_scan(const float *g, const uint8_t *mask, const uint16_t *kp_dir,
                                      const float *grad_out, float *G, int N, int C, int D, int H,
                                      int W, int dir, void *stream)
{
  const char *who = "ganet_sga_backward_scan";
  GA_TRY(check_ptrs(who, g, mask, kp_dir, grad_out, G));
  GA_TRY(check_dir(who, dir));
  GA_TRY(check_dims5(who, N, C, D, H, W));
  return scan_bwdg(g, mask, kp_dir, grad_out, G, N, C, D, H, W, dir, (hipStream_t)stream);
}

GA_EXPORT int ganet_sga_backward_dir(const float *x, const float *g, const float *A,
                                     const uint8_t *mask, const uint16_t *kp_dir,
                                     const float *grad_out, float *G_ws, float *grad_x, float *gw,
                                     int N, int C, int D, int H, int W, int dir, int accumulate,
                                     void *stream)
{
  const char *who = "ganet_sga_backward_dir";
  GA_TRY(check_ptrs(who, x, g, A, mask, kp_dir, grad_out, G_ws, grad_x, gw));
  GA_TRY(check_dir(who, dir));
  GA_TRY(check_dims5(who, N, C, D, H, W));
  hipStream_t st = (hipStream_t)stream;
  GA_TRY(scan_bwdg(g, mask, kp_dir, grad_out, G_ws, N, C, D, H, W, dir, st));
  PointArgs pa = {};
  pa.G[0] = G_ws; pa.A[0] = A; pa.g[0] = g; pa.gw[0] = gw; pa.dir[0] = dir;
  return bwd_point(x, grad_x, pa, 1, N, C, D, H, W, accumulate ? 1 : 0, st);
}

namespace {
// the per-pixel kernel over all four directions, with the layout of G_down / G_up DECIDED BY THE CALLER (one read of the options
// per backward: ADVICE r4)
int backward_point_impl(const float *x, const float *g0, const float *g1, const float *g2, const float *g3,
                        const float *A_ws, const float *G_ws, float *grad_x, float *gw0, float *gw1, float *gw2,
                        float *gw3, int N, int C, int D, int H, int W, hipStream_t st, int tiled)
{
  const i64 n = (i64)N * C * D * H * W;
  const float *gs[4] = {g0, g1, g2, g3};
  float *gws[4] = {gw0, gw1, gw2, gw3};
  PointArgs pa = {};
  for (int d = 0; d < 4; d++) {
    pa.G[d] = G_ws + d * n; pa.A[d] = A_ws + d * n; pa.g[d] = gs[d]; pa.gw[d] = gws[d]; pa.dir[d] = d;
  }
  return bwd_point(x, grad_x, pa, 4, N, C, D, H, W, 0, st, tiled);
}
}  // namespace

GA_EXPORT int ganet_sga_backward_point(const float *x, const float *g0, const float *g1, const float *g2, const float *g3,
                                        const float *A_ws, const float *G_ws, float *grad_x, float *gw0, float *gw1, float *gw2,
                                        float *gw3, int N, int C, int D, int H, int W, void *stream)
{
  const char *who = "ganet_sga_backward_point";
  GA_TRY(check_ptrs(who, x, g0, g1, g2, g3, A_ws, G_ws, grad_x, gw0, gw1, gw2, gw3));
  GA_TRY(check_dims5(who, N, C, D, H, W));
  // pairs with ganet_sga_backward_scan_ws, which keeps G_down / G_up in the layout ganet_sga_workspace_layout reports
  return backward_point_impl(x, g0, g1, g2, g3, A_ws, G_ws, grad_x, gw0, gw1, gw2, gw3, N, C, D, H, W, (hipStream_t)stream,
                             sga_ws_tiled(N, C, D, H, W));
}

GA_EXPORT int ganet_sga_backward(const float *x, const float *g0, const float *g1, const float *g2,
                                 const float *g3, const float *A_ws, const uint8_t *mask,
                                 const uint16_t *kp, const float *grad_out, float *G_ws,
                                 float *grad_x, float *gw0, float *gw1, float *gw2, float *gw3,
                                 int N, int C, int D, int H, int W, void *stream)
{
  const char *who = "ganet_sga_backward";
  GA_TRY(check_ptrs(who, x, g0, g1, g2, g3, A_ws, mask, kp, grad_out, G_ws, grad_x, gw0, gw1, gw2, gw3));
  GA_TRY(check_dims5(who, N, C, D, H, W));
  const i64 n = (i64)N * C * D * H * W;
  const i64 npix = (i64)N * C * H * W;
  hipStream_t st = (hipStream_t)stream;
  const float *gs[4] = {g0, g1, g2, g3};
  // The layout of G_down / G_up is private to this call: decided ONCE, from the dimensions, the options and the alignment of what
  // the tiled column kernels touch (a contiguous but 4-byte aligned gradient takes the API layout and the generic scans).
  const int tiled = sga_ws_tiled(N, C, D, H, W, aligned16(g0, g1, grad_out, G_ws) && (n % 4 == 0), aligned4(mask));
  for (int d = 0; d < 4; d++)
    GA_TRY(scan_bwdg(gs[d], mask, kp + d * npix, grad_out, G_ws + d * n, N, C, D, H, W, d, st, d < 2 && tiled));
  return backward_point_impl(x, g0, g1, g2, g3, A_ws, G_ws, grad_x, gw0, gw1, gw2, gw3, N, C, D, H, W, st, tiled);
}

GA_EXPORT int ganet_sga_forward_compat(const float *x, const float *g0, const float *g1,
                                       const float *g2, const float *g3, float *temp_out,
                                       float *out, float *mask_f32, int N, int C, int D, int H,
                                       int W, void *stream)
{
  const char *who = "ganet_sga_forward_compat";
  GA_TRY(check_ptrs(who, x, g0, g1, g2, g3, temp_out, out, mask_f32));
  GA_TRY(check_dims5(who, N, C, D, H, W));
  const i64 n = (i64)N * C * D * H * W;
  hipStream_t st = (hipStream_t)stream;
  const float *gs[4] = {g0, g1, g2, g3};
  GA_TRY(scan_fwd(x, gs[0], out, N, C, D, H, W, 0, st));
  for (int d = 1; d < 4; d++) {
    GA_TRY(scan_fwd(x, gs[d], temp_out, N, C, D, H, W, d, st));
    GA_LAUNCH((sga_merge_running<float>), dim3(ew_grid(n)), dim3(256), st, temp_out, out, mask_f32,
              n, d, d == 1 ? 1 : 0);
    GA_TRY(check_launch("sga merge (compat)"));
  }
  return GANET_OK;
}

GA_EXPORT int ganet_sga_backward_compat(const float *x, const float *g0, const float *g1,
                                        const float *g2, const float *g3, float *temp_out,
                                        const float *mask_f32, float *max_idx,
                                        const float *grad_out, float *temp_grad, float *grad_x,
                                        float *gw0, float *gw1, float *gw2, float *gw3, int N,
                                        int C, int D, int H, int W, void *stream)
{
  const char *who = "ganet_sga_backward_compat";
  GA_TRY(check_ptrs(who, x, g0, g1, g2, g3, temp_out, mask_f32, max_idx, grad_out, temp_grad, grad_x, gw0, gw1, gw2, gw3));
  GA_TRY(check_dims5(who, N, C, D, H, W));
  if (D > 65535) return fail(GANET_E_UNSUPPORTED, "%s: D > 65535", who);
  const i64 npix = (i64)N * C * H * W;
  hipStream_t st = (hipStream_t)stream;
  // scratch roles as in the reference: temp_out = A_dir, temp_grad = adjoint volume,
  // max_idx = first-argmax per pixel (stored as uint16 in the first half of the buffer)
  uint16_t *kp = reinterpret_cast<uint16_t *>(max_idx);
  const float *gs[4] = {g0, g1, g2, g3};
  float *gws[4] = {gw0, gw1, gw2, gw3};
  const int order[4] = {3, 0, 1, 2};   // GANet_kernel.cu:1040-1128
  for (int i = 0; i < 4; i++) {
    const int d = order[i];
    if (d != 3) GA_TRY(scan_fwd(x, gs[d], temp_out, N, C, D, H, W, d, st));
    GA_LAUNCH(sga_argmax_px, dim3(px_grid(npix)), dim3(256), st, temp_out, kp, D, (i64)H * W, npix);
    GA_TRY(check_launch("sga argmax"));
    GA_TRY(scan_bwdg_f32mask(gs[d], mask_f32, kp, grad_out, temp_grad, N, C, D, H, W, d, st));
    PointArgs pa = {};
    pa.G[0] = temp_grad; pa.A[0] = temp_out; pa.g[0] = gs[d]; pa.gw[0] = gws[d]; pa.dir[0] = d;
    // gradInput is accumulated into (caller zero-fills); gw is written (each pixel once per direction)
    GA_TRY(bwd_point(x, grad_x, pa, 1, N, C, D, H, W, 1, st));
  }
  return GANET_OK;
}

GA_EXPORT int ganet_lga_forward(const float *x, const float *f, float *y, int B, int D, int H,
                                int W, int radius, void *stream)
{
  const char *who = "ganet_lga_forward";
  GA_TRY(check_ptrs(who, x, f, y));
  if (x == y) return fail(GANET_E_INVALID, "%s: y must not alias x", who);
  GA_TRY(check_lga(who, B, D, H, W, radius));
  int rc;
  with_int_else<3, 1, 2>(radius, [&](auto R) { rc = launch_lga_fwd<decltype(R)::value>(x, f, y, B, D, H, W, false, (hipStream_t)stream); });
  return rc;
}

namespace {
int lga_apply_paired_impl(const char *who, const float *x, const float *f, float *y, float *edge, int B, int D, int H, int W, int radius,
                          int transposed, int x_paired, int y_paired, void *stream)
{
  if (!x || !f || !y) return fail(GANET_E_INVALID, "%s: null pointer", who);
  if (x == y) return fail(GANET_E_INVALID, "%s: y must not alias x", who);
  GA_TRY(check_lga(who, B, D, H, W, radius));
  if (x_paired && y_paired) return fail(GANET_E_INVALID, "%s: at most one of x_paired / y_paired", who);
  if (radius != 2) return fail(GANET_E_UNSUPPORTED, "%s: radius 2 only", who);
  if (!x_paired && !y_paired) {
    if (edge) return fail(GANET_E_UNSUPPORTED, "%s: the edge-sum side channel belongs to the pair-interleaved forms", who);
    return launch_lga_fwd<2>(x, f, y, B, D, H, W, transposed != 0, (hipStream_t)stream);
  }
  return launch_lga_paired(x, f, y, B, D, H, W, transposed != 0, x_paired != 0, (hipStream_t)stream, edge);
}
}  // namespace

GA_EXPORT int ganet_lga_apply_paired(const float *x, const float *f, float *y, int B, int D, int H, int W, int radius,
                                     int transposed, int x_paired, int y_paired, void *stream)
{
  return lga_apply_paired_impl("ganet_lga_apply_paired", x, f, y, nullptr, B, D, H, W, radius, transposed, x_paired, y_paired, stream);
}

GA_EXPORT int ganet_lga_apply_paired_edges(const float *x, const float *f, float *y, float *edge, int B, int D, int H, int W, int radius,
                                           int transposed, int x_paired, int y_paired, void *stream)
{
  const char *who = "ganet_lga_apply_paired_edges";
  if (!edge) return fail(GANET_E_INVALID, "%s: null edge buffer", who);
  return lga_apply_paired_impl(who, x, f, y, edge, B, D, H, W, radius, transposed, x_paired, y_paired, stream);
}

GA_EXPORT int ganet_lga_filter_grad_paired(const float *x, const float *gy, float *gf, int B, int D, int H, int W, int radius,
                                           int accumulate_gf, int x_paired, int gy_paired, void *stream)
{
  const char *who = "ganet_lga_filter_grad_paired";
  GA_TRY(check_ptrs(who, x, gy, gf));
  GA_TRY(check_lga(who, B, D, H, W, radius));
  if (x_paired && gy_paired) return fail(GANET_E_INVALID, "%s: at most one of x_paired / gy_paired", who);
  if (radius != 2) return fail(GANET_E_UNSUPPORTED, "%s: radius 2 only", who);
  if (!x_paired && !gy_paired) return launch_lga_gf<2>(x, gy, gf, B, D, H, W, accumulate_gf != 0, (hipStream_t)stream);
  return launch_lga_gf_paired(x, gy, gf, B, D, H, W, accumulate_gf != 0, x_paired != 0, (hipStream_t)stream);
}

GA_EXPORT int ganet_lga_forward_regress(const float *x, const float *f, float *y, float *snorm, float *sdy, int B, int D,
                                        int H, int W, int radius, void *stream)
{
  const char *who = "ganet_lga_forward_regress";
  GA_TRY(check_ptrs(who, x, f, snorm, sdy));
  if (x == y) return fail(GANET_E_INVALID, "%s: y must not alias x", who);
  GA_TRY(check_lga(who, B, D, H, W, radius));
  int rc;
  with_int_else<3, 1, 2>(radius, [&](auto R) { rc = launch_lga_fwd_regress<decltype(R)::value>(x, f, y, snorm, sdy, B, D, H, W, (hipStream_t)stream); });
  return rc;
}

GA_EXPORT int ganet_lga_backward(const float *x, const float *f, const float *gy, float *gx,
                                 float *gf, int B, int D, int H, int W, int radius,
                                 int accumulate_gf, void *stream)
{
  const char *who = "ganet_lga_backward";
  GA_TRY(check_ptrs(who, x, f, gy, gx, gf));
  if (gx == gy) return fail(GANET_E_INVALID, "%s: gx must not alias gy", who);
  GA_TRY(check_lga(who, B, D, H, W, radius));
  hipStream_t st = (hipStream_t)stream;
  const int acc = accumulate_gf ? 1 : 0;
  // filter gradient first: it is the only consumer of x, so gx may alias x afterwards
  // (the reference's chained LGA2/LGA3 backward relies on that, functions/GANet.py:197).
  // (the two kernels of a pass on two streams: measured slower, 0.215 -> 0.238 ms, profiles/r2m_*)
  int rc;
  with_int_else<3, 1, 2>(radius, [&](auto R) {
    rc = launch_lga_gf<decltype(R)::value>(x, gy, gf, B, D, H, W, acc, st);
    if (rc == GANET_OK) rc = launch_lga_fwd<decltype(R)::value>(gy, f, gx, B, D, H, W, true, st);
  });
  return rc;
}

GA_EXPORT int ganet_cost_volume_forward(const float *x, const float *y, float *cost, int N, int C,
                                        int Dn, int H, int W, void *stream)
{
  const char *who = "ganet_cost_volume_forward";
  GA_TRY(check_ptrs(who, x, y, cost));
  GA_TRY(check_positive(who, N, C, Dn, H, W));
  const i64 n = (i64)N * 2 * C * Dn * H * W;
  if (W % 4 == 0 && aligned16(x, cost))
    GA_LAUNCH(cost_volume_fwd4, dim3(ew_grid(n / 4)), dim3(256), (hipStream_t)stream, x, y, cost, N, C, Dn, H, W);
  else
    GA_LAUNCH(cost_volume_fwd<float>, dim3(ew_grid(n)), dim3(256), (hipStream_t)stream, x, y, cost, N, C, Dn, H, W);
  return check_launch("cost volume forward");
}

GA_EXPORT int ganet_cost_volume_backward(const float *grad_cost, float *grad_x, float *grad_y,
                                         int N, int C, int Dn, int H, int W, void *stream)
{
  const char *who = "ganet_cost_volume_backward";
  GA_TRY(check_ptrs(who, grad_cost, grad_x, grad_y));
  GA_TRY(check_positive(who, N, C, Dn, H, W));
  const i64 n = (i64)N * C * H * W;
  GA_LAUNCH(cost_volume_bwd, dim3(ew_grid(n)), dim3(256), (hipStream_t)stream, grad_cost, grad_x, grad_y, N, C, Dn, H, W);
  return check_launch("cost volume backward");
}

GA_EXPORT int ganet_disparity_regression_forward(const float *x, float *out, int N, int Dn, int H,
                                                 int W, void *stream)
{
  const char *who = "ganet_disparity_regression_forward";
  GA_TRY(check_ptrs(who, x, out));
  GA_TRY(check_positive(who, N, Dn, H, W));
  const i64 HW = (i64)H * W;
  GA_LAUNCH(disp_regression_fwd, dim3(ew_grid((i64)N * HW)), dim3(256), (hipStream_t)stream, x, out, N, Dn, HW);
  return check_launch("disparity regression forward");
}

GA_EXPORT int ganet_disparity_regression_backward(const float *grad_out, float *grad_x, int N,
                                                  int Dn, int H, int W, void *stream)
{
  const char *who = "ganet_disparity_regression_backward";
  GA_TRY(check_ptrs(who, grad_out, grad_x));
  GA_TRY(check_positive(who, N, Dn, H, W));
  const i64 HW = (i64)H * W;
  if (HW % 4 == 0 && aligned16(grad_out, grad_x))
    GA_LAUNCH(disp_regression_bwd4, dim3(ew_grid((i64)N * (HW / 4))), dim3(256), (hipStream_t)stream, grad_out, grad_x, N, Dn, HW);
  else
    GA_LAUNCH(disp_regression_bwd, dim3(ew_grid((i64)N * Dn * HW)), dim3(256), (hipStream_t)stream, grad_out, grad_x, N, Dn, HW);
  return check_launch("disparity regression backward");
}

// ---- callers' normalisations folded into single kernels ------------------------
namespace {
int check_norm(const char *who, int N, int G, int C, int K, int H, int W)
{
  if (N <= 0 || G <= 0 || C <= 0 || K <= 0 || H <= 0 || W <= 0)
    return fail(GANET_E_INVALID, "%s: non-positive size N=%d G=%d C=%d K=%d H=%d W=%d", who, N, G, C, K, H, W);
  if (G > 4) return fail(GANET_E_UNSUPPORTED, "%s: at most 4 groups, got %d", who, G);
  return GANET_OK;
}
}  // namespace

GA_EXPORT int ganet_l1_normalize_forward(const float *x, float *y0, float *y1, float *y2, float *y3,
                                         int N, int G, int C, int K, int H, int W, void *stream)
{
  const char *who = "ganet_l1_normalize_forward";
  GA_TRY(check_norm(who, N, G, C, K, H, W));
  float *ys[4] = {y0, y1, y2, y3};
  GA_TRY(check_ptrs(who, x));
  NormPtrs p = {};
  for (int g = 0; g < 4; g++) {
    if (g < G && !ys[g]) return fail(GANET_E_INVALID, "%s: null output %d", who, g);
    p.y[g] = ys[g < G ? g : 0];
  }
  const i64 HW = (i64)H * W;
  const dim3 grid(ew_grid((i64)N * G * C * HW)), block(256);
  hipStream_t st = (hipStream_t)stream;
  with_int_else<0, 5, 75>(K, [&](auto KC) { GA_LAUNCH((l1norm_fwd<decltype(KC)::value>), grid, block, st, x, p, N, G, C, K, HW); });
  return check_launch("l1 normalise forward");
}

GA_EXPORT int ganet_l1_normalize_backward(const float *x, const float *gy0, const float *gy1,
                                          const float *gy2, const float *gy3, float *grad_x,
                                          int N, int G, int C, int K, int H, int W, void *stream)
{
  const char *who = "ganet_l1_normalize_backward";
  GA_TRY(check_norm(who, N, G, C, K, H, W));
  const float *gs[4] = {gy0, gy1, gy2, gy3};
  GA_TRY(check_ptrs(who, x, grad_x));
  NormPtrs p = {};
  for (int g = 0; g < 4; g++) {
    if (g < G && !gs[g]) return fail(GANET_E_INVALID, "%s: null gradient %d", who, g);
    p.gy[g] = gs[g < G ? g : 0];
  }
  const i64 HW = (i64)H * W;
  const dim3 grid(ew_grid((i64)N * G * C * HW)), block(256);
  hipStream_t st = (hipStream_t)stream;
  with_int_else<0, 5, 75>(K, [&](auto KC) { GA_LAUNCH((l1norm_bwd<decltype(KC)::value>), grid, block, st, x, p, grad_x, N, G, C, K, HW); });
  return check_launch("l1 normalise backward");
}

GA_EXPORT int ganet_norm_disparity_regression_forward(const float *x, float *out, float *snorm, int N,
                                                      int Dn, int H, int W, void *stream)
{
  const char *who = "ganet_norm_disparity_regression_forward";
  GA_TRY(check_ptrs(who, x, out, snorm));
  GA_TRY(check_positive(who, N, Dn, H, W));
  const i64 HW = (i64)H * W;
  GA_LAUNCH(norm_disp_regression_fwd, dim3(ew_grid((i64)N * HW)), dim3(256), (hipStream_t)stream, x, out, snorm, N, Dn, HW);
  return check_launch("normalised disparity regression forward");
}

GA_EXPORT int ganet_norm_disparity_regression_backward(const float *x, const float *out,
                                                       const float *snorm, const float *grad_out,
                                                       float *grad_x, int N, int Dn, int H, int W,
                                                       void *stream)
{
  const char *who = "ganet_norm_disparity_regression_backward";
  GA_TRY(check_ptrs(who, x, out, snorm, grad_out, grad_x));
  GA_TRY(check_positive(who, N, Dn, H, W));
  const i64 HW = (i64)H * W;
  if (HW % 4 == 0 && aligned16(x, out, snorm, grad_out, grad_x))
    GA_LAUNCH(norm_disp_regression_bwd4, dim3(ew_grid((i64)N * (HW / 4))), dim3(256), (hipStream_t)stream, x, out, snorm,
              grad_out, grad_x, N, Dn, HW);
  else
    GA_LAUNCH(norm_disp_regression_bwd, dim3(ew_grid((i64)N * Dn * HW)), dim3(256), (hipStream_t)stream, x, out, snorm,
              grad_out, grad_x, N, Dn, HW);
  return check_launch("normalised disparity regression backward");
}

namespace {
int check_up(const char *who, const void *a, const void *b, int S, int Di, int Hi, int Wi, int Do, int Ho, int Wo)
{
  GA_TRY(check_ptrs(who, a, b));
  return check_positive(who, S, Di, Hi, Wi, Do, Ho, Wo);
}
UpAxis up_axis(int in, int out)
{
  UpAxis a;
  a.in = in; a.out = out;
  a.scale = (float)in / (float)out;      // ATen: area_pixel_compute_scale<float>(in, out, align_corners = false, nullopt)
  return a;
}
}  // namespace

GA_EXPORT int ganet_trilinear_upsample_forward(const float *x, float *y, int S, int Di, int Hi, int Wi, int Do, int Ho,
                                               int Wo, void *stream)
{
  GA_TRY(check_up("ganet_trilinear_upsample_forward", x, y, S, Di, Hi, Wi, Do, Ho, Wo));
  const i64 total = (i64)S * Do * Ho * Wo;
  GA_LAUNCH(trilinear_up_fwd, dim3(ew_grid(total)), dim3(256), (hipStream_t)stream, x, y, (i64)S, up_axis(Di, Do),
            up_axis(Hi, Ho), up_axis(Wi, Wo));
  return check_launch("trilinear upsample forward");
}

GA_EXPORT int ganet_trilinear_upsample_backward(const float *grad_y, float *grad_x, int S, int Di, int Hi, int Wi, int Do,
                                                int Ho, int Wo, void *stream)
{
  GA_TRY(check_up("ganet_trilinear_upsample_backward", grad_y, grad_x, S, Di, Hi, Wi, Do, Ho, Wo));
  const i64 total = (i64)S * Di * Hi * Wi;
  GA_LAUNCH(trilinear_up_bwd, dim3(ew_grid(total)), dim3(256), (hipStream_t)stream, grad_y, grad_x, (i64)S, up_axis(Di, Do),
            up_axis(Hi, Ho), up_axis(Wi, Wo));
  return check_launch("trilinear upsample backward");
}

GA_EXPORT int ganet_softmin_forward(const float *x, float *y, int N, int Dn, int H, int W, void *stream)
{
  const char *who = "ganet_softmin_forward";
  GA_TRY(check_ptrs(who, x, y));
  GA_TRY(check_positive(who, N, Dn, H, W));
  const i64 HW = (i64)H * W;
  with_width<4>(HW % 4 == 0 && aligned16(x, y), [&](auto v) {
    constexpr int V = decltype(v)::value;
    GA_LAUNCH(softmin_fwd<V>, dim3(ew_grid((i64)N * HW / V)), dim3(256), (hipStream_t)stream, x, y, N, Dn, HW);
  });
  return check_launch("softmin forward");
}

GA_EXPORT int ganet_softmin_backward(const float *y, const float *grad_y, float *grad_x, int N, int Dn, int H,
                                     int W, void *stream)
{
  const char *who = "ganet_softmin_backward";
  GA_TRY(check_ptrs(who, y, grad_y, grad_x));
  GA_TRY(check_positive(who, N, Dn, H, W));
  const i64 HW = (i64)H * W;
  if (HW % 4 == 0 && aligned16(y, grad_y, grad_x))
    GA_LAUNCH(softmin_bwd4, dim3(ew_grid((i64)N * HW / 4)), dim3(256), (hipStream_t)stream, y, grad_y, grad_x, N, Dn, HW);
  else
    GA_LAUNCH(softmin_bwd, dim3(ew_grid((i64)N * HW)), dim3(256), (hipStream_t)stream, y, grad_y, grad_x, N, Dn, HW);
  return check_launch("softmin backward");
}

GA_EXPORT int ganet_softmin_regression_forward(const float *x, float *out, float *mx, float *ssum, int N, int Dn,
                                               int H, int W, void *stream)
{
  const char *who = "ganet_softmin_regression_forward";
  GA_TRY(check_ptrs(who, x, out, mx, ssum));
  GA_TRY(check_positive(who, N, Dn, H, W));
  const i64 HW = (i64)H * W;
  GA_LAUNCH(softmin_regression_fwd, dim3(ew_grid((i64)N * HW)), dim3(256), (hipStream_t)stream, x, out, mx, ssum, N, Dn, HW);
  return check_launch("softmin regression forward");
}

GA_EXPORT int ganet_softmin_regression_backward(const float *x, const float *out, const float *mx,
                                                const float *ssum, const float *grad_out, float *grad_x,
                                                int N, int Dn, int H, int W, void *stream)
{
  const char *who = "ganet_softmin_regression_backward";
  GA_TRY(check_ptrs(who, x, out, mx, ssum, grad_out, grad_x));
  GA_TRY(check_positive(who, N, Dn, H, W));
  const i64 HW = (i64)H * W;
  GA_LAUNCH(softmin_regression_bwd, dim3(ew_grid((i64)N * HW)), dim3(256), (hipStream_t)stream, x, out, mx, ssum,
            grad_out, grad_x, N, Dn, HW);
  return check_launch("softmin regression backward");
}

// ---- Disp.forward behind conv32x1 without the up-sampled volume (models/GANet_deep.py:214-219; disp_tail_kernels.h) ----
namespace {
int check_up_tail(const char *who, int N, int Di, int Hi, int Wi, int Do, int Ho, int Wo)
{
  GA_TRY(check_positive(who, N, Di, Hi, Wi, Do, Ho, Wo));
  if (Do >= (1 << 24)) return fail(GANET_E_INVALID, "%s: Do=%d, the disparity index must be exact in float (Do < 2^24)", who, Do);
  return GANET_OK;
}
}  // namespace

// models/GANet_deep.py:214-219
GA_EXPORT int ganet_up_softmin_regression_forward(const float *x, float *out, float *mx, float *ssum, int N, int Di, int Hi,
                                                  int Wi, int Do, int Ho, int Wo, void *stream)
{
  const char *who = "ganet_up_softmin_regression_forward";
  GA_TRY(check_ptrs(who, x, out, mx, ssum));
  GA_TRY(check_up_tail(who, N, Di, Hi, Wi, Do, Ho, Wo));
  GA_LAUNCH(up_softmin_regression_fwd, dim3(ew_grid((i64)N * Ho * Wo)), dim3(256), (hipStream_t)stream, x, out, mx, ssum,
            (i64)N, up_axis(Di, Do), up_axis(Hi, Ho), up_axis(Wi, Wo));
  return check_launch("up-sampled softmin regression forward");
}

// models/GANet_deep.py:214-219 (adjoint): the column pass into gcol_ws [N,Di,Ho,Wo], then the H x W gather of
// trilinear_up_bwd on N*Di slices of depth 1 -> 1
GA_EXPORT int ganet_up_softmin_regression_backward(const float *x, const float *out, const float *mx, const float *ssum,
                                                   const float *grad_out, float *gcol_ws, float *grad_x, int N, int Di,
                                                   int Hi, int Wi, int Do, int Ho, int Wo, void *stream)
{
  const char *who = "ganet_up_softmin_regression_backward";
  GA_TRY(check_ptrs(who, x, out, mx, ssum, grad_out, gcol_ws, grad_x));
  GA_TRY(check_up_tail(who, N, Di, Hi, Wi, Do, Ho, Wo));
  GA_LAUNCH(up_softmin_regression_bwd_cols, dim3(ew_grid((i64)N * Ho * Wo)), dim3(256), (hipStream_t)stream, x, out, mx, ssum,
            grad_out, gcol_ws, (i64)N, up_axis(Di, Do), up_axis(Hi, Ho), up_axis(Wi, Wo));
  GA_TRY(check_launch("up-sampled softmin regression backward (columns)"));
  const i64 S = (i64)N * Di;
  GA_LAUNCH(trilinear_up_bwd, dim3(ew_grid(S * Hi * Wi)), dim3(256), (hipStream_t)stream, (const float *)gcol_ws, grad_x, S,
            up_axis(1, 1), up_axis(Hi, Ho), up_axis(Wi, Wo));
  return check_launch("up-sampled softmin regression backward (gather)");
}

// ---- the tails' conv32x1: Conv3d(C, 1, 3, 1, 1, bias=False) (models/GANet_deep.py:212, 232; disp_conv_kernels.h) ----
namespace {
int check_disp_conv(const char *who, int N, int C, int D, int H, int W, DispConvGeom &g, dim3 &grid)
{
  GA_TRY(check_ncdhw(who, N, C, D, H, W));
  if (C > DCV_MAX_C) return fail(GANET_E_UNSUPPORTED, "%s: C=%d, at most %d channels", who, C, DCV_MAX_C);
  g.N = N; g.C = C; g.D = D; g.H = H; g.W = W;
  g.W4 = (W + DCV_PX - 1) / DCV_PX;
  g.groups = (i64)H * g.W4;
  const i64 bx = (g.groups + 63) / 64, by = ((i64)D + DCV_DEPTH - 1) / DCV_DEPTH;
  if (bx > 0x7fffffff || by > 65535 || N > 65535)
    return fail(GANET_E_UNSUPPORTED, "%s: N=%d D=%d H=%d W=%d is beyond the launch grid", who, N, D, H, W);
  grid = dim3((unsigned)bx, (unsigned)by, (unsigned)N);
  return GANET_OK;
}
i64 disp_conv_rows(const dim3 &grid) { return (i64)grid.x * grid.y * grid.z; }
bool type16(int t) { return t == GANET_F16 || t == GANET_BF16; }

// The launch of each direction, once, behind the entry of every storage type ST of the big volume (x, grad_x): the entry has
// checked its operands and decides `vec`; `what` is its name for the launch.
template <typename ST>
int launch_disp_conv_fwd(const void *x, const float *weight, float *y, const DispConvGeom &g, dim3 grid, bool vec, void *stream,
                         const char *what)
{
  with_flags([&](auto v) {
    GA_LAUNCH((disp_conv_fwd<ST, decltype(v)::value>), grid, dim3(64 * DCV_WAVES), (hipStream_t)stream, (const typename ST::T *)x, weight, y, g);
  }, vec);
  return check_launch(what);
}

template <typename ST>
int launch_disp_conv_bwd_data(const float *grad_y, const float *weight, void *grad_x, const DispConvGeom &g, dim3 grid, bool vec,
                              void *stream, const char *what)
{
  with_flags([&](auto v) {
    GA_LAUNCH((disp_conv_bwd_data<ST, decltype(v)::value>), grid, dim3(64 * DCV_WAVES), (hipStream_t)stream, grad_y, weight,
              (typename ST::T *)grad_x, g);
  }, vec);
  return check_launch(what);
}

// ... and the second stage: the workspace rows added up in fp64
template <typename ST>
int launch_disp_conv_bwd_weight(const char *who, const void *x, const float *grad_y, float *workspace, float *grad_weight,
                                const DispConvGeom &g, dim3 grid, bool vec, void *stream, const char *what)
{
  const i64 rows = disp_conv_rows(grid);
  if (rows * 27 * g.C > 0x7fffffff) return fail(GANET_E_UNSUPPORTED, "%s: the workspace is beyond ganet_disp_conv_workspace's answer", who);
  hipStream_t st = (hipStream_t)stream;
  with_flags([&](auto v) {
    GA_LAUNCH((disp_conv_bwd_weight_partials<ST, decltype(v)::value>), grid, dim3(64 * DCV_WAVES), st, (const typename ST::T *)x, grad_y,
              workspace, g);
  }, vec);
  GA_TRY(check_launch(what));
  const int K = 27 * g.C;
  GA_LAUNCH(disp_conv_bwd_weight_sum, dim3((unsigned)((K + DCV_SUM_COLS - 1) / DCV_SUM_COLS)),
            dim3(DCV_SUM_COLS * DCV_SUM_SLICES), st, (const float *)workspace, grad_weight, K, rows);
  return check_launch("disp conv backward (weight sum)");
}
}  // namespace

GA_EXPORT int ganet_disp_conv_workspace(int N, int C, int D, int H, int W)
{
  const char *who = "ganet_disp_conv_workspace";
  DispConvGeom g;
  dim3 grid;
  GA_TRY(check_disp_conv(who, N, C, D, H, W, g, grid));
  const i64 n = disp_conv_rows(grid) * 27 * C;
  if (n > 0x7fffffff) return fail(GANET_E_UNSUPPORTED, "%s: %lld elements do not fit the answer", who, n);
  return (int)n;
}

GA_EXPORT int ganet_disp_conv_forward(const float *x, const float *weight, float *y, int N, int C, int D, int H, int W,
                                      void *stream)
{
  const char *who = "ganet_disp_conv_forward";
  GA_TRY(check_ptrs(who, x, weight, y));
  DispConvGeom g;
  dim3 grid;
  GA_TRY(check_disp_conv(who, N, C, D, H, W, g, grid));
  if (y == x || y == weight) return fail(GANET_E_INVALID, "%s: y must not alias an input", who);
  return launch_disp_conv_fwd<st_f32>(x, weight, y, g, grid, W % 4 == 0 && aligned16(x, y), stream, "disp conv forward");
}

GA_EXPORT int ganet_disp_conv_backward_data(const float *grad_y, const float *weight, float *grad_x, int N, int C, int D,
                                            int H, int W, void *stream)
{
  const char *who = "ganet_disp_conv_backward_data";
  GA_TRY(check_ptrs(who, grad_y, weight, grad_x));
  DispConvGeom g;
  dim3 grid;
  GA_TRY(check_disp_conv(who, N, C, D, H, W, g, grid));
  if (grad_x == grad_y || grad_x == weight) return fail(GANET_E_INVALID, "%s: grad_x must not alias an input", who);
  return launch_disp_conv_bwd_data<st_f32>(grad_y, weight, grad_x, g, grid, W % 4 == 0 && aligned16(grad_y, grad_x), stream,
                                           "disp conv backward (data)");
}

GA_EXPORT int ganet_disp_conv_backward_weight(const float *x, const float *grad_y, float *workspace, float *grad_weight,
                                              int N, int C, int D, int H, int W, void *stream)
{
  const char *who = "ganet_disp_conv_backward_weight";
  GA_TRY(check_ptrs(who, x, grad_y, workspace, grad_weight));
  DispConvGeom g;
  dim3 grid;
  GA_TRY(check_disp_conv(who, N, C, D, H, W, g, grid));
  if (grad_weight == x || grad_weight == grad_y || workspace == x || workspace == grad_y || workspace == grad_weight)
    return fail(GANET_E_INVALID, "%s: workspace and grad_weight must not alias anything", who);
  return launch_disp_conv_bwd_weight<st_f32>(who, x, grad_y, workspace, grad_weight, g, grid, W % 4 == 0 && aligned16(x, grad_y), stream,
                                             "disp conv backward (weight partials)");
}

// ---- SGABlock's residual epilogue (models/GANet_deep.py:270-277) --------------------
namespace {
// x: enough 256-thread blocks per slice to fill the chip about four times over, y: the slices
dim3 residual_grid(i64 S, i64 per_slice)
{
  i64 gx = (per_slice + 255) / 256;
  const i64 want = (256 * 16 + S - 1) / S;
  if (gx > want) gx = want;
  if (gx < 1) gx = 1;
  return dim3((unsigned)gx, (unsigned)(S < 65535 ? S : 65535));
}
}  // namespace

GA_EXPORT int ganet_residual_relu_forward(const float *t, const float *rem, const float *bn_scale, const float *bn_shift,
                                          float *y, int N, int C, int D, int H, int W, void *stream)
{
  const char *who = "ganet_residual_relu_forward";
  GA_TRY(check_ncdhw(who, N, C, D, H, W));
  GA_TRY(check_ptrs(who, t, rem, y));
  if ((bn_scale == nullptr) != (bn_shift == nullptr)) return fail(GANET_E_INVALID, "%s: bn_scale and bn_shift come together", who);
  const i64 S = (i64)N * C, slice = (i64)D * H * W;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = slice % 4 == 0 && aligned16(t, rem, y);
  const dim3 grid = residual_grid(S, vec ? slice / 4 : slice);
  with_flags([&](auto v) { GA_LAUNCH((residual_relu_fwd<decltype(v)::value>), grid, dim3(256), st, t, rem, bn_scale, bn_shift, y, S, C, slice); }, vec);
  return check_launch("residual + relu forward");
}

GA_EXPORT int ganet_residual_relu_backward(const float *y, const float *grad_y, const float *bn_scale, float *grad_t,
                                           float *grad_rem, int N, int C, int D, int H, int W, void *stream)
{
  const char *who = "ganet_residual_relu_backward";
  GA_TRY(check_ncdhw(who, N, C, D, H, W));
  GA_TRY(check_ptrs(who, y, grad_y, grad_rem));
  if (bn_scale && !grad_t) return fail(GANET_E_INVALID, "%s: a scaled gradient needs a buffer of its own (grad_t)", who);
  const i64 S = (i64)N * C, slice = (i64)D * H * W;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = slice % 4 == 0 && aligned16(y, grad_y, grad_rem, grad_t);
  const dim3 grid = residual_grid(S, vec ? slice / 4 : slice);
  with_flags([&](auto v) { GA_LAUNCH((residual_relu_bwd<decltype(v)::value>), grid, dim3(256), st, y, grad_y, bn_scale, grad_t, grad_rem, S, C, slice); }, vec);
  return check_launch("residual + relu backward");
}

// ---- the training criterion and its error read-out (train.py:100-126, evaluation.py:199-202) --------------
namespace {
int check_loss(const char *who, const float *const *p, const float *target, const float *params, int N, int H, int W, int P,
               const int *kind, int mask_mode)
{
  if (N <= 0 || H <= 0 || W <= 0) return fail(GANET_E_INVALID, "%s: non-positive size N=%d H=%d W=%d", who, N, H, W);
  if (P < 1 || P > 3) return fail(GANET_E_INVALID, "%s: P=%d, 1 <= P <= 3", who, P);
  if (mask_mode != 0 && mask_mode != 1) return fail(GANET_E_INVALID, "%s: mask_mode=%d (0: t < hi, 1: lo <= t <= hi)", who, mask_mode);
  if (!target || !params) return fail(GANET_E_INVALID, "%s: null pointer", who);
  for (int k = 0; k < P; k++) {
    if (!p[k]) return fail(GANET_E_INVALID, "%s: null prediction %d", who, k);
    if (kind[k] != 0 && kind[k] != 1) return fail(GANET_E_INVALID, "%s: kind%d=%d (0: smooth-L1, 1: MyLoss2)", who, k, kind[k]);
  }
  if ((i64)N * H * W >= (1 << 24))
    return fail(GANET_E_UNSUPPORTED, "%s: %lld pixels; counts are reported as floats, which holds below 2^24", who, (long long)N * H * W);
  return GANET_OK;
}
}  // namespace

GA_EXPORT int ganet_disparity_loss_workspace(int N, int H, int W)
{
  const char *who = "ganet_disparity_loss_workspace";
  GA_TRY(check_positive(who, N, H, W));
  if ((i64)N * H * W >= (1 << 24)) return fail(GANET_E_UNSUPPORTED, "%s: 2^24 pixels or more", who);
  return LOSS_MAX_BLOCKS * LOSS_ROW;
}

GA_EXPORT int ganet_disparity_loss_forward(const float *p0, const float *p1, const float *p2, const float *target,
                                           const float *params, double *workspace, float *loss, float *stats, int N, int H,
                                           int W, int P, int kind0, int kind1, int kind2, int mask_mode, void *stream)
{
  const char *who = "ganet_disparity_loss_forward";
  const float *ps[3] = {p0, p1, p2};
  const int kinds[3] = {kind0, kind1, kind2};
  GA_TRY(check_loss(who, ps, target, params, N, H, W, P, kinds, mask_mode));
  GA_TRY(check_ptrs(who, workspace, loss, stats));
  LossMaps m = {};
  bool vec = aligned16(target);
  for (int k = 0; k < P; k++) { m.p[k] = ps[k]; m.kind[k] = kinds[k]; vec = vec && aligned16(ps[k]); }
  const i64 total = (i64)N * H * W;
  vec = vec && total % 4 == 0;
  const i64 want = ((vec ? total / 4 : total) + LOSS_BLOCK - 1) / LOSS_BLOCK;
  const int rows = (int)(want < LOSS_MAX_BLOCKS ? want : LOSS_MAX_BLOCKS);
  hipStream_t st = (hipStream_t)stream;
  with_width<4>(vec, [&](auto V) { GA_LAUNCH((loss_partials<decltype(V)::value>), dim3(rows), dim3(LOSS_BLOCK), st, m, target, params, workspace, total, P, mask_mode); });
  GA_TRY(check_launch("disparity loss partial sums"));
  GA_LAUNCH(loss_finish, dim3(1), dim3(64), st, workspace, rows, params, P, loss, stats);
  return check_launch("disparity loss finish");
}

GA_EXPORT int ganet_disparity_loss_backward(const float *p0, const float *p1, const float *p2, const float *target,
                                            const float *params, const float *stats, const float *grad_loss, float *g0,
                                            float *g1, float *g2, int N, int H, int W, int P, int kind0, int kind1, int kind2,
                                            int mask_mode, void *stream)
{
  const char *who = "ganet_disparity_loss_backward";
  const float *ps[3] = {p0, p1, p2};
  float *gs[3] = {g0, g1, g2};
  const int kinds[3] = {kind0, kind1, kind2};
  GA_TRY(check_loss(who, ps, target, params, N, H, W, P, kinds, mask_mode));
  GA_TRY(check_ptrs(who, stats, grad_loss));
  LossMaps m = {};
  bool vec = aligned16(target), any = false;
  for (int k = 0; k < P; k++) {
    m.p[k] = ps[k]; m.g[k] = gs[k]; m.kind[k] = kinds[k];
    if (gs[k]) { any = true; vec = vec && aligned16(ps[k], gs[k]); }
  }
  if (!any) return GANET_OK;
  const i64 total = (i64)N * H * W;
  vec = vec && total % 4 == 0;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(ew_grid(vec ? total / 4 : total));
  with_width<4>(vec, [&](auto V) { GA_LAUNCH((loss_bwd<decltype(V)::value>), grid, dim3(256), st, m, target, params, stats, grad_loss, total, P, mask_mode); });
  return check_launch("disparity loss backward");
}

// ---- training-mode BatchNorm + (residual) + ReLU (models/GANet_deep.py:35-41, :270-277) ---------------------------------------
namespace {
int bn_rows_cap(int C)
{
  const int want = BN_TARGET_BLOCKS / C;
  return want < 1 ? 1 : (want < BN_MAX_ROWS ? want : BN_MAX_ROWS);
}

// rows per channel: Rs blocks along a slice (each lane at least one trip of V elements), the rest of the cap over the channel's N slices
int bn_geom(const char *who, int N, int C, int S, int V, bool training, BnGeom *g)
{
  if (N <= 0 || C <= 0 || S <= 0) return fail(GANET_E_INVALID, "%s: non-positive size N=%d C=%d S=%d", who, N, C, S);
  if (training && (i64)N * S == 1) return fail(GANET_E_INVALID, "%s: one value per channel (N * S = 1): batch statistics need more", who);
  if (C > 65535) return fail(GANET_E_UNSUPPORTED, "%s: C=%d > 65535 (grid.y)", who, C);
  const int cap = bn_rows_cap(C);
  const i64 want = (S / V + BN_BLOCK - 1) / BN_BLOCK;
  g->N = N; g->C = C; g->S = S;
  g->Rs = (int)(want < cap ? want : cap);
  g->Rn = cap / g->Rs < N ? cap / g->Rs : N;
  return GANET_OK;
}
float bn_float(int bits)
{
  float f;
  memcpy(&f, &bits, sizeof f);
  return f;
}

// The launches of each pass, once, behind the entries of every storage type (bn_kernels.h: Tx of x and grad_x, Ty of y and
// grad_y; Tr of the affine form's rem).  The entry has checked its operands, made g for V elements per lane and names its
// launches (what_*) for check_launch.
struct BnForwardArgs {
  const void *x;
  const float *rem, *weight, *bias;
  float *running_mean, *running_var;
  double *workspace;
  void *y;
  float *save_mean, *save_invstd;
  int momentum_bits, eps_bits, relu;
  void *stream;
  const char *what_sums, *what_apply;
};

template <typename Tx, typename Ty, int V>
int launch_bn_train_forward(const BnForwardArgs &a, const BnGeom &g)
{
  const typename Tx::T *xp = (const typename Tx::T *)a.x;
  const float momentum = bn_float(a.momentum_bits), eps = bn_float(a.eps_bits);
  const dim3 grid(g.Rs * g.Rn, g.C);
  hipStream_t st = (hipStream_t)a.stream;
  GA_LAUNCH((bn_stat_partials<Tx, V>), grid, dim3(BN_BLOCK), st, xp, a.workspace, g);
  GA_TRY(check_launch(a.what_sums));
  // (the apply pass of a 16-bit x is a sibling kernel: mixed_train_kernels.h says why)
  if constexpr (std::is_same_v<Tx, st_f32>)
    GA_LAUNCH((bn_train_apply<V>), grid, dim3(BN_BLOCK), st, xp, a.rem, a.weight, a.bias, a.running_mean, a.running_var, a.workspace,
              (float *)a.y, a.save_mean, a.save_invstd, g, momentum, eps, a.relu);
  else
    GA_LAUNCH((bn_train_apply_mixed<Tx, Ty, V>), grid, dim3(BN_BLOCK), st, xp, a.rem, a.weight, a.bias, a.running_mean, a.running_var,
              a.workspace, (typename Ty::T *)a.y, a.save_mean, a.save_invstd, g, momentum, eps, a.relu);
  return check_launch(a.what_apply);
}

struct BnBackwardArgs {
  const void *x;
  const float *rem;
  const void *grad_y;
  const float *weight, *bias, *save_mean, *save_invstd;
  double *workspace;
  void *grad_x;
  float *grad_rem, *grad_weight, *grad_bias;
  int relu;
  void *stream;
  const char *what_sums, *what_apply;
};

template <typename Tx, typename Ty, int V>
int launch_bn_train_backward(const BnBackwardArgs &a, const BnGeom &g)
{
  if (!a.grad_x && !a.grad_rem && !a.grad_weight && !a.grad_bias) return GANET_OK;
  const typename Tx::T *xp = (const typename Tx::T *)a.x;
  const typename Ty::T *gp = (const typename Ty::T *)a.grad_y;
  const dim3 grid(g.Rs * g.Rn, g.C), apply_grid = (a.grad_x || a.grad_rem) ? grid : dim3(1, g.C);
  hipStream_t st = (hipStream_t)a.stream;
  GA_LAUNCH((bn_bwd_partials<Tx, Ty, V>), grid, dim3(BN_BLOCK), st, xp, a.rem, gp, a.weight, a.bias, a.save_mean, a.save_invstd, a.workspace,
            g, a.relu);
  GA_TRY(check_launch(a.what_sums));
  GA_LAUNCH((bn_bwd_apply<Tx, Ty, V>), apply_grid, dim3(BN_BLOCK), st, xp, a.rem, gp, a.weight, a.bias, a.save_mean, a.save_invstd,
            a.workspace, (typename Tx::T *)a.grad_x, a.grad_rem, a.grad_weight, a.grad_bias, g, a.relu);
  return check_launch(a.what_apply);
}

// (the all-fp32 form and the forms with a 16-bit operand are sibling kernels: mixed_kernels.h says why)
template <typename Tx, typename Tr, typename Ty, int V>
int launch_bn_affine(const void *x, const void *rem, const float *scale, const float *shift, void *y, const BnGeom &g, int relu,
                     void *stream, const char *what)
{
  const dim3 grid(g.Rs * g.Rn, g.C);
  hipStream_t st = (hipStream_t)stream;
  if constexpr (std::is_same_v<Tx, st_f32> && std::is_same_v<Tr, st_f32> && std::is_same_v<Ty, st_f32>)
    GA_LAUNCH((bn_affine_apply<V>), grid, dim3(BN_BLOCK), st, (const float *)x, (const float *)rem, scale, shift, (float *)y, g, relu);
  else
    GA_LAUNCH((bn_affine_apply_mixed<Tx, Tr, Ty, V>), grid, dim3(BN_BLOCK), st, (const typename Tx::T *)x, (const typename Tr::T *)rem,
              scale, shift, (typename Ty::T *)y, g, relu);
  return check_launch(what);
}
}  // namespace

GA_EXPORT int ganet_bn_workspace(int N, int C, int S)
{
  BnGeom g;
  GA_TRY(bn_geom("ganet_bn_workspace", N, C, S, 1, true, &g));
  return 2 * C * bn_rows_cap(C);
}

GA_EXPORT int ganet_bn_train_forward(const float *x, const float *rem, const float *weight, const float *bias,
                                     float *running_mean, float *running_var, double *workspace, float *y, float *save_mean,
                                     float *save_invstd, int N, int C, int S, int momentum_bits, int eps_bits, int relu,
                                     void *stream)
{
  const char *who = "ganet_bn_train_forward";
  GA_TRY(check_ptrs(who, x, workspace, y, save_mean, save_invstd));
  if ((running_mean == nullptr) != (running_var == nullptr)) return fail(GANET_E_INVALID, "%s: running_mean and running_var come together", who);
  if (y == x || y == rem) return fail(GANET_E_INVALID, "%s: y must not alias an input", who);
  const bool vec = S % 4 == 0 && aligned16(x, y, rem);
  BnGeom g;
  GA_TRY(bn_geom(who, N, C, S, vec ? 4 : 1, true, &g));
  const BnForwardArgs a = {x, rem, weight, bias, running_mean, running_var, workspace, y, save_mean, save_invstd, momentum_bits, eps_bits,
                           relu, stream, "batch norm statistics", "batch norm forward"};
  int rc;
  with_width<4>(vec, [&](auto v) { rc = launch_bn_train_forward<st_f32, st_f32, decltype(v)::value>(a, g); });
  return rc;
}

GA_EXPORT int ganet_bn_train_backward(const float *x, const float *rem, const float *grad_y, const float *weight,
                                      const float *bias, const float *save_mean, const float *save_invstd, double *workspace,
                                      float *grad_x, float *grad_rem, float *grad_weight, float *grad_bias, int N, int C, int S,
                                      int relu, void *stream)
{
  const char *who = "ganet_bn_train_backward";
  GA_TRY(check_ptrs(who, x, grad_y, save_mean, save_invstd, workspace));
  for (const float *o : {(const float *)grad_x, (const float *)grad_rem})
    if (o && (o == x || o == rem || o == grad_y)) return fail(GANET_E_INVALID, "%s: a gradient must not alias an input", who);
  if (grad_x && grad_x == grad_rem) return fail(GANET_E_INVALID, "%s: grad_x and grad_rem are two buffers", who);
  const bool vec = S % 4 == 0 && aligned16(x, rem, grad_y, grad_x, grad_rem);
  BnGeom g;
  GA_TRY(bn_geom(who, N, C, S, vec ? 4 : 1, true, &g));
  const BnBackwardArgs a = {x, rem, grad_y, weight, bias, save_mean, save_invstd, workspace, grad_x, grad_rem, grad_weight, grad_bias, relu,
                            stream, "batch norm backward sums", "batch norm backward"};
  int rc;
  with_width<4>(vec, [&](auto v) { rc = launch_bn_train_backward<st_f32, st_f32, decltype(v)::value>(a, g); });
  return rc;
}

GA_EXPORT int ganet_bn_apply_forward(const float *x, const float *rem, const float *scale, const float *shift, float *y, int N,
                                     int C, int S, int relu, void *stream)
{
  const char *who = "ganet_bn_apply_forward";
  GA_TRY(check_ptrs(who, x, scale, shift, y));
  if (y == rem) return fail(GANET_E_INVALID, "%s: y may alias x, not rem", who);
  const bool vec = S % 4 == 0 && aligned16(x, y, rem);
  BnGeom g;
  GA_TRY(bn_geom(who, N, C, S, vec ? 4 : 1, false, &g));
  int rc;
  with_width<4>(vec, [&](auto v) {
    rc = launch_bn_affine<st_f32, st_f32, st_f32, decltype(v)::value>(x, rem, scale, shift, y, g, relu, stream, "batch norm apply");
  });
  return rc;
}

// ---- mixed precision: 16-bit storage around the fp32 ops (mixed_kernels.h) ----------------------------------------------------
namespace {
bool type_code(int t) { return t == GANET_F32 || t == GANET_F16 || t == GANET_BF16; }

// f(type_c<T>) for the storage type of a type code
template <class F> void with_storage(int code, F &&f) { with_type<st_f32, st_f16, st_bf16>(code == GANET_F32 ? 0 : code == GANET_F16 ? 1 : 2, f); }
template <class F> void with_st16(int code, F &&f) { with_type<st_f16, st_bf16>(code == GANET_F16 ? 0 : 1, f); }

template <typename Ts, typename Td>
void launch_cast(const void *src, void *dst, i64 n, hipStream_t st)
{
  const typename Ts::T *sp = (const typename Ts::T *)src;
  typename Td::T *dp = (typename Td::T *)dst;
  const bool vec = aligned16(src, dst) && n >= MX_V;
  with_width<MX_V>(vec, [&](auto v) {
    constexpr int V = decltype(v)::value;
    // (16 bits to the same 16 bits is ganet_cast's raw copy, never a typed kernel)
    if constexpr (!(std::is_same_v<Ts, Td> && Ts::CODE > 0))
      GA_LAUNCH((cast_kernel<Ts, Td, V>), dim3(ew_grid(n / V)), dim3(256), st, sp, dp, n);
  });
}
}  // namespace

GA_EXPORT int ganet_cast(const void *src, void *dst, int n_hi, int n_lo, int src_type, int dst_type, void *stream)
{
  const char *who = "ganet_cast";
  GA_TRY(check_ptrs(who, src, dst));
  if (!type_code(src_type) || !type_code(dst_type)) return fail(GANET_E_INVALID, "%s: type code %d -> %d", who, src_type, dst_type);
  if (n_hi < 0 || n_lo < 0) return fail(GANET_E_INVALID, "%s: negative count n_hi=%d n_lo=%d", who, n_hi, n_lo);
  const i64 n = ((i64)n_hi << 31) + n_lo;
  if (n <= 0) return fail(GANET_E_INVALID, "%s: non-positive count", who);
  if (src == dst) return fail(GANET_E_INVALID, "%s: dst must not alias src", who);
  hipStream_t st = (hipStream_t)stream;
  const bool same = src_type == dst_type;
  if (same && dst_type != GANET_F32) launch_cast<st_raw16, st_raw16>(src, dst, n, st);      // 16 bits to the same 16 bits: a copy
  else
    with_storage(src_type, [&](auto ts) {
      with_storage(dst_type, [&](auto td) { launch_cast<typename decltype(ts)::type, typename decltype(td)::type>(src, dst, n, st); });
    });
  return check_launch("cast");
}

GA_EXPORT int ganet_bn_apply_forward_mixed(const void *x, const void *rem, const float *scale, const float *shift, void *y, int N,
                                           int C, int S, int relu, int x_type, int rem_type, int y_type, void *stream)
{
  const char *who = "ganet_bn_apply_forward_mixed";
  GA_TRY(check_ptrs(who, x, scale, shift, y));
  if (!type_code(x_type) || !type_code(rem_type) || !type_code(y_type))
    return fail(GANET_E_INVALID, "%s: type codes x=%d rem=%d y=%d", who, x_type, rem_type, y_type);
  if (y == rem) return fail(GANET_E_INVALID, "%s: y may alias x, not rem", who);
  if (y == x && (y_type == GANET_F32) != (x_type == GANET_F32)) return fail(GANET_E_INVALID, "%s: y may alias x only where both have one width", who);
  const bool rem16 = rem != nullptr && rem_type != GANET_F32, y16 = y_type != GANET_F32, x32 = x_type == GANET_F32;
  if (x32 && !y16) return fail(GANET_E_UNSUPPORTED, "%s: x and y are fp32: that is ganet_bn_apply_forward's case", who);
  if (x32 && rem16) return fail(GANET_E_UNSUPPORTED, "%s: no kernel for an fp32 x with a 16-bit rem", who);
  if (!x32 && ((rem16 && rem_type != x_type) || (y16 && y_type != x_type)))
    return fail(GANET_E_UNSUPPORTED, "%s: no kernel for x=%d rem=%d y=%d: 16-bit rem and y have x's format", who, x_type, rem_type, y_type);
  const bool vec = S % MX_V == 0 && aligned16(x, y, rem);
  BnGeom g;
  GA_TRY(bn_geom(who, N, C, S, vec ? MX_V : 1, false, &g));
  int rc = GANET_OK;
  // the 16-bit format of the call (x's, or y's under an fp32 x); every operand is that or fp32
  with_st16(x32 ? y_type : x_type, [&](auto t16) {
    with_flags([&](auto fx, auto r16, auto o16, auto v) {
      using T16 = typename decltype(t16)::type;
      using Tx = std::conditional_t<decltype(fx)::value, st_f32, T16>;
      using Tr = std::conditional_t<decltype(r16)::value, T16, st_f32>;
      using Ty = std::conditional_t<decltype(o16)::value, T16, st_f32>;
      // (an fp32 x has an fp32 rem and a 16-bit y: checked above)
      if constexpr (!decltype(fx)::value || (!decltype(r16)::value && decltype(o16)::value))
        rc = launch_bn_affine<Tx, Tr, Ty, decltype(v)::value ? MX_V : 1>(x, rem, scale, shift, y, g, relu, stream, "batch norm apply (mixed)");
    }, x32, rem16, y16, vec);
  });
  return rc;
}

GA_EXPORT int ganet_cost_volume_forward_16(const void *x, const void *y, void *cost, int N, int C, int Dn, int H, int W,
                                           void *stream)
{
  const char *who = "ganet_cost_volume_forward_16";
  GA_TRY(check_ptrs(who, x, y, cost));
  GA_TRY(check_positive(who, N, C, Dn, H, W));
  if (cost == x || cost == y) return fail(GANET_E_INVALID, "%s: cost must not alias an input", who);
  const i64 n = (i64)N * 2 * C * Dn * H * W;
  const uint16_t *xp = (const uint16_t *)x, *yp = (const uint16_t *)y;
  uint16_t *cp = (uint16_t *)cost;
  if (W % MX_V == 0 && aligned16(x, cost))
    GA_LAUNCH(cost_volume_fwd16, dim3(ew_grid(n / MX_V)), dim3(256), (hipStream_t)stream, xp, yp, cp, N, C, Dn, H, W);
  else
    GA_LAUNCH(cost_volume_fwd<uint16_t>, dim3(ew_grid(n)), dim3(256), (hipStream_t)stream, xp, yp, cp, N, C, Dn, H, W);
  return check_launch("cost volume forward (16-bit)");
}

GA_EXPORT int ganet_l1_normalize_forward_mixed(const void *x, float *y0, float *y1, float *y2, float *y3, int N, int G, int C,
                                               int K, int H, int W, int x_type, void *stream)
{
  const char *who = "ganet_l1_normalize_forward_mixed";
  GA_TRY(check_norm(who, N, G, C, K, H, W));
  float *ys[4] = {y0, y1, y2, y3};
  GA_TRY(check_ptrs(who, x));
  if (!type_code(x_type)) return fail(GANET_E_INVALID, "%s: type code %d", who, x_type);
  if (x_type == GANET_F32) return fail(GANET_E_UNSUPPORTED, "%s: x is fp32: that is ganet_l1_normalize_forward's case", who);
  NormPtrs p = {};
  for (int g = 0; g < 4; g++) {
    if (g < G && !ys[g]) return fail(GANET_E_INVALID, "%s: null output %d", who, g);
    p.y[g] = ys[g < G ? g : 0];
  }
  const i64 HW = (i64)H * W;
  const dim3 grid(ew_grid((i64)N * G * C * HW)), block(256);
  hipStream_t st = (hipStream_t)stream;
  const uint16_t *xp = (const uint16_t *)x;
  with_st16(x_type, [&](auto t16) {
    with_int_else<0, 5, 75>(K, [&](auto KC) {
      GA_LAUNCH((l1norm_fwd<decltype(KC)::value, typename decltype(t16)::type>), grid, block, st, xp, p, N, G, C, K, HW);
    });
  });
  return check_launch("l1 normalise forward (mixed)");
}

// ---- mixed precision, training: batch statistics and the backwards on 16-bit storage (bn_kernels.h, mixed_train_kernels.h) -----
namespace {
// the three sites of a model under autocast: x 16-bit; y (grad_y) in x's format with an fp32 residual or none, or fp32 with none
int check_bn_mixed_types(const char *who, const void *rem, int x_type, int rem_type, int y_type)
{
  if (!type_code(x_type) || !type_code(rem_type) || !type_code(y_type))
    return fail(GANET_E_INVALID, "%s: type codes x=%d rem=%d y=%d", who, x_type, rem_type, y_type);
  if (x_type == GANET_F32) return fail(GANET_E_UNSUPPORTED, "%s: x is fp32: no kernel (all fp32 is ganet_bn_train_*'s case)", who);
  if (y_type != GANET_F32 && y_type != x_type)
    return fail(GANET_E_UNSUPPORTED, "%s: no kernel for x=%d y=%d: a 16-bit y has x's format", who, x_type, y_type);
  if (rem && rem_type != GANET_F32) return fail(GANET_E_UNSUPPORTED, "%s: no kernel for a 16-bit rem (type %d)", who, rem_type);
  if (rem && y_type == GANET_F32) return fail(GANET_E_UNSUPPORTED, "%s: no kernel for a residual with an fp32 y", who);
  return GANET_OK;
}
}  // namespace

GA_EXPORT int ganet_bn_train_forward_mixed(const void *x, const float *rem, const float *weight, const float *bias,
                                           float *running_mean, float *running_var, double *workspace, void *y, float *save_mean,
                                           float *save_invstd, int N, int C, int S, int momentum_bits, int eps_bits, int relu,
                                           int x_type, int rem_type, int y_type, void *stream)
{
  const char *who = "ganet_bn_train_forward_mixed";
  GA_TRY(check_ptrs(who, x, workspace, y, save_mean, save_invstd));
  if ((running_mean == nullptr) != (running_var == nullptr)) return fail(GANET_E_INVALID, "%s: running_mean and running_var come together", who);
  if (y == x || y == (const void *)rem) return fail(GANET_E_INVALID, "%s: y must not alias an input", who);
  GA_TRY(check_bn_mixed_types(who, rem, x_type, rem_type, y_type));
  const bool vec = S % MX_V == 0 && aligned16(x, y, rem);
  BnGeom g;
  GA_TRY(bn_geom(who, N, C, S, vec ? MX_V : 1, true, &g));
  const BnForwardArgs a = {x, rem, weight, bias, running_mean, running_var, workspace, y, save_mean, save_invstd, momentum_bits, eps_bits,
                           relu, stream, "batch norm statistics (mixed)", "batch norm forward (mixed)"};
  int rc;
  with_st16(x_type, [&](auto t16) {
    with_flags([&](auto o16, auto v) {
      using Tx = typename decltype(t16)::type;
      using Ty = std::conditional_t<decltype(o16)::value, Tx, st_f32>;
      rc = launch_bn_train_forward<Tx, Ty, decltype(v)::value ? MX_V : 1>(a, g);
    }, y_type != GANET_F32, vec);
  });
  return rc;
}

GA_EXPORT int ganet_bn_train_backward_mixed(const void *x, const float *rem, const void *grad_y, const float *weight,
                                            const float *bias, const float *save_mean, const float *save_invstd, double *workspace,
                                            void *grad_x, float *grad_rem, float *grad_weight, float *grad_bias, int N, int C, int S,
                                            int relu, int x_type, int rem_type, int gy_type, void *stream)
{
  const char *who = "ganet_bn_train_backward_mixed";
  GA_TRY(check_ptrs(who, x, grad_y, save_mean, save_invstd, workspace));
  for (const void *o : {(const void *)grad_x, (const void *)grad_rem})
    if (o && (o == x || o == (const void *)rem || o == grad_y)) return fail(GANET_E_INVALID, "%s: a gradient must not alias an input", who);
  if (grad_x && grad_x == (void *)grad_rem) return fail(GANET_E_INVALID, "%s: grad_x and grad_rem are two buffers", who);
  GA_TRY(check_bn_mixed_types(who, rem, x_type, rem_type, gy_type));
  const bool vec = S % MX_V == 0 && aligned16(x, rem, grad_y, grad_x, grad_rem);
  BnGeom g;
  GA_TRY(bn_geom(who, N, C, S, vec ? MX_V : 1, true, &g));
  const BnBackwardArgs a = {x, rem, grad_y, weight, bias, save_mean, save_invstd, workspace, grad_x, grad_rem, grad_weight, grad_bias, relu,
                            stream, "batch norm backward sums (mixed)", "batch norm backward (mixed)"};
  int rc;
  with_st16(x_type, [&](auto t16) {
    with_flags([&](auto o16, auto v) {
      using Tx = typename decltype(t16)::type;
      using Ty = std::conditional_t<decltype(o16)::value, Tx, st_f32>;
      rc = launch_bn_train_backward<Tx, Ty, decltype(v)::value ? MX_V : 1>(a, g);
    }, gy_type != GANET_F32, vec);
  });
  return rc;
}

GA_EXPORT int ganet_cost_volume_backward_16(const void *grad_cost, void *grad_x, void *grad_y, int N, int C, int Dn, int H, int W,
                                            int type, void *stream)
{
  const char *who = "ganet_cost_volume_backward_16";
  GA_TRY(check_ptrs(who, grad_cost, grad_x, grad_y));
  GA_TRY(check_positive(who, N, C, Dn, H, W));
  if (!type_code(type)) return fail(GANET_E_INVALID, "%s: type code %d", who, type);
  if (type == GANET_F32) return fail(GANET_E_UNSUPPORTED, "%s: fp32: that is ganet_cost_volume_backward's case", who);
  if (grad_x == grad_cost || grad_y == grad_cost || grad_x == grad_y) return fail(GANET_E_INVALID, "%s: three buffers, none an alias of another", who);
  const bool vec = W % MX_V == 0 && aligned16(grad_cost, grad_x, grad_y);
  const i64 n = (i64)N * C * H * W;
  with_st16(type, [&](auto t16) {
    with_width<MX_V>(vec, [&](auto v) {
      constexpr int V = decltype(v)::value;
      GA_LAUNCH((cost_volume_bwd16<typename decltype(t16)::type, V>), dim3(ew_grid(n / V)), dim3(256), (hipStream_t)stream,
                (const uint16_t *)grad_cost, (uint16_t *)grad_x, (uint16_t *)grad_y, N, C, Dn, H, W);
    });
  });
  return check_launch("cost volume backward (16-bit)");
}

GA_EXPORT int ganet_l1_normalize_backward_mixed(const void *x, const float *gy0, const float *gy1, const float *gy2, const float *gy3,
                                                void *grad_x, int N, int G, int C, int K, int H, int W, int x_type, void *stream)
{
  const char *who = "ganet_l1_normalize_backward_mixed";
  GA_TRY(check_norm(who, N, G, C, K, H, W));
  const float *gs[4] = {gy0, gy1, gy2, gy3};
  GA_TRY(check_ptrs(who, x, grad_x));
  if (!type_code(x_type)) return fail(GANET_E_INVALID, "%s: type code %d", who, x_type);
  if (x_type == GANET_F32) return fail(GANET_E_UNSUPPORTED, "%s: x is fp32: that is ganet_l1_normalize_backward's case", who);
  if (grad_x == x) return fail(GANET_E_INVALID, "%s: grad_x must not alias x", who);
  NormPtrs p = {};
  for (int g = 0; g < 4; g++) {
    if (g < G && !gs[g]) return fail(GANET_E_INVALID, "%s: null gradient %d", who, g);
    p.gy[g] = gs[g < G ? g : 0];
  }
  const i64 HW = (i64)H * W;
  const dim3 grid(ew_grid((i64)N * G * C * HW)), block(256);
  hipStream_t st = (hipStream_t)stream;
  with_st16(x_type, [&](auto t16) {
    with_int_else<0, 5, 75>(K, [&](auto KC) {
      GA_LAUNCH((l1norm_bwd<decltype(KC)::value, typename decltype(t16)::type>), grid, block, st, (const uint16_t *)x, p,
                (uint16_t *)grad_x, N, G, C, K, HW);
    });
  });
  return check_launch("l1 normalise backward (mixed)");
}

// ---- image front and back end (predict.py:75-114, :132-138; dataloader/dataset.py:48-92) --------------------------------------
namespace {
int io_rows(i64 pixels)
{
  const i64 want = (pixels + IO_PIX_PER_BLOCK - 1) / IO_PIX_PER_BLOCK;
  return (int)(want < IO_MAX_ROWS ? want : IO_MAX_ROWS);
}

int io_blocks(i64 units)
{
  return clamp_grid(units, IO_BLOCK, IO_MAX_BLOCKS);
}

int io_check_image(const char *who, int H, int W, int CP)
{
  if (H <= 0 || W <= 0) return fail(GANET_E_INVALID, "%s: non-positive size H=%d W=%d", who, H, W);
  if (CP != 3 && CP != 4) return fail(GANET_E_INVALID, "%s: CP=%d bytes per pixel, 3 or 4", who, CP);
  if ((i64)H * W > (1 << 24)) return fail(GANET_E_INVALID, "%s: %lld pixels; the integer sums are exact up to 2^24", who, (long long)H * W);
  return GANET_OK;
}

int io_check_window(const char *who, int Hc, int Wc, int oy, int ox)
{
  if (Hc <= 0 || Wc <= 0) return fail(GANET_E_INVALID, "%s: non-positive window Hc=%d Wc=%d", who, Hc, Wc);
  if ((i64)Hc * Wc > (1 << 28)) return fail(GANET_E_INVALID, "%s: window of %lld pixels", who, (long long)Hc * Wc);
  const int lim = 1 << 28;
  if (oy < -lim || oy > lim || ox < -lim || ox > lim) return fail(GANET_E_INVALID, "%s: offset (%d, %d) out of range", who, oy, ox);
  return GANET_OK;
}
}  // namespace

GA_EXPORT int ganet_stereo_input_workspace(int H, int W, int CP)
{
  GA_TRY(io_check_image("ganet_stereo_input_workspace", H, W, CP));
  return 2 * IO_MAX_ROWS * IO_ROW;
}

GA_EXPORT int ganet_stereo_input_stats(const uint8_t *left, const uint8_t *right, uint64_t *workspace, int H, int W, int CP,
                                       void *stream)
{
  const char *who = "ganet_stereo_input_stats";
  GA_TRY(check_ptrs(who, left, right, workspace));
  GA_TRY(io_check_image(who, H, W, CP));
  IoImage g = {left, right, H, W, CP, io_rows((i64)H * W), (aligned16(left) ? 1 : 0) | (aligned16(right) ? 2 : 0)};
  GA_LAUNCH(io_stats, dim3(g.R, 2), dim3(IO_BLOCK), (hipStream_t)stream, g, (u64 *)workspace);
  return check_launch("stereo input statistics");
}

GA_EXPORT int ganet_stereo_input_apply(const uint8_t *left, const uint8_t *right, const uint64_t *workspace, float *left_out,
                                       float *right_out, int H, int W, int CP, int Hc, int Wc, int oy, int ox_left, int ox_right,
                                       int form, void *stream)
{
  const char *who = "ganet_stereo_input_apply";
  GA_TRY(check_ptrs(who, left, right, workspace, left_out, right_out));
  GA_TRY(io_check_image(who, H, W, CP));
  GA_TRY(io_check_window(who, Hc, Wc, oy, ox_left));
  GA_TRY(io_check_window(who, Hc, Wc, oy, ox_right));
  if (form != 0 && form != 1) return fail(GANET_E_INVALID, "%s: form=%d (0: table, 1: direct)", who, form);
  IoImage g = {left, right, H, W, CP, io_rows((i64)H * W), 0};
  IoWindow w = {left_out, right_out, Hc, Wc, oy, ox_left, ox_right};
  const bool vec = Wc % 4 == 0 && aligned16(left_out, right_out);
  const dim3 grid(io_blocks((i64)Hc * (vec ? Wc / 4 : Wc)), 2);
  hipStream_t st = (hipStream_t)stream;
  const u64 *ws = (const u64 *)workspace;
  with_flags([&](auto v, auto table) {
    GA_LAUNCH((io_apply<decltype(v)::value ? 4 : 1, decltype(table)::value>), grid, dim3(IO_BLOCK), st, g, w, ws);
  }, vec, form == 0);
  return check_launch("stereo input apply");
}

GA_EXPORT int ganet_window_f32(const float *src, float *dst, int H, int W, int Hc, int Wc, int oy, int ox, int sub_bits,
                               int fill_bits, void *stream)
{
  const char *who = "ganet_window_f32";
  GA_TRY(check_ptrs(who, src, dst));
  if (src == dst) return fail(GANET_E_INVALID, "%s: dst must not alias src", who);
  if (H <= 0 || W <= 0 || (i64)H * W > (1 << 28)) return fail(GANET_E_INVALID, "%s: bad size H=%d W=%d", who, H, W);
  GA_TRY(io_check_window(who, Hc, Wc, oy, ox));
  const float sub = bn_float(sub_bits), fill = bn_float(fill_bits);
  const bool vec = Wc % 4 == 0 && aligned16(dst);
  const dim3 grid(io_blocks((i64)Hc * (vec ? Wc / 4 : Wc)));
  hipStream_t st = (hipStream_t)stream;
  with_width<4>(vec, [&](auto V) { GA_LAUNCH((io_window_f32<decltype(V)::value>), grid, dim3(IO_BLOCK), st, src, dst, H, W, Hc, Wc, oy, ox, sub, fill); });
  return check_launch("float window");
}

GA_EXPORT int ganet_disparity_to_u16(const float *disp, uint16_t *out, int Hd, int Wd, int h, int w, int oy, int ox,
                                     int scale_bits, void *stream)
{
  const char *who = "ganet_disparity_to_u16";
  GA_TRY(check_ptrs(who, disp, out));
  if (Hd <= 0 || Wd <= 0 || h <= 0 || w <= 0 || (i64)Hd * Wd > (1 << 28))
    return fail(GANET_E_INVALID, "%s: bad size Hd=%d Wd=%d h=%d w=%d", who, Hd, Wd, h, w);
  if (oy < 0 || ox < 0 || (i64)oy + h > Hd || (i64)ox + w > Wd)
    return fail(GANET_E_INVALID, "%s: the [%d, %d] window at (%d, %d) leaves the [%d, %d] map", who, h, w, oy, ox, Hd, Wd);
  const float scale = bn_float(scale_bits);
  const bool vec = aligned16(out);
  const i64 n = (i64)h * w;
  const dim3 grid(io_blocks(vec ? n / 8 : n));
  hipStream_t st = (hipStream_t)stream;
  with_width<8>(vec, [&](auto V) { GA_LAUNCH((io_disp_u16<decltype(V)::value>), grid, dim3(IO_BLOCK), st, disp, out, Wd, h, w, oy, ox, scale); });
  return check_launch("disparity to 16 bit");
}

namespace {
// copy the probe's `npat` x 64 results back and hold them to expect(lane, out[npat]); `tag`: "" | " (wave)"
template <class Expect>
int dpp_selftest_report(const char *tag, int npat, const int *scratch_dev, int *host_out, hipStream_t st, Expect expect)
{
#if defined(GA_HIPSIM)
  memcpy(host_out, scratch_dev, sizeof(int) * npat * 64);
#else
  GA_HIP(hipMemcpyAsync(host_out, scratch_dev, sizeof(int) * npat * 64, hipMemcpyDeviceToHost, st));
  GA_HIP(hipStreamSynchronize(st));
#endif
  int bad = 0, first_pat = -1, first_lane = -1;
  for (int lane = 0; lane < 64; lane++) {
    int want[8];
    expect(lane, want);
    for (int p = 0; p < npat; p++)
      if (host_out[p * 64 + lane] != want[p]) {
        if (!bad) { first_pat = p; first_lane = lane; }
        bad++;
      }
  }
  if (bad)
    return fail(GANET_E_RUNTIME, "DPP self-test%s: %d mismatches, first at pattern %d lane %d (got %d)", tag,
                bad, first_pat, first_lane, host_out[first_pat * 64 + first_lane]);
  return GANET_OK;
}
}  // namespace

GA_EXPORT int ganet_selftest_dpp_wave(int *scratch_dev, int *host_out, void *stream)
{
  GA_TRY(check_ptrs("ganet_selftest_dpp_wave", scratch_dev, host_out));
  hipStream_t st = (hipStream_t)stream;
  GA_LAUNCH(dpp_probe_wave, dim3(1), dim3(64), st, scratch_dev);
  GA_TRY(check_launch("dpp probe (wave)"));
  return dpp_selftest_report(" (wave)", 4, scratch_dev, host_out, st, [](int lane, int *expect) {
    expect[0] = lane < 63 ? lane + 1 : -1;
    expect[1] = lane > 0 ? lane - 1 : -1;
    expect[2] = 63;
    expect[3] = 2016;
  });
}

GA_EXPORT int ganet_selftest_dpp(int *scratch_dev, int *host_out, void *stream)
{
  GA_TRY(check_ptrs("ganet_selftest_dpp", scratch_dev, host_out));
  hipStream_t st = (hipStream_t)stream;
  GA_LAUNCH(dpp_probe, dim3(1), dim3(64), st, scratch_dev);
  GA_TRY(check_launch("dpp probe"));
  return dpp_selftest_report("", 8, scratch_dev, host_out, st, [](int lane, int *expect) {
    const int r = lane & 15, row = lane & ~15;
    expect[0] = lane ^ 1;
    expect[1] = lane ^ 2;
    expect[2] = r < 15 ? lane + 1 : -1;
    expect[3] = r > 0 ? lane - 1 : -1;
    expect[4] = row + 15 - r;
    expect[5] = (lane & ~7) + 7 - (lane & 7);
    // argmax of (lane*37)%64 over the 16-lane row, smallest lane on ties
    int bk = row;
    for (int l = row; l < row + 16; l++)
      if ((l * 37) % 64 > (bk * 37) % 64) bk = l;
    expect[6] = bk;
    expect[7] = 16 * row + 120;
  });
}

// ---- conv32x1 on a 16-bit x (include/ganet_hip_conv16.h; disp_conv_kernels.h with a 16-bit ST) -------------------------------------
GA_EXPORT int ganet_disp_conv_forward_16(const void *x, const float *weight, float *y, int N, int C, int D, int H, int W,
                                         int x_type, void *stream)
{
  const char *who = "ganet_disp_conv_forward_16";
  GA_TRY(check_ptrs(who, x, weight, y));
  DispConvGeom g;
  dim3 grid;
  GA_TRY(check_disp_conv(who, N, C, D, H, W, g, grid));
  if (!type16(x_type)) return fail(GANET_E_INVALID, "%s: type code %d (fp16 or bf16)", who, x_type);
  if ((const void *)y == x || y == weight) return fail(GANET_E_INVALID, "%s: y must not alias an input", who);
  int rc;
  with_st16(x_type, [&](auto t) {
    rc = launch_disp_conv_fwd<typename decltype(t)::type>(x, weight, y, g, grid, W % 4 == 0 && aligned8(x) && aligned16(y), stream,
                                                          "disp conv forward (16-bit x)");
  });
  return rc;
}

GA_EXPORT int ganet_disp_conv_backward_data_16(const float *grad_y, const float *weight, void *grad_x, int N, int C, int D,
                                               int H, int W, int gx_type, void *stream)
{
  const char *who = "ganet_disp_conv_backward_data_16";
  GA_TRY(check_ptrs(who, grad_y, weight, grad_x));
  DispConvGeom g;
  dim3 grid;
  GA_TRY(check_disp_conv(who, N, C, D, H, W, g, grid));
  if (!type16(gx_type)) return fail(GANET_E_INVALID, "%s: type code %d (fp16 or bf16)", who, gx_type);
  if (grad_x == (const void *)grad_y || grad_x == (const void *)weight) return fail(GANET_E_INVALID, "%s: grad_x must not alias an input", who);
  int rc;
  with_st16(gx_type, [&](auto t) {
    rc = launch_disp_conv_bwd_data<typename decltype(t)::type>(grad_y, weight, grad_x, g, grid, W % 4 == 0 && aligned8(grad_x) && aligned16(grad_y),
                                                               stream, "disp conv backward (data, 16-bit grad_x)");
  });
  return rc;
}

GA_EXPORT int ganet_disp_conv_backward_weight_16(const void *x, const float *grad_y, float *workspace, float *grad_weight,
                                                 int N, int C, int D, int H, int W, int x_type, void *stream)
{
  const char *who = "ganet_disp_conv_backward_weight_16";
  GA_TRY(check_ptrs(who, x, grad_y, workspace, grad_weight));
  DispConvGeom g;
  dim3 grid;
  GA_TRY(check_disp_conv(who, N, C, D, H, W, g, grid));
  if (!type16(x_type)) return fail(GANET_E_INVALID, "%s: type code %d (fp16 or bf16)", who, x_type);
  if ((const void *)grad_weight == x || grad_weight == grad_y || (const void *)workspace == x || workspace == grad_y || workspace == grad_weight)
    return fail(GANET_E_INVALID, "%s: workspace and grad_weight must not alias anything", who);
  int rc;
  with_st16(x_type, [&](auto t) {
    rc = launch_disp_conv_bwd_weight<typename decltype(t)::type>(who, x, grad_y, workspace, grad_weight, g, grid,
                                                                 W % 4 == 0 && aligned8(x) && aligned16(grad_y), stream,
                                                                 "disp conv backward (weight partials, 16-bit x)");
  });
  return rc;
}

// ---- the channels-last inference path (include/ganet_hip_cl.h; cl_kernels.h) ---------------------------------------------------
namespace {
bool layout_code(int l) { return l == GANET_LAYOUT_PLANAR || l == GANET_LAYOUT_CL; }
}  // namespace

GA_EXPORT int ganet_bn_apply_forward_cl(const float *x, const float *rem, const float *scale, const float *shift, float *y, int N,
                                        int C, int S, int relu, int x_layout, int rem_layout, int y_layout, void *stream)
{
  const char *who = "ganet_bn_apply_forward_cl";
  GA_TRY(check_ptrs(who, x, scale, shift, y));
  GA_TRY(check_positive(who, N, C, S));
  if (!layout_code(x_layout) || !layout_code(rem_layout) || !layout_code(y_layout))
    return fail(GANET_E_INVALID, "%s: layout codes x=%d rem=%d y=%d", who, x_layout, rem_layout, y_layout);
  const bool xcl = x_layout == GANET_LAYOUT_CL, ycl = y_layout == GANET_LAYOUT_CL;
  if (y == rem) return fail(GANET_E_INVALID, "%s: y may alias x, not rem", who);
  if (y == x && xcl != ycl) return fail(GANET_E_INVALID, "%s: y may alias x only where both have one layout", who);
  if (rem && rem_layout == GANET_LAYOUT_CL) return fail(GANET_E_UNSUPPORTED, "%s: no kernel for a channels-last rem", who);
  if (!xcl && !ycl) return fail(GANET_E_UNSUPPORTED, "%s: every operand is planar: that is ganet_bn_apply_forward's case", who);
  if (C > 65535) return fail(GANET_E_UNSUPPORTED, "%s: C = %d is beyond 65535", who, C);
  hipStream_t st = (hipStream_t)stream;
  if (xcl && ycl && !rem) {
    const i64 n = (i64)N * C * S;
    with_width<4>(C % 4 == 0 && aligned16(x, y), [&](auto v) {
      constexpr int V = decltype(v)::value;
      GA_LAUNCH((cl_bn_stream<V>), dim3(clamp_grid(n / V, CL_BLOCK, CL_MAX_BLOCKS)), dim3(CL_BLOCK), st, x, scale, shift, y, n / V, C, relu);
    });
    return check_launch("batch norm apply (channels-last)");
  }
  ClGeom g;
  g.N = N; g.C = C; g.S = S;
  g.nst = ((i64)S + CL_T - 1) / CL_T;
  g.ncb = (C + CL_CB - 1) / CL_CB;
  g.ntiles = (i64)N * g.nst * g.ncb;
  const dim3 grid(clamp_grid(g.ntiles, 1, CL_MAX_BLOCKS)), block(CL_BLOCK);
  // the staged operand changes layout, the direct one (if any) is read by the lanes that compute: see cl_kernels.h
  const float *staged = xcl == ycl ? rem : x, *direct = xcl == ycl ? x : rem;
  const bool src_cl = !ycl;
  const int mode = !direct ? 0 : src_cl ? 1 : xcl ? 2 : 3;
  const float *none = nullptr, *yc = y;
  const bool vc = C % 4 == 0 && aligned16(xcl ? x : none, ycl ? yc : none);
  const bool vp = S % 4 == 0 && aligned16(xcl ? none : x, rem, ycl ? none : yc);
  with_flags([&](auto scl, auto c4, auto p4) {
    with_int<0, 1, 2, 3>(mode, [&](auto m) {
      constexpr bool SRC_CL = decltype(scl)::value;
      constexpr int MODE = decltype(m)::value;
      if constexpr (SRC_CL ? MODE <= 1 : MODE != 1)
        GA_LAUNCH((cl_bn_transpose<SRC_CL, MODE, decltype(c4)::value ? 4 : 1, decltype(p4)::value ? 4 : 1>), grid, block, st, staged, direct,
                  scale, shift, y, g, relu);
    });
  }, src_cl, vc, vp);
  return check_launch("batch norm apply (layout change)");
}

GA_EXPORT int ganet_cost_volume_forward_cl(const float *x, const float *y, float *cost, int N, int C, int Dn, int H, int W,
                                           void *stream)
{
  const char *who = "ganet_cost_volume_forward_cl";
  GA_TRY(check_ptrs(who, x, y, cost));
  GA_TRY(check_positive(who, N, C, Dn, H, W));
  if (cost == x || cost == y) return fail(GANET_E_INVALID, "%s: cost must not alias an input", who);
  CvClGeom g;
  g.N = N; g.C = C; g.Dn = Dn; g.H = H; g.W = W;
  g.nwb = (W + CV_TW - 1) / CV_TW;
  g.ndb = (Dn + CV_DB - 1) / CV_DB;
  g.ncb = (C + CV_CB - 1) / CV_CB;
  g.ntiles = (i64)N * H * g.nwb * g.ndb * g.ncb;
  const dim3 grid(clamp_grid(g.ntiles, 1, CL_MAX_BLOCKS)), block(CL_BLOCK);
  with_width<4>(C % 4 == 0 && aligned16(cost), [&](auto v) {
    GA_LAUNCH((cost_volume_cl<decltype(v)::value>), grid, block, (hipStream_t)stream, x, y, cost, g);
  });
  return check_launch("cost volume forward (channels-last)");
}
