// OpenCV's uint8 warpAffine INTER_LINEAR arithmetic for one output pixel, shared by
// warp_affine_kernel (align.hip, BORDER_CONSTANT 0) and augment_kernel (augment.hip,
// BORDER_REPLICATE): the AB_BITS=10 fixed-point source position with cvRound (round-half-even)
// of double products, 5-bit sub-pixel fractions and 15-bit bilinear weights
// (oracle/align_ref.py warp_maps / warp_affine_linear).  The kernels differ only in which
// pixels they read for taps that fall outside the image.
#pragma once
#include <hip/hip_runtime.h>

// The map arithmetic must round exactly like OpenCV (separate double mul and add).
#pragma clang fp contract(off)

namespace frhip {

// Top-left tap (sx, sy) and the weights of the taps (sy, sx), (sy, sx+1), (sy+1, sx), (sy+1, sx+1).
struct WarpTap {
  int sx, sy;
  int w00, w01, w10, w11;
};

// The terms of the map that depend on the output row only (a work-item that makes several pixels
// of one row computes them once).  m: inverse map [2][3] (double).
struct WarpRow {
  long long X0, Y0;
};

__device__ __forceinline__ WarpRow warp_row(const double* m, int oy) {
  WarpRow r;
  r.X0 = (long long)__builtin_rint((m[1] * oy + m[2]) * 1024.0) + 16;
  r.Y0 = (long long)__builtin_rint((m[4] * oy + m[5]) * 1024.0) + 16;
  return r;
}

// Output pixel ox of the row r.
__device__ __forceinline__ WarpTap warp_tap(const double* m, const WarpRow& r, int ox) {
  const long long X0 = r.X0, Y0 = r.Y0;
  const long long adx = (long long)__builtin_rint(m[0] * ox * 1024.0);
  const long long bdx = (long long)__builtin_rint(m[3] * ox * 1024.0);
  const long long X = (X0 + adx) >> 5, Y = (Y0 + bdx) >> 5;
  // The position is 64-bit (a caller's map may put it anywhere: contract |position| <= 2^40 px);
  // narrowing it would wrap a far tap back into the frame.  Saturated to +-2^30 it stays outside
  // every frame (sx + 1 cannot overflow) and clamps to the same edge pixel under BORDER_REPLICATE.
  constexpr long long FAR = 1ll << 30;
  const long long sx = X >> 5, sy = Y >> 5;
  WarpTap t;
  t.sx = (int)(sx < -FAR ? -FAR : (sx > FAR ? FAR : sx));
  t.sy = (int)(sy < -FAR ? -FAR : (sy > FAR ? FAR : sy));
  const int fx = (int)(X & 31), fy = (int)(Y & 31);
  t.w00 = (32 - fx) * (32 - fy) * 32;
  t.w01 = fx * (32 - fy) * 32;
  t.w10 = (32 - fx) * fy * 32;
  t.w11 = fx * fy * 32;
  return t;
}

__device__ __forceinline__ uint8_t warp_blend(const WarpTap& t, int p00, int p01, int p10, int p11) {
  const int v = (p00 * t.w00 + p01 * t.w01 + p10 * t.w10 + p11 * t.w11 + (1 << 14)) >> 15;
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

}  // namespace frhip
