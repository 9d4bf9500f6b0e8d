// One entry of cv::resize's INTER_LINEAR coefficient table for one axis, shared by the host
// (resize_axis_table, detector.cpp) and resize_tables_kernel (detect.hip), so that tables built on
// the device are bitwise the host's: the same IEEE operations in the same order, with fp
// contraction off.  Output d of dsize reads source elements t[0] and t[1] of ssize with the 11-bit
// weights t[2] and t[3] (their sum is 2048).
//
//   scale = 1.0 / ((double)dsize / ssize)         two double divisions, correctly rounded on both
//   f     = (float)((d + 0.5) * scale - 0.5)      double multiply, double subtract, one narrowing
//   s     = floor(f), f -= s                      exact in float
//   the two clamps (s < 0, s >= ssize - 1) set f = 0
//   w     = lrint(f * 2048.f)                     a multiply by a power of two is exact and
//                                                 |f * 2048| <= 2048, so rintf (round-half-even in
//                                                 the default rounding mode, as lrint) and the
//                                                 conversion are exact
#pragma once
#include <hip/hip_runtime.h>

// Every operation of the two functions rounds on its own; contraction is switched back on at the
// end of the header, as resize_axis_table's own pair of pragmas did.  (A file that keeps it off for
// its own code, as detect.hip does, says so after its includes.)
#pragma clang fp contract(off)

namespace frhip {

// 1.0 / ((double)dsize / ssize): the same for every entry of an axis.
__host__ __device__ __forceinline__ double resize_axis_scale(int dsize, int ssize) {
  return 1.0 / ((double)dsize / ssize);
}

__host__ __device__ __forceinline__ void resize_table_entry(int d, double scale, int ssize, int* t) {
  float f = (float)((d + 0.5) * scale - 0.5);
  int s = (int)__builtin_floorf(f);
  f -= (float)s;
  if (s < 0) {
    f = 0.f;
    s = 0;
  }
  if (s >= ssize - 1) {
    f = 0.f;
    s = ssize - 1;
  }
  t[0] = s;
  t[1] = s + 1 < ssize - 1 ? s + 1 : ssize - 1;
  t[2] = (int)__builtin_rintf((1.f - f) * 2048.f);
  t[3] = (int)__builtin_rintf(f * 2048.f);
}

}  // namespace frhip

#pragma clang fp contract(on)
