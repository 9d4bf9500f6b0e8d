// The three identity aggregations of the evaluation notebook (aggregate_max / _mean / _topk), stated
// once for evaluate.hip's identity_agg_kernel and identify.hip's match_small_kernel: the score of
// an identity depends on nothing but its similarity values, whichever kernel staged them.
#pragma once
#include <hip/hip_runtime.h>

#include "frhip_kernels.h"

namespace frhip {

// |norm - 1| < 0.01: cosine_similarity takes the plain dot when both rows pass.
__device__ __forceinline__ bool unit_norm(float nrm) { return fabsf(nrm - 1.0f) < 0.01f; }

// The score of the identity whose similarity values are tile[a .. b) (1 <= b - a <= EVAL_MAX_ROWS), in
// row order: the f32 maximum, the f32 rounding of (double sum in row order) / count, or the
// min(k, count) largest values summed in double in descending order over their number (k <= EVAL_MAX_K).
// Everything is f32 compares or double sums in one fixed order that depends on nothing but b - a.
template <int AGG>
__device__ __forceinline__ float aggregate_identity(const float* tile, int a, int b, int k) {
  float res;
  if (AGG == AGG_MAX) {
    res = tile[a];
    for (int r = a + 1; r < b; ++r) res = fmaxf(res, tile[r]);
  } else if (AGG == AGG_MEAN) {
    double s = 0.0;
    for (int r = a; r < b; ++r) s += (double)tile[r];
    res = (float)(s / (double)(b - a));
  } else {
    // the EVAL_MAX_K largest values in descending order (a value pushes the smaller ones down)
    float top[EVAL_MAX_K];
#pragma unroll
    for (int j = 0; j < EVAL_MAX_K; ++j) top[j] = -INFINITY;
    for (int r = a; r < b; ++r) {
      float v = tile[r];
      if (!(v > top[EVAL_MAX_K - 1])) continue;
#pragma unroll
      for (int j = 0; j < EVAL_MAX_K; ++j) {
        const float hi = fmaxf(top[j], v);
        v = fminf(top[j], v);
        top[j] = hi;
      }
    }
    const int m = min(k, b - a);
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < EVAL_MAX_K; ++j)
      if (j < m) s += (double)top[j];
    res = (float)(s / (double)m);
  }
  return res;
}

}  // namespace frhip
