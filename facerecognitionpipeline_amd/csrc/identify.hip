// Identity matching on gfx950, the serving counterpart of evaluate.hip: a few queries against the
// handle's resident sample gallery (fr_samples_set), every identity scored over all of its rows.
//
//   match_small_kernel   serving-sized batches (fr_match_identities: one query, or up to
//                        IDENT_SMALL_N with n x rows <= IDENT_QUERY_ROWS): the raw
//                        dots, cosine_similarity's 0.01 rule and aggregate_max / _mean / _topk per
//                        identity in one launch; only the [n][n_ids] scores reach HBM.
//
// A workgroup takes one query and one tile, a run of consecutive whole identities of at most
// IDENT_TILE_ROWS rows (an identity longer than that is a tile of its own, up to EVAL_MAX_ROWS rows;
// fr_samples_set cuts the tiles).  The query row stays in LDS, unscaled; its norm is
// row_norms_kernel's: every wave loads the row as that kernel's one wave does and sums the same
// double terms in the same order.  Groups of 4 lanes dot gallery rows as scores_small_kernel does,
// a quarter of the 512 dimensions per lane (32 float4 loads, 8 in flight), the quarters summed in
// a fixed order; the dot goes through the 0.01 rule on the stored row norms into an LDS tile, and
// each thread then owns identities of the tile and aggregates them with the loop evaluate.hip
// uses (identity_agg.h).  out[p][i] depends on nothing but query p and identity i's rows.
//
// Workgroups of one tile are neighbours in the grid (the query index runs fastest), so the n
// readers of a tile's rows run close together.  Every query still reads every row: measured, the
// launch's time grows with n x rows, which is what fr_match_identities' rule reads.
#include <climits>

#include "block_reduce.h"
#include "frhip_kernels.h"

#pragma clang fp contract(off)

#include "identity_agg.h"

namespace frhip {

namespace {

constexpr int IDENT_BLOCK = 256;
constexpr int IDENT_PASS_ROWS = IDENT_BLOCK / 4;  // gallery rows one pass of the workgroup dots

template <int AGG>
__global__ __launch_bounds__(IDENT_BLOCK) void match_small_kernel(
    const float* __restrict__ Q, int n, const float* __restrict__ E, const float* __restrict__ enorm,
    const int* __restrict__ e_any_off, const int* __restrict__ offsets, int n_ids, const int* __restrict__ tiles,
    int k, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float qs[512];
  __shared__ float tile[EVAL_MAX_ROWS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int tl = blockIdx.x / n, p = blockIdx.x - tl * n;
  const int i0 = tiles[tl], i1 = tiles[tl + 1];
  const int r0 = offsets[i0], r1 = offsets[i1];  // r1 - r0 <= EVAL_MAX_ROWS (fr_samples_set)
  // the query row and its norm, in every wave as row_norms_kernel's wave has them
  const float4* qg = reinterpret_cast<const float4*>(Q + (long long)p * 512);
  float4 qv[2];
  double s = 0.0;
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const float4 v = qg[lane + 64 * m];
    s += (double)v.x * (double)v.x;
    s += (double)v.y * (double)v.y;
    s += (double)v.z * (double)v.z;
    s += (double)v.w * (double)v.w;
    qv[m] = v;
  }
  s = wave_sum(s);
  const float qn = (float)sqrt(s);
  const bool q_unit = unit_norm(qn);
  const bool plain = q_unit && *e_any_off == 0;  // every pair of this query is the plain dot
  if (w == 0) {
    reinterpret_cast<float4*>(qs)[lane] = qv[0];
    reinterpret_cast<float4*>(qs)[lane + 64] = qv[1];
  }
  __syncthreads();
  const int part = lane >> 4;
  const float4* q4 = reinterpret_cast<const float4*>(qs + part * 128);
  for (int base = r0; base < r1; base += IDENT_PASS_ROWS) {  // uniform: every lane reaches the shuffles
    const int row = base + w * 16 + (lane & 15);
    float acc = 0.f;
    if (row < r1) {
      const float4* g4 = reinterpret_cast<const float4*>(E + (long long)row * 512 + part * 128);
      for (int c0 = 0; c0 < 32; c0 += 8) {
        float4 a[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) a[u] = g4[c0 + u];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const float4 b = q4[c0 + u];
          acc = fmaf(a[u].x, b.x, acc);
          acc = fmaf(a[u].y, b.y, acc);
          acc = fmaf(a[u].z, b.z, acc);
          acc = fmaf(a[u].w, b.w, acc);
        }
      }
    }
    // quarters in order: (p0 + p1) + (p2 + p3)
    const float o1 = __shfl_xor(acc, 16, 64);
    const float s01 = (lane & 16) ? o1 + acc : acc + o1;
    const float o2 = __shfl_xor(s01, 32, 64);
    float v = (lane & 32) ? o2 + s01 : s01 + o2;
    if (part == 0 && row < r1) {
      if (!plain) {
        const float en = enorm[row];
        if (!(q_unit && unit_norm(en))) v = v / (qn * en);
      }
      tile[row - r0] = v;
    }
  }
  __syncthreads();
  for (int i = i0 + tid; i < i1; i += IDENT_BLOCK) {
    const int a = offsets[i] - r0, b = offsets[i + 1] - r0;  // 1 <= b - a <= EVAL_MAX_ROWS
    out[(long long)p * n_ids + i] = aggregate_identity<AGG>(tile, a, b, k);
  }
}

}  // namespace

hipError_t launch_match_small(const float* Q, int n, const float* E, const float* enorm, const int* e_any_off,
                              const int* offsets, int n_ids, const int* tiles, int n_tiles, int aggregation, int k,
                              float* out, hipStream_t s) {
  if (n <= 0 || n_tiles <= 0) return hipSuccess;
  if ((long long)n * n_tiles > INT_MAX) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((long long)n * n_tiles)), block(IDENT_BLOCK);
  if (aggregation == AGG_MAX)
    hipLaunchKernelGGL(match_small_kernel<AGG_MAX>, grid, block, 0, s, Q, n, E, enorm, e_any_off, offsets, n_ids,
                       tiles, k, out);
  else if (aggregation == AGG_MEAN)
    hipLaunchKernelGGL(match_small_kernel<AGG_MEAN>, grid, block, 0, s, Q, n, E, enorm, e_any_off, offsets, n_ids,
                       tiles, k, out);
  else if (aggregation == AGG_TOPK)
    hipLaunchKernelGGL(match_small_kernel<AGG_TOPK>, grid, block, 0, s, Q, n, E, enorm, e_any_off, offsets, n_ids,
                       tiles, k, out);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace frhip
