// Model evaluation on gfx950: the identification and verification loops of the reference's
// evaluate_models_v2.ipynb over score matrices that stay in HBM.
//
//   row_norms_kernel      np.linalg.norm of every probe and gallery row, once per call
//   identity_agg_kernel   cosine_similarity's 0.01 rule on each raw dot of the score GEMM, then
//                         aggregate_max / aggregate_mean / aggregate_topk per identity (a CSR slice
//                         of gallery rows) as identify_probe applies them
//   eval_probes_kernel    identify_probe(threshold=0.0)'s best identity, compute_rank_metrics' rank,
//                         the genuine / impostor scores and the tp / fp / fn counts of a threshold
//                         list (the loops of evaluate_{probes,verification,impostors}_comprehensive)
//
// identity_agg_kernel: a workgroup takes one probe and one tile, a run of consecutive identities of
// at most EVAL_TILE_ROWS gallery rows.  The tile's slice of the probe's score row is contiguous; it
// is loaded coalesced into LDS once, and each thread then owns identities of the tile and walks
// their values in row order.  One-row identities therefore cost one thread each, not a wave, and a
// 1024-row identity is one thread's loop (identity_agg.h, shared with identify.hip's serving
// kernel).  Everything past the f32 loads is f32 compares or double
// sums in one fixed order that depends on nothing but the identity's row count, so out[p] depends
// on nothing but sim[p] and the offsets.
//
// eval_probes_kernel: a workgroup walks probes blockIdx.x, + gridDim.x, ...; its 256 threads scan the
// probe's score row and reduce (best, rank counts, impostor maximum) over integers and f32
// compares.  Thread j keeps the four counts of threshold j in registers over all of the workgroup's
// probes and adds them to counts[j] with integer atomics at the end.
#include <algorithm>
#include <climits>

#include "block_reduce.h"
#include "frhip_kernels.h"

#pragma clang fp contract(off)

#include "identity_agg.h"

namespace frhip {

namespace {

constexpr int EVAL_BLOCK = 256;
static_assert(EVAL_MAX_THRESHOLDS <= EVAL_BLOCK, "thread j owns threshold j");
static_assert(EVAL_MAX_ROWS <= EVAL_TILE_ROWS, "an identity fits one tile");

// One wave per 512-float row.
__global__ __launch_bounds__(EVAL_BLOCK) void row_norms_kernel(const float* __restrict__ x, int n,
                                                               float* __restrict__ norm, int* __restrict__ any_off) {
  const int row = blockIdx.x * (EVAL_BLOCK / 64) + (threadIdx.x >> 6);
  if (row >= n) return;
  const int lane = threadIdx.x & 63;
  const float4* p = reinterpret_cast<const float4*>(x + (long long)row * 512);
  double s = 0.0;
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const float4 v = p[lane + 64 * m];
    s += (double)v.x * (double)v.x;
    s += (double)v.y * (double)v.y;
    s += (double)v.z * (double)v.z;
    s += (double)v.w * (double)v.w;
  }
  s = wave_sum(s);
  if (lane != 0) return;
  const float nrm = (float)sqrt(s);
  norm[row] = nrm;
  if (any_off && !unit_norm(nrm)) atomicOr(any_off, 1);
}

template <int AGG>
__global__ __launch_bounds__(EVAL_BLOCK) void identity_agg_kernel(
    float* __restrict__ sim, int G, const int* __restrict__ offsets, int n_ids, const int* __restrict__ tiles,
    int n_tiles, const float* __restrict__ qnorm, const float* __restrict__ enorm, const int* __restrict__ e_any_off,
    int k, int write_sim, float* __restrict__ out) {
  __shared__ float tile[EVAL_TILE_ROWS];
  const int t = threadIdx.x;
  const int p = blockIdx.x / n_tiles, tl = blockIdx.x - p * n_tiles;
  const int i0 = tiles[tl], i1 = tiles[tl + 1];
  const int r0 = offsets[i0], r1 = offsets[i1];  // r1 - r0 <= EVAL_TILE_ROWS (fr_identity_scores)
  float* row = sim + (long long)p * G;
  const float qn = qnorm[p];
  const bool q_unit = unit_norm(qn);
  const bool plain = q_unit && *e_any_off == 0;  // every pair of this row is the plain dot
  for (int r = r0 + t; r < r1; r += EVAL_BLOCK) {
    float v = row[r];
    if (!plain) {
      const float en = enorm[r];
      if (!(q_unit && unit_norm(en))) {
        v = v / (qn * en);
        if (write_sim) row[r] = v;
      }
    }
    tile[r - r0] = v;
  }
  __syncthreads();
  for (int i = i0 + t; i < i1; i += EVAL_BLOCK) {
    const int a = offsets[i] - r0, b = offsets[i + 1] - r0;  // 1 <= b - a <= EVAL_MAX_ROWS
    out[(long long)p * n_ids + i] = aggregate_identity<AGG>(tile, a, b, k);
  }
}

__global__ __launch_bounds__(EVAL_BLOCK) void eval_probes_kernel(
    const float* __restrict__ scores, int n, int n_ids, const int* __restrict__ true_id,
    const double* __restrict__ thr, int n_thr, int* __restrict__ rec_i, float* __restrict__ rec_f,
    unsigned long long* __restrict__ counts) {
  __shared__ float red_bv[4], red_mo[4];
  __shared__ int red_bi[4], red_gt[4], red_eq[4];
  const int t = threadIdx.x;
  const double my_thr = t < n_thr ? thr[t] : 0.0;
  unsigned long long c_tp = 0, c_fp = 0, c_fn = 0, c_gen = 0;
  for (int p = blockIdx.x; p < n; p += gridDim.x) {
    const float* a = scores + (long long)p * n_ids;
    const int tid = true_id[p];
    const bool enrolled = tid >= 0 && tid < n_ids;
    const float at = enrolled ? a[tid] : 0.0f;
    float bv = -INFINITY, mo = -INFINITY;
    int bi = INT_MAX, gt = 0, eq = 0;
    for (int j = t; j < n_ids; j += EVAL_BLOCK) {
      const float v = a[j];
      if (v > bv) {  // j rises: equal scores keep the lower index
        bv = v;
        bi = j;
      }
      if (enrolled) {
        gt += v > at;
        eq += v == at && j < tid;
        if (j != tid) mo = fmaxf(mo, v);
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(bv, off, 64);
      const int oi = __shfl_xor(bi, off, 64);
      if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
      }
      gt += __shfl_xor(gt, off, 64);
      eq += __shfl_xor(eq, off, 64);
      mo = fmaxf(mo, __shfl_xor(mo, off, 64));
    }
    __syncthreads();  // the previous probe's reads of red_* are done
    if ((t & 63) == 0) {
      const int w = t >> 6;
      red_bv[w] = bv;
      red_bi[w] = bi;
      red_gt[w] = gt;
      red_eq[w] = eq;
      red_mo[w] = mo;
    }
    __syncthreads();
    bv = red_bv[0];
    bi = red_bi[0];
    gt = red_gt[0];
    eq = red_eq[0];
    mo = red_mo[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      if (red_bv[w] > bv || (red_bv[w] == bv && red_bi[w] < bi)) {
        bv = red_bv[w];
        bi = red_bi[w];
      }
      gt += red_gt[w];
      eq += red_eq[w];
      mo = fmaxf(mo, red_mo[w]);
    }
    if (bi == INT_MAX) bi = 0;  // no score above -inf (not a valid input): still an identity in range
    const int predicted = bv < 0.0f ? -1 : bi;
    const float genuine = at;  // 0.0f when not enrolled
    const bool has_imp = !enrolled || n_ids > 1;
    const float impostor = !enrolled ? bv : (n_ids > 1 ? mo : -1.0f);
    if (t == 0) {
      int* ri = rec_i + (long long)p * 4;
      ri[0] = predicted;
      ri[1] = bi;
      ri[2] = enrolled ? 1 + gt + eq : 0;
      ri[3] = has_imp;
      float* rf = rec_f + (long long)p * 4;
      rf[0] = bv;
      rf[1] = genuine;
      rf[2] = impostor;
      rf[3] = 0.0f;
    }
    const bool accepted = (double)bv >= my_thr;
    const bool tp = accepted && enrolled && predicted == tid;
    c_tp += tp;
    c_fp += accepted && !tp;
    c_fn += !accepted;
    c_gen += enrolled && (double)genuine >= my_thr;
  }
  if (t < n_thr) {
    unsigned long long* c = counts + (long long)t * 4;
    if (c_tp) atomicAdd(c + 0, c_tp);
    if (c_fp) atomicAdd(c + 1, c_fp);
    if (c_fn) atomicAdd(c + 2, c_fn);
    if (c_gen) atomicAdd(c + 3, c_gen);
  }
}

}  // namespace

hipError_t launch_row_norms(const float* x, int n, float* norm, int* any_off, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int rows_per_block = EVAL_BLOCK / 64;
  hipLaunchKernelGGL(row_norms_kernel, dim3((n + rows_per_block - 1) / rows_per_block), dim3(EVAL_BLOCK), 0, s, x, n,
                     norm, any_off);
  return hipGetLastError();
}

hipError_t launch_identity_agg(float* sim, int n, int G, const int* offsets, int n_ids, const int* tiles, int n_tiles,
                               const float* qnorm, const float* enorm, const int* e_any_off, int aggregation, int k,
                               bool write_sim, float* out, hipStream_t s) {
  if (n <= 0 || n_tiles <= 0) return hipSuccess;
  if ((long long)n * n_tiles > INT_MAX) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((long long)n * n_tiles)), block(EVAL_BLOCK);
  const int ws = write_sim ? 1 : 0;
  if (aggregation == AGG_MAX)
    hipLaunchKernelGGL(identity_agg_kernel<AGG_MAX>, grid, block, 0, s, sim, G, offsets, n_ids, tiles, n_tiles, qnorm,
                       enorm, e_any_off, k, ws, out);
  else if (aggregation == AGG_MEAN)
    hipLaunchKernelGGL(identity_agg_kernel<AGG_MEAN>, grid, block, 0, s, sim, G, offsets, n_ids, tiles, n_tiles, qnorm,
                       enorm, e_any_off, k, ws, out);
  else if (aggregation == AGG_TOPK)
    hipLaunchKernelGGL(identity_agg_kernel<AGG_TOPK>, grid, block, 0, s, sim, G, offsets, n_ids, tiles, n_tiles, qnorm,
                       enorm, e_any_off, k, ws, out);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_eval_probes(const float* scores, int n, int n_ids, const int* true_id, const double* thr, int n_thr,
                              int* rec_i, float* rec_f, long long* counts, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(eval_probes_kernel, dim3(std::min(n, 2048)), dim3(EVAL_BLOCK), 0, s, scores, n, n_ids, true_id,
                     thr, n_thr, rec_i, rec_f, reinterpret_cast<unsigned long long*>(counts));
  return hipGetLastError();
}

}  // namespace frhip
