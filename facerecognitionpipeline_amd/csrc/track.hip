// Track-level recognition on gfx950: FaceMatcher._aggregate_matches and _get_best_candidate
// (face_matcher.py:321-385) for a whole batch of tracks at once, over the top-k output of
// fr_match_topk / fr_embed_match while it is still in HBM.  One workgroup per track; a track's
// frames are a CSR slice of the [total][k] idx / score matrices, of which only column 0 (each
// frame's top-1) is read.  A gallery row stands for its student id (rows and ids are one-to-one).
//
//   quality frame   (double)score >= min_quality
//   pool            the quality frames, or every frame when there is none (:367-370)
//   votes           frames of the pool per gallery row; the rows rank by count, equal counts by
//                   their first pool frame (collections.Counter.most_common: a stable sort of
//                   insertion order); winner = rank 0, second = rank 1 (count 0 without one)
//   ratio           winner_count / pool_size
//   consensus       ratio > 0.5, or with a second row ratio > 0.4 && winner >= 2 * second (:339-343)
//   confidence      mean of the winner's pool scores
//   status          FEW_FRAMES (quality frames < min_frames), else NO_CONSENSUS, else
//                   BELOW_THRESHOLD (confidence < similarity_threshold), else RECOGNIZED
//
// Everything past the f32 score loads is integer or double arithmetic.  The counts and the ranking
// are integer reductions; the confidence sum runs in one fixed order (per thread in frame order,
// then block_reduce.h's block_sum_double: a fixed shuffle tree, then the four waves in order), so a
// track's record depends on nothing but its own frames.  Where the pool is the quality frames of
// the default min_quality (f32 scores in [0.55, 2): multiples of 2^-24) every partial sum of
// <= 1024 of them is exact in double, so that fixed order gives what any order gives.
#include "block_reduce.h"
#include "frhip_kernels.h"

#pragma clang fp contract(off)

namespace frhip {

namespace {

constexpr int TRACK_BLOCK = 256;
constexpr int TRACK_PER_THREAD = TRACK_MAX_FRAMES / TRACK_BLOCK;
static_assert(TRACK_MAX_FRAMES == 1024, "vote keys pack the first frame in 10 bits");

}  // namespace

__global__ __launch_bounds__(TRACK_BLOCK) void track_consensus_kernel(
    const int* __restrict__ idx, const float* __restrict__ score, int k, const int* __restrict__ offsets,
    double min_quality, int min_frames, double similarity_threshold, int* __restrict__ out_i,
    double* __restrict__ out_d) {
  __shared__ int rows[TRACK_MAX_FRAMES];
  __shared__ float sc[TRACK_MAX_FRAMES];
  __shared__ unsigned char in_pool[TRACK_MAX_FRAMES];
  __shared__ int red_i[4];
  __shared__ double red_d[4];
  const int tr = blockIdx.x, t = threadIdx.x;
  const int r0 = offsets[tr];
  const int N = offsets[tr + 1] - r0;  // 1..TRACK_MAX_FRAMES (checked by the host)
  // ---- top-1 of every frame into LDS; quality frames
  int nq_mine = 0;
  for (int i = t; i < N; i += TRACK_BLOCK) {
    const long long at = (long long)(r0 + i) * k;
    const float s = score[at];
    rows[i] = idx[at];
    sc[i] = s;
    nq_mine += (double)s >= min_quality;
  }
  const int nq = block_sum(nq_mine, red_i);
  const bool all = nq == 0;  // no quality frame: the pool is every frame
  const int pool = all ? N : nq;
  for (int i = t; i < N; i += TRACK_BLOCK) in_pool[i] = all || (double)sc[i] >= min_quality;
  __syncthreads();
  // ---- votes.  The first pool frame i of a row carries that row's key: count << 10 | (1023 - i),
  // so a larger key is a larger count, or at equal counts an earlier first frame; keys are unique.
  int key[TRACK_PER_THREAD];
  int kmax = 0;
#pragma unroll
  for (int m = 0; m < TRACK_PER_THREAD; ++m) {
    const int i = t + m * TRACK_BLOCK;
    key[m] = 0;
    if (i < N && in_pool[i]) {
      const int r = rows[i];
      int cnt = 0;
      bool earlier = false;
      for (int j = 0; j < N; ++j) {
        const bool same = rows[j] == r && in_pool[j];
        cnt += same;
        earlier |= same && j < i;
      }
      if (!earlier) key[m] = cnt << 10 | (TRACK_MAX_FRAMES - 1 - i);
    }
    kmax = max(kmax, key[m]);
  }
  const int wkey = block_max(kmax, red_i);  // > 0: the pool is never empty
  int kmax2 = 0;
#pragma unroll
  for (int m = 0; m < TRACK_PER_THREAD; ++m)
    if (key[m] != wkey) kmax2 = max(kmax2, key[m]);
  const int skey = block_max(kmax2, red_i);
  const int winner_count = wkey >> 10, second_count = skey >> 10;
  const int winner_row = rows[TRACK_MAX_FRAMES - 1 - (wkey & (TRACK_MAX_FRAMES - 1))];
  // ---- confidence: the winner's pool scores, summed in double in a fixed order
  double sum_mine = 0.0;
#pragma unroll
  for (int m = 0; m < TRACK_PER_THREAD; ++m) {
    const int i = t + m * TRACK_BLOCK;
    if (i < N && in_pool[i] && rows[i] == winner_row) sum_mine += (double)sc[i];
  }
  const double sum = block_sum_double(sum_mine, red_d);
  if (t != 0) return;
  const double confidence = sum / (double)winner_count;
  const double ratio = (double)winner_count / (double)pool;
  bool consensus = ratio > 0.5;
  if (!consensus && second_count > 0) consensus = ratio > 0.4 && winner_count >= 2 * second_count;
  int status = TRACK_RECOGNIZED;
  if (nq < min_frames)
    status = TRACK_FEW_FRAMES;
  else if (!consensus)
    status = TRACK_NO_CONSENSUS;
  else if (confidence < similarity_threshold)
    status = TRACK_BELOW_THRESHOLD;
  int* oi = out_i + (long long)tr * 8;
  oi[0] = status;
  oi[1] = winner_row;
  oi[2] = winner_count;
  oi[3] = pool;
  oi[4] = second_count;
  oi[5] = N;
  oi[6] = nq;
  oi[7] = 0;
  out_d[(long long)tr * 2] = confidence;
  out_d[(long long)tr * 2 + 1] = ratio;
}

hipError_t launch_track_consensus(const int* idx, const float* score, int k, const int* offsets, int n_tracks,
                                  double min_quality, int min_frames, double similarity_threshold, int* out_i,
                                  double* out_d, hipStream_t s) {
  if (n_tracks <= 0) return hipSuccess;
  hipLaunchKernelGGL(track_consensus_kernel, dim3(n_tracks), dim3(TRACK_BLOCK), 0, s, idx, score, k, offsets,
                     min_quality, min_frames, similarity_threshold, out_i, out_d);
  return hipGetLastError();
}

}  // namespace frhip
