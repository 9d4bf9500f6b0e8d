// Photograph roll call on gfx950: who is in each photograph, decided for all faces of all photographs
// in one launch over the top-k output of fr_match_topk / fr_embed_match / fr_match_identities while
// it is still in HBM.  One workgroup per photograph; a photograph's faces are a CSR slice of the
// [total][k] idx / score matrices.  A gallery row (or identity index) stands for its student.
//
//   claim        a column c of a face with (double)score[f][c] >= similarity_threshold (the
//                comparison FaceMatcher.match_single_image makes on the Python float; never a NaN)
//   INDEPENDENT  the reference's rule: RECOGNIZED if column 0 is a claim, else CANDIDATE
//   EXCLUSIVE    all claims of the photograph by score descending (as f32 values), then face, then
//                column ascending; scanned in that order a claim is granted if its face holds nothing
//                yet and no face holds its row.  A face with a grant is RECOGNIZED with that row,
//                score and column; one whose column 0 was a claim but which got nothing is DISPLACED;
//                one whose column 0 was no claim is CANDIDATE (both report column 0).
//
// The scan is run as rounds.  Each free face keeps its candidate: its best claim (score, then lower
// column: its first claim in the scan order) whose row is not yet held.  A round takes the block
// maximum over the candidates of a 64-bit key -- the order-preserving image of the f32 score, then the
// inverted face index -- which is the first claim of the scan order that can still be granted; the
// winner's row goes into the held set, and the faces whose candidate was that row look for their
// next one.  The loop ends when no face has a candidate left: one round per grant.  The held set is
// an open-addressing table in LDS keyed by the row (at most 1024 grants in 2048 slots): a row is
// compared, never used as an address.  Only comparisons, no floating-point arithmetic: the result is
// exact and depends on nothing but the photograph's own faces.
#include "block_reduce.h"
#include "frhip_kernels.h"

namespace frhip {

namespace {

constexpr int ROLLCALL_BLOCK = 256;
constexpr int ROLLCALL_PER_THREAD = ROLLCALL_MAX_FACES / ROLLCALL_BLOCK;
constexpr int ROLLCALL_SLOTS = 2 * ROLLCALL_MAX_FACES;  // load <= 1/2: a probe always meets a free slot
static_assert(ROLLCALL_MAX_FACES == 1024, "round keys pack the face in 10 bits");

// Order-preserving image of a non-NaN f32 (a < b as floats <=> image(a) < image(b) as unsigned, the
// two zeros equal); > 0 for every such value.
__device__ __forceinline__ unsigned ordered_bits(float s) {
  const unsigned b = s == 0.0f ? 0u : __float_as_uint(s);
  return b & 0x80000000u ? ~b : b | 0x80000000u;
}

__device__ __forceinline__ unsigned row_slot(int row) { return ((unsigned)row * 2654435761u) >> 21; }
static_assert(ROLLCALL_SLOTS == 1 << 11, "row_slot keeps the top 11 bits");

__device__ __forceinline__ bool row_held(const int* tab_key, const unsigned char* tab_used, int row) {
  for (unsigned s = row_slot(row);; s = (s + 1) & (ROLLCALL_SLOTS - 1)) {
    if (!tab_used[s]) return false;
    if (tab_key[s] == row) return true;
  }
}

}  // namespace

__global__ __launch_bounds__(ROLLCALL_BLOCK) void photo_rollcall_kernel(
    const int* __restrict__ idx, const float* __restrict__ score, int k, const int* __restrict__ offsets,
    double similarity_threshold, int mode, int* __restrict__ out_face, float* __restrict__ out_score,
    int* __restrict__ out_image) {
  __shared__ int tab_key[ROLLCALL_SLOTS];
  __shared__ unsigned char tab_used[ROLLCALL_SLOTS];
  __shared__ unsigned long long red_k[4];
  __shared__ int red_i[4];
  __shared__ int taken_row;
  const int p = blockIdx.x, t = threadIdx.x;
  const int f0 = offsets[p];
  const int N = offsets[p + 1] - f0;  // 0..ROLLCALL_MAX_FACES (checked by the host)
  for (int s = t; s < ROLLCALL_SLOTS; s += ROLLCALL_BLOCK) tab_used[s] = 0;
  __syncthreads();
  // what a face reports: column 0 until a claim is granted
  int status[ROLLCALL_PER_THREAD], rep_row[ROLLCALL_PER_THREAD], rep_col[ROLLCALL_PER_THREAD];
  float rep_score[ROLLCALL_PER_THREAD];
  // a free face's candidate: cand_ord == 0 for none
  unsigned cand_ord[ROLLCALL_PER_THREAD];
  int cand_row[ROLLCALL_PER_THREAD], cand_col[ROLLCALL_PER_THREAD];
  float cand_score[ROLLCALL_PER_THREAD];
  // The best claim of face i (slot m of this thread) whose row is not held.
  auto select = [&](int m, int i) {
    const long long at = (long long)(f0 + i) * k;
    unsigned best = 0;
    for (int c = 0; c < k; ++c) {
      const float s = score[at + c];
      if (!((double)s >= similarity_threshold)) continue;
      const unsigned o = ordered_bits(s);
      if (o <= best) continue;  // equal scores: the lower column stays
      const int r = idx[at + c];
      if (row_held(tab_key, tab_used, r)) continue;
      best = o;
      cand_row[m] = r;
      cand_col[m] = c;
      cand_score[m] = s;
    }
    cand_ord[m] = best;
  };
#pragma unroll
  for (int m = 0; m < ROLLCALL_PER_THREAD; ++m) {
    const int i = t + m * ROLLCALL_BLOCK;
    cand_ord[m] = 0;
    status[m] = FACE_CANDIDATE;
    if (i < N) {
      const long long at = (long long)(f0 + i) * k;
      rep_row[m] = idx[at];
      rep_score[m] = score[at];
      rep_col[m] = 0;
      const bool claim0 = (double)rep_score[m] >= similarity_threshold;
      if (mode == ROLLCALL_INDEPENDENT) {
        if (claim0) status[m] = FACE_RECOGNIZED;
      } else {
        if (claim0) status[m] = FACE_DISPLACED;  // until a round grants it a claim
        select(m, i);                            // nothing is held yet
      }
    }
  }
  if (mode != ROLLCALL_INDEPENDENT) {
    for (;;) {
      unsigned long long mine = 0;
#pragma unroll
      for (int m = 0; m < ROLLCALL_PER_THREAD; ++m) {
        const unsigned long long key =
            (unsigned long long)cand_ord[m] << 32 | (unsigned)(ROLLCALL_MAX_FACES - 1 - (t + m * ROLLCALL_BLOCK));
        if (cand_ord[m] && key > mine) mine = key;
      }
      const unsigned long long won = block_max_u64(mine, red_k);
      if (won == 0) break;  // the same value in every thread
      const int winner = ROLLCALL_MAX_FACES - 1 - (int)(won & (ROLLCALL_MAX_FACES - 1));
#pragma unroll
      for (int m = 0; m < ROLLCALL_PER_THREAD; ++m) {
        if (t + m * ROLLCALL_BLOCK != winner) continue;
        status[m] = FACE_RECOGNIZED;
        rep_row[m] = cand_row[m];
        rep_col[m] = cand_col[m];
        rep_score[m] = cand_score[m];
        cand_ord[m] = 0;
        // the table was last read before block_max_u64's barriers: this thread alone writes it now
        unsigned s = row_slot(rep_row[m]);
        while (tab_used[s]) s = (s + 1) & (ROLLCALL_SLOTS - 1);  // the row is not in the table: it was no candidate else
        tab_key[s] = rep_row[m];
        tab_used[s] = 1;
        taken_row = rep_row[m];
      }
      __syncthreads();
      const int taken = taken_row;  // next written after the next round's block_max_u64
#pragma unroll
      for (int m = 0; m < ROLLCALL_PER_THREAD; ++m)
        if (cand_ord[m] && cand_row[m] == taken) select(m, t + m * ROLLCALL_BLOCK);
    }
  }
  int n_rec = 0, n_cand = 0, n_disp = 0;
#pragma unroll
  for (int m = 0; m < ROLLCALL_PER_THREAD; ++m) {
    const int i = t + m * ROLLCALL_BLOCK;
    if (i >= N) continue;
    int* of = out_face + (long long)(f0 + i) * 4;
    of[0] = status[m];
    of[1] = rep_row[m];
    of[2] = rep_col[m];
    of[3] = 0;
    out_score[f0 + i] = rep_score[m];
    n_rec += status[m] == FACE_RECOGNIZED;
    n_cand += status[m] == FACE_CANDIDATE;
    n_disp += status[m] == FACE_DISPLACED;
  }
  n_rec = block_sum(n_rec, red_i);
  n_cand = block_sum(n_cand, red_i);
  n_disp = block_sum(n_disp, red_i);
  if (t != 0) return;
  int* oi = out_image + (long long)p * 4;
  oi[0] = N;
  oi[1] = n_rec;
  oi[2] = n_cand;
  oi[3] = n_disp;
}

hipError_t launch_photo_rollcall(const int* idx, const float* score, int k, const int* offsets, int n_images,
                                 double similarity_threshold, int mode, int* out_face, float* out_score,
                                 int* out_image, hipStream_t s) {
  if (n_images <= 0) return hipSuccess;
  hipLaunchKernelGGL(photo_rollcall_kernel, dim3(n_images), dim3(ROLLCALL_BLOCK), 0, s, idx, score, k, offsets,
                     similarity_threshold, mode, out_face, out_score, out_image);
  return hipGetLastError();
}

}  // namespace frhip
