// Capture sessions on gfx950: SimpleTracker.update and FrameAccumulator (face_detection.py:11-228)
// with the is_valid test of CameraFaceCapture.process_frame (:271-283), for a batch of independent
// clips (cameras) in one launch.  One workgroup per clip: a clip's frames are sequential, so the
// parallelism is across clips, across the track x detection pairs of a frame and across the
// detections of a clip.  A clip's detections are a CSR slice (frames of the clip, detections of
// each frame).
//
//   tracker      The live tracks are an ordered list in LDS (the reference's dict insertion order):
//                id, sx = x1 + x2, sy = y1 + y2, disappeared.  A pair's q = (sx_t - sx_d)^2 +
//                (sy_t - sy_d)^2 in int64 is 4 x the squared centroid distance, exact.  The greedy
//                loop takes the unmatched pair with the smallest key (q << 14 | flat index) among
//                those with q < q_limit; the flat index track_pos * n_dets + det_idx breaks ties as
//                numpy's argmin does.  A round commits every pair that is the best of its track
//                and of its detection, which are the pairs that loop is bound to take (see the
//                rounds below).  Nothing of size tracks x detections is stored; the pairs are
//                recomputed each round.  Then the unmatched tracks age and the dead ones leave by a
//                stable compaction, and the unmatched detections are appended in detection order
//                with the next ids.
//   accumulator  quality = compute_quality_score in double, in the reference's order of operations
//                (contraction off).  A detection passes when valid and !(quality < min_quality); a
//                track accepts its first target_frames passing detections; they are saved when
//                there are target_frames of them, or with save_partial.  slot = the rank by
//                descending quality, equal qualities in frame order (Python's stable
//                sort(reverse=True)).
//
// Everything but the quality is integer arithmetic, so a clip's result depends on nothing but the
// clip.  A clip that would hold more than CAPTURE_MAX_TRACKS live tracks, or has a coordinate beyond
// +-CAPTURE_COORD_MAX, gets its error word set, track_id 0 and slot -1 throughout, and nothing is
// written out of range.
#include "block_reduce.h"
#include "frhip_kernels.h"

#pragma clang fp contract(off)

namespace frhip {

namespace {

constexpr int CAP_BLOCK = 256;
constexpr int CAP_PER_THREAD = CAPTURE_MAX_DETS / CAP_BLOCK;
constexpr int CAP_INDEX_BITS = 14;  // flat index < CAPTURE_MAX_TRACKS * CAPTURE_MAX_FACES
static_assert(CAPTURE_MAX_TRACKS * CAPTURE_MAX_FACES <= (1 << CAP_INDEX_BITS), "flat pair index bits");
// |sx_t - sx_d| <= 4 * COORD_MAX, so q <= 2 * (4 * COORD_MAX)^2 = 2^45 and the key fits 60 bits
static_assert(CAPTURE_COORD_MAX == (1 << 20), "q << CAP_INDEX_BITS must stay below 2^63");
static_assert(CAPTURE_MAX_TRACKS + CAPTURE_MAX_FACES == CAP_BLOCK, "one thread per track and per detection");
static_assert(CAP_PER_THREAD <= 32, "accepted flags of a thread's detections are one int mask");

constexpr unsigned long long NO_PAIR = ~0ull;

// FrameAccumulator.compute_quality_score (face_detection.py:137-153)
__device__ __forceinline__ double quality_score(const double* m) {
  const double blur = m[1] / 200.0;
  const double nb = 1.0 < blur ? 1.0 : blur;  // min(blur / 200.0, 1.0)
  const double p = 1.0 - (fabs(m[2]) / 90.0 + fabs(m[3]) / 90.0 + fabs(m[4]) / 90.0) / 3.0;
  const double pose = p > 0.0 ? p : 0.0;  // max(0, pose_score)
  return (m[0] * 0.4 + nb * 0.3) + pose * 0.3;
}

}  // namespace

__global__ __launch_bounds__(CAP_BLOCK) void capture_tracks_kernel(
    const int* __restrict__ bbox, const double* __restrict__ metrics, const unsigned char* __restrict__ valid,
    const int* __restrict__ frame_off, const int* __restrict__ clip_off, int max_disappeared, long long q_limit,
    int target, double min_quality, int save_partial, int* __restrict__ track_id, double* __restrict__ quality,
    int* __restrict__ slot, int* __restrict__ clip_info) {
  // the live list, in the reference's dict order
  __shared__ int t_id[CAPTURE_MAX_TRACKS], t_sx[CAPTURE_MAX_TRACKS], t_sy[CAPTURE_MAX_TRACKS];
  __shared__ int t_dis[CAPTURE_MAX_TRACKS];
  __shared__ unsigned char t_flag[CAPTURE_MAX_TRACKS];  // matched in the greedy rounds, then: kept
  // the frame's detections
  __shared__ int d_sx[CAPTURE_MAX_FACES], d_sy[CAPTURE_MAX_FACES];
  __shared__ unsigned char d_matched[CAPTURE_MAX_FACES];
  // the clip's detections
  __shared__ int ids[CAPTURE_MAX_DETS];
  __shared__ double qual[CAPTURE_MAX_DETS];
  __shared__ unsigned char state[CAPTURE_MAX_DETS];  // bit 0: passes, bit 1: accepted
  __shared__ unsigned long long row_best[CAPTURE_MAX_TRACKS], col_best[CAPTURE_MAX_FACES];
  __shared__ int red_i[4];

  const int c = blockIdx.x, t = threadIdx.x;
  const int f0 = clip_off[c], f1 = clip_off[c + 1];
  const int d0 = frame_off[f0];
  const int n = frame_off[f1] - d0;  // 0..CAPTURE_MAX_DETS (checked by the host)
  int* info = clip_info + (long long)c * 4;

  // ---- qualities, the pass test and the coordinate range
  int bad = 0;
  for (int i = t; i < n; i += CAP_BLOCK) {
    const long long at = d0 + i;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int v = bbox[at * 4 + k];
      bad |= v > CAPTURE_COORD_MAX || v < -CAPTURE_COORD_MAX;
    }
    const double q = quality_score(metrics + at * 5);
    quality[at] = q;
    qual[i] = q;
    state[i] = valid[at] != 0 && !(q < min_quality);
  }
  int error = block_sum(bad, red_i) > 0 ? CAPTURE_ERR_COORD : 0;

  // ---- the tracker, frame by frame.  Its loops over the list and over the frame's detections
  // are short and wait on LDS: they are unrolled by 4 so that the reads of four entries overlap.
  // nt, next_id and every branch around a barrier are the same in all threads: they come from LDS,
  // from the offsets or from a block reduction.
  int nt = 0, next_id = 1;
  for (int f = f0; f < f1 && !error; ++f) {
    const int b = frame_off[f] - d0;
    const int nd = frame_off[f + 1] - frame_off[f];  // 0..CAPTURE_MAX_FACES (checked by the host)
    if (t < nd) {
      const int* bb = bbox + (long long)(d0 + b + t) * 4;
      d_sx[t] = bb[0] + bb[2];
      d_sy[t] = bb[1] + bb[3];
      d_matched[t] = 0;
    }
    if (t < nt) t_flag[t] = 0;
    __syncthreads();
    // Greedy matching, many pairs to a round.  Keys are distinct (they carry the flat index), so
    // the greedy order is a strict order of the pairs.  A free pair whose key is the smallest of
    // its track's free pairs and of its detection's free pairs is taken by the greedy loop whatever
    // else happens: any pair taken before it would have a smaller key and share its track or its
    // detection.  So every such pair is committed at once, and the rest is the same problem
    // again.  The smallest free key of all is always one of them: a round without a commit means
    // no free pair is left under q_limit (distances.min() >= max_distance), after at most
    // min(tracks, dets) rounds.  Threads 0..127 scan for the tracks, threads 128..255 for the
    // detections; the scans read LDS words that are the same for every thread (broadcasts).
    while (nt > 0 && nd > 0) {
      unsigned long long best = NO_PAIR;
      if (t < CAPTURE_MAX_TRACKS) {
        if (t < nt && !t_flag[t]) {
          const long long sx = t_sx[t], sy = t_sy[t];
#pragma unroll 4
          for (int di = 0; di < nd; ++di) {
            const long long dx = sx - d_sx[di], dy = sy - d_sy[di];
            const long long q = dx * dx + dy * dy;
            const unsigned long long key = (unsigned long long)q << CAP_INDEX_BITS | (unsigned)(t * nd + di);
            if (!d_matched[di] && q < q_limit && key < best) best = key;
          }
        }
        row_best[t] = best;
      } else {
        const int di = t - CAPTURE_MAX_TRACKS;
        if (di < nd && !d_matched[di]) {
          const long long sx = d_sx[di], sy = d_sy[di];
#pragma unroll 4
          for (int tp = 0; tp < nt; ++tp) {
            const long long dx = t_sx[tp] - sx, dy = t_sy[tp] - sy;
            const long long q = dx * dx + dy * dy;
            const unsigned long long key = (unsigned long long)q << CAP_INDEX_BITS | (unsigned)(tp * nd + di);
            if (!t_flag[tp] && q < q_limit && key < best) best = key;
          }
        }
        col_best[di] = best;
      }
      __syncthreads();
      int commit = 0;
      if (t < nt) {
        const unsigned long long key = row_best[t];
        if (key != NO_PAIR) {
          const int di = (int)(key & ((1u << CAP_INDEX_BITS) - 1)) - t * nd;
          if (col_best[di] == key) {  // the track's and the detection's best pair: pairs are disjoint
            commit = 1;
            t_flag[t] = 1;
            d_matched[di] = 1;
            t_sx[t] = d_sx[di];
            t_sy[t] = d_sy[di];
            t_dis[t] = 0;
            ids[b + di] = t_id[t];
          }
        }
      }
      if (!__syncthreads_or(commit)) break;
    }
    // unmatched tracks age; those past max_disappeared leave
    int my_id = 0, my_sx = 0, my_sy = 0, my_dis = 0;
    bool keep = false;
    if (t < nt) {
      my_id = t_id[t], my_sx = t_sx[t], my_sy = t_sy[t];
      my_dis = t_flag[t] ? 0 : t_dis[t] + 1;
      keep = my_dis <= max_disappeared;
      t_flag[t] = keep;
    }
    __syncthreads();
    int pos = 0, kept = 0;
#pragma unroll 4
    for (int j = 0; j < nt; ++j) {
      const int k = t_flag[j];
      pos += j < t ? k : 0;
      kept += k;
    }
    int rank = 0, opened = 0;
#pragma unroll 4
    for (int j = 0; j < nd; ++j) {
      const int u = !d_matched[j];
      rank += j < t ? u : 0;
      opened += u;
    }
    if (kept + opened > CAPTURE_MAX_TRACKS) {
      error = CAPTURE_ERR_TRACKS;
      break;
    }
    __syncthreads();  // every thread has read its own entry and the flags
    if (keep) t_id[pos] = my_id, t_sx[pos] = my_sx, t_sy[pos] = my_sy, t_dis[pos] = my_dis;
    if (t < nd && !d_matched[t]) {  // a new track per unmatched detection, in detection order
      const int at = kept + rank;
      t_id[at] = next_id + rank, t_sx[at] = d_sx[t], t_sy[at] = d_sy[t], t_dis[at] = 0;
      ids[b + t] = next_id + rank;
    }
    nt = kept + opened;
    next_id += opened;
    __syncthreads();
  }

  if (error) {
    for (int i = t; i < n; i += CAP_BLOCK) {
      track_id[d0 + i] = 0;
      slot[d0 + i] = -1;
    }
    if (t == 0) info[0] = 0, info[1] = 0, info[2] = 0, info[3] = error;
    return;
  }
  __syncthreads();

  // ---- the accumulator over the whole clip.  A track has at most one detection per frame, so the
  // clip order of a track's detections is its frame order.
  unsigned accepted_mask = 0;
  int completed = 0;
#pragma unroll 1
  for (int m = 0; m < CAP_PER_THREAD; ++m) {
    const int i = t + m * CAP_BLOCK;
    if (i >= n || !(state[i] & 1)) continue;
    const int id = ids[i];
    int before = 0;
#pragma unroll 4
    for (int j = 0; j < i; ++j) before += (state[j] & 1) && ids[j] == id;
    if (before < target) accepted_mask |= 1u << m;
    completed += before == target - 1;  // the detection that completes its track
  }
  __syncthreads();
#pragma unroll 1
  for (int m = 0; m < CAP_PER_THREAD; ++m)
    if (accepted_mask >> m & 1) state[t + m * CAP_BLOCK] = 3;
  __syncthreads();
  int saved = 0;
#pragma unroll 1
  for (int m = 0; m < CAP_PER_THREAD; ++m) {
    const int i = t + m * CAP_BLOCK;
    if (i >= n) continue;
    int s = -1;
    if (accepted_mask >> m & 1) {
      const int id = ids[i];
      const double q = qual[i];
      int count = 0, ahead = 0;
#pragma unroll 4
      for (int j = 0; j < n; ++j) {
        if (!(state[j] & 2) || ids[j] != id) continue;
        ++count;
        const double qj = qual[j];
        ahead += qj > q || (qj == q && j < i);
      }
      if (count == target || save_partial) s = ahead;
    }
    track_id[d0 + i] = ids[i];
    slot[d0 + i] = s;
    saved += s >= 0;
  }
  completed = block_sum(completed, red_i);
  saved = block_sum(saved, red_i);
  if (t == 0) info[0] = next_id - 1, info[1] = completed, info[2] = saved, info[3] = 0;
}

hipError_t launch_capture_tracks(const int* bbox, const double* metrics, const unsigned char* valid,
                                 const int* frame_off, const int* clip_off, int n_clips, int max_disappeared,
                                 long long q_limit, int target_frames, double min_quality_score, int save_partial,
                                 int* track_id, double* quality, int* slot, int* clip_info, hipStream_t s) {
  if (n_clips <= 0) return hipSuccess;
  hipLaunchKernelGGL(capture_tracks_kernel, dim3(n_clips), dim3(CAP_BLOCK), 0, s, bbox, metrics, valid, frame_off,
                     clip_off, max_disappeared, q_limit, target_frames, min_quality_score, save_partial, track_id,
                     quality, slot, clip_info);
  return hipGetLastError();
}

}  // namespace frhip
