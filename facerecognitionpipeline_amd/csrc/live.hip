// Live sessions on gfx950: LiveFaceRecognition._simple_track_assignment (face_recognition_live.py:
// 249-285) and the gating and frame selection of LiveRecognitionTracker (:18-80) as process_frame
// drives them (:339-355), for a batch of independent clips (cameras) in one launch.  One workgroup
// per clip, as capture.hip: a clip's frames are sequential, the faces of a frame are independent.
// A clip's detections are a CSR slice (frames of the clip, detections of each frame).
//
//   assignment   The live list is the previous frame's faces in that frame's detection order (the
//                reference's dict, replaced wholesale each frame), two copies in LDS that swap.  One
//                thread per face finds its nearest live track: q = (sx_t - sx_d)^2 + (sy_t - sy_d)^2
//                in int64 with sx = x1 + x2, sy = y1 + y2 (4 x the squared centroid distance), only
//                q < q_limit, equal q to the earlier list position (the reference's strict <).  A
//                track goes to the lowest-indexed face that chose it (an LDS atomicMin on the face
//                index); every other face opens the next id, in detection order, whatever else is in
//                range.  A track nobody chose is gone.  prev = the global index of the track's
//                detection in the previous frame.
//   gating       frame_count = index in the clip + 1.  On a frame with frame_count % interval == 0
//                a track that was present on a < max_attempts earlier such frames of its run gets
//                attempt = a.  The count travels with the list entry, saturated at max_attempts.
//   selection    After the frames, one thread per candidate walks its prev chain over the last
//                min(run length, buffer_size) detections: the largest key det_score *
//                min(blur / 100, 1) in double (contraction off), the oldest of equal keys (Python's
//                max over the deque).  The chain was written by this workgroup before a barrier.
//
// Everything but the key is integer arithmetic, so a clip's result depends on nothing but the clip.
// A clip with a coordinate beyond +-CAPTURE_COORD_MAX gets its error word set, track_id 0 and -1 in
// the other three arrays, and nothing is written out of range.
#include "block_reduce.h"
#include "frhip_kernels.h"

#pragma clang fp contract(off)

namespace frhip {

namespace {

constexpr int LIVE_BLOCK = 256;  // block_reduce.h's workgroup; the faces of a frame take threads 0..127
static_assert(LIVE_MAX_FACES <= LIVE_BLOCK, "one thread per face");
// |sx_t - sx_d| <= 4 * COORD_MAX, so q <= 2 * (4 * COORD_MAX)^2 = 2^45
static_assert(CAPTURE_COORD_MAX == (1 << 20), "q must stay below 2^63");

// LiveRecognitionTracker.get_best_frame's quality_score (face_recognition_live.py:59-63)
__device__ __forceinline__ double live_key(const double* m) {
  const double blur = m[1] / 100.0;
  const double nb = 1.0 < blur ? 1.0 : blur;  // min(blur_score / 100.0, 1.0)
  return m[0] * nb;
}

}  // namespace

// track_id, prev and attempt are read back in the selection pass by threads that did not write them:
// no __restrict__ on them
__global__ __launch_bounds__(LIVE_BLOCK) void live_tracks_kernel(
    const int* __restrict__ bbox, const double* __restrict__ metrics, const int* __restrict__ frame_off,
    const int* __restrict__ clip_off, long long q_limit, int interval, int max_attempts, int buffer_size,
    int* track_id, int* prev, int* attempt, int* __restrict__ best, int* __restrict__ clip_info) {
  // the live list (the previous frame's faces) and the one this frame builds
  __shared__ int l_id[2][LIVE_MAX_FACES], l_sx[2][LIVE_MAX_FACES], l_sy[2][LIVE_MAX_FACES];
  __shared__ int l_ticks[2][LIVE_MAX_FACES];  // tick frames of the track's run so far, <= max_attempts
  __shared__ int owner[LIVE_MAX_FACES];       // per live track: the lowest face index that chose it
  __shared__ unsigned char fresh_of[LIVE_MAX_FACES];
  __shared__ int red_i[4];

  const int c = blockIdx.x, t = threadIdx.x;
  const int f0 = clip_off[c], f1 = clip_off[c + 1];
  const int d0 = frame_off[f0];
  const int n = frame_off[f1] - d0;
  int* info = clip_info + (long long)c * 4;

  // ---- the coordinate range
  int bad = 0;
  for (int i = t; i < n; i += LIVE_BLOCK) {
    const long long at = d0 + i;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int v = bbox[at * 4 + k];
      bad |= v > CAPTURE_COORD_MAX || v < -CAPTURE_COORD_MAX;
    }
  }
  if (block_sum(bad, red_i) > 0) {
    for (int i = t; i < n; i += LIVE_BLOCK) {
      track_id[d0 + i] = 0;
      prev[d0 + i] = -1;
      attempt[d0 + i] = -1;
      best[d0 + i] = -1;
    }
    if (t == 0) info[0] = 0, info[1] = 0, info[2] = 0, info[3] = LIVE_ERR_COORD;
    return;
  }

  // ---- assignment and gating, frame by frame.  nt, next_id, cur and every branch around a barrier
  // are the same in all threads: they come from the offsets.
  int nt = 0, next_id = 0, cur = 0, prev_base = 0, candidates = 0;
  for (int f = f0; f < f1; ++f) {
    const int b = frame_off[f];
    const int nd = frame_off[f + 1] - b;  // 0..LIVE_MAX_FACES (checked by the host)
    const bool tick = (f - f0 + 1) % interval == 0;
    const int *p_id = l_id[cur], *p_sx = l_sx[cur], *p_sy = l_sy[cur], *p_ticks = l_ticks[cur];
    if (t < nt) owner[t] = LIVE_MAX_FACES;
    int choice = -1, sx = 0, sy = 0;
    if (t < nd) {
      const int* bb = bbox + (long long)(b + t) * 4;
      sx = bb[0] + bb[2];
      sy = bb[1] + bb[3];
      long long best_q = q_limit;
#pragma unroll 4
      for (int tp = 0; tp < nt; ++tp) {  // LDS words that are the same for every thread (broadcasts)
        const long long dx = (long long)p_sx[tp] - sx, dy = (long long)p_sy[tp] - sy;
        const long long q = dx * dx + dy * dy;
        if (q < best_q) best_q = q, choice = tp;
      }
    }
    __syncthreads();
    if (choice >= 0) atomicMin(&owner[choice], t);
    __syncthreads();
    const bool fresh = t < nd && (choice < 0 || owner[choice] != t);
    if (t < nd) fresh_of[t] = fresh;
    __syncthreads();
    int rank = 0, opened = 0;
#pragma unroll 4
    for (int j = 0; j < nd; ++j) {
      const int u = fresh_of[j];
      rank += j < t ? u : 0;
      opened += u;
    }
    if (t < nd) {
      const int id = fresh ? next_id + rank : p_id[choice];
      const int before = fresh ? 0 : p_ticks[choice];
      int a = -1, ticks = before;
      if (tick) {
        if (before < max_attempts) a = before, ticks = before + 1;
        candidates += a >= 0;
      }
      const int o = cur ^ 1;
      l_id[o][t] = id, l_sx[o][t] = sx, l_sy[o][t] = sy, l_ticks[o][t] = ticks;
      track_id[b + t] = id;
      prev[b + t] = fresh ? -1 : prev_base + choice;
      attempt[b + t] = a;
    }
    next_id += opened;
    nt = nd;
    prev_base = b;
    cur ^= 1;
    __syncthreads();  // the new list is complete; owner and fresh_of are free again
  }

  // ---- selection: the best of the ring of every candidate
  __syncthreads();
  for (int i = t; i < n; i += LIVE_BLOCK) {
    const int at = d0 + i;
    int pick = -1;
    if (attempt[at] >= 0) {
      pick = at;
      double key = live_key(metrics + (long long)at * 2);
      int at2 = at;
      for (int s = 1; s < buffer_size; ++s) {
        at2 = prev[at2];
        if (at2 < 0) break;
        const double k2 = live_key(metrics + (long long)at2 * 2);
        if (k2 >= key) key = k2, pick = at2;  // older and not smaller: the oldest of equal keys wins
      }
    }
    best[at] = pick;
  }
  candidates = block_sum(candidates, red_i);
  if (t == 0) info[0] = next_id, info[1] = candidates, info[2] = f1 - f0, info[3] = 0;
}

hipError_t launch_live_tracks(const int* bbox, const double* metrics, const int* frame_off, const int* clip_off,
                              int n_clips, long long q_limit, int recognition_interval, int max_attempts,
                              int buffer_size, int* track_id, int* prev, int* attempt, int* best, int* clip_info,
                              hipStream_t s) {
  if (n_clips <= 0) return hipSuccess;
  hipLaunchKernelGGL(live_tracks_kernel, dim3(n_clips), dim3(LIVE_BLOCK), 0, s, bbox, metrics, frame_off, clip_off,
                     q_limit, recognition_interval, max_attempts, buffer_size, track_id, prev, attempt, best, clip_info);
  return hipGetLastError();
}

}  // namespace frhip
