// Server sessions on gfx950: the recognition gating, the retry cooldown and the frame selection of
// the server's LiveRecognitionTracker (face_recognition_server.py:23-124) as process_faces and
// process_full_frame drive it (:368-413, :638-678), for every track of a recorded request log in one
// launch.  Track ids come from outside (the client's, or a fresh one per face), so tracks do not
// interact: the log is grouped by track (order + track_off, a CSR) and one wave owns one track.
//
//   steps      The appearances of a track are sequential; the state (attempts of the cycle, attempts
//              of the track, cooldown deadline, first appearance of the run) is the same in every
//              lane.  Per appearance j at the request's clock `now`:
//                in cooldown, now < deadline              SERVER_COOLDOWN
//                in cooldown, now >= deadline             SERVER_RESET: attempts = 0 and the ring is
//                                                         emptied, the face just appended included:
//                                                         the run starts at j + 1
//                attempts == max_attempts                 SERVER_COOLDOWN_SET: deadline = now +
//                                                         retry_cooldown (one double addition)
//                otherwise                                the best face of the window; an attempt iff
//                                                         that face's det_score > det_gate
//   window     The ring is never stored.  The window of j is the last min(j - run start + 1,
//              buffer_size) appearances.  Appearances are loaded 64 at a time, lane l holding
//              appearance c0 + l of this chunk and c0 - 64 + l of the one before, so with buffer_size
//              <= 64 the window of step c0 + r is the lanes l <= r of this chunk and the lanes l > r of
//              the last one: no LDS, no scratch, a track of any length.
//   selection  key = det_score * min(blur / 100, 1) in double, contraction off, as live.hip; a wave
//              argmax over (key, appearance) that prefers the larger key and then the older
//              appearance (Python's max over the deque keeps the first of equal keys).
//
// attempt[d] is the ordinal of the attempt among all attempts of the track, through cooldown cycles,
// as if none before it had succeeded; the host drops what follows a success.  A track with a
// non-finite metric or clock, or an order entry outside [0, n_dets), gets its error word, -1 / -1 /
// SERVER_GATED on its (in-range) detections and nothing else is touched.  Lane r keeps step r's
// result and the chunk is written by all lanes at once: vector stores only.
#include "frhip_kernels.h"

#pragma clang fp contract(off)

namespace frhip {

namespace {

constexpr int SERVER_BLOCK = 256;  // four waves: four tracks
static_assert(SERVER_MAX_BUFFER <= 64, "the window must fit the lanes of one wave");

// LiveRecognitionTracker.get_best_frame's quality_score (face_recognition_server.py:78-82)
__device__ __forceinline__ double server_key(double det, double blur_score) {
  const double blur = blur_score / 100.0;
  const double nb = 1.0 < blur ? 1.0 : blur;  // min(blur_score / 100.0, 1.0)
  return det * nb;
}

}  // namespace

__global__ __launch_bounds__(SERVER_BLOCK) void server_tracks_kernel(
    const double* __restrict__ metrics, const double* __restrict__ clock, const int* __restrict__ order,
    const int* __restrict__ track_off, int n_tracks, int n_dets, int max_attempts, int buffer_size,
    double retry_cooldown, double det_gate, int* __restrict__ attempt, int* __restrict__ best,
    int* __restrict__ state, int* __restrict__ track_info) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * (SERVER_BLOCK / 64) + (threadIdx.x >> 6);
  if (t >= n_tracks) return;  // the whole wave: no barrier anywhere below
  const int o0 = track_off[t];
  const int n = track_off[t + 1] - o0;
  int* info = track_info + (long long)t * 4;

  // ---- the values and the indices of the track
  int bad = 0;
  for (int i = lane; i < n; i += 64) {
    const int d = order[o0 + i];
    if ((unsigned)d >= (unsigned)n_dets) {
      bad |= SERVER_ERR_ORDER;
    } else {
      const double* m = metrics + (long long)d * 2;
      if (!(__builtin_isfinite(m[0]) && __builtin_isfinite(m[1]) && __builtin_isfinite(clock[d])))
        bad |= SERVER_ERR_VALUE;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) bad |= __shfl_xor(bad, off, 64);
  if (bad) {
    for (int i = lane; i < n; i += 64) {
      const int d = order[o0 + i];
      if ((unsigned)d < (unsigned)n_dets) attempt[d] = -1, best[d] = -1, state[d] = SERVER_GATED;
    }
    if (lane == 0) info[0] = 0, info[1] = 0, info[2] = 0, info[3] = bad;
    return;
  }

  // ---- the steps.  Everything but lane-indexed values is the same in all 64 lanes.
  int attempts = 0, made = 0, cooldowns = 0, resets = 0, run_start = 0;
  bool cooling = false;
  double deadline = 0.0;
  int d_old = -1;
  double key_old = 0.0, det_old = 0.0;
  for (int c0 = 0; c0 < n; c0 += 64) {
    const bool have = c0 + lane < n;
    const int d_cur = have ? order[o0 + c0 + lane] : -1;
    double clk = 0.0, key = 0.0, det = 0.0;
    if (have) {
      const double* m = metrics + (long long)d_cur * 2;
      det = m[0];
      key = server_key(det, m[1]);
      clk = clock[d_cur];
    }
    int my_attempt = -1, my_best = -1, my_state = SERVER_GATED;
    const int steps = n - c0 < 64 ? n - c0 : 64;
    for (int r = 0; r < steps; ++r) {
      const int j = c0 + r;
      const double now = __shfl(clk, r, 64);
      int st = SERVER_GATED, ordinal = -1, pick = -1;
      if (cooling) {
        if (now < deadline) {
          st = SERVER_COOLDOWN;
        } else {
          cooling = false, attempts = 0, run_start = j + 1, ++resets;
          st = SERVER_RESET;
        }
      } else if (attempts >= max_attempts) {
        deadline = now + retry_cooldown;
        cooling = true, ++cooldowns;
        st = SERVER_COOLDOWN_SET;
      } else {
        const int first = j - buffer_size + 1;
        const int lo = run_start > first ? run_start : first;  // <= j
        int at = lane <= r ? c0 + lane : c0 - 64 + lane;
        double k = lane <= r ? key : key_old;
        if (at < lo) k = -__builtin_huge_val(), at = 0x7fffffff;  // no finite key is that small
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const double k2 = __shfl_xor(k, off, 64);
          const int at2 = __shfl_xor(at, off, 64);
          if (k2 > k || (k2 == k && at2 < at)) k = k2, at = at2;  // the oldest of equal keys
        }
        const int from = at & 63;
        const int d_a = __shfl(d_cur, from, 64), d_b = __shfl(d_old, from, 64);
        const double det_a = __shfl(det, from, 64), det_b = __shfl(det_old, from, 64);
        const bool in_chunk = at >= c0;
        if ((in_chunk ? det_a : det_b) > det_gate) {
          st = SERVER_ATTEMPT;
          ordinal = made++, ++attempts;
          pick = in_chunk ? d_a : d_b;
        }
      }
      if (lane == r) my_attempt = ordinal, my_best = pick, my_state = st;
    }
    if (have) attempt[d_cur] = my_attempt, best[d_cur] = my_best, state[d_cur] = my_state;
    d_old = d_cur, key_old = key, det_old = det;
  }
  if (lane == 0) info[0] = made, info[1] = cooldowns, info[2] = resets, info[3] = 0;
}

hipError_t launch_server_tracks(const double* metrics, const double* clock, const int* order, const int* track_off,
                                int n_tracks, int n_dets, int max_attempts, int buffer_size, double retry_cooldown,
                                double det_gate, int* attempt, int* best, int* state, int* track_info,
                                hipStream_t s) {
  if (n_tracks <= 0) return hipSuccess;
  const long long per_block = SERVER_BLOCK / 64;
  hipLaunchKernelGGL(server_tracks_kernel, dim3((unsigned)((n_tracks + per_block - 1) / per_block)), dim3(SERVER_BLOCK), 0, s,
                     metrics, clock, order, track_off, n_tracks, n_dets, max_attempts, buffer_size, retry_cooldown,
                     det_gate, attempt, best, state, track_info);
  return hipGetLastError();
}

}  // namespace frhip
