// libfrhip public C API (include/frhip.h), the calls over CSR batches: fr_build_templates,
// fr_track_consensus, fr_photo_rollcall, fr_capture_tracks, fr_live_tracks, fr_server_tracks, fr_identity_scores and
// fr_eval_probes.
// They share one shape: lock_handle; the argument checks, which need no handle and so report the
// same way for h == NULL (csr_check for the offsets); "NULL handle"; the offsets staged with
// stage_int32; the launch; one stream synchronise, because the staging read pageable host memory.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "runtime.h"

using namespace frhip;
using namespace frhip_rt;

namespace frhip_rt {

long long capture_q_limit(double max_distance) {
  if (!(max_distance > 0.0)) return 0;  // also NaN: `distances.min() < nan` is never true
  // past every q in range (q <= 2^45: coordinates within +-FR_CAPTURE_COORD_MAX)
  if (max_distance >= 4194304.0) return 1ll << 46;
  long long q = (long long)std::floor(4.0 * max_distance * max_distance);
  while (q > 0 && std::sqrt((double)(q - 1) / 4.0) >= max_distance) --q;
  while (std::sqrt((double)q / 4.0) < max_distance) ++q;
  return q;
}

int g_eval_chunk = 0;
int g_identify_path = 0;
int g_identify_tile_rows = IDENT_TILE_ROWS;

// Tiles of the aggregation kernels: runs of whole identities of <= max_ids identities and <= max_rows
// rows, an identity longer than max_rows alone; n_tiles + 1 boundaries (first identities, then n_ids).
static std::vector<int32_t> cut_tiles(const int32_t* id_offsets, int n_ids, int max_ids, int max_rows) {
  std::vector<int32_t> tiles;
  for (int i = 0, first = 0; i <= n_ids; ++i) {
    if (i == n_ids || (i > first && (i - first == max_ids || id_offsets[i + 1] - id_offsets[first] > max_rows))) {
      tiles.push_back(first);
      first = i;
    }
  }
  tiles.push_back(n_ids);
  return tiles;
}

// Probes per chunk of a score GEMM against G rows: score matrices below 2 GiB (the conv epilogue's
// 32-bit offsets), or frt_set_eval_chunk's fewer.
static int score_chunk(int n, int G) {
  int nc = (int)std::max<long long>(1, std::min<long long>(n, ((1ll << 31) - 1) / ((long long)G * 4)));
  if (g_eval_chunk > 0) nc = std::min(nc, g_eval_chunk);
  return nc;
}

int match_identities_device(fr_handle* h, const float* Q, int n, int aggregation, int agg_k, int k, int32_t* idx,
                            float* score, hipStream_t s) {
  if (aggregation < FR_AGG_MAX || aggregation > FR_AGG_TOPK)
    return fail(h, FR_ERR_INVALID_ARGUMENT, "aggregation must be FR_AGG_MAX, _MEAN or _TOPK");
  if (aggregation == FR_AGG_TOPK && agg_k < 1) return fail(h, FR_ERR_INVALID_ARGUMENT, "agg_k must be >= 1");
  if (aggregation == FR_AGG_TOPK && agg_k > EVAL_MAX_K)
    return fail(h, FR_ERR_UNSUPPORTED, "top-k aggregation takes agg_k <= " + std::to_string(EVAL_MAX_K));
  const int n_ids = h->sample_ids, G = h->sample_rows;
  if (n_ids <= 0) return fail(h, FR_ERR_STATE, "sample gallery is empty (fr_samples_set first)");
  if (k < 1 || k > n_ids) return fail(h, FR_ERR_INVALID_ARGUMENT, "k must be in [1, n_ids]");
  if (n <= 0) return FR_OK;
  // the fused kernel reads the gallery once per query: one query, or a few against a small gallery
  const bool small = n == 1 || (n <= IDENT_SMALL_N && (long long)n * G <= IDENT_QUERY_ROWS);
  const bool fused = g_identify_path == 0 ? small : g_identify_path == 1;
  const int nc = fused ? n : score_chunk(n, G);
  // [query norms: n][identity scores: nc x n_ids]
  const size_t norm_floats = ((size_t)n + 3) & ~(size_t)3;
  int rc = ensure_buf(h, &h->ident_ws, &h->ident_ws_cap, (norm_floats + (size_t)nc * n_ids) * sizeof(float));
  if (rc) return rc;
  float* d_qnorm = (float*)h->ident_ws;
  float* d_out = d_qnorm + norm_floats;
  if (fused) {
    ProfScope ps(h, s, 0.0, 0);
    hipError_t e = launch_match_small(Q, n, h->samples, h->d_sample_norm, h->d_sample_flag, h->d_sample_off, n_ids,
                                      h->d_sample_tiles, h->sample_tiles, aggregation, agg_k, d_out, s);
    if (e == hipSuccess) e = launch_topk(d_out, n, n_ids, k, idx, score, s, true);
    if (e != hipSuccess) return launch_fail(h, "identity match", e);
    return FR_OK;
  }
  // composed: the score GEMM into the scores workspace, fr_identity_scores' aggregation on the
  // stored offsets, tiles and norms, then the top-k, a chunk of queries at a time
  LaneWs& L = h->lane_ws[0];
  if (ensure_stream_k(h->device, &h->cus, &L.sk_ws, &L.sk_ws_floats, &L.sk_cnt, &L.sk_cnt_cap) != FR_OK)
    return fail(h, FR_ERR_HIP, "stream-K workspace allocation failed");
  rc = ensure_buf(h, (void**)&h->scores, &h->scores_cap, (size_t)nc * G * sizeof(float));
  if (rc) return rc;
  {
    ProfScope ps(h, s, 0.0, 0);
    const hipError_t e = launch_row_norms(Q, n, d_qnorm, nullptr, s);
    if (e != hipSuccess) return launch_fail(h, "row norms", e);
  }
  ConvW g;
  g.w = h->samples;
  g.geometry(512, G, 1, 1, 1, 0);
  for (int q0 = 0; q0 < n; q0 += nc) {
    const int qn = std::min(nc, n - q0);
    // raw dots: no renormalisation of either side (the notebook's np.dot)
    rc = run_conv(h, g, ConvCall{Q + (size_t)q0 * 512, h->scores, qn, 1, 1, EPI_RAW}, L, s);
    if (rc) return rc;
    ProfScope ps(h, s, 0.0, 0);
    hipError_t e = launch_identity_agg(h->scores, qn, G, h->d_sample_off, n_ids, h->d_sample_eval_tiles,
                                       h->sample_eval_tiles, d_qnorm + q0, h->d_sample_norm, h->d_sample_flag,
                                       aggregation, agg_k, false, d_out, s);
    if (e == hipSuccess) e = launch_topk(d_out, qn, n_ids, k, idx + (size_t)q0 * k, score + (size_t)q0 * k, s, true);
    if (e != hipSuccess) return launch_fail(h, "identity match", e);
  }
  return FR_OK;
}

}  // namespace frhip_rt

extern "C" {

int fr_build_templates(fr_handle* h, const float* emb, const int32_t* offsets, int n_students, int method,
                       float min_similarity, float* templates, int32_t* kept, void* stream) {
  auto lk = lock_handle(h);
  if (n_students < 0 || (n_students > 0 && (!emb || !offsets || !templates)))
    return fail(h, FR_ERR_INVALID_ARGUMENT, "bad n_students or NULL buffer");
  if (method < FR_TEMPLATE_MEAN || method > FR_TEMPLATE_WEIGHTED_MEAN)
    return fail(h, FR_ERR_INVALID_ARGUMENT, "method must be FR_TEMPLATE_MEAN, _MEDIAN or _WEIGHTED_MEAN");
  const std::string bad = csr_check(offsets, n_students, 1, TEMPLATE_MAX_SAMPLES, {"offsets", "student", "samples"});
  if (!bad.empty()) return fail(h, FR_ERR_INVALID_ARGUMENT, bad);
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  if (n_students == 0) return FR_OK;
  DeviceGuard dg(h->device);
  hipStream_t s = (hipStream_t)stream;
  const int* d_off;
  if (int rc = stage_int32(h, s, {{offsets, (size_t)n_students + 1}}, &d_off)) return rc;
  const hipError_t e = launch_templates(emb, d_off, n_students, method, min_similarity, templates, kept, s);
  if (e != hipSuccess) return launch_fail(h, "template", e);
  FR_HIP(h, hipStreamSynchronize(s));  // the offsets were staged from pageable host memory
  return FR_OK;
}

int fr_track_consensus(fr_handle* h, const int32_t* idx, const float* score, int k, const int32_t* offsets,
                       int n_tracks, double min_quality, int min_frames, double similarity_threshold,
                       int32_t* out_i, double* out_d, void* stream) {
  auto lk = lock_handle(h);
  if (n_tracks < 0 || (n_tracks > 0 && (!idx || !score || !offsets || !out_i || !out_d)))
    return fail(h, FR_ERR_INVALID_ARGUMENT, "bad n_tracks or NULL buffer");
  if (k < 1) return fail(h, FR_ERR_INVALID_ARGUMENT, "k must be >= 1");
  if (min_frames < 1) return fail(h, FR_ERR_INVALID_ARGUMENT, "min_frames must be >= 1");
  const std::string bad = csr_check(offsets, n_tracks, 1, TRACK_MAX_FRAMES, {"offsets", "track", "frames"});
  if (!bad.empty()) return fail(h, FR_ERR_INVALID_ARGUMENT, bad);
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  if (n_tracks == 0) return FR_OK;
  DeviceGuard dg(h->device);
  hipStream_t s = (hipStream_t)stream;
  const int* d_off;
  if (int rc = stage_int32(h, s, {{offsets, (size_t)n_tracks + 1}}, &d_off)) return rc;
  const hipError_t e = launch_track_consensus(idx, score, k, d_off, n_tracks, min_quality, min_frames,
                                              similarity_threshold, out_i, out_d, s);
  if (e != hipSuccess) return launch_fail(h, "track consensus", e);
  FR_HIP(h, hipStreamSynchronize(s));  // the offsets were staged from pageable host memory
  return FR_OK;
}

int fr_photo_rollcall(fr_handle* h, const int32_t* idx, const float* score, int k, const int32_t* offsets,
                      int n_images, double similarity_threshold, int mode, int32_t* out_face, float* out_score,
                      int32_t* out_image, void* stream) {
  auto lk = lock_handle(h);
  if (n_images < 0 || (n_images > 0 && (!offsets || !out_image)))
    return fail(h, FR_ERR_INVALID_ARGUMENT, "bad n_images or NULL buffer");
  if (k < 1) return fail(h, FR_ERR_INVALID_ARGUMENT, "k must be >= 1");
  if (mode != FR_ROLLCALL_INDEPENDENT && mode != FR_ROLLCALL_EXCLUSIVE)
    return fail(h, FR_ERR_INVALID_ARGUMENT, "mode must be FR_ROLLCALL_INDEPENDENT or _EXCLUSIVE");
  // photographs of any number of faces up to the cap, also none
  const std::string bad = csr_check(offsets, n_images, 0, ROLLCALL_MAX_FACES, {"offsets", "photograph", "faces"});
  if (!bad.empty()) return fail(h, FR_ERR_INVALID_ARGUMENT, bad);
  if (n_images > 0 && offsets[n_images] > 0 && (!idx || !score || !out_face || !out_score))
    return fail(h, FR_ERR_INVALID_ARGUMENT, "NULL buffer");
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  if (n_images == 0) return FR_OK;
  DeviceGuard dg(h->device);
  hipStream_t s = (hipStream_t)stream;
  const int* d_off;
  if (int rc = stage_int32(h, s, {{offsets, (size_t)n_images + 1}}, &d_off)) return rc;
  const hipError_t e = launch_photo_rollcall(idx, score, k, d_off, n_images, similarity_threshold, mode, out_face,
                                             out_score, out_image, s);
  if (e != hipSuccess) return launch_fail(h, "photo rollcall", e);
  FR_HIP(h, hipStreamSynchronize(s));  // the offsets were staged from pageable host memory
  return FR_OK;
}

int fr_capture_tracks(fr_handle* h, const int32_t* bbox, const double* metrics, const uint8_t* valid,
                      const int32_t* frame_offsets, const int32_t* clip_offsets, int n_clips, int max_disappeared,
                      double max_distance, int target_frames, double min_quality_score, int save_partial,
                      int32_t* track_id, double* quality, int32_t* slot, int32_t* clip_info, void* stream) {
  auto lk = lock_handle(h);
  if (n_clips < 0) return fail(h, FR_ERR_INVALID_ARGUMENT, "n_clips must be >= 0");
  if (target_frames < 1 || target_frames > CAPTURE_MAX_TARGET)
    return fail(h, FR_ERR_INVALID_ARGUMENT, "target_frames must be in [1, " + std::to_string(CAPTURE_MAX_TARGET) + "]");
  if (max_disappeared < 0) return fail(h, FR_ERR_INVALID_ARGUMENT, "max_disappeared must be >= 0");
  int n_frames = 0;
  if (n_clips > 0) {
    if (!frame_offsets || !clip_offsets) return fail(h, FR_ERR_INVALID_ARGUMENT, "NULL buffer (offsets)");
    // clips of any number of frames; frames may be empty; a cap per frame and one per clip
    std::string bad = csr_check(clip_offsets, n_clips, 0, INT32_MAX, {"clip_offsets", "clip", "frames"});
    n_frames = bad.empty() ? clip_offsets[n_clips] : 0;
    if (bad.empty())
      bad = csr_check(frame_offsets, n_frames, 0, CAPTURE_MAX_FACES, {"frame_offsets", "frame", "detections"});
    // (csr_check reads nothing of an array of no slices, but clips without frames still have a total)
    if (bad.empty() && n_frames == 0 && frame_offsets[0] != 0) bad = "frame_offsets[0] must be 0";
    if (bad.empty())
      bad = csr_check(frame_offsets, n_clips, 0, CAPTURE_MAX_DETS, {"frame_offsets", "clip", "detections"},
                      clip_offsets);
    if (!bad.empty()) return fail(h, FR_ERR_INVALID_ARGUMENT, bad);
    const int total = frame_offsets[n_frames];
    if (!clip_info || (total > 0 && (!bbox || !metrics || !valid || !track_id || !quality || !slot)))
      return fail(h, FR_ERR_INVALID_ARGUMENT, "NULL buffer");
  }
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  if (n_clips == 0) return FR_OK;
  DeviceGuard dg(h->device);
  hipStream_t s = (hipStream_t)stream;
  const int* d_off[2];  // frame offsets, then clip offsets
  if (int rc = stage_int32(h, s, {{frame_offsets, (size_t)n_frames + 1}, {clip_offsets, (size_t)n_clips + 1}}, d_off))
    return rc;
  const hipError_t e = launch_capture_tracks(bbox, metrics, valid, d_off[0], d_off[1], n_clips, max_disappeared,
                                             capture_q_limit(max_distance), target_frames, min_quality_score,
                                             save_partial != 0, track_id, quality, slot, clip_info, s);
  if (e != hipSuccess) return launch_fail(h, "capture tracks", e);
  std::vector<int32_t> info((size_t)n_clips * 4);
  FR_HIP(h, hipMemcpyAsync(info.data(), clip_info, info.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  FR_HIP(h, hipStreamSynchronize(s));  // the offsets were staged from pageable host memory
  for (int c = 0; c < n_clips; ++c) {
    const int err = info[(size_t)c * 4 + 3];
    if (err)
      return fail(h, FR_ERR_UNSUPPORTED,
                  "clip " + std::to_string(c) +
                      (err == CAPTURE_ERR_TRACKS
                           ? ": more than " + std::to_string(CAPTURE_MAX_TRACKS) + " tracks alive at once"
                           : ": a box coordinate beyond +-" + std::to_string(CAPTURE_COORD_MAX)));
  }
  return FR_OK;
}

int fr_live_tracks(fr_handle* h, const int32_t* bbox, const double* metrics, const int32_t* frame_offsets,
                   const int32_t* clip_offsets, int n_clips, double max_distance, int recognition_interval,
                   int max_attempts, int buffer_size, int32_t* track_id, int32_t* prev, int32_t* attempt,
                   int32_t* best, int32_t* clip_info, void* stream) {
  auto lk = lock_handle(h);
  if (n_clips < 0) return fail(h, FR_ERR_INVALID_ARGUMENT, "n_clips must be >= 0");
  if (recognition_interval < 1) return fail(h, FR_ERR_INVALID_ARGUMENT, "recognition_interval must be >= 1");
  if (max_attempts < 1 || max_attempts > LIVE_MAX_ATTEMPTS)
    return fail(h, FR_ERR_INVALID_ARGUMENT, "max_attempts must be in [1, " + std::to_string(LIVE_MAX_ATTEMPTS) + "]");
  if (buffer_size < 1 || buffer_size > LIVE_MAX_BUFFER)
    return fail(h, FR_ERR_INVALID_ARGUMENT, "buffer_size must be in [1, " + std::to_string(LIVE_MAX_BUFFER) + "]");
  int n_frames = 0;
  if (n_clips > 0) {
    if (!frame_offsets || !clip_offsets) return fail(h, FR_ERR_INVALID_ARGUMENT, "NULL buffer (offsets)");
    // clips of any number of frames and detections; frames may be empty; a cap per frame
    std::string bad = csr_check(clip_offsets, n_clips, 0, INT32_MAX, {"clip_offsets", "clip", "frames"});
    n_frames = bad.empty() ? clip_offsets[n_clips] : 0;
    if (bad.empty())
      bad = csr_check(frame_offsets, n_frames, 0, LIVE_MAX_FACES, {"frame_offsets", "frame", "detections"});
    // (csr_check reads nothing of an array of no slices, but clips without frames still have a total)
    if (bad.empty() && n_frames == 0 && frame_offsets[0] != 0) bad = "frame_offsets[0] must be 0";
    if (!bad.empty()) return fail(h, FR_ERR_INVALID_ARGUMENT, bad);
    const int total = frame_offsets[n_frames];
    if (!clip_info || (total > 0 && (!bbox || !metrics || !track_id || !prev || !attempt || !best)))
      return fail(h, FR_ERR_INVALID_ARGUMENT, "NULL buffer");
  }
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  if (n_clips == 0) return FR_OK;
  DeviceGuard dg(h->device);
  hipStream_t s = (hipStream_t)stream;
  const int* d_off[2];  // frame offsets, then clip offsets
  if (int rc = stage_int32(h, s, {{frame_offsets, (size_t)n_frames + 1}, {clip_offsets, (size_t)n_clips + 1}}, d_off))
    return rc;
  const hipError_t e =
      launch_live_tracks(bbox, metrics, d_off[0], d_off[1], n_clips, capture_q_limit(max_distance),
                         recognition_interval, max_attempts, buffer_size, track_id, prev, attempt, best, clip_info, s);
  if (e != hipSuccess) return launch_fail(h, "live tracks", e);
  std::vector<int32_t> info((size_t)n_clips * 4);
  FR_HIP(h, hipMemcpyAsync(info.data(), clip_info, info.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  FR_HIP(h, hipStreamSynchronize(s));  // the offsets were staged from pageable host memory
  for (int c = 0; c < n_clips; ++c)
    if (info[(size_t)c * 4 + 3])
      return fail(h, FR_ERR_UNSUPPORTED,
                  "clip " + std::to_string(c) + ": a box coordinate beyond +-" + std::to_string(CAPTURE_COORD_MAX));
  return FR_OK;
}

int fr_server_tracks(fr_handle* h, const double* metrics, const double* clock, const int32_t* order,
                     const int32_t* track_offsets, int n_tracks, int n_dets, int max_attempts, int buffer_size,
                     double retry_cooldown, double det_gate, int32_t* attempt, int32_t* best, int32_t* state,
                     int32_t* track_info, void* stream) {
  auto lk = lock_handle(h);
  if (n_tracks < 0 || n_dets < 0) return fail(h, FR_ERR_INVALID_ARGUMENT, "n_tracks and n_dets must be >= 0");
  if (max_attempts < 1 || max_attempts > SERVER_MAX_ATTEMPTS)
    return fail(h, FR_ERR_INVALID_ARGUMENT, "max_attempts must be in [1, " + std::to_string(SERVER_MAX_ATTEMPTS) + "]");
  if (buffer_size < 1 || buffer_size > SERVER_MAX_BUFFER)
    return fail(h, FR_ERR_INVALID_ARGUMENT, "buffer_size must be in [1, " + std::to_string(SERVER_MAX_BUFFER) + "]");
  if (!std::isfinite(retry_cooldown) || retry_cooldown < 0.0)
    return fail(h, FR_ERR_INVALID_ARGUMENT, "retry_cooldown must be finite and >= 0");
  if (!std::isfinite(det_gate)) return fail(h, FR_ERR_INVALID_ARGUMENT, "det_gate must be finite");
  if (n_tracks > 0) {
    if (!track_offsets) return fail(h, FR_ERR_INVALID_ARGUMENT, "NULL buffer (offsets)");
    // tracks of any number of appearances, also none
    const std::string bad = csr_check(track_offsets, n_tracks, 0, INT32_MAX, {"track_offsets", "track", "appearances"});
    if (!bad.empty()) return fail(h, FR_ERR_INVALID_ARGUMENT, bad);
    const int total = track_offsets[n_tracks];
    if (!track_info || (total > 0 && (!metrics || !clock || !order || !attempt || !best || !state)))
      return fail(h, FR_ERR_INVALID_ARGUMENT, "NULL buffer");
  }
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  if (n_tracks == 0) return FR_OK;
  DeviceGuard dg(h->device);
  hipStream_t s = (hipStream_t)stream;
  const int* d_off;
  if (int rc = stage_int32(h, s, {{track_offsets, (size_t)n_tracks + 1}}, &d_off)) return rc;
  const hipError_t e = launch_server_tracks(metrics, clock, order, d_off, n_tracks, n_dets, max_attempts, buffer_size,
                                            retry_cooldown, det_gate, attempt, best, state, track_info, s);
  if (e != hipSuccess) return launch_fail(h, "server tracks", e);
  std::vector<int32_t> info((size_t)n_tracks * 4);
  FR_HIP(h, hipMemcpyAsync(info.data(), track_info, info.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  FR_HIP(h, hipStreamSynchronize(s));  // the offsets were staged from pageable host memory
  for (int t = 0; t < n_tracks; ++t) {
    const int err = info[(size_t)t * 4 + 3];
    if (err)
      return fail(h, FR_ERR_UNSUPPORTED,
                  "track " + std::to_string(t) +
                      (err & SERVER_ERR_ORDER ? ": an order entry outside [0, " + std::to_string(n_dets) + ")"
                                              : ": a non-finite metric or clock"));
  }
  return FR_OK;
}

int fr_identity_scores(fr_handle* h, const float* Q, int n, const float* E, const int32_t* id_offsets, int n_ids,
                       int aggregation, int k, float* out, float* sim, void* stream) {
  auto lk = lock_handle(h);
  if (n < 0 || n_ids < 1 || !id_offsets || !E || (n > 0 && (!Q || !out)))
    return fail(h, FR_ERR_INVALID_ARGUMENT, "bad n or n_ids, or NULL buffer");
  if (aggregation < FR_AGG_MAX || aggregation > FR_AGG_TOPK)
    return fail(h, FR_ERR_INVALID_ARGUMENT, "aggregation must be FR_AGG_MAX, _MEAN or _TOPK");
  if (aggregation == FR_AGG_TOPK && k < 1) return fail(h, FR_ERR_INVALID_ARGUMENT, "k must be >= 1");
  if (aggregation == FR_AGG_TOPK && k > EVAL_MAX_K)
    return fail(h, FR_ERR_UNSUPPORTED, "top-k aggregation takes k <= " + std::to_string(EVAL_MAX_K));
  const std::string bad = csr_check(id_offsets, n_ids, 1, EVAL_MAX_ROWS, {"id_offsets", "identity", "gallery rows"});
  if (!bad.empty()) return fail(h, FR_ERR_INVALID_ARGUMENT, bad);
  const int G = id_offsets[n_ids];
  if ((long long)G * 4 > (1ll << 31) - 1) return fail(h, FR_ERR_UNSUPPORTED, "one probe's score row must stay below 2 GiB");
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  if (n == 0) return FR_OK;
  if (int rc = check_dev_err(h)) return rc;  // reported by earlier asynchronous work
  DeviceGuard dg(h->device);
  hipStream_t s = (hipStream_t)stream;
  // tiles of the aggregation kernel: runs of identities of <= EVAL_TILE_IDS identities and
  // <= EVAL_TILE_ROWS rows (n_tiles + 1 boundaries), staged behind the offsets
  const std::vector<int32_t> tiles = cut_tiles(id_offsets, n_ids, EVAL_TILE_IDS, EVAL_TILE_ROWS);
  const int n_tiles = (int)tiles.size() - 1;
  const int* d_stage[2];  // offsets, then tiles
  int rc = stage_int32(h, s, {{id_offsets, (size_t)n_ids + 1}, {tiles.data(), tiles.size()}}, d_stage);
  if (rc) return rc;
  const int *d_off = d_stage[0], *d_tiles = d_stage[1];
  // row norms: [flag][n probes][G gallery rows]
  rc = ensure_buf(h, &h->eval_ws, &h->eval_ws_cap, (1 + (size_t)n + (size_t)G) * sizeof(float));
  if (rc) return rc;
  int* d_flag = (int*)h->eval_ws;
  float* d_qnorm = (float*)h->eval_ws + 1;
  float* d_enorm = d_qnorm + n;
  LaneWs& L = h->lane_ws[0];
  if (ensure_stream_k(h->device, &h->cus, &L.sk_ws, &L.sk_ws_floats, &L.sk_cnt, &L.sk_cnt_cap) != FR_OK)
    return fail(h, FR_ERR_HIP, "stream-K workspace allocation failed");
  FR_HIP(h, hipMemsetAsync(d_flag, 0, sizeof(int), s));
  {
    ProfScope ps(h, s, 0.0, 0);
    hipError_t e = launch_row_norms(Q, n, d_qnorm, nullptr, s);
    if (e == hipSuccess) e = launch_row_norms(E, G, d_enorm, d_flag, s);
    if (e != hipSuccess) return launch_fail(h, "row norms", e);
  }
  ConvW g;
  g.w = const_cast<float*>(E);
  g.geometry(512, G, 1, 1, 1, 0);
  // score matrices below 2 GiB (the conv epilogue's 32-bit offsets): probes in chunks
  const int nc = score_chunk(n, G);
  if (!sim) {
    rc = ensure_buf(h, (void**)&h->scores, &h->scores_cap, (size_t)nc * G * sizeof(float));
    if (rc) return rc;
  }
  for (int q0 = 0; q0 < n; q0 += nc) {
    const int qn = std::min(nc, n - q0);
    float* chunk = sim ? sim + (size_t)q0 * G : h->scores;
    // raw dots: no renormalisation of either side (the notebook's np.dot)
    rc = run_conv(h, g, ConvCall{Q + (size_t)q0 * 512, chunk, qn, 1, 1, EPI_RAW}, L, s);
    if (rc) return rc;
    ProfScope ps(h, s, 0.0, 0);
    const hipError_t e = launch_identity_agg(chunk, qn, G, d_off, n_ids, d_tiles, n_tiles, d_qnorm + q0, d_enorm,
                                             d_flag, aggregation, k, sim != nullptr, out + (size_t)q0 * n_ids, s);
    if (e != hipSuccess) return launch_fail(h, "identity scores", e);
  }
  FR_HIP(h, hipStreamSynchronize(s));  // the offsets were staged from pageable host memory
  return check_dev_err(h);
}

int fr_eval_probes(fr_handle* h, const float* scores, int n, int n_ids, const int32_t* true_id,
                   const double* thresholds, int n_thr, int32_t* rec_i, float* rec_f, int64_t* counts, void* stream) {
  auto lk = lock_handle(h);
  if (n < 0 || n_ids < 1) return fail(h, FR_ERR_INVALID_ARGUMENT, "n must be >= 0 and n_ids >= 1");
  if (n_thr < 0 || n_thr > EVAL_MAX_THRESHOLDS)
    return fail(h, FR_ERR_INVALID_ARGUMENT, "n_thr must be in [0, " + std::to_string(EVAL_MAX_THRESHOLDS) + "]");
  if ((n > 0 && (!scores || !true_id || !rec_i || !rec_f)) || (n_thr > 0 && (!thresholds || !counts)))
    return fail(h, FR_ERR_INVALID_ARGUMENT, "NULL buffer");
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  DeviceGuard dg(h->device);
  hipStream_t s = (hipStream_t)stream;
  if (n_thr > 0) FR_HIP(h, hipMemsetAsync(counts, 0, (size_t)n_thr * 4 * sizeof(int64_t), s));
  if (n > 0) {
    // no offsets here: what this call stages is its thresholds (doubles, into eval_ws)
    int rc = ensure_buf(h, &h->eval_ws, &h->eval_ws_cap, EVAL_MAX_THRESHOLDS * sizeof(double));
    if (rc) return rc;
    if (n_thr > 0)
      FR_HIP(h, hipMemcpyAsync(h->eval_ws, thresholds, (size_t)n_thr * sizeof(double), hipMemcpyHostToDevice, s));
    ProfScope ps(h, s, 0.0, 0);
    const hipError_t e = launch_eval_probes(scores, n, n_ids, true_id, (const double*)h->eval_ws, n_thr, rec_i, rec_f,
                                            (long long*)counts, s);
    if (e != hipSuccess) return launch_fail(h, "eval probes", e);
  }
  FR_HIP(h, hipStreamSynchronize(s));  // the thresholds were staged from pageable host memory
  return FR_OK;
}

int fr_samples_set(fr_handle* h, const float* E, const int32_t* id_offsets, int n_ids, int src_is_device,
                   void* stream) {
  auto lk = lock_handle(h);
  if (n_ids < 0 || (n_ids > 0 && (!E || !id_offsets)))
    return fail(h, FR_ERR_INVALID_ARGUMENT, "bad n_ids or NULL buffer");
  const std::string bad = csr_check(id_offsets, n_ids, 1, EVAL_MAX_ROWS, {"id_offsets", "identity", "gallery rows"});
  if (!bad.empty()) return fail(h, FR_ERR_INVALID_ARGUMENT, bad);
  const int G = n_ids > 0 ? id_offsets[n_ids] : 0;
  if ((long long)G * 4 > (1ll << 31) - 1) return fail(h, FR_ERR_UNSUPPORTED, "one query's score row must stay below 2 GiB");
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  h->sample_ids = h->sample_rows = h->sample_tiles = h->sample_eval_tiles = 0;  // cleared until the new one is whole
  if (n_ids == 0) return FR_OK;
  DeviceGuard dg(h->device);
  hipStream_t s = (hipStream_t)stream;
  const std::vector<int32_t> serve = cut_tiles(id_offsets, n_ids, INT32_MAX, g_identify_tile_rows);
  const std::vector<int32_t> eval = cut_tiles(id_offsets, n_ids, EVAL_TILE_IDS, EVAL_TILE_ROWS);
  // [flag][norms: G][offsets: n_ids + 1][serving tiles][evaluation tiles]
  std::vector<int32_t> ints(id_offsets, id_offsets + n_ids + 1);
  ints.insert(ints.end(), serve.begin(), serve.end());
  ints.insert(ints.end(), eval.begin(), eval.end());
  void* p = h->samples;
  int rc = ensure_buf(h, &p, &h->samples_cap, (size_t)G * 512 * sizeof(float));
  h->samples = (float*)p;
  if (rc) return rc;
  rc = ensure_buf(h, &h->sample_meta, &h->sample_meta_cap, (1 + (size_t)G + ints.size()) * sizeof(int32_t));
  if (rc) return rc;
  h->d_sample_flag = (int*)h->sample_meta;
  h->d_sample_norm = (float*)h->sample_meta + 1;
  h->d_sample_off = (int*)h->sample_meta + 1 + G;
  h->d_sample_tiles = h->d_sample_off + n_ids + 1;
  h->d_sample_eval_tiles = h->d_sample_tiles + serve.size();
  FR_HIP(h, hipMemcpyAsync(h->samples, E, (size_t)G * 512 * sizeof(float),
                           src_is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
  FR_HIP(h, hipMemcpyAsync(h->d_sample_off, ints.data(), ints.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  FR_HIP(h, hipMemsetAsync(h->d_sample_flag, 0, sizeof(int), s));
  {
    ProfScope ps(h, s, 0.0, 0);
    const hipError_t e = launch_row_norms(h->samples, G, h->d_sample_norm, h->d_sample_flag, s);
    if (e != hipSuccess) return launch_fail(h, "row norms", e);
  }
  FR_HIP(h, hipStreamSynchronize(s));  // the offsets and tiles were staged from pageable host memory
  h->sample_ids = n_ids;
  h->sample_rows = G;
  h->sample_tiles = (int)serve.size() - 1;
  h->sample_eval_tiles = (int)eval.size() - 1;
  return FR_OK;
}

int fr_samples_size(fr_handle* h, int* n_ids, int* rows) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (n_ids) *n_ids = h->sample_ids;
  if (rows) *rows = h->sample_rows;
  return FR_OK;
}

int fr_match_identities(fr_handle* h, const float* Q, int n, int aggregation, int agg_k, int k, int32_t* idx,
                        float* score, void* stream) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (n < 0 || (n > 0 && (!Q || !idx || !score))) return fail(h, FR_ERR_INVALID_ARGUMENT, "bad n or NULL buffer");
  if (int rc = check_dev_err(h)) return rc;  // reported by earlier asynchronous work
  DeviceGuard dg(h->device);
  return match_identities_device(h, Q, n, aggregation, agg_k, k, idx, score, (hipStream_t)stream);
}

int fr_embed_match_identities(fr_handle* h, const uint8_t* rgb, int n, int aggregation, int agg_k, int k,
                              int32_t* idx, float* score, float* emb_out, void* stream) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (h->detector) return fail(h, FR_ERR_STATE, "this handle is a detector (scrfd_10g); use fr_detect");
  if (!h->finalized) return fail(h, FR_ERR_STATE, "model not finalised (fr_finalize)");
  if (n < 0 || (n > 0 && (!rgb || !idx || !score))) return fail(h, FR_ERR_INVALID_ARGUMENT, "bad n or NULL buffer");
  if (h->sample_ids <= 0) return fail(h, FR_ERR_STATE, "sample gallery is empty (fr_samples_set first)");
  if (int rc = check_dev_err(h)) return rc;  // reported by earlier asynchronous work
  DeviceGuard dg(h->device);
  hipStream_t s = (hipStream_t)stream;
  float* emb = emb_out;
  if (!emb) {
    int rc = ensure_buf(h, &h->match_io, &h->match_io_cap, (size_t)n * 512 * sizeof(float));
    if (rc) return rc;
    emb = (float*)h->match_io;
  }
  int rc = embed_device(h, rgb, n, emb, 1, s);
  if (rc) return rc;
  return match_identities_device(h, emb, n, aggregation, agg_k, k, idx, score, s);
}

}  // extern "C"
