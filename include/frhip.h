/*
 * frhip.h — C ABI of the MI355X (gfx950) face embed + match hot path.
 *
 * The reference (tuoasty/FaceRecognitionPipeline) has no FFI: its seams are
 * Python duck types.  Each entry point below replaces one
 * of them; the Python host layer (facerecognitionpipeline_amd/face_embedder.py,
 * gallery_manager.py) binds these symbols with ctypes and keeps the
 * reference's method names, argument meaning and exception types.
 *
 * Conventions
 *  - Return value: FR_OK (0) or a negative FR_ERR_* code; fr_last_error()
 *    gives the message.  No call aborts the process.
 *  - "device" pointers are HIP device allocations on the handle's device;
 *    "host" pointers are ordinary host memory, borrowed for the call only.
 *  - `stream` is a hipStream_t (NULL = the null stream).  Device-pointer calls
 *    are asynchronous on that stream; host-pointer calls synchronise.  Every call
 *    on one handle must use the SAME stream: the handle's workspace (activations,
 *    stream-K slabs and tickets, staging buffers, captured graphs) is shared by
 *    all of its calls and only stream order keeps them apart.
 *  - Device-side errors: a kernel that detects a broken invariant (wino4_kernel: an LDS ring
 *    hand-off that timed out) records it in the handle's error word instead of hanging the GPU.
 *    Calls that synchronise (fr_embed_host, fr_match_topk_host, fr_detect, fr_blur_scores,
 *    fr_profile_read) then return FR_ERR_HIP for their own work; asynchronous calls (fr_embed,
 *    fr_embed_match, fr_match_topk) return it at their next entry once the faulty work has
 *    completed.  Results of the work queued before such an error are invalid.
 *  - One mutex per handle: a handle may be shared by threads (the reference
 *    server shares one FaceEmbedder/GalleryManager across Flask request
 *    threads, face_recognition_server.py:1102).
 *  - Embeddings are 512-d float32 rows; images are uint8 RGB HWC, C-contiguous:
 *    112x112x3 (the reference's aligned crops, face_recognition.py:64-74), or any
 *    size for fr_embed / fr_embed_host, which resize it first (face_embedder.py:94-96).
 */
#ifndef FRHIP_H_
#define FRHIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FR_OK 0
#define FR_ERR_INVALID_ARGUMENT (-1) /* Python: ValueError  */
#define FR_ERR_MISSING_PARAM (-2)    /* Python: RuntimeError (load_state_dict strict) */
#define FR_ERR_HIP (-3)              /* Python: RuntimeError */
#define FR_ERR_STATE (-4)            /* Python: RuntimeError (not finalised / no gallery) */
#define FR_ERR_UNSUPPORTED (-5)      /* Python: NotImplementedError */

#define FR_EMBED_DIM 512
#define FR_INPUT_SIZE 112

typedef struct fr_handle fr_handle;

/* Build an empty model.  Replaces FaceEmbedder.__init__'s
 * `net.build_model(architecture)` (face_embedder.py:27-49).
 * architecture: "ir_50" | "ir_101" (also "ir_18", "ir_34"); model_type: "adaface" (AdaFace
 * net.py keys) or "arcface" (the insightface arcface_torch IResNet behind the reference's ONNX
 * files, face_embedder.py:64-88: (x-127.5)/127.5 input, conv downsample in every stage, affine
 * BN1d, no L2 inside the model; keys conv1, bn1, prelu, layerS.U.{bn1,conv1,...}, bn2, fc, features).
 * max_batch: images per internal forward chunk (workspace sizing), 1..512. */
int fr_create(const char* architecture, const char* model_type, int device, int max_batch, fr_handle** out);
int fr_destroy(fr_handle* h);

/* One state-dict tensor (AdaFace: key WITHOUT the "model." prefix), float32
 * host data in PyTorch's layout (conv weights [out][in][kh][kw]).  Replaces
 * `self.model.load_state_dict(model_statedict)` (face_embedder.py:51-53);
 * num_batches_tracked keys are accepted and ignored. */
int fr_set_param(fr_handle* h, const char* name, const float* host_data, int64_t numel);
/* Fold BatchNorms, repack weights NHWC, upload.  Missing keys -> FR_ERR_MISSING_PARAM
 * (strict load_state_dict semantics).  Replaces `.to(device).eval()` (face_embedder.py:55-56). */
int fr_finalize(fr_handle* h);

/* Embed n crops.  Replaces FaceEmbedder.extract_embeddings_batch
 * (face_embedder.py:137-182) and extract_embedding (:112-135): cv2.resize to 112x112
 * (INTER_LINEAR, OpenCV fixed point) when height x width is not 112x112 (:94-96), BGR + LUT
 * normalise, IR forward, x/||x||, and with normalize!=0 the extra e/(||e||+1e-8).
 * rgb: device [n][height][width][3] uint8 (1 <= height, width <= 8192); out: device [n][512]. */
int fr_embed(fr_handle* h, const uint8_t* rgb, int n, int height, int width, float* out, int normalize,
             void* stream);
/* Same with host buffers (H2D, forward, D2H, synchronise). */
int fr_embed_host(fr_handle* h, const uint8_t* rgb, int n, int height, int width, float* out, int normalize);
/* The resize step alone: dst[i] = cv2.resize(src[i], (112, 112), INTER_LINEAR) for n device crops
 * of height x width (face_embedder.py:94-96).  src: device [n][height][width][3] uint8; dst: device
 * [n][112][112][3] uint8. */
int fr_resize_crops(fr_handle* h, const uint8_t* src, int n, int height, int width, uint8_t* dst, void* stream);

/* augment_face_for_enrollment (enroll_students.py:20-48) for n crops of one size: variant v of crop i,
 * in the reference's list order, at out[i][v].  v = 0 the crop; 1 cv2.flip(img, 1); 2..5
 * cv2.warpAffine by getRotationMatrix2D((W/2, H/2), -10 / -5 / 5 / 10, 1.0), INTER_LINEAR,
 * BORDER_REPLICATE; 6..9 clip(p + beta, 0, 255), beta -20 / -10 / 10 / 20; 10..13
 * clip(float32(p) * alpha, 0, 255) truncated, alpha 0.85 / 0.92 / 1.08 / 1.15.  Every variant is
 * uint8-exact; the rotation is pinned to this project's restatement of OpenCV's fixed-point warp
 * (oracle/align_ref.py: 10-bit map, 5-bit fractions, 15-bit weights, each tap clamped to the
 * image), not to cv2 itself, which is not a dependency.  The list's entries 14 (cv2.GaussianBlur)
 * and 15 (unseeded np.random.normal noise) are not implemented: num_augmentations 15 or 16 ->
 * FR_ERR_UNSUPPORTED; outside [1, 16] -> FR_ERR_INVALID_ARGUMENT.
 * crops: device uint8 [n][height][width][3] (1 <= height, width <= 8192); out: device uint8
 * [n][num_augmentations][height][width][3], face-major, so its first two axes flattened are the
 * reference's all_face_images order (:212-216); out must not overlap crops.  Asynchronous on
 * `stream`, no host staging; any handle will do, finalised or not (as fr_resize_crops).  n == 0 is
 * a no-op. */
#define FR_AUGMENT_MAX 14
int fr_augment_faces(fr_handle* h, const uint8_t* crops, int n, int height, int width, int num_augmentations,
                     uint8_t* out, void* stream);

/* Replace the gallery matrix (G rows of D=512 float32).  Replaces the per-query
 * `np.vstack` of GalleryManager.get_gallery_embeddings (gallery_manager.py:177-187):
 * the handle keeps one device-resident copy until the next fr_gallery_set.
 * src_is_device: 1 if E is a device pointer.  G == 0 clears the gallery. */
int fr_gallery_set(fr_handle* h, const float* E, int G, int D, int src_is_device, void* stream);
int fr_gallery_size(fr_handle* h, int* G);
/* Incremental gallery maintenance, so an enrollment change does not re-upload (or, across
 * GPUs, re-broadcast) the whole matrix.  Rows are in get_gallery_embeddings order (dict
 * insertion order, gallery_manager.py:177-187).
 * write_rows: rows [row0, row0+n) := E (row0 <= G; rows past G extend the gallery) -- add_student
 *   appends (:71-102), add_student(overwrite=True) / update_embeddings rewrite in place (:124-158).
 * delete_rows: drop rows [row0, row0+n), later rows move up -- delete_student (:160-169).
 * read: copy rows out (host or device). */
int fr_gallery_write_rows(fr_handle* h, int row0, int n, const float* E, int src_is_device, void* stream);
int fr_gallery_delete_rows(fr_handle* h, int row0, int n, void* stream);
int fr_gallery_read(fr_handle* h, int row0, int n, float* out, int dst_is_device, void* stream);

/* GalleryManager._aggregate_embeddings (gallery_manager.py:297-317) incl. the quality
 * filter (:104-122) for n_students at once (bulk enrollment).  emb: device [total][512] f32,
 * student i = rows [offsets[i], offsets[i+1]) (host offsets, offsets[0] = 0, 1..1024 rows
 * each); templates: device [n_students][512]; kept: device [n_students] rows surviving the
 * filter, or NULL.  Synchronises. */
#define FR_TEMPLATE_MEAN 0
#define FR_TEMPLATE_MEDIAN 1
#define FR_TEMPLATE_WEIGHTED_MEAN 2
int fr_build_templates(fr_handle* h, const float* emb, const int32_t* offsets, int n_students, int method,
                       float min_similarity, float* templates, int32_t* kept, void* stream);

/* Batched GalleryManager.search (gallery_manager.py:189-205): q/(||q||+1e-8),
 * S = E.q (fp32), top-k by descending score; equal scores by DESCENDING gallery row (a stable
 * ascending argsort reversed, which is what the reference's np.argsort(S)[::-1] gives; DESIGN.md
 * §3 "Tie policy").  k must be in [1, G] (G = fr_gallery_size), else FR_ERR_INVALID_ARGUMENT:
 * the Python layer clamps top_k to G as search() does.
 * Q: device [n][512]; idx: device [n][k] int32 gallery rows; score: device [n][k]. */
int fr_match_topk(fr_handle* h, const float* Q, int n, int k, int32_t* idx, float* score, void* stream);
/* Host-buffer variant (synchronises). */
int fr_match_topk_host(fr_handle* h, const float* Q, int n, int k, int32_t* idx, float* score);

/* Fused unit of work of FaceMatcher.match_single_face (face_matcher.py:52-58),
 * batched: embed(normalize=1) then match (same k contract and tie policy as fr_match_topk).
 * emb_out may be NULL.  Device pointers. */
int fr_embed_match(fr_handle* h, const uint8_t* rgb, int n, int k, int32_t* idx, float* score, float* emb_out,
                   void* stream);

/* FaceMatcher._aggregate_matches and _get_best_candidate (face_matcher.py:321-385) for n_tracks
 * tracks in one launch, on the top-k output of fr_match_topk / fr_embed_match while it is on the
 * device.  idx / score: device [total][k] (k >= 1; only column 0, each frame's top-1, is read; a
 * gallery row stands for its student id); track t = frames [offsets[t], offsets[t+1]) (host offsets,
 * offsets[0] = 0, 1..FR_TRACK_MAX_FRAMES frames each).  Per track:
 *   quality frame  (double)score >= min_quality (the reference's 0.55)
 *   pool           the quality frames, or all frames when there is none
 *   winner         the row with the most pool frames; equal counts: the row whose first pool frame
 *                  comes earliest (Counter.most_common order); second = the next row in that order
 *   ratio          winner_count / pool_size;  confidence = mean of the winner's pool scores (double)
 *   consensus      ratio > 0.5, or with a second row: ratio > 0.4 && winner_count >= 2 * second_count
 *   status         FR_TRACK_FEW_FRAMES if quality_frames < min_frames (the reference's 3), else
 *                  FR_TRACK_NO_CONSENSUS, else FR_TRACK_BELOW_THRESHOLD if confidence <
 *                  similarity_threshold, else FR_TRACK_RECOGNIZED
 * out_i[t] = {status, winner_row, winner_count, pool_size, second_count, n_frames, quality_frames, 0};
 * out_d[t] = {confidence, ratio}.  The winner over the pool is both _aggregate_matches' winner and
 * _get_best_candidate's candidate, so one record serves both.  Deterministic: integer votes, the
 * confidence summed in double in one fixed order.  Any handle will do, finalised or not (as
 * fr_resize_crops).  Synchronises (the offsets are staged from the host).  n_tracks == 0 is a
 * no-op; NULL buffers, k < 1, min_frames < 1, offsets[0] != 0 and an empty or over-long track ->
 * FR_ERR_INVALID_ARGUMENT (checked before the handle, so also reported for h == NULL). */
#define FR_TRACK_RECOGNIZED 0
#define FR_TRACK_FEW_FRAMES 1 /* fewer than min_frames quality frames */
#define FR_TRACK_NO_CONSENSUS 2
#define FR_TRACK_BELOW_THRESHOLD 3
#define FR_TRACK_MAX_FRAMES 1024
int fr_track_consensus(fr_handle* h, const int32_t* idx, const float* score, int k, const int32_t* offsets,
                       int n_tracks, double min_quality, int min_frames, double similarity_threshold,
                       int32_t* out_i /* device [n_tracks][8] */, double* out_d /* device [n_tracks][2] */,
                       void* stream);

/* Photograph roll call: the decision of FaceMatcher.match_single_image (face_matcher.py:148-271) for
 * every face of n_images photographs in one launch, on the top-k output of fr_match_topk /
 * fr_embed_match / fr_match_identities while it is on the device.  idx / score: device [total][k]
 * (k >= 1, rows descending; a gallery row or identity index stands for its student); photograph p =
 * faces [offsets[p], offsets[p+1]) (host offsets, offsets[0] = 0, 0..FR_ROLLCALL_MAX_FACES faces each).
 * A claim of a face is a column c with (double)score[f][c] >= similarity_threshold (never a NaN; the
 * threshold may be negative).
 *   FR_ROLLCALL_INDEPENDENT  the reference's rule, every face on its column 0 alone:
 *                            FR_FACE_RECOGNIZED if it is a claim, else FR_FACE_CANDIDATE (the
 *                            reference's best_candidate)
 *   FR_ROLLCALL_EXCLUSIVE    a row is held by at most one face of a photograph: all claims (f, c) of
 *                            the photograph ordered by score descending (as f32 values), then face
 *                            ascending, then column ascending, are scanned, and a claim is granted if
 *                            its face holds nothing yet and its row is not held.  A face with a
 *                            granted claim is FR_FACE_RECOGNIZED with that row, score and column; a
 *                            face whose column 0 was a claim but which was granted nothing is
 *                            FR_FACE_DISPLACED, one whose column 0 was no claim FR_FACE_CANDIDATE
 *                            (both report column 0)
 * out_face[f] = {status, row, column, 0}; out_score[f] = the reported score, bit for bit;
 * out_image[p] = {n_faces, recognized, candidates, displaced}.  Comparisons only: exact, and a
 * photograph's result depends on nothing but its own faces.  Any handle will do, finalised or not.
 * Synchronises (the offsets are staged from the host).  n_images == 0 is a no-op; NULL buffers,
 * k < 1, offsets[0] != 0, an over-long photograph and an unknown mode -> FR_ERR_INVALID_ARGUMENT
 * (checked before the handle, so also reported for h == NULL). */
#define FR_ROLLCALL_INDEPENDENT 0
#define FR_ROLLCALL_EXCLUSIVE 1
#define FR_FACE_RECOGNIZED 0
#define FR_FACE_CANDIDATE 1
#define FR_FACE_DISPLACED 2 /* its top-1 row went to another face of the photograph */
#define FR_ROLLCALL_MAX_FACES 1024
int fr_photo_rollcall(fr_handle* h, const int32_t* idx, const float* score, int k,
                      const int32_t* offsets /* host [n_images + 1] */, int n_images, double similarity_threshold,
                      int mode, int32_t* out_face /* device [total][4] */, float* out_score /* device [total] */,
                      int32_t* out_image /* device [n_images][4] */, void* stream);

/* Capture sessions: SimpleTracker.update and FrameAccumulator (face_detection.py:11-228) with the
 * is_valid test of CameraFaceCapture.process_frame (:271-283) for n_clips independent sessions
 * (cameras) in one launch.  Each session starts from an empty tracker with next_track_id = 1.
 * Detections are a CSR over frames, frames a CSR over clips; the number of frames is
 * clip_offsets[n_clips] and the number of detections frame_offsets[that].
 *   tracker   The live tracks are an ordered list (the reference's dict order): a matched track keeps
 *             its place, deleted tracks leave with the order of the rest kept, new tracks are appended
 *             in detection order.  Per track x detection pair q = (sx_t - sx_d)^2 + (sy_t - sy_d)^2
 *             with sx = x1 + x2, sy = y1 + y2 in int64: 4 x the squared centroid distance, exact.
 *             Greedy matching takes the unmatched pair of smallest q, ties to the smallest flat
 *             index track_pos * n_dets + det_idx (numpy's argmin), until no unmatched pair has
 *             q < q_limit; q_limit is the smallest integer q >= 0 with sqrt(q / 4.0) >= max_distance
 *             in double, so the test is the reference's `distances.min() < max_distance` bit for bit
 *             (max_distance <= 0 or NaN: no pair matches).  A matched track takes the detection's box
 *             and disappeared = 0; an unmatched one gets disappeared += 1 and is deleted when that
 *             exceeds max_disappeared; every unmatched detection opens a track with the next id.
 *   quality   nb = min(blur / 200.0, 1.0); pose = max(0, 1.0 - (|yaw| / 90.0 + |pitch| / 90.0 +
 *             |roll| / 90.0) / 3.0); quality = det * 0.4 + nb * 0.3 + pose * 0.3, in double in this
 *             order without contraction (compute_quality_score); metrics must be finite.
 *   saving    A detection passes when valid != 0 and !(quality < min_quality_score).  A track accepts
 *             its first target_frames passing detections in frame order; with target_frames of them
 *             it is completed and they are saved, with fewer they are saved only if save_partial != 0
 *             (the reference's 's' key, then quitting).  slot = the rank among the track's accepted
 *             frames by descending quality, equal qualities in frame order (Python's stable
 *             sort(reverse=True)): the NNN of frame_NNN.jpg; -1 for everything that is not saved.
 * clip_info[c] = {tracks opened, tracks completed, frames saved, error}.  A clip whose live tracks
 * would exceed FR_CAPTURE_MAX_TRACKS (error FR_CAPTURE_ERR_TRACKS) or with a coordinate beyond
 * +-FR_CAPTURE_COORD_MAX (FR_CAPTURE_ERR_COORD) gets {0, 0, 0, error}, track_id 0 and slot -1
 * throughout (its qualities are still written), the other clips their results, and the call returns
 * FR_ERR_UNSUPPORTED after its synchronisation.  Deterministic: integers but for the quality.  Any
 * handle will do, finalised or not.  Synchronises (the offsets are staged from the host).
 * n_clips == 0 is a no-op.  NULL buffers, n_clips < 0, offsets that do not start at 0 or that
 * decrease, a frame over FR_CAPTURE_MAX_FACES, a clip over FR_CAPTURE_MAX_DETS, target_frames outside
 * [1, FR_CAPTURE_MAX_TARGET] and max_disappeared < 0 -> FR_ERR_INVALID_ARGUMENT (checked before the
 * handle, so also reported for h == NULL). */
#define FR_CAPTURE_MAX_FACES 128  /* detections in one frame */
#define FR_CAPTURE_MAX_TRACKS 128 /* tracks alive at once in one clip */
#define FR_CAPTURE_MAX_DETS 4096  /* detections in one clip */
#define FR_CAPTURE_MAX_TARGET 64  /* target_frames */
#define FR_CAPTURE_COORD_MAX (1 << 20)
#define FR_CAPTURE_ERR_TRACKS 1
#define FR_CAPTURE_ERR_COORD 2
int fr_capture_tracks(fr_handle* h,
                      const int32_t* bbox,          /* device [total][4] x1 y1 x2 y2 (bbox.astype(int)) */
                      const double* metrics,        /* device [total][5] det_score, blur_score, yaw, pitch, roll */
                      const uint8_t* valid,         /* device [total] face['is_valid'] */
                      const int32_t* frame_offsets, /* host [n_frames + 1] */
                      const int32_t* clip_offsets,  /* host [n_clips + 1] */
                      int n_clips, int max_disappeared, double max_distance, int target_frames,
                      double min_quality_score, int save_partial,
                      int32_t* track_id, /* device [total] >= 1 */
                      double* quality,   /* device [total] */
                      int32_t* slot,     /* device [total] */
                      int32_t* clip_info /* device [n_clips][4] */, void* stream);

/* Live sessions: LiveFaceRecognition._simple_track_assignment (face_recognition_live.py:249-285) and
 * the gating and frame selection of LiveRecognitionTracker (:18-80) as process_frame drives them
 * (:339-355), for n_clips independent sessions (cameras) in one launch.  Each session starts with no
 * tracks and next_track_id = 0; a frame's 1-based frame_count is its index in the clip plus 1.
 * Detections are a CSR over frames, frames a CSR over clips, as fr_capture_tracks takes them; a clip
 * may hold any number of detections.
 *   assignment  The live list is the previous frame's faces in that frame's detection order (the
 *               reference's dict, replaced wholesale each frame: no disappearance tolerance).  Per
 *               face the nearest live track by q = (sx_t - sx_d)^2 + (sy_t - sy_d)^2 with
 *               sx = x1 + x2, sy = y1 + y2 in int64 (4 x the squared centroid distance, exact), among
 *               the tracks with q < q_limit (fr_capture_tracks' q_limit of max_distance: the
 *               reference's `distance < best_distance` from best_distance = max_distance, bit for
 *               bit; max_distance <= 0 or NaN: nothing matches); equal q goes to the earlier list
 *               position (the strict <).  The search reads the previous frame only.  A track goes to
 *               the lowest-indexed face that chose it; every other face, one whose nearest track was
 *               taken included (it does not fall back to another track in range), opens the next id
 *               in detection order.  A track that no face chose is gone.
 *               track_id[d] >= 0; prev[d] = the global index of the track's detection in the previous
 *               frame, -1 for a new track.
 *   gating      On a frame with frame_count % recognition_interval == 0, a track that was present on
 *               a < max_attempts earlier such frames gets attempt[d] = a (should_recognize without
 *               its "already recognised" test: the count is speculative, the caller drops the
 *               attempts that follow a recognition); otherwise attempt[d] = -1.
 *   selection   With attempt[d] >= 0, best[d] = the global index of the detection with the largest
 *               key among the last min(run length, buffer_size) detections of d's prev chain, d
 *               included; key = (double)det_score * min(blur_score / 100.0, 1.0) without contraction;
 *               the oldest of equal keys (Python's max over the deque).  Otherwise best[d] = -1.
 *               metrics must be finite.
 * clip_info[c] = {tracks opened, candidates (attempt >= 0), frames, error}.  A clip with a coordinate
 * beyond +-FR_CAPTURE_COORD_MAX gets {0, 0, 0, FR_LIVE_ERR_COORD}, track_id 0 and -1 in prev, attempt
 * and best throughout, the other clips their results, and the call returns FR_ERR_UNSUPPORTED after
 * its synchronisation.  Deterministic: integers but for the key.  Any handle will do, finalised or
 * not.  Synchronises (the offsets are staged from the host).  n_clips == 0 is a no-op.  NULL buffers,
 * n_clips < 0, offsets that do not start at 0 or that decrease, a frame over FR_LIVE_MAX_FACES,
 * recognition_interval < 1, max_attempts outside [1, FR_LIVE_MAX_ATTEMPTS] and buffer_size outside
 * [1, FR_LIVE_MAX_BUFFER] -> FR_ERR_INVALID_ARGUMENT (checked before the handle, so also reported for
 * h == NULL). */
#define FR_LIVE_MAX_FACES 128   /* detections in one frame */
#define FR_LIVE_MAX_ATTEMPTS 16 /* max_attempts */
#define FR_LIVE_MAX_BUFFER 64   /* buffer_size */
#define FR_LIVE_ERR_COORD 2
int fr_live_tracks(fr_handle* h,
                   const int32_t* bbox,          /* device [total][4] x1 y1 x2 y2 (bbox.astype(int)) */
                   const double* metrics,        /* device [total][2] det_score, blur_score */
                   const int32_t* frame_offsets, /* host [n_frames + 1] */
                   const int32_t* clip_offsets,  /* host [n_clips + 1] */
                   int n_clips, double max_distance, int recognition_interval, int max_attempts, int buffer_size,
                   int32_t* track_id, /* device [total] >= 0 */
                   int32_t* prev,     /* device [total] */
                   int32_t* attempt,  /* device [total] */
                   int32_t* best,     /* device [total] */
                   int32_t* clip_info /* device [n_clips][4] */, void* stream);

/* Server sessions: the gating, the retry cooldown and the frame selection of the server's
 * LiveRecognitionTracker (face_recognition_server.py:23-124) as process_faces / process_full_frame
 * drive it (:368-413, :638-678), for every track of a recorded request log in one launch.  Track ids
 * come from outside, so tracks do not interact: the log's n_dets detections are grouped by track,
 * track t = order[track_offsets[t] .. track_offsets[t+1]), detection indices in arrival order.  Per
 * appearance, with now = clock[d] (the request's clock, the same for all faces of a request):
 *   FR_SERVER_COOLDOWN      the track is in cooldown and now < deadline.
 *   FR_SERVER_RESET         in cooldown and now >= deadline: the cooldown ends, the cycle's attempts
 *                           go to 0 and the ring is emptied, this appearance included (no attempt).
 *   FR_SERVER_COOLDOWN_SET  the cycle's attempts reached max_attempts: deadline = now +
 *                           retry_cooldown (one double addition).  So a cooldown starts on the first
 *                           appearance after the last failed attempt.
 *   FR_SERVER_ATTEMPT       otherwise, when the best face of the window has det_score > det_gate.
 *   FR_SERVER_GATED         otherwise.
 * The window is the last min(appearances since the run start, buffer_size) appearances, this one
 * included; a run starts at the track's first appearance and after every reset.  The best face is the
 * one of largest key = (double)det_score * min(blur_score / 100.0, 1.0), without contraction, the
 * oldest of equal keys.  attempt[d] = the 0-based ordinal of the attempt among all attempts of the
 * track, through cooldown cycles, as if no earlier attempt had succeeded (the caller drops what
 * follows a success); best[d] = the detection the attempt embeds; both -1 without an attempt.
 * track_info[t] = {attempts, cooldowns set, resets, error}.  A track with a non-finite metric or
 * clock (FR_SERVER_ERR_VALUE) or an order entry outside [0, n_dets) (FR_SERVER_ERR_ORDER) gets
 * {0, 0, 0, error}, -1 / -1 / FR_SERVER_GATED on its detections, the other tracks their results, and
 * the call returns FR_ERR_UNSUPPORTED after its synchronisation.  Detections no track names are not
 * written.  Deterministic.  Any handle will do, finalised or not.  Synchronises (the offsets are
 * staged from the host).  n_tracks == 0 is a no-op.  NULL buffers, n_tracks < 0, n_dets < 0, offsets
 * that do not start at 0 or that decrease, max_attempts outside [1, FR_SERVER_MAX_ATTEMPTS],
 * buffer_size outside [1, FR_SERVER_MAX_BUFFER], retry_cooldown negative or not finite and det_gate
 * not finite -> FR_ERR_INVALID_ARGUMENT (checked before the handle, so also reported for h == NULL). */
#define FR_SERVER_MAX_ATTEMPTS 16 /* max_attempts */
#define FR_SERVER_MAX_BUFFER 64   /* buffer_size */
#define FR_SERVER_GATED 0
#define FR_SERVER_ATTEMPT 1
#define FR_SERVER_COOLDOWN 2
#define FR_SERVER_COOLDOWN_SET 3
#define FR_SERVER_RESET 4
#define FR_SERVER_ERR_VALUE 1
#define FR_SERVER_ERR_ORDER 2
int fr_server_tracks(fr_handle* h,
                     const double* metrics,        /* device [n_dets][2] det_score, blur_score */
                     const double* clock,          /* device [n_dets] seconds */
                     const int32_t* order,         /* device [track_offsets[n_tracks]] */
                     const int32_t* track_offsets, /* host [n_tracks + 1] */
                     int n_tracks, int n_dets, int max_attempts, int buffer_size, double retry_cooldown,
                     double det_gate,
                     int32_t* attempt,   /* device [n_dets] */
                     int32_t* best,      /* device [n_dets] */
                     int32_t* state,     /* device [n_dets] */
                     int32_t* track_info /* device [n_tracks][4] */, void* stream);

/* Model evaluation, step 1 (evaluate_models_v2.ipynb: cosine_similarity, aggregate_max / _mean /
 * _topk as identify_probe applies them): the score of every probe against every identity of a
 * multi-embedding gallery.  Q: device [n][512]; E: device [G][512], an explicit matrix (the handle's
 * serving gallery is neither read nor changed); identity i owns rows [id_offsets[i], id_offsets[i+1])
 * of E (host offsets, id_offsets[0] = 0, 1..FR_EVAL_MAX_ROWS rows each, G = id_offsets[n_ids]).
 *   sim[p][r]   cosine_similarity(Q[p], E[r]): the f32 dot when |norm - 1| < 0.01 for both rows, else
 *               dot / (norm_q * norm_e) in f32.  A row's norm is the f32 rounding of the square root of
 *               its double sum of squares, computed once per call.  The dots run on the implicit-GEMM
 *               conv path without renormalisation, in the handle's precision mode (fr_set_precision).
 *   out[p][i]   FR_AGG_MAX: the f32 maximum of the identity's sim values.  FR_AGG_MEAN: the f32
 *               rounding of (double sum in row order) / count.  FR_AGG_TOPK: the min(k, count) largest
 *               values summed in double in descending order, divided by their number, rounded to f32
 *               (k is ignored by the other two).
 * out[p] depends on nothing but sim[p] and the offsets.  sim: device [n][G] and then filled, or NULL
 * (the scores then live in the handle's workspace, a chunk of probes below 2 GiB at a time).  Any
 * handle will do, finalised or not.  Synchronises (the offsets are staged from the host).  n == 0 is
 * a no-op.  NULL buffers, n < 0, n_ids < 1, id_offsets[0] != 0, an empty identity or one over
 * FR_EVAL_MAX_ROWS, an unknown aggregation and FR_AGG_TOPK with k < 1 -> FR_ERR_INVALID_ARGUMENT;
 * FR_AGG_TOPK with k > FR_EVAL_MAX_K -> FR_ERR_UNSUPPORTED (all checked before the handle, so also
 * reported for h == NULL). */
#define FR_AGG_MAX 0
#define FR_AGG_MEAN 1
#define FR_AGG_TOPK 2
#define FR_EVAL_MAX_ROWS 1024 /* gallery rows of one identity */
#define FR_EVAL_MAX_K 16
int fr_identity_scores(fr_handle* h, const float* Q /* device [n][512] */, int n,
                       const float* E /* device [G][512] */, const int32_t* id_offsets /* host [n_ids + 1] */,
                       int n_ids, int aggregation, int k, float* out /* device [n][n_ids] */,
                       float* sim /* device [n][G], or NULL */, void* stream);

/* Model evaluation, step 2: the per-probe part of identify_probe(threshold=0.0) and
 * compute_rank_metrics plus the threshold loops of the evaluate_*_comprehensive functions, in one
 * launch over a score matrix that is on the device.  Probe p has row a = scores[p] and t = true_id[p];
 * a t outside [0, n_ids) means "not enrolled" and reads nothing.
 *   best        the largest score, equal scores to the lowest identity index (Python's stable
 *               sorted(..., reverse=True) over the dict order)
 *   predicted   best, or -1 if a[best] < 0 (identify_probe returns None)
 *   enrolled    rank = 1 + #{j : a[j] > a[t]} + #{j < t : a[j] == a[t]}; genuine = a[t];
 *               impostor = max over j != t, has_impostor = (n_ids > 1)
 *   otherwise   rank = 0; genuine = 0.0f; impostor = a[best], has_impostor = 1
 * rec_i[p] = {predicted, best, rank, has_impostor}; rec_f[p] = {a[best], genuine, impostor or -1.0f, 0}.
 * counts[j] for thresholds[j], with accepted = (double)a[best] >= thresholds[j] (in double: the
 * notebook's thresholds are float64): {tp: accepted, enrolled and predicted == t; fp: accepted and
 * not tp; fn: not accepted; the number of enrolled probes with (double)genuine >= thresholds[j]}.
 * The call zeroes counts itself.  Deterministic: integer sums; a record depends on nothing but its
 * row.  Scores must not be NaN.  Any handle will do.  Synchronises (the thresholds are staged from the
 * host).  n == 0 zeroes counts only.  NULL buffers, n < 0, n_ids < 1 and n_thr outside
 * [0, FR_EVAL_MAX_THRESHOLDS] -> FR_ERR_INVALID_ARGUMENT (checked before the handle). */
#define FR_EVAL_MAX_THRESHOLDS 256
int fr_eval_probes(fr_handle* h, const float* scores /* device [n][n_ids] */, int n, int n_ids,
                   const int32_t* true_id /* device [n] */, const double* thresholds /* host [n_thr] */, int n_thr,
                   int32_t* rec_i /* device [n][4] */, float* rec_f /* device [n][4] */,
                   int64_t* counts /* device [n_thr][4] */, void* stream);

/* Identity matching: serving with the configuration the evaluation recommends.  Where fr_match_topk
 * scores one template per student, these calls score every identity over all of its enrolled rows,
 * as identify_probe does (fr_identity_scores' sim and out), against a sample gallery that lives in the
 * handle beside the template gallery; fr_gallery_* and fr_match_topk neither read nor change it, and
 * these calls neither read nor change theirs.
 *
 * fr_samples_set: E [id_offsets[n_ids]][512] f32 (host, or device with src_is_device), identity i =
 * rows [id_offsets[i], id_offsets[i+1]) (host offsets, id_offsets[0] = 0, 1..FR_EVAL_MAX_ROWS rows each).
 * Copies the rows and stages everything a match needs: the offsets, the kernels' tile cuts, every
 * row's norm (the f32 rounding of the square root of its double sum of squares, as fr_identity_scores
 * computes it per call) and whether any row is off-unit.  Replaces the previous sample gallery;
 * n_ids == 0 clears it.  Synchronises -- the only call of the four that does.  Any handle will do.
 * NULL buffers, n_ids < 0 and offsets fr_identity_scores refuses -> FR_ERR_INVALID_ARGUMENT (checked
 * before the handle, so also reported for h == NULL); 2^29 rows or more -> FR_ERR_UNSUPPORTED.
 * fr_samples_size: the identities and rows held (0, 0 without a sample gallery); either may be NULL. */
int fr_samples_set(fr_handle* h, const float* E, const int32_t* id_offsets /* host [n_ids + 1] */, int n_ids,
                   int src_is_device, void* stream);
int fr_samples_size(fr_handle* h, int* n_ids, int* rows);

/* The k best identities of n queries.  Q: device [n][512]; idx / score: device [n][k], idx identity
 * indices (the order of fr_samples_set's offsets).  The scores of query p are row p of
 * fr_identity_scores' out for (Q, the sample rows, the offsets, aggregation, agg_k): the notebook's
 * cosine_similarity 0.01 rule on raw dots, neither side renormalised, then FR_AGG_MAX / _MEAN / _TOPK
 * (agg_k is the top-k mean's k and ignored by the other two).  The k largest come back in descending
 * order, equal scores with the LOWER identity index first: Python's stable sorted(..., reverse=True)
 * over the dict order in identify_probe, the rule of fr_eval_probes' best.  (fr_match_topk ranks the
 * higher row first.)  Scores must not be NaN.
 *   small    one query, or n <= 16 queries with n * rows <= 65,536: one fused launch.  A workgroup
 *            dots one query against one tile of whole identities, applies the 0.01 rule on the
 *            stored norms and aggregates in LDS; only [n][n_ids] scores reach HBM.  The dots are f32
 *            fmaf chains in a fixed order, whatever the precision mode.
 *   larger   fr_identity_scores' launches on the stored offsets, tiles and norms: the score GEMM in
 *            the handle's precision mode into its workspace (chunks of queries below 2 GiB), the
 *            aggregation kernel, the top-k.
 * Both paths aggregate with one loop, so a score depends on nothing but the identity's similarity
 * values; the two paths' dots differ in summation order (a few f32 ulp).  Asynchronous on stream: no
 * host synchronise, nothing staged from host memory (workspace may grow on first use).  n == 0 is a
 * no-op.  No sample gallery -> FR_ERR_STATE.  NULL buffers, n < 0, an unknown aggregation, FR_AGG_TOPK
 * with agg_k < 1 and k outside [1, n_ids] -> FR_ERR_INVALID_ARGUMENT; FR_AGG_TOPK with agg_k >
 * FR_EVAL_MAX_K -> FR_ERR_UNSUPPORTED. */
int fr_match_identities(fr_handle* h, const float* Q /* device [n][512] */, int n, int aggregation, int agg_k, int k,
                        int32_t* idx /* device [n][k] */, float* score /* device [n][k] */, void* stream);
/* fr_embed_match with identity matching in place of the template match: the same forward (normalised
 * embeddings, graph replay and lanes as fr_embed_match runs them, so emb_out is bitwise its emb_out),
 * then fr_match_identities on the embeddings, on the same stream.  emb_out: device [n][512], or NULL. */
int fr_embed_match_identities(fr_handle* h, const uint8_t* rgb /* device [n][112][112][3] */, int n, int aggregation,
                              int agg_k, int k, int32_t* idx, float* score, float* emb_out, void* stream);

/* FaceAligner.align for n faces of one frame (face_recognition.py:50-75): similarity fit of
 * each face's 5 landmarks to the reference template (cv2.estimateAffinePartial2D semantics,
 * host, double) then warpAffine INTER_LINEAR / BORDER_CONSTANT 0 on the device, so the crops
 * stay in HBM for fr_embed.  frame: device uint8 [height][width][3] RGB; landmarks: host float
 * [n][5][2]; out: device uint8 [n][out_size][out_size][3]; tforms: host double [n][2][3] forward
 * maps as cv2 returns them, or NULL.  Synchronises (the maps are staged from the host). */
int fr_align_faces(fr_handle* h, const uint8_t* frame, int height, int width, const float* landmarks, int n,
                   int out_size, uint8_t* out, double* tforms, void* stream);
/* cv2.warpAffine(frame, M, (out_size, out_size), INTER_LINEAR, BORDER_CONSTANT, 0) for n
 * caller-supplied FORWARD maps (host double [n][2][3], e.g. cv2.getAffineTransform's for
 * FaceAligner.align(method != 'similarity'), face_recognition.py:66-67).  Synchronises. */
int fr_warp_affine(fr_handle* h, const uint8_t* frame, int height, int width, const double* tforms, int n,
                   int out_size, uint8_t* out, void* stream);
/* FaceQualityFilter.compute_blur_score for n images of one size (face_recognition.py:94-99):
 * cv2.Laplacian(gray, CV_64F).var() with gray = cvtColor(RGB2GRAY) of a 3- (or 4-) channel
 * image, or the image itself for channels == 1 (the reference's 2-D branch); ksize 1,
 * BORDER_REFLECT_101.  The variance is summed in numpy's order (ndarray.var's chunked pairwise
 * sum; derived for and checked against numpy 2.2), so it is bitwise the reference's value there.
 * crops: device uint8 [n][height][width][channels], any height, width >= 1 (height * width
 * < 2^31); channels 1, 3 or 4; scores: host double [n].  Runs on `stream` (NULL: the null stream)
 * and synchronises that stream only. */
int fr_blur_scores(fr_handle* h, const uint8_t* crops, int n, int height, int width, int channels, double* scores,
                   void* stream);

/* FaceDetector.detect (face_recognition.py:31-48: insightface SCRFD det_10g at det_size
 * 640x640, det_thresh, NMS IoU 0.4) for n frames of one size.  The handle is created with
 * fr_create("scrfd_10g", "scrfd", device, max_frames (1..64), &h) and loaded with the
 * state dict of oracle/scrfd.py's network (fr_set_param / fr_finalize).
 * frames: device uint8 [n][height][width][3] RGB.  Per frame f, counts[f] = detections
 * after NMS (score order) and dets[f][i][0..14] = x1 y1 x2 y2 score, then 5 landmarks
 * (x, y), in frame pixels, for i < min(counts[f], max_faces) (host buffers; synchronises).
 * That holds for every max_faces >= 0 (a frame keeps at most 4096 detections, and the
 * detector's own buffer holds that many); rows from min(counts[f], max_faces) on are not
 * written.  More than 4096 anchors above det_thresh in one frame -> FR_ERR_UNSUPPORTED. */
int fr_detect(fr_handle* h, const uint8_t* frames, int n, int height, int width, float det_thresh, int max_faces,
              float* dets, int32_t* counts, void* stream);

/* fr_detect for n images of n different sizes (a folder of photographs): images: host array of n
 * device pointers, image i uint8 [h_i][w_i][3] RGB; sizes: host int32 [n][2] = h_i, w_i, each side in
 * [1, FR_IMAGE_MAX_SIDE].  Every image gets its own letterbox geometry (new_w, new_h, det_scale, resize
 * tables and SIMD / scalar rounding split, as fr_detect computes them for that size): its canvas is
 * bitwise fr_detect's canvas of that image alone, and decode divides by its own det_scale.  NMS, the
 * layout of dets / counts (host; synchronises) and the 4096-anchor limit (FR_ERR_UNSUPPORTED; the
 * message names the image) are fr_detect's.
 *   Chunk rule (part of the contract: the conv kernels' fp32 rounding depends on the batch an image
 *   runs in): images run in input order in chunks of the handle's max_frames, chunk c = images
 *   [c * max_frames, min(n, (c + 1) * max_frames)).
 *   Row-reduction rule: a chunk skips the letterbox's invariant bottom rows as fr_detect does, planned
 *   for the largest new_h of the chunk (the canvas rows from there on are zeros in every image of the
 *   chunk); a chunk that holds a portrait image therefore skips nothing.
 *   A chunk whose images all have one size runs fr_detect's network launches on fr_detect's canvases:
 *   its dets and counts are bitwise fr_detect's for the same frames.
 * FR_ERR_INVALID_ARGUMENT, with the image's index in the message: a NULL pointer in images, a side
 * outside [1, FR_IMAGE_MAX_SIDE], an image too small to letterbox (new_w < 1 or new_h < 1); also
 * max_faces < 1 and NULL arrays.  Nothing runs when any image is refused.  n == 0 is a no-op. */
#define FR_IMAGE_MAX_SIDE 8192
int fr_detect_images(fr_handle* h, const uint8_t* const* images /* host [n] device pointers */,
                     const int32_t* sizes /* host [n][2] = height, width */, int n, float det_thresh,
                     int max_faces, float* dets /* host [n][max_faces][15] */, int32_t* counts /* host [n] */,
                     void* stream);

/* fr_align_faces for faces that come from different images: face j reads image face_image[j] (images /
 * sizes as fr_detect_images takes them, any side >= 1; an image no face refers to is fine).  The
 * similarity fit is fr_align_faces' (host, double), the warp its arithmetic (INTER_LINEAR,
 * BORDER_CONSTANT 0): out[j] and tforms[j] are bitwise what fr_align_faces gives for that image and that
 * face alone.  One launch and one staging copy for any n_faces.  Synchronises.  Any handle will do,
 * finalised or not.  FR_ERR_INVALID_ARGUMENT: face_image[j] outside [0, n_images), NULL buffers or image
 * pointers, a side < 1, out_size outside [1, 1024], a failed fit.  n_faces == 0 is a no-op. */
int fr_align_images(fr_handle* h, const uint8_t* const* images, const int32_t* sizes, int n_images,
                    const float* landmarks /* host [n_faces][5][2] */, const int32_t* face_image /* host [n_faces] */,
                    int n_faces, int out_size, uint8_t* out /* device [n_faces][S][S][3] */,
                    double* tforms /* host [n_faces][2][3] or NULL */, void* stream);

/* fr_resize_crops for n crops of n different sizes (a folder of probe crops): images / sizes as
 * fr_detect_images takes them.  dst[i] = cv2.resize(image i, (112, 112), INTER_LINEAR), bitwise what
 * fr_resize_crops gives for image i alone at its size; a 112 x 112 image comes through byte for byte.
 * Images run in input order in chunks of the handle's max_batch: one staging copy (the chunk's
 * descriptors and its coefficient tables, built once per distinct size of the chunk) and one launch
 * per chunk.  Any handle will do, finalised or not.  Synchronises `stream` at entry (the host
 * staging of an earlier call may still be read by a pending copy) and is asynchronous on it after
 * that: the images must stay alive until the stream reaches the end of the call's work.
 * FR_ERR_INVALID_ARGUMENT, with the image's index in the message: a NULL pointer in images, a side
 * outside [1, FR_IMAGE_MAX_SIDE]; also NULL arrays.  Nothing runs when any image is refused.
 * n == 0 is a no-op. */
int fr_resize_images(fr_handle* h, const uint8_t* const* images /* host [n] device pointers */,
                     const int32_t* sizes /* host [n][2] = height, width */, int n,
                     uint8_t* dst /* device [n][112][112][3] */, void* stream);
/* fr_embed for the same kind of list: chunk c = images [c * max_batch, min(n, (c + 1) * max_batch))
 * (fr_embed's chunk boundaries) is resized straight into the forward's input and embedded, so out is
 * bitwise fr_embed(h, dst, n, 112, 112, out, normalize, stream) on fr_resize_images' dst.
 * Synchronises as fr_resize_images does; its errors, and fr_embed's FR_ERR_STATE on a handle that is
 * not a finalised embedder. */
int fr_embed_images(fr_handle* h, const uint8_t* const* images, const int32_t* sizes, int n,
                    float* out /* device [n][512] */, int normalize, void* stream);

/* ---- The frames -> (detections, crops, blur) chain with device outputs.  The three calls below
 * are fr_detect, fr_align_faces and fr_blur_scores with every output in device memory: they are
 * asynchronous on `stream`, synchronise nothing and read no host memory after they return, so the
 * chain can run behind other work, be captured in a hipGraph, and a batch of frames needs one
 * device -> host copy (of dets, counts, ok and the blur scores) before the host quality gate.
 * While a captured graph of them is in use, the handle's workspace it was captured with must stay:
 * make no fr_align_device call with more slots and no multi-block fr_blur_scores* call with more
 * images than the captured ones. */

/* fr_detect with dets (device float [n][max_faces][15]) and counts (device int32 [n]) on the
 * device: the same chunks of max_frames, the same row reduction, the same kernels, NMS writing
 * the caller's rows, so counts[f] and rows i < min(counts[f], max_faces) are bitwise fr_detect's
 * (the other rows are not written).  A frame with more than 4096 anchors above det_thresh, where
 * fr_detect returns FR_ERR_UNSUPPORTED, gets counts[f] = -1 (its rows are unspecified); the other
 * frames of the call are unaffected.  The letterbox resize tables are kept on the device per frame
 * size (the last 16 sizes): the first call on a size allocates and uploads its tables with one
 * synchronous copy (not capturable: warm a size up once), a later call copies nothing. */
int fr_detect_device(fr_handle* h, const uint8_t* frames /* device [n][height][width][3] */, int n, int height,
                     int width, float det_thresh, int max_faces, float* dets, int32_t* counts, void* stream);

/* FaceAligner.align for n_frames frames of one size with max_faces slots each, landmarks read from
 * device memory: slot j = f * max_faces + i reads its 5 x (x, y) floats at landmarks + j * stride
 * (stride >= 10; fr_detect_device's dets + 5 with stride 15 reads detection rows in place), and is
 * live when i < min(counts[f], max_faces) (counts: device int32 [n_frames], a negative count makes
 * none live; NULL: every slot is live).  One kernel fits every live slot (one lane each: the host
 * fit of fr_align_faces restated for the device, bitwise its doubles), one launch warps all slots.
 *   ok (device uint8 [slots]): 1 for a live slot whose fit succeeded.  Then out[j] (device uint8
 *     [slots][out_size][out_size][3]) and tforms[j] (device double [slots][2][3], or NULL) are
 *     bitwise fr_align_faces' for that frame and that face alone.
 *   Every other slot (not live, or a fit cv2 returns None for, which fr_align_faces refuses) has
 *     ok = 0, an all-zero crop and a NaN tform; no source pixel is read for it.
 * Any handle will do, finalised or not.  Allocates only when the call has more slots than any
 * before it.  FR_ERR_INVALID_ARGUMENT: NULL buffers, a side < 1, out_size outside [1, 1024],
 * stride < 10, n_frames * max_faces >= 2^31.  Zero slots is a no-op. */
int fr_align_device(fr_handle* h, const uint8_t* frames /* device [n_frames][height][width][3] */, int n_frames,
                    int height, int width, const float* landmarks /* device */, int stride,
                    const int32_t* counts /* device [n_frames] or NULL */, int max_faces, int out_size,
                    uint8_t* out, double* tforms, uint8_t* ok, void* stream);

/* ---- The same chain for images of different sizes (a folder of photographs): fr_detect_images and
 * fr_align_images with every output in device memory.  Like the three calls above they are
 * asynchronous on `stream`, synchronise nothing and stage nothing: images and sizes (host arrays,
 * as fr_detect_images takes them) are read before the call returns and never after, so the caller
 * may free or overwrite them at once.  The images themselves must stay alive until the stream
 * reaches the end of the call's work.  A chunk is kernel launches only (its first launch makes the
 * tables and zeroes the chunk's candidate counters), so after one warm-up call the chain with
 * fr_blur_scores_device and fr_quality_gate_device captures into a hipGraph and replays to the eager
 * results (the workspace rule above holds for them too). */

/* fr_detect_images with dets (device float [n][max_faces][15]) and counts (device int32 [n]) on the
 * device.  The chunk rule, the row-reduction rule and the argument checks are fr_detect_images'
 * (nothing runs when any image is refused; the message names the image); counts[i] and rows
 * k < min(counts[i], max_faces) are bitwise fr_detect_images' (the other rows are not written).  An
 * image with more than 4096 anchors above det_thresh gets counts[i] = -1 (its rows are unspecified);
 * the other images are unaffected.  Each image's resize tables and det_scale are made on the device
 * by one kernel per chunk (the host's arithmetic, bitwise) in an arena planned with the detector's
 * workspace; the per-image geometry travels in the kernel arguments.  Allocates nothing after the
 * handle's first detect call. */
int fr_detect_images_device(fr_handle* h, const uint8_t* const* images /* host [n] device pointers */,
                            const int32_t* sizes /* host [n][2] = height, width */, int n, float det_thresh,
                            int max_faces, float* dets /* device [n][max_faces][15] */,
                            int32_t* counts /* device [n] */, void* stream);

/* fr_align_device with a source per image: slot j = i * max_faces + k reads image i (images / sizes as
 * fr_align_images takes them, any side >= 1).  Liveness, ok, the zero crop and the NaN tform of a slot
 * that is not live or not fitted are fr_align_device's; for a live, fitted slot out[j] and tforms[j]
 * are bitwise fr_align_images' for that face.  No pixel of an image with counts[i] <= 0 is read (its
 * pointer must still be non-NULL).  The image descriptors travel in the fit kernel's arguments, 192
 * images per launch (a longer list takes several fit launches); the warp is one launch over all slots.
 * Any handle will do.  Allocates only when the call has more slots than any before it.
 * FR_ERR_INVALID_ARGUMENT: fr_align_device's, plus (with the image's index in the message) a NULL
 * image pointer or a side < 1; nothing runs then.  Zero slots is a no-op. */
int fr_align_images_device(fr_handle* h, const uint8_t* const* images, const int32_t* sizes, int n_images,
                           const float* landmarks /* device */, int stride,
                           const int32_t* counts /* device [n_images] or NULL */, int max_faces, int out_size,
                           uint8_t* out /* device [n_images * max_faces][S][S][3] */,
                           double* tforms /* device or NULL */, uint8_t* ok /* device */, void* stream);

/* fr_blur_scores with scores in device memory (double [n]): the same launches, no copy and no
 * synchronisation; the values are bitwise fr_blur_scores'. */
int fr_blur_scores_device(fr_handle* h, const uint8_t* crops, int n, int height, int width, int channels,
                          double* scores /* device [n] */, void* stream);

/* ---- The quality gate, the per-frame order and the packed face lists of
 * FaceProcessor.process_numpy on the device: the link between the chain above and the embedder /
 * the session kernels.  Asynchronous on `stream`, no synchronisation, no host read after return,
 * capturable; allocates (n_frames ints) only when n_frames exceeds any earlier call's; any handle
 * will do, finalised or not.
 *
 * Slot i of frame f (F = max_faces slots per frame) is live when i < min(counts[f], F); a negative
 * count makes none live, counts == NULL all.  A live slot goes through FaceQualityFilter.is_valid's
 * tests in is_valid's order and the first failing one is its stage; metrics the early exit never
 * computes are stored as 0.0:
 *   bbox       the C cast (truncation) of the row's four floats, d[:4].astype(np.int32); the floats
 *              must lie inside int32's range
 *   FR_GATE_DET_SCORE  (double)score < min_det_score
 *   FR_GATE_FACE_SIZE  (double)min(x1 - x0, y1 - y0) < min_face_size, on bbox's ints
 *   FR_GATE_POSE       compute_pose_angles in float32 operations, none contracted: dx, dy, the eye
 *              and mouth centres as the reference forms them, dist = sqrtf(dx*dx + dy*dy),
 *              ratio = clamp((nose_x - eye_cx) / dist, -1, 1) (a NaN stays),
 *              roll = (float)atan2((double)dy, (double)dx) * K,
 *              yaw = (float)asin((double)ratio) * K * 2.0f,
 *              pitch = ((nose_y - eye_cy) / (mouth_cy - eye_cy) - 0.5f) * 60.0f, K = 180.0f / (float)pi;
 *              fails when fabsf(angle) > (float)limit for any of the three (numpy 2 compares a
 *              float32 with a Python scalar in float32); a NaN angle passes, as on the host.
 *              Pitch is bitwise numpy's; yaw and roll are the correctly rounded float32 values up to
 *              the double library's error at a rounding boundary, where numpy's own float32
 *              functions are up to 4 ulp off and host-dependent (the device quality gate)
 *   FR_GATE_BLUR       only with cfg->check_blur and blur != NULL: blur_score is recorded, then
 *              blur < blur_threshold fails
 *   FR_GATE_FIT        passed every test, but ok[slot] == 0 (fr_align_device refused the fit)
 *   FR_GATE_VALID      otherwise.  A slot that is not live has stage FR_GATE_NOT_LIVE, rank -1, zeros.
 * metrics: det_score, blur_score, yaw, pitch, roll, the angles as the doubles of their float32 values.
 *
 * rank[i]: the position of the slot in process_numpy's stable sort(reverse=True) over the frame's
 * live slots: the number of live slots j with key_j > key_i, or key_j == key_i and j < i, with
 * key = (double)score * (blur_score where recorded, else 1000.0).  Keys must not be NaN.
 * frame_offsets: the exclusive prefix sum of the live counts, frame_offsets[n_frames] the total;
 * rows[frame_offsets[f] + rank] = f * F + i, entries from the total on are -1;
 * valid_slots: the slot indices f * F + i of stage FR_GATE_VALID in rows order, n_valid[0] their
 * number, the tail -1.
 *
 * FR_ERR_INVALID_ARGUMENT: a NULL required buffer or cfg, max_faces outside [1, FR_GATE_MAX_FACES],
 * n_frames < 0 or n_frames * max_faces >= 2^31, a limit that is not finite or lies beyond
 * +-FLT_MAX.  n_frames == 0 is a no-op (nothing is written). */
typedef struct {
  double min_det_score, min_face_size, max_yaw, max_pitch, max_roll, blur_threshold;
  int check_blur;
} fr_gate_config;
#define FR_GATE_MAX_FACES 1024 /* slots per frame */
#define FR_GATE_VALID 0
#define FR_GATE_DET_SCORE 1
#define FR_GATE_FACE_SIZE 2
#define FR_GATE_POSE 3
#define FR_GATE_BLUR 4
#define FR_GATE_FIT 5
#define FR_GATE_NOT_LIVE 255
int fr_quality_gate_device(fr_handle* h, const float* dets /* device [n][F][15], fr_detect_device's rows */,
                           const int32_t* counts /* device [n] or NULL */,
                           const uint8_t* ok /* device [n][F] (fr_align_device) or NULL */,
                           const double* blur /* device [n][F] (fr_blur_scores_device) or NULL */, int n_frames,
                           int max_faces, const fr_gate_config* cfg, uint8_t* stage /* device [n][F] */,
                           double* metrics /* device [n][F][5] */, int32_t* bbox /* device [n][F][4] */,
                           int32_t* rank /* device [n][F] */, int32_t* rows /* device [n*F] */,
                           int32_t* frame_offsets /* device [n+1] */, int32_t* valid_slots /* device [n*F] */,
                           int32_t* n_valid /* device [1] */, void* stream);

/* Conv arithmetic of this handle.  FR_PRECISION_F32 (default): exact f32 products and f32
 * accumulation on fp32 MFMA -- the parity path.  FR_PRECISION_BF16X3 (opt-in fast mode):
 * each f32 operand split into bf16 hi + lo, x.y ~= hi.hi + hi.lo + lo.hi on bf16 MFMA with f32
 * accumulation (per-product relative error ~2^-16; measured score drift in DESIGN.md). */
#define FR_PRECISION_F32 0
#define FR_PRECISION_BF16X3 1
int fr_set_precision(fr_handle* h, int mode);

/* Algorithm of the stride-1 3x3 convs (the bulk of the network's MACs).  All compute in f32.
 * FR_CONV_WINOGRAD4 (default): Winograd F(4x4,3x3) -- 36 f32-MFMA products per 4x4 tile
 * instead of 144, filters transformed once (on selection / at fr_finalize), pre-BN folded
 * into them; embeddings within 1e-5 of the CPU reference (tests).  FR_CONV_WINOGRAD:
 * F(2x2,3x3), 16 products per 2x2 tile instead of 36.  FR_CONV_DIRECT: the implicit-GEMM
 * kernel for every conv.  FR_PRECISION_BF16X3 runs the direct split-bf16 kernel. */
#define FR_CONV_DIRECT 0
#define FR_CONV_WINOGRAD 1
#define FR_CONV_WINOGRAD4 2
int fr_set_conv_algorithm(fr_handle* h, int algo);

/* hipGraph replay of small forwards.  With max_n > 0 (<= max_batch), every embed of n <= max_n
 * crops (fr_embed, fr_embed_host, fr_embed_match) runs its ~100 kernel launches as one captured
 * graph: the first call for an n runs eagerly and captures, later calls replay (same kernels and
 * arguments, so bit-identical results).  0 (default) disables; changing the precision, the conv
 * algorithm or the weights drops the captured graphs.  fr_graph_count reports how many exist. */
int fr_set_graph_batch(fr_handle* h, int max_n);

/* Lanes of a large forward.  With min_n > 0, a forward of n crops runs as
 * min(max_lanes, n / min_n) concurrent parts of near-equal size (n < 2 * min_n: one part;
 * max_lanes in [1, 4]): the first
 * part on the call's stream, the others on internal streams forked from it and joined back
 * before the call returns, each with its own activation and split-K workspace (allocated on first
 * use, ~1 GB per extra lane of 64 crops).  Launches alternate between the parts, so the last,
 * part-empty round of one part's layer runs beside another part's launch of the same layer.
 * Embeddings are those of separate forwards of the parts (batch-invariant to ~1e-6).
 * min_n 0 = one lane.  fr_create's default: FR_LANES_MIN_DEFAULT crops per lane, at most
 * FR_LANES_MAX_DEFAULT lanes (measured on MI355X, IR-101 C3: batch 256 as 2 x 128 +6%, as 3 or 4
 * parts -1..-2%; batch 128 as 2 x 64 +8%; batch 64 as 2 x 32 -6%).  Lane 1's workspace (~1.7 GB
 * at max_batch 256: 1.23 GB of activations for 128 crops, 0.27 GB of stream-K slabs, the
 * shortcut, split-K and head-partial buffers) is allocated by the first forward that uses it; if that allocation fails the
 * forward runs as one lane and lanes stay off until the next fr_set_lanes. */
#define FR_LANES_MIN_DEFAULT 64
#define FR_LANES_MAX_DEFAULT 2
int fr_set_lanes(fr_handle* h, int min_n, int max_lanes);
/* The lane setting in force: min_n is 0 after a failed lane-workspace allocation turned lanes off,
 * and fell_back is then 1 (until the next fr_set_lanes).  Any output pointer may be NULL. */
int fr_get_lanes(fr_handle* h, int* min_n, int* max_lanes, int* fell_back);
int fr_graph_count(fr_handle* h, int* count);

/* Per-kernel-class timing with HIP events on the call stream (bench roofline).
 * enable=1 starts recording; fr_profile_read synchronises and returns, since the
 * last read: summed milliseconds and algorithmic FLOPs of the conv launches (direct and
 * Winograd), their launch count, and the summed milliseconds of all launches. */
int fr_profile_enable(fr_handle* h, int enable);
int fr_profile_read(fr_handle* h, double* conv_ms, double* conv_flop, int64_t* conv_launches, double* total_ms);
/* Breakdown of the last fr_profile_read by kernel class: summed ms, algorithmic (direct-conv)
 * FLOPs, FLOPs the MFMA pipe executed (F(4x4,3x3), the default: 36 products per 4x4 canvas tile
 * instead of the direct conv's 144; F(2x2,3x3): 16 per 2x2 tile instead of 36) and launch count. */
#define FR_PROF_OTHER 0
#define FR_PROF_CONV_DIRECT 1
#define FR_PROF_CONV_WINOGRAD 2
int fr_profile_kernel(fr_handle* h, int kind, double* ms, double* flop, double* exec_flop, int64_t* launches);

/* Last error message of this handle (or of the last failed fr_create if h is NULL). */
const char* fr_last_error(fr_handle* h);
/* Library build/version string; it ends in "build <id>", the content hash of every source and
 * flag the library was built from (build.py build_id), which profiles are stamped with. */
const char* fr_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FRHIP_H_ */
