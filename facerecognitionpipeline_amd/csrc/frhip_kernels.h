// Internal kernel launch interface for libfrhip (not part of the public C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace frhip {

// Epilogue of the implicit-GEMM conv kernel.
enum Epi : int {
  EPI_AFFINE = 0,        // y = acc*scale + shift                      (shortcut conv1x1 + BN)
  EPI_AFFINE_PRELU = 1,  // y = prelu(acc*scale + shift)               (conv1 + BN + PReLU)
  EPI_AFFINE_RES = 2,    // y = acc*scale + shift + res[m]             (conv2 + BN + identity / conv shortcut)
  EPI_AFFINE_RES_SUB = 3,// y = acc*scale + shift + res[b, 2oy, 2ox]   (conv2 + BN + MaxPool2d(1,2) shortcut)
  EPI_RAW = 4,           // y[split] = acc                             (split-K partial / gallery scores)
  EPI_AFFINE_RES_PRELU = 5,  // y = prelu(acc*scale + shift + res[m])  (detector BasicBlock conv2 + BN + add + ReLU)
};

// One convolution (or GEMM, as a 1x1 conv over a 1x1 image) in NHWC f32.
//   x   [B][H][W][Cin]         w [Cout][KH][KW][Cin]        y [B][Ho][Wo][Cout]
// pre_scale/pre_shift: per-Cin affine applied to in-bounds input taps only (the
// pre-activation BatchNorm in front of a zero-padded conv), may be null.
struct ConvParams {
  const float* x;
  const float* w;
  float* y;
  const float* pre_scale;
  const float* pre_shift;
  const float* post_scale;
  const float* post_shift;
  const float* prelu;
  const float* res;
  int B, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad;
  int res_H, res_W;
  int M;                 // B*Ho*Wo
  int steps_total;       // KH*KW*Cin / 32
  int steps_per_split;   // K-steps per blockIdx.y slice
  long long split_stride;// elements between split-K partial slabs
  int mtiles, ntiles;
  // stream-K schedule (sk_cus > 0): persistent grid of sk_cus x blocks-per-CU blocks.
  int sk_cus;            // input: CUs to fill (0 = grid mode)
  int sk_blocks;         // set by the launcher: persistent grid size P
  int sk_dp_tiles;       // set by the launcher: tiles done whole, round-robin
  float* sk_ws;          // [P][2][BM*BN] partial-accumulator slabs
  long long sk_ws_floats;
  int* sk_cnt;           // per stream-K tile arrival counters, zero at allocation
  int sk_cnt_cap;
  // fused 1x1 shortcut (Cin2 > 0): K-steps [steps1, steps_total) read x2 [B][H][W][Cin2] at the
  // output's stride and no padding, 32 channels per step, against weight columns
  // KH*KW*Cin .. + Cin2 (w rows are KH*KW*Cin + Cin2 long): conv2 and the block's conv
  // shortcut as one GEMM (both BN scales folded into the weights, the shifts into post_shift)
  const float* x2;
  int Cin2, steps1;
  // serving conv kernel only (conv_small.hip): also y2 = y * y2_scale[c] + y2_shift[c] (the next
  // block's pre-activation BN, applied once here instead of per tap in its conv1); null: none
  float* y2;
  const float* y2_scale;
  const float* y2_shift;
  // serving conv kernel only: which activations are channel-blocked [B][C/16][H][W][16] instead
  // of NHWC (CONVS_BLK_* bits; y2 follows y)
  int blk;
};
constexpr int CONVS_BLK_X = 1, CONVS_BLK_X2 = 2, CONVS_BLK_RES = 4, CONVS_BLK_Y = 8;

// Tile family of a conv launch.
enum ConvTile : int {
  TILE_256x64 = 0,
  TILE_128x128 = 1,
  TILE_128x64 = 2,
  TILE_64x128 = 3,
  TILE_256x128 = 4,
  TILE_128x256 = 5,
  TILE_128x128_W8 = 6,  // 8 waves (512 threads)
  TILE_256x128_W8 = 7,
  TILE_128x64_W8 = 8,
  TILE_64x256_W8 = 9,
  TILE_256x64_W8 = 10,
  TILE_COUNT = 11
};

// Arithmetic of the conv GEMM: exact-f32 MFMA (default, the parity path) or the opt-in
// split-bf16 "bf16x3" (x = hi + lo, x.y ~= hi.hi + hi.lo + lo.hi, f32 accumulation).
enum Precision : int { PREC_F32 = 0, PREC_BF16X3 = 1 };

// y = epilogue(sum of S raw split-K slabs part[s][M][Cout], in split order) for EPI_AFFINE,
// EPI_AFFINE_RES and EPI_AFFINE_RES_SUB (conv_mfma.hip; serving-sized direct convs)
hipError_t launch_conv_split_fixup(const ConvParams& p, Epi epi, const float* part, int S, long long stride,
                                   hipStream_t s);
hipError_t launch_conv(const ConvParams& p, ConvTile tile, bool pre, Epi epi, int nsplit, hipStream_t s,
                       Precision prec = PREC_F32);
int conv_tile_bm(ConvTile t);
int conv_tile_bn(ConvTile t);

// Winograd F(2x2,3x3) stride-1 pad-1 conv in f32 (conv_winograd.hip), NHWC like ConvParams.
//   u: transformed filters from launch_wino_weights (wino_weight_floats(Cout, Cin) floats).
// Epilogues: EPI_AFFINE_PRELU (with pre-BN) and EPI_AFFINE_RES (without).
struct WinoParams {
  const float* x;
  const float* u;
  float* y;
  const float* pre_scale;
  const float* pre_shift;
  const float* post_scale;
  const float* post_shift;
  const float* prelu;
  const float* res;  // same shape as y
  int B, H, W, Cin, Cout;
  int TH, TW, ntiles, mblocks, nblocks;  // set by launch_wino
};
bool wino_supported(int Cin, int Cout, int kh, int kw, int stride, int pad);
size_t wino_weight_floats(int Cout, int Cin);
// w: [Cout][3][3][Cin] f32 (device) -> u (device), fragment-ordered G g G^T.
hipError_t launch_wino_weights(const float* w, float* u, int Cout, int Cin, hipStream_t s);
hipError_t launch_wino(const WinoParams& p, bool pre, Epi epi, hipStream_t s);

// Winograd F(4x4,3x3) stride-1 pad-1 conv in f32 (conv_winograd4.hip), NHWC like ConvParams:
// one fused persistent kernel (transform waves -> LDS ring -> 16x16x4 MFMA waves with the
// output transform and the epilogue lane-local).  u: launch_wino4_weights output
// (wino4_weight_floats(Cout, Cin) floats).  Tiles are cut from a canvas of the batch (period
// Pr x Pc per image, NC images per canvas row, one zero separator row/column when 4 does not
// divide H/W).
struct Wino4Params {
  const float* x;
  const float* u;
  float* y;
  // pre-activation BN folded into the filters: U built from w * scale (launch_wino4_weights),
  // and t = shift / scale per input channel added to the in-image input pixels
  const float* pre_t;
  const float* post_scale;
  const float* post_shift;
  const float* prelu;
  const float* res;   // same shape as y
  int B, H, W, Cin, Cout;
  int Pr, Pc, NC, TWc, ntiles, mblocks, nblocks;  // set by launch_wino4 (wino4_canvas)
  int nbg;  // tile blocks per XCD group of items (set by launch_wino4)
  // split-K workspace (optional): compact raw partial outputs, one 16-tile x 16-pixel
  // x 64-cout slot (64 KiB) per item part; launch_wino4 splits the K loop of a small grid's items
  // when part_floats holds the slots
  float* part;
  long long part_floats;
  int ksplit, ks_per;      // set by launch_wino4
  int item0, nitem;        // set by launch_wino4: the launch's range of the layer's item order
  int no_split;  // 1: never split-K (tests compare the two schedules)
  int max_split;  // > 0: at most this many K parts per item in a split-K launch (serving sweeps)
  // ring hand-off guard: a wave that has polled its LDS counters poll_max times without seeing
  // the step it waits for stores FR_DEVERR_W4_HANDOFF into *err (a host-pinned word the
  // runtime reads at its sync points; nullable) and carries on, so a lost hand-off ends the
  // launch instead of hanging the GPU and is reported instead of passing as a result.
  // poll_max 0 means the default (WINO4_POLL_DEFAULT), < 0 no polls at all (tests).
  int* err;
  int poll_max;
  // layouts (W4_BLK_* bits): which of x, res, y are channel-blocked [B][C/16][H][W][16] instead of
  // NHWC (the same per-element arithmetic either way: outputs are bitwise the NHWC launch's)
  int blk;
  int nbg_override;  // > 0: tile blocks per XCD item group instead of the rule (A/B only)
  // item shapes of whole-item launches without pre-BN: 1 = a layer of 65..96 output channels runs
  // items of 16 tiles x 96 couts (wino4w_kernel), one of at most 32 channels items of 32 tiles x 32
  // couts (wino4t_kernel), when its 64-cout items take more than one round of workgroups; 2 = at
  // every grid size (tests); 0 = 64-cout items only
  int shapes;
};
constexpr int W4_BLK_X = 1, W4_BLK_RES = 2, W4_BLK_Y = 4;
constexpr int WINO4_POLL_DEFAULT = 1 << 16;
constexpr int FR_DEVERR_W4_HANDOFF = 1;
bool wino4_supported(int Cin, int Cout, int kh, int kw, int stride, int pad);  // Cin % 16, Cout % 16

// Serving-batch 3x3 convs (conv_small.hip): pad 1, stride 1 or 2, optional fused shortcut
// (Cin2 / x2, weight rows 9*Cin + Cin2), one workgroup per 16 pixels x 16 couts with the whole K
// reduction inside it (no split-K, no fixup).  pre: pre-BN + EPI_AFFINE_PRELU (conv1); else
// EPI_AFFINE / EPI_AFFINE_PRELU / EPI_AFFINE_RES / EPI_AFFINE_RES_SUB.  Reads p.x, w, y, pre_*,
// post_*, prelu, res, res_H/W, B, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, M, x2, Cin2, y2*.
// p.w is in fragment order (launch_convs_weights), not [Cout][9 Cin + Cin2].
bool convs_supported(const ConvParams& p, bool pre, Epi epi);
hipError_t launch_convs(const ConvParams& p, bool pre, Epi epi, hipStream_t s);
// w [Cout][KR] (KR = 9 Cin + Cin2, both % 16 == 0) -> wf, Cout * KR floats in fragment order:
// per 16-cout block cb and 16-wide K chunk kc, the 1 KiB one load instruction of a wave reads
// (lane l: couts cb * 16 + (l & 15), K kc * 16 + 4 (l >> 4) .. + 3).
hipError_t launch_convs_weights(const float* w, float* wf, int Cout, int KR, hipStream_t s);

// Stride-2 3x3 conv, 64 -> 64 channels, + BN + MaxPool2d(1,2) shortcut (conv_s2.hip): the first
// block of the AdaFace stage 1.  y[b][oy][ox] = conv(x)*scale + shift + res[b][2oy][2ox], NHWC f32;
// w [64][3][3][64]; res has x's shape.
struct S2Params {
  const float* x;
  const float* w;
  const float* post_scale;
  const float* post_shift;
  const float* res;
  float* y;
  int B, H, W;  // input
  int Ho, Wo;   // set by launch_s2c64
};
bool s2c64_supported(int Cin, int Cout, int kh, int kw, int stride, int pad, int H, int W);
hipError_t launch_s2c64(const S2Params& p, hipStream_t s);
size_t wino4_weight_floats(int Cout, int Cin);
void wino4_canvas(Wino4Params& p);
// w: [Cout][3][3][Cin] -> u = G (w * pre_scale[cin]) G^T in fragment order (pre_scale nullable)
hipError_t launch_wino4_weights(const float* w, const float* pre_scale, float* u, int Cout, int Cin, hipStream_t s);
hipError_t launch_wino4(const Wino4Params& p, bool pre, Epi epi, hipStream_t s);

// uint8 RGB HWC 112x112 -> (BGR, LUT normalise) -> conv3x3 3->64 -> BN -> PReLU, NHWC f32.
hipError_t launch_stem(const uint8_t* img, int B, const float* lut, const float* w27x64,
                       const float* bn_scale, const float* bn_shift, const float* prelu,
                       float* y, hipStream_t s);

// Sum split-K partials + FC bias -> BN1d(affine=False) -> x/||x|| -> optional e/(||e||+1e-8).
hipError_t launch_head_reduce(const float* partial, int nsplit, long long split_stride,
                              const float* fc_bias, const float* bn_scale, const float* bn_shift,
                              float* emb, int n, int normalize, int model_l2, hipStream_t s);

// q / (||q|| + 1e-8) row-wise over D=512 rows.
hipError_t launch_l2norm_rows(const float* q, float* out, int n, int d, hipStream_t s);
// serving-sized match scores (n <= 16 queries, D = 512): q / (||q|| + 1e-8) as l2norm_rows computes
// it, fused with the scores against the G x 512 gallery rows: scores [n][G]
hipError_t launch_scores_small(const float* q, const float* gallery, int G, float* scores, int n, hipStream_t s);

// Per row of a [n][G] score matrix: top-k by (score desc, index desc), k in [1, G]; with
// low_index_first by (score desc, index asc), the order of fr_match_identities.
hipError_t launch_topk(const float* scores, int n, int G, int k, int32_t* idx, float* val, hipStream_t s,
                       bool low_index_first = false);

// warpAffine INTER_LINEAR / BORDER_CONSTANT 0 of n crops from one uint8 RGB frame;
// minv: device [n][6] inverse maps (double), out: [n][S][S][3].
hipError_t launch_warp_affine(const uint8_t* frame, int H, int W, const double* minv, int n, int S, uint8_t* out,
                              hipStream_t s);
// The same with up to WARP_MAPS_BY_VALUE host maps passed by value in the kernel arguments
// (2.3 KB of the 4 KB limit): nothing to copy, so nothing for the caller to wait on.
constexpr int WARP_MAPS_BY_VALUE = 48;
struct WarpMaps {
  double m[WARP_MAPS_BY_VALUE][6];
};
hipError_t launch_warp_affine_by_value(const uint8_t* frame, int H, int W, const double* host_minv, int n, int S,
                                       uint8_t* out, hipStream_t s);

// The same for n faces of different frames, in one launch for any n: face f warps its own frame by
// its own inverse map; faces: device [n]; out: [n][S][S][3], S <= 4096.
struct WarpFace {
  const uint8_t* src;  // device uint8 [H][W][3]
  int H, W;
  double minv[6];
};
hipError_t launch_warp_affine_images(const WarpFace* faces, int n, int S, uint8_t* out, hipStream_t s);

// The similarity fit of fr_align_faces on the device (align_fit.hip), one lane per slot.
// update_num_iters' logarithms for 5 points and confidence 0.99 (align_host.cpp fit_logs).
struct FitLogs {
  double log_num;     // log(max(1 - p, DBL_MIN))
  double log_den[6];  // log(1 - q * q), q = 1 - (5 - g) / 5, per inlier count g
  int den_zero;       // bit g: 1 - q * q < DBL_MIN (update_num_iters returns 0)
};
struct FitSlots {
  const uint8_t* frames;   // device uint8 [n_frames][H][W][3], or NULL with faces == NULL
  int n_frames, H, W;
  const float* landmarks;  // device: slot j's 5 x (x, y) at landmarks + j * stride
  int stride;
  const int* counts;       // device [n_frames]: slots i < min(counts[f], max_faces) of frame f are live; NULL: all
  int max_faces;           // slots per frame
  float tmpl[10];          // reference_template(out_size)
  FitLogs logs;
  double* tforms;          // device [slots][6] forward maps (NaN for a slot that is not ok), or NULL
  uint8_t* ok;             // device [slots]: 1 = live and fitted
  WarpFace* faces;         // device [slots] descriptors for launch_warp_affine_images, or NULL
};
// Slot (f, i): fit_similarity(landmarks, tmpl, 5) bitwise as the host computes it; ok, the forward map
// and the slot's WarpFace (frame f, H, W, invert_affine of the map).  A slot that is not live or whose
// fit fails gets ok = 0, a NaN map and a descriptor of an empty (0 x 0) source: the warp writes
// zeros and reads nothing.  n_frames * max_faces < 2^31.
hipError_t launch_fit_similarity(const FitSlots& p, hipStream_t s);
// The ragged form (fr_align_images_device): frame f is an image of its own size at its own address.
// The descriptors travel by value, at most FIT_IMAGES_BY_VALUE per launch: with FitSlots that is
// 3.3 KB of the 4 KB argument limit (a launch's hidden arguments take a few hundred bytes more); a
// longer list takes several launches (frhip_runtime.cpp).  The one-size launch keeps FitSlots alone.
struct FitImage {
  const uint8_t* src;  // device uint8 [H][W][3]
  int H, W;
};
constexpr int FIT_IMAGES_BY_VALUE = 192;
struct FitImageSlots {
  FitSlots s;  // frames, H and W are not read; n_frames = the images of this launch (<= FIT_IMAGES_BY_VALUE)
  FitImage images[FIT_IMAGES_BY_VALUE];  // frame f is images[f] (entries >= s.n_frames are not read)
};
static_assert(sizeof(FitImage) == 16 && sizeof(FitImageSlots) <= 3328, "FitImageSlots fits the kernel arguments");
hipError_t launch_fit_similarity_images(const FitImageSlots& p, hipStream_t s);

// Laplacian variance (numpy's summation order) of the gray image of n uint8 images [n][H][W][C]
// (C = 3 / 4: RGB(A) -> gray; C = 1: gray) -> var[n] (double).  Images whose gray copy and
// summation trees fit BLUR_LDS_MAX bytes of LDS take one block each; larger ones take three
// launches over (chunk, image) blocks and blur_workspace_bytes(n, H, W) of device workspace ws.
// BLUR_LDS_MAX is a gfx950 workgroup's whole LDS and blur_lds_bytes all that blur_kernel uses (it
// has no static LDS): at most 106,576 pixels take the one-block form.
constexpr size_t BLUR_LDS_MAX = 160 * 1024;
size_t blur_lds_bytes(int H, int W);
size_t blur_workspace_bytes(int n, int H, int W);
hipError_t launch_blur(const uint8_t* crops, int n, int H, int W, int C, double* var, void* ws, hipStream_t s);

// Enrollment augmentation (augment.hip): A <= AUG_VARIANTS variants of each of n uint8 crops
// [n][H][W][3] -> out [n][A][H][W][3] (1 <= H, W <= 8192; out must not overlap crops).  The
// host-built tables travel by value in the kernel arguments (1.2 KB), so the launch needs no copy
// and nothing for the caller to wait on.
constexpr int AUG_VARIANTS = 14;
struct AugTables {
  double minv[4][6];    // inverse maps of the rotations by -10, -5, 5, 10 degrees (variants 2..5)
  uint8_t lut[4][256];  // contrast 0.85, 0.92, 1.08, 1.15 of every byte value (variants 10..13)
};
hipError_t launch_augment(const uint8_t* crops, int n, int H, int W, int A, const AugTables& tab, uint8_t* out,
                          hipStream_t s);

// Gallery templates (GalleryManager._aggregate_embeddings) for n_students CSR slices of
// emb [total][512]; offsets: device [n_students + 1]; out: [n_students][512]; kept: [n] or NULL.
constexpr int TEMPLATE_MAX_SAMPLES = 1024;
enum TemplateMethod : int { TEMPLATE_MEAN = 0, TEMPLATE_MEDIAN = 1, TEMPLATE_WEIGHTED_MEAN = 2 };
hipError_t launch_templates(const float* emb, const int* offsets, int n_students, int method, float min_sim,
                            float* out, int* kept, hipStream_t s);

// Track consensus (track.hip: FaceMatcher._aggregate_matches / _get_best_candidate) of n_tracks CSR
// slices of the top-k output idx / score [total][k] (column 0 is read); offsets: device
// [n_tracks + 1], 1..TRACK_MAX_FRAMES frames each; out_i: [n_tracks][8] = status, winner row,
// winner count, pool size, second count, frames, quality frames, 0; out_d: [n_tracks][2] =
// confidence, ratio.
constexpr int TRACK_MAX_FRAMES = 1024;
enum TrackStatus : int {
  TRACK_RECOGNIZED = 0,
  TRACK_FEW_FRAMES = 1,
  TRACK_NO_CONSENSUS = 2,
  TRACK_BELOW_THRESHOLD = 3
};
hipError_t launch_track_consensus(const int* idx, const float* score, int k, const int* offsets, int n_tracks,
                                  double min_quality, int min_frames, double similarity_threshold, int* out_i,
                                  double* out_d, hipStream_t s);

// Photograph roll call (rollcall.hip: FaceMatcher.match_single_image's decision, and its exclusive
// form) of n_images CSR slices of the top-k output idx / score [total][k]; offsets: device
// [n_images + 1], 0..ROLLCALL_MAX_FACES faces each; out_face: [total][4] = status, row, column, 0;
// out_score: [total] = the reported score; out_image: [n_images][4] = faces, recognized, candidates,
// displaced.
constexpr int ROLLCALL_MAX_FACES = 1024;
enum RollcallMode : int { ROLLCALL_INDEPENDENT = 0, ROLLCALL_EXCLUSIVE = 1 };
enum FaceStatus : int { FACE_RECOGNIZED = 0, FACE_CANDIDATE = 1, FACE_DISPLACED = 2 };
hipError_t launch_photo_rollcall(const int* idx, const float* score, int k, const int* offsets, int n_images,
                                 double similarity_threshold, int mode, int* out_face, float* out_score,
                                 int* out_image, hipStream_t s);

// Capture sessions (capture.hip: SimpleTracker.update + FrameAccumulator) of n_clips CSR slices: clip c
// = frames [clip_off[c], clip_off[c+1]), frame f = detections [frame_off[f], frame_off[f+1]) of bbox
// [total][4] / metrics [total][5] / valid [total]; both offset arrays on the device, at most
// CAPTURE_MAX_FACES detections per frame and CAPTURE_MAX_DETS per clip.  q_limit: the smallest 4 x
// squared centroid distance that is no match.  track_id / quality / slot: [total]; clip_info:
// [n_clips][4] = tracks opened, tracks completed, frames saved, CAPTURE_ERR_* (0: none).
constexpr int CAPTURE_MAX_FACES = 128;
constexpr int CAPTURE_MAX_TRACKS = 128;
constexpr int CAPTURE_MAX_DETS = 4096;
constexpr int CAPTURE_MAX_TARGET = 64;
constexpr int CAPTURE_COORD_MAX = 1 << 20;
enum CaptureError : int { CAPTURE_ERR_TRACKS = 1, CAPTURE_ERR_COORD = 2 };
hipError_t launch_capture_tracks(const int* bbox, const double* metrics, const unsigned char* valid,
                                 const int* frame_off, const int* clip_off, int n_clips, int max_disappeared,
                                 long long q_limit, int target_frames, double min_quality_score, int save_partial,
                                 int* track_id, double* quality, int* slot, int* clip_info, hipStream_t s);

// Live sessions (live.hip: LiveFaceRecognition._simple_track_assignment + LiveRecognitionTracker) of
// n_clips CSR slices laid out as launch_capture_tracks takes them, at most LIVE_MAX_FACES detections
// per frame and any number per clip; metrics [total][2] = det_score, blur_score.  q_limit as above.
// track_id (from 0) / prev / attempt / best: [total], -1 for none, prev and best global detection
// indices; clip_info: [n_clips][4] = tracks opened, candidates, frames, LIVE_ERR_* (0: none).
constexpr int LIVE_MAX_FACES = 128;
constexpr int LIVE_MAX_ATTEMPTS = 16;
constexpr int LIVE_MAX_BUFFER = 64;
enum LiveError : int { LIVE_ERR_COORD = 2 };  // CAPTURE_ERR_COORD's value: the same limit
hipError_t launch_live_tracks(const int* bbox, const double* metrics, const int* frame_off, const int* clip_off,
                              int n_clips, long long q_limit, int recognition_interval, int max_attempts,
                              int buffer_size, int* track_id, int* prev, int* attempt, int* best, int* clip_info,
                              hipStream_t s);

// Server sessions (server.hip: the server's LiveRecognitionTracker) of n_tracks CSR slices of `order`
// [track_off[n_tracks]], detection indices into metrics [n_dets][2] = det_score, blur_score and clock
// [n_dets] (seconds), a track's appearances in arrival order; track_off on the device.  attempt
// (ordinal among the track's attempts) / best (detection index) / state (SERVER_*): [n_dets], -1 for
// none; track_info: [n_tracks][4] = attempts, cooldowns set, resets, SERVER_ERR_* (0: none).
constexpr int SERVER_MAX_ATTEMPTS = 16;
constexpr int SERVER_MAX_BUFFER = 64;
enum ServerState : int {
  SERVER_GATED = 0, SERVER_ATTEMPT = 1, SERVER_COOLDOWN = 2, SERVER_COOLDOWN_SET = 3, SERVER_RESET = 4
};
enum ServerError : int { SERVER_ERR_VALUE = 1, SERVER_ERR_ORDER = 2 };  // a bit each
hipError_t launch_server_tracks(const double* metrics, const double* clock, const int* order, const int* track_off,
                                int n_tracks, int n_dets, int max_attempts, int buffer_size, double retry_cooldown,
                                double det_gate, int* attempt, int* best, int* state, int* track_info,
                                hipStream_t s);

// Model evaluation (evaluate.hip: the notebook's cosine_similarity / aggregate_* / identify_probe /
// compute_rank_metrics and the threshold loops of evaluate_*_comprehensive).
constexpr int EVAL_MAX_ROWS = 1024;      // gallery rows of one identity
constexpr int EVAL_MAX_K = 16;           // top-k mean
constexpr int EVAL_MAX_THRESHOLDS = 256;
constexpr int EVAL_TILE_ROWS = 4096;     // gallery rows one workgroup stages in LDS
constexpr int EVAL_TILE_IDS = 1024;      // identities one workgroup owns
enum EvalAgg : int { AGG_MAX = 0, AGG_MEAN = 1, AGG_TOPK = 2 };
// norm[r] = (float)sqrt(double sum of squares) of n rows of x [n][512]; *any_off |= 1 when a row has
// |norm - 1| >= 0.01 (any_off may be NULL).
hipError_t launch_row_norms(const float* x, int n, float* norm, int* any_off, hipStream_t s);
// out[p][i] = aggregation of sim[p][offsets[i] .. offsets[i+1]) for n probes, after the 0.01 rule is
// applied to every sim element (written back when write_sim).  offsets: device [n_ids + 1];
// tiles: device [n_tiles + 1] first identities of runs of <= EVAL_TILE_IDS identities and
// <= EVAL_TILE_ROWS rows (fr_identity_scores builds them); qnorm [n], enorm [G], e_any_off as launch_row_norms
// wrote them.  sim [n][G] with n * G * 4 < 2 GiB.
hipError_t launch_identity_agg(float* sim, int n, int G, const int* offsets, int n_ids, const int* tiles, int n_tiles,
                               const float* qnorm, const float* enorm, const int* e_any_off, int aggregation, int k,
                               bool write_sim, float* out, hipStream_t s);
// Records and threshold counts of n probes over scores [n][n_ids] (frhip.h: fr_eval_probes); thr:
// device [n_thr] doubles; counts must be zero at launch.
hipError_t launch_eval_probes(const float* scores, int n, int n_ids, const int* true_id, const double* thr, int n_thr,
                              int* rec_i, float* rec_f, long long* counts, hipStream_t s);

// Identity matching (identify.hip: fr_match_identities' serving-sized path).  out[p][i] = the
// aggregation of cosine_similarity(Q[p], E[r]) over identity i's rows r in [offsets[i], offsets[i+1]),
// for n queries in one launch: what launch_identity_agg gives on the raw dots of Q and E, without
// the [n][G] matrix.  enorm [G] / e_any_off as launch_row_norms wrote them for E; offsets: device
// [n_ids + 1]; tiles: device [n_tiles + 1] first identities of runs of whole identities of
// <= EVAL_MAX_ROWS rows (fr_samples_set cuts them at IDENT_TILE_ROWS rows, a longer identity alone).
// Every query reads every row, so the launch costs n * G row reads.
// fr_match_identities takes this kernel for one query, and for n <= IDENT_SMALL_N queries against G
// rows with n * G <= IDENT_QUERY_ROWS; the composed path otherwise (all three measured)
constexpr int IDENT_TILE_ROWS = 64;  // gallery rows of a serving tile
constexpr int IDENT_SMALL_N = 16;
constexpr long long IDENT_QUERY_ROWS = 65536;
hipError_t launch_match_small(const float* Q, int n, const float* E, const float* enorm, const int* e_any_off,
                              const int* offsets, int n_ids, const int* tiles, int n_tiles, int aggregation, int k,
                              float* out, hipStream_t s);

// ---- SCRFD detector glue (detect.hip)
constexpr int DET_MAX_CANDIDATES = 4096;  // per frame, above det_thresh, before NMS

struct DetDecodeParams {
  const float* head[3];  // per level [B][hw][32]
  int hw[3], w[3], stride[3], anchor_base[3];
  float thresh, det_scale;
  const float* det_scales;  // device [B] per-frame scales (fr_detect_images), or NULL: det_scale for all
  int cap;
  int* count;   // [B] candidates found (may exceed cap)
  float* cand;  // [B][cap][16]: score, anchor (int bits), x1 y1 x2 y2, 5 x (x, y)
};

// cv2.resize INTER_LINEAR (fixed point) of n frames into the top-left new_w x new_h of
// zero dw x dh canvases; xtab/ytab: device [new_w|new_h][4] = (src0, src1, w0, w1).
hipError_t launch_letterbox(const uint8_t* frames, int n, int H, int W, const int* xtab, const int* ytab, int new_w,
                            int new_h, int simd_end, int dw, int dh, uint8_t* out, hipStream_t s);
// The same for n images of different sizes (n <= 65535), each with its own geometry: imgs: device
// [n]; tabs: device ints, image f's tables at tabs + xtab ([new_w][4]) and tabs + ytab ([new_h][4]).
struct LetterboxImage {
  const uint8_t* src;  // device uint8 [H][W][3]; the tables hold every row index, so H itself is not needed
  int W, new_w, new_h, simd_end;
  int xtab, ytab;  // offsets into tabs, in ints
};
hipError_t launch_letterbox_images(const LetterboxImage* imgs, const int* tabs, int n, int dw, int dh, uint8_t* out,
                                   hipStream_t s);
// The same with the descriptors by value in the kernel arguments: a chunk of at most
// LETTERBOX_BY_VALUE images (the detector's largest max_frames; 2.5 KB of the 4 KB argument limit),
// each with its source height and its det_scale.  Nothing is staged, so nothing has to be waited for.
constexpr int LETTERBOX_BY_VALUE = 64;
struct LetterboxChunk {
  LetterboxImage im[LETTERBOX_BY_VALUE];
  int H[LETTERBOX_BY_VALUE];        // source heights (the y tables' ssize)
  float scale[LETTERBOX_BY_VALUE];  // det_scale = new_h / H as float
};
static_assert(sizeof(LetterboxImage) == 32 && sizeof(LetterboxChunk) <= 3072, "a chunk fits the kernel arguments");
hipError_t launch_letterbox_images_by_value(const LetterboxChunk& c, const int* tabs, int n, int dw, int dh,
                                            uint8_t* out, hipStream_t s);
// The chunk's resize tables made on the device (resize_table.h's arithmetic: bitwise
// resize_axis_table's): image f's x table ([new_w][4], ssize W) at tabs + xtab, its y table
// ([new_h][4], ssize H[f]) at tabs + ytab, scale[f] into scales[f] and 0 into raw[f] (decode_kernel's
// count of the image; scales and raw may be NULL).  tabs:
// device, 16-byte aligned, tabs_ints ints; an offset that is negative, not a multiple of 4 or whose
// table ends beyond tabs_ints is refused before anything is launched.
hipError_t launch_resize_tables(const LetterboxChunk& c, int n, int* tabs, long long tabs_ints, float* scales,
                                int* raw, hipStream_t s);
// cv2.resize INTER_LINEAR of n images of different sizes (n <= 65535) to 112 x 112 x 3 each (out:
// [n][112][112][3], 4-byte aligned): image f's tables at tabs + xtab / ytab ([112][4] each).
struct CropImage {
  const uint8_t* src;  // device uint8 [H][W][3]
  int W;
  int xtab, ytab;  // offsets into tabs, in ints
  int copy;        // the image is 112 x 112 at a 4-byte aligned address: copied, its tables unused
};
hipError_t launch_resize_images(const CropImage* imgs, const int* tabs, int n, int simd_end, uint8_t* out,
                                hipStream_t s);
// (x - 127.5)/128 -> conv3x3 s2 p1 3->C (C % 8 == 0, <= 32; weights [27][C]) -> BN -> ReLU, NHWC.
// force_scalar: det_stem_kernel also where the MFMA kernel would run (tests compare the two).
hipError_t launch_det_stem(const uint8_t* img, int n, int H, int W, int C, const float* w27xC, const float* scale,
                           const float* shift, float* y, hipStream_t s, bool force_scalar = false);
hipError_t launch_maxpool3(const float* x, int B, int H, int W, int C, float* y, hipStream_t s);
hipError_t launch_upsample_add(float* big, const float* small, int B, int h, int w, int C, hipStream_t s);
// AvgPool2d(2, 2), NHWC, even H and W, C % 4 == 0.
hipError_t launch_avgpool2(const float* x, int B, int H, int W, int C, float* y, hipStream_t s);
// [B][Hs][W][C] -> [B][Hd][W][C]: rows [m, m + Hd - Hs) are copies of src row m (C % 4 == 0).
hipError_t launch_row_expand(const float* x, int B, int Hs, int W, int C, int m, int Hd, float* y, hipStream_t s);
hipError_t launch_decode(const DetDecodeParams& p, int n, hipStream_t s);
hipError_t launch_nms(const float* cand, const int* count, int n, int cap, float iou_thresh, int max_out, float* out,
                      int* out_count, hipStream_t s);
// counts[f] = -1 for every frame f < n with raw[f] > cap (more candidates than decode kept).
hipError_t launch_det_overflow(const int* raw, int n, int cap, int* counts, hipStream_t s);

}  // namespace frhip
