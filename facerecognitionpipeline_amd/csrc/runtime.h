// Internals shared by the libfrhip runtime translation units: the handle, folded-parameter types
// and the launch helpers.
//   frhip_runtime.cpp  the public fr_* C API (include/frhip.h): model, gallery rows, match, align,
//                      detect, settings, profiling
//   batch_ops.cpp      the fr_* calls over CSR batches: templates, track consensus, capture
//                      and live sessions, identity scores, probe evaluation, the sample gallery
//                      and identity matching
//   finalize.cpp       handle and entry-point helpers, state-dict schema, BatchNorm folding, arenas,
//                      workspace
//   conv_dispatch.cpp  run_conv and its kernel-selection rules
//   embed_forward.cpp  lanes, the layout plan, the IR forward, graphs, resize, gallery match
//   align_host.cpp     cv2.estimateAffinePartial2D and the augmentation tables (host only)
//   detector.cpp       the SCRFD detector
//   frhip_testing.cpp  the frt_* test entry points (include/frhip_testing.h)
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <initializer_list>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/frhip.h"
#include "frhip_kernels.h"

namespace frhip_rt {

struct BlockSpec {
  int cin, depth, stride;
};

// Device-side folded parameters of one conv.
struct ConvW {
  float* w = nullptr;  // [Cout][KH][KW][Cin]
  float* pre_scale = nullptr;
  float* pre_shift = nullptr;
  float* post_scale = nullptr;
  float* post_shift = nullptr;
  float* prelu = nullptr;
  float* wino = nullptr;  // Winograd-transformed filters (stride-1 3x3 only), or null
  float* wino4 = nullptr; // F(4x4,3x3) transformed filters G (g * pre_scale) G^T (built on demand), or null
  float* wino4_t = nullptr;  // F(4x4) folded pre-BN: pre_shift / pre_scale per input channel
  float* w_frag = nullptr;   // the serving conv kernel's copy of w in fragment order (launch_convs_weights), or null
  int cin = 0, cout = 0, kh = 0, kw = 0, stride = 1, pad = 0;
  int cin2 = 0;  // fused 1x1 shortcut input channels (w rows KH*KW*cin + cin2 long), else 0
  void geometry(int cin_, int cout_, int kh_, int kw_, int stride_, int pad_) {
    cin = cin_, cout = cout_, kh = kh_, kw = kw_, stride = stride_, pad = pad_;
  }
};

struct BlockW {
  BlockSpec spec;
  ConvW conv1, conv2, sc;
  bool has_sc_conv = false;
  // conv2 and the conv shortcut as one GEMM (stride-2 blocks with a conv shortcut): both BN
  // scales folded into the weights [Cout][3][3][Cout | Cin], the two BN shifts summed
  ConvW conv2_sc;
};

// kind: 0 other launch, 1 direct implicit-GEMM conv, 2 Winograd conv (frhip.h FR_PROF_*)
struct ProfEvent {
  hipEvent_t a, b;
  double flop;       // algorithmic (direct-conv) FLOPs
  double exec_flop;  // FLOPs the MFMA pipe actually executes
  int kind;
};

// The buffers one running forward writes (a lane).  Lane 0 (fr_finalize, max_batch crops) is also
// the workspace of every launch outside a forward; lanes 1 .. MAX_LANES - 1 (fr_set_lanes) are
// further sets, so the parts of a large batch run as concurrent forwards on their own streams and
// one part's part-empty last round of a layer fills with another part's work.
struct LaneWs {
  float* act[3] = {nullptr, nullptr, nullptr};
  float* sc_buf = nullptr;
  float* partial = nullptr;  // head FC split-K parts (fr_handle::HEAD_PARTS x max_batch rows)
  float* w4part = nullptr;   // F(4x4) split-K partial outputs (small batches), W4PART_FLOATS
  // stream-K workspace shared by every conv launch of the lane (launches are stream-ordered)
  float* sk_ws = nullptr;
  long long sk_ws_floats = 0;
  int* sk_cnt = nullptr;
  int sk_cnt_cap = 0;
};
constexpr int MAX_LANES = 4;

// What one run_conv launch reads and writes.
struct ConvCall {
  const float* x;
  float* y;
  int B, H, W;
  frhip::Epi epi;
  const float* res = nullptr;
  int res_H = 0, res_W = 0;
  const float* x2 = nullptr;  // the fused shortcut's input (cw.cin2 > 0)
  int nsplit = 1;             // split-K slices, split_stride elements apart
  long long split_stride = 0;
  // channel-blocked layout bits of this launch (plan_layouts): CONVS_BLK_* for the serving conv
  // kernel (ConvParams::blk), W4_BLK_* for the F(4x4) kernel (Wino4Params::blk)
  int convs_blk = 0, w4_blk = 0;
  // serving conv kernel only: also write y * y2_scale + y2_shift, the next block's pre-BN input
  float* y2 = nullptr;
  const float *y2_scale = nullptr, *y2_shift = nullptr;
};

// Process-wide A/B knobs of the conv dispatch (set through frt_set_*; conv_dispatch.cpp).
struct ConvKnobs {
  // frt_set_conv2sc_tile: the tile of the fused stride-2 conv2 + conv-shortcut launches, -1 = the rule
  int conv2sc_tile = -1;
  // frt_set_wino4_nbg: tile blocks per XCD item group of the F(4x4) launches, 0 = the rule
  int wino4_nbg = 0;
  // cap on the F(4x4) split-K parts of small grids (frt_set_wino4_max_split: serving sweeps); 0 = none
  int wino4_max_split = 0;
  // the stage-1 stride-2 conv2 on its band kernel (frt_set_s2_band: tests compare it with the
  // implicit-GEMM kernel)
  int s2band = 1;
  // poll bound of wino4_kernel's ring hand-off waits (frt_set_wino4_poll_limit: tests force expiry)
  int wino4_poll = frhip::WINO4_POLL_DEFAULT;
  // F(4x4) item shapes for layers of 65..96 and of <= 32 couts (frt_set_wino4_shapes: A/B and tests)
  int wino4_shapes = 1;
};
extern ConvKnobs g_knobs;

struct Detector;  // detector.cpp
void detector_destroy(Detector* d);
void detector_set_row_reduction(Detector* d, bool on);
// every conv of the detector (for the Winograd filter builds); no-op for d == nullptr
void detector_convs(Detector* d, std::vector<ConvW*>& out);

}  // namespace frhip_rt

struct fr_handle {
  std::mutex mu;
  std::string arch, model_type, err;
  bool arcface = false;   // insightface IResNet keys/semantics (face_embedder.py:64-88)
  bool detector = false;  // arch "scrfd_10g": a face detector, not an embedding model
  int device = 0;
  int max_batch = 256;
  bool finalized = false;
  std::vector<frhip_rt::BlockSpec> specs;
  std::map<std::string, size_t> expected;  // key -> numel
  std::map<std::string, std::vector<float>> params;

  // device arena with every folded weight
  float* arena = nullptr;
  size_t arena_floats = 0;
  float *lut = nullptr, *stem_w = nullptr, *stem_scale = nullptr, *stem_shift = nullptr, *stem_prelu = nullptr;
  std::vector<frhip_rt::BlockW> blocks;
  frhip_rt::ConvW head;  // BN2d pre-affine + FC as 7x7 valid conv
  float *fc_bias = nullptr, *bn1d_scale = nullptr, *bn1d_shift = nullptr;

  // workspace (activations, partials and the stream-K slabs: lane_ws below)
  // head FC split-K parts: serving batches (4 n <= max_batch) / larger; partial buffers hold
  // HEAD_PARTS x max_batch rows (>= 98 n for the serving split at 4 n <= max_batch, >= 32 n for the other)
  static constexpr int HEAD_SPLIT_SMALL = 98, HEAD_SPLIT = 32, HEAD_PARTS = 49;
  uint8_t* in_stage = nullptr;
  float* emb_stage = nullptr;

  // resize branch of FaceEmbedder.preprocess (face_embedder.py:94-96): cv2.resize INTER_LINEAR
  // coefficient tables per source size ([112 x][4] then [112 y][4], device), resized crops of one
  // chunk, and host-API staging of the raw crops
  struct ResizeTab {
    int H, W, simd_end;
    int* tab;
    unsigned long long used;  // last use (LRU clock)
    hipEvent_t last;          // recorded after the table's last resize launch (on that call's stream)
  };
  static constexpr size_t RS_TABS_MAX = 16;  // coefficient tables kept per handle (LRU)
  std::vector<ResizeTab> rs_tabs;
  unsigned long long rs_clock = 0;
  uint8_t* rs_stage = nullptr;
  void* rs_src = nullptr;
  size_t rs_src_cap = 0;
  // fr_resize_images / fr_embed_images: the host staging of every chunk of one call (descriptors +
  // tables; chunk c starts at ri_chunks[c]) and the device copy of the chunk in flight
  std::vector<char> ri_host;
  std::vector<size_t> ri_chunks;
  void* ri_dev = nullptr;
  size_t ri_dev_cap = 0;

  // gallery + match workspace
  float* gallery = nullptr;
  int G = 0;
  size_t gallery_cap = 0;
  float* qn = nullptr;
  size_t qn_cap = 0;
  float* scores = nullptr;
  size_t scores_cap = 0;
  void* match_io = nullptr;
  size_t match_io_cap = 0;
  void* gallery_tmp = nullptr;  // tail staging for row deletes
  size_t gallery_tmp_cap = 0;
  // int32 arrays the batch calls stage from the host (stage_int32): the CSR offsets of students,
  // tracks, frames and clips, and fr_identity_scores' offsets and tile list (all synchronise)
  void* csr_stage = nullptr;
  size_t csr_stage_cap = 0;
  std::vector<int32_t> csr_host;  // the packed host copy of a call that stages several arrays
  // fr_identity_scores: row norms of the probes and the gallery + the off-unit flag;
  // fr_eval_probes: the staged thresholds
  void* eval_ws = nullptr;
  size_t eval_ws_cap = 0;
  // sample gallery (fr_samples_set): every enrolled row of every identity, beside the template
  // gallery, and what a match needs of it, staged once: sample_meta = [off-unit flag][row norms:
  // sample_rows][offsets: sample_ids + 1][serving tiles: sample_tiles + 1][evaluation tiles:
  // sample_eval_tiles + 1] (d_sample_* point into it)
  float* samples = nullptr;
  size_t samples_cap = 0;
  void* sample_meta = nullptr;
  size_t sample_meta_cap = 0;
  int sample_ids = 0, sample_rows = 0, sample_tiles = 0, sample_eval_tiles = 0;
  int* d_sample_flag = nullptr;
  float* d_sample_norm = nullptr;
  int *d_sample_off = nullptr, *d_sample_tiles = nullptr, *d_sample_eval_tiles = nullptr;
  // fr_match_identities: [query norms: n][identity scores: chunk x sample_ids]
  void* ident_ws = nullptr;
  size_t ident_ws_cap = 0;

  // alignment / quality workspace
  void* align_m = nullptr;  // [n][6] inverse affine maps (double), or fr_align_images' [n] WarpFace
  size_t align_m_cap = 0;
  void* blur_out = nullptr;  // [n] double
  size_t blur_out_cap = 0;
  void* blur_ws = nullptr;  // multi-block blur: per (image, chunk) int64 L sums + double values
  size_t blur_ws_cap = 0;
  // fr_align_device: [slots] WarpFace written by the fit kernel (a buffer of its own: the call is
  // asynchronous, and a captured graph keeps replaying into it)
  void* align_slots = nullptr;
  size_t align_slots_cap = 0;
  // fr_quality_gate_device: [n_frames] int32 valid slots per frame, between its two launches
  void* gate_ws = nullptr;
  size_t gate_ws_cap = 0;

  int cus = 0;  // CUs of the device (ensure_stream_k)
  bool stream_k = true;
  bool fuse_shortcut = true;  // conv2 + conv shortcut as one launch (frt_set_fuse_shortcut: A/B)
  frhip::Precision prec = frhip::PREC_F32;
  bool winograd = true;          // FR_CONV_WINOGRAD / _WINOGRAD4 for stride-1 3x3 convs
  int wino_m = 4;                // output tile of the Winograd algorithm: 4 = F(4x4,3x3) (default), 2 = F(2x2,3x3)
  float* wino_arena = nullptr;   // F(2x2) filters, built when that algorithm is selected
  float* wino4_arena = nullptr;  // F(4x4) filters, likewise
  float* convs_arena = nullptr;  // the serving conv kernel's filters (ConvW::w_frag), built at fr_finalize
  static constexpr long long W4PART_FLOATS = 16ll << 20;

  // lanes (fr_set_lanes): a forward of n crops runs as min(lane_max, n / lane_min) concurrent
  // parts with workspace lane_ws[l], lane 0 on the caller's stream, lane l >= 1 on lane_stream[l]
  int lane_min = 0, lane_max = 1;
  bool lanes_fallback = false;  // lanes were turned off by a failed lane-workspace allocation
  frhip_rt::LaneWs lane_ws[frhip_rt::MAX_LANES];
  int lane_batch[frhip_rt::MAX_LANES] = {0, 0, 0, 0};  // crops lane l's buffers hold
  hipStream_t lane_stream[frhip_rt::MAX_LANES] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t lane_fork = nullptr;
  hipEvent_t lane_join[frhip_rt::MAX_LANES] = {nullptr, nullptr, nullptr, nullptr};

  // SCRFD detector (arch "scrfd_10g"): layers, workspace (detector.cpp)
  frhip_rt::Detector* det = nullptr;

  // hipGraph replay of small forwards (fr_set_graph_batch): one executable graph per
  // (n, normalize), captured on cap_stream from in_stage to emb_stage
  struct GraphEntry {
    int n, normalize;
    hipGraphExec_t exec;
  };
  int graph_max_n = 0;
  bool capturing = false;  // forwards captured into a graph run one lane
  hipStream_t cap_stream = nullptr;
  std::vector<GraphEntry> graphs;

  // forwards of n <= convs_max_n crops run every body 3x3 conv on conv_small.hip's kernel (one
  // launch per layer, whole K per 16x16 tile) instead of F(4x4) split-K + fixup / the split-K
  // direct convs (frt_set_small_conv)
  int convs_max_n = 2;
  // output-pixel limit of a batch-1 layer on that kernel (frt_set_small_conv_pixels; batch 2: 1,024)
  int convs_max_m1 = 4096;
  // a one-lane forward's conv2 on that kernel also writes the next block's pre-BN input
  // (ConvCall::y2), and that block's conv1 then runs without pre-BN on it
  // (frt_set_small_conv_pre_epilogue: A/B)
  bool convs_pre_epilogue = true;
  // activations passed between two serving-kernel layers of a one-lane forward are channel-blocked
  // (ConvCall::convs_blk, from plan_layouts); frt_set_small_conv_blocked: A/B
  bool convs_blocked = true;
  // channel-blocked activations between F(4x4) layers of larger forwards (ConvCall::w4_blk, from
  // plan_layouts); frt_set_wino4_blocked: A/B
  bool w4_blocked = true;

  // device-side error word (host-pinned, coherent): kernels that detect a broken invariant
  // store an FR_DEVERR_* code here (wino4_kernel: a ring hand-off that timed out); the runtime
  // reads it at its sync points and at the entry of every compute call (check_dev_err)
  int* dev_err = nullptr;

  // profiling
  bool prof = false;
  std::vector<frhip_rt::ProfEvent> events;
  std::vector<hipEvent_t> pool;
  double last_ms[3] = {0, 0, 0}, last_flop[3] = {0, 0, 0}, last_exec[3] = {0, 0, 0};
  int64_t last_n[3] = {0, 0, 0};

  ~fr_handle() {
    frhip_rt::detector_destroy(det);
    for (auto& e : events) {
      (void)hipEventDestroy(e.a);
      (void)hipEventDestroy(e.b);
    }
    for (auto e : pool) (void)hipEventDestroy(e);
    for (auto& g : graphs) (void)hipGraphExecDestroy(g.exec);
    if (cap_stream) (void)hipStreamDestroy(cap_stream);
    if (lane_fork) (void)hipEventDestroy(lane_fork);
    for (int l = 0; l < frhip_rt::MAX_LANES; ++l) {  // (lane 0 has no stream / event of its own)
      if (lane_stream[l]) (void)hipStreamDestroy(lane_stream[l]);
      if (lane_join[l]) (void)hipEventDestroy(lane_join[l]);
      frhip_rt::LaneWs& L = lane_ws[l];
      for (auto p : L.act) (void)hipFree(p);
      (void)hipFree(L.sc_buf);
      (void)hipFree(L.partial);
      (void)hipFree(L.w4part);
      (void)hipFree(L.sk_ws);
      (void)hipFree(L.sk_cnt);
    }
    (void)hipFree(arena);
    (void)hipFree(wino_arena);
    (void)hipFree(wino4_arena);
    (void)hipFree(convs_arena);
    (void)hipFree(in_stage);
    (void)hipFree(emb_stage);
    for (auto& t : rs_tabs) {
      (void)hipFree(t.tab);
      if (t.last) (void)hipEventDestroy(t.last);
    }
    (void)hipFree(rs_stage);
    (void)hipFree(rs_src);
    (void)hipFree(ri_dev);
    (void)hipFree(gallery);
    (void)hipFree(qn);
    (void)hipFree(scores);
    (void)hipFree(match_io);
    (void)hipFree(gallery_tmp);
    (void)hipFree(csr_stage);
    (void)hipFree(eval_ws);
    (void)hipFree(samples);
    (void)hipFree(sample_meta);
    (void)hipFree(ident_ws);
    (void)hipFree(align_m);
    (void)hipFree(blur_out);
    (void)hipFree(blur_ws);
    (void)hipFree(align_slots);
    (void)hipFree(gate_ws);
    if (dev_err) (void)hipHostFree(dev_err);
  }
};

namespace frhip_rt {

int fail(fr_handle* h, int code, const std::string& msg);
// The handle's device error word: allocated (zeroed) on first use; FR_OK or FR_ERR_HIP.
int ensure_dev_err(fr_handle* h);
// FR_ERR_HIP (and the word cleared) if a kernel of work that has completed by now reported a
// broken invariant, else FR_OK.  Call after a stream sync to cover that call's own work.
int check_dev_err(fr_handle* h);

#define FR_HIP(h, call)                                                                          \
  do {                                                                                           \
    hipError_t e_ = (call);                                                                      \
    if (e_ != hipSuccess)                                                                        \
      return ::frhip_rt::fail(h, FR_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)

// "<what> launch: <HIP's text>" as the handle's error; returns FR_ERR_HIP.
int launch_fail(fr_handle* h, const char* what, hipError_t e);
// The handle's lock, or no lock for h == NULL: for the calls that check their arguments before the
// handle, so that those checks report the same way without one.
std::unique_lock<std::mutex> lock_handle(fr_handle* h);

// The nouns of csr_check's messages, e.g. {"offsets", "track", "frames"}.
struct CsrNouns {
  const char *array, *item, *unit;
};
// Checks the CSR array offsets[0 .. n]: offsets[0] == 0 and every slice length in [min_len, max_len],
// in long long, so decreasing or wrapping offsets are reported.  With `outer` (itself checked CSR
// offsets into `offsets`) slice i runs from offsets[outer[i]] to offsets[outer[i + 1]].  Returns
// the error text, or an empty string.
std::string csr_check(const int32_t* offsets, int n, long long min_len, long long max_len, const CsrNouns& nouns,
                      const int32_t* outer = nullptr);

// Copies host int32 arrays back to back into h->csr_stage with one copy on stream s; dev[i] is the
// device address of parts[i].  The host memory is pageable: the caller synchronises s before it
// returns.
struct Int32Span {
  const int32_t* p;
  size_t n;
};
int stage_int32(fr_handle* h, hipStream_t s, std::initializer_list<Int32Span> parts, const int** dev);

// Restores the caller's current device on scope exit.
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

// Host staging of every folded tensor before one upload into an arena.
struct Packer {
  std::vector<float> buf;
  std::vector<std::pair<float**, size_t>> fix;  // (destination pointer, float offset)
  void put(float** dst, const std::vector<float>& v) {
    size_t off = (buf.size() + 3) & ~size_t(3);  // 16-B alignment for float4 loads
    buf.resize(off);
    buf.insert(buf.end(), v.begin(), v.end());
    fix.push_back({dst, off});
  }
};

void add_bn(std::map<std::string, size_t>& m, const std::string& p, int c, bool affine = true);
void bn_fold(const std::vector<float>* gamma, const std::vector<float>* beta, const std::vector<float>& mean,
             const std::vector<float>& var, std::vector<float>& scale, std::vector<float>& shift);
std::vector<float> repack_oihw(const std::vector<float>& w, int O, int I, int kh, int kw);
int ensure_buf(fr_handle* h, void** p, size_t* cap, size_t bytes);
int ensure_stream_k(int device, int* cus, float** ws, long long* ws_floats, int** cnt, int* cnt_cap);
const std::vector<float>* getp(fr_handle* h, const std::string& k);

// finalize.cpp
extern thread_local std::string g_create_error;  // fail(nullptr, ...): fr_last_error(NULL)
std::vector<BlockSpec> block_specs(const std::string& arch, bool* ok);
std::map<std::string, size_t> embedder_schema(bool arcface, const std::vector<BlockSpec>& specs);
// t = pre_shift / pre_scale per input channel of c (zeros without pre-BN); false if not finite
bool wino4_pre_fold(const ConvW* c, std::vector<float>& t);
// the filters of the selected Winograd algorithm, built on first use after fr_finalize
int ensure_winograd(fr_handle* h);
// fr_finalize under the handle's lock and device: fold, upload, allocate the workspace
int finalize_model(fr_handle* h);

// batch_ops.cpp
// fr_capture_tracks' and fr_live_tracks' match threshold: the smallest integer q >= 0 with sqrt(q / 4.0) >= max_distance
// in double (q = 4 x a squared centroid distance), so that q < q_limit is the reference's
// `distance < max_distance`; 0 for max_distance <= 0 or NaN
long long capture_q_limit(double max_distance);
// frt_set_eval_chunk: probes per GEMM chunk of fr_identity_scores and of fr_match_identities'
// composed path, 0 = the 2 GiB rule
extern int g_eval_chunk;
// frt_set_identify_path: 0 = fr_match_identities' rule (the fused kernel for small n x rows),
// 1 = the fused kernel, 2 = the composed path, for every n
extern int g_identify_path;
// frt_set_identify_tile_rows: the row cap of the serving tiles the next fr_samples_set cuts
extern int g_identify_tile_rows;
// fr_match_identities under the handle's lock and device (fr_embed_match_identities' second half)
int match_identities_device(fr_handle* h, const float* Q, int n, int aggregation, int agg_k, int k, int32_t* idx,
                            float* score, hipStream_t s);

// conv_dispatch.cpp
// The geometry and K-step fields of conv cw over a B x H x W input in nsplit K-slices: what the
// kernel-selection rules read, and every non-pointer field a launch needs.
frhip::ConvParams conv_shape(const ConvW& cw, int B, int H, int W, int nsplit = 1);
// Whether run_conv puts a launch on the serving conv kernel / the F(4x4) kernel: one rule each
// for run_conv's branches and for plan_layouts, so the two cannot disagree.
bool convs_takes(const fr_handle* h, const ConvW& cw, frhip::ConvParams p, frhip::Epi epi, int nsplit, bool has_x2);
bool w4_takes(const fr_handle* h, const ConvW& cw, frhip::Epi epi, int res_H, int res_W, int Ho, int Wo);
// One conv launch on stream s with lane L's stream-K / split-K workspace.  *wrote_y2 is set when
// the launch wrote c.y2 (only the serving conv kernel does).
int run_conv(fr_handle* h, const ConvW& cw, const ConvCall& c, const LaneWs& L, hipStream_t s,
             bool* wrote_y2 = nullptr);

// embed_forward.cpp
// Times the launches of its scope with a pair of events when profiling is on (fr_profile_enable).
struct ProfScope {
  fr_handle* h;
  hipStream_t s;
  ProfEvent ev{};
  bool on;
  ProfScope(fr_handle* h_, hipStream_t s_, double flop, int kind, double exec_flop = -1.0);
  ~ProfScope();
};
void clear_graphs(fr_handle* h);
int forward_staged(fr_handle* h, int n, int normalize, hipStream_t s);
int embed_device(fr_handle* h, const uint8_t* rgb, int n, float* out, int normalize, hipStream_t s);
int resize_device(fr_handle* h, const uint8_t* src, int n, int H, int W, uint8_t* dst, hipStream_t s);
int check_crop_size(fr_handle* h, int height, int width);
int embed_any(fr_handle* h, const uint8_t* rgb, int n, int height, int width, float* out, int normalize,
              hipStream_t s);
// fr_resize_images / fr_embed_images: check_images refuses a NULL image or a side out of range
// (naming the image); the other two run a checked list (and synchronise s at entry)
int check_images(fr_handle* h, const uint8_t* const* images, const int32_t* sizes, int n);
int resize_images(fr_handle* h, const uint8_t* const* images, const int32_t* sizes, int n, uint8_t* dst,
                  hipStream_t s);
int embed_images(fr_handle* h, const uint8_t* const* images, const int32_t* sizes, int n, float* out, int normalize,
                 hipStream_t s);
int match_device(fr_handle* h, const float* Q, int n, int k, int32_t* idx, float* score, hipStream_t s);
// Grow the gallery allocation to hold `rows` rows, keeping the first G rows (stream-ordered).
int gallery_reserve(fr_handle* h, int rows, hipStream_t s);

// align_host.cpp
// estimateAffinePartial2D(src, dst)[0]: returns false (M NaN) where cv2 returns None
bool fit_similarity(const float* src, const float* dst, int n, double M[6]);
void invert_affine(const double Mf[6], double Mi[6]);
// what the device fit takes in place of update_num_iters' logarithms (frhip_kernels.h FitLogs)
void fit_logs(frhip::FitLogs* lg);
void augment_tables(int H, int W, frhip::AugTables* t);
void reference_template(int S, float t[10]);

// detector.cpp
// cv::resize INTER_LINEAR (uint8) coefficient table of one axis: (src0, src1, w0, w1) per output
void resize_axis_table(int dsize, int ssize, int* t);
// end of the SSE2-vectorised part of a resized row of row_elems bytes (the rest rounds as scalar code)
int resize_simd_end(int row_elems);
std::map<std::string, size_t> detector_schema();
int detector_finalize(fr_handle* h);
int detector_run(fr_handle* h, const uint8_t* frames, int n, int height, int width, float det_thresh, int max_faces,
                 float* dets, int32_t* counts, hipStream_t s);
// fr_detect_device: detector_run's launches with dets [n][max_faces][15] and counts [n] on the
// device (NMS writes them in place; counts[f] = -1 for a frame over the candidate limit) and the
// resize tables cached per frame size.  Asynchronous on s once the size has been seen.
int detector_run_device(fr_handle* h, const uint8_t* frames, int n, int height, int width, float det_thresh,
                        int max_faces, float* dets, int32_t* counts, hipStream_t s);
int detector_forward(fr_handle* h, const uint8_t* frames, int n, int height, int width, float* heads,
                     uint8_t* canvas, hipStream_t s);
// The same for n images of their own sizes (host arrays: images[n] device pointers, sizes[n][2] =
// height, width), in chunks of max_frames with per-image letterbox geometry (frhip.h: fr_detect_images);
// detector_forward_images runs one chunk as detector_run_images runs it.
int detector_run_images(fr_handle* h, const uint8_t* const* images, const int32_t* sizes, int n, float det_thresh,
                        int max_faces, float* dets, int32_t* counts, hipStream_t s);
// fr_detect_images_device: detector_run_images' chunks with dets and counts on the device, as
// detector_run_device writes them; tables and scales made on the device, nothing staged.  Asynchronous.
int detector_run_images_device(fr_handle* h, const uint8_t* const* images, const int32_t* sizes, int n,
                               float det_thresh, int max_faces, float* dets, int32_t* counts, hipStream_t s);
int detector_forward_images(fr_handle* h, const uint8_t* const* images, const int32_t* sizes, int n, float* heads,
                            uint8_t* canvas, hipStream_t s);
// The post-processing alone (frhip_testing.h: frt_detector_postprocess): heads (device, n <= max_frames
// frames in detector_forward's layout) into the detector's head buffers, then postprocess_chunk with
// det_scale or, when det_scales (host [n]) is given, with those uploaded as the per-frame scales.
int detector_postprocess(fr_handle* h, const float* heads, int n, float det_scale, const float* det_scales,
                         float det_thresh, int max_faces, float* dets, int32_t* counts, hipStream_t s);

}  // namespace frhip_rt
