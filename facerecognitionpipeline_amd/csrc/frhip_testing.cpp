// libfrhip test entry points (include/frhip_testing.h): single kernels behind a C call, and the
// A/B knobs of the conv dispatch and of a handle.  Not part of the public API.
#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "gate_math.h"
#include "runtime.h"
// (after runtime.h: it declares fr_handle through frhip.h)
#include "../../include/frhip_testing.h"

using namespace frhip;
using namespace frhip_rt;

// An A/B knob of a handle: set under its lock; graphs captured with the old value are dropped.
template <class Set>
static int set_handle_knob(fr_handle* h, Set set) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  DeviceGuard dg(h->device);
  set();
  clear_graphs(h);
  return FR_OK;
}

extern "C" {

// frt_conv2d / frt_conv2d_fused: one launch_conv, a ConvParams built as run_conv builds it
// (conv_shape of a ConvW with cin2 > 0 sets steps1 / steps_total of the fused shortcut).
// Only what would dereference a null pointer is refused here; every other rule (channel multiples,
// which epilogues take pre-BN or a fused shortcut, the tiles of the detector's instances) is left
// to launch_conv, so tests pin the launcher's refusals, not this wrapper's.
static int conv2d_entry(const char* who, const float* x, const float* x2, const float* w, float* y, int B, int H, int W,
                        int cin, int cin2, int cout, int kh, int kw, int stride, int pad, const float* pre_scale,
                        const float* pre_shift, const float* post_scale, const float* post_shift, const float* prelu,
                        const float* res, int res_h, int res_w, int epi, int nsplit, int tile, int stream_k,
                        int precision, void* stream) {
  static int t_cus = 0, t_cap = 0;
  static float* t_ws = nullptr;
  static long long t_wsf = 0;
  static int* t_cnt = nullptr;
  const bool res_epi = epi == EPI_AFFINE_RES || epi == EPI_AFFINE_RES_SUB || epi == EPI_AFFINE_RES_PRELU;
  const bool prelu_epi = epi == EPI_AFFINE_PRELU || epi == EPI_AFFINE_RES_PRELU;
  if (epi < 0 || epi > EPI_AFFINE_RES_PRELU || nsplit < 1 || (nsplit > 1 && epi != EPI_RAW) ||
      (tile < 0 || tile >= TILE_COUNT) || stride < 1 || kh < 1 || kw < 1 || B < 1 || H < 1 || W < 1 || cin < 1 ||
      cout < 1 || cin2 < 0 || pad < 0 || H + 2 * pad < kh || W + 2 * pad < kw)
    return fail(nullptr, FR_ERR_INVALID_ARGUMENT, std::string(who) + ": bad arguments");
  if (!x || !w || !y || (cin2 > 0 && !x2) || ((pre_scale != nullptr) != (pre_shift != nullptr)) ||
      (epi != EPI_RAW && (!post_scale || !post_shift)) || (prelu_epi && !prelu) || (res_epi && !res) ||
      (epi == EPI_AFFINE_RES_SUB && (res_h < 1 || res_w < 1)) || (epi == EPI_AFFINE_RES_PRELU && pre_scale))
    return fail(nullptr, FR_ERR_INVALID_ARGUMENT, std::string(who) + ": a pointer this epilogue reads is missing");
  ConvW cw;
  cw.geometry(cin, cout, kh, kw, stride, pad);
  cw.cin2 = cin2;
  ConvParams p = conv_shape(cw, B, H, W, nsplit);
  p.x = x;
  p.x2 = cin2 > 0 ? x2 : nullptr;
  p.w = w;
  p.y = y;
  p.pre_scale = pre_scale;
  p.pre_shift = pre_shift;
  p.post_scale = post_scale;
  p.post_shift = post_shift;
  p.prelu = prelu;
  p.res = res;
  p.res_H = res_h;
  p.res_W = res_w;
  p.split_stride = (long long)p.M * cout;
  if (stream_k) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (ensure_stream_k(dev, &t_cus, &t_ws, &t_wsf, &t_cnt, &t_cap) != FR_OK)
      return fail(nullptr, FR_ERR_HIP, std::string(who) + ": stream-K workspace allocation failed");
    p.sk_cus = t_cus;
    p.sk_ws = t_ws;
    p.sk_ws_floats = t_wsf;
    p.sk_cnt = t_cnt;
    p.sk_cnt_cap = t_cap;
  }
  hipError_t e = launch_conv(p, (ConvTile)tile, pre_scale != nullptr, (Epi)epi, nsplit, (hipStream_t)stream,
                             precision == 1 ? PREC_BF16X3 : PREC_F32);
  if (e != hipSuccess) return fail(nullptr, FR_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
  return FR_OK;
}

int frt_conv2d(const float* x, const float* w, float* y, int B, int H, int W, int cin, int cout, int kh, int kw,
               int stride, int pad, const float* pre_scale, const float* pre_shift, const float* post_scale,
               const float* post_shift, const float* prelu, const float* res, int res_h, int res_w, int epi,
               int nsplit, int tile, int stream_k, int precision, void* stream) {
  return conv2d_entry("frt_conv2d", x, nullptr, w, y, B, H, W, cin, 0, cout, kh, kw, stride, pad, pre_scale, pre_shift,
                      post_scale, post_shift, prelu, res, res_h, res_w, epi, nsplit, tile, stream_k, precision, stream);
}

int frt_conv2d_fused(const float* x, const float* x2, const float* w, float* y, int B, int H, int W, int cin, int cin2,
                     int cout, int kh, int kw, int stride, int pad, const float* pre_scale, const float* pre_shift,
                     const float* post_scale, const float* post_shift, const float* prelu, const float* res, int res_h,
                     int res_w, int epi, int nsplit, int tile, int stream_k, int precision, void* stream) {
  return conv2d_entry("frt_conv2d_fused", x, x2, w, y, B, H, W, cin, cin2, cout, kh, kw, stride, pad, pre_scale,
                      pre_shift, post_scale, post_shift, prelu, res, res_h, res_w, epi, nsplit, tile, stream_k,
                      precision, stream);
}

int frt_conv_split_fixup(const float* part, int S, long long stride, int B, int Ho, int Wo, int cout,
                         const float* post_scale, const float* post_shift, const float* res, int res_h, int res_w,
                         int epi, float* y, void* stream) {
  const bool sub = epi == EPI_AFFINE_RES_SUB;
  if (!part || !y || !post_scale || !post_shift || B < 1 || Ho < 1 || Wo < 1 || cout < 1 ||
      (long long)B * Ho * Wo * cout >= (1ll << 31) || stride < (long long)B * Ho * Wo * cout ||
      ((epi == EPI_AFFINE_RES || sub) && !res) ||
      (sub && (res_h < 2 * (Ho - 1) + 1 || res_w < 2 * (Wo - 1) + 1)))  // the pixel (2 oy, 2 ox) must exist
    return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "frt_conv_split_fixup: bad arguments");
  ConvParams p{};  // exactly the fields conv_split_fixup_kernel reads
  p.y = y;
  p.post_scale = post_scale;
  p.post_shift = post_shift;
  p.res = res;
  p.M = B * Ho * Wo;
  p.Cout = cout;
  p.Ho = Ho;
  p.Wo = Wo;
  p.res_H = res_h;
  p.res_W = res_w;
  const hipError_t e = launch_conv_split_fixup(p, (Epi)epi, part, S, stride, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "frt_conv_split_fixup: refused");
  if (e != hipSuccess) return fail(nullptr, FR_ERR_HIP, std::string("frt_conv_split_fixup: ") + hipGetErrorString(e));
  return FR_OK;
}

int frt_conv2d_winograd(const float* x, const float* w, float* y, int B, int H, int W, int cin, int cout,
                        const float* pre_scale, const float* pre_shift, const float* post_scale,
                        const float* post_shift, const float* prelu, const float* res, int epi, void* stream) {
  if (!wino_supported(cin, cout, 3, 3, 1, 1) || (epi != EPI_AFFINE_PRELU && epi != EPI_AFFINE_RES) ||
      (epi == EPI_AFFINE_PRELU && (!pre_scale || !pre_shift || !prelu)) || (epi == EPI_AFFINE_RES && (pre_scale || !res)) ||
      !post_scale || !post_shift || B < 1 || H < 1 || W < 1)
    return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "frt_conv2d_winograd: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  float* u = nullptr;
  if (hipMalloc((void**)&u, wino_weight_floats(cout, cin) * sizeof(float)) != hipSuccess)
    return fail(nullptr, FR_ERR_HIP, "frt_conv2d_winograd: allocation failed");
  hipError_t e = launch_wino_weights(w, u, cout, cin, s);
  if (e == hipSuccess) {
    WinoParams p{};
    p.x = x;
    p.u = u;
    p.y = y;
    p.pre_scale = pre_scale;
    p.pre_shift = pre_shift;
    p.post_scale = post_scale;
    p.post_shift = post_shift;
    p.prelu = prelu;
    p.res = res;
    p.B = B;
    p.H = H;
    p.W = W;
    p.Cin = cin;
    p.Cout = cout;
    e = launch_wino(p, pre_scale != nullptr, (Epi)epi, s);
  }
  const hipError_t se = hipStreamSynchronize(s);
  (void)hipFree(u);
  if (e == hipSuccess) e = se;
  if (e != hipSuccess) return fail(nullptr, FR_ERR_HIP, std::string("frt_conv2d_winograd: ") + hipGetErrorString(e));
  return FR_OK;
}

static int g_frt_wino4_split = 1;
int frt_set_wino4_shapes(int mode) {
  if (mode < 0 || mode > 2) return FR_ERR_INVALID_ARGUMENT;
  g_knobs.wino4_shapes = mode;
  return FR_OK;
}
int frt_set_wino4_nbg(int nbg) {
  if (nbg < 0) return FR_ERR_INVALID_ARGUMENT;
  g_knobs.wino4_nbg = nbg;
  return FR_OK;
}
int frt_set_conv2sc_tile(int tile) {
  if (tile < -1 || tile >= TILE_COUNT) return FR_ERR_INVALID_ARGUMENT;
  g_knobs.conv2sc_tile = tile;
  return FR_OK;
}
int frt_set_wino4_max_split(int s) {
  g_knobs.wino4_max_split = s < 0 ? 0 : s;
  return FR_OK;
}
int frt_conv2d_s2band(const float* x, const float* w, float* y, int B, int H, int W, const float* post_scale,
                      const float* post_shift, const float* res, void* stream) {
  if (!s2c64_supported(64, 64, 3, 3, 2, 1, H, W) || B < 1)
    return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "frt_conv2d_s2band: 64 -> 64 channels, even H, W <= 112");
  S2Params sp{};
  sp.x = x;
  sp.w = w;
  sp.post_scale = post_scale;
  sp.post_shift = post_shift;
  sp.res = res;
  sp.y = y;
  sp.B = B;
  sp.H = H;
  sp.W = W;
  const hipError_t e = launch_s2c64(sp, (hipStream_t)stream);
  if (e != hipSuccess) return fail(nullptr, FR_ERR_HIP, std::string("frt_conv2d_s2band: ") + hipGetErrorString(e));
  return FR_OK;
}
int frt_set_eval_chunk(int probes) {
  if (probes < 0) return FR_ERR_INVALID_ARGUMENT;
  g_eval_chunk = probes;
  return FR_OK;
}
int frt_set_identify_path(int mode) {
  if (mode < 0 || mode > 2) return FR_ERR_INVALID_ARGUMENT;
  g_identify_path = mode;
  return FR_OK;
}
int frt_set_identify_tile_rows(int rows) {
  if (rows < 0 || rows > EVAL_MAX_ROWS) return FR_ERR_INVALID_ARGUMENT;
  g_identify_tile_rows = rows == 0 ? IDENT_TILE_ROWS : rows;
  return FR_OK;
}
int frt_set_s2_band(int on) {
  g_knobs.s2band = on != 0;
  return FR_OK;
}
int frt_set_wino4_poll_limit(int n) {
  g_knobs.wino4_poll = n < 0 ? WINO4_POLL_DEFAULT : n;
  return FR_OK;
}
int frt_conv2d_small_ex(const float* x, const float* x2, const float* w, float* y, int B, int H, int W, int cin,
                     int cin2, int cout, int stride, const float* pre_scale, const float* pre_shift,
                     const float* post_scale, const float* post_shift, const float* prelu, const float* res, int epi,
                     int blk, float* y2, const float* y2_scale, const float* y2_shift, void* stream) {
  // Only what conv_shape and the weight reorder below need, and a pre-BN pointer pair the kernel
  // would dereference, are checked here: which epilogues take pre-BN, the shortcut's width and
  // pointer, the residual, y2's operands are launch_convs' refusals, so tests pin the launcher's.
  if (B < 1 || H < 1 || W < 1 || (stride != 1 && stride != 2) || cin < 16 || cout < 16 || cin2 < 0 ||
      ((pre_scale != nullptr) != (pre_shift != nullptr)) || !w || cout % 16 || cin % 16 || cin2 % 16)
    return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "frt_conv2d_small_ex: bad arguments");
  ConvW cw;
  cw.geometry(cin, cout, 3, 3, stride, 1);
  cw.cin2 = cin2;
  ConvParams p = conv_shape(cw, B, H, W);  // (the kernel reads none of the K-step fields)
  p.x = x;
  p.x2 = cin2 > 0 ? x2 : nullptr;
  p.w = w;
  p.y = y;
  p.pre_scale = pre_scale;
  p.pre_shift = pre_shift;
  p.post_scale = post_scale;
  p.post_shift = post_shift;
  p.prelu = prelu;
  p.res = res;
  p.res_H = H;
  p.res_W = W;
  p.blk = blk;
  p.y2 = y2;
  p.y2_scale = y2_scale;
  p.y2_shift = y2_shift;
  // the kernel reads its filters in fragment order: a temporary copy (test entry point)
  float* wf = nullptr;
  const size_t wbytes = (size_t)cout * (9 * cin + cin2) * sizeof(float);
  hipError_t e = hipMalloc((void**)&wf, wbytes);
  if (e == hipSuccess) e = launch_convs_weights(w, wf, cout, 9 * cin + cin2, (hipStream_t)stream);
  if (e == hipSuccess) {
    p.w = wf;
    e = launch_convs(p, pre_scale != nullptr, (Epi)epi, (hipStream_t)stream);
  }
  if (wf) {
    const hipError_t e2 = hipStreamSynchronize((hipStream_t)stream);
    (void)hipFree(wf);
    if (e == hipSuccess) e = e2;
  }
  if (e == hipErrorInvalidValue) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "frt_conv2d_small_ex: refused");
  if (e != hipSuccess) return fail(nullptr, FR_ERR_HIP, std::string("frt_conv2d_small_ex: ") + hipGetErrorString(e));
  return FR_OK;
}
int frt_conv2d_small(const float* x, const float* x2, const float* w, float* y, int B, int H, int W, int cin,
                     int cin2, int cout, int stride, const float* pre_scale, const float* pre_shift,
                     const float* post_scale, const float* post_shift, const float* prelu, const float* res, int epi,
                     void* stream) {
  return frt_conv2d_small_ex(x, x2, w, y, B, H, W, cin, cin2, cout, stride, pre_scale, pre_shift, post_scale,
                             post_shift, prelu, res, epi, 0, nullptr, nullptr, nullptr, stream);
}
int frt_set_small_conv(fr_handle* h, int max_n) {
  return set_handle_knob(h, [&] { h->convs_max_n = std::max(0, max_n); });
}
int frt_set_small_conv_pre_epilogue(fr_handle* h, int on) {
  return set_handle_knob(h, [&] { h->convs_pre_epilogue = on != 0; });
}
int frt_set_small_conv_pixels(fr_handle* h, int max_m1) {
  if (!h || max_m1 < 0) return fail(h, FR_ERR_INVALID_ARGUMENT, "bad handle or pixel limit");
  return set_handle_knob(h, [&] { h->convs_max_m1 = max_m1; });
}
int frt_set_wino4_blocked(fr_handle* h, int on) {
  return set_handle_knob(h, [&] { h->w4_blocked = on != 0; });
}
int frt_set_small_conv_blocked(fr_handle* h, int on) {
  return set_handle_knob(h, [&] { h->convs_blocked = on != 0; });
}
int frt_set_fuse_shortcut(fr_handle* h, int on) {
  return set_handle_knob(h, [&] { h->fuse_shortcut = on != 0; });
}
int frt_set_wino4_split(int on) {
  g_frt_wino4_split = on != 0;
  return FR_OK;
}

int frt_conv2d_winograd4_ex(const float* x, const float* w, float* y, int B, int H, int W, int cin, int cout,
                           const float* pre_scale, const float* pre_shift, const float* post_scale,
                           const float* post_shift, const float* prelu, const float* res, int epi, int blk,
                           void* stream) {
  // epilogues: the IR body's (1 with pre-BN, 2) and the detector's (0, 1 without pre-BN, 5)
  const bool res_epi = epi == EPI_AFFINE_RES || epi == EPI_AFFINE_RES_PRELU;
  const bool prelu_epi = epi == EPI_AFFINE_PRELU || epi == EPI_AFFINE_RES_PRELU;
  if (!wino4_supported(cin, cout, 3, 3, 1, 1) ||
      (epi != EPI_AFFINE && epi != EPI_AFFINE_PRELU && epi != EPI_AFFINE_RES && epi != EPI_AFFINE_RES_PRELU) ||
      (pre_scale && (epi != EPI_AFFINE_PRELU || !pre_shift)) || (prelu_epi && !prelu) || (res_epi != (res != nullptr)) ||
      !post_scale || !post_shift || B < 1 || H < 1 || W < 1)
    return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "frt_conv2d_winograd4_ex: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  ConvW cw;
  cw.cin = cin;
  cw.pre_scale = const_cast<float*>(pre_scale);
  cw.pre_shift = const_cast<float*>(pre_shift);
  std::vector<float> t;
  if (hipStreamSynchronize(s) != hipSuccess || !wino4_pre_fold(&cw, t))
    return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "frt_conv2d_winograd4_ex: pre-BN scale has a zero");
  float *u = nullptr, *part = nullptr, *pre_t = nullptr;
  if (hipMalloc((void**)&u, (wino4_weight_floats(cout, cin) + cin) * sizeof(float)) != hipSuccess)
    return fail(nullptr, FR_ERR_HIP, "frt_conv2d_winograd4_ex: allocation failed");
  pre_t = u + wino4_weight_floats(cout, cin);
  hipError_t e = hipMemcpy(pre_t, t.data(), cin * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = launch_wino4_weights(w, pre_scale, u, cout, cin, s);
  static int* frt_err = nullptr;  // this entry point's device error word (no handle to own one)
  if (e == hipSuccess && !frt_err) e = hipHostMalloc((void**)&frt_err, sizeof(int), hipHostMallocCoherent | hipHostMallocMapped);
  if (e == hipSuccess) *(volatile int*)frt_err = 0;
  if (e == hipSuccess) {
    Wino4Params p{};
    p.x = x;
    p.u = u;
    p.y = y;
    p.pre_t = pre_scale ? pre_t : nullptr;
    p.post_scale = post_scale;
    p.post_shift = post_shift;
    p.prelu = prelu;
    p.res = res;
    p.B = B;
    p.H = H;
    p.W = W;
    p.Cin = cin;
    p.Cout = cout;
    p.no_split = !g_frt_wino4_split;
    p.poll_max = g_knobs.wino4_poll > 0 ? g_knobs.wino4_poll : -1;
    p.err = frt_err;
    p.shapes = g_knobs.wino4_shapes;
    p.blk = blk;
    if (g_frt_wino4_split) {  // split-K partial slots (64 KiB each)
      p.part_floats = 257ll * 2 * 16 * 16 * 64;
      if (hipMalloc((void**)&part, p.part_floats * sizeof(float)) != hipSuccess) e = hipErrorOutOfMemory;
      p.part = part;
    }
    if (e == hipSuccess) e = launch_wino4(p, pre_scale != nullptr, (Epi)epi, s);
  }
  const hipError_t se = hipStreamSynchronize(s);
  (void)hipFree(u);
  (void)hipFree(part);
  if (e == hipSuccess) e = se;
  if (e != hipSuccess) return fail(nullptr, FR_ERR_HIP, std::string("frt_conv2d_winograd4_ex: ") + hipGetErrorString(e));
  if (*(volatile int*)frt_err & FR_DEVERR_W4_HANDOFF)
    return fail(nullptr, FR_ERR_HIP, "frt_conv2d_winograd4_ex: F(4x4) ring hand-off timed out in wino4_kernel");
  return FR_OK;
}

int frt_conv2d_winograd4(const float* x, const float* w, float* y, int B, int H, int W, int cin, int cout,
                         const float* pre_scale, const float* pre_shift, const float* post_scale,
                         const float* post_shift, const float* prelu, const float* res, int epi, void* stream) {
  return frt_conv2d_winograd4_ex(x, w, y, B, H, W, cin, cout, pre_scale, pre_shift, post_scale, post_shift, prelu, res,
                                 epi, 0, stream);
}

int frt_stem(const uint8_t* img, int B, const float* lut, const float* w27x64, const float* bn_scale,
             const float* bn_shift, const float* prelu, float* y, void* stream) {
  hipError_t e = launch_stem(img, B, lut, w27x64, bn_scale, bn_shift, prelu, y, (hipStream_t)stream);
  if (e != hipSuccess) return fail(nullptr, FR_ERR_HIP, std::string("frt_stem: ") + hipGetErrorString(e));
  return FR_OK;
}

int frt_head_reduce(const float* partial, int nsplit, long long split_stride, const float* fc_bias,
                    const float* bn_scale, const float* bn_shift, float* emb, int n, int normalize, int model_l2,
                    void* stream) {
  if (!partial || !fc_bias || !bn_scale || !bn_shift || !emb || n < 1 || nsplit < 1 ||
      split_stride < (long long)n * 512)
    return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "frt_head_reduce: bad arguments");
  const hipError_t e = launch_head_reduce(partial, nsplit, split_stride, fc_bias, bn_scale, bn_shift, emb, n,
                                          normalize != 0, model_l2 != 0, (hipStream_t)stream);
  if (e != hipSuccess) return fail(nullptr, FR_ERR_HIP, std::string("frt_head_reduce: ") + hipGetErrorString(e));
  return FR_OK;
}

int frt_fit_similarity(const float* src, const float* dst, int n, double* M) {
  if (n < 2 || n > 8) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "n in [2, 8]");
  return fit_similarity(src, dst, n, M) ? FR_OK : fail(nullptr, FR_ERR_INVALID_ARGUMENT, "similarity fit failed");
}

int frt_fit_similarity_device(const float* landmarks, int n, int out_size, double* M, uint8_t* ok, float* ms) {
  if (n < 1 || !landmarks || !M || !ok || out_size < 1)
    return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "frt_fit_similarity_device: bad arguments");
  const size_t lm_bytes = (size_t)n * 10 * sizeof(float), m_bytes = (size_t)n * 6 * sizeof(double);
  char* buf = nullptr;  // [maps | landmarks | ok]
  hipEvent_t ev[2] = {nullptr, nullptr};
  hipError_t e = hipMalloc((void**)&buf, m_bytes + lm_bytes + (size_t)n);
  if (e == hipSuccess) e = hipMemcpy(buf + m_bytes, landmarks, lm_bytes, hipMemcpyHostToDevice);
  FitSlots p{};
  p.n_frames = 1;
  p.landmarks = reinterpret_cast<const float*>(buf + m_bytes);
  p.stride = 10;
  p.max_faces = n;
  reference_template(out_size, p.tmpl);
  fit_logs(&p.logs);
  p.tforms = reinterpret_cast<double*>(buf);
  p.ok = reinterpret_cast<uint8_t*>(buf + m_bytes + lm_bytes);
  if (e == hipSuccess) e = launch_fit_similarity(p, nullptr);
  if (ms) {  // a second launch between two events: the first one also loaded the code object
    if (e == hipSuccess) e = hipEventCreate(&ev[0]);
    if (e == hipSuccess) e = hipEventCreate(&ev[1]);
    if (e == hipSuccess) e = hipEventRecord(ev[0], nullptr);
    if (e == hipSuccess) e = launch_fit_similarity(p, nullptr);
    if (e == hipSuccess) e = hipEventRecord(ev[1], nullptr);
    if (e == hipSuccess) e = hipEventSynchronize(ev[1]);
    if (e == hipSuccess) e = hipEventElapsedTime(ms, ev[0], ev[1]);
  }
  if (e == hipSuccess) e = hipMemcpy(M, p.tforms, m_bytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(ok, p.ok, (size_t)n, hipMemcpyDeviceToHost);
  for (hipEvent_t v : ev)
    if (v) (void)hipEventDestroy(v);
  (void)hipFree(buf);
  if (e != hipSuccess)
    return fail(nullptr, FR_ERR_HIP, std::string("frt_fit_similarity_device: ") + hipGetErrorString(e));
  return FR_OK;
}

int frt_warp_affine_images(const uint8_t* const* images, const int32_t* sizes, int n_images,
                           const int32_t* face_image, const double* tforms, int n_faces, int out_size, uint8_t* out,
                           void* stream) {
  // fr_align_images' checks and descriptors, the maps the caller's instead of fitted ones
  if (n_faces < 0 || n_images < 0 || out_size <= 0 || out_size > 1024 ||
      (n_faces > 0 && (!images || !sizes || !tforms || !face_image || !out)))
    return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "frt_warp_affine_images: bad arguments");
  if (n_faces == 0) return FR_OK;
  for (int i = 0; i < n_images; ++i)
    if (!images[i] || sizes[2 * i] <= 0 || sizes[2 * i + 1] <= 0)
      return fail(nullptr, FR_ERR_INVALID_ARGUMENT,
                  "frt_warp_affine_images: image " + std::to_string(i) + " is NULL or has a side < 1");
  std::vector<WarpFace> faces((size_t)n_faces);
  for (int f = 0; f < n_faces; ++f) {
    const int i = face_image[f];
    if (i < 0 || i >= n_images)
      return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "frt_warp_affine_images: face " + std::to_string(f) +
                                                        " names image " + std::to_string(i) + " of " +
                                                        std::to_string(n_images));
    faces[f].src = images[i];
    faces[f].H = sizes[2 * i];
    faces[f].W = sizes[2 * i + 1];
    invert_affine(tforms + (size_t)f * 6, faces[f].minv);
  }
  hipStream_t s = (hipStream_t)stream;
  const size_t bytes = faces.size() * sizeof(WarpFace);
  WarpFace* dev = nullptr;
  hipError_t e = hipMalloc((void**)&dev, bytes);
  if (e == hipSuccess) e = hipMemcpyAsync(dev, faces.data(), bytes, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = launch_warp_affine_images(dev, n_faces, out_size, out, s);
  const hipError_t es = hipStreamSynchronize(s);  // also before the free when a step failed
  if (e == hipSuccess) e = es;
  (void)hipFree(dev);
  if (e != hipSuccess)
    return fail(nullptr, FR_ERR_HIP, std::string("frt_warp_affine_images: ") + hipGetErrorString(e));
  return FR_OK;
}

namespace {
// What launch_letterbox / launch_letterbox_images refuse, asked before anything is staged.
bool letterbox_canvas_ok(int dw, int dh, const uint8_t* out) {
  return dw >= 1 && dh >= 1 && (dw * 3LL) % 4 == 0 && (long long)dh * dw * 3 < (1ll << 31) && out &&
         (reinterpret_cast<uintptr_t>(out) & 3) == 0;
}
}  // namespace

int frt_letterbox(const uint8_t* frames, int n, int H, int W, int new_w, int new_h, int dw, int dh, uint8_t* out,
                  void* stream) {
  if (n < 1 || !frames || H < 1 || W < 1 || new_w < 1 || new_h < 1 || new_w > dw || new_h > dh ||
      !letterbox_canvas_ok(dw, dh, out))
    return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "frt_letterbox: bad arguments");
  // setup_geometry's tables: [new_w][4] for x, then [new_h][4] for y
  std::vector<int> host((size_t)(new_w + new_h) * 4, 0);
  resize_axis_table(new_w, W, host.data());
  resize_axis_table(new_h, H, host.data() + 4 * new_w);
  hipStream_t s = (hipStream_t)stream;
  int* tabs = nullptr;
  hipError_t e = hipMalloc((void**)&tabs, host.size() * sizeof(int));
  if (e == hipSuccess) e = hipMemcpyAsync(tabs, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice, s);
  if (e == hipSuccess)
    e = launch_letterbox(frames, n, H, W, tabs, tabs + 4 * new_w, new_w, new_h, resize_simd_end(new_w * 3), dw, dh,
                         out, s);
  const hipError_t es = hipStreamSynchronize(s);
  if (e == hipSuccess) e = es;
  (void)hipFree(tabs);
  if (e == hipErrorInvalidValue) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "frt_letterbox: refused");
  if (e != hipSuccess) return fail(nullptr, FR_ERR_HIP, std::string("frt_letterbox: ") + hipGetErrorString(e));
  return FR_OK;
}

int frt_letterbox_images(const uint8_t* const* images, const int32_t* sizes, const int32_t* new_sizes, int n, int dw,
                         int dh, uint8_t* out, void* stream) {
  if (n < 1 || !images || !sizes || !new_sizes || !letterbox_canvas_ok(dw, dh, out))
    return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "frt_letterbox_images: bad arguments");
  size_t ints = 0;
  for (int i = 0; i < n; ++i) {
    const int new_h = new_sizes[2 * i], new_w = new_sizes[2 * i + 1];
    if (!images[i] || sizes[2 * i] < 1 || sizes[2 * i + 1] < 1 || new_w < 1 || new_h < 1 || new_w > dw || new_h > dh)
      return fail(nullptr, FR_ERR_INVALID_ARGUMENT,
                  "frt_letterbox_images: image " + std::to_string(i) + " is NULL or has a bad size");
    ints += (size_t)(new_w + new_h) * 4;
  }
  // letterbox_images' staging: [n] LetterboxImage | tables, image i's x table then its y table
  const size_t tab_off = (size_t)n * sizeof(LetterboxImage);
  std::vector<char> host(tab_off + ints * sizeof(int), 0);
  auto* im = reinterpret_cast<LetterboxImage*>(host.data());
  int* tabs = reinterpret_cast<int*>(host.data() + tab_off);
  int at = 0;
  for (int i = 0; i < n; ++i) {
    const int height = sizes[2 * i], width = sizes[2 * i + 1];
    const int new_h = new_sizes[2 * i], new_w = new_sizes[2 * i + 1];
    im[i] = LetterboxImage{images[i], width, new_w, new_h, resize_simd_end(new_w * 3), at, at + 4 * new_w};
    resize_axis_table(new_w, width, tabs + im[i].xtab);
    resize_axis_table(new_h, height, tabs + im[i].ytab);
    at += (new_w + new_h) * 4;
  }
  hipStream_t s = (hipStream_t)stream;
  char* dev = nullptr;
  hipError_t e = hipMalloc((void**)&dev, host.size());
  if (e == hipSuccess) e = hipMemcpyAsync(dev, host.data(), host.size(), hipMemcpyHostToDevice, s);
  if (e == hipSuccess)
    e = launch_letterbox_images(reinterpret_cast<const LetterboxImage*>(dev),
                                reinterpret_cast<const int*>(dev + tab_off), n, dw, dh, out, s);
  const hipError_t es = hipStreamSynchronize(s);
  if (e == hipSuccess) e = es;
  (void)hipFree(dev);
  if (e == hipErrorInvalidValue) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "frt_letterbox_images: refused");
  if (e != hipSuccess)
    return fail(nullptr, FR_ERR_HIP, std::string("frt_letterbox_images: ") + hipGetErrorString(e));
  return FR_OK;
}

int frt_resize_simd_end(int row_elems) { return resize_simd_end(row_elems); }

int frt_fit_images_by_value(void) { return FIT_IMAGES_BY_VALUE; }

int frt_resize_axis_table(int dsize, int ssize, int32_t* out) {
  if (dsize < 1 || ssize < 1 || !out) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "frt_resize_axis_table: bad arguments");
  resize_axis_table(dsize, ssize, out);
  return FR_OK;
}

int frt_resize_tables_device(int dsize, int ssize, int32_t* out) {
  if (dsize < 1 || ssize < 1 || dsize > (1 << 20) || !out)
    return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "frt_resize_tables_device: bad arguments");
  // one image whose x and y axes are both the axis asked for: the kernel's two branches
  LetterboxChunk c{};
  c.im[0] = LetterboxImage{nullptr, ssize, dsize, dsize, 0, 0, 4 * dsize};
  c.H[0] = ssize;
  const size_t ints = (size_t)dsize * 8;
  std::vector<int> host(ints);
  int* tabs = nullptr;
  hipError_t e = hipMalloc((void**)&tabs, ints * sizeof(int));
  if (e == hipSuccess) e = launch_resize_tables(c, 1, tabs, (long long)ints, nullptr, nullptr, nullptr);
  if (e == hipSuccess) e = hipMemcpy(host.data(), tabs, ints * sizeof(int), hipMemcpyDeviceToHost);
  (void)hipFree(tabs);
  if (e == hipErrorInvalidValue) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "frt_resize_tables_device: refused");
  if (e != hipSuccess)
    return fail(nullptr, FR_ERR_HIP, std::string("frt_resize_tables_device: ") + hipGetErrorString(e));
  if (memcmp(host.data(), host.data() + 4 * (size_t)dsize, 4 * (size_t)dsize * sizeof(int)))
    return fail(nullptr, FR_ERR_STATE, "frt_resize_tables_device: the x and y tables of one axis differ");
  memcpy(out, host.data(), 4 * (size_t)dsize * sizeof(int));
  return FR_OK;
}

int frt_quality_gate_host(const float* dets, const int32_t* counts, const uint8_t* ok, const double* blur,
                          int n_frames, int max_faces, const fr_gate_config* cfg, uint8_t* stage, double* metrics,
                          int32_t* bbox, int32_t* rank, int32_t* rows, int32_t* frame_offsets, int32_t* valid_slots,
                          int32_t* n_valid) {
  const int F = max_faces;
  if (n_frames < 0 || F < 1 || F > FR_GATE_MAX_FACES || (long long)n_frames * F >= (1ll << 31) || !cfg)
    return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "frt_quality_gate_host: bad n_frames / max_faces / config");
  GateLimits lim;
  if (!gate_limits(*cfg, blur != nullptr, &lim))
    return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "frt_quality_gate_host: a limit is not finite or beyond +-FLT_MAX");
  if (n_frames == 0) return FR_OK;
  if (!dets || !stage || !metrics || !bbox || !rank || !rows || !frame_offsets || !valid_slots || !n_valid)
    return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "frt_quality_gate_host: NULL buffer");
  std::vector<double> key((size_t)F);
  int total = 0, n_ok = 0;
  for (int f = 0; f < n_frames; ++f) {
    const int live = gate_live(counts, f, F);
    const size_t base = (size_t)f * F;
    for (int i = 0; i < F; ++i) {
      const size_t slot = base + i;
      GateSlot r{};
      if (i < live) {
        r = gate_slot(dets + slot * 15, ok ? ok[slot] : 1, lim.check_blur ? blur[slot] : 0.0, lim);
        key[i] = r.key;
      } else {
        r.stage = FR_GATE_NOT_LIVE;
        rank[slot] = -1;
      }
      stage[slot] = (uint8_t)r.stage;
      const double m[5] = {r.det_score, r.blur_score, r.yaw, r.pitch, r.roll};
      std::copy(m, m + 5, metrics + slot * 5);
      const int32_t b[4] = {r.x0, r.y0, r.x1, r.y1};
      std::copy(b, b + 4, bbox + slot * 4);
    }
    frame_offsets[f] = total;
    for (int i = 0; i < live; ++i) {
      int before = 0;
      for (int j = 0; j < live; ++j) before += gate_before(key[j], j, key[i], i);
      rank[base + i] = before;
      rows[total + before] = (int32_t)(base + i);
    }
    for (int r = 0; r < live; ++r) {  // rows of this frame are complete: the valid ones in rows order
      const int32_t slot = rows[total + r];
      if (stage[slot] == FR_GATE_VALID) valid_slots[n_ok++] = slot;
    }
    total += live;
  }
  frame_offsets[n_frames] = total;
  n_valid[0] = n_ok;
  std::fill(rows + total, rows + (size_t)n_frames * F, -1);
  std::fill(valid_slots + n_ok, valid_slots + (size_t)n_frames * F, -1);
  return FR_OK;
}

int frt_detector_forward(fr_handle* h, const uint8_t* frames, int n, int height, int width, float* heads,
                         uint8_t* canvas, void* stream) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (!h->detector || !h->finalized) return fail(h, FR_ERR_STATE, "not a finalised detector handle");
  if (n < 1 || !frames || !heads || height < 2 || width < 2) return fail(h, FR_ERR_INVALID_ARGUMENT, "bad arguments");
  DeviceGuard dg(h->device);
  return detector_forward(h, frames, n, height, width, heads, canvas, (hipStream_t)stream);
}

int frt_detector_forward_images(fr_handle* h, const uint8_t* const* images, const int32_t* sizes, int n, float* heads,
                                uint8_t* canvas, void* stream) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (!h->detector || !h->finalized) return fail(h, FR_ERR_STATE, "not a finalised detector handle");
  if (n < 1 || !images || !sizes || !heads) return fail(h, FR_ERR_INVALID_ARGUMENT, "bad arguments");
  DeviceGuard dg(h->device);
  return detector_forward_images(h, images, sizes, n, heads, canvas, (hipStream_t)stream);
}

int frt_set_detector_row_reduction(fr_handle* h, int on) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (!h->detector || !h->det) return fail(h, FR_ERR_STATE, "not a finalised detector handle");
  detector_set_row_reduction(h->det, on != 0);
  return FR_OK;
}

int frt_maxpool3(const float* x, int B, int H, int W, int C, float* y, void* stream) {
  if (B < 1 || H < 1 || W < 1 || C < 4 || !x || !y)
    return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "frt_maxpool3: bad arguments");
  const hipError_t e = launch_maxpool3(x, B, H, W, C, y, (hipStream_t)stream);
  if (e != hipSuccess) return fail(nullptr, FR_ERR_HIP, std::string("frt_maxpool3: ") + hipGetErrorString(e));
  return FR_OK;
}

int frt_upsample_add(float* big, const float* small, int B, int h, int w, int C, void* stream) {
  if (B < 1 || h < 1 || w < 1 || C < 4 || !big || !small)
    return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "frt_upsample_add: bad arguments");
  const hipError_t e = launch_upsample_add(big, small, B, h, w, C, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "frt_upsample_add: refused");
  if (e != hipSuccess) return fail(nullptr, FR_ERR_HIP, std::string("frt_upsample_add: ") + hipGetErrorString(e));
  return FR_OK;
}

int frt_avgpool2(const float* x, int B, int H, int W, int C, float* y, void* stream) {
  if (B < 1 || H < 2 || W < 2 || C < 4 || !x || !y ||
      ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15))
    return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "frt_avgpool2: bad arguments");
  const hipError_t e = launch_avgpool2(x, B, H, W, C, y, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "frt_avgpool2: refused");
  if (e != hipSuccess) return fail(nullptr, FR_ERR_HIP, std::string("frt_avgpool2: ") + hipGetErrorString(e));
  return FR_OK;
}

int frt_row_expand(const float* x, int B, int Hs, int W, int C, int m, int Hd, float* y, void* stream) {
  if (B < 1 || W < 1 || C < 4 || !x || !y || ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15))
    return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "frt_row_expand: bad arguments");
  const hipError_t e = launch_row_expand(x, B, Hs, W, C, m, Hd, y, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "frt_row_expand: refused");
  if (e != hipSuccess) return fail(nullptr, FR_ERR_HIP, std::string("frt_row_expand: ") + hipGetErrorString(e));
  return FR_OK;
}

int frt_det_stem(const uint8_t* img, int B, int H, int W, int C, const float* w27xC, const float* scale,
                 const float* shift, float* y, int force_scalar, void* stream) {
  if (B < 1 || !img || !w27xC || !scale || !shift || !y || (reinterpret_cast<uintptr_t>(y) & 15) ||
      (reinterpret_cast<uintptr_t>(img) & 3))
    return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "frt_det_stem: bad arguments");
  const hipError_t e =
      launch_det_stem(img, B, H, W, C, w27xC, scale, shift, y, (hipStream_t)stream, force_scalar != 0);
  if (e == hipErrorInvalidValue) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "frt_det_stem: refused");
  if (e != hipSuccess) return fail(nullptr, FR_ERR_HIP, std::string("frt_det_stem: ") + hipGetErrorString(e));
  return FR_OK;
}

int frt_detector_postprocess(fr_handle* h, const float* heads, int n, float det_scale, const float* det_scales,
                             float det_thresh, int max_faces, float* dets, int32_t* counts, void* stream) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (!h->detector || !h->finalized) return fail(h, FR_ERR_STATE, "not a finalised detector handle");
  if (n < 1 || !heads || !counts || max_faces < 0 || (max_faces > 0 && !dets))
    return fail(h, FR_ERR_INVALID_ARGUMENT, "bad arguments");
  DeviceGuard dg(h->device);
  return detector_postprocess(h, heads, n, det_scale, det_scales, det_thresh, max_faces, dets, counts,
                              (hipStream_t)stream);
}

int frt_topk_ex(const float* scores, int n, int G, int k, int low_index_first, int32_t* idx, float* val,
                void* stream) {
  if (k < 1 || k > G) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "frt_topk: k must be in [1, G]");
  hipError_t e = launch_topk(scores, n, G, k, idx, val, (hipStream_t)stream, low_index_first != 0);
  if (e != hipSuccess) return fail(nullptr, FR_ERR_HIP, std::string("frt_topk: ") + hipGetErrorString(e));
  return FR_OK;
}

int frt_topk(const float* scores, int n, int G, int k, int32_t* idx, float* val, void* stream) {
  return frt_topk_ex(scores, n, G, k, 0, idx, val, stream);
}

}  // extern "C"
