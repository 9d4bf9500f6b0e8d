// libfrhip public C API (include/frhip.h): argument checks, the handle's lock and device, and
// calls into the runtime's other translation units (runtime.h lists them; their headers name the
// reference code each replaces): the model, gallery-row, match, align, detect, settings and
// profiling calls.  The calls over CSR batches are in batch_ops.cpp.  The gallery rows kept in
// HBM here replace
//   GalleryManager.get_gallery_embeddings   gallery_manager.py:177-187 (A10)
#include <algorithm>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "gate_math.h"
#include "runtime.h"

using namespace frhip;
using namespace frhip_rt;

extern "C" {

int fr_create(const char* architecture, const char* model_type, int device, int max_batch, fr_handle** out) {
  if (!out) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "out is NULL");
  *out = nullptr;
  const std::string arch = architecture ? architecture : "";
  const std::string mt = model_type ? model_type : "";
  const bool detector = arch == "scrfd_10g";
  bool ok = detector;
  auto specs = detector ? std::vector<BlockSpec>{} : block_specs(arch, &ok);
  if (!ok)
    return fail(nullptr, FR_ERR_INVALID_ARGUMENT,
                "Unknown architecture: " + arch + ". Available: ['ir_50', 'ir_101', 'scrfd_10g']");
  if (detector ? mt != "scrfd" : (mt != "adaface" && mt != "arcface"))
    return fail(nullptr, FR_ERR_INVALID_ARGUMENT,
                "Unknown model_type: " + mt + (detector ? ". scrfd_10g takes 'scrfd'" : ". Must be 'adaface' or 'arcface'"));
  if (max_batch < 1 || max_batch > 512)
    return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "max_batch must be in [1, 512]");
  if (detector && max_batch > 64)
    return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "scrfd_10g: max_batch (frames per forward) must be in [1, 64]");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(nullptr, FR_ERR_HIP, "no HIP device available");
  if (device < 0 || device >= ndev) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "device index out of range");
  auto h = std::make_unique<fr_handle>();
  h->arch = arch;
  h->model_type = mt;
  h->arcface = mt == "arcface";
  h->device = device;
  h->max_batch = max_batch;
  h->lane_min = detector ? 0 : FR_LANES_MIN_DEFAULT;
  h->lane_max = FR_LANES_MAX_DEFAULT;
  h->specs = specs;
  h->detector = detector;
  h->expected = detector ? detector_schema() : embedder_schema(h->arcface, specs);
  *out = h.release();
  return FR_OK;
}

int fr_destroy(fr_handle* h) {
  if (!h) return FR_OK;
  {
    DeviceGuard g(h->device);
    (void)hipDeviceSynchronize();
    delete h;
  }
  return FR_OK;
}

int fr_set_param(fr_handle* h, const char* name, const float* host_data, int64_t numel) {
  if (!h || !name) return fail(h, FR_ERR_INVALID_ARGUMENT, "NULL argument");
  std::lock_guard<std::mutex> lk(h->mu);
  const std::string k = name;
  auto it = h->expected.find(k);
  if (it == h->expected.end()) return fail(h, FR_ERR_INVALID_ARGUMENT, "Unexpected key(s) in state_dict: \"" + k + "\"");
  if (k.size() > 20 && k.compare(k.size() - 20, 20, ".num_batches_tracked") == 0) return FR_OK;
  if (numel != (int64_t)it->second || (!host_data && numel > 0))
    return fail(h, FR_ERR_INVALID_ARGUMENT,
                "size mismatch for " + k + ": expected " + std::to_string(it->second) + " elements, got " +
                    std::to_string(numel));
  h->params[k].assign(host_data, host_data + numel);
  h->finalized = false;
  return FR_OK;
}

int fr_finalize(fr_handle* h) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  std::string missing;
  for (const auto& kv : h->expected) {
    if (kv.first.size() > 20 && kv.first.compare(kv.first.size() - 20, 20, ".num_batches_tracked") == 0) continue;
    if (!h->params.count(kv.first)) missing += (missing.empty() ? "\"" : ", \"") + kv.first + "\"";
  }
  if (!missing.empty()) return fail(h, FR_ERR_MISSING_PARAM, "Missing key(s) in state_dict: " + missing);
  DeviceGuard dg(h->device);
  return finalize_model(h);
}

int fr_embed(fr_handle* h, const uint8_t* rgb, int n, int height, int width, float* out, int normalize,
             void* stream) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (h->detector) return fail(h, FR_ERR_STATE, "this handle is a detector (scrfd_10g); use fr_detect");
  if (!h->finalized) return fail(h, FR_ERR_STATE, "model not finalised (fr_finalize)");
  if (int rc = check_crop_size(h, height, width)) return rc;
  if (n < 0 || (n > 0 && (!rgb || !out))) return fail(h, FR_ERR_INVALID_ARGUMENT, "bad n or NULL buffer");
  if (int rc = check_dev_err(h)) return rc;  // reported by earlier asynchronous work
  DeviceGuard dg(h->device);
  return embed_any(h, rgb, n, height, width, out, normalize, (hipStream_t)stream);
}

int fr_resize_crops(fr_handle* h, const uint8_t* src, int n, int height, int width, uint8_t* dst, void* stream) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = check_crop_size(h, height, width)) return rc;
  if (n < 0 || (n > 0 && (!src || !dst))) return fail(h, FR_ERR_INVALID_ARGUMENT, "bad n or NULL buffer");
  if (n == 0) return FR_OK;
  DeviceGuard dg(h->device);
  return resize_device(h, src, n, height, width, dst, (hipStream_t)stream);
}

int fr_resize_images(fr_handle* h, const uint8_t* const* images, const int32_t* sizes, int n, uint8_t* dst,
                     void* stream) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (n < 0 || (n > 0 && (!images || !sizes || !dst)))
    return fail(h, FR_ERR_INVALID_ARGUMENT, "bad n or NULL images / sizes / dst");
  if (n == 0) return FR_OK;
  if (int rc = check_images(h, images, sizes, n)) return rc;
  DeviceGuard dg(h->device);
  return resize_images(h, images, sizes, n, dst, (hipStream_t)stream);
}

int fr_embed_images(fr_handle* h, const uint8_t* const* images, const int32_t* sizes, int n, float* out,
                    int normalize, void* stream) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (h->detector) return fail(h, FR_ERR_STATE, "this handle is a detector (scrfd_10g); use fr_detect");
  if (!h->finalized) return fail(h, FR_ERR_STATE, "model not finalised (fr_finalize)");
  if (n < 0 || (n > 0 && (!images || !sizes || !out)))
    return fail(h, FR_ERR_INVALID_ARGUMENT, "bad n or NULL images / sizes / out");
  if (n == 0) return FR_OK;
  if (int rc = check_images(h, images, sizes, n)) return rc;
  if (int rc = check_dev_err(h)) return rc;  // reported by earlier asynchronous work
  DeviceGuard dg(h->device);
  return embed_images(h, images, sizes, n, out, normalize, (hipStream_t)stream);
}

int fr_augment_faces(fr_handle* h, const uint8_t* crops, int n, int height, int width, int num_augmentations,
                     uint8_t* out, void* stream) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = check_crop_size(h, height, width)) return rc;
  if (num_augmentations > FR_AUGMENT_MAX && num_augmentations <= 16)
    return fail(h, FR_ERR_UNSUPPORTED,
                "num_augmentations 15 and 16 (cv2.GaussianBlur and the unseeded np.random.normal noise) are not "
                "implemented; at most " + std::to_string(FR_AUGMENT_MAX));
  if (num_augmentations < 1 || num_augmentations > FR_AUGMENT_MAX)
    return fail(h, FR_ERR_INVALID_ARGUMENT, "num_augmentations must be in [1, " + std::to_string(FR_AUGMENT_MAX) + "]");
  if (n < 0 || (n > 0 && (!crops || !out))) return fail(h, FR_ERR_INVALID_ARGUMENT, "bad n or NULL buffer");
  if (n == 0) return FR_OK;
  const size_t in_bytes = (size_t)n * height * width * 3, out_bytes = in_bytes * num_augmentations;
  const uintptr_t ci = (uintptr_t)crops, oi = (uintptr_t)out;
  if (ci < oi + out_bytes && oi < ci + in_bytes) return fail(h, FR_ERR_INVALID_ARGUMENT, "out overlaps crops");
  DeviceGuard dg(h->device);
  AugTables tab;
  augment_tables(height, width, &tab);
  const hipError_t e = launch_augment(crops, n, height, width, num_augmentations, tab, out, (hipStream_t)stream);
  if (e != hipSuccess) return launch_fail(h, "augment", e);
  return FR_OK;
}

int fr_embed_host(fr_handle* h, const uint8_t* rgb, int n, int height, int width, float* out, int normalize) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (h->detector) return fail(h, FR_ERR_STATE, "this handle is a detector (scrfd_10g); use fr_detect");
  if (!h->finalized) return fail(h, FR_ERR_STATE, "model not finalised (fr_finalize)");
  if (int rc = check_crop_size(h, height, width)) return rc;
  if (n < 0 || (n > 0 && (!rgb || !out))) return fail(h, FR_ERR_INVALID_ARGUMENT, "bad n or NULL buffer");
  DeviceGuard dg(h->device);
  hipStream_t s = nullptr;
  const size_t crop = (size_t)height * width * 3;
  for (int off = 0; off < n; off += h->max_batch) {
    const int bn = std::min(h->max_batch, n - off);
    if (height == 112 && width == 112) {
      FR_HIP(h, hipMemcpyAsync(h->in_stage, rgb + (size_t)off * crop, (size_t)bn * crop, hipMemcpyHostToDevice, s));
    } else {  // raw crops to the device, then cv2.resize to 112 x 112 into the forward's input
      int rc = ensure_buf(h, &h->rs_src, &h->rs_src_cap, (size_t)bn * crop);
      if (rc) return rc;
      FR_HIP(h, hipMemcpyAsync(h->rs_src, rgb + (size_t)off * crop, (size_t)bn * crop, hipMemcpyHostToDevice, s));
      rc = resize_device(h, static_cast<const uint8_t*>(h->rs_src), bn, height, width, h->in_stage, s);
      if (rc) return rc;
    }
    int rc = forward_staged(h, bn, normalize, s);
    if (rc) return rc;
    FR_HIP(h, hipMemcpyAsync(out + (size_t)off * 512, h->emb_stage, (size_t)bn * 512 * sizeof(float),
                             hipMemcpyDeviceToHost, s));
  }
  FR_HIP(h, hipStreamSynchronize(s));
  return check_dev_err(h);
}

int fr_gallery_set(fr_handle* h, const float* E, int G, int D, int src_is_device, void* stream) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (G < 0 || (G > 0 && !E)) return fail(h, FR_ERR_INVALID_ARGUMENT, "bad gallery");
  if (G > 0 && D != 512) return fail(h, FR_ERR_INVALID_ARGUMENT, "gallery rows must be 512-d");
  DeviceGuard dg(h->device);
  hipStream_t s = (hipStream_t)stream;
  if (G == 0) {
    h->G = 0;
    return FR_OK;
  }
  void* p = h->gallery;
  int rc = ensure_buf(h, &p, &h->gallery_cap, (size_t)G * 512 * sizeof(float));
  h->gallery = (float*)p;
  if (rc) return rc;
  FR_HIP(h, hipMemcpyAsync(h->gallery, E, (size_t)G * 512 * sizeof(float),
                           src_is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
  if (!src_is_device) FR_HIP(h, hipStreamSynchronize(s));
  h->G = G;
  return FR_OK;
}

int fr_gallery_write_rows(fr_handle* h, int row0, int n, const float* E, int src_is_device, void* stream) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (n < 0 || row0 < 0 || row0 > h->G || (n > 0 && !E))
    return fail(h, FR_ERR_INVALID_ARGUMENT, "rows must satisfy 0 <= row0 <= G, n >= 0");
  if (n == 0) return FR_OK;
  DeviceGuard dg(h->device);
  hipStream_t s = (hipStream_t)stream;
  const int G2 = std::max(h->G, row0 + n);
  int rc = gallery_reserve(h, G2, s);
  if (rc) return rc;
  FR_HIP(h, hipMemcpyAsync(h->gallery + (size_t)row0 * 512, E, (size_t)n * 512 * sizeof(float),
                           src_is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
  if (!src_is_device) FR_HIP(h, hipStreamSynchronize(s));
  h->G = G2;
  return FR_OK;
}

int fr_gallery_delete_rows(fr_handle* h, int row0, int n, void* stream) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (n < 0 || row0 < 0 || row0 + n > h->G) return fail(h, FR_ERR_INVALID_ARGUMENT, "rows out of range");
  if (n == 0) return FR_OK;
  DeviceGuard dg(h->device);
  hipStream_t s = (hipStream_t)stream;
  const size_t tail = (size_t)(h->G - row0 - n) * 512 * sizeof(float);
  if (tail > 0) {
    int rc = ensure_buf(h, &h->gallery_tmp, &h->gallery_tmp_cap, tail);
    if (rc) return rc;
    float* src = h->gallery + (size_t)(row0 + n) * 512;
    FR_HIP(h, hipMemcpyAsync(h->gallery_tmp, src, tail, hipMemcpyDeviceToDevice, s));
    FR_HIP(h, hipMemcpyAsync(h->gallery + (size_t)row0 * 512, h->gallery_tmp, tail, hipMemcpyDeviceToDevice, s));
  }
  h->G -= n;
  return FR_OK;
}

int fr_gallery_read(fr_handle* h, int row0, int n, float* out, int dst_is_device, void* stream) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (n < 0 || row0 < 0 || row0 + n > h->G || (n > 0 && !out))
    return fail(h, FR_ERR_INVALID_ARGUMENT, "rows out of range");
  if (n == 0) return FR_OK;
  DeviceGuard dg(h->device);
  hipStream_t s = (hipStream_t)stream;
  FR_HIP(h, hipMemcpyAsync(out, h->gallery + (size_t)row0 * 512, (size_t)n * 512 * sizeof(float),
                           dst_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
  if (!dst_is_device) FR_HIP(h, hipStreamSynchronize(s));
  return FR_OK;
}

int fr_gallery_size(fr_handle* h, int* G) {
  if (!h || !G) return fail(h, FR_ERR_INVALID_ARGUMENT, "NULL argument");
  std::lock_guard<std::mutex> lk(h->mu);
  *G = h->G;
  return FR_OK;
}

int fr_match_topk(fr_handle* h, const float* Q, int n, int k, int32_t* idx, float* score, void* stream) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (n < 0 || (n > 0 && (!Q || !idx || !score))) return fail(h, FR_ERR_INVALID_ARGUMENT, "bad n or NULL buffer");
  if (int rc = check_dev_err(h)) return rc;
  DeviceGuard dg(h->device);
  return match_device(h, Q, n, k, idx, score, (hipStream_t)stream);
}

int fr_match_topk_host(fr_handle* h, const float* Q, int n, int k, int32_t* idx, float* score) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (n < 0 || (n > 0 && (!Q || !idx || !score))) return fail(h, FR_ERR_INVALID_ARGUMENT, "bad n or NULL buffer");
  if (n == 0) return FR_OK;
  if (k < 1 || k > h->G) return fail(h, FR_ERR_INVALID_ARGUMENT, "k must be in [1, G]");
  DeviceGuard dg(h->device);
  hipStream_t s = nullptr;
  const size_t qb = (size_t)n * 512 * sizeof(float), rb = (size_t)n * k * 4;
  int rc = ensure_buf(h, &h->match_io, &h->match_io_cap, qb + 2 * rb);
  if (rc) return rc;
  char* base = (char*)h->match_io;
  float* dq = (float*)base;
  int32_t* di = (int32_t*)(base + qb);
  float* ds = (float*)(base + qb + rb);
  FR_HIP(h, hipMemcpyAsync(dq, Q, qb, hipMemcpyHostToDevice, s));
  rc = match_device(h, dq, n, k, di, ds, s);
  if (rc) return rc;
  FR_HIP(h, hipMemcpyAsync(idx, di, rb, hipMemcpyDeviceToHost, s));
  FR_HIP(h, hipMemcpyAsync(score, ds, rb, hipMemcpyDeviceToHost, s));
  FR_HIP(h, hipStreamSynchronize(s));
  return check_dev_err(h);
}

int fr_embed_match(fr_handle* h, const uint8_t* rgb, int n, int k, int32_t* idx, float* score, float* emb_out,
                   void* stream) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (h->detector) return fail(h, FR_ERR_STATE, "this handle is a detector (scrfd_10g); use fr_detect");
  if (!h->finalized) return fail(h, FR_ERR_STATE, "model not finalised (fr_finalize)");
  if (n < 0 || (n > 0 && (!rgb || !idx || !score))) return fail(h, FR_ERR_INVALID_ARGUMENT, "bad n or NULL buffer");
  if (h->G <= 0) return fail(h, FR_ERR_STATE, "gallery is empty (fr_gallery_set first)");
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
  return match_device(h, emb, n, k, idx, score, s);
}

int fr_align_faces(fr_handle* h, const uint8_t* frame, int height, int width, const float* landmarks, int n,
                   int out_size, uint8_t* out, double* tforms, void* stream) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::vector<double> fits;
  {
    std::lock_guard<std::mutex> lk(h->mu);
    if (n < 0 || height <= 0 || width <= 0 || out_size <= 0 || out_size > 1024 ||
        (n > 0 && (!frame || !landmarks || !out)))
      return fail(h, FR_ERR_INVALID_ARGUMENT, "bad alignment arguments");
    if (n == 0) return FR_OK;
    float tmpl[10];
    reference_template(out_size, tmpl);
    fits.resize((size_t)n * 6);
    for (int f = 0; f < n; ++f) {
      double* Mf = &fits[(size_t)f * 6];
      if (!fit_similarity(landmarks + (size_t)f * 10, tmpl, 5, Mf))
        // cv2.estimateAffinePartial2D returns None here and the reference's warpAffine raises
        return fail(h, FR_ERR_INVALID_ARGUMENT, "similarity fit failed for face " + std::to_string(f));
      if (tforms) memcpy(tforms + (size_t)f * 6, Mf, 6 * sizeof(double));
    }
  }
  // the warp by the fitted maps is fr_warp_affine (which takes the handle's lock itself)
  return fr_warp_affine(h, frame, height, width, fits.data(), n, out_size, out, stream);
}

int fr_warp_affine(fr_handle* h, const uint8_t* frame, int height, int width, const double* tforms, int n,
                   int out_size, uint8_t* out, void* stream) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (n < 0 || height <= 0 || width <= 0 || out_size <= 0 || out_size > 1024 ||
      (n > 0 && (!frame || !tforms || !out)))
    return fail(h, FR_ERR_INVALID_ARGUMENT, "bad warp arguments");
  if (n == 0) return FR_OK;
  DeviceGuard dg(h->device);
  std::vector<double> minv((size_t)n * 6);
  for (int f = 0; f < n; ++f) invert_affine(tforms + (size_t)f * 6, &minv[(size_t)f * 6]);
  hipStream_t s = (hipStream_t)stream;
  if (n <= WARP_MAPS_BY_VALUE) {  // maps in the kernel arguments: no copy, no sync
    const hipError_t e = launch_warp_affine_by_value(frame, height, width, minv.data(), n, out_size, out, s);
    if (e != hipSuccess) return launch_fail(h, "warp", e);
    return FR_OK;
  }
  int rc = ensure_buf(h, &h->align_m, &h->align_m_cap, minv.size() * sizeof(double));
  if (rc) return rc;
  FR_HIP(h, hipMemcpyAsync(h->align_m, minv.data(), minv.size() * sizeof(double), hipMemcpyHostToDevice, s));
  hipError_t e = launch_warp_affine(frame, height, width, (const double*)h->align_m, n, out_size, out, s);
  if (e != hipSuccess) return launch_fail(h, "warp", e);
  FR_HIP(h, hipStreamSynchronize(s));
  return FR_OK;
}

namespace {
// The blur launches of n checked images into var (device double [n]), under the handle's lock and
// device: what fr_blur_scores and fr_blur_scores_device share.  Asynchronous.
int blur_device(fr_handle* h, const uint8_t* crops, int n, int height, int width, int channels, double* var,
                hipStream_t s) {
  const size_t img = (size_t)height * width * channels;
  const int per = 65535;  // images per launch (grid y of the multi-block form)
  const size_t ws = blur_workspace_bytes(std::min(n, per), height, width);
  if (ws)
    if (int rc = ensure_buf(h, &h->blur_ws, &h->blur_ws_cap, ws)) return rc;
  for (int off = 0; off < n; off += per) {
    const int m = std::min(per, n - off);
    const hipError_t e = launch_blur(crops + (size_t)off * img, m, height, width, channels, var + off, h->blur_ws, s);
    if (e != hipSuccess) return launch_fail(h, "blur", e);
  }
  return FR_OK;
}

bool blur_args_ok(const uint8_t* crops, int n, int height, int width, int channels, const double* scores) {
  return n >= 0 && height >= 1 && width >= 1 && (long long)height * width < (1ll << 31) &&
         (channels == 1 || channels == 3 || channels == 4) && (n == 0 || (crops && scores));
}
}  // namespace

int fr_blur_scores(fr_handle* h, const uint8_t* crops, int n, int height, int width, int channels, double* scores,
                   void* stream) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (!blur_args_ok(crops, n, height, width, channels, scores))
    return fail(h, FR_ERR_INVALID_ARGUMENT, "bad blur arguments (height, width >= 1; channels 1, 3 or 4)");
  if (n == 0) return FR_OK;
  DeviceGuard dg(h->device);
  int rc = ensure_buf(h, &h->blur_out, &h->blur_out_cap, (size_t)n * sizeof(double));
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  if ((rc = blur_device(h, crops, n, height, width, channels, (double*)h->blur_out, s))) return rc;
  FR_HIP(h, hipMemcpyAsync(scores, h->blur_out, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
  FR_HIP(h, hipStreamSynchronize(s));
  return check_dev_err(h);
}

int fr_detect(fr_handle* h, const uint8_t* frames, int n, int height, int width, float det_thresh, int max_faces,
              float* dets, int32_t* counts, void* stream) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (!h->detector) return fail(h, FR_ERR_STATE, "not a detector handle (fr_create(\"scrfd_10g\", \"scrfd\", ...))");
  if (!h->finalized) return fail(h, FR_ERR_STATE, "model not finalised (fr_finalize)");
  if (n < 0 || (n > 0 && (!frames || !counts || (max_faces > 0 && !dets))) || height < 2 || width < 2 ||
      max_faces < 0)
    return fail(h, FR_ERR_INVALID_ARGUMENT, "bad frames / sizes / output buffers");
  if (n == 0) return FR_OK;
  DeviceGuard dg(h->device);
  if (int rc = detector_run(h, frames, n, height, width, det_thresh, max_faces, dets, counts, (hipStream_t)stream))
    return rc;
  return check_dev_err(h);  // detector_run synchronised its stream
}

int fr_detect_images(fr_handle* h, const uint8_t* const* images, const int32_t* sizes, int n, float det_thresh,
                     int max_faces, float* dets, int32_t* counts, void* stream) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (!h->detector) return fail(h, FR_ERR_STATE, "not a detector handle (fr_create(\"scrfd_10g\", \"scrfd\", ...))");
  if (!h->finalized) return fail(h, FR_ERR_STATE, "model not finalised (fr_finalize)");
  if (max_faces < 1) return fail(h, FR_ERR_INVALID_ARGUMENT, "max_faces must be at least 1");
  if (n < 0 || (n > 0 && (!images || !sizes || !dets || !counts)))
    return fail(h, FR_ERR_INVALID_ARGUMENT, "bad n or NULL images / sizes / output buffers");
  if (n == 0) return FR_OK;
  DeviceGuard dg(h->device);
  if (int rc = detector_run_images(h, images, sizes, n, det_thresh, max_faces, dets, counts, (hipStream_t)stream))
    return rc;
  return check_dev_err(h);  // detector_run_images synchronised its stream
}

int fr_align_images(fr_handle* h, const uint8_t* const* images, const int32_t* sizes, int n_images,
                    const float* landmarks, const int32_t* face_image, int n_faces, int out_size, uint8_t* out,
                    double* tforms, void* stream) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (n_faces < 0 || n_images < 0 || out_size <= 0 || out_size > 1024 ||
      (n_faces > 0 && (!images || !sizes || !landmarks || !face_image || !out)))
    return fail(h, FR_ERR_INVALID_ARGUMENT, "bad alignment arguments");
  if (n_faces == 0) return FR_OK;
  for (int i = 0; i < n_images; ++i)
    if (!images[i] || sizes[2 * i] <= 0 || sizes[2 * i + 1] <= 0)
      return fail(h, FR_ERR_INVALID_ARGUMENT, "image " + std::to_string(i) + " is NULL or has a side < 1");
  float tmpl[10];
  reference_template(out_size, tmpl);
  std::vector<WarpFace> faces((size_t)n_faces);
  for (int f = 0; f < n_faces; ++f) {
    const int i = face_image[f];
    if (i < 0 || i >= n_images)
      return fail(h, FR_ERR_INVALID_ARGUMENT,
                  "face " + std::to_string(f) + " names image " + std::to_string(i) + " of " + std::to_string(n_images));
    double Mf[6];
    if (!fit_similarity(landmarks + (size_t)f * 10, tmpl, 5, Mf))
      return fail(h, FR_ERR_INVALID_ARGUMENT, "similarity fit failed for face " + std::to_string(f));
    if (tforms) memcpy(tforms + (size_t)f * 6, Mf, 6 * sizeof(double));
    faces[f].src = images[i];
    faces[f].H = sizes[2 * i];
    faces[f].W = sizes[2 * i + 1];
    invert_affine(Mf, faces[f].minv);
  }
  DeviceGuard dg(h->device);
  const size_t bytes = faces.size() * sizeof(WarpFace);
  int rc = ensure_buf(h, &h->align_m, &h->align_m_cap, bytes);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  FR_HIP(h, hipMemcpyAsync(h->align_m, faces.data(), bytes, hipMemcpyHostToDevice, s));
  const hipError_t e = launch_warp_affine_images((const WarpFace*)h->align_m, n_faces, out_size, out, s);
  if (e != hipSuccess) return launch_fail(h, "warp", e);
  FR_HIP(h, hipStreamSynchronize(s));
  return FR_OK;
}

int fr_detect_device(fr_handle* h, const uint8_t* frames, int n, int height, int width, float det_thresh,
                     int max_faces, float* dets, int32_t* counts, void* stream) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (!h->detector) return fail(h, FR_ERR_STATE, "not a detector handle (fr_create(\"scrfd_10g\", \"scrfd\", ...))");
  if (!h->finalized) return fail(h, FR_ERR_STATE, "model not finalised (fr_finalize)");
  if (n < 0 || (n > 0 && (!frames || !counts || (max_faces > 0 && !dets))) || height < 2 || width < 2 ||
      max_faces < 0)
    return fail(h, FR_ERR_INVALID_ARGUMENT, "bad frames / sizes / output buffers");
  if (n == 0) return FR_OK;
  if (int rc = check_dev_err(h)) return rc;  // reported by earlier asynchronous work
  DeviceGuard dg(h->device);
  return detector_run_device(h, frames, n, height, width, det_thresh, max_faces, dets, counts, (hipStream_t)stream);
}

int fr_align_device(fr_handle* h, const uint8_t* frames, int n_frames, int height, int width, const float* landmarks,
                    int stride, const int32_t* counts, int max_faces, int out_size, uint8_t* out, double* tforms,
                    uint8_t* ok, void* stream) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  const long long slots = (long long)n_frames * max_faces;
  if (n_frames < 0 || max_faces < 0 || height <= 0 || width <= 0 || out_size <= 0 || out_size > 1024 || stride < 10 ||
      slots >= (1ll << 31) || (slots > 0 && (!frames || !landmarks || !out || !ok)))
    return fail(h, FR_ERR_INVALID_ARGUMENT, "bad alignment arguments");
  if (slots == 0) return FR_OK;
  DeviceGuard dg(h->device);
  // sized before the first launch; a call that fits the buffer allocates nothing
  if (int rc = ensure_buf(h, &h->align_slots, &h->align_slots_cap, (size_t)slots * sizeof(WarpFace))) return rc;
  FitSlots p{};
  p.frames = frames;
  p.n_frames = n_frames;
  p.H = height;
  p.W = width;
  p.landmarks = landmarks;
  p.stride = stride;
  p.counts = counts;
  p.max_faces = max_faces;
  reference_template(out_size, p.tmpl);
  fit_logs(&p.logs);
  p.tforms = tforms;
  p.ok = ok;
  p.faces = static_cast<WarpFace*>(h->align_slots);
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = launch_fit_similarity(p, s);
  if (e != hipSuccess) return launch_fail(h, "similarity fit", e);
  e = launch_warp_affine_images(p.faces, (int)slots, out_size, out, s);
  if (e != hipSuccess) return launch_fail(h, "warp", e);
  return FR_OK;
}

int fr_detect_images_device(fr_handle* h, const uint8_t* const* images, const int32_t* sizes, int n, float det_thresh,
                            int max_faces, float* dets, int32_t* counts, void* stream) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (!h->detector) return fail(h, FR_ERR_STATE, "not a detector handle (fr_create(\"scrfd_10g\", \"scrfd\", ...))");
  if (!h->finalized) return fail(h, FR_ERR_STATE, "model not finalised (fr_finalize)");
  if (max_faces < 1) return fail(h, FR_ERR_INVALID_ARGUMENT, "max_faces must be at least 1");
  if (n < 0 || (n > 0 && (!images || !sizes || !dets || !counts)))
    return fail(h, FR_ERR_INVALID_ARGUMENT, "bad n or NULL images / sizes / output buffers");
  if (n == 0) return FR_OK;
  if (int rc = check_dev_err(h)) return rc;  // reported by earlier asynchronous work
  DeviceGuard dg(h->device);
  return detector_run_images_device(h, images, sizes, n, det_thresh, max_faces, dets, counts, (hipStream_t)stream);
}

int fr_align_images_device(fr_handle* h, const uint8_t* const* images, const int32_t* sizes, int n_images,
                           const float* landmarks, int stride, const int32_t* counts, int max_faces, int out_size,
                           uint8_t* out, double* tforms, uint8_t* ok, void* stream) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  const long long slots = (long long)n_images * max_faces;
  if (n_images < 0 || max_faces < 0 || out_size <= 0 || out_size > 1024 || stride < 10 || slots >= (1ll << 31) ||
      (slots > 0 && (!images || !sizes || !landmarks || !out || !ok)))
    return fail(h, FR_ERR_INVALID_ARGUMENT, "bad alignment arguments");
  if (slots == 0) return FR_OK;
  for (int i = 0; i < n_images; ++i)
    if (!images[i] || sizes[2 * i] <= 0 || sizes[2 * i + 1] <= 0)
      return fail(h, FR_ERR_INVALID_ARGUMENT, "image " + std::to_string(i) + " is NULL or has a side < 1");
  DeviceGuard dg(h->device);
  // sized before the first launch; a call that fits the buffer allocates nothing
  if (int rc = ensure_buf(h, &h->align_slots, &h->align_slots_cap, (size_t)slots * sizeof(WarpFace))) return rc;
  FitImageSlots q{};
  FitSlots& p = q.s;
  p.stride = stride;
  p.max_faces = max_faces;
  reference_template(out_size, p.tmpl);
  fit_logs(&p.logs);
  hipStream_t s = (hipStream_t)stream;
  // the image descriptors by value, FIT_IMAGES_BY_VALUE per fit launch: launch c fits the slots of
  // images [base, base + m) into their places of the one descriptor list the warp reads
  for (int base = 0; base < n_images; base += FIT_IMAGES_BY_VALUE) {
    const int m = std::min(FIT_IMAGES_BY_VALUE, n_images - base);
    const size_t slot0 = (size_t)base * max_faces;
    p.n_frames = m;
    for (int i = 0; i < m; ++i)
      q.images[i] = FitImage{images[base + i], sizes[2 * (base + i)], sizes[2 * (base + i) + 1]};
    p.landmarks = landmarks + slot0 * stride;
    p.counts = counts ? counts + base : nullptr;
    p.tforms = tforms ? tforms + slot0 * 6 : nullptr;
    p.ok = ok + slot0;
    p.faces = static_cast<WarpFace*>(h->align_slots) + slot0;
    const hipError_t e = launch_fit_similarity_images(q, s);
    if (e != hipSuccess) return launch_fail(h, "similarity fit", e);
  }
  const hipError_t e = launch_warp_affine_images(static_cast<WarpFace*>(h->align_slots), (int)slots, out_size, out, s);
  if (e != hipSuccess) return launch_fail(h, "warp", e);
  return FR_OK;
}

int fr_blur_scores_device(fr_handle* h, const uint8_t* crops, int n, int height, int width, int channels,
                          double* scores, void* stream) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (!blur_args_ok(crops, n, height, width, channels, scores))
    return fail(h, FR_ERR_INVALID_ARGUMENT, "bad blur arguments (height, width >= 1; channels 1, 3 or 4)");
  if (n == 0) return FR_OK;
  DeviceGuard dg(h->device);
  return blur_device(h, crops, n, height, width, channels, scores, (hipStream_t)stream);
}

int fr_quality_gate_device(fr_handle* h, const float* dets, const int32_t* counts, const uint8_t* ok,
                           const double* blur, int n_frames, int max_faces, const fr_gate_config* cfg,
                           uint8_t* stage, double* metrics, int32_t* bbox, int32_t* rank, int32_t* rows,
                           int32_t* frame_offsets, int32_t* valid_slots, int32_t* n_valid, void* stream) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (n_frames < 0 || max_faces < 1 || max_faces > FR_GATE_MAX_FACES ||
      (long long)n_frames * max_faces >= (1ll << 31) || !cfg)
    return fail(h, FR_ERR_INVALID_ARGUMENT,
                "bad quality gate arguments (n_frames >= 0, max_faces in [1, " + std::to_string(FR_GATE_MAX_FACES) +
                    "], a config)");
  GateArgs a{};
  if (!gate_limits(*cfg, blur != nullptr, &a.lim))
    return fail(h, FR_ERR_INVALID_ARGUMENT, "a quality gate limit is not finite or lies beyond +-FLT_MAX");
  if (n_frames == 0) return FR_OK;
  if (!dets || !stage || !metrics || !bbox || !rank || !rows || !frame_offsets || !valid_slots || !n_valid)
    return fail(h, FR_ERR_INVALID_ARGUMENT, "NULL quality gate buffer (only counts, ok and blur may be NULL)");
  DeviceGuard dg(h->device);
  if (int rc = ensure_buf(h, &h->gate_ws, &h->gate_ws_cap, (size_t)n_frames * sizeof(int32_t))) return rc;
  a.dets = dets;
  a.counts = counts;
  a.ok = ok;
  a.blur = blur;
  a.n_frames = n_frames;
  a.F = max_faces;
  a.stage = stage;
  a.metrics = metrics;
  a.bbox = bbox;
  a.rank = rank;
  a.rows = rows;
  a.frame_offsets = frame_offsets;
  a.valid_slots = valid_slots;
  a.n_valid = n_valid;
  a.frame_valid = static_cast<int32_t*>(h->gate_ws);
  const hipError_t e = launch_quality_gate(a, (hipStream_t)stream);
  if (e != hipSuccess) return launch_fail(h, "quality gate", e);
  return FR_OK;
}

int fr_set_precision(fr_handle* h, int mode) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (mode != FR_PRECISION_F32 && mode != FR_PRECISION_BF16X3)
    return fail(h, FR_ERR_INVALID_ARGUMENT, "precision must be FR_PRECISION_F32 or FR_PRECISION_BF16X3");
  h->prec = mode == FR_PRECISION_BF16X3 ? PREC_BF16X3 : PREC_F32;
  DeviceGuard dg(h->device);
  clear_graphs(h);
  if (h->finalized) return ensure_winograd(h);
  return FR_OK;
}

int fr_set_conv_algorithm(fr_handle* h, int algo) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (algo != FR_CONV_DIRECT && algo != FR_CONV_WINOGRAD && algo != FR_CONV_WINOGRAD4)
    return fail(h, FR_ERR_INVALID_ARGUMENT, "algorithm must be FR_CONV_DIRECT, FR_CONV_WINOGRAD or FR_CONV_WINOGRAD4");
  h->winograd = algo != FR_CONV_DIRECT;
  h->wino_m = algo == FR_CONV_WINOGRAD ? 2 : 4;
  DeviceGuard dg(h->device);
  clear_graphs(h);
  if (h->finalized) return ensure_winograd(h);
  return FR_OK;
}

int fr_set_graph_batch(fr_handle* h, int max_n) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (h->detector) return fail(h, FR_ERR_STATE, "this handle is a detector (scrfd_10g)");
  if (max_n < 0 || max_n > h->max_batch) return fail(h, FR_ERR_INVALID_ARGUMENT, "max_n must be in [0, max_batch]");
  DeviceGuard dg(h->device);
  h->graph_max_n = max_n;
  clear_graphs(h);
  return FR_OK;
}

int fr_set_lanes(fr_handle* h, int min_n, int max_lanes) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (h->detector) return fail(h, FR_ERR_STATE, "this handle is a detector (scrfd_10g)");
  if (min_n < 0) return fail(h, FR_ERR_INVALID_ARGUMENT, "min_n must be >= 0 (0: one lane)");
  if (max_lanes < 1 || max_lanes > MAX_LANES) return fail(h, FR_ERR_INVALID_ARGUMENT, "max_lanes must be in [1, 4]");
  h->lane_min = min_n;
  h->lane_max = max_lanes;
  h->lanes_fallback = false;
  return FR_OK;
}

int fr_get_lanes(fr_handle* h, int* min_n, int* max_lanes, int* fell_back) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  if (min_n) *min_n = h->lane_min;
  if (max_lanes) *max_lanes = h->lane_max;
  if (fell_back) *fell_back = h->lanes_fallback ? 1 : 0;
  return FR_OK;
}

int fr_graph_count(fr_handle* h, int* count) {
  if (!h || !count) return fail(h, FR_ERR_INVALID_ARGUMENT, "NULL argument");
  std::lock_guard<std::mutex> lk(h->mu);
  *count = (int)h->graphs.size();
  return FR_OK;
}

int fr_profile_enable(fr_handle* h, int enable) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  h->prof = enable != 0;
  return FR_OK;
}

int fr_profile_read(fr_handle* h, double* conv_ms, double* conv_flop, int64_t* conv_launches, double* total_ms) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  std::lock_guard<std::mutex> lk(h->mu);
  DeviceGuard dg(h->device);
  double tms = 0;
  for (int k = 0; k < 3; ++k) {
    h->last_ms[k] = h->last_flop[k] = h->last_exec[k] = 0;
    h->last_n[k] = 0;
  }
  for (auto& e : h->events) {
    FR_HIP(h, hipEventSynchronize(e.b));
    float ms = 0.f;
    FR_HIP(h, hipEventElapsedTime(&ms, e.a, e.b));
    tms += ms;
    const int k = e.kind >= 0 && e.kind < 3 ? e.kind : 0;
    h->last_ms[k] += ms;
    h->last_flop[k] += e.flop;
    h->last_exec[k] += e.exec_flop;
    ++h->last_n[k];
    h->pool.push_back(e.a);
    h->pool.push_back(e.b);
  }
  h->events.clear();
  if (int rc = check_dev_err(h)) return rc;  // every profiled launch has completed
  if (conv_ms) *conv_ms = h->last_ms[1] + h->last_ms[2];
  if (conv_flop) *conv_flop = h->last_flop[1] + h->last_flop[2];
  if (conv_launches) *conv_launches = h->last_n[1] + h->last_n[2];
  if (total_ms) *total_ms = tms;
  return FR_OK;
}

int fr_profile_kernel(fr_handle* h, int kind, double* ms, double* flop, double* exec_flop, int64_t* launches) {
  if (!h) return fail(nullptr, FR_ERR_INVALID_ARGUMENT, "NULL handle");
  if (kind < 0 || kind > 2) return fail(h, FR_ERR_INVALID_ARGUMENT, "kind must be FR_PROF_OTHER/CONV_DIRECT/CONV_WINOGRAD");
  std::lock_guard<std::mutex> lk(h->mu);
  if (ms) *ms = h->last_ms[kind];
  if (flop) *flop = h->last_flop[kind];
  if (exec_flop) *exec_flop = h->last_exec[kind];
  if (launches) *launches = h->last_n[kind];
  return FR_OK;
}

const char* fr_last_error(fr_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

// content hash of the library's sources and flags (build.py build_id, a generated translation unit)
extern "C" const char* frhip_build_id(void);
const char* fr_version(void) {
  static const std::string v = std::string("frhip 0.1 gfx950 fp32-mfma build ") + frhip_build_id();
  return v.c_str();
}

}  // extern "C"
