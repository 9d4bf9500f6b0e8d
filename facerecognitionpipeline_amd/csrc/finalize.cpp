// libfrhip handle state: error reporting, buffers, the helpers the entry points share (the lock,
// the CSR offsets check, the offsets staging), the state-dict schema, BatchNorm folding and
// the upload of every folded tensor, the derived filter arenas and the workspace.  What it
// replaces in the reference:
//   FaceEmbedder.__init__/load_state_dict   face_embedder.py:27-62
#include <cmath>
#include <string>
#include <vector>

#include "runtime.h"

using namespace frhip;

namespace frhip_rt {

thread_local std::string g_create_error;

int fail(fr_handle* h, int code, const std::string& msg) {
  if (h)
    h->err = msg;
  else
    g_create_error = msg;
  return code;
}

int ensure_dev_err(fr_handle* h) {
  if (h->dev_err) return FR_OK;
  FR_HIP(h, hipHostMalloc((void**)&h->dev_err, sizeof(int), hipHostMallocCoherent | hipHostMallocMapped));
  *(volatile int*)h->dev_err = 0;
  return FR_OK;
}

int check_dev_err(fr_handle* h) {
  if (!h->dev_err) return FR_OK;
  const int v = *(volatile int*)h->dev_err;
  if (!v) return FR_OK;
  *(volatile int*)h->dev_err = 0;
  return fail(h, FR_ERR_HIP,
              (v & FR_DEVERR_W4_HANDOFF)
                  ? "F(4x4) ring hand-off timed out in wino4_kernel: the results of the work queued on this handle "
                    "before this call are invalid"
                  : "device error word set (" + std::to_string(v) + ")");
}

int ensure_buf(fr_handle* h, void** p, size_t* cap, size_t bytes) {
  if (*cap >= bytes) return FR_OK;
  if (*p) FR_HIP(h, hipFree(*p));
  *p = nullptr;
  *cap = 0;
  FR_HIP(h, hipMalloc(p, bytes));
  *cap = bytes;
  return FR_OK;
}

int launch_fail(fr_handle* h, const char* what, hipError_t e) {
  return fail(h, FR_ERR_HIP, std::string(what) + " launch: " + hipGetErrorString(e));
}

std::unique_lock<std::mutex> lock_handle(fr_handle* h) {
  return h ? std::unique_lock<std::mutex>(h->mu) : std::unique_lock<std::mutex>();
}

std::string csr_check(const int32_t* offsets, int n, long long min_len, long long max_len, const CsrNouns& nouns,
                      const int32_t* outer) {
  const std::string array = nouns.array, item = nouns.item;
  if (n > 0 && !outer && offsets[0] != 0) return array + "[0] must be 0";
  for (int i = 0; i < n; ++i) {
    const long long len =
        outer ? (long long)offsets[outer[i + 1]] - offsets[outer[i]] : (long long)offsets[i + 1] - offsets[i];
    if (len >= min_len && len <= max_len) continue;
    const std::string at = item + " " + std::to_string(i);
    return (len < 0 ? array + " decrease at " + at + ": " : std::string()) + "every " + item + " needs " +
           std::to_string(min_len) + ".." + std::to_string(max_len) + " " + nouns.unit + " (" + at + " has " +
           std::to_string(len) + ")";
  }
  return std::string();
}

int stage_int32(fr_handle* h, hipStream_t s, std::initializer_list<Int32Span> parts, const int** dev) {
  size_t total = 0;
  for (const Int32Span& p : parts) total += p.n;
  if (int rc = ensure_buf(h, &h->csr_stage, &h->csr_stage_cap, total * sizeof(int32_t))) return rc;
  const int32_t* src = parts.begin()->p;
  if (parts.size() > 1) {  // packed on the host first: one copy per call
    h->csr_host.clear();
    for (const Int32Span& p : parts) h->csr_host.insert(h->csr_host.end(), p.p, p.p + p.n);
    src = h->csr_host.data();
  }
  FR_HIP(h, hipMemcpyAsync(h->csr_stage, src, total * sizeof(int32_t), hipMemcpyHostToDevice, s));
  const int* d = (const int*)h->csr_stage;
  for (const Int32Span& p : parts) {
    *dev++ = d;
    d += p.n;
  }
  return FR_OK;
}

// Stream-K slabs for P = CUs x (<=2 blocks/CU) blocks x 2 slots x the largest tile (256x128).
int ensure_stream_k(int device, int* cus, float** ws, long long* ws_floats, int** cnt, int* cnt_cap) {
  if (*ws) return FR_OK;
  int n = 0;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n <= 0) n = 256;
  const long long floats = (long long)n * 4 * 2 * 256 * 128;
  const int cap = 8 * n;
  if (hipMalloc((void**)ws, floats * sizeof(float)) != hipSuccess) return FR_ERR_HIP;
  if (hipMalloc((void**)cnt, cap * sizeof(int)) != hipSuccess) return FR_ERR_HIP;
  if (hipMemset(*cnt, 0, cap * sizeof(int)) != hipSuccess) return FR_ERR_HIP;
  *cus = n;
  *ws_floats = floats;
  *cnt_cap = cap;
  return FR_OK;
}

const std::vector<float>* getp(fr_handle* h, const std::string& k) {
  auto it = h->params.find(k);
  return it == h->params.end() ? nullptr : &it->second;
}

std::vector<BlockSpec> block_specs(const std::string& arch, bool* ok) {
  static const struct {
    const char* arch;
    int units[4];
  } kArchs[] = {{"ir_50", {3, 4, 14, 3}}, {"ir_101", {3, 13, 30, 3}}, {"ir_34", {3, 4, 6, 3}}, {"ir_18", {2, 2, 2, 2}}};
  const int* units = nullptr;
  for (const auto& a : kArchs)
    if (arch == a.arch) units = a.units;
  *ok = units != nullptr;
  if (!units) return {};
  const int widths[4] = {64, 128, 256, 512};
  std::vector<BlockSpec> v;
  int in = 64;
  for (int s = 0; s < 4; ++s) {
    v.push_back({in, widths[s], 2});
    for (int u = 1; u < units[s]; ++u) v.push_back({widths[s], widths[s], 1});
    in = widths[s];
  }
  return v;
}

void add_bn(std::map<std::string, size_t>& m, const std::string& p, int c, bool affine) {
  if (affine) {
    m[p + ".weight"] = c;
    m[p + ".bias"] = c;
  }
  m[p + ".running_mean"] = c;
  m[p + ".running_var"] = c;
  m[p + ".num_batches_tracked"] = 1;
}

// State-dict key names of one residual unit / the stem / the head, per model family.
struct UnitKeys {
  std::string pre_bn, conv1, mid_bn, prelu, conv2, out_bn, sc_conv, sc_bn;
};

static UnitKeys unit_keys(bool arcface, const std::vector<BlockSpec>& specs, size_t i) {
  if (!arcface) {
    const std::string p = "body." + std::to_string(i) + ".";
    return {p + "res_layer.0", p + "res_layer.1.weight", p + "res_layer.2", p + "res_layer.3.weight",
            p + "res_layer.4.weight", p + "res_layer.5", p + "shortcut_layer.0.weight", p + "shortcut_layer.1"};
  }
  int stage = 0, unit = 0;
  for (size_t j = 1; j <= i; ++j) {
    if (specs[j].stride == 2) {
      ++stage;
      unit = 0;
    } else {
      ++unit;
    }
  }
  const std::string p = "layer" + std::to_string(stage + 1) + "." + std::to_string(unit) + ".";
  return {p + "bn1", p + "conv1.weight", p + "bn2", p + "prelu.weight", p + "conv2.weight", p + "bn3",
          p + "downsample.0.weight", p + "downsample.1"};
}

// Whether unit s has a conv shortcut.  AdaFace: only where the width changes (MaxPool2d(1,2) in
// stage 1); ArcFace: a conv1x1 downsample on every strided unit.
static bool has_conv_shortcut(bool arcface, const BlockSpec& s) { return arcface ? s.stride == 2 : s.cin != s.depth; }

// Expected state-dict keys and sizes.  ArcFace: the insightface arcface_torch IResNet keys (the
// network behind the reference's ArcFace ONNX files, face_embedder.py:64-88), whose BN1d
// `features` is affine and whose output is not L2-normalised.
std::map<std::string, size_t> embedder_schema(bool af, const std::vector<BlockSpec>& specs) {
  std::map<std::string, size_t> m;
  m[af ? "conv1.weight" : "input_layer.0.weight"] = 64 * 3 * 9;
  add_bn(m, af ? "bn1" : "input_layer.1", 64);
  m[af ? "prelu.weight" : "input_layer.2.weight"] = 64;
  add_bn(m, af ? "bn2" : "output_layer.0", 512);
  m[af ? "fc.weight" : "output_layer.3.weight"] = (size_t)512 * 512 * 49;
  m[af ? "fc.bias" : "output_layer.3.bias"] = 512;
  add_bn(m, af ? "features" : "output_layer.4", 512, af);
  for (size_t i = 0; i < specs.size(); ++i) {
    const auto& s = specs[i];
    const UnitKeys k = unit_keys(af, specs, i);
    add_bn(m, k.pre_bn, s.cin);
    m[k.conv1] = (size_t)s.depth * s.cin * 9;
    add_bn(m, k.mid_bn, s.depth);
    m[k.prelu] = s.depth;
    m[k.conv2] = (size_t)s.depth * s.depth * 9;
    add_bn(m, k.out_bn, s.depth);
    if (has_conv_shortcut(af, s)) {
      m[k.sc_conv] = (size_t)s.depth * s.cin;
      add_bn(m, k.sc_bn, s.depth);
    }
  }
  return m;
}

// PyTorch CPU eval BatchNorm computes alpha = gamma/sqrt(var+eps), beta = bias - mean*alpha
// in the input dtype and applies x*alpha + beta (ATen batch_norm_cpu_collect_linear_and_constant_terms).
void bn_fold(const std::vector<float>* gamma, const std::vector<float>* beta, const std::vector<float>& mean,
             const std::vector<float>& var, std::vector<float>& scale, std::vector<float>& shift) {
  const size_t c = mean.size();
  scale.resize(c);
  shift.resize(c);
  for (size_t i = 0; i < c; ++i) {
    const float invstd = 1.0f / std::sqrt(var[i] + 1e-5f);
    const float g = gamma ? (*gamma)[i] : 1.0f;
    const float b = beta ? (*beta)[i] : 0.0f;
    scale[i] = invstd * g;
    shift[i] = b - mean[i] * scale[i];
  }
}

// [O][I][kh][kw] -> [O][kh][kw][I]
std::vector<float> repack_oihw(const std::vector<float>& w, int O, int I, int kh, int kw) {
  std::vector<float> r((size_t)O * I * kh * kw);
  for (int o = 0; o < O; ++o)
    for (int i = 0; i < I; ++i)
      for (int y = 0; y < kh; ++y)
        for (int x = 0; x < kw; ++x)
          r[(((size_t)o * kh + y) * kw + x) * I + i] = w[(((size_t)o * I + i) * kh + y) * kw + x];
  return r;
}

// Every body conv (conv1 and conv2 of each block, with `fused` also its fused conv2 + shortcut),
// plus the detector's convs (detector handles have no body, embedding handles no detector).
static std::vector<ConvW*> model_convs(fr_handle* h, bool fused) {
  std::vector<ConvW*> all;
  for (auto& b : h->blocks) {
    all.push_back(&b.conv1);
    all.push_back(&b.conv2);
    if (fused) all.push_back(&b.conv2_sc);
  }
  detector_convs(h->det, all);
  return all;
}

// F(2x2,3x3) filters G g G^T of every eligible body conv, built on the device from the arena the
// first time the algorithm is selected after fr_finalize (16/9 of the 3x3 weights).
static int ensure_wino2(fr_handle* h) {
  if (h->wino_arena || h->detector) return FR_OK;
  std::vector<ConvW*> wconvs;
  size_t wfloats = 0;
  for (ConvW* c : model_convs(h, false)) {
    c->wino = nullptr;
    if (c->w && wino_supported(c->cin, c->cout, c->kh, c->kw, c->stride, c->pad)) {
      wconvs.push_back(c);
      wfloats += wino_weight_floats(c->cout, c->cin);
    }
  }
  if (!wfloats) return FR_OK;
  FR_HIP(h, hipMalloc((void**)&h->wino_arena, wfloats * sizeof(float)));
  size_t off = 0;
  for (ConvW* c : wconvs) {
    c->wino = h->wino_arena + off;
    FR_HIP(h, launch_wino_weights(c->w, c->wino, c->cout, c->cin, nullptr));
    off += wino_weight_floats(c->cout, c->cin);
  }
  FR_HIP(h, hipDeviceSynchronize());
  return FR_OK;
}

// F(4x4,3x3) filters of every eligible conv, built on the device from the arena the first
// time the algorithm is selected after fr_finalize (36/9 = 4x the 3x3 weights).
// The pre-activation BN of a conv1 is folded: U = G (g * scale) G^T and t = shift / scale is
// added to the in-image input pixels, so BN(x) = scale (x + t).  A conv whose BN scale has a
// zero (t not finite) keeps the direct kernel.
bool wino4_pre_fold(const ConvW* c, std::vector<float>& t) {
  t.assign(c->cin, 0.f);
  if (!c->pre_scale) return true;
  std::vector<float> sc(c->cin), sh(c->cin);
  if (hipMemcpy(sc.data(), c->pre_scale, c->cin * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(sh.data(), c->pre_shift, c->cin * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
    return false;
  for (int i = 0; i < c->cin; ++i) {
    t[i] = sh[i] / sc[i];
    if (sc[i] == 0.f || !std::isfinite(t[i])) return false;
  }
  return true;
}

static int ensure_wino4(fr_handle* h) {
  if (h->wino4_arena) return FR_OK;
  std::vector<ConvW*> wconvs;
  std::vector<std::vector<float>> ts;
  size_t wfloats = 0;
  for (ConvW* c : model_convs(h, false)) {
    c->wino4 = nullptr;
    c->wino4_t = nullptr;
    std::vector<float> t;
    if (c->w && wino4_supported(c->cin, c->cout, c->kh, c->kw, c->stride, c->pad) && wino4_pre_fold(c, t)) {
      wconvs.push_back(c);
      ts.push_back(std::move(t));
      wfloats += wino4_weight_floats(c->cout, c->cin) + (c->pre_scale ? c->cin : 0);
    }
  }
  if (!wfloats) return FR_OK;
  FR_HIP(h, hipMalloc((void**)&h->wino4_arena, wfloats * sizeof(float)));
  size_t off = 0;
  for (size_t k = 0; k < wconvs.size(); ++k) {
    ConvW* c = wconvs[k];
    c->wino4 = h->wino4_arena + off;
    off += wino4_weight_floats(c->cout, c->cin);
    FR_HIP(h, launch_wino4_weights(c->w, c->pre_scale, c->wino4, c->cout, c->cin, nullptr));
    if (c->pre_scale) {
      c->wino4_t = h->wino4_arena + off;
      off += c->cin;
      FR_HIP(h, hipMemcpy(c->wino4_t, ts[k].data(), c->cin * sizeof(float), hipMemcpyHostToDevice));
    }
  }
  FR_HIP(h, hipDeviceSynchronize());
  return FR_OK;
}

static void drop_wino4(fr_handle* h) {
  (void)hipFree(h->wino4_arena);
  h->wino4_arena = nullptr;
  for (ConvW* c : model_convs(h, false)) {
    c->wino4 = nullptr;
    c->wino4_t = nullptr;
  }
}

// The serving conv kernel's filters (fragment order) for every body 3x3 conv it can run: conv1,
// conv2 and the fused conv2 + shortcut of each block (embedding models only).
static int ensure_convs_weights(fr_handle* h) {
  if (h->convs_arena || h->detector) return FR_OK;
  std::vector<ConvW*> cs;
  size_t floats = 0;
  for (ConvW* c : model_convs(h, true)) {
    c->w_frag = nullptr;
    if (c->w && c->kh == 3 && c->kw == 3 && c->cin % 16 == 0 && c->cout % 16 == 0 && c->cin2 % 16 == 0) {
      cs.push_back(c);
      floats += (size_t)c->cout * (9 * c->cin + c->cin2);
    }
  }
  if (!floats) return FR_OK;
  FR_HIP(h, hipMalloc((void**)&h->convs_arena, floats * sizeof(float)));
  size_t off = 0;
  for (ConvW* c : cs) {
    c->w_frag = h->convs_arena + off;
    off += (size_t)c->cout * (9 * c->cin + c->cin2);
    FR_HIP(h, launch_convs_weights(c->w, c->w_frag, c->cout, 9 * c->cin + c->cin2, nullptr));
  }
  FR_HIP(h, hipDeviceSynchronize());
  return FR_OK;
}

int ensure_winograd(fr_handle* h) {
  if (!h->winograd) return FR_OK;
  if (h->wino_m == 2) return ensure_wino2(h);
  // bf16x3 runs the direct split-bf16 kernel; the F(4x4) path is f32 only
  return ensure_wino4(h);
}

// Stem, body blocks and head: every folded tensor staged in pk, the ConvW geometry filled in.
static void pack_model(fr_handle* h, Packer& pk) {
  std::vector<float> sc, sh;
  auto P = [&](const std::string& k) -> const std::vector<float>& { return *getp(h, k); };
  auto bn = [&](const std::string& p, float** dsc, float** dsh, bool affine = true) {
    bn_fold(affine ? &P(p + ".weight") : nullptr, affine ? &P(p + ".bias") : nullptr, P(p + ".running_mean"),
            P(p + ".running_var"), sc, sh);
    pk.put(dsc, sc);
    pk.put(dsh, sh);
  };

  // preprocessing LUT in float64 then float32: AdaFace (v/255.0 - 0.5)/0.5 (face_embedder.py:99-101),
  // ArcFace (v - 127.5)/127.5 (face_embedder.py:105-110)
  std::vector<float> lut(256);
  for (int v = 0; v < 256; ++v) lut[v] = h->arcface ? (float)((v - 127.5) / 127.5) : (float)((v / 255.0 - 0.5) / 0.5);
  pk.put(&h->lut, lut);
  const bool af = h->arcface;
  // stem: [64][3][3][3] (BGR channel order) -> [ky][kx][c_rgb][64]
  {
    const auto& w = P(af ? "conv1.weight" : "input_layer.0.weight");
    std::vector<float> r(27 * 64);
    for (int o = 0; o < 64; ++o)
      for (int c = 0; c < 3; ++c)
        for (int y = 0; y < 3; ++y)
          for (int x = 0; x < 3; ++x) r[((y * 3 + x) * 3 + (2 - c)) * 64 + o] = w[((o * 3 + c) * 3 + y) * 3 + x];
    pk.put(&h->stem_w, r);
    bn(af ? "bn1" : "input_layer.1", &h->stem_scale, &h->stem_shift);
    pk.put(&h->stem_prelu, P(af ? "prelu.weight" : "input_layer.2.weight"));
  }
  h->blocks.assign(h->specs.size(), BlockW{});
  for (size_t i = 0; i < h->specs.size(); ++i) {
    const auto& s = h->specs[i];
    BlockW& b = h->blocks[i];
    b.spec = s;
    const UnitKeys k = unit_keys(af, h->specs, i);
    b.conv1.geometry(s.cin, s.depth, 3, 3, 1, 1);
    pk.put(&b.conv1.w, repack_oihw(P(k.conv1), s.depth, s.cin, 3, 3));
    bn(k.pre_bn, &b.conv1.pre_scale, &b.conv1.pre_shift);
    bn(k.mid_bn, &b.conv1.post_scale, &b.conv1.post_shift);
    pk.put(&b.conv1.prelu, P(k.prelu));
    b.conv2.geometry(s.depth, s.depth, 3, 3, s.stride, 1);
    const std::vector<float> w2 = repack_oihw(P(k.conv2), s.depth, s.depth, 3, 3);
    pk.put(&b.conv2.w, w2);
    bn(k.out_bn, &b.conv2.post_scale, &b.conv2.post_shift);
    const std::vector<float> sc2 = sc, sh2 = sh;
    if (has_conv_shortcut(af, s)) {
      b.has_sc_conv = true;
      b.sc.geometry(s.cin, s.depth, 1, 1, s.stride, 0);
      pk.put(&b.sc.w, P(k.sc_conv));  // [O][I][1][1] == [O][1][1][I]
      bn(k.sc_bn, &b.sc.post_scale, &b.sc.post_shift);
      if (s.stride == 2 && s.depth % 32 == 0 && s.cin % 32 == 0) {
        // fused conv2 + shortcut: y = sum (w2 * s2) r + sum (wsc * s_sc) x + (b2 + b_sc)
        const auto& wsc = P(k.sc_conv);
        const int K2 = 9 * s.depth, Kf = K2 + s.cin;
        std::vector<float> wf((size_t)s.depth * Kf), one(s.depth, 1.f), shf(s.depth);
        for (int o = 0; o < s.depth; ++o) {
          for (int q = 0; q < K2; ++q) wf[(size_t)o * Kf + q] = w2[(size_t)o * K2 + q] * sc2[o];
          for (int c = 0; c < s.cin; ++c) wf[(size_t)o * Kf + K2 + c] = wsc[(size_t)o * s.cin + c] * sc[o];
          shf[o] = sh2[o] + sh[o];
        }
        b.conv2_sc = b.conv2;
        b.conv2_sc.cin2 = s.cin;
        pk.put(&b.conv2_sc.w, wf);
        pk.put(&b.conv2_sc.post_scale, one);
        pk.put(&b.conv2_sc.post_shift, shf);
      }
    }
  }
  // head: BN2d(512) as pre-affine; Linear(25088,512) with NCHW-flatten columns
  // (c*49 + y*7 + x) permuted to NHWC taps ((y*7 + x)*512 + c); BN1d (affine for ArcFace).
  {
    h->head.geometry(512, 512, 7, 7, 1, 0);
    const auto& w = P(af ? "fc.weight" : "output_layer.3.weight");
    std::vector<float> r((size_t)512 * 25088);
    for (int o = 0; o < 512; ++o)
      for (int c = 0; c < 512; ++c)
        for (int t = 0; t < 49; ++t) r[(size_t)o * 25088 + (size_t)t * 512 + c] = w[(size_t)o * 25088 + (size_t)c * 49 + t];
    pk.put(&h->head.w, r);
    bn(af ? "bn2" : "output_layer.0", &h->head.pre_scale, &h->head.pre_shift);
    pk.put(&h->fc_bias, P(af ? "fc.bias" : "output_layer.3.bias"));
    bn(af ? "features" : "output_layer.4", &h->bn1d_scale, &h->bn1d_shift, af);
  }
}

// Lane 0's workspace for max_batch crops, the staging buffers and the stream-K slabs.
static int ensure_workspace(fr_handle* h) {
  const size_t mb = h->max_batch;
  LaneWs& L = h->lane_ws[0];
  if (!L.act[0]) {
    for (auto& a : L.act) FR_HIP(h, hipMalloc((void**)&a, mb * 112 * 112 * 64 * sizeof(float)));
    // shortcut output: 28x28x128 per image (AdaFace; stage 1 has no conv shortcut), 56x56x64 (ArcFace)
    FR_HIP(h, hipMalloc((void**)&L.sc_buf, mb * 56 * 56 * 64 * sizeof(float)));
    FR_HIP(h, hipMalloc((void**)&L.partial, (size_t)fr_handle::HEAD_PARTS * mb * 512 * sizeof(float)));
    FR_HIP(h, hipMalloc((void**)&h->in_stage, mb * 112 * 112 * 3));
    FR_HIP(h, hipMalloc((void**)&h->rs_stage, mb * 112 * 112 * 3));
    FR_HIP(h, hipMalloc((void**)&h->emb_stage, mb * 512 * sizeof(float)));
    FR_HIP(h, hipMalloc((void**)&L.w4part, fr_handle::W4PART_FLOATS * sizeof(float)));
    h->lane_batch[0] = h->max_batch;
  }
  if (ensure_stream_k(h->device, &h->cus, &L.sk_ws, &L.sk_ws_floats, &L.sk_cnt, &L.sk_cnt_cap) != FR_OK)
    return fail(h, FR_ERR_HIP, "stream-K workspace allocation failed");
  return FR_OK;
}

int finalize_model(fr_handle* h) {
  if (int rc = ensure_dev_err(h)) return rc;
  clear_graphs(h);
  if (h->detector) {
    int rc = detector_finalize(h);
    if (rc) return rc;
    // the detector's stride-1 3x3 convs run on the F(4x4) kernel as well (run_conv)
    drop_wino4(h);
    if (h->wino_m == 4 && (rc = ensure_winograd(h)) != FR_OK) return rc;
    h->finalized = true;
    return FR_OK;
  }

  Packer pk;
  pack_model(h, pk);
  if (h->arena) FR_HIP(h, hipFree(h->arena));
  h->arena = nullptr;
  FR_HIP(h, hipMalloc((void**)&h->arena, pk.buf.size() * sizeof(float)));
  FR_HIP(h, hipMemcpy(h->arena, pk.buf.data(), pk.buf.size() * sizeof(float), hipMemcpyHostToDevice));
  h->arena_floats = pk.buf.size();
  for (auto& f : pk.fix) *f.first = h->arena + f.second;

  // Winograd filters are built from the arena on the device for the selected algorithm only
  // (ensure_wino2 / ensure_wino4); a later fr_set_conv_algorithm builds the other set
  if (h->wino_arena) FR_HIP(h, hipFree(h->wino_arena));
  h->wino_arena = nullptr;
  drop_wino4(h);
  if (h->convs_arena) FR_HIP(h, hipFree(h->convs_arena));
  h->convs_arena = nullptr;
  for (auto& b : h->blocks) {
    b.conv1.wino = nullptr;
    b.conv2.wino = nullptr;
  }

  if (int rc = ensure_workspace(h)) return rc;
  h->finalized = true;
  if (h->winograd) {
    const int rc = ensure_winograd(h);
    if (rc != FR_OK) {
      h->finalized = false;
      return rc;
    }
  }
  if (const int rc = ensure_convs_weights(h)) {
    h->finalized = false;
    return rc;
  }
  return FR_OK;
}

}  // namespace frhip_rt
