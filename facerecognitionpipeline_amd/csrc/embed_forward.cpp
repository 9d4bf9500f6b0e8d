// libfrhip embedding forward: lanes, the per-forward layout plan, the IR forward executor, its
// hipGraph replay, the crop resize and the gallery matcher.  What it replaces in the reference:
//   FaceEmbedder.extract_embeddings_batch   face_embedder.py:137-182 (A3)
//   GalleryManager.search                   gallery_manager.py:189-205 (A11)
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "runtime.h"

using namespace frhip;

namespace frhip_rt {

static hipEvent_t take_event(fr_handle* h) {
  if (!h->pool.empty()) {
    hipEvent_t e = h->pool.back();
    h->pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}

ProfScope::ProfScope(fr_handle* h_, hipStream_t s_, double flop, int kind, double exec_flop)
    : h(h_), s(s_), on(h_->prof) {
  if (!on) return;
  ev.a = take_event(h);
  ev.b = take_event(h);
  ev.flop = flop;
  ev.exec_flop = exec_flop < 0 ? flop : exec_flop;
  ev.kind = kind;
  if (!ev.a || !ev.b) {
    on = false;
    return;
  }
  (void)hipEventRecord(ev.a, s);
}

ProfScope::~ProfScope() {
  if (!on) return;
  (void)hipEventRecord(ev.b, s);
  h->events.push_back(ev);
}

// Frees lane l's (>= 1) activation workspace (after a failed ensure_lane).  Only work queued on
// the lane's own stream can still read it (earlier calls joined that stream back into theirs),
// so a sync of that stream -- not of the device, which would stall other handles -- suffices.
static void release_lane(fr_handle* h, int l) {
  LaneWs& L = h->lane_ws[l];
  if (h->lane_stream[l]) (void)hipStreamSynchronize(h->lane_stream[l]);
  for (auto& a : L.act) {
    if (a) (void)hipFree(a);
    a = nullptr;
  }
  if (L.sc_buf) (void)hipFree(L.sc_buf);
  if (L.partial) (void)hipFree(L.partial);
  L.sc_buf = L.partial = nullptr;
  h->lane_batch[l] = 0;
}

// Lane l's (>= 1) workspace for up to `batch` crops, its stream and its join event.
static int ensure_lane(fr_handle* h, int l, int batch) {
  LaneWs& L = h->lane_ws[l];
  if (h->lane_batch[l] < batch) {
    for (auto& a : L.act) {
      if (a) FR_HIP(h, hipFree(a));
      a = nullptr;
    }
    if (L.sc_buf) FR_HIP(h, hipFree(L.sc_buf));
    if (L.partial) FR_HIP(h, hipFree(L.partial));
    L.sc_buf = L.partial = nullptr;
    h->lane_batch[l] = 0;
    const size_t mb = batch;
    for (auto& a : L.act) FR_HIP(h, hipMalloc((void**)&a, mb * 112 * 112 * 64 * sizeof(float)));
    FR_HIP(h, hipMalloc((void**)&L.sc_buf, mb * 56 * 56 * 64 * sizeof(float)));
    // head partials: also a serving batch's 4x split (forward_lanes), whatever the lane's size
    FR_HIP(h, hipMalloc((void**)&L.partial, (size_t)fr_handle::HEAD_PARTS * std::max<size_t>(mb, h->max_batch) * 512 *
                                                sizeof(float)));
    h->lane_batch[l] = batch;
  }
  if (!L.w4part) {
    FR_HIP(h, hipMalloc((void**)&L.w4part, fr_handle::W4PART_FLOATS * sizeof(float)));
  }
  if (ensure_stream_k(h->device, &h->cus, &L.sk_ws, &L.sk_ws_floats, &L.sk_cnt, &L.sk_cnt_cap) != FR_OK)
    return fail(h, FR_ERR_HIP, "stream-K workspace allocation failed");
  if (!h->lane_stream[l]) FR_HIP(h, hipStreamCreateWithFlags(&h->lane_stream[l], hipStreamNonBlocking));
  if (!h->lane_fork) FR_HIP(h, hipEventCreateWithFlags(&h->lane_fork, hipEventDisableTiming));
  if (!h->lane_join[l]) FR_HIP(h, hipEventCreateWithFlags(&h->lane_join[l], hipEventDisableTiming));
  return FR_OK;
}

// Which activations of one forward are channel-blocked, per body block (on the stack: a batch-1
// forward is launch-bound, so the plan allocates nothing).
struct LayoutPlan {
  static constexpr size_t MAX_BLOCKS = 64;  // ir_101 has 49
  // serving conv kernel: conv1 and conv2 of the block both run on it (conv1's output is blocked);
  // the block's output is blocked
  bool all_convs[MAX_BLOCKS] = {}, out_blk[MAX_BLOCKS] = {};
  // F(4x4): the block's conv1 output / the block's output is blocked
  bool w4r_blk[MAX_BLOCKS] = {}, w4y_blk[MAX_BLOCKS] = {};
};

// The layout plan of a forward of nl lanes of cnt[l] crops (once per forward).
static int plan_layouts(fr_handle* h, const int* cnt, int nl, LayoutPlan& pl) {
  const size_t nb = h->blocks.size();
  if (nb > LayoutPlan::MAX_BLOCKS) return fail(h, FR_ERR_HIP, "internal: more body blocks than the layout plan holds");
  // Which activations are channel-blocked: in a one-lane serving forward, those passed between
  // two layers that run_conv puts on the serving conv kernel (same rule as its branch).
  {
    const bool serving = nl == 1 && h->convs_blocked;
    // the launches forward_lanes makes: conv1 (pre-BN, BN, PReLU) at the block's input size;
    // conv2 with the fused conv shortcut (EPI_AFFINE + x2), the identity residual or the
    // MaxPool(1,2) one (an unfused conv shortcut keeps NHWC: its own launch reads the input)
    auto on_convs = [&](const ConvW& c, int hw, Epi epi, bool x2) {
      return serving && convs_takes(h, c, conv_shape(c, cnt[0], hw, hw), epi, 1, x2);
    };
    bool conv2_convs[LayoutPlan::MAX_BLOCKS] = {};
    int hw = 112;
    for (size_t bi = 0; bi < nb; ++bi) {
      const BlockW& b = h->blocks[bi];
      const bool fused = b.has_sc_conv && h->fuse_shortcut && b.conv2_sc.w;
      const int ho = hw / b.spec.stride;
      conv2_convs[bi] = fused ? on_convs(b.conv2_sc, hw, EPI_AFFINE, true)
                              : !b.has_sc_conv && on_convs(b.conv2, hw, b.spec.stride == 1 ? EPI_AFFINE_RES
                                                                                          : EPI_AFFINE_RES_SUB, false);
      pl.all_convs[bi] = conv2_convs[bi] && on_convs(b.conv1, hw, EPI_AFFINE_PRELU, false);
      hw = ho;
    }
    for (size_t bi = 0; bi + 1 < nb; ++bi) pl.out_blk[bi] = conv2_convs[bi] && pl.all_convs[bi + 1];
  }
  // Channel-blocked activations between F(4x4) layers (batches the serving kernel does not take):
  // a block's conv1 output when both convs of the block run on F(4x4); a block's output when its
  // conv2 and the next block's conv1 and conv2 (identity residual) do.  Every other tensor -- the
  // stem's, the stride-2 / shortcut / FC kernels' inputs and outputs -- stays NHWC.  The layouts
  // change nothing in the arithmetic: embeddings are bitwise the NHWC forward's (tested).
  // (every lane must be past the serving kernel's batch limit: with an uneven split a smaller lane
  // could take the serving branch, which does not read the F(4x4) layout bits)
  int cnt_min = cnt[0];
  for (int l = 1; l < nl; ++l) cnt_min = std::min(cnt_min, cnt[l]);
  if (h->w4_blocked && cnt_min > h->convs_max_n && !h->detector) {
    bool c1[LayoutPlan::MAX_BLOCKS] = {}, c2[LayoutPlan::MAX_BLOCKS] = {}, y[LayoutPlan::MAX_BLOCKS] = {};
    int hw = 112;
    for (size_t bi = 0; bi < nb; ++bi) {
      const BlockW& b = h->blocks[bi];
      const int ho = hw / b.spec.stride;
      c1[bi] = w4_takes(h, b.conv1, EPI_AFFINE_PRELU, 0, 0, hw, hw);
      // (a conv shortcut or a stride-2 conv2 runs on another kernel)
      c2[bi] = !b.has_sc_conv && b.spec.stride == 1 && w4_takes(h, b.conv2, EPI_AFFINE_RES, hw, hw, hw, hw);
      hw = ho;
    }
    for (size_t bi = 0; bi < nb; ++bi) {
      pl.w4r_blk[bi] = c1[bi] && c2[bi];
      y[bi] = c2[bi] && bi + 1 < nb && c1[bi + 1] && c2[bi + 1];
    }
    // a lone blocked block output makes both conv2s around it seams (residual and output in
    // different layouts: the RMIX instances, ~1% slower than NHWC, profiles/r05/w4ab_layouts_table.txt)
    // and no conv2 of the run gains: IR stages 1 and 4 (two F(4x4) blocks each) stay NHWC
    for (size_t bi = 0; bi < nb; ++bi)
      pl.w4y_blk[bi] = y[bi] && ((bi > 0 && y[bi - 1]) || (bi + 1 < nb && y[bi + 1]));
  }
  return FR_OK;
}

// One forward of up to max_batch crops: rgb (device) -> out (device) [n][512], as nl lanes
// (lane l: crops [off[l], off[l] + cnt[l]) on stream st[l] with workspace L[l]).  Every launch is
// issued for each lane in turn, so while one lane's layer runs its last, part-empty round the
// other lane's launch of the same layer is already queued.
static int forward_lanes(fr_handle* h, const uint8_t* rgb, const int* off, const int* cnt, int nl, float* out,
                         int normalize, const hipStream_t* st, const LaneWs* L) {
  for (int l = 0; l < nl; ++l) {
    const int n = cnt[l];
    ProfScope ps(h, st[l], 2.0 * n * 112.0 * 112.0 * 64 * 27, 0);
    hipError_t e = launch_stem(rgb + (size_t)off[l] * 112 * 112 * 3, n, h->lut, h->stem_w, h->stem_scale,
                               h->stem_shift, h->stem_prelu, L[l].act[0], st[l]);
    if (e != hipSuccess) return fail(h, FR_ERR_HIP, std::string("stem launch: ") + hipGetErrorString(e));
  }
  LayoutPlan pl;
  if (int rc = plan_layouts(h, cnt, nl, pl)) return rc;
  int cur = 0, HW = 112;
  bool pre_done = false;  // the previous conv2 wrote this block's pre-BN input into L[0].sc_buf
  const size_t nb = h->blocks.size();
  for (size_t bi = 0; bi < nb; ++bi) {
    const BlockW& b = h->blocks[bi];
    const int nxt = cur == 0 ? 1 : 0;
    const int Ho = HW / b.spec.stride;
    const bool in_blk = bi > 0 && pl.out_blk[bi - 1], r_blk = pl.all_convs[bi];
    const bool w4_in = bi > 0 && pl.w4y_blk[bi - 1];
    // BN(x) already in sc_buf (pre_done): conv1 without pre-BN (and not on the F(4x4) / F(2x2)
    // filters, which have the pre-BN scale folded in)
    ConvW c1w = b.conv1;
    if (pre_done) {
      c1w.pre_scale = c1w.pre_shift = nullptr;
      c1w.wino = c1w.wino4 = c1w.wino4_t = nullptr;
    }
    for (int l = 0; l < nl; ++l) {
      ConvCall c{pre_done ? L[l].sc_buf : L[l].act[cur], L[l].act[2], cnt[l], HW, HW, EPI_AFFINE_PRELU};
      c.convs_blk = (in_blk ? CONVS_BLK_X : 0) | (r_blk ? CONVS_BLK_Y : 0);
      c.w4_blk = (w4_in ? W4_BLK_X : 0) | (pl.w4r_blk[bi] ? W4_BLK_Y : 0);
      if (int rc = run_conv(h, c1w, c, L[l], st[l])) return rc;
    }
    // conv2 (and an unfused conv shortcut in front of it): the layout bits and, in a one-lane
    // forward, the next block's pre-BN input as a second output of a serving-kernel conv2 (sc_buf
    // is free then unless this block's unfused shortcut uses it)
    const bool fused = b.has_sc_conv && h->fuse_shortcut && b.conv2_sc.w;
    ConvCall c2{};  // x, y, B and epi: per lane below
    c2.H = c2.W = HW;
    c2.convs_blk = (r_blk ? CONVS_BLK_X : 0) | (in_blk ? CONVS_BLK_X2 | CONVS_BLK_RES : 0) | (pl.out_blk[bi] ? CONVS_BLK_Y : 0);
    c2.w4_blk = (pl.w4r_blk[bi] ? W4_BLK_X : 0) | (w4_in ? W4_BLK_RES : 0) | (pl.w4y_blk[bi] ? W4_BLK_Y : 0);
    if (nl == 1 && h->convs_pre_epilogue && bi + 1 < nb && (fused || !b.has_sc_conv) &&
        h->blocks[bi + 1].conv1.pre_scale && (size_t)Ho * Ho * b.spec.depth <= (size_t)56 * 56 * 64) {
      c2.y2 = L[0].sc_buf;
      c2.y2_scale = h->blocks[bi + 1].conv1.pre_scale;
      c2.y2_shift = h->blocks[bi + 1].conv1.pre_shift;
    }
    pre_done = false;
    for (int l = 0; l < nl; ++l) {
      float* x = L[l].act[cur];
      ConvCall c = c2;
      c.x = L[l].act[2];
      c.y = L[l].act[nxt];
      c.B = cnt[l];
      const ConvW* cw = &b.conv2;
      if (fused) {
        cw = &b.conv2_sc;
        c.epi = EPI_AFFINE;
        c.x2 = x;
      } else if (b.has_sc_conv) {
        ConvCall sc = c2;
        sc.x = x;
        sc.y = L[l].sc_buf;
        sc.B = cnt[l];
        sc.epi = EPI_AFFINE;
        if (int rc = run_conv(h, b.sc, sc, L[l], st[l])) return rc;
        c.epi = EPI_AFFINE_RES;
        c.res = L[l].sc_buf;
        c.res_H = c.res_W = Ho;
      } else {
        c.epi = b.spec.stride == 1 ? EPI_AFFINE_RES : EPI_AFFINE_RES_SUB;
        c.res = x;
        c.res_H = c.res_W = HW;
      }
      if (int rc = run_conv(h, *cw, c, L[l], st[l], &pre_done)) return rc;
    }
    cur = nxt;
    HW = Ho;
  }
  for (int l = 0; l < nl; ++l) {
    const int n = cnt[l];
    // serving batches (4 n <= max_batch): the FC's 784 K-steps in 98 splits of 8, so its 51 MB
    // of weights stream through many workgroups (batch 1: 78 us with 49 splits on 256x128, 27.7
    // with 196 on 64x128, 24.8 with 98: tools/fc_sweep.py --batch 1); larger batches in 32
    // splits of 25 (tools/fc_sweep.py: B = 256 79.2 -> 69.3 us, a 128-crop lane 47.3 -> 43.0,
    // vs 49 splits).  Decided by n alone (every lane's partials hold HEAD_PARTS x max_batch
    // rows), so a lane's part computes exactly as a one-lane forward of the same crops.
    ConvCall c{L[l].act[cur], L[l].partial, n, 7, 7, EPI_RAW};
    c.nsplit = 4 * n <= h->max_batch ? fr_handle::HEAD_SPLIT_SMALL : fr_handle::HEAD_SPLIT;
    c.split_stride = (long long)n * 512;
    if (int rc = run_conv(h, h->head, c, L[l], st[l])) return rc;
    ProfScope ps(h, st[l], 0.0, 0);
    hipError_t e = launch_head_reduce(L[l].partial, c.nsplit, c.split_stride, h->fc_bias, h->bn1d_scale,
                                      h->bn1d_shift, out + (size_t)off[l] * 512, n, normalize, !h->arcface, st[l]);
    if (e != hipSuccess) return fail(h, FR_ERR_HIP, std::string("head launch: ") + hipGetErrorString(e));
  }
  return FR_OK;
}

// One forward of up to max_batch crops: rgb (device) -> out (device) [n][512].  With lanes on
// (fr_set_lanes), the batch runs as nl = min(lane_max, n / lane_min) near-equal parts: lanes
// 1 .. nl - 1 fork from s and join back into it, so the call is stream-ordered on s like a single
// forward.  Profiled and graph-captured forwards stay one lane (per-launch events would overlap;
// a captured graph replays on one stream).
static int forward_chunk(fr_handle* h, const uint8_t* rgb, int n, float* out, int normalize, hipStream_t s) {
  const int nl = (h->lane_min <= 0 || h->prof || h->capturing) ? 1 : std::max(1, std::min(h->lane_max, n / h->lane_min));
  const int off0 = 0;
  if (nl == 1) return forward_lanes(h, rgb, &off0, &n, 1, out, normalize, &s, h->lane_ws);
  int off[MAX_LANES], cnt[MAX_LANES];
  hipStream_t st[MAX_LANES];
  // lane buffers sized for the largest part of a max_batch forward, so they are made once
  const int cap = (h->max_batch + nl - 1) / nl;
  for (int l = 0, o = 0; l < nl; ++l) {
    cnt[l] = n / nl + (l < n % nl ? 1 : 0);
    off[l] = o;
    o += cnt[l];
    if (l > 0 && ensure_lane(h, l, std::max(cnt[l], cap)) != FR_OK) {
      // no memory for the second lane's workspace: run this and later forwards as one lane
      // (what worked before lanes existed) instead of failing the call; fr_set_lanes re-enables
      (void)hipGetLastError();  // clear the failed allocation's sticky error
      release_lane(h, l);
      h->lane_min = 0;  // visible through fr_get_lanes
      h->lanes_fallback = true;
      h->err.clear();  // the call succeeds: no stale allocation message for the next failure
      return forward_lanes(h, rgb, &off0, &n, 1, out, normalize, &s, h->lane_ws);
    }
    st[l] = l ? h->lane_stream[l] : s;
  }
  FR_HIP(h, hipEventRecord(h->lane_fork, s));
  for (int l = 1; l < nl; ++l) FR_HIP(h, hipStreamWaitEvent(st[l], h->lane_fork, 0));
  const int rc = forward_lanes(h, rgb, off, cnt, nl, out, normalize, st, h->lane_ws);
  // join even after a failed launch, so that nothing of this call is left unordered behind s
  hipError_t e = hipSuccess;
  for (int l = 1; l < nl; ++l) {
    hipError_t e1 = hipEventRecord(h->lane_join[l], st[l]);
    if (e1 == hipSuccess) e1 = hipStreamWaitEvent(s, h->lane_join[l], 0);
    if (e == hipSuccess) e = e1;
  }
  if (rc) return rc;
  FR_HIP(h, e);
  return FR_OK;
}

void clear_graphs(fr_handle* h) {
  if (h->graphs.empty()) return;
  (void)hipDeviceSynchronize();  // no replay of these graphs may still be in flight
  for (auto& g : h->graphs) (void)hipGraphExecDestroy(g.exec);
  h->graphs.clear();
}

// Capture forward_chunk(in_stage -> emb_stage) for n crops as a hipGraph.  Every pointer and
// size a launch takes is fixed for (n, normalize) once the handle is finalised, and the
// stream-K tickets re-arm themselves, so the graph replays without updates.
static int capture_graph(fr_handle* h, int n, int normalize) {
  if (!h->cap_stream) FR_HIP(h, hipStreamCreateWithFlags(&h->cap_stream, hipStreamNonBlocking));
  FR_HIP(h, hipStreamBeginCapture(h->cap_stream, hipStreamCaptureModeThreadLocal));
  h->capturing = true;
  const int rc = forward_chunk(h, h->in_stage, n, h->emb_stage, normalize, h->cap_stream);
  h->capturing = false;
  hipGraph_t g = nullptr;
  const hipError_t e = hipStreamEndCapture(h->cap_stream, &g);
  if (rc != FR_OK || e != hipSuccess) {
    if (g) (void)hipGraphDestroy(g);
    return rc != FR_OK ? rc : fail(h, FR_ERR_HIP, std::string("graph capture: ") + hipGetErrorString(e));
  }
  hipGraphExec_t ex = nullptr;
  const hipError_t ei = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (ei != hipSuccess) return fail(h, FR_ERR_HIP, std::string("graph instantiate: ") + hipGetErrorString(ei));
  h->graphs.push_back({n, normalize, ex});
  return FR_OK;
}

// One forward of n <= max_batch crops from in_stage to emb_stage.  Small n (the serving
// pattern: a frame's faces, or batch 1) is launch-bound, so with fr_set_graph_batch those
// forwards replay a captured graph: the first call for an n runs eagerly (loading every
// kernel), then captures; later calls are one hipGraphLaunch.
int forward_staged(fr_handle* h, int n, int normalize, hipStream_t s) {
  if (n > h->graph_max_n || h->prof) return forward_chunk(h, h->in_stage, n, h->emb_stage, normalize, s);
  for (const auto& g : h->graphs)
    if (g.n == n && g.normalize == normalize) {
      FR_HIP(h, hipGraphLaunch(g.exec, s));
      return FR_OK;
    }
  const int rc = forward_chunk(h, h->in_stage, n, h->emb_stage, normalize, s);
  if (rc != FR_OK) return rc;
  return capture_graph(h, n, normalize);
}

int embed_device(fr_handle* h, const uint8_t* rgb, int n, float* out, int normalize, hipStream_t s) {
  if (n > 0 && n <= h->graph_max_n && !h->prof) {
    FR_HIP(h, hipMemcpyAsync(h->in_stage, rgb, (size_t)n * 112 * 112 * 3, hipMemcpyDeviceToDevice, s));
    const int rc = forward_staged(h, n, normalize, s);
    if (rc != FR_OK) return rc;
    FR_HIP(h, hipMemcpyAsync(out, h->emb_stage, (size_t)n * 512 * sizeof(float), hipMemcpyDeviceToDevice, s));
    return FR_OK;
  }
  for (int off = 0; off < n; off += h->max_batch) {
    const int bn = std::min(h->max_batch, n - off);
    int rc = forward_chunk(h, rgb + (size_t)off * 112 * 112 * 3, bn, out + (size_t)off * 512, normalize, s);
    if (rc) return rc;
  }
  return FR_OK;
}

// cv2.resize(crop, (112, 112), INTER_LINEAR) of n H x W crops (face_embedder.py:94-96), device to
// device, in OpenCV's fixed point (the letterbox kernel of the detector with a 112 x 112 canvas).
// The coefficient tables are built once per source size and kept on the device, at most
// RS_TABS_MAX of them (least recently used one replaced: a server resizing crops of arbitrary
// sizes keeps a bounded cache).
int resize_device(fr_handle* h, const uint8_t* src, int n, int H, int W, uint8_t* dst, hipStream_t s) {
  fr_handle::ResizeTab* t = nullptr;
  for (auto& r : h->rs_tabs)
    if (r.H == H && r.W == W) t = &r;
  if (!t) {
    std::vector<int> host(4 * (112 + 112));
    resize_axis_table(112, W, host.data());
    resize_axis_table(112, H, host.data() + 4 * 112);
    if (h->rs_tabs.size() >= fr_handle::RS_TABS_MAX) {
      t = &*std::min_element(h->rs_tabs.begin(), h->rs_tabs.end(),
                             [](const fr_handle::ResizeTab& a, const fr_handle::ResizeTab& b) { return a.used < b.used; });
      // the replaced table may still be read by a resize queued earlier, on s or on another
      // stream: the copy waits for that launch (its event), then goes in stream order on s
      if (t->last) FR_HIP(h, hipStreamWaitEvent(s, t->last, 0));
      FR_HIP(h, hipMemcpyAsync(t->tab, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice, s));
      FR_HIP(h, hipStreamSynchronize(s));  // the pageable host table must outlive the copy
      t->H = H;
      t->W = W;
      t->simd_end = resize_simd_end(112 * 3);
    } else {
      int* d = nullptr;
      FR_HIP(h, hipMalloc((void**)&d, host.size() * sizeof(int)));
      FR_HIP(h, hipMemcpy(d, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice));
      h->rs_tabs.push_back({H, W, resize_simd_end(112 * 3), d, 0, nullptr});
      t = &h->rs_tabs.back();
    }
  }
  t->used = ++h->rs_clock;
  ProfScope ps(h, s, 0.0, 0);
  hipError_t e = launch_letterbox(src, n, H, W, t->tab, t->tab + 4 * 112, 112, 112, t->simd_end, 112, 112, dst, s);
  if (e != hipSuccess) return fail(h, FR_ERR_HIP, std::string("resize launch: ") + hipGetErrorString(e));
  // (never inside a graph capture: captured forwards start at in_stage, after the resize)
  if (!t->last) FR_HIP(h, hipEventCreateWithFlags(&t->last, hipEventDisableTiming));
  FR_HIP(h, hipEventRecord(t->last, s));
  return FR_OK;
}

int check_crop_size(fr_handle* h, int height, int width) {
  if (height < 1 || width < 1 || height > 8192 || width > 8192)
    return fail(h, FR_ERR_INVALID_ARGUMENT, "crop height/width must be in [1, 8192]");
  return FR_OK;
}

// Embed n crops of any size: 112 x 112 go straight to the forward, others through resize_device
// one max_batch chunk at a time.
int embed_any(fr_handle* h, const uint8_t* rgb, int n, int height, int width, float* out, int normalize,
              hipStream_t s) {
  if (height == 112 && width == 112) return embed_device(h, rgb, n, out, normalize, s);
  for (int off = 0; off < n; off += h->max_batch) {
    const int bn = std::min(h->max_batch, n - off);
    int rc = resize_device(h, rgb + (size_t)off * height * width * 3, bn, height, width, h->rs_stage, s);
    if (rc) return rc;
    rc = embed_device(h, h->rs_stage, bn, out + (size_t)off * 512, normalize, s);
    if (rc) return rc;
  }
  return FR_OK;
}

int check_images(fr_handle* h, const uint8_t* const* images, const int32_t* sizes, int n) {
  for (int i = 0; i < n; ++i) {
    const int height = sizes[2 * i], width = sizes[2 * i + 1];
    if (!images[i]) return fail(h, FR_ERR_INVALID_ARGUMENT, "image " + std::to_string(i) + " is NULL");
    if (height < 1 || height > FR_IMAGE_MAX_SIDE || width < 1 || width > FR_IMAGE_MAX_SIDE)
      return fail(h, FR_ERR_INVALID_ARGUMENT,
                  "image " + std::to_string(i) + " is " + std::to_string(height) + " x " + std::to_string(width) +
                      " (each side must be in [1, " + std::to_string(FR_IMAGE_MAX_SIDE) + "])");
  }
  return FR_OK;
}

// The ragged resize (fr_resize_images / fr_embed_images; images validated by check_images), in chunks
// of max_batch.  stage_images lays every chunk's staging out in h->ri_host, chunk c at ri_chunks[c]:
//   [bn] CropImage | coefficient tables, [112 x][4] then [112 y][4] per distinct size of the chunk
// (resize_device's tables, built once per size, not per image; 112 x 112 images that the kernel
// copies need none).  One host buffer holds all chunks of a call, so no chunk's pageable bytes are
// rewritten while its copy may be pending; an earlier call's copies are waited for at entry.
// resize_images_chunk then makes chunk c's one copy and one launch.
int stage_images(fr_handle* h, const uint8_t* const* images, const int32_t* sizes, int n, hipStream_t s) {
  FR_HIP(h, hipStreamSynchronize(s));
  constexpr size_t TAB_INTS = 4 * (112 + 112);
  h->ri_host.clear();
  h->ri_chunks.clear();
  std::vector<int> sized;  // (H, W, table offset) of the chunk's distinct sizes
  size_t largest = 0;
  for (int off = 0; off < n; off += h->max_batch) {
    const int bn = std::min(h->max_batch, n - off);
    const size_t at = h->ri_host.size(), tab_off = (size_t)bn * sizeof(CropImage);
    h->ri_chunks.push_back(at);
    h->ri_host.resize(at + tab_off);
    sized.clear();
    for (int i = 0; i < bn; ++i) {
      const int H = sizes[2 * (off + i)], W = sizes[2 * (off + i) + 1];
      const uint8_t* src = images[off + i];
      CropImage im{src, W, 0, 0, H == 112 && W == 112 && (reinterpret_cast<uintptr_t>(src) & 3) == 0};
      if (!im.copy) {
        int t = -1;
        for (size_t k = 0; k < sized.size(); k += 3)
          if (sized[k] == H && sized[k + 1] == W) t = sized[k + 2];
        if (t < 0) {
          t = (int)(sized.size() / 3 * TAB_INTS);
          sized.insert(sized.end(), {H, W, t});
          h->ri_host.resize(at + tab_off + (t + TAB_INTS) * sizeof(int));
          int* tab = reinterpret_cast<int*>(h->ri_host.data() + at + tab_off) + t;
          resize_axis_table(112, W, tab);
          resize_axis_table(112, H, tab + 4 * 112);
        }
        im.xtab = t;
        im.ytab = t + 4 * 112;
      }
      memcpy(h->ri_host.data() + at + (size_t)i * sizeof(CropImage), &im, sizeof(im));
    }
    h->ri_host.resize((h->ri_host.size() + 15) & ~size_t(15));
    largest = std::max(largest, h->ri_host.size() - at);
  }
  return ensure_buf(h, &h->ri_dev, &h->ri_dev_cap, largest);
}

int resize_images_chunk(fr_handle* h, size_t c, int bn, uint8_t* dst, hipStream_t s) {
  const size_t at = h->ri_chunks[c];
  const size_t bytes = (c + 1 < h->ri_chunks.size() ? h->ri_chunks[c + 1] : h->ri_host.size()) - at;
  // (stream order on s keeps the copy behind the previous chunk's launch, which reads ri_dev)
  FR_HIP(h, hipMemcpyAsync(h->ri_dev, h->ri_host.data() + at, bytes, hipMemcpyHostToDevice, s));
  const char* base = static_cast<const char*>(h->ri_dev);
  ProfScope ps(h, s, 0.0, 0);
  const hipError_t e = launch_resize_images(reinterpret_cast<const CropImage*>(base),
                                            reinterpret_cast<const int*>(base + (size_t)bn * sizeof(CropImage)), bn,
                                            resize_simd_end(112 * 3), dst, s);
  if (e != hipSuccess) return fail(h, FR_ERR_HIP, std::string("resize launch: ") + hipGetErrorString(e));
  return FR_OK;
}

int resize_images(fr_handle* h, const uint8_t* const* images, const int32_t* sizes, int n, uint8_t* dst,
                  hipStream_t s) {
  if (int rc = stage_images(h, images, sizes, n, s)) return rc;
  for (size_t c = 0; c < h->ri_chunks.size(); ++c) {
    const int off = (int)c * h->max_batch, bn = std::min(h->max_batch, n - off);
    if (int rc = resize_images_chunk(h, c, bn, dst + (size_t)off * 112 * 112 * 3, s)) return rc;
  }
  return FR_OK;
}

// embed_any for such a list: each chunk resized into rs_stage, then through embed_device.
int embed_images(fr_handle* h, const uint8_t* const* images, const int32_t* sizes, int n, float* out, int normalize,
                 hipStream_t s) {
  if (int rc = stage_images(h, images, sizes, n, s)) return rc;
  for (size_t c = 0; c < h->ri_chunks.size(); ++c) {
    const int off = (int)c * h->max_batch, bn = std::min(h->max_batch, n - off);
    if (int rc = resize_images_chunk(h, c, bn, h->rs_stage, s)) return rc;
    if (int rc = embed_device(h, h->rs_stage, bn, out + (size_t)off * 512, normalize, s)) return rc;
  }
  return FR_OK;
}

int gallery_reserve(fr_handle* h, int rows, hipStream_t s) {
  const size_t need = (size_t)rows * 512 * sizeof(float);
  if (h->gallery_cap >= need) return FR_OK;
  const size_t want = std::max(need, std::min((size_t)h->gallery_cap * 2, need + ((size_t)256 << 20)));
  float* p = nullptr;
  FR_HIP(h, hipMalloc((void**)&p, want));
  if (h->G > 0) FR_HIP(h, hipMemcpyAsync(p, h->gallery, (size_t)h->G * 512 * sizeof(float), hipMemcpyDeviceToDevice, s));
  FR_HIP(h, hipStreamSynchronize(s));
  FR_HIP(h, hipFree(h->gallery));
  h->gallery = p;
  h->gallery_cap = want;
  return FR_OK;
}

int match_device(fr_handle* h, const float* Q, int n, int k, int32_t* idx, float* score, hipStream_t s) {
  if (h->G <= 0) return fail(h, FR_ERR_STATE, "gallery is empty (fr_gallery_set first)");
  if (k < 1 || k > h->G) return fail(h, FR_ERR_INVALID_ARGUMENT, "k must be in [1, G]");
  if (n <= 0) return FR_OK;
  int rc;
  if (n <= 16 && (long long)n * h->G * 4 < (1ll << 31)) {
    // serving-sized: normalisation fused into one scores launch (embed_misc.hip), then top-k
    rc = ensure_buf(h, (void**)&h->scores, &h->scores_cap, (size_t)n * h->G * sizeof(float));
    if (rc) return rc;
    ProfScope ps(h, s, 0.0, 0);
    hipError_t e = launch_scores_small(Q, h->gallery, h->G, h->scores, n, s);
    if (e == hipSuccess) e = launch_topk(h->scores, n, h->G, k, idx, score, s);
    if (e != hipSuccess) return fail(h, FR_ERR_HIP, std::string("match launch: ") + hipGetErrorString(e));
    return FR_OK;
  }
  rc = ensure_buf(h, (void**)&h->qn, &h->qn_cap, (size_t)n * 512 * sizeof(float));
  if (rc) return rc;
  LaneWs& L = h->lane_ws[0];
  if (ensure_stream_k(h->device, &h->cus, &L.sk_ws, &L.sk_ws_floats, &L.sk_cnt, &L.sk_cnt_cap) != FR_OK)
    return fail(h, FR_ERR_HIP, "stream-K workspace allocation failed");
  {
    ProfScope ps(h, s, 0.0, 0);
    hipError_t e = launch_l2norm_rows(Q, h->qn, n, 512, s);
    if (e != hipSuccess) return fail(h, FR_ERR_HIP, std::string("l2norm launch: ") + hipGetErrorString(e));
  }
  ConvW g;
  g.w = h->gallery;
  g.geometry(512, h->G, 1, 1, 1, 0);
  // score matrices below 2 GiB (the conv epilogue's 32-bit offsets): queries in chunks
  const int nc = (int)std::max<long long>(1, std::min<long long>(n, ((1ll << 31) - 1) / ((long long)h->G * 4)));
  rc = ensure_buf(h, (void**)&h->scores, &h->scores_cap, (size_t)nc * h->G * sizeof(float));
  if (rc) return rc;
  for (int q0 = 0; q0 < n; q0 += nc) {
    const int qn = std::min(nc, n - q0);
    rc = run_conv(h, g, ConvCall{h->qn + (size_t)q0 * 512, h->scores, qn, 1, 1, EPI_RAW}, L, s);
    if (rc) return rc;
    ProfScope ps(h, s, 0.0, 0);
    hipError_t e = launch_topk(h->scores, qn, h->G, k, idx + (size_t)q0 * k, score + (size_t)q0 * k, s);
    if (e != hipSuccess) return fail(h, FR_ERR_HIP, std::string("topk launch: ") + hipGetErrorString(e));
  }
  return FR_OK;
}

}  // namespace frhip_rt
