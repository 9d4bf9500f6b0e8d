// libfrhip conv dispatch: run_conv, the one place that decides which kernel a convolution (or
// GEMM, as a 1x1 conv over a 1x1 image) runs on, and the rules it decides by.
#include <algorithm>
#include <string>

#include "runtime.h"

using namespace frhip;

namespace frhip_rt {

ConvKnobs g_knobs;

// serving conv kernel: layers of at most this many output pixels (n * Ho * Wo).  Batch 1 also
// takes stage 1's 56x56 layers: 1.0626 vs 1.0740 ms per embed + match, medians of 8 runs each
// interleaved in one process, spreads 0.0003 / 0.0007 ms (profiles/r05/serving_pixel_limit_ab.txt,
// tools/serve_small_ab.py --pixels); at batch 2 their 6,272 pixels, and stage 2's 1,568, are
// faster on F(4x4) split-K (1.50 vs 1.52-1.54 ms with 4,096; profiles/r04/serving/pixel_threshold_ab.txt)
static inline long long convs_max_m(const fr_handle* h, int n) { return n == 1 ? h->convs_max_m1 : 1024; }

ConvParams conv_shape(const ConvW& cw, int B, int H, int W, int nsplit) {
  ConvParams p{};
  p.B = B;
  p.H = H;
  p.W = W;
  p.Cin = cw.cin;
  p.Cout = cw.cout;
  p.KH = cw.kh;
  p.KW = cw.kw;
  p.stride = cw.stride;
  p.pad = cw.pad;
  p.Ho = (H + 2 * cw.pad - cw.kh) / cw.stride + 1;
  p.Wo = (W + 2 * cw.pad - cw.kw) / cw.stride + 1;
  p.M = B * p.Ho * p.Wo;
  p.steps_total = cw.kh * cw.kw * cw.cin / 32;
  if (cw.cin2 > 0) {
    p.Cin2 = cw.cin2;
    p.steps1 = p.steps_total;
    p.steps_total += cw.cin2 / 32;
  }
  p.steps_per_split = (p.steps_total + nsplit - 1) / nsplit;
  return p;
}

// has_x2: the fused shortcut's input will be passed (cw.cin2 > 0).
bool convs_takes(const fr_handle* h, const ConvW& cw, ConvParams p, Epi epi, int nsplit, bool has_x2) {
  static const float sentinel = 0.f;
  if (has_x2 && !p.x2) p.x2 = &sentinel;  // convs_supported only checks that it is given
  return p.B <= h->convs_max_n && p.M <= convs_max_m(h, p.B) && !h->detector && h->prec == PREC_F32 && nsplit == 1 &&
         cw.w_frag && convs_supported(p, cw.pre_scale != nullptr, epi);
}

// The epilogues of the F(2x2) kernel: the IR body's conv1 (pre-BN, BN, PReLU) and its stride-1
// conv2 (BN + a residual of the output's height).
static bool wino_epi(const ConvW& cw, Epi epi, int res_H, int Ho) {
  return (epi == EPI_AFFINE_PRELU && cw.pre_scale) || (epi == EPI_AFFINE_RES && !cw.pre_scale && res_H == Ho);
}

// Ho / Wo: the conv's output size.
bool w4_takes(const fr_handle* h, const ConvW& cw, Epi epi, int res_H, int res_W, int Ho, int Wo) {
  // F(4x4) also takes the detector's epilogues (no pre-BN; residual of the output's shape)
  const bool wino4_epi =
      wino_epi(cw, epi, res_H, Ho) || (!cw.pre_scale && (epi == EPI_AFFINE_PRELU || epi == EPI_AFFINE ||
                                                         ((epi == EPI_AFFINE_RES || epi == EPI_AFFINE_RES_PRELU) &&
                                                          (res_H == 0 || res_H == Ho) && (res_W == 0 || res_W == Wo))));
  return h->winograd && h->wino_m == 4 && h->prec == PREC_F32 && cw.wino4 && wino4_epi &&
         wino4_supported(cw.cin, cw.cout, cw.kh, cw.kw, cw.stride, cw.pad);
}

int run_conv(fr_handle* h, const ConvW& cw, const ConvCall& c, const LaneWs& L, hipStream_t s, bool* wrote_y2) {
  const Epi epi = c.epi;
  const int nsplit = c.nsplit;
  ConvParams p = conv_shape(cw, c.B, c.H, c.W, nsplit);
  p.x = c.x;
  p.w = cw.w;
  p.y = c.y;
  p.pre_scale = cw.pre_scale;
  p.pre_shift = cw.pre_shift;
  p.post_scale = cw.post_scale;
  p.post_shift = cw.post_shift;
  p.prelu = cw.prelu;
  p.res = c.res;
  p.res_H = c.res_H;
  p.res_W = c.res_W;
  if (cw.cin2 > 0) p.x2 = c.x2;
  p.split_stride = c.split_stride;
  if (h->stream_k && nsplit == 1 && L.sk_ws) {
    p.sk_cus = h->cus;
    p.sk_ws = L.sk_ws;
    p.sk_ws_floats = L.sk_ws_floats;
    p.sk_cnt = L.sk_cnt;
    p.sk_cnt_cap = L.sk_cnt_cap;
  }
  const double flop = 2.0 * p.M * (double)p.Cout * (cw.kh * cw.kw * cw.cin + cw.cin2);
  // serving batches (n <= convs_max_n): every body 3x3 conv as one launch with the whole K per
  // 16x16 tile (conv_small.hip); f32 parity path only
  // (layers of at most convs_max_m(B) output pixels: stage 1's 112x112 conv1, 784 pixel blocks
  // x 4 cout blocks, stays on F(4x4) split-K, which is faster there: 54 vs ~20 us)
  if (convs_takes(h, cw, p, epi, nsplit, c.x2 != nullptr)) {
    if (c.w4_blk)  // plan_layouts plans F(4x4) layouts only when no lane reaches this branch
      return fail(h, FR_ERR_HIP, "internal: F(4x4) channel-blocked activations in the serving conv kernel");
    p.w = cw.w_frag;
    p.blk = c.convs_blk;
    if (c.y2 && epi != EPI_AFFINE_PRELU) {
      p.y2 = c.y2;
      p.y2_scale = c.y2_scale;
      p.y2_shift = c.y2_shift;
    }
    ProfScope ps(h, s, flop, FR_PROF_CONV_DIRECT);
    const hipError_t e = launch_convs(p, cw.pre_scale != nullptr, epi, s);
    if (e != hipSuccess) return fail(h, FR_ERR_HIP, std::string("serving conv launch: ") + hipGetErrorString(e));
    if (p.y2 && wrote_y2) *wrote_y2 = true;
    return FR_OK;
  }
  if (c.convs_blk)  // plan_layouts only sets it for layers the branch above takes
    return fail(h, FR_ERR_HIP, "internal: channel-blocked activations outside the serving conv kernel");
  // Tile per layer shape, from tools/conv_sweep.py on MI355X at B=256 with the stream-K
  // schedule (profiles/r01/sweep.txt): 8-wave 128x64 for the 64-channel
  // stage and the 128-channel residual convs, 8-wave 128x128 for the 1x1 shortcuts,
  // 8-wave 256x128 for every other 3x3 conv and the FC.
  // Winograd F(4x4,3x3) for the stride-1 3x3 convs (f32 parity path only)
  if (w4_takes(h, cw, epi, c.res_H, c.res_W, p.Ho, p.Wo)) {
    Wino4Params wp{};
    wp.x = c.x;
    wp.u = cw.wino4;
    wp.y = c.y;
    wp.pre_t = cw.wino4_t;
    wp.post_scale = cw.post_scale;
    wp.post_shift = cw.post_shift;
    wp.prelu = cw.prelu;
    wp.res = c.res;
    wp.B = c.B;
    wp.H = c.H;
    wp.W = c.W;
    wp.Cin = cw.cin;
    wp.Cout = cw.cout;
    wp.part = L.w4part;
    wp.part_floats = L.w4part ? fr_handle::W4PART_FLOATS : 0;
    wp.max_split = g_knobs.wino4_max_split;
    wp.err = h->dev_err;
    wp.poll_max = g_knobs.wino4_poll > 0 ? g_knobs.wino4_poll : -1;
    wp.blk = c.w4_blk;  // plan_layouts' plan of channel-blocked activations
    wp.nbg_override = g_knobs.wino4_nbg;
    wp.shapes = g_knobs.wino4_shapes;
    Wino4Params cv = wp;
    cv.blk = 0;
    wino4_canvas(cv);
    // executed: 36 products per (canvas) 4x4 tile and (cin, cout) pair (the same canvas either kernel)
    const double exec = 2.0 * 36.0 * cv.ntiles * (double)cw.cin * cw.cout;
    ProfScope ps(h, s, flop, FR_PROF_CONV_WINOGRAD, exec);
    const bool pre = cw.pre_scale != nullptr;
    hipError_t e = launch_wino4(wp, pre, epi, s);
    if (e != hipSuccess) return fail(h, FR_ERR_HIP, std::string("winograd4 launch: ") + hipGetErrorString(e));
    return FR_OK;
  }
  if (c.w4_blk)  // plan_layouts only sets it for layers the F(4x4) branch above takes
    return fail(h, FR_ERR_HIP, "internal: channel-blocked activations outside the F(4x4) kernel");
  // Winograd F(2x2,3x3) for the stride-1 3x3 convs (f32 parity path only)
  if (h->winograd && h->prec == PREC_F32 && cw.wino && wino_epi(cw, epi, c.res_H, p.Ho)) {
    WinoParams wp{};
    wp.x = c.x;
    wp.u = cw.wino;
    wp.y = c.y;
    wp.pre_scale = cw.pre_scale;
    wp.pre_shift = cw.pre_shift;
    wp.post_scale = cw.post_scale;
    wp.post_shift = cw.post_shift;
    wp.prelu = cw.prelu;
    wp.res = c.res;
    wp.B = c.B;
    wp.H = c.H;
    wp.W = c.W;
    wp.Cin = cw.cin;
    wp.Cout = cw.cout;
    // executed: 16 products per 2x2 output tile (padded tiles included) and (cin, cout) pair
    const double exec = 2.0 * 16.0 * c.B * ((c.H + 1) / 2) * ((c.W + 1) / 2) * (double)cw.cin * cw.cout;
    ProfScope ps(h, s, flop, FR_PROF_CONV_WINOGRAD, exec);
    hipError_t e = launch_wino(wp, cw.pre_scale != nullptr, epi, s);
    if (e != hipSuccess) return fail(h, FR_ERR_HIP, std::string("winograd launch: ") + hipGetErrorString(e));
    return FR_OK;
  }
  // the stage-1 stride-2 conv2 + MaxPool shortcut (64 -> 64 channels) of a batch of >= 16 crops on
  // its band kernel (conv_s2.hip: input rows staged once in LDS for all 9 taps); serving batches
  // keep the split-K direct path below, which spreads a few images' work over every CU
  if (g_knobs.s2band && !h->detector && h->prec == PREC_F32 && epi == EPI_AFFINE_RES_SUB && !cw.pre_scale &&
      cw.cin2 == 0 && nsplit == 1 && c.B >= 16 && c.res_H == c.H && c.res_W == c.W &&
      s2c64_supported(cw.cin, cw.cout, cw.kh, cw.kw, cw.stride, cw.pad, c.H, c.W)) {
    S2Params sp{};
    sp.x = c.x;
    sp.w = cw.w;
    sp.post_scale = cw.post_scale;
    sp.post_shift = cw.post_shift;
    sp.res = c.res;
    sp.y = c.y;
    sp.B = c.B;
    sp.H = c.H;
    sp.W = c.W;
    ProfScope ps(h, s, flop, FR_PROF_CONV_DIRECT);
    const hipError_t e = launch_s2c64(sp, s);
    if (e != hipSuccess) return fail(h, FR_ERR_HIP, std::string("stride-2 band conv launch: ") + hipGetErrorString(e));
    return FR_OK;
  }
  // Round-2 sweep with loads two K-steps ahead on the <= 32-accumulator tiles
  // (profiles/r02/sweep_s2.txt): 128x64/W8 also for the 256-channel stride-2 conv2 (111.9 ->
  // 115.6 TF/s) and 256x128/W8 for the 512-channel shortcut (49.4 -> 63.2).
  ConvTile tile = TILE_256x128_W8;
  if (cw.cout <= 64 || (cw.cout == 128 && epi == EPI_AFFINE_RES && cw.kh == 3) ||
      (cw.cout == 256 && epi == EPI_AFFINE_RES && cw.kh == 3 && cw.stride == 2))
    tile = TILE_128x64_W8;
  else if (cw.kh == 1 && cw.kw == 1 && p.H > 1)
    tile = cw.cout >= 512 ? TILE_256x128_W8 : TILE_128x128_W8;
  else if (p.H == 1)
    tile = TILE_64x128;  // gallery scores (1x1 GEMM)
  // embedding serving batches (M = B*Ho*Wo <= 4096: the stride-2 / 1x1 convs at batch <= ~20):
  // the 64x128 tile gives stream-K more, smaller tiles (batch 1: 2.28 -> 2.15 ms per forward).
  // The detector's tile set (conv_det.hip) has no 64x128 instance.
  // the detector's implicit-GEMM convs (tools/det_conv_sweep.py at the C4 shapes, 32 frames, every
  // tile of the instance sets): the stride-2 3x3 convs of 96 / 224 couts on 128x128/W8 (stage 2 / 3 /
  // 4 conv1: 299 -> 295, 123 -> 117, 77 -> 72 us), the stride-8 lateral 1x1 (M = 204,800, N = 64) on
  // 256x64 (72 -> 64 us); the rest keep the rule's tile (within 5 us of their best)
  if (h->detector && nsplit == 1) {
    if (cw.kh == 3 && cw.cout > 64)
      tile = TILE_128x128_W8;
    else if (cw.kh == 1 && cw.cout <= 64 && p.M >= 131072)
      tile = TILE_256x64;
  }
  if (cw.cin2 > 0 && g_knobs.conv2sc_tile >= 0 && nsplit == 1) tile = (ConvTile)g_knobs.conv2sc_tile;
  if (!h->detector && p.M <= 4096 && nsplit == 1) tile = TILE_64x128;
  // the head FC (split-K) of a serving batch (M = n <= 64 rows) or of <= 256 crops (tools/fc_sweep.py,
  // 32 splits: --batch 128 43.0 us on 128x64/W8 vs 106 on 256x128/W8; --batch 256 69.3 vs 111.8).
  // 129..256 rows on 64x128 (round 3, inside a one-lane IR-101 forward: 75.6 -> 63.9 us,
  // tools/gpu_fc_ab.sh)
  if (!h->detector && nsplit > 1 && cw.kh == 7 && p.M <= 256)
    tile = (p.M <= 64 || p.M > 128) ? TILE_64x128 : TILE_128x64_W8;
  // serving batches: a stride-2 conv2 (+ fused shortcut) as a split-K launch of >= 4 K-steps per
  // split in one round of workgroups, then a parallel fixup, instead of stream-K, whose last
  // arriver per tile summed ~20 slabs of 32 KB alone (batch 1: 26-31 us per launch)
  if (!h->detector && nsplit == 1 && p.M <= 4096 && cw.kh == 3 && h->prec == PREC_F32 && !cw.pre_scale &&
      (epi == EPI_AFFINE || epi == EPI_AFFINE_RES || epi == EPI_AFFINE_RES_SUB) && L.sk_ws && h->cus > 0) {
    const long long ntile = (long long)((p.M + 63) / 64) * ((p.Cout + 127) / 128);
    const long long cap = L.sk_ws_floats / ((long long)p.M * p.Cout);
    int S = (int)std::min<long long>(std::min<long long>(32, p.steps_total / 4), std::min<long long>(h->cus / ntile, cap));
    if (S > 1) {
      ConvParams q = p;
      q.sk_cus = 0;
      q.steps_per_split = (p.steps_total + S - 1) / S;
      S = (p.steps_total + q.steps_per_split - 1) / q.steps_per_split;
      q.split_stride = (long long)p.M * p.Cout;
      q.y = L.sk_ws;
      q.res = nullptr;
      ProfScope ps(h, s, flop, FR_PROF_CONV_DIRECT);
      hipError_t e = launch_conv(q, TILE_64x128, false, EPI_RAW, S, s, h->prec);
      if (e == hipSuccess) e = launch_conv_split_fixup(p, epi, L.sk_ws, S, q.split_stride, s);
      if (e != hipSuccess) return fail(h, FR_ERR_HIP, std::string("conv split-K launch: ") + hipGetErrorString(e));
      return FR_OK;
    }
  }
  ProfScope ps(h, s, flop, FR_PROF_CONV_DIRECT);
  hipError_t e = launch_conv(p, tile, cw.pre_scale != nullptr, epi, nsplit, s, h->prec);
  if (e != hipSuccess) return fail(h, FR_ERR_HIP, std::string("conv launch: ") + hipGetErrorString(e));
  return FR_OK;
}

}  // namespace frhip_rt
