/*
 * frhip_testing.h — kernel-level entry points of libfrhip for parity tests.
 *
 * Not part of the drop-in surface (include/frhip.h): these expose single
 * kernels so tests can compare each against a PyTorch-CPU op of the same shape
 * (one Conv2d of net.BasicBlockIR, the stem, the matcher's top-k).
 * All pointers are device pointers; every call is asynchronous on `stream`.
 */
#ifndef FRHIP_TESTING_H_
#define FRHIP_TESTING_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* y = epi(conv(pre(x))) in NHWC f32, w [cout][kh][kw][cin].
 * epi: 0 affine, 1 affine+PReLU, 2 affine+residual(res same shape as y),
 *      3 affine+residual(res[b][2oy][2ox], res spatial res_h x res_w), 4 raw,
 *      5 PReLU(affine+residual(res same shape as y)), no pre-affine (the detector's BasicBlock conv2).
 * pre_scale/pre_shift may be NULL (no pre-affine).  nsplit > 1 only with epi 4:
 * y then holds nsplit partial slabs of B*Ho*Wo*cout floats.
 * epi 1 without pre-affine and epi 5 run the detector's instances (conv_det.hip: tiles 6, 7, 8
 * only, f32 whatever `precision`); any other tile is refused (FR_ERR_HIP, y untouched).
 * A pointer the epilogue reads that is NULL (post_* unless epi 4, prelu for epi 1 / 5, res for
 * epi 2 / 3 / 5, one of pre_scale / pre_shift alone) or a pre-affine with epi 5 is
 * FR_ERR_INVALID_ARGUMENT before any launch.
 * tile: 0 = 256x64, 1 = 128x128, 2 = 128x64, 3 = 64x128, 4 = 256x128, 5 = 128x256, and with 8
 * waves 6 = 128x128, 7 = 256x128, 8 = 128x64, 9 = 64x256, 10 = 256x64.
 * stream_k: 1 = persistent stream-K schedule (nsplit must be 1), 0 = one block per tile.
 * precision: 0 = f32 MFMA, 1 = bf16x3 split (tiles 1, 3, 4, 6, 7, 8 only). */
int frt_conv2d(const float* x, const float* w, float* y, int B, int H, int W, int cin, int cout, int kh, int kw,
               int stride, int pad, const float* pre_scale, const float* pre_shift, const float* post_scale,
               const float* post_shift, const float* prelu, const float* res, int res_h, int res_w, int epi,
               int nsplit, int tile, int stream_k, int precision, void* stream);
/* frt_conv2d with the kernel's fused 1x1 shortcut (ConvParams::x2 / Cin2 / steps1, set as the
 * runtime sets them for a conv with cin2 > 0): y = epi(conv(x) + conv1x1 stride `stride` (x2)),
 * x2 [B][H][W][cin2], w [cout][kh*kw*cin + cin2] (the shortcut's columns last).  launch_conv
 * refuses cin2 % 32 != 0, a pre-affine and epi 1 / 5 with cin2 > 0 (FR_ERR_HIP, y untouched).
 * cin2 = 0 is frt_conv2d. */
int frt_conv2d_fused(const float* x, const float* x2, const float* w, float* y, int B, int H, int W, int cin, int cin2,
                     int cout, int kh, int kw, int stride, int pad, const float* pre_scale, const float* pre_shift,
                     const float* post_scale, const float* post_shift, const float* prelu, const float* res, int res_h,
                     int res_w, int epi, int nsplit, int tile, int stream_k, int precision, void* stream);
/* The split-K finish of a serving-sized stride-2 conv2 alone (conv_split_fixup_kernel):
 * y [B][Ho][Wo][cout] = epi(sum over s < S of part[s * stride + i], in split order), epi 0, 2 (res
 * shaped like y) or 3 (res [B][res_h][res_w][cout] read at (2 oy, 2 ox)); S in [1, 32], stride >=
 * B*Ho*Wo*cout floats.  Arguments the launcher refuses -> FR_ERR_INVALID_ARGUMENT.  Asynchronous. */
int frt_conv_split_fixup(const float* part, int S, long long stride, int B, int Ho, int Wo, int cout,
                         const float* post_scale, const float* post_shift, const float* res, int res_h, int res_w,
                         int epi, float* y, void* stream);

/* Winograd F(2x2,3x3) stride-1 pad-1 conv (the FR_CONV_WINOGRAD path): same tensors as
 * frt_conv2d with kh = kw = 3; w is the untransformed [cout][3][3][cin] filter (transformed
 * into a scratch buffer here).  epi: 1 (needs pre) or 2 (no pre).  cin, cout % 32 == 0.
 * Synchronises. */
int frt_conv2d_winograd(const float* x, const float* w, float* y, int B, int H, int W, int cin, int cout,
                        const float* pre_scale, const float* pre_shift, const float* post_scale,
                        const float* post_shift, const float* prelu, const float* res, int epi, void* stream);
/* Winograd F(4x4,3x3) (the FR_CONV_WINOGRAD4 path, conv_winograd4.hip), same arguments;
 * cin % 16 == 0, cout % 16 == 0; epi also 0 (affine) and 5 (affine + residual + PReLU), and 1 without
 * pre-BN (the detector's convs).  frt_conv2d_winograd4 gives launch_wino4 a split-K workspace
 * (small grids then split the K loop over items + a reduce pass) unless frt_set_wino4_split(0).
 * frt_conv2d_winograd4_ex's blk: W4_BLK_* bits (1 x, 2 res, 4 y): that tensor is channel-blocked [B][C/16][H][W][16] instead
 * of NHWC; a residual laid out unlike y is for epi 2 only (launch_wino4 refuses epi 5: FR_ERR_HIP). */
int frt_set_wino4_split(int on);
/* A/B (process-wide): the ConvTile of the fused stride-2 conv2 + conv-shortcut launches of
 * non-serving batches (-1: the built-in rule).  Forwards already captured in graphs keep theirs. */
int frt_set_conv2sc_tile(int tile);
/* A/B (process-wide): tile blocks per XCD item group of the F(4x4) launches (0: the built-in rule,
 * 32 items per group; 8 x 8 at 512 channels).  Forwards already captured in graphs keep theirs. */
int frt_set_wino4_nbg(int nbg);
/* A/B (process-wide, default 1): item shapes of whole-item F(4x4) launches without pre-BN.  A layer
 * of 65..96 output channels (the detector's 80/88-channel convs) runs items of 16 tiles x 96 couts
 * (six MFMA waves, two transform waves) instead of two 64-cout items; one of at most 32 (the
 * detector's stem conv and head outputs) items of 32 tiles x 32 couts instead of 64-cout items
 * with two idle MFMA waves.  mode 1: when the 64-cout items take more than one round of
 * workgroups; 2: at every grid size (tests); 0: never.  Graphs captured before keep theirs. */
int frt_set_wino4_shapes(int mode);
/* At most s K parts per item when a small F(4x4) grid runs split-K (0 = no cap; graphs captured
 * before the call keep their schedule). */
int frt_set_wino4_max_split(int s);
/* Poll bound of wino4_kernel's ring hand-off waits (default 65536; n < 0 restores it, 0 makes
 * every wait that does not find its step ready at once expire).  An expired wait stores an error
 * code into the launch's host-pinned error word: handle calls then fail with FR_ERR_HIP ("F(4x4)
 * ring hand-off timed out") -- fr_embed_host / fr_match_topk_host / fr_detect / fr_profile_read
 * after their sync, the asynchronous calls at their next entry -- and frt_conv2d_winograd4 after
 * its sync.  Applies to launches issued after the call (captured graphs keep theirs). */
int frt_set_wino4_poll_limit(int n);
/* The stage-1 stride-2 conv2 (64 -> 64, MaxPool2d(1,2) shortcut) of batches >= 16 on its band
 * kernel (conv_s2.hip, on = 1, default) or on the implicit-GEMM kernel (0).  Handles issue the
 * choice at launch time; graphs captured before the call keep theirs. */
int frt_set_s2_band(int on);
/* The band kernel alone: y [B][H/2][W/2][64] = conv3x3 s2 p1 (x [B][H][W][64], w [64][3][3][64])
 * * post_scale + post_shift + res[b][2oy][2ox] (res [B][H][W][64]); even H, W in [16, 112].
 * Asynchronous on stream. */
int frt_conv2d_s2band(const float* x, const float* w, float* y, int B, int H, int W, const float* post_scale,
                      const float* post_shift, const float* res, void* stream);
/* Handle h runs every body 3x3 conv of forwards of n <= max_n crops (default 2; 0 = never) on the
 * serving-batch kernel (conv_small.hip: one launch per layer, 16 pixels x 16 couts per workgroup
 * with the whole K reduction inside it) instead of F(4x4) split-K + fixup and the split-K direct
 * convs.  Drops captured graphs. */
int frt_set_small_conv(fr_handle* h, int max_n);
/* Output-pixel limit (n * Ho * Wo) of a batch-1 layer on the serving kernel (default 4,096:
 * stage 1's 56x56 layers join stages 2-4; 1,024 keeps them on F(4x4) split-K).  A/B only. */
int frt_set_small_conv_pixels(fr_handle* h, int max_m1);
/* A/B switch (default on): in a one-lane forward, a body conv2 on the serving kernel also writes
 * BN(y) for the next block's conv1 (its pre-activation BN), which then runs without pre-BN. */
int frt_set_small_conv_pre_epilogue(fr_handle* h, int on);
/* A/B switch (default on): in a forward the serving kernel does not take (n > 2 crops),
 * activations passed between two F(4x4) layers are stored channel-blocked ([n][C/16][H][W][16])
 * instead of NHWC (bitwise the same embeddings). */
int frt_set_wino4_blocked(fr_handle* h, int on);
/* A/B switch (default on): in a one-lane forward, activations passed between two layers on the
 * serving kernel are stored channel-blocked ([n][C/16][H][W][16]) instead of NHWC. */
int frt_set_small_conv_blocked(fr_handle* h, int on);
/* The serving-batch kernel alone: y = epi(conv3x3 pad 1 stride s (x) [+ conv1x1 stride s (x2)
 * against weight columns 9*cin .. + cin2]), w [cout][9*cin + cin2]; pre-BN only with epi 1 (epi 1
 * without it is the instance conv1 runs on a y2 input);
 * epi 0, 1, 2 (res shaped like y) or 3 (res [B][H][W][cout], read at (s oy, s ox)).
 * blk: CONVS_BLK_* bits (1 x, 2 x2, 4 res, 8 y): that tensor is channel-blocked
 * [B][C/16][H][W][16] instead of NHWC.  y2 (nullable): also y2 = y * y2_scale[c] + y2_shift[c], in
 * y's shape and layout.  cin, cout, cin2 % 16 == 0.  What launch_convs refuses (pre-BN with another
 * epilogue or more than 512 channels, cin2 > 256 or without x2, a missing epilogue operand, y2
 * without its scale / shift) is FR_ERR_INVALID_ARGUMENT with y untouched.  Synchronises the stream
 * before it returns (it frees the temporary fragment-order copy of w it launched with).
 * frt_conv2d_small is frt_conv2d_small_ex with blk = 0 and no y2 (its callers' signature stays). */
int frt_conv2d_small_ex(const float* x, const float* x2, const float* w, float* y, int B, int H, int W, int cin,
                        int cin2, int cout, int stride, const float* pre_scale, const float* pre_shift,
                        const float* post_scale, const float* post_shift, const float* prelu, const float* res, int epi,
                        int blk, float* y2, const float* y2_scale, const float* y2_shift, void* stream);
int frt_conv2d_small(const float* x, const float* x2, const float* w, float* y, int B, int H, int W, int cin,
                     int cin2, int cout, int stride, const float* pre_scale, const float* pre_shift,
                     const float* post_scale, const float* post_shift, const float* prelu, const float* res, int epi,
                     void* stream);
/* Handle h runs the stride-2 conv2 of a block with a conv shortcut and that shortcut as one
 * GEMM (on = 1, default: BN scales folded into the weights, extra K-steps over the block input)
 * or as two launches (0).  Drops captured graphs. */
int frt_set_fuse_shortcut(fr_handle* h, int on);
int frt_conv2d_winograd4(const float* x, const float* w, float* y, int B, int H, int W, int cin, int cout,
                         const float* pre_scale, const float* pre_shift, const float* post_scale,
                         const float* post_shift, const float* prelu, const float* res, int epi, void* stream);
/* (frt_conv2d_winograd4 is this with blk = 0) */
int frt_conv2d_winograd4_ex(const float* x, const float* w, float* y, int B, int H, int W, int cin, int cout,
                            const float* pre_scale, const float* pre_shift, const float* post_scale,
                            const float* post_shift, const float* prelu, const float* res, int epi, int blk,
                            void* stream);

/* Fused preprocess + input_layer on uint8 RGB [B][112][112][3]; w27x64 is the
 * repacked [ky][kx][c_rgb][64] weight; lut the 256-entry normalisation table. */
int frt_stem(const uint8_t* img, int B, const float* lut, const float* w27x64, const float* bn_scale,
             const float* bn_shift, const float* prelu, float* y, void* stream);

/* head_reduce_kernel alone: emb [n][512] = tail(sum over s < nsplit of partial[s * split_stride +
 * row * 512 + c] + fc_bias[c]) * bn_scale[c] + bn_shift[c], then x / ||x|| with model_l2 and
 * e / (||e|| + 1e-8) with normalize.  nsplit < 1, split_stride < n * 512, n < 1 or a null pointer
 * is FR_ERR_INVALID_ARGUMENT before any launch.  Asynchronous on stream. */
int frt_head_reduce(const float* partial, int nsplit, long long split_stride, const float* fc_bias,
                    const float* bn_scale, const float* bn_shift, float* emb, int n, int normalize, int model_l2,
                    void* stream);

/* The host similarity fit of fr_align_faces: src/dst float [n][2] -> M double [2][3]. */
int frt_fit_similarity(const float* src, const float* dst, int n, double* M);

/* The device similarity fit of fr_align_device alone: n landmark sets (host float [n][5][2]) against
 * the reference template of out_size -> M (host double [n][2][3], NaN where ok is 0) and ok (host
 * uint8 [n]).  Stages through temporary device buffers on the current device and synchronises.
 * With ms != NULL also the kernel's time between two HIP events of one more launch (milliseconds). */
int frt_fit_similarity_device(const float* landmarks, int n, int out_size, double* M, uint8_t* ok, float* ms);

/* warp_affine_images_kernel (the ragged warp of fr_align_images / fr_align_device) on caller-supplied
 * FORWARD maps: tforms host double [n_faces][2][3], each inverted with the runtime's invert_affine
 * into the WarpFace of its face exactly as fr_align_images fills it (images / sizes / face_image as
 * fr_align_images takes them; out device uint8 [n_faces][S][S][3]).  The same argument checks as
 * fr_align_images (FR_ERR_INVALID_ARGUMENT, out untouched).  Stages through a temporary device
 * buffer and synchronises.  Contract domain of the warp kernels (csrc/warp_map.h): finite maps whose
 * source positions stay within +-2^40 px; there the crop is bitwise oracle/align_ref.py's. */
int frt_warp_affine_images(const uint8_t* const* images, const int32_t* sizes, int n_images,
                           const int32_t* face_image, const double* tforms, int n_faces, int out_size, uint8_t* out,
                           void* stream);
/* letterbox_kernel alone: n frames uint8 [n][H][W][3] resized to new_w x new_h (cv2.resize INTER_LINEAR)
 * into the top-left of zero dw x dh canvases, out [n][dh][dw][3].  The tables are
 * resize_axis_table(new_w, W) then resize_axis_table(new_h, H) and simd_end =
 * resize_simd_end(new_w * 3), laid out as the detector's setup_geometry lays them out.
 * frt_letterbox_images: letterbox_images_kernel alone, image i of sizes[i] = (h, w) resized to
 * new_sizes[i] = (new_h, new_w), descriptors and tables staged as the detector's letterbox_images
 * stages them.  new_w > dw, new_h > dh, a side < 1 and what the launchers refuse (dw * 3 % 4 != 0, out
 * not 4-byte aligned) are FR_ERR_INVALID_ARGUMENT with out untouched.  Both synchronise. */
int frt_letterbox(const uint8_t* frames, int n, int H, int W, int new_w, int new_h, int dw, int dh, uint8_t* out,
                  void* stream);
int frt_letterbox_images(const uint8_t* const* images, const int32_t* sizes, const int32_t* new_sizes, int n, int dw,
                         int dh, uint8_t* out, void* stream);
/* The host's resize_simd_end: where the SSE2-rounded part of a resized row of row_elems bytes ends. */
int frt_resize_simd_end(int row_elems);
/* The resize coefficient table of one axis, [dsize][4] = (src0, src1, w0, w1): frt_resize_axis_table
 * the host's (resize_axis_table), frt_resize_tables_device resize_tables_kernel's for an image whose
 * two axes are both (dsize, ssize), copied back (its x and y tables must agree: FR_ERR_STATE
 * otherwise).  out: host int32 [dsize][4].  Synchronises. */
int frt_resize_axis_table(int dsize, int ssize, int32_t* out);
int frt_resize_tables_device(int dsize, int ssize, int32_t* out);
/* FIT_IMAGES_BY_VALUE: the images one fit launch of fr_align_images_device takes by value. */
int frt_fit_images_by_value(void);

/* fr_quality_gate_device on the CPU: the same per-slot arithmetic (csrc/gate_math.h, compiled for the
 * host) and the same rank / pack rules, every buffer in host memory; no handle, no stream.  The
 * same argument checks.  yaw and roll go through the host's double atan2 / asin, the device's
 * through its own: they may differ by one float32 ulp at a rounding boundary, all else is bitwise. */
int frt_quality_gate_host(const float* dets, const int32_t* counts, const uint8_t* ok, const double* blur,
                          int n_frames, int max_faces, const fr_gate_config* cfg, uint8_t* stage, double* metrics,
                          int32_t* bbox, int32_t* rank, int32_t* rows, int32_t* frame_offsets, int32_t* valid_slots,
                          int32_t* n_valid);

/* The detector stem's MaxPool2d(3, 2, 1) alone: x [B][H][W][C] -> y [B][(H+1)/2][(W+1)/2][C], NHWC
 * f32, C % 4 == 0, 16-byte aligned.  Asynchronous on stream. */
int frt_maxpool3(const float* x, int B, int H, int W, int C, float* y, void* stream);
/* The detector's other glue kernels alone (detect.hip), NHWC f32, C % 4 == 0, 16-byte aligned,
 * asynchronous on stream; arguments the launchers refuse -> FR_ERR_INVALID_ARGUMENT.
 * frt_upsample_add: big [B][2h][2w][C] += nearest-2x(small [B][h][w][C]) (the FPN top-down add).
 * frt_avgpool2:     y [B][H/2][W/2][C] = AvgPool2d(2, 2)(x [B][H][W][C]); even H and W.
 * frt_row_expand:   y [B][Hd][W][C]: row r of x [B][Hs][W][C] above row m, Hd - Hs + 1 copies of row
 *                   m, then the rows below it (detector.cpp row_plan); 0 <= m < Hs <= Hd. */
int frt_upsample_add(float* big, const float* small, int B, int h, int w, int C, void* stream);
int frt_avgpool2(const float* x, int B, int H, int W, int C, float* y, void* stream);
int frt_row_expand(const float* x, int B, int Hs, int W, int C, int m, int Hd, float* y, void* stream);
/* The detector stem alone: y [B][H/2][W/2][C] = relu(conv3x3 s2 p1((img - 127.5) / 128) * scale + shift),
 * img uint8 [B][H][W][3], w27xC the repacked [ky][kx][c][C] weight; C in {8, 16, 24, 32}, even H, W.
 * C = 16 / 32 with W % 32 == 0 and even H / 2 run the MFMA kernel unless force_scalar. */
int frt_det_stem(const uint8_t* img, int B, int H, int W, int C, const float* w27xC, const float* scale,
                 const float* shift, float* y, int force_scalar, void* stream);

/* Row-wise top-k of a [n][G] score matrix (score desc, equal scores by descending index; k in [1, G]). */
int frt_topk(const float* scores, int n, int G, int k, int32_t* idx, float* val, void* stream);
/* The same with the tie order chosen: low_index_first != 0 ranks equal scores by ASCENDING index
 * (the instances fr_match_identities launches), 0 is frt_topk.  NaN never ranks; a row with fewer
 * than k rankable scores ends in idx -1 / val -inf.  scores needs 4-byte alignment only. */
int frt_topk_ex(const float* scores, int n, int G, int k, int low_index_first, int32_t* idx, float* val,
                void* stream);

/* Process-wide: fr_identity_scores scores at most `probes` probes per GEMM chunk (0: the built-in
 * rule, the most whose [probes][G] score matrix stays below 2 GiB), so a test can put a chunk seam
 * inside a small batch. */
int frt_set_eval_chunk(int probes);
/* Process-wide: the path of fr_match_identities / fr_embed_match_identities.  0: the built-in rule
 * (the fused kernel for one query and for n <= 16 queries with n * rows <= 65,536, else the composed
 * path); 1: the fused kernel for every n;
 * 2: the composed path for every n (its GEMM chunks follow frt_set_eval_chunk).  Tests put both
 * paths on the same inputs. */
int frt_set_identify_path(int mode);
/* Process-wide: the row cap of the fused kernel's tiles, read by the next fr_samples_set (1..1024;
 * 0: the default).  An identity longer than the cap is a tile of its own.  A/B of the tile size. */
int frt_set_identify_tile_rows(int rows);

/* Detector internals of fr_detect for n <= max_frames frames: letterbox + network only.
 * heads: device f32, the three levels' maps back to back, each [n][H/s][W/s][32] for
 * s = 8, 16, 32 (channels: cls a0, cls a1 logits | bbox a0 (4), a1 (4) | kps a0 (10), a1 (10)
 * in stride units | 2 zero pads); canvas: device uint8 [n][640][640][3] letterboxed frames,
 * or NULL.  Synchronises. */
int frt_detector_forward(fr_handle* h, const uint8_t* frames, int n, int height, int width, float* heads,
                         uint8_t* canvas, void* stream);
/* The same for one chunk of fr_detect_images: n <= max_frames images of their own sizes (images /
 * sizes as fr_detect_images takes them), run exactly as fr_detect_images runs that chunk: per-image
 * letterbox, the chunk's row plan (none with row reduction switched off: the full canvas).  heads and
 * canvas as above, canvas i the full 640-row canvas of image i.  Synchronises. */
int frt_detector_forward_images(fr_handle* h, const uint8_t* const* images, const int32_t* sizes, int n, float* heads,
                                uint8_t* canvas, void* stream);
/* The post-processing of fr_detect / fr_detect_images alone, on caller-supplied head maps: heads
 * (device, the layout frt_detector_forward writes, n <= max_frames frames) is copied into the
 * detector's own head buffers and the product's decode + sort + NMS + copy-out runs on them.
 * det_scales: NULL (every frame decodes with det_scale, as fr_detect does) or a host array of n
 * per-frame scales (uploaded and handed to the kernel, as fr_detect_images does).  dets: host
 * [n][max_faces][15], counts: host [n], as fr_detect fills them.  Synchronises. */
int frt_detector_postprocess(fr_handle* h, const float* heads, int n, float det_scale, const float* det_scales,
                             float det_thresh, int max_faces, float* dets, int32_t* counts, void* stream);
/* A/B: the stem and stage 1 skip the letterbox's invariant bottom rows (on, the default) or run
 * the full 640-row canvas (0).  Both compute the same network to fp32 rounding. */
int frt_set_detector_row_reduction(fr_handle* h, int on);

#ifdef __cplusplus
}
#endif
#endif /* FRHIP_TESTING_H_ */
