// Enrollment augmentation on gfx950: the reference's augment_face_for_enrollment
// (enroll_students.py:20-48) for the first 14 entries of its list, so the copies of a face are
// made where fr_embed reads them.  Variant v of a crop, all uint8-exact:
//   0      the crop                      1      cv2.flip(img, 1)
//   2..5   warpAffine about (W/2, H/2) by -10, -5, 5, 10 degrees, INTER_LINEAR,
//          BORDER_REPLICATE (the fixed-point map and weights of warp_map.h; each of the four
//          taps clamped on its own, OpenCV's remapBilinear replicate branch)
//   6..9   clip(p + beta, 0, 255), beta -20, -10, 10, 20
//   10..13 clip(float32(p) * float32(alpha), 0, 255) truncated, alpha 0.85, 0.92, 1.08, 1.15,
//          from a host-built table
// A pure HBM gather / scatter: out is A times the input (40 crops of 224 x 224, A = 8: 6 MB in,
// 48 MB out).
#include "frhip_kernels.h"
#include "warp_map.h"

namespace frhip {

namespace {

constexpr int AUG_PIX = 4;  // pixels per work-item: 12 output bytes, three dword stores

__device__ __forceinline__ uint8_t aug_point(int v, int p, const uint8_t* lut) {
  if (v < 6) return (uint8_t)p;
  if (v < 10) {
    const int beta = v < 8 ? (v - 8) * 10 : (v - 7) * 10;  // -20, -10, 10, 20
    const int q = p + beta;
    return (uint8_t)(q < 0 ? 0 : (q > 255 ? 255 : q));
  }
  return lut[p];
}

}  // namespace

// One work-item per AUG_PIX consecutive pixels of one output image; a block's 256 items lie in one
// (face, variant) image, so the variant is uniform per block.  Blocks walk the
// n * A * blocks-per-image list with a grid stride (no grid dimension has to hold n * A).
// vec: H * W % 4 == 0 and both buffers 4-byte aligned, so every item's 12 bytes are whole dwords.
__global__ __launch_bounds__(256) void augment_kernel(const uint8_t* __restrict__ crops, long long nimg, int A,
                                                      int H, int W, AugTables tab, int vec,
                                                      uint8_t* __restrict__ out) {
  __shared__ uint8_t s_lut[256];
  const int HW = H * W;
  const int groups = (HW + AUG_PIX - 1) / AUG_PIX;
  const int bpi = (groups + 255) / 256;
  const long long total = nimg * bpi;
  const int tid = threadIdx.x;
  for (long long b = blockIdx.x; b < total; b += gridDim.x) {
    const long long img = b / bpi;
    const int chunk = (int)(b - img * bpi);
    const long long face = img / A;
    const int v = (int)(img - face * A);
    if (v >= 10) {  // uniform per block
      __syncthreads();
      s_lut[tid] = tab.lut[v - 10][tid];
      __syncthreads();
    }
    const int g = chunk * 256 + tid;
    if (g >= groups) continue;
    const int p0 = g * AUG_PIX;
    const int np = min(AUG_PIX, HW - p0);
    const uint8_t* src = crops + face * HW * 3;
    uint8_t* dst = out + (img * HW + p0) * 3;
    uint8_t px[AUG_PIX * 3] = {};  // static indices only, so it stays in registers
    if (v == 0 || v >= 6) {
      if (vec) {
        const uint32_t* s4 = reinterpret_cast<const uint32_t*>(src + (long long)p0 * 3);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const uint32_t w = s4[k];
#pragma unroll
          for (int j = 0; j < 4; ++j) px[k * 4 + j] = aug_point(v, (w >> (8 * j)) & 255, s_lut);
        }
      } else {
#pragma unroll
        for (int k = 0; k < AUG_PIX * 3; ++k)
          if (k < np * 3) px[k] = aug_point(v, src[(long long)p0 * 3 + k], s_lut);
      }
    } else if (v == 1) {
      int y = p0 / W, x = p0 - y * W;  // one division per work-item; the pixels follow in row order
#pragma unroll
      for (int k = 0; k < AUG_PIX; ++k) {
        if (k < np) {
          const uint8_t* q = src + ((long long)y * W + (W - 1 - x)) * 3;
          px[k * 3] = q[0];
          px[k * 3 + 1] = q[1];
          px[k * 3 + 2] = q[2];
        }
        if (++x == W) {
          x = 0;
          ++y;
        }
      }
    } else {
      const double* m = tab.minv[v - 2];
      int y = p0 / W, x = p0 - y * W;
      WarpRow row = warp_row(m, y);  // again only where the work-item's pixels cross into the next row
#pragma unroll
      for (int k = 0; k < AUG_PIX; ++k) {
        if (k < np) {
          const WarpTap t = warp_tap(m, row, x);
          const int x0 = min(max(t.sx, 0), W - 1), x1 = min(max(t.sx + 1, 0), W - 1);
          const int y0 = min(max(t.sy, 0), H - 1), y1 = min(max(t.sy + 1, 0), H - 1);
          const uint8_t* r0 = src + (long long)y0 * W * 3;
          const uint8_t* r1 = src + (long long)y1 * W * 3;
#pragma unroll
          for (int c = 0; c < 3; ++c)
            px[k * 3 + c] = warp_blend(t, r0[x0 * 3 + c], r0[x1 * 3 + c], r1[x0 * 3 + c], r1[x1 * 3 + c]);
        }
        if (++x == W) {
          x = 0;
          ++y;
          row = warp_row(m, y);
        }
      }
    }
    if (vec) {
      uint32_t* d4 = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
      for (int k = 0; k < 3; ++k)
        d4[k] = (uint32_t)px[k * 4] | ((uint32_t)px[k * 4 + 1] << 8) | ((uint32_t)px[k * 4 + 2] << 16) |
                ((uint32_t)px[k * 4 + 3] << 24);
    } else {
#pragma unroll
      for (int k = 0; k < AUG_PIX * 3; ++k)
        if (k < np * 3) dst[k] = px[k];
    }
  }
}

hipError_t launch_augment(const uint8_t* crops, int n, int H, int W, int A, const AugTables& tab, uint8_t* out,
                          hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (H < 1 || W < 1 || H > 8192 || W > 8192 || A < 1 || A > AUG_VARIANTS) return hipErrorInvalidValue;
  const long long HW = (long long)H * W;
  const long long bpi = ((HW + AUG_PIX - 1) / AUG_PIX + 255) / 256;
  const long long total = (long long)n * A * bpi;
  const int vec = HW % 4 == 0 && (reinterpret_cast<uintptr_t>(crops) & 3) == 0 &&
                  (reinterpret_cast<uintptr_t>(out) & 3) == 0;
  const unsigned grid = (unsigned)(total < (1ll << 20) ? total : (1ll << 20));
  hipLaunchKernelGGL(augment_kernel, dim3(grid), dim3(256), 0, s, crops, (long long)n * A, A, H, W, tab, vec, out);
  return hipGetLastError();
}

}  // namespace frhip
