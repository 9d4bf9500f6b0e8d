// The similarity fit of FaceAligner.align on gfx950 (cv2.estimateAffinePartial2D with its
// defaults: RANSAC 3 px / 2000 iterations / 0.99 and 10 Levenberg-Marquardt iterations), so that
// detections in HBM become warp descriptors in HBM without a host hop (fr_align_device).
//
// One lane per slot (frame f, face i); the arithmetic is align_fit.h's, bitwise the host's
// fit_similarity.  The work per lane is ~0.2 k double operations per RANSAC iteration, and lanes
// of one wave leave the RANSAC loop when the slowest has its iteration count: latency-bound
// scalar-style code, a few blocks for a batch of frames, not a throughput kernel.  64 lanes per
// block spread the slots over CUs; the launch bound lets the allocator use the whole register
// file of a SIMD for one wave, so the 4 x 5 elimination matrix, J^T J and the residuals stay in
// VGPRs (no scratch).
#include "align_fit.h"

namespace frhip {

// Slot `slot` = (f, i) of p, frame f being src of H x W (unused when p.faces is NULL).
__device__ __forceinline__ void fit_slot(const FitSlots& p, int slot, int f, int i, const uint8_t* src, int H,
                                         int W) {
  const bool live = i < (p.counts ? p.counts[f] : p.max_faces);  // a negative count: no slot
  double M[6];
  bool ok = false;
  if (live) {
    const float* q = p.landmarks + (long long)slot * p.stride;
    float lm[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) lm[k] = q[k];
    ok = fit_similarity5(lm, p.tmpl, p.logs, M);
  } else {
#pragma unroll
    for (int k = 0; k < 6; ++k) M[k] = __builtin_nan("");
  }
  p.ok[slot] = ok ? 1 : 0;
  if (p.tforms) {
#pragma unroll
    for (int k = 0; k < 6; ++k) p.tforms[(long long)slot * 6 + k] = M[k];
  }
  if (p.faces) {
    WarpFace w;
    w.src = src;
    // not ok: no tap of a 0 x 0 source is in range, so warp_pixel reads nothing and writes zeros
    w.H = ok ? H : 0;
    w.W = ok ? W : 0;
    if (ok) {
      invert_affine5(M, w.minv);
    } else {
      w.minv[0] = w.minv[4] = 1.0;
      w.minv[1] = w.minv[2] = w.minv[3] = w.minv[5] = 0.0;
    }
    p.faces[slot] = w;
  }
}

__global__ __launch_bounds__(64) void fit_similarity_kernel(FitSlots p) {
  const int slot = blockIdx.x * 64 + threadIdx.x;
  if (slot >= p.n_frames * p.max_faces) return;
  const int f = slot / p.max_faces, i = slot - f * p.max_faces;
  fit_slot(p, slot, f, i, p.frames + (long long)f * p.H * p.W * 3, p.H, p.W);
}

// The ragged form: frame f is p.images[f], a load per lane from the argument segment (no copy).
__global__ __launch_bounds__(64) void fit_similarity_images_kernel(FitImageSlots p) {
  const int slot = blockIdx.x * 64 + threadIdx.x;
  if (slot >= p.s.n_frames * p.s.max_faces) return;
  const int f = slot / p.s.max_faces, i = slot - f * p.s.max_faces;
  const FitImage im = p.images[f];
  fit_slot(p.s, slot, f, i, im.src, im.H, im.W);
}

hipError_t launch_fit_similarity(const FitSlots& p, hipStream_t s) {
  if (p.n_frames <= 0 || p.max_faces <= 0) return hipSuccess;
  const long long slots = (long long)p.n_frames * p.max_faces;
  if (slots >= (1ll << 31) || !p.landmarks || !p.ok || p.stride < 10 || (p.faces && !p.frames) || p.H < 0 || p.W < 0)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(fit_similarity_kernel, dim3((unsigned)((slots + 63) / 64)), dim3(64), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_fit_similarity_images(const FitImageSlots& p, hipStream_t s) {
  if (p.s.n_frames <= 0 || p.s.max_faces <= 0) return hipSuccess;
  const long long slots = (long long)p.s.n_frames * p.s.max_faces;
  if (slots >= (1ll << 31) || !p.s.landmarks || !p.s.ok || p.s.stride < 10 || p.s.n_frames > FIT_IMAGES_BY_VALUE)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(fit_similarity_images_kernel, dim3((unsigned)((slots + 63) / 64)), dim3(64), 0, s, p);
  return hipGetLastError();
}

}  // namespace frhip
