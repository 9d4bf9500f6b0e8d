// The quality gate of FaceQualityFilter.is_valid for one detection row, stated once for the GPU
// kernel (gate.hip) and for the host restatement (frt_quality_gate_host): the tests of is_valid in
// is_valid's order, the first failing one being the slot's stage, and the sort key of
// FaceProcessor.process_numpy.
//
// Everything but two calls is plain IEEE arithmetic with every operation rounding on its own
// (fp contraction off), so host and device agree bit for bit.  The two calls are atan2 and asin:
// they are taken in DOUBLE and rounded to float32, which pins yaw and roll to the correctly rounded
// float32 value except where the double result lies within a double-library error of a float32
// rounding boundary (two conforming libraries then differ by one float32 ulp).  numpy's own float32
// arctan2 / arcsin are up to 4 ulp off that value and depend on the host's SIMD library, so
// "bitwise numpy" is not a property anything could have; "within a derived bound of numpy" is
// (the device quality gate).
//
// No array is indexed at run time: the row is read with constant offsets and the results travel in
// scalars, so a GPU lane runs this out of registers.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "frhip.h"
#include "frhip_kernels.h"

#define FRHIP_GATE_FN __host__ __device__ __forceinline__

namespace frhip {

// fr_gate_config as the comparisons take it: the pose limits rounded to float32 (numpy 2 compares a
// float32 angle with a Python scalar in float32), the others in double.
struct GateLimits {
  double min_det_score, min_face_size, blur_threshold;
  float max_yaw, max_pitch, max_roll;
  int check_blur;  // the blur test runs (cfg->check_blur and a blur array)
};

// false: a limit that is not finite or lies beyond +-FLT_MAX (its float32 image would be infinite)
inline bool gate_limits(const fr_gate_config& c, bool have_blur, GateLimits* g) {
  const double v[6] = {c.min_det_score, c.min_face_size, c.max_yaw, c.max_pitch, c.max_roll, c.blur_threshold};
  for (double x : v)
    if (!(x >= -(double)FLT_MAX && x <= (double)FLT_MAX)) return false;  // NaN fails both
  g->min_det_score = c.min_det_score;
  g->min_face_size = c.min_face_size;
  g->blur_threshold = c.blur_threshold;
  g->max_yaw = (float)c.max_yaw;
  g->max_pitch = (float)c.max_pitch;
  g->max_roll = (float)c.max_roll;
  g->check_blur = c.check_blur && have_blur;
  return true;
}

struct GateSlot {
  int stage;
  int x0, y0, x1, y1;                          // d[:4].astype(np.int32)
  double det_score, blur_score, yaw, pitch, roll;  // 0.0 where the early exit never computes them
  double key;                                  // det_score * (blur_score if recorded else 1000)
};

namespace gate {
constexpr float kDeg = 180.0f / (float)M_PI;  // np.degrees on float32: the float32 quotient 57.295776f
}

// d: the 15 floats of a detection row (x0 y0 x1 y1 score, 5 x (x, y)); fit_ok: fr_align_device's ok
// of the slot (1 without one); blur: the slot's blur score (read only when lim.check_blur).
FRHIP_GATE_FN GateSlot gate_slot(const float* d, int fit_ok, double blur, const GateLimits& lim) {
#pragma clang fp contract(off)  // every operation rounds on its own, on the host and on the device
  GateSlot r;
  r.x0 = (int)d[0];
  r.y0 = (int)d[1];
  r.x1 = (int)d[2];
  r.y1 = (int)d[3];
  r.det_score = (double)d[4];
  r.blur_score = r.yaw = r.pitch = r.roll = 0.0;
  r.key = r.det_score * 1000.0;
  r.stage = FR_GATE_DET_SCORE;
  if (r.det_score < lim.min_det_score) return r;
  const int w = r.x1 - r.x0, h = r.y1 - r.y0;
  const int face_size = w < h ? w : h;
  r.stage = FR_GATE_FACE_SIZE;
  if ((double)face_size < lim.min_face_size) return r;
  // compute_pose_angles in float32: landmarks left eye, right eye, nose, left mouth, right mouth
  const float lex = d[5], ley = d[6], rex = d[7], rey = d[8], nx = d[9], ny = d[10], lmy = d[12], rmy = d[14];
  const float ecx = (lex + rex) / 2.0f, ecy = (ley + rey) / 2.0f;
  const float dx = rex - lex, dy = rey - ley;
  const float dist = sqrtf(dx * dx + dy * dy);
  float ratio = (nx - ecx) / dist;
  ratio = ratio < -1.0f ? -1.0f : (ratio > 1.0f ? 1.0f : ratio);  // np.clip: a NaN stays a NaN
  const float roll = (float)atan2((double)dy, (double)dx) * gate::kDeg;
  const float yaw = (float)asin((double)ratio) * gate::kDeg * 2.0f;
  const float mcy = (lmy + rmy) / 2.0f;
  const float pitch = ((ny - ecy) / (mcy - ecy) - 0.5f) * 60.0f;
  r.yaw = (double)yaw;
  r.pitch = (double)pitch;
  r.roll = (double)roll;
  r.stage = FR_GATE_POSE;
  // a NaN angle compares false and passes, as on the host
  if (fabsf(yaw) > lim.max_yaw || fabsf(pitch) > lim.max_pitch || fabsf(roll) > lim.max_roll) return r;
  if (lim.check_blur) {
    r.blur_score = blur;
    r.key = r.det_score * blur;
    r.stage = FR_GATE_BLUR;
    if (blur < lim.blur_threshold) return r;
  }
  r.stage = fit_ok ? FR_GATE_VALID : FR_GATE_FIT;
  return r;
}

// Live slots of a frame: min(count, F), none for a negative count, all without counts.
FRHIP_GATE_FN int gate_live(const int32_t* counts, int f, int F) {
  if (!counts) return F;
  const int c = counts[f];
  return c < 0 ? 0 : (c < F ? c : F);
}

// key_j ranks before key_i in process_numpy's stable sort(reverse=True)
FRHIP_GATE_FN bool gate_before(double kj, int j, double ki, int i) { return kj > ki || (kj == ki && j < i); }

// Device pointers of one fr_quality_gate_device call (gate.hip).
struct GateArgs {
  const float* dets;
  const int32_t* counts;
  const uint8_t* ok;
  const double* blur;
  int n_frames, F;
  GateLimits lim;
  uint8_t* stage;
  double* metrics;
  int32_t *bbox, *rank, *rows, *frame_offsets, *valid_slots, *n_valid;
  int32_t* frame_valid;  // workspace [n_frames]: valid slots per frame, written by the first launch
};
// Two launches, one workgroup of 256 threads per frame each: gate + rank, then prefixes + scatter.
// 1 <= F <= FR_GATE_MAX_FACES, n_frames >= 1.
hipError_t launch_quality_gate(const GateArgs& a, hipStream_t s);

}  // namespace frhip
