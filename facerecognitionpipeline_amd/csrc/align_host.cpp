// FaceAligner (face_recognition.py:50-75) host side: cv2.estimateAffinePartial2D with its
// defaults (RANSAC 3 px / 2000 iterations / 0.99, 10 LM refine iterations), restating OpenCV's
// ptsetreg.cpp + levmarq.cpp, and warpAffine's inverse.  Same IEEE operation order as
// oracle/align_ref.py (fit_similarity and helpers), so both produce identical doubles.
// Also the host tables of fr_augment_faces.  Pure host code: no HIP call in this file.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "runtime.h"

using namespace frhip;

namespace frhip_rt {

#pragma clang fp contract(off)
namespace {
constexpr double kDblMin = 2.2250738585072014e-308, kDblEps = 2.220446049250313e-16;
constexpr double kFltEps = 1.1920928955078125e-07;

// cv::RNG (core/rand.cpp): 64-bit multiply-with-carry
struct CvRng {
  uint64_t state;
  explicit CvRng(uint64_t s) : state(s ? s : 0xffffffffull) {}
  unsigned next() {
    state = (uint64_t)(unsigned)state * 4164903690u + (unsigned)(state >> 32);
    return (unsigned)state;
  }
  int uniform(int a, int b) { return a == b ? a : (int)(next() % (unsigned)(b - a) + (unsigned)a); }
};

// AffinePartial2DEstimatorCallback::runKernel: the similarity through 2 point pairs
void kernel2(const double f[4], const double t[4], double H[6]) {
  const double x1 = f[0], y1 = f[1], x2 = f[2], y2 = f[3];
  const double X1 = t[0], Y1 = t[1], X2 = t[2], Y2 = t[3];
  const double den = (x1 - x2) * (x1 - x2) + (y1 - y2) * (y1 - y2);
  const double d = den != 0 ? 1. / den : INFINITY;
  const double S0 = d * ((X1 - X2) * (x1 - x2) + (Y1 - Y2) * (y1 - y2));
  const double S1 = d * ((Y1 - Y2) * (x1 - x2) - (X1 - X2) * (y1 - y2));
  const double S2 = d * ((Y1 - Y2) * (x1 * y2 - x2 * y1) - (X1 * y2 - X2 * y1) * (y1 - y2) - (X1 * x2 - X2 * x1) * (x1 - x2));
  const double S3 = d * (-(X1 - X2) * (x1 * y2 - x2 * y1) - (Y1 * x2 - Y2 * x1) * (x1 - x2) - (Y1 * y2 - Y2 * y1) * (y1 - y2));
  H[0] = H[4] = S0;
  H[1] = -S1;
  H[2] = S2;
  H[3] = S1;
  H[5] = S3;
}

// computeError (float32 model and arithmetic) + findInliers
int find_inliers(const double M[6], const float* src, const float* dst, int n, double thr, bool* mask) {
  const float F0 = (float)M[0], F1 = (float)M[1], F2 = (float)M[2], F3 = (float)M[3], F4 = (float)M[4], F5 = (float)M[5];
  const float t = (float)(thr * thr);
  int nz = 0;
  for (int i = 0; i < n; ++i) {
    const float a = F0 * src[2 * i] + F1 * src[2 * i + 1] + F2 - dst[2 * i];
    const float b = F3 * src[2 * i] + F4 * src[2 * i + 1] + F5 - dst[2 * i + 1];
    mask[i] = a * a + b * b <= t;
    nz += mask[i];
  }
  return nz;
}

// RANSACUpdateNumIters, (1 - ep)^2 as one product
int update_num_iters(double p, double ep, int max_iters) {
  p = std::min(std::max(p, 0.), 1.);
  ep = std::min(std::max(ep, 0.), 1.);
  double num = std::max(1. - p, kDblMin);
  const double q = 1. - ep;
  double denom = 1. - q * q;
  if (denom < kDblMin) return 0;
  num = std::log(num);
  denom = std::log(denom);
  return denom >= 0 || -num >= max_iters * (-denom) ? max_iters : (int)std::nearbyint(num / denom);
}

// Gaussian elimination with partial pivoting (n = 4); a zero pivot leaves its unknown 0
void solve4(const double A[4][4], const double b[4], double x[4]) {
  double M[4][5];
  for (int i = 0; i < 4; ++i) {
    for (int j = 0; j < 4; ++j) M[i][j] = A[i][j];
    M[i][4] = b[i];
  }
  for (int c = 0; c < 4; ++c) {
    int p = c;
    for (int r = c + 1; r < 4; ++r)
      if (std::fabs(M[r][c]) > std::fabs(M[p][c])) p = r;
    if (p != c)
      for (int k = 0; k < 5; ++k) std::swap(M[c][k], M[p][k]);
    if (M[c][c] == 0.0) continue;
    for (int r = c + 1; r < 4; ++r) {
      const double f = M[r][c] / M[c][c];
      for (int k = c; k < 5; ++k) M[r][k] = M[r][k] - f * M[c][k];
    }
  }
  for (int c = 3; c >= 0; --c) {
    x[c] = 0.0;
    if (M[c][c] == 0.0) continue;
    double s = M[c][4];
    for (int k = c + 1; k < 4; ++k) s = s - M[c][k] * x[k];
    x[c] = s / M[c][c];
  }
}

// AffinePartial2DRefineCallback::compute, h = (a, b, tx, ty): residuals r[2n] and, if J, the
// normal equations A = J^T J, v = J^T r (sums in index order)
void refine_compute(const double h[4], const double* src, const double* dst, int n, double* r, double A[4][4],
                    double v[4]) {
  for (int i = 0; i < n; ++i) {
    const double Mx = src[2 * i], My = src[2 * i + 1];
    const double xi = h[0] * Mx - h[1] * My + h[2];
    const double yi = h[1] * Mx + h[0] * My + h[3];
    r[2 * i] = xi - dst[2 * i];
    r[2 * i + 1] = yi - dst[2 * i + 1];
  }
  if (!A) return;
  double J[16][4];
  for (int i = 0; i < n; ++i) {
    const double Mx = src[2 * i], My = src[2 * i + 1];
    const double j0[4] = {Mx, -My, 1., 0.}, j1[4] = {My, Mx, 0., 1.};
    for (int c = 0; c < 4; ++c) {
      J[2 * i][c] = j0[c];
      J[2 * i + 1][c] = j1[c];
    }
  }
  for (int i = 0; i < 4; ++i) {
    for (int j = 0; j < 4; ++j) {
      double s = 0.0;
      for (int k = 0; k < 2 * n; ++k) s += J[k][i] * J[k][j];
      A[i][j] = s;
    }
    double s = 0.0;
    for (int k = 0; k < 2 * n; ++k) s += J[k][i] * r[k];
    v[i] = s;
  }
}

double sumsq(const double* r, int m) {
  double s = 0.0;
  for (int i = 0; i < m; ++i) s += r[i] * r[i];
  return s;
}

double dot4(const double* a, const double* b) {
  double s = 0.0;
  for (int i = 0; i < 4; ++i) s += a[i] * b[i];
  return s;
}

double maxabs(const double* a, int m) {
  double s = 0.0;
  for (int i = 0; i < m; ++i) s = std::max(s, std::fabs(a[i]));
  return s;
}

// LMSolverImpl::run (levmarq.cpp, OpenCV 3.x-4.5)
void lm_refine(double x[4], const double* src, const double* dst, int n, int max_iters) {
  double r[16], rd[16], A[4][4], v[4], D[4];
  refine_compute(x, src, dst, n, r, A, v);
  double S = sumsq(r, 2 * n);
  for (int i = 0; i < 4; ++i) D[i] = A[i][i];
  const double Rlo = 0.25, Rhi = 0.75;
  double lambda = 1, lc = 0.75;
  for (int iter = 0;;) {
    double Ap[4][4], d[4], xd[4], temp[4];
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) Ap[i][j] = A[i][j] + (i == j ? lambda * D[i] : 0.0);
    solve4(Ap, v, d);
    for (int i = 0; i < 4; ++i) xd[i] = x[i] - d[i];
    refine_compute(xd, src, dst, n, rd, nullptr, nullptr);
    const double Sd = sumsq(rd, 2 * n);
    for (int i = 0; i < 4; ++i) temp[i] = -dot4(A[i], d) + 2.0 * v[i];  // gemm(A, d, -1, v, 2)
    const double dS = dot4(d, temp);
    const double R = (S - Sd) / (std::fabs(dS) > kDblEps ? dS : 1.0);
    if (R > Rhi) {
      lambda *= 0.5;
      if (lambda < lc) lambda = 0;
    } else if (R < Rlo) {
      const double t = dot4(d, v);
      double nu = (Sd - S) / (std::fabs(t) > kDblEps ? t : 1.0) + 2.0;
      nu = std::min(std::max(nu, 2.0), 10.0);
      if (lambda == 0) {
        double maxval = kDblEps;
        for (int i = 0; i < 4; ++i) {
          double e[4] = {0, 0, 0, 0}, col[4];
          e[i] = 1.0;
          solve4(A, e, col);
          maxval = std::max(maxval, std::fabs(col[i]));
        }
        lambda = lc = 1.0 / maxval;
        nu *= 0.5;
      }
      lambda *= nu;
    }
    if (Sd < S) {
      S = Sd;
      memcpy(x, xd, sizeof(xd));
      refine_compute(x, src, dst, n, r, A, v);
    }
    ++iter;
    if (!(iter < max_iters && maxabs(d, 4) >= kFltEps && maxabs(r, 2 * n) >= kFltEps)) break;
  }
}
}  // namespace

bool fit_similarity(const float* src_f, const float* dst_f, int n, double M[6]) {
  for (int i = 0; i < 6; ++i) M[i] = NAN;
  if (n < 2 || n > 8) return false;
  double src[16], dst[16];
  for (int i = 0; i < 2 * n; ++i) {
    src[i] = src_f[i];
    dst[i] = dst_f[i];
  }
  if (n == 2) {
    kernel2(src, dst, M);
    return true;
  }
  CvRng rng(~0ull);
  bool mask[8], best_mask[8];
  double best[6];
  int niters = 2000, good = 0;
  for (int it = 0; it < niters; ++it) {
    const int i0 = rng.uniform(0, n);
    int i1 = rng.uniform(0, n);
    while (i1 == i0) i1 = rng.uniform(0, n);
    const double f[4] = {src[2 * i0], src[2 * i0 + 1], src[2 * i1], src[2 * i1 + 1]};
    const double t[4] = {dst[2 * i0], dst[2 * i0 + 1], dst[2 * i1], dst[2 * i1 + 1]};
    double Mi[6];
    kernel2(f, t, Mi);
    const int g = find_inliers(Mi, src_f, dst_f, n, 3.0, mask);
    if (g > std::max(good, 1)) {
      memcpy(best, Mi, sizeof(best));
      memcpy(best_mask, mask, sizeof(mask));
      good = g;
      niters = update_num_iters(0.99, (double)(n - g) / n, niters);
    }
  }
  if (good <= 0) return false;
  double si[16], di[16];
  int m = 0;
  for (int i = 0; i < n; ++i)
    if (best_mask[i]) {
      si[2 * m] = src[2 * i];
      si[2 * m + 1] = src[2 * i + 1];
      di[2 * m] = dst[2 * i];
      di[2 * m + 1] = dst[2 * i + 1];
      ++m;
    }
  double h[4] = {best[0], best[3], best[2], best[5]};
  lm_refine(h, si, di, m, 10);
  M[0] = M[4] = h[0];
  M[1] = -h[1];
  M[2] = h[2];
  M[3] = h[1];
  M[5] = h[3];
  return true;
}

// The logarithms update_num_iters takes in fit_similarity's calls for n = 5 (p = 0.99,
// ep = (5 - g) / 5 for g inliers), with its clamps and its std::log: what the device fit
// (align_fit.h) gets by value in place of a device log.
void fit_logs(FitLogs* lg) {
  const double p = std::min(std::max(0.99, 0.), 1.);
  lg->log_num = std::log(std::max(1. - p, kDblMin));
  lg->den_zero = 0;
  for (int g = 0; g <= 5; ++g) {
    const double ep = std::min(std::max((double)(5 - g) / 5, 0.), 1.);
    const double q = 1. - ep;
    const double denom = 1. - q * q;
    const bool zero = denom < kDblMin;
    if (zero) lg->den_zero |= 1 << g;
    lg->log_den[g] = zero ? 0.0 : std::log(denom);
  }
}

void invert_affine(const double Mf[6], double Mi[6]) {
  double m[6];
  memcpy(m, Mf, sizeof(m));
  double D = m[0] * m[4] - m[1] * m[3];
  D = D != 0 ? 1. / D : 0;
  const double A11 = m[4] * D, A22 = m[0] * D;
  m[0] = A11;
  m[1] *= -D;
  m[3] *= -D;
  m[4] = A22;
  const double b1 = -m[0] * m[2] - m[1] * m[5];
  const double b2 = -m[3] * m[2] - m[4] * m[5];
  m[2] = b1;
  m[5] = b2;
  memcpy(Mi, m, sizeof(m));
}

// Host tables of fr_augment_faces for crops of H x W (enroll_students.py:26-39).  Rotations:
// cv2.getRotationMatrix2D((W / 2, H / 2), angle, 1.0) in double, as OpenCV builds it, inverted as
// warpAffine inverts it.  Contrast: numpy multiplies a float32 array by a Python float in float32,
// clips in float32 and truncates.
void augment_tables(int H, int W, AugTables* t) {
  const double angles[4] = {-10, -5, 5, 10};
  const double cx = W / 2, cy = H / 2;
  for (int i = 0; i < 4; ++i) {
    const double rad = angles[i] * (M_PI / 180);
    const double a = std::cos(rad), b = std::sin(rad);
    const double Mf[6] = {a, b, (1 - a) * cx - b * cy, -b, a, b * cx + (1 - a) * cy};
    invert_affine(Mf, t->minv[i]);
  }
  const double alphas[4] = {0.85, 0.92, 1.08, 1.15};
  for (int i = 0; i < 4; ++i) {
    const float alpha = (float)alphas[i];
    for (int p = 0; p < 256; ++p) {
      float r = (float)p * alpha;
      r = r < 0.f ? 0.f : (r > 255.f ? 255.f : r);
      t->lut[i][p] = (uint8_t)r;
    }
  }
}
#pragma clang fp contract(on)

void reference_template(int S, float t[10]) {
  const double r[10] = {0.34, 0.46, 0.66, 0.46, 0.50, 0.61, 0.37, 0.74, 0.63, 0.74};
  for (int i = 0; i < 10; ++i) t[i] = (float)(r[i] * S);
}

}  // namespace frhip_rt
