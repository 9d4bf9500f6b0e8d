// fit_similarity (align_host.cpp) for 5 points, restated so that one GPU lane can run it out of
// registers: every array index is a compile-time constant (the loops are fully unrolled, a runtime
// point index is a chain of selects, solve4's row swap is a chain of conditional moves, the
// RANSAC inlier set is a bit mask that the sums skip by instead of a compacted copy), so nothing
// is addressed at run time and nothing has to live in scratch memory.  Same IEEE operations in the
// same order as the host function, with fp contraction off: the doubles are bitwise the host's
// (tests/test_gpu_device_chain.py).  The functions are __host__ __device__: tools/fit_check.cpp
// runs them on the CPU against fit_similarity under the host sanitizers.
//
// What is not computed here: the two logarithms of RANSACUpdateNumIters.  Its confidence is the
// constant 0.99 and its outlier ratio (5 - g) / 5 takes six values, so the host passes
// log(1 - 0.99) and the six log(1 - (g / 5)^2) by value (FitLogs, from the same std::log the host
// fit calls); the comparison, the division and the rounding are exact and are done here.
#pragma once
#include "frhip_kernels.h"

#define FRHIP_FIT_FN __host__ __device__ __forceinline__

// Every operation rounds on its own, as the host's (this stays in force for the including file).
#pragma clang fp contract(off)

namespace frhip {

namespace fit {

constexpr double kDblEps = 2.220446049250313e-16, kFltEps = 1.1920928955078125e-07;
constexpr int kMaxIters = 2000, kLmIters = 10;
// bound of the "second index differs from the first" redraw (the host's loop has none): the
// index stream does not depend on the data, and its longest run of redraws within the 2000
// iterations is 5 (tools/fit_check.cpp counts it), so the bound is never reached
constexpr int kRedrawMax = 64;

// std::max / std::min as the host calls them (a NaN second argument is dropped, a NaN first kept)
FRHIP_FIT_FN double mx(double a, double b) { return a < b ? b : a; }
FRHIP_FIT_FN double mn(double a, double b) { return b < a ? b : a; }

// cv::RNG, seeded with ~0
FRHIP_FIT_FN unsigned rng_next(uint64_t& st) {
  st = (uint64_t)(unsigned)st * 4164903690u + (unsigned)(st >> 32);
  return (unsigned)st;
}

// element i of a[5] by selects
template <typename T>
FRHIP_FIT_FN T pick5(T a0, T a1, T a2, T a3, T a4, int i) {
  return i == 0 ? a0 : (i == 1 ? a1 : (i == 2 ? a2 : (i == 3 ? a3 : a4)));
}

FRHIP_FIT_FN void kernel2(double x1, double y1, double x2, double y2, double X1, double Y1, double X2, double Y2,
                          double H[6]) {
  const double den = (x1 - x2) * (x1 - x2) + (y1 - y2) * (y1 - y2);
  const double d = den != 0 ? 1. / den : __builtin_inf();
  const double S0 = d * ((X1 - X2) * (x1 - x2) + (Y1 - Y2) * (y1 - y2));
  const double S1 = d * ((Y1 - Y2) * (x1 - x2) - (X1 - X2) * (y1 - y2));
  const double S2 =
      d * ((Y1 - Y2) * (x1 * y2 - x2 * y1) - (X1 * y2 - X2 * y1) * (y1 - y2) - (X1 * x2 - X2 * x1) * (x1 - x2));
  const double S3 =
      d * (-(X1 - X2) * (x1 * y2 - x2 * y1) - (Y1 * x2 - Y2 * x1) * (x1 - x2) - (Y1 * y2 - Y2 * y1) * (y1 - y2));
  H[0] = H[4] = S0;
  H[1] = -S1;
  H[2] = S2;
  H[3] = S1;
  H[5] = S3;
}

// computeError + findInliers in float32: bit i of *mask = point i within 3 px; returns the count
FRHIP_FIT_FN int find_inliers(const double M[6], const float* src, const float* dst, unsigned* mask) {
  const float F0 = (float)M[0], F1 = (float)M[1], F2 = (float)M[2], F3 = (float)M[3], F4 = (float)M[4],
              F5 = (float)M[5];
  const float t = (float)(3.0 * 3.0);
  unsigned bits = 0;
  int nz = 0;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const float a = F0 * src[2 * i] + F1 * src[2 * i + 1] + F2 - dst[2 * i];
    const float b = F3 * src[2 * i] + F4 * src[2 * i + 1] + F5 - dst[2 * i + 1];
    const bool in = a * a + b * b <= t;
    bits |= in ? 1u << i : 0u;
    nz += in;
  }
  *mask = bits;
  return nz;
}

// update_num_iters(0.99, (5 - g) / 5, max_iters) with the logarithms from lg
FRHIP_FIT_FN int update_num_iters(const FitLogs& lg, int g, int max_iters) {
  if ((lg.den_zero >> g) & 1) return 0;
  const double num = lg.log_num;
  const double denom = g <= 0   ? lg.log_den[0]
                       : g == 1 ? lg.log_den[1]
                       : g == 2 ? lg.log_den[2]
                       : g == 3 ? lg.log_den[3]
                       : g == 4 ? lg.log_den[4]
                                : lg.log_den[5];
  return denom >= 0 || -num >= max_iters * (-denom) ? max_iters : (int)__builtin_rint(num / denom);
}

// solve4 of the host: Gaussian elimination with partial pivoting, a zero pivot leaves its unknown 0.
// The pivot search keeps the best row so far by value (the host keeps its index) and the swap is
// conditional moves: the same rows end in the same places.
FRHIP_FIT_FN void solve4(const double A[4][4], const double b[4], double x[4]) {
  double M[4][5];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) M[i][j] = A[i][j];
    M[i][4] = b[i];
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    double best[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) best[k] = M[c][k];
    int p = c;
#pragma unroll
    for (int r = c + 1; r < 4; ++r)
      if (__builtin_fabs(M[r][c]) > __builtin_fabs(best[c])) {
#pragma unroll
        for (int k = 0; k < 5; ++k) best[k] = M[r][k];
        p = r;
      }
#pragma unroll
    for (int r = c + 1; r < 4; ++r)
      if (p == r) {
#pragma unroll
        for (int k = 0; k < 5; ++k) M[r][k] = M[c][k];
      }
#pragma unroll
    for (int k = 0; k < 5; ++k) M[c][k] = best[k];
    if (M[c][c] != 0.0) {
#pragma unroll
      for (int r = c + 1; r < 4; ++r) {
        const double f = M[r][c] / M[c][c];
#pragma unroll
        for (int k = c; k < 5; ++k) M[r][k] = M[r][k] - f * M[c][k];
      }
    }
  }
#pragma unroll
  for (int c = 3; c >= 0; --c) {
    x[c] = 0.0;
    if (M[c][c] != 0.0) {
      double s = M[c][4];
#pragma unroll
      for (int k = c + 1; k < 4; ++k) s = s - M[c][k] * x[k];
      x[c] = s / M[c][c];
    }
  }
}

// refine_compute's residuals for all 5 points (the sums below read the inliers' only)
FRHIP_FIT_FN void residuals(const double h[4], const double* src, const double* dst, double r[10]) {
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const double Mx = src[2 * i], My = src[2 * i + 1];
    const double xi = h[0] * Mx - h[1] * My + h[2];
    const double yi = h[1] * Mx + h[0] * My + h[3];
    r[2 * i] = xi - dst[2 * i];
    r[2 * i + 1] = yi - dst[2 * i + 1];
  }
}

// refine_compute's normal equations A = J^T J, v = J^T r over the inliers, in index order.  The
// host sums over a compacted copy of the inliers; skipping the others adds the same terms in the
// same order.  J's zero entries stay in the sums as products, as on the host.
FRHIP_FIT_FN void normal_equations(const double* src, const double* r, unsigned mask, double A[4][4], double v[4]) {
  double J[10][4];
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const double Mx = src[2 * i], My = src[2 * i + 1];
    J[2 * i][0] = Mx, J[2 * i][1] = -My, J[2 * i][2] = 1., J[2 * i][3] = 0.;
    J[2 * i + 1][0] = My, J[2 * i + 1][1] = Mx, J[2 * i + 1][2] = 0., J[2 * i + 1][3] = 1.;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 10; ++k)
        if ((mask >> (k / 2)) & 1) s += J[k][i] * J[k][j];
      A[i][j] = s;
    }
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 10; ++k)
      if ((mask >> (k / 2)) & 1) s += J[k][i] * r[k];
    v[i] = s;
  }
}

FRHIP_FIT_FN double sumsq(const double* r, unsigned mask) {
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < 10; ++k)
    if ((mask >> (k / 2)) & 1) s += r[k] * r[k];
  return s;
}

FRHIP_FIT_FN double dot4(const double* a, const double* b) {
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) s += a[i] * b[i];
  return s;
}

// LMSolverImpl::run as the host's lm_refine runs it, over the points of mask
FRHIP_FIT_FN void lm_refine(double x[4], const double* src, const double* dst, unsigned mask) {
  double r[10], rd[10], A[4][4], v[4], D[4];
  residuals(x, src, dst, r);
  normal_equations(src, r, mask, A, v);
  double S = sumsq(r, mask);
#pragma unroll
  for (int i = 0; i < 4; ++i) D[i] = A[i][i];
  const double Rlo = 0.25, Rhi = 0.75;
  double lambda = 1, lc = 0.75;
#pragma unroll 1
  for (int iter = 0; iter < kLmIters;) {
    double Ap[4][4], d[4], xd[4], temp[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) Ap[i][j] = A[i][j] + (i == j ? lambda * D[i] : 0.0);
    solve4(Ap, v, d);
#pragma unroll
    for (int i = 0; i < 4; ++i) xd[i] = x[i] - d[i];
    residuals(xd, src, dst, rd);
    const double Sd = sumsq(rd, mask);
#pragma unroll
    for (int i = 0; i < 4; ++i) temp[i] = -dot4(A[i], d) + 2.0 * v[i];
    const double dS = dot4(d, temp);
    const double R = (S - Sd) / (__builtin_fabs(dS) > kDblEps ? dS : 1.0);
    if (R > Rhi) {
      lambda *= 0.5;
      if (lambda < lc) lambda = 0;
    } else if (R < Rlo) {
      const double t = dot4(d, v);
      double nu = (Sd - S) / (__builtin_fabs(t) > kDblEps ? t : 1.0) + 2.0;
      nu = mn(mx(nu, 2.0), 10.0);
      if (lambda == 0) {
        double maxval = kDblEps;
#pragma unroll 1
        for (int i = 0; i < 4; ++i) {
          double e[4], col[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) e[k] = k == i ? 1.0 : 0.0;
          solve4(A, e, col);
          const double ci = i == 0 ? col[0] : (i == 1 ? col[1] : (i == 2 ? col[2] : col[3]));
          maxval = mx(maxval, __builtin_fabs(ci));
        }
        lambda = lc = 1.0 / maxval;
        nu *= 0.5;
      }
      lambda *= nu;
    }
    if (Sd < S) {
      S = Sd;
#pragma unroll
      for (int i = 0; i < 4; ++i) x[i] = xd[i];
      residuals(x, src, dst, r);
      normal_equations(src, r, mask, A, v);
    }
    ++iter;
    double md = 0.0, mr = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) md = mx(md, __builtin_fabs(d[i]));
#pragma unroll
    for (int k = 0; k < 10; ++k)
      if ((mask >> (k / 2)) & 1) mr = mx(mr, __builtin_fabs(r[k]));
    if (!(md >= kFltEps && mr >= kFltEps)) break;
  }
}

}  // namespace fit

// fit_similarity(src_f, dst_f, 5, M): false (M NaN) where the host returns false.
FRHIP_FIT_FN bool fit_similarity5(const float* src_f, const float* dst_f, const FitLogs& lg, double M[6]) {
  using namespace fit;
#pragma unroll
  for (int i = 0; i < 6; ++i) M[i] = __builtin_nan("");
  double src[10], dst[10];
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    src[i] = src_f[i];
    dst[i] = dst_f[i];
  }
  uint64_t st = ~0ull;
  unsigned best_mask = 0;
  double best[6] = {0, 0, 0, 0, 0, 0};
  int niters = kMaxIters, good = 0;
#pragma unroll 1
  for (int it = 0; it < niters; ++it) {
    const int i0 = (int)(rng_next(st) % 5u);
    int i1 = (int)(rng_next(st) % 5u);
#pragma unroll 1
    for (int redraw = 0; i1 == i0 && redraw < kRedrawMax; ++redraw) i1 = (int)(rng_next(st) % 5u);
    const double x1 = pick5(src[0], src[2], src[4], src[6], src[8], i0);
    const double y1 = pick5(src[1], src[3], src[5], src[7], src[9], i0);
    const double x2 = pick5(src[0], src[2], src[4], src[6], src[8], i1);
    const double y2 = pick5(src[1], src[3], src[5], src[7], src[9], i1);
    const double X1 = pick5(dst[0], dst[2], dst[4], dst[6], dst[8], i0);
    const double Y1 = pick5(dst[1], dst[3], dst[5], dst[7], dst[9], i0);
    const double X2 = pick5(dst[0], dst[2], dst[4], dst[6], dst[8], i1);
    const double Y2 = pick5(dst[1], dst[3], dst[5], dst[7], dst[9], i1);
    double Mi[6];
    kernel2(x1, y1, x2, y2, X1, Y1, X2, Y2, Mi);
    unsigned mask;
    const int g = find_inliers(Mi, src_f, dst_f, &mask);
    if (g > (good > 1 ? good : 1)) {
#pragma unroll
      for (int i = 0; i < 6; ++i) best[i] = Mi[i];
      best_mask = mask;
      good = g;
      niters = update_num_iters(lg, g, niters);
    }
  }
  if (good <= 0) return false;
  double h[4] = {best[0], best[3], best[2], best[5]};
  lm_refine(h, src, dst, best_mask);
  M[0] = M[4] = h[0];
  M[1] = -h[1];
  M[2] = h[2];
  M[3] = h[1];
  M[5] = h[3];
  return true;
}

// invert_affine of the host (warpAffine's double-precision inverse)
FRHIP_FIT_FN void invert_affine5(const double Mf[6], double Mi[6]) {
  double m0 = Mf[0], m1 = Mf[1], m2 = Mf[2], m3 = Mf[3], m4 = Mf[4], m5 = Mf[5];
  double D = m0 * m4 - m1 * m3;
  D = D != 0 ? 1. / D : 0;
  const double A11 = m4 * D, A22 = m0 * D;
  m0 = A11;
  m1 *= -D;
  m3 *= -D;
  m4 = A22;
  const double b1 = -m0 * m2 - m1 * m5;
  const double b2 = -m3 * m2 - m4 * m5;
  Mi[0] = m0, Mi[1] = m1, Mi[2] = b1, Mi[3] = m3, Mi[4] = m4, Mi[5] = b2;
}

}  // namespace frhip
