// Scan de-skewing (rules: include/rslo_hip.h "Scan de-skewing"; float64 restatement: rslo_amd/deskew.py): every point of a
// sweep is moved from the sensor frame at its own time to the sensor frame at `stamp`, under the constant-velocity model
// of LOAM / LIO-SAM: the sensor pose at sweep fraction s is (s t, R^s) for the motion (t, R) of the whole sweep.
//
// One launch, one thread per row.  The motion block {axis, theta, t', status} is a pure function of the arguments; every
// workgroup derives it again (one lane, into LDS, one barrier) instead of waiting for a launch of its own: the kernel
// moves a few megabytes, so a second launch would cost more than the few hundred flops it saves.  Workgroup 0 stores the
// block.  All arithmetic is IEEE double without contraction in the order the header states, the one libm call is the
// atan2 of the block's angle, and the result is rounded to float once, at the store: the per-point result is
// reproducible to the bit in numpy.
#include "rslo_common.h"

#include <math.h>

#pragma clang fp contract(off)

#include "se3.h"      /* the pose algebra, after the pragma: uncontracted here */
#include "azimuth.h"  /* the sweep fraction of an azimuth, likewise */

#define DSK_THREADS 256
#define DSK_HALF_PI AZ_HALF_PI

// Taylor polynomials in Horner form in z = x*x, coefficients the doubles nearest +-1/k!, for |x| <= pi/4
__device__ __forceinline__ double dsk_sin(double x) {
  const double z = x * x;
  double p = -1.0 / 1307674368000.0;
  p = 1.0 / 6227020800.0 + z * p;
  p = -1.0 / 39916800.0 + z * p;
  p = 1.0 / 362880.0 + z * p;
  p = -1.0 / 5040.0 + z * p;
  p = 1.0 / 120.0 + z * p;
  p = -1.0 / 6.0 + z * p;
  p = 1.0 + z * p;
  return x * p;
}

__device__ __forceinline__ double dsk_cos(double x) {
  const double z = x * x;
  double p = 1.0 / 20922789888000.0;
  p = -1.0 / 87178291200.0 + z * p;
  p = 1.0 / 479001600.0 + z * p;
  p = -1.0 / 3628800.0 + z * p;
  p = 1.0 / 40320.0 + z * p;
  p = -1.0 / 720.0 + z * p;
  p = 1.0 / 24.0 + z * p;
  p = -1.0 / 2.0 + z * p;
  p = 1.0 + z * p;
  return p;
}

__device__ __forceinline__ bool dsk_finite(double v) { return fabs(v) < (double)__builtin_inff(); }

// the motion block {a.x, a.y, a.z, theta, t'.x, t'.y, t'.z, status} of one call, by one lane
__device__ void dsk_motion(const float *rel7, const double *pose_a, const double *pose_b, double stamp, double max_angle,
                           double *m) {
  for (int i = 0; i < 7; ++i) m[i] = 0.0;
  if (!rel7 && !pose_a) {
    m[7] = 1.0;
    return;
  }
  double M[7];
  if (rel7) {
    for (int i = 0; i < 7; ++i) M[i] = (double)rel7[i];
  } else {
    double A[7], B[7];
    for (int i = 0; i < 7; ++i) A[i] = pose_a[i], B[i] = pose_b[i];
    se3_between(A, B, M);
  }
  double q[4] = {M[3], M[4], M[5], M[6]};
  const double n2 = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3];
  if (!(n2 > 0.0 && n2 < (double)__builtin_inff()) || !dsk_finite(M[0]) || !dsk_finite(M[1]) || !dsk_finite(M[2])) {
    m[7] = 2.0;
    return;
  }
  const double nrm = sqrt(n2);
  for (int i = 0; i < 4; ++i) q[i] = q[i] / nrm;
  if (q[0] < 0.0)
    for (int i = 0; i < 4; ++i) q[i] = -q[i];
  const double su = sqrt((q[1] * q[1] + q[2] * q[2]) + q[3] * q[3]);
  const double theta = 2.0 * atan2(su, q[0]);
  double a[3] = {0.0, 0.0, 0.0};
  if (su != 0.0)
    for (int i = 0; i < 3; ++i) a[i] = q[1 + i] / su;
  if (theta > max_angle) {
    m[7] = 3.0;
    return;
  }
  const double h = ((-stamp) * theta) * 0.5;
  const double sh = dsk_sin(h);
  const double qs[4] = {dsk_cos(h), sh * a[0], sh * a[1], sh * a[2]};
  double ts[3];
  se3_rotate(qs, M, ts);
  m[0] = a[0], m[1] = a[1], m[2] = a[2], m[3] = theta;
  m[4] = ts[0], m[5] = ts[1], m[6] = ts[2], m[7] = 0.0;
}

__global__ __launch_bounds__(DSK_THREADS) void k_deskew(const float *points, size_t stride, int N, int n_cols,
                                                        int normal_col, const float *__restrict__ times,
                                                        const float *__restrict__ rel7, const double *__restrict__ pose_a,
                                                        const double *__restrict__ pose_b, double stamp,
                                                        double az_start_turn, int az_clockwise, double max_angle,
                                                        float *out, size_t out_stride, double *motion_out) {
  __shared__ double s_m[8];
  if (threadIdx.x == 0) {
    dsk_motion(rel7, pose_a, pose_b, stamp, max_angle, s_m);
    if (blockIdx.x == 0 && motion_out)
      for (int i = 0; i < 8; ++i) motion_out[i] = s_m[i];
  }
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * DSK_THREADS + threadIdx.x;
  if (i >= (size_t)N) return;
  // `out` may be `points` itself (equal strides): neither pointer is __restrict__, a thread touches its own row only and
  // has read x, y, z and the normal before its first store; the other columns go load by load to the same column
  const uint32_t *src = (const uint32_t *)(points + i * stride);
  uint32_t *dst = (uint32_t *)(out + i * out_stride);
  const uint32_t bx = src[0], by = src[1], bz = src[2];
  const double p[3] = {(double)__uint_as_float(bx), (double)__uint_as_float(by), (double)__uint_as_float(bz)};
  bool move = s_m[7] == 0.0 && dsk_finite(p[0]) && dsk_finite(p[1]) && dsk_finite(p[2]);
  double s = 0.0;
  if (move) {
    if (times)
      s = (double)times[i];
    else if (p[0] == 0.0 && p[1] == 0.0)
      move = false;
    else
      s = az_fraction(p[0], p[1], az_start_turn, az_clockwise);
    move = move && dsk_finite(s);
  }
  if (!move) {
    dst[0] = bx, dst[1] = by, dst[2] = bz;
    for (int c = 3; c < n_cols; ++c) dst[c] = src[c];
    return;
  }
  s = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);
  const double alpha = s - stamp;
  const double h = (alpha * s_m[3]) * 0.5;
  const double sh = dsk_sin(h);
  const double qp[4] = {dsk_cos(h), sh * s_m[0], sh * s_m[1], sh * s_m[2]};
  double o[3];
  se3_rotate(qp, p, o);
  for (int a = 0; a < 3; ++a) o[a] = o[a] + alpha * s_m[4 + a];
  float nf[3] = {0.f, 0.f, 0.f};
  if (normal_col >= 0) {
    const float *np_ = (const float *)src + normal_col;
    const double nv[3] = {(double)np_[0], (double)np_[1], (double)np_[2]};
    double no[3];
    se3_rotate(qp, nv, no);
    for (int a = 0; a < 3; ++a) nf[a] = (float)no[a];
  }
  for (int a = 0; a < 3; ++a) ((float *)dst)[a] = (float)o[a];
  for (int c = 3; c < n_cols; ++c) {
    if (normal_col >= 0 && c >= normal_col && c < normal_col + 3)
      ((float *)dst)[c] = nf[c - normal_col];
    else
      dst[c] = src[c];
  }
}

extern "C" int rslo_deskew(const float *points, int stride_floats, int N, int n_cols, int normal_col, const float *times,
                           const float *rel7, const double *pose_a, const double *pose_b, double stamp,
                           double az_start_turn, int az_clockwise, double max_angle, float *out, int out_stride_floats,
                           double *motion_out, void *stream) {
  RSLO_CHECK_ARG(N >= 0, "rslo_deskew: N = %d is negative", N);
  RSLO_CHECK_ARG(N == 0 || (points && out), "rslo_deskew: points and out must not be null");
  RSLO_CHECK_ARG(n_cols >= 3 && n_cols <= stride_floats && n_cols <= out_stride_floats,
                 "rslo_deskew: n_cols = %d must lie in 3 .. the strides (%d, %d)", n_cols, stride_floats, out_stride_floats);
  RSLO_CHECK_ARG(normal_col == -1 || (normal_col >= 3 && normal_col <= n_cols - 3),
                 "rslo_deskew: normal_col = %d must be -1 or lie in 3 .. n_cols - 3", normal_col);
  RSLO_CHECK_ARG(stamp >= 0.0 && stamp <= 1.0, "rslo_deskew: stamp must lie in [0, 1]");
  RSLO_CHECK_ARG(max_angle > 0.0 && max_angle <= DSK_HALF_PI, "rslo_deskew: max_angle must lie in (0, pi/2]");
  RSLO_CHECK_ARG(fabs(az_start_turn) < (double)__builtin_inff(), "rslo_deskew: az_start_turn must be finite");
  RSLO_CHECK_ARG(!(rel7 && (pose_a || pose_b)), "rslo_deskew: give rel7 or the pose pair, not both");
  RSLO_CHECK_ARG((pose_a != nullptr) == (pose_b != nullptr), "rslo_deskew: pose_a and pose_b go together");
  const unsigned blocks = N == 0 ? 1u : (unsigned)rslo_cdiv(N, DSK_THREADS);
  hipLaunchKernelGGL(k_deskew, dim3(blocks), dim3(DSK_THREADS), 0, (hipStream_t)stream, points, (size_t)stride_floats, N,
                     n_cols, normal_col, times, rel7, pose_a, pose_b, stamp, az_start_turn, az_clockwise, max_angle, out,
                     (size_t)out_stride_floats, motion_out);
  RSLO_CHECK_LAUNCH("rslo_deskew");
  return RSLO_OK;
}
