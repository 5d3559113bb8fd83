// The Gauss-Newton core of scan-to-map registration (mapreg.hip) and loop verification (loopverify.hip), float64 (host
// twin: rslo_amd/gauss_newton.py): the 28 addends of a matched point, the fixed-order reduction of the 29 sums over a
// workgroup, and the damped Cholesky step on a pose.  posegraph.hip takes the scalar block sum from here.
//
// gn_register.h builds the registration calls' kernels, launches and argument rules on top of this file.
//
// Like se3.h this header carries no `#pragma clang fp contract`: its functions take the contraction state of the file
// that includes them, so every includer places the include AFTER its own pragma and after se3.h.  All three includers
// switch contraction off, and there every operation below rounds on its own, in the order written.
#pragma once

#define GN_NSUM 29                       /* 21 H (upper triangle, row-major) + 6 g + cost + pairs */

// The 28 addends of a matched point at world position w with residual d, for the world-frame twist (dt, dtheta): the
// three rows of J = [I | -[w]x]; addend of H(a, b) = J0[a]*J0[b] + J1[a]*J1[b] + J2[a]*J2[b], left to right.
// add (a constant at every call): false ASSIGNS t28[k] = addend k, as k_gn_accum needs it (0.0 + (-0.0) would
// lose the sign); true adds, t28[k] = t28[k] + addend k, one addend at a time.  Adding a finished array of addends
// afterwards is the same arithmetic but holds 28 more doubles live: in k_loop_verify, which sits at the 128 registers
// of a 1024-thread workgroup, that is 60 bytes more scratch per thread.
__device__ __forceinline__ void gn_point_terms(const double *w, const double *d, double *t28, bool add) {
  double J[3][6];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) J[a][b] = a == b ? 1.0 : 0.0;
  J[0][3] = 0.0, J[0][4] = w[2], J[0][5] = -w[1];
  J[1][3] = -w[2], J[1][4] = 0.0, J[1][5] = w[0];
  J[2][3] = w[1], J[2][4] = -w[0], J[2][5] = 0.0;
  double v;
  int o = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
#pragma unroll
    for (int b = a; b < 6; ++b, ++o) {
      v = J[0][a] * J[0][b] + J[1][a] * J[1][b] + J[2][a] * J[2][b];
      t28[o] = add ? t28[o] + v : v;
    }
  }
#pragma unroll
  for (int a = 0; a < 6; ++a, ++o) {
    v = J[0][a] * d[0] + J[1][a] * d[1] + J[2][a] * d[2];
    t28[o] = add ? t28[o] + v : v;
  }
  v = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
  t28[o] = add ? t28[o] + v : v;
}

// The 28 addends of a plane term: the one row (n, wn) with wn = w x n, residual r0 = n . d
__device__ __forceinline__ void gn_plane_terms(const double *n, const double *wn, double r0, double *t28) {
  const double J[6] = {n[0], n[1], n[2], wn[0], wn[1], wn[2]};
  int o = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
#pragma unroll
    for (int b = a; b < 6; ++b) t28[o++] = J[a] * J[b];
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) t28[o++] = J[a] * r0;
  t28[o] = r0 * r0;
}

// The 28 addends of a point-to-distribution term: the rows J = [I | -[w]x] of gn_point_terms, residual d = w - mean and
// the symmetric information matrix M of the matched cell (M6: 00 01 02 11 12 22, world frame).  m = M d, B = M J;
// addend of H(k, l) = J0[k]*B0[l] + J1[k]*B1[l] + J2[k]*B2[l], of g(k) = J0[k]*m0 + J1[k]*m1 + J2[k]*m2, of the cost
// e = d0*m0 + d1*m1 + d2*m2, every sum left to right.  Assigns t28 (host twin: gauss_newton.py info_terms).
__device__ __forceinline__ void gn_info_terms(const double *w, const double *d, const double *M6, double *t28) {
  const double M[3][3] = {{M6[0], M6[1], M6[2]}, {M6[1], M6[3], M6[4]}, {M6[2], M6[4], M6[5]}};
  double J[3][6], B[3][6], m[3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) J[a][b] = a == b ? 1.0 : 0.0;
  J[0][3] = 0.0, J[0][4] = w[2], J[0][5] = -w[1];
  J[1][3] = -w[2], J[1][4] = 0.0, J[1][5] = w[0];
  J[2][3] = w[1], J[2][4] = -w[0], J[2][5] = 0.0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    m[a] = M[a][0] * d[0] + M[a][1] * d[1] + M[a][2] * d[2];
#pragma unroll
    for (int k = 0; k < 6; ++k) B[a][k] = M[a][0] * J[0][k] + M[a][1] * J[1][k] + M[a][2] * J[2][k];
  }
  int o = 0;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
#pragma unroll
    for (int l = k; l < 6; ++l) t28[o++] = J[0][k] * B[0][l] + J[1][k] * B[1][l] + J[2][k] * B[2][l];
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) t28[o++] = J[0][k] * m[0] + J[1][k] * m[1] + J[2][k] * m[2];
  t28[o] = d[0] * m[0] + d[1] * m[1] + d[2] * m[2];
}

// The workgroup's sums of the GN_NSUM values of every thread, in a fixed order: lane l takes l + 32, then + 16, ...
// inside its wave, lane 0 leaves the wave's sums in part (LDS, [n_waves, GN_NSUM] doubles), and after a barrier thread
// k < GN_NSUM adds the waves in wave order and writes sum k to dst[k].  Called by every thread of the workgroup; acc is
// overwritten, and dst is not yet visible to the other threads on return.
__device__ __forceinline__ void gn_block_reduce(double *acc, double *part, int n_waves, double *dst) {
#pragma unroll
  for (int k = 0; k < GN_NSUM; ++k) {
    double v = acc[k];
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_down(v, off, 64);
    acc[k] = v;
  }
  if ((threadIdx.x & 63) == 0) {
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < GN_NSUM; ++k) part[wave * GN_NSUM + k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < GN_NSUM) {
    double v = part[threadIdx.x];
    for (int q = 1; q < n_waves; ++q) v = v + part[q * GN_NSUM + threadIdx.x];
    dst[threadIdx.x] = v;
  }
}

// The workgroup's sum of `v` in the same fixed order, valid in every thread.  red: [n_waves] doubles of LDS
__device__ __forceinline__ double gn_block_sum(double v, double *red, int n_waves) {
  for (int off = 32; off > 0; off >>= 1) v = v + __shfl_down(v, off, 64);
  __syncthreads();      // the readers of an earlier sum
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = red[0];
  for (int q = 1; q < n_waves; ++q) s = s + red[q];
  return s;
}

// One thread: the Gauss-Newton step on the sums tot (H upper triangle, g; cost and pairs are not read) at pose7 (t, q).
// M = H + damping * I = L L^T row by row, delta = -M^-1 g = (dt, dr), q' = normalize(dq(dr) (x) q), t' = dt + rotate(dq, t)
// in form B (se3.h).  true: pose7 was advanced, nt = |dt|, th = |dr|.  false: M is not positive definite or the step
// overflowed; pose7 is untouched, nt and th are not meaningful.
__device__ __forceinline__ bool gn_step(const double *tot, double damping, double *pose7, double &nt, double &th) {
  double M[6][6], L[6][6], y[6], x[6];
  int o = 0;
  for (int a = 0; a < 6; ++a)
    for (int b = a; b < 6; ++b) M[a][b] = M[b][a] = tot[o++];
  for (int a = 0; a < 6; ++a) M[a][a] = M[a][a] + damping;
  for (int a = 0; a < 6; ++a) {
    for (int b = 0; b <= a; ++b) {
      double sum = M[a][b];
      for (int k = 0; k < b; ++k) sum = sum - L[a][k] * L[b][k];
      if (a == b) {
        if (!(sum > 0.0 && sum < (double)__builtin_inff())) return false;
        L[a][a] = sqrt(sum);
      } else {
        L[a][b] = sum / L[b][b];
      }
    }
  }
  for (int a = 0; a < 6; ++a) {      // L y = g
    double sum = tot[21 + a];
    for (int k = 0; k < a; ++k) sum = sum - L[a][k] * y[k];
    y[a] = sum / L[a][a];
  }
  for (int a = 5; a >= 0; --a) {     // L^T x = y
    double sum = y[a];
    for (int k = a + 1; k < 6; ++k) sum = sum - L[k][a] * x[k];
    x[a] = sum / L[a][a];
  }
  const double dt[3] = {-x[0], -x[1], -x[2]}, dr[3] = {-x[3], -x[4], -x[5]};
  nt = sqrt(dt[0] * dt[0] + dt[1] * dt[1] + dt[2] * dt[2]);
  th = sqrt(dr[0] * dr[0] + dr[1] * dr[1] + dr[2] * dr[2]);
  if (!(nt < (double)__builtin_inff() && th < (double)__builtin_inff())) return false;      // an overflowed step is no step
  double dq[4], t[3], q[4], b[3], c[3], r[4];
  se3_dquat(dr, th, dq);
  for (int a = 0; a < 3; ++a) t[a] = pose7[a];
  for (int a = 0; a < 4; ++a) q[a] = pose7[3 + a];
  se3_cross(dq + 1, t, b);
  se3_cross(dq + 1, b, c);
  for (int a = 0; a < 3; ++a) pose7[a] = dt[a] + (t[a] + 2.0 * b[a] * dq[0] + 2.0 * c[a]);      // form B
  se3_qmul(dq, q, r);
  const double nr = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3]);
  for (int a = 0; a < 4; ++a) pose7[3 + a] = r[a] / nr;
  return true;
}
