// The pose algebra of the streaming back end on the device, float64 (host twin: rslo_amd/se3.py).  A pose is (t, q) with
// q = (w, x, y, z); rotate(q, v) = v + 2 w (u x v) + 2 u x (u x v) with u = (x, y, z); products are not renormalised
// (the caller divides by the norm where its rule says so); a tangent vector phi is applied through the unit
// quaternion se3_dquat(phi).
//
// This header carries no `#pragma clang fp contract`: its functions take the contraction state of the file that
// includes them, so every includer places the include AFTER its own pragma.  map_table.h (map.hip, mapreg.hip) and
// posegraph.hip switch contraction off, and there every operation below rounds on its own.  pose.hip has no pragma:
// k_pose_chain is compiled with fused multiply-adds and always was.
//
// The rotation is summed in two ways in this project, and the two differ in the last bit:
//   form A  v + (2 b w + 2 c)      se3_rotate: map_point, the normals of mapreg.hip's cost, the pose graph;
//                                  host: se3.rotate, VoxelMapRef
//   form B  (v + 2 b w) + 2 c      the translation updates of k_pose_chain (pose.hip) and gn_step (gauss_newton.h), each
//                                  written out where it is; host: inference.pose_chain_host,
//                                  gauss_newton.gauss_newton_step
// with b = u x v, c = u x b.  Both are correct and both are pinned by bit-equality tests against their host
// restatements, so neither may be turned into the other.
#pragma once

__device__ __forceinline__ void se3_cross(const double *a, const double *b, double *c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// o = q v q^-1 for a unit q, form A
__device__ __forceinline__ void se3_rotate(const double *q, const double *v, double *o) {
  double b[3], c[3];
  se3_cross(q + 1, v, b);
  se3_cross(q + 1, b, c);
  for (int i = 0; i < 3; ++i) o[i] = v[i] + (2.0 * b[i] * q[0] + 2.0 * c[i]);
}

__device__ __forceinline__ void se3_qmul(const double *a, const double *b, double *r) {
  double vx[3];
  se3_cross(a + 1, b + 1, vx);
  r[0] = a[0] * b[0] - (a[1] * b[1] + a[2] * b[2] + a[3] * b[3]);
  for (int i = 0; i < 3; ++i) r[1 + i] = a[1 + i] * b[0] + b[1 + i] * a[0] + vx[i];
}

// A^-1 o B
__device__ __forceinline__ void se3_between(const double *A, const double *B, double *o) {
  const double qc[4] = {A[3], -A[4], -A[5], -A[6]};
  const double d[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]};
  se3_rotate(qc, d, o);
  se3_qmul(qc, B + 3, o + 3);
}

__device__ __forceinline__ void se3_rotmat(const double *q, double *R) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  R[0] = 1.0 - 2.0 * (y * y + z * z), R[1] = 2.0 * (x * y - w * z), R[2] = 2.0 * (x * z + w * y);
  R[3] = 2.0 * (x * y + w * z), R[4] = 1.0 - 2.0 * (x * x + z * z), R[5] = 2.0 * (y * z - w * x);
  R[6] = 2.0 * (x * z - w * y), R[7] = 2.0 * (y * z + w * x), R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// the unit quaternion of the rotation vector phi, theta = |phi| (the caller has it already)
__device__ __forceinline__ void se3_dquat(const double *phi, double theta, double *dq) {
  if (theta < 1e-12) {
    dq[0] = 1.0;
    for (int a = 0; a < 3; ++a) dq[1 + a] = phi[a] / 2.0;
  } else {
    const double f = sin(theta / 2.0) / theta;
    dq[0] = cos(theta / 2.0);
    for (int a = 0; a < 3; ++a) dq[1 + a] = f * phi[a];
  }
}
