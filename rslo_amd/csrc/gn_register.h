// The Gauss-Newton registration scaffold of the map backends (mapreg.hip: the voxel map; surfel.hip: the plane and the
// distribution cost of the surfel map): everything between a backend's "the 28 addends of this point" and the C ABI --
// the workspace, the accumulate kernel, the second stage with the step and the info row, the launches of one
// evaluation, the iteration loop and the argument rules the calls share.  A backend supplies a Cost (below) and its own
// argument checks.
//
// Like gauss_newton.h this header carries no `#pragma clang fp contract`: include it AFTER the includer's pragma and after
// gauss_newton.h.  One object per .hip and no relocatable device code: the kernels here have internal linkage, every
// includer gets its own copy.
#pragma once

#define GN_BLOCK 256
#define GN_WS_HDR 256                    /* workspace: 256-byte header (int32 word 0: the "converged" flag) | block partials */
#define GN_MAX_ITERS 32

struct GnSolve {
  int min_pairs;
  double damping, tol_t, tol_r;
  int row;                 // the info row of this iteration (`iter` counts inside a stage, the rows run on)
  double stage, level;     // info columns 5 and 6 (0 outside a schedule)
};

// block partial [GN_NSUM] of the addends of points blockIdx.x * 256 .. + 255 at the pose in pose7.  Cost: a trivially
// copyable struct (map, cap_max, voxel and the backend's parameters) with
//   __device__ bool terms(const float *p, const double *pose, double max_dist, double *acc) const
// which, for a point with a usable match, ASSIGNS the 28 addends (gauss_newton.h: 0.0 + (-0.0) would lose the sign)
// and returns true.  WEIGHTED: the 28 addends of a matched point are multiplied by rho = u*u, u = s2 / (s2 + e), e its
// cost addend (s2 = scale*scale > 0); the other instantiation is the unweighted kernel, to the bit.
template <class Cost, bool WEIGHTED>
static __global__ __launch_bounds__(GN_BLOCK) void k_gn_accum(Cost cost, const float *__restrict__ points, int stride, int N,
                                                              const double *__restrict__ pose, double max_dist, int iter,
                                                              const int32_t *__restrict__ flag,
                                                              double *__restrict__ partials, double s2) {
  if (iter > 0 && *flag) return;      // converged in an earlier iteration: the second stage does not read the partials
  __shared__ double part[GN_BLOCK / 64 * GN_NSUM];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double acc[GN_NSUM];
#pragma unroll
  for (int k = 0; k < GN_NSUM; ++k) acc[k] = 0.0;
  if (i < N && cost.terms(points + (int64_t)i * stride, pose, max_dist, acc)) {
    acc[GN_NSUM - 1] = 1.0;
    if (WEIGHTED) {      // e = acc[27] >= 0 (or NaN, which stays NaN as it would unweighted); s2 > 0: u is in [0, 1]
      const double u = s2 / (s2 + acc[GN_NSUM - 2]);
      const double rho = u * u;
#pragma unroll
      for (int k = 0; k < GN_NSUM - 1; ++k) acc[k] = rho * acc[k];
    }
  }
  gn_block_reduce(acc, part, GN_BLOCK / 64, partials + (size_t)blockIdx.x * GN_NSUM);
}

// Second stage, one wave: lane j sums partial j of the blocks in block order.  out29 (the normal_eq calls) receives the
// sums; with pose7 (the register calls) lane 0 then takes the Gauss-Newton step of iteration `iter` and writes its info row.
// Iteration 0 (of a call, or of a stage of a schedule) does not read the flag and rewrites it: that clears it.
static __global__ __launch_bounds__(64) void k_gn_finish(const double *__restrict__ partials, int n_blocks,
                                                         double *__restrict__ out29, double *__restrict__ pose7, int iter,
                                                         GnSolve sp, int32_t *__restrict__ flag, double *__restrict__ info) {
  __shared__ double tot[GN_NSUM];
  double *row = info ? info + (size_t)sp.row * 8 : nullptr;
  if (pose7 && iter > 0 && *flag) {
    if (threadIdx.x < 8)
      row[threadIdx.x] = threadIdx.x == 0 ? 3.0 : threadIdx.x == 5 ? sp.stage : threadIdx.x == 6 ? sp.level : 0.0;
    return;
  }
  if (threadIdx.x < GN_NSUM) {
    double v = 0.0;
    for (int b = 0; b < n_blocks; ++b) v = v + partials[(size_t)b * GN_NSUM + threadIdx.x];
    tot[threadIdx.x] = v;
    if (out29) out29[threadIdx.x] = v;
  }
  __syncthreads();
  if (!pose7 || threadIdx.x != 0) return;
  int status = 0;
  double nt = 0.0, th = 0.0;
  const double pairs = tot[28], cost = tot[27];
  if (pairs < (double)sp.min_pairs) {
    status = 1;
  } else if (!gn_step(tot, sp.damping, pose7, nt, th)) {
    status = 2;      // not positive definite, or an overflowed step: no step
    nt = th = 0.0;
  }
  *flag = (status == 0 && nt < sp.tol_t && th < sp.tol_r) ? 1 : 0;
  row[0] = (double)status;
  row[1] = pairs;
  row[2] = cost;
  row[3] = nt;
  row[4] = th;
  row[5] = sp.stage;
  row[6] = sp.level;
  row[7] = 0.0;
}

// the launches of one evaluation of the normal equations (+ the step of iteration `iter` when pose_rw is given)
template <class Cost>
static void gn_evaluate(const Cost &cost, const float *points, int stride, int N, const double *pose, double max_dist,
                        double scale, double *out29, double *pose_rw, int iter, const GnSolve &sp, double *info, void *ws,
                        hipStream_t s) {
  int32_t *flag = (int32_t *)ws;
  double *partials = (double *)((unsigned char *)ws + GN_WS_HDR);
  const int nb = (int)rslo_cdiv(N, GN_BLOCK);
  if (nb > 0 && scale == 0.0)      // no weights: the unweighted kernel, to the bit
    hipLaunchKernelGGL((k_gn_accum<Cost, false>), dim3((unsigned)nb), dim3(GN_BLOCK), 0, s, cost, points, stride, N, pose,
                       max_dist, iter, (const int32_t *)flag, partials, 0.0);
  else if (nb > 0)
    hipLaunchKernelGGL((k_gn_accum<Cost, true>), dim3((unsigned)nb), dim3(GN_BLOCK), 0, s, cost, points, stride, N, pose,
                       max_dist, iter, (const int32_t *)flag, partials, scale * scale);
  hipLaunchKernelGGL(k_gn_finish, dim3(1), dim3(64), 0, s, (const double *)partials, nb, out29, pose_rw, iter, sp, flag, info);
}

// the normal equations alone, into out29
template <class Cost>
static void gn_normal_eq(const Cost &cost, const float *points, int stride, int N, const double *pose7, double max_dist,
                         double scale, double *out29, void *ws, hipStream_t s) {
  const GnSolve sp = {0, 0.0, 0.0, 0.0, 0, 0.0, 0.0};
  gn_evaluate(cost, points, stride, N, pose7, max_dist, scale, out29, nullptr, 0, sp, nullptr, ws, s);
}

// `iters` iterations on pose7 whose info rows start at sp.row; the first one ignores and rewrites the flag
template <class Cost>
static void gn_iterate(const Cost &cost, const float *points, int stride, int N, double *pose7, int iters, double max_dist,
                       double scale, GnSolve sp, double *info, void *ws, hipStream_t s) {
  for (int it = 0; it < iters; ++it, ++sp.row)
    gn_evaluate(cost, points, stride, N, pose7, max_dist, scale, nullptr, pose7, it, sp, info, ws, s);
}

// ---------------------------------------------------------------------------------------------------------------------
// The argument rules the calls share; `name` is the call's, `bytes_fn` the backend's rslo_*_bytes.
// ---------------------------------------------------------------------------------------------------------------------
static int gn_check(const char *name, const char *bytes_fn, const void *map, long long cap_max, double voxel, int stride,
                    int N, const double *pose7, double max_dist) {
  RSLO_CHECK_ARG(map && cap_max > 0, "%s: no map (map_bytes below %s(1024))", name, bytes_fn);
  RSLO_CHECK_ARG(N >= 0 && stride >= 3, "%s: N < 0 or stride_floats < 3", name);
  RSLO_CHECK_ARG(pose7, "%s: pose7 is null", name);
  RSLO_CHECK_ARG(voxel > 0.0 && voxel < (double)__builtin_inff(), "%s: voxel_size must be positive and finite", name);
  RSLO_CHECK_ARG(max_dist > 0.0 && max_dist <= voxel, "%s: need 0 < max_dist <= voxel_size (NaN is refused)", name);
  return RSLO_OK;
}

// scale == 0: no weights; otherwise scale*scale must be a positive finite double (u = s2 / (s2 + e) is then defined
// for every e >= 0, e == 0 included)
static bool gn_scale_ok(double scale) {
  const double s2 = scale * scale;
  return scale == 0.0 || (scale > 0.0 && s2 > 0.0 && s2 < (double)__builtin_inff());
}
#define GN_SCALE_TEXT "robust_scale must be 0 (no weights) or positive with a finite, non-zero square"

static int gn_check_tol(const char *name, double tol_t, double tol_r) {
  RSLO_CHECK_ARG(tol_t >= 0.0 && tol_r >= 0.0, "%s: tol_t and tol_r must be >= 0 (NaN is refused)", name);
  return RSLO_OK;
}

static int gn_check_iters(const char *name, int iters, double tol_t, double tol_r) {
  RSLO_CHECK_ARG(iters >= 1 && iters <= GN_MAX_ITERS, "%s: iters must be in 1 .. 32", name);
  return gn_check_tol(name, tol_t, tol_r);
}

static size_t gn_ws_bytes(int N) {      // N <= 0: one block's partials
  const size_t nb = N > 0 ? (size_t)rslo_cdiv(N, GN_BLOCK) : 1;
  return GN_WS_HDR + (nb * GN_NSUM * sizeof(double) + 255) / 256 * 256;
}

static int gn_check_ws(const char *name, const float *points, int N, void *ws, size_t ws_bytes) {
  RSLO_CHECK_ARG(ws && ((uintptr_t)ws & 7) == 0 && (N == 0 || points),
                 "%s: null pointer, or a workspace that is not 8-byte aligned", name);
  if (ws_bytes < gn_ws_bytes(N)) {
    rslo_set_error("%s: workspace too small", name);
    return RSLO_EWS;
  }
  return RSLO_OK;
}
