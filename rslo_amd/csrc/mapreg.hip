// Scan-to-map registration against the world voxel map (rules: include/rslo_hip.h "Scan-to-map registration"; float64
// restatement: rslo_amd/mapping.py VoxelMapRef.nearest / normal_equations / register): the exact nearest stored point of
// every scan point among the 27 cells around it, the 6 x 6 normal equations of a point-to-point / point-to-plane
// cost over the matched pairs, and Gauss-Newton iterations that stay on the device.  Everything here only READS the map.
//
// Nearest: one thread per point.  The 27 probe chains of a point are independent 8-byte gathers into a table far larger
// than L2, so the first-slot keys of all 27 are loaded before any of them is examined (27 loads in flight per lane); a
// chain goes on alone only when its first slot held another cell's key.  Rows, hits and tags are read for matching
// cells only, a tag only to break a tie on d2.
//
// Sums: 28 doubles and the pair count per point, reduced in a fixed order -- a shuffle tree inside each wave, the four
// waves of a block in wave order, the blocks in block order by the second stage (one wave; lane j owns sum j).  No
// floating-point atomic anywhere: two runs give the same bits.  The addends, the two levels inside a block and the step
// that lane 0 of the second stage takes are gauss_newton.h's, shared with loop verification.
//
// Robust weights (rslo_map_normal_eq_w / _register_w / _register_sched): the accumulate kernel is one template; its
// WEIGHTED instantiation scales the 28 addends of a matched point by the Geman-McClure weight of its cost addend, the
// other one is the unweighted kernel as it always was.  A schedule is a host loop over (map, iterations, max_dist,
// scale) stages on one pose: the launches are those of separate register calls, the info rows run on.
#include "rslo_common.h"
#include "map_table.h"

#include <math.h>
#include <string.h>

#pragma clang fp contract(off)   /* the sums are specified operation by operation */

#include "gauss_newton.h"        /* after the pragma and after map_table.h's se3.h: the addends, the reduction, the step */

#define MR_BLOCK 256
#define MR_WS_HDR 256                    /* int32 word 0: the "converged" flag of rslo_map_register */
#define MR_MAX_ITERS 32
#define MR_MAX_SCHED_ITERS 64              /* sum of the iterations of a schedule */
#define MR_MAX_LEVELS 8

static long long mr_cap_max(size_t bytes) {      // the largest capacity the allocation can hold (0: none)
  long long cap = 0;
  for (long long c = MAP_MIN_CAP; c <= ((long long)1 << 31) && rslo_map_bytes(c) <= bytes; c *= 2) cap = c;
  return cap;
}

// The stored point nearest to w among the cells key + {-1,0,1}^3: slot and d2 of the winner (smallest d2, then smallest
// tag), its position in mm.  False when no candidate cell is stored with hits >= min_hits.
__device__ __forceinline__ bool mr_nearest(const MapView &m, map_u64 key, const double *w, int min_hits, uint32_t &bslot,
                                           double &bd2, double *mm) {
  const uint32_t mask = (uint32_t)((map_u64)m.hdr->capacity - 1);      // capacity <= 2^31
  const int c[3] = {(int)(key >> 42) & 0x1fffff, (int)(key >> 21) & 0x1fffff, (int)key & 0x1fffff};
  map_u64 k0[27];
  uint32_t s0[27];
#pragma unroll
  for (int j = 0; j < 27; ++j) {
    const int x = c[0] + j / 9 - 1, y = c[1] + (j / 3) % 3 - 1, z = c[2] + j % 3 - 1;
    const map_u64 nk = ((map_u64)(uint32_t)x << 42) | ((map_u64)(uint32_t)y << 21) | (map_u64)(uint32_t)z;
    s0[j] = (uint32_t)map_mix(nk) & mask;      // (a neighbour outside the key space is not examined below; its slot is in range)
    k0[j] = m.keys[s0[j]];
  }
  bool found = false;
#pragma unroll
  for (int j = 0; j < 27; ++j) {
    const int x = c[0] + j / 9 - 1, y = c[1] + (j / 3) % 3 - 1, z = c[2] + j % 3 - 1;
    if (x < 1 || x > 0x1fffff || y < 1 || y > 0x1fffff || z < 1 || z > 0x1fffff) continue;      // |cell| >= 2^20
    const map_u64 nk = ((map_u64)(uint32_t)x << 42) | ((map_u64)(uint32_t)y << 21) | (map_u64)(uint32_t)z;
    map_u64 k = k0[j];
    uint32_t s = s0[j];
    for (int probe = 1; k != nk && k != MAP_KEY_NONE && probe < RSLO_MAP_MAX_PROBE; ++probe) {
      s = (s + 1) & mask;
      k = m.keys[s];
    }
    if (k != nk) continue;
    if (min_hits > 1 && m.hits[s] < min_hits) continue;      // a stored cell has hits >= 1
    const float4 r = *(const float4 *)(m.rows + (size_t)s * 4);
    const double p[3] = {(double)r.x, (double)r.y, (double)r.z};
    const double dx = w[0] - p[0], dy = w[1] - p[1], dz = w[2] - p[2];
    const double d2 = dx * dx + dy * dy + dz * dz;
    if (!found || d2 < bd2 || (d2 == bd2 && m.tags[s] < m.tags[bslot])) {
      found = true;
      bslot = s;
      bd2 = d2;
      mm[0] = p[0];
      mm[1] = p[1];
      mm[2] = p[2];
    }
  }
  return found;
}

// the map as the registration calls accept it: reset, and with the cell edge the caller was checked against
__device__ __forceinline__ bool mr_view(const void *map, long long cap_max, double voxel, MapView &m) {
  return map_view((void *)map, cap_max, m) && m.hdr->voxel == voxel;
}

__global__ __launch_bounds__(MR_BLOCK) void k_map_nearest(const void *map, long long cap_max, double voxel,
                                                          const float *__restrict__ points, int stride, int N,
                                                          const double *__restrict__ pose, double max_dist, int min_hits,
                                                          long long *__restrict__ tags_out, double *__restrict__ d2_out,
                                                          float *__restrict__ rows_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  MapView m;
  long long tag = -1;
  double d2 = -1.0;
  float4 row = make_float4(0.f, 0.f, 0.f, 0.f);
  map_u64 key;
  double w[3], mm[3], bd2;
  uint32_t s;
  if (mr_view(map, cap_max, voxel, m) &&
      !map_point(points + (int64_t)i * stride, pose, m.hdr->voxel, m.hdr->min_range, m.hdr->max_range, key, w) &&
      mr_nearest(m, key, w, min_hits, s, bd2, mm) && bd2 < max_dist * max_dist) {
    tag = (long long)m.tags[s];
    d2 = bd2;
    row = *(const float4 *)(m.rows + (size_t)s * 4);
  }
  tags_out[i] = tag;
  d2_out[i] = d2;
  if (rows_out) *(float4 *)(rows_out + (size_t)i * 4) = row;
}

// block partial [GN_NSUM] of the addends of points blockIdx.x * 256 .. + 255 at the pose in pose7.  WEIGHTED: the 28
// addends of a matched point are multiplied by rho = u*u, u = s2 / (s2 + e), e its cost addend (s2 = scale*scale > 0).
template <bool WEIGHTED>
__global__ __launch_bounds__(MR_BLOCK) void k_mapreg_accum(const void *map, long long cap_max, double voxel,
                                                           const float *__restrict__ points, int stride, int width, int N,
                                                           const double *__restrict__ pose, int metric, double max_dist,
                                                           int min_hits, int iter, const int32_t *__restrict__ flag,
                                                           double *__restrict__ partials, double s2) {
  if (iter > 0 && *flag) return;      // converged in an earlier iteration: the second stage does not read the partials
  __shared__ double part[MR_BLOCK / 64 * GN_NSUM];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double acc[GN_NSUM];
#pragma unroll
  for (int k = 0; k < GN_NSUM; ++k) acc[k] = 0.0;
  MapView m;
  map_u64 key;
  double w[3], mm[3], bd2;
  uint32_t s;
  if (i < N && mr_view(map, cap_max, voxel, m)) {
    const float *p = points + (int64_t)i * stride;
    if (!map_point(p, pose, m.hdr->voxel, m.hdr->min_range, m.hdr->max_range, key, w) &&
        mr_nearest(m, key, w, min_hits, s, bd2, mm) && bd2 < max_dist * max_dist) {
      const double d[3] = {w[0] - mm[0], w[1] - mm[1], w[2] - mm[2]};
      // one plane term, or the three rows of a point term; the addends are assigned, not added to the zeros
      bool plane = false;
      if (metric == 1) {
        const double ns[3] = {(double)p[4], (double)p[5], (double)p[6]};
        if (ns[0] * ns[0] + ns[1] * ns[1] + ns[2] * ns[2] >= 0.25) {      // false for a NaN normal as well
          double n[3], wn[3];
          se3_rotate(pose + 3, ns, n);
          se3_cross(w, n, wn);
          gn_plane_terms(n, wn, n[0] * d[0] + n[1] * d[1] + n[2] * d[2], acc);
          plane = true;
        }
      }
      if (!plane) gn_point_terms(w, d, acc, false);
      acc[GN_NSUM - 1] = 1.0;
      if (WEIGHTED) {      // e = acc[27] >= 0 (or NaN, which stays NaN as it would unweighted); s2 > 0: u is in [0, 1]
        const double u = s2 / (s2 + acc[GN_NSUM - 2]);
        const double rho = u * u;
#pragma unroll
        for (int k = 0; k < GN_NSUM - 1; ++k) acc[k] = rho * acc[k];
      }
    }
  }
  gn_block_reduce(acc, part, MR_BLOCK / 64, partials + (size_t)blockIdx.x * GN_NSUM);
}

struct MrSolve {
  int iters, min_pairs;
  double damping, tol_t, tol_r;
  int row;                 // the info row of this iteration (`iter` counts inside a stage, the rows run on)
  double stage, level;     // info columns 5 and 6 (0 outside a schedule)
};

// Second stage, one wave: lane j sums partial j of the blocks in block order.  out29 (rslo_map_normal_eq) receives the
// sums; with pose7 (rslo_map_register) lane 0 then takes the Gauss-Newton step of iteration `iter` and writes its info row.
// Iteration 0 (of a call, or of a stage of a schedule) does not read the flag and rewrites it: that clears it.
__global__ __launch_bounds__(64) void k_mapreg_finish(const double *__restrict__ partials, int n_blocks,
                                                      double *__restrict__ out29, double *__restrict__ pose7, int iter,
                                                      MrSolve sp, int32_t *__restrict__ flag, double *__restrict__ info) {
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

extern "C" int rslo_map_params(const void *map, size_t map_bytes, double *params3_host, void *stream) {
  RSLO_CHECK_ARG(map && mr_cap_max(map_bytes) > 0, "map_params: no map (map_bytes below rslo_map_bytes(1024))");
  RSLO_CHECK_ARG(params3_host, "map_params: params3_host is null");
  long long words[5];
  RSLO_HIP(hipMemcpyAsync(words, map, sizeof(words), hipMemcpyDeviceToHost, (hipStream_t)stream));
  RSLO_HIP(hipStreamSynchronize((hipStream_t)stream));
  RSLO_CHECK_ARG((map_u64)words[0] == MAP_MAGIC, "map_params: the allocation holds no map (never reset)");
  for (int a = 0; a < 3; ++a) memcpy(&params3_host[a], &words[2 + a], sizeof(double));
  return RSLO_OK;
}

static int mr_check(const char *name, const void *map, long long cap_max, double voxel, int stride, int N,
                    const double *pose7, double max_dist) {
  char msg[160];
#define MR_ARG(cond, text)                         \
  do {                                             \
    if (!(cond)) {                                 \
      snprintf(msg, sizeof(msg), "%s: " text, name); \
      rslo_set_error("%s", msg);                   \
      return RSLO_EINVAL;                          \
    }                                              \
  } while (0)
  MR_ARG(map && cap_max > 0, "no map (map_bytes below rslo_map_bytes(1024))");
  MR_ARG(N >= 0 && stride >= 3, "N < 0 or stride_floats < 3");
  MR_ARG(pose7, "pose7 is null");
  MR_ARG(voxel > 0.0 && voxel < (double)__builtin_inff(), "voxel_size must be positive and finite");
  MR_ARG(max_dist > 0.0 && max_dist <= voxel, "need 0 < max_dist <= voxel_size (NaN is refused)");
#undef MR_ARG
  return RSLO_OK;
}

extern "C" int rslo_map_nearest(const void *map, size_t map_bytes, double voxel_size, const float *points,
                                int stride_floats, int N, const double *pose7, double max_dist, int min_hits,
                                int64_t *tags_out, double *d2_out, float *rows_out, void *stream) {
  const long long cap_max = mr_cap_max(map_bytes);
  const int rc = mr_check("map_nearest", map, cap_max, voxel_size, stride_floats, N, pose7, max_dist);
  if (rc) return rc;
  if (N == 0) return RSLO_OK;
  RSLO_CHECK_ARG(points && tags_out && d2_out, "map_nearest: null pointer");
  hipLaunchKernelGGL(k_map_nearest, dim3((unsigned)rslo_cdiv(N, MR_BLOCK)), dim3(MR_BLOCK), 0, (hipStream_t)stream, map,
                     cap_max, voxel_size, points, stride_floats, N, pose7, max_dist, min_hits, (long long *)tags_out,
                     d2_out, rows_out);
  RSLO_CHECK_LAUNCH("map_nearest");
  return RSLO_OK;
}

extern "C" size_t rslo_map_register_ws_bytes(int N) {
  const size_t nb = N > 0 ? (size_t)rslo_cdiv(N, MR_BLOCK) : 1;
  return MR_WS_HDR + (nb * GN_NSUM * sizeof(double) + 255) / 256 * 256;
}

// the launches of one evaluation of the normal equations (+ the step of iteration `iter` when pose_rw is given)
static int mr_launch(const void *map, long long cap_max, double voxel, const float *points, int stride, int width, int N,
                     const double *pose, int metric, double max_dist, int min_hits, double *out29, double *pose_rw,
                     int iter, const MrSolve &sp, double *info, void *ws, hipStream_t s, double scale = 0.0) {
  int32_t *flag = (int32_t *)ws;
  double *partials = (double *)((unsigned char *)ws + MR_WS_HDR);
  const int nb = (int)rslo_cdiv(N, MR_BLOCK);
  if (nb > 0 && scale == 0.0)      // no weights: the unweighted kernel, to the bit
    hipLaunchKernelGGL(k_mapreg_accum<false>, dim3((unsigned)nb), dim3(MR_BLOCK), 0, s, map, cap_max, voxel, points, stride,
                       width, N, pose, metric, max_dist, min_hits, iter, (const int32_t *)flag, partials, 0.0);
  else if (nb > 0)
    hipLaunchKernelGGL(k_mapreg_accum<true>, dim3((unsigned)nb), dim3(MR_BLOCK), 0, s, map, cap_max, voxel, points, stride,
                       width, N, pose, metric, max_dist, min_hits, iter, (const int32_t *)flag, partials, scale * scale);
  hipLaunchKernelGGL(k_mapreg_finish, dim3(1), dim3(64), 0, s, (const double *)partials, nb, out29, pose_rw, iter, sp, flag,
                     info);
  return RSLO_OK;
}

static int mr_check_sums(const char *name, const float *points, int stride, int width, int N, int metric, void *ws,
                         size_t ws_bytes) {
  if (!(metric == 0 || metric == 1) || width < 3 || (metric == 1 && (width < 7 || stride < 7))) {
    rslo_set_error("%s: metric must be 0 (point) or 1 (plane); the plane metric reads normals at columns 4..6 "
                   "(width and stride_floats >= 7)", name);
    return RSLO_EINVAL;
  }
  if (!ws || ((uintptr_t)ws & 7) || (N > 0 && !points)) {
    rslo_set_error("%s: null pointer, or a workspace that is not 8-byte aligned", name);
    return RSLO_EINVAL;
  }
  if (ws_bytes < rslo_map_register_ws_bytes(N)) {
    rslo_set_error("%s: workspace too small", name);
    return RSLO_EWS;
  }
  return RSLO_OK;
}

// scale == 0: no weights; otherwise scale*scale must be a positive finite double (u = s2 / (s2 + e) is then defined
// for every e >= 0, e == 0 included)
static bool mr_scale_ok(double scale) {
  const double s2 = scale * scale;
  return scale == 0.0 || (scale > 0.0 && s2 > 0.0 && s2 < (double)__builtin_inff());
}

static int mr_normal_eq(const char *name, const void *map, size_t map_bytes, double voxel_size, const float *points,
                        int stride_floats, int width, int N, const double *pose7, int metric, double max_dist,
                        int min_hits, double scale, double *out29, void *ws, size_t ws_bytes, void *stream) {
  const long long cap_max = mr_cap_max(map_bytes);
  int rc = mr_check(name, map, cap_max, voxel_size, stride_floats, N, pose7, max_dist);
  if (rc) return rc;
  RSLO_CHECK_ARG(out29, "%s: out29 is null", name);
  RSLO_CHECK_ARG(mr_scale_ok(scale), "%s: robust_scale must be 0 (no weights) or positive with a finite, non-zero square", name);
  rc = mr_check_sums(name, points, stride_floats, width, N, metric, ws, ws_bytes);
  if (rc) return rc;
  const MrSolve sp = {0, 0, 0.0, 0.0, 0.0, 0, 0.0, 0.0};
  mr_launch(map, cap_max, voxel_size, points, stride_floats, width, N, pose7, metric, max_dist, min_hits, out29, nullptr, 0,
            sp, nullptr, ws, (hipStream_t)stream, scale);
  RSLO_CHECK_LAUNCH(name);
  return RSLO_OK;
}

extern "C" int rslo_map_normal_eq(const void *map, size_t map_bytes, double voxel_size, const float *points,
                                  int stride_floats, int width, int N, const double *pose7, int metric, double max_dist,
                                  int min_hits, double *out29, void *ws, size_t ws_bytes, void *stream) {
  return mr_normal_eq("map_normal_eq", map, map_bytes, voxel_size, points, stride_floats, width, N, pose7, metric, max_dist,
                      min_hits, 0.0, out29, ws, ws_bytes, stream);
}

extern "C" int rslo_map_normal_eq_w(const void *map, size_t map_bytes, double voxel_size, const float *points,
                                    int stride_floats, int width, int N, const double *pose7, int metric,
                                    double max_dist, int min_hits, double robust_scale, double *out29, void *ws,
                                    size_t ws_bytes, void *stream) {
  return mr_normal_eq("map_normal_eq_w", map, map_bytes, voxel_size, points, stride_floats, width, N, pose7, metric,
                      max_dist, min_hits, robust_scale, out29, ws, ws_bytes, stream);
}

static int mr_register(const char *name, const void *map, size_t map_bytes, double voxel_size, const float *points,
                       int stride_floats, int width, int N, double *pose7, int iters, int metric, double max_dist,
                       int min_hits, double damping, int min_pairs, double tol_t, double tol_r, double scale, double *info,
                       void *ws, size_t ws_bytes, void *stream) {
  const long long cap_max = mr_cap_max(map_bytes);
  int rc = mr_check(name, map, cap_max, voxel_size, stride_floats, N, pose7, max_dist);
  if (rc) return rc;
  RSLO_CHECK_ARG(iters >= 1 && iters <= MR_MAX_ITERS, "%s: iters must be in 1 .. 32", name);
  RSLO_CHECK_ARG(tol_t >= 0.0 && tol_r >= 0.0, "%s: tol_t and tol_r must be >= 0 (NaN is refused)", name);
  RSLO_CHECK_ARG(mr_scale_ok(scale), "%s: robust_scale must be 0 (no weights) or positive with a finite, non-zero square", name);
  RSLO_CHECK_ARG(info, "%s: info is null", name);
  rc = mr_check_sums(name, points, stride_floats, width, N, metric, ws, ws_bytes);
  if (rc) return rc;
  MrSolve sp = {iters, min_pairs, damping, tol_t, tol_r, 0, 0.0, 0.0};
  for (int it = 0; it < iters; ++it) {
    sp.row = it;
    mr_launch(map, cap_max, voxel_size, points, stride_floats, width, N, pose7, metric, max_dist, min_hits, nullptr, pose7,
              it, sp, info, ws, (hipStream_t)stream, scale);
  }
  RSLO_CHECK_LAUNCH(name);
  return RSLO_OK;
}

extern "C" int rslo_map_register(const void *map, size_t map_bytes, double voxel_size, const float *points,
                                 int stride_floats, int width, int N, double *pose7, int iters, int metric,
                                 double max_dist, int min_hits, double damping, int min_pairs, double tol_t, double tol_r,
                                 double *info, void *ws, size_t ws_bytes, void *stream) {
  return mr_register("map_register", map, map_bytes, voxel_size, points, stride_floats, width, N, pose7, iters, metric,
                     max_dist, min_hits, damping, min_pairs, tol_t, tol_r, 0.0, info, ws, ws_bytes, stream);
}

extern "C" int rslo_map_register_w(const void *map, size_t map_bytes, double voxel_size, const float *points,
                                   int stride_floats, int width, int N, double *pose7, int iters, int metric,
                                   double max_dist, int min_hits, double damping, int min_pairs, double tol_t,
                                   double tol_r, double robust_scale, double *info, void *ws, size_t ws_bytes,
                                   void *stream) {
  return mr_register("map_register_w", map, map_bytes, voxel_size, points, stride_floats, width, N, pose7, iters, metric,
                     max_dist, min_hits, damping, min_pairs, tol_t, tol_r, robust_scale, info, ws, ws_bytes, stream);
}

// Every argument of every stage is checked before the first launch; then the stages are the launches of
// rslo_map_register_w calls on maps[level], with the info rows running on and columns 5 / 6 naming stage and level.
extern "C" int rslo_map_register_sched(const void *const *maps, const size_t *map_bytes, const double *voxel_sizes,
                                       int n_levels, const double *stages, int n_stages, const float *points,
                                       int stride_floats, int width, int N, double *pose7, int metric, int min_hits,
                                       double damping, int min_pairs, double tol_t, double tol_r, double *info, void *ws,
                                       size_t ws_bytes, void *stream) {
  const char *name = "map_register_sched";
  RSLO_CHECK_ARG(n_levels >= 1 && n_levels <= MR_MAX_LEVELS, "%s: n_levels must be in 1 .. 8", name);
  RSLO_CHECK_ARG(maps && map_bytes && voxel_sizes && stages, "%s: null array", name);
  RSLO_CHECK_ARG(n_stages >= 1 && n_stages <= MR_MAX_SCHED_ITERS, "%s: n_stages must be in 1 .. 64", name);
  long long cap_max[MR_MAX_LEVELS];
  for (int l = 0; l < n_levels; ++l) {
    cap_max[l] = mr_cap_max(map_bytes[l]);
    RSLO_CHECK_ARG(maps[l] && cap_max[l] > 0, "%s: level %d has no map (null, or map_bytes below rslo_map_bytes(1024))", name, l);
    RSLO_CHECK_ARG(voxel_sizes[l] > 0.0 && voxel_sizes[l] < (double)__builtin_inff(),
                   "%s: voxel_sizes[%d] must be positive and finite", name, l);
  }
  int total = 0;
  for (int k = 0; k < n_stages; ++k) {
    const double *st = stages + (size_t)k * 4;
    RSLO_CHECK_ARG(st[0] >= 0.0 && st[0] < (double)n_levels && st[0] == (double)(int)st[0],
                   "%s: stage %d: level must be an integer in 0 .. n_levels - 1", name, k);
    RSLO_CHECK_ARG(st[1] >= 1.0 && st[1] <= (double)MR_MAX_SCHED_ITERS && st[1] == (double)(int)st[1],
                   "%s: stage %d: iters must be an integer >= 1 (all stages together: at most 64)", name, k);
    total += (int)st[1];
    RSLO_CHECK_ARG(total <= MR_MAX_SCHED_ITERS, "%s: the iterations of all stages must sum to 1 .. 64", name);
    RSLO_CHECK_ARG(st[2] > 0.0 && st[2] <= voxel_sizes[(int)st[0]],
                   "%s: stage %d: need 0 < max_dist <= the level's voxel_size (NaN is refused)", name, k);
    RSLO_CHECK_ARG(mr_scale_ok(st[3]),
                   "%s: stage %d: robust_scale must be 0 (no weights) or positive with a finite, non-zero square", name, k);
  }
  RSLO_CHECK_ARG(N >= 0 && stride_floats >= 3, "%s: N < 0 or stride_floats < 3", name);
  RSLO_CHECK_ARG(pose7, "%s: pose7 is null", name);
  RSLO_CHECK_ARG(tol_t >= 0.0 && tol_r >= 0.0, "%s: tol_t and tol_r must be >= 0 (NaN is refused)", name);
  RSLO_CHECK_ARG(info, "%s: info is null", name);
  const int rc = mr_check_sums(name, points, stride_floats, width, N, metric, ws, ws_bytes);
  if (rc) return rc;
  MrSolve sp = {0, min_pairs, damping, tol_t, tol_r, 0, 0.0, 0.0};
  int row = 0;
  for (int k = 0; k < n_stages; ++k) {
    const double *st = stages + (size_t)k * 4;
    const int level = (int)st[0], iters = (int)st[1];
    sp.iters = iters;
    sp.stage = (double)k;
    sp.level = (double)level;
    for (int it = 0; it < iters; ++it) {      // `it` restarts: the stage's first iteration ignores and rewrites the flag
      sp.row = row++;
      mr_launch(maps[level], cap_max[level], voxel_sizes[level], points, stride_floats, width, N, pose7, metric, st[2],
                min_hits, nullptr, pose7, it, sp, info, ws, (hipStream_t)stream, st[3]);
    }
  }
  RSLO_CHECK_LAUNCH(name);
  return RSLO_OK;
}
