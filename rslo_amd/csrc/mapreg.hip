// Scan-to-map registration against the world voxel map (rules: include/rslo_hip.h "Scan-to-map registration"; float64
// restatement: rslo_amd/mapping.py VoxelMapRef.nearest / normal_equations / register): the exact nearest stored point of
// every scan point among the 27 cells around it, the 6 x 6 normal equations of a point-to-point / point-to-plane
// cost over the matched pairs, and Gauss-Newton iterations that stay on the device.  Everything here only READS the map.
//
// Nearest: one thread per point; the 27-cell search is map_table.h's map_neighbours, the candidate test (hits) and the
// tie-break (tags) are mr_nearest's.
//
// Sums: 28 doubles and the pair count per point, reduced in a fixed order -- a shuffle tree inside each wave, the four
// waves of a block in wave order, the blocks in block order by the second stage (one wave; lane j owns sum j).  No
// floating-point atomic anywhere: two runs give the same bits.  The addends, the two levels inside a block and the step
// are gauss_newton.h's, shared with loop verification; the kernels, their launches, the iteration loop and the argument
// rules common to all registration calls are gn_register.h's, shared with surfel.hip.  This file holds what is the voxel
// map's own: the match, the cost (MrCost: a plane term with the scan's normal, or a point term), its argument checks.
//
// Robust weights (rslo_map_normal_eq_w / _register_w / _register_sched): a scale of 0 launches the unweighted
// instantiation of the accumulate kernel, as it always was.  A schedule is a host loop over (map, iterations, max_dist,
// scale) stages on one pose: the launches are those of separate register calls, the info rows run on.
#include "rslo_common.h"
#include "map_table.h"

#include <math.h>
#include <string.h>

#pragma clang fp contract(off)   /* the sums are specified operation by operation */

#include "gauss_newton.h"        /* after the pragma and after map_table.h's se3.h: the addends, the reduction, the step */
#include "gn_register.h"         /* the scaffold: workspace, accumulate and finish kernels, launches, shared argument rules */

#define MR_MAX_SCHED_ITERS 64              /* sum of the iterations of a schedule */
#define MR_MAX_LEVELS 8

// The stored point nearest to w among the cells key + {-1,0,1}^3: slot and d2 of the winner (smallest d2, then smallest
// tag), its position in mm.  False when no candidate cell is stored with hits >= min_hits.  Rows, hits and tags are read
// for stored cells only, a tag only to break a tie on d2.
__device__ __forceinline__ bool mr_nearest(const MapView &m, map_u64 key, const double *w, int min_hits, uint32_t &bslot,
                                           double &bd2, double *mm) {
  bool found = false;
  map_neighbours(m.keys, m.hdr->capacity, key, [&](uint32_t s, map_u64) {
    if (min_hits > 1 && m.hits[s] < min_hits) return;      // a stored cell has hits >= 1
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
  });
  return found;
}

// The match of scan point p under `pose` in the map as the registration calls accept it (reset, and with the cell edge
// the caller was checked against): world position w, slot s and position mm of the nearest stored point, closer than max_dist
__device__ __forceinline__ bool mr_match(const void *map, long long cap_max, double voxel, const float *p, const double *pose,
                                         double max_dist, int min_hits, MapView &m, double *w, uint32_t &s, double &bd2,
                                         double *mm) {
  map_u64 key;
  return map_view((void *)map, cap_max, m) && m.hdr->voxel == voxel &&
         !map_point(p, pose, m.hdr->voxel, m.hdr->min_range, m.hdr->max_range, key, w) &&
         mr_nearest(m, key, w, min_hits, s, bd2, mm) && bd2 < max_dist * max_dist;
}

__global__ __launch_bounds__(GN_BLOCK) void k_map_nearest(const void *map, long long cap_max, double voxel,
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
  double w[3], mm[3], bd2;
  uint32_t s;
  if (mr_match(map, cap_max, voxel, points + (int64_t)i * stride, pose, max_dist, min_hits, m, w, s, bd2, mm)) {
    tag = (long long)m.tags[s];
    d2 = bd2;
    row = *(const float4 *)(m.rows + (size_t)s * 4);
  }
  tags_out[i] = tag;
  d2_out[i] = d2;
  if (rows_out) *(float4 *)(rows_out + (size_t)i * 4) = row;
}

// The voxel map's cost: one plane term with the scan point's normal (metric 1, columns 4..6 of its row), or the three
// rows of a point term
struct MrCost {
  const void *map;
  long long cap_max;
  double voxel;
  int metric, min_hits;

  __device__ __forceinline__ bool terms(const float *p, const double *pose, double max_dist, double *acc) const {
    MapView m;
    double w[3], mm[3], bd2;
    uint32_t s;
    if (!mr_match(map, cap_max, voxel, p, pose, max_dist, min_hits, m, w, s, bd2, mm)) return false;
    const double d[3] = {w[0] - mm[0], w[1] - mm[1], w[2] - mm[2]};
    if (metric == 1) {
      const double ns[3] = {(double)p[4], (double)p[5], (double)p[6]};
      if (ns[0] * ns[0] + ns[1] * ns[1] + ns[2] * ns[2] >= 0.25) {      // false for a NaN normal as well
        double n[3], wn[3];
        se3_rotate(pose + 3, ns, n);
        se3_cross(w, n, wn);
        gn_plane_terms(n, wn, n[0] * d[0] + n[1] * d[1] + n[2] * d[2], acc);
        return true;
      }
    }
    gn_point_terms(w, d, acc, false);
    return true;
  }
};

extern "C" int rslo_map_params(const void *map, size_t map_bytes, double *params3_host, void *stream) {
  RSLO_CHECK_ARG(map && map_cap_of_bytes(map_bytes) > 0, "map_params: no map (map_bytes below rslo_map_bytes(1024))");
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
  return gn_check(name, "rslo_map_bytes", map, cap_max, voxel, stride, N, pose7, max_dist);
}

extern "C" int rslo_map_nearest(const void *map, size_t map_bytes, double voxel_size, const float *points,
                                int stride_floats, int N, const double *pose7, double max_dist, int min_hits,
                                int64_t *tags_out, double *d2_out, float *rows_out, void *stream) {
  const long long cap_max = map_cap_of_bytes(map_bytes);
  const int rc = mr_check("map_nearest", map, cap_max, voxel_size, stride_floats, N, pose7, max_dist);
  if (rc) return rc;
  if (N == 0) return RSLO_OK;
  RSLO_CHECK_ARG(points && tags_out && d2_out, "map_nearest: null pointer");
  hipLaunchKernelGGL(k_map_nearest, dim3((unsigned)rslo_cdiv(N, GN_BLOCK)), dim3(GN_BLOCK), 0, (hipStream_t)stream, map,
                     cap_max, voxel_size, points, stride_floats, N, pose7, max_dist, min_hits, (long long *)tags_out,
                     d2_out, rows_out);
  RSLO_CHECK_LAUNCH("map_nearest");
  return RSLO_OK;
}

extern "C" size_t rslo_map_register_ws_bytes(int N) { return gn_ws_bytes(N); }

// the metric and the columns it reads, then the workspace
static int mr_check_sums(const char *name, const float *points, int stride, int width, int N, int metric, void *ws,
                         size_t ws_bytes) {
  RSLO_CHECK_ARG((metric == 0 || metric == 1) && width >= 3 && !(metric == 1 && (width < 7 || stride < 7)),
                 "%s: metric must be 0 (point) or 1 (plane); the plane metric reads normals at columns 4..6 "
                 "(width and stride_floats >= 7)", name);
  return gn_check_ws(name, points, N, ws, ws_bytes);
}

static int mr_normal_eq(const char *name, const void *map, size_t map_bytes, double voxel_size, const float *points,
                        int stride_floats, int width, int N, const double *pose7, int metric, double max_dist,
                        int min_hits, double scale, double *out29, void *ws, size_t ws_bytes, void *stream) {
  const long long cap_max = map_cap_of_bytes(map_bytes);
  int rc = mr_check(name, map, cap_max, voxel_size, stride_floats, N, pose7, max_dist);
  if (rc) return rc;
  RSLO_CHECK_ARG(out29, "%s: out29 is null", name);
  RSLO_CHECK_ARG(gn_scale_ok(scale), "%s: " GN_SCALE_TEXT, name);
  rc = mr_check_sums(name, points, stride_floats, width, N, metric, ws, ws_bytes);
  if (rc) return rc;
  const MrCost cost = {map, cap_max, voxel_size, metric, min_hits};
  gn_normal_eq(cost, points, stride_floats, N, pose7, max_dist, scale, out29, ws, (hipStream_t)stream);
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
  const long long cap_max = map_cap_of_bytes(map_bytes);
  int rc = mr_check(name, map, cap_max, voxel_size, stride_floats, N, pose7, max_dist);
  if (rc) return rc;
  rc = gn_check_iters(name, iters, tol_t, tol_r);
  if (rc) return rc;
  RSLO_CHECK_ARG(gn_scale_ok(scale), "%s: " GN_SCALE_TEXT, name);
  RSLO_CHECK_ARG(info, "%s: info is null", name);
  rc = mr_check_sums(name, points, stride_floats, width, N, metric, ws, ws_bytes);
  if (rc) return rc;
  const MrCost cost = {map, cap_max, voxel_size, metric, min_hits};
  const GnSolve sp = {min_pairs, damping, tol_t, tol_r, 0, 0.0, 0.0};
  gn_iterate(cost, points, stride_floats, N, pose7, iters, max_dist, scale, sp, info, ws, (hipStream_t)stream);
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
    cap_max[l] = map_cap_of_bytes(map_bytes[l]);
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
    RSLO_CHECK_ARG(gn_scale_ok(st[3]), "%s: stage %d: " GN_SCALE_TEXT, name, k);
  }
  RSLO_CHECK_ARG(N >= 0 && stride_floats >= 3, "%s: N < 0 or stride_floats < 3", name);
  RSLO_CHECK_ARG(pose7, "%s: pose7 is null", name);
  int rc = gn_check_tol(name, tol_t, tol_r);
  if (rc) return rc;
  RSLO_CHECK_ARG(info, "%s: info is null", name);
  rc = mr_check_sums(name, points, stride_floats, width, N, metric, ws, ws_bytes);
  if (rc) return rc;
  GnSolve sp = {min_pairs, damping, tol_t, tol_r, 0, 0.0, 0.0};
  for (int k = 0; k < n_stages; ++k) {      // every stage restarts the iteration count: its first one ignores and rewrites the flag
    const double *st = stages + (size_t)k * 4;
    const int level = (int)st[0], iters = (int)st[1];
    const MrCost cost = {maps[level], cap_max[level], voxel_sizes[level], metric, min_hits};
    sp.stage = (double)k;
    sp.level = (double)level;
    gn_iterate(cost, points, stride_floats, N, pose7, iters, st[2], st[3], sp, info, ws, (hipStream_t)stream);
    sp.row += iters;
  }
  RSLO_CHECK_LAUNCH(name);
  return RSLO_OK;
}
