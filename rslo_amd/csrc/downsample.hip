// Voxel down-sample of one cloud: the second offline step of the reference's script/create_hdf5.py:149-165, 337-347
//     pcd.voxel_down_sample(voxel_size)            (0.1 / 0.2 / 0.4 / 0.8 m, each from the full-resolution cloud)
//
// Open3D is not part of the reference tree and was not available when this was written: the rules below are RECALLED
// from its PointCloud::VoxelDownSample and could not be checked against it.  The arbiter of the tests is the float64
// restatement rslo_amd/downsample.py of exactly these rules.  All arithmetic is double (Open3D stores points as doubles).
//   1. a point is valid when its three coordinates are finite; an invalid point belongs to no voxel.
//   2. minb = component-wise minimum of the valid points; vmin = minb - 0.5 * voxel_size.
//   3. cell c = floor((double(p) - vmin) / voxel_size) per axis (a true IEEE division).
//   4. one output row per occupied cell: sum(p) / n and sum(normal) / n (NOT renormalised), the sums formed in double in
//      ASCENDING INPUT INDEX (the order in which Open3D's hash map accumulates), rounded to fp32 on store.
// Fixed by us, not by Open3D: rows are ordered by ascending (cx, cy, cz), cx most significant (Open3D's order is that
// of an unordered_map); a cell index >= 2^21 sets flag bit 0 and gives Q = 0, reported on the device.
//
// Structure.  (a) minimum: block reduction + atomicMin on an order-preserving integer image of the floats (min does not
// depend on order).  (b) one 64-bit key cx << 42 | cy << 21 | cz per point, value = point index; invalid points get the
// all-ones key.  (c) rocPRIM radix_sort_pairs over all 64 bits (the all-ones key must stay above the largest valid
// key, whose low 63 bits may all be set); the sort is stable, so a cell's points stay in ascending index.  (d) run heads
// are flagged and scanned (rocPRIM inclusive_scan): output row of every sorted slot, Q, and the start of every run.
// (e) the runs are reduced: a run of up to DS_WAVE points by one lane that walks it in order; a longer run by one wave,
// whose lanes gather 64 rows at a time into LDS (parallel) and whose lane c then adds component c in order
// (sequential: double adds cannot be re-associated without changing bits, so nothing is tree-reduced).  Which block
// takes which long run depends on the arrival order of an atomic counter; what a run sums to does not.
#include <string.h>

#include <rocprim/rocprim.hpp>

#include "rslo_common.h"

#pragma clang fp contract(off)   /* the cell index and the means must not depend on FMA formation */

#define DS_WAVE 64
#define DS_MAXC 2097152.0        /* 2^21: the first cell index a 21-bit key field cannot hold */
#define DS_LONG_BLOCKS 1024

typedef unsigned long long ds_u64;
#define DS_KEY_NONE (~(ds_u64)0)

struct DsState {
  uint32_t minkey[3];     // order-preserving image of the minimum; all-ones while no valid point was seen
  int32_t flags;          // bit 0: a cell index >= 2^21
  int32_t n_long;         // entries of the long-run list
};

// float -> unsigned with the same order (-0 sorts just below +0; both are 0.0 in the arithmetic that follows)
__device__ __forceinline__ uint32_t ds_encode(float v) {
  const uint32_t u = (uint32_t)__float_as_int(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float ds_decode(uint32_t k) {
  return __int_as_float((int)((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k));
}

__device__ __forceinline__ bool ds_finite3(float x, float y, float z) {
  const float inf = __builtin_inff();
  return fabsf(x) < inf && fabsf(y) < inf && fabsf(z) < inf;      // NaN compares false
}

__global__ void k_ds_init(DsState *__restrict__ st) {
  if (threadIdx.x < 3) st->minkey[threadIdx.x] = 0xFFFFFFFFu;
  if (threadIdx.x == 3) st->flags = 0;
  if (threadIdx.x == 4) st->n_long = 0;
}

__global__ __launch_bounds__(256) void k_ds_min(const float *__restrict__ points, int stride, int N,
                                                DsState *__restrict__ st) {
  __shared__ uint32_t red[4][3];
  uint32_t m0 = 0xFFFFFFFFu, m1 = 0xFFFFFFFFu, m2 = 0xFFFFFFFFu;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
    const float *p = points + (int64_t)i * stride;
    const float x = p[0], y = p[1], z = p[2];
    if (ds_finite3(x, y, z)) {
      m0 = min(m0, ds_encode(x));
      m1 = min(m1, ds_encode(y));
      m2 = min(m2, ds_encode(z));
    }
  }
  for (int d = 32; d > 0; d >>= 1) {
    m0 = min(m0, (uint32_t)__shfl_down((int)m0, d, 64));
    m1 = min(m1, (uint32_t)__shfl_down((int)m1, d, 64));
    m2 = min(m2, (uint32_t)__shfl_down((int)m2, d, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6][0] = m0;
    red[threadIdx.x >> 6][1] = m1;
    red[threadIdx.x >> 6][2] = m2;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const uint32_t m = min(min(red[0][threadIdx.x], red[1][threadIdx.x]), min(red[2][threadIdx.x], red[3][threadIdx.x]));
    if (m != 0xFFFFFFFFu) atomicMin(&st->minkey[threadIdx.x], m);
  }
}

// keys[i] = cx << 42 | cy << 21 | cz (all-ones: invalid, or a cell the key cannot hold), vals[i] = i
__global__ void k_ds_keys(const float *__restrict__ points, int stride, int N, double voxel, DsState *__restrict__ st,
                          ds_u64 *__restrict__ keys, int32_t *__restrict__ vals) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const float *p = points + (int64_t)i * stride;
  const float x = p[0], y = p[1], z = p[2];
  ds_u64 key = DS_KEY_NONE;
  if (ds_finite3(x, y, z)) {       // then some point is valid and the three minima are set
    const double hx = (double)ds_decode(st->minkey[0]) - 0.5 * voxel;
    const double hy = (double)ds_decode(st->minkey[1]) - 0.5 * voxel;
    const double hz = (double)ds_decode(st->minkey[2]) - 0.5 * voxel;
    const double cx = floor(((double)x - hx) / voxel), cy = floor(((double)y - hy) / voxel),
                 cz = floor(((double)z - hz) / voxel);
    if (cx < DS_MAXC && cy < DS_MAXC && cz < DS_MAXC)      // >= 0 by construction: vmin <= minb <= p
      key = ((ds_u64)cx << 42) | ((ds_u64)cy << 21) | (ds_u64)cz;
    else
      atomicOr(&st->flags, 1);
  }
  keys[i] = key;
  vals[i] = i;
}

__global__ void k_ds_heads(const ds_u64 *__restrict__ skeys, int N, int32_t *__restrict__ head) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= N) return;
  const ds_u64 k = skeys[j];
  head[j] = (k != DS_KEY_NONE && (j == 0 || skeys[j - 1] != k)) ? 1 : 0;
}

// row[j] = inclusive scan of the heads.  start[r] = first sorted slot of output row r, start[Q] = number of valid points;
// voxel_of_point; counts.  On overflow only counts is written.
__global__ void k_ds_rows(const ds_u64 *__restrict__ skeys, const int32_t *__restrict__ sidx,
                          const int32_t *__restrict__ row, int N, const DsState *__restrict__ st,
                          int32_t *__restrict__ start, int32_t *__restrict__ voxel_of_point,
                          int32_t *__restrict__ counts) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= N) return;
  const int flags = st->flags;
  if (j == N - 1) {
    counts[0] = flags ? 0 : row[N - 1];
    counts[1] = flags;
  }
  if (flags) return;
  const bool valid = skeys[j] != DS_KEY_NONE;
  const int r = row[j] - 1;
  if (valid && (j == 0 || row[j - 1] != row[j])) start[r] = j;
  if (!valid && (j == 0 || skeys[j - 1] != DS_KEY_NONE)) start[row[N - 1]] = j;      // the first invalid slot
  if (valid && j == N - 1) start[row[N - 1]] = N;
  if (voxel_of_point) voxel_of_point[sidx[j]] = valid ? r : -1;
}

// one lane per output row; a run longer than a wave goes on the list of k_ds_reduce_long
template <bool NRM>
__global__ __launch_bounds__(256) void k_ds_reduce(const float *__restrict__ points, int stride,
                                                   const float *__restrict__ normals, int nstride,
                                                   const int32_t *__restrict__ sidx, const int32_t *__restrict__ row,
                                                   const int32_t *__restrict__ start, int N, DsState *__restrict__ st,
                                                   float *__restrict__ out, int32_t *__restrict__ npts,
                                                   int32_t *__restrict__ long_list) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (st->flags || r >= row[N - 1]) return;
  const int b = start[r], e = start[r + 1], n = e - b;
  if (npts) npts[r] = n;
  if (n > DS_WAVE) {
    long_list[atomicAdd(&st->n_long, 1)] = r;
    return;
  }
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0, s5 = 0.0;
#pragma unroll 4
  for (int j = b; j < e; ++j) {
    const int i = sidx[j];
    const float *p = points + (int64_t)i * stride;
    s0 += (double)p[0];
    s1 += (double)p[1];
    s2 += (double)p[2];
    if (NRM) {
      const float *q = normals + (int64_t)i * nstride;
      s3 += (double)q[0];
      s4 += (double)q[1];
      s5 += (double)q[2];
    }
  }
  const double dn = (double)n;
  float *o = out + (int64_t)r * (NRM ? 6 : 3);
  o[0] = (float)(s0 / dn);
  o[1] = (float)(s1 / dn);
  o[2] = (float)(s2 / dn);
  if (NRM) {
    o[3] = (float)(s3 / dn);
    o[4] = (float)(s4 / dn);
    o[5] = (float)(s5 / dn);
  }
}

// one wave per long run: 64 rows gathered at a time, lane c < C adds component c in slot order
template <bool NRM>
__global__ __launch_bounds__(DS_WAVE) void k_ds_reduce_long(const float *__restrict__ points, int stride,
                                                            const float *__restrict__ normals, int nstride,
                                                            const int32_t *__restrict__ sidx,
                                                            const int32_t *__restrict__ start,
                                                            const DsState *__restrict__ st,
                                                            const int32_t *__restrict__ long_list,
                                                            float *__restrict__ out) {
  constexpr int C = NRM ? 6 : 3;
  __shared__ float slot[DS_WAVE][C];
  const int lane = threadIdx.x;
  const int n_long = st->n_long;
  for (int k = blockIdx.x; k < n_long; k += gridDim.x) {
    const int r = long_list[k];
    const int b = start[r], e = start[r + 1];
    double s = 0.0;
    for (int t = b; t < e; t += DS_WAVE) {
      const int m = e - t < DS_WAVE ? e - t : DS_WAVE;
      if (lane < m) {
        const int i = sidx[t + lane];
        const float *p = points + (int64_t)i * stride;
        slot[lane][0] = p[0];
        slot[lane][1] = p[1];
        slot[lane][2] = p[2];
        if constexpr (NRM) {
          const float *q = normals + (int64_t)i * nstride;
          slot[lane][3] = q[0];
          slot[lane][4] = q[1];
          slot[lane][5] = q[2];
        }
      }
      __syncthreads();
      if (lane < C)
        for (int j = 0; j < m; ++j) s += (double)slot[j][lane];
      __syncthreads();
    }
    if (lane < C) out[(int64_t)r * C + lane] = (float)(s / (double)(e - b));
  }
}

static size_t ds_sort_tmp_bytes(int N) {
  size_t tmp = 0;
  (void)rocprim::radix_sort_pairs(nullptr, tmp, (ds_u64 *)nullptr, (ds_u64 *)nullptr, (int32_t *)nullptr,
                                  (int32_t *)nullptr, (size_t)N, 0u, 64u, (hipStream_t)0);
  return (tmp + 255) / 256 * 256;
}

static size_t ds_scan_tmp_bytes(int N) {
  size_t tmp = 0;
  (void)rocprim::inclusive_scan(nullptr, tmp, (int32_t *)nullptr, (int32_t *)nullptr, (size_t)N,
                                rocprim::plus<int32_t>(), (hipStream_t)0);
  return (tmp + 255) / 256 * 256;
}

// state | keys, sorted keys [N] u64 | index, sorted index, heads, rows [N] i32 | starts [N + 1] | long-run list [N / 64 + 1] |
// the sort's and the scan's own scratch
extern "C" size_t rslo_voxel_downsample_ws_bytes(int N) {
  if (N <= 0) return 256;
  const size_t n = (size_t)N;
  return 256 + 2 * n * 8 + 4 * n * 4 + (n + 1) * 4 + (n / DS_WAVE + 1) * 4 + ds_sort_tmp_bytes(N) + ds_scan_tmp_bytes(N) +
         12 * 256;      // + alignment of the sections
}

extern "C" int rslo_voxel_downsample(const float *points, int stride_floats, const float *normals, int nstride_floats,
                                     int N, double voxel_size, float *out, int32_t *voxel_of_point, int32_t *npts,
                                     int32_t *counts, void *ws, size_t ws_bytes, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  RSLO_CHECK_ARG(N >= 0, "voxel_downsample: N < 0");
  RSLO_CHECK_ARG(voxel_size > 0.0 && voxel_size < (double)__builtin_inff(),
                 "voxel_downsample: voxel_size must be positive and finite");
  RSLO_CHECK_ARG(stride_floats >= 3, "voxel_downsample: stride_floats must be >= 3");
  RSLO_CHECK_ARG(!normals || nstride_floats >= 3, "voxel_downsample: nstride_floats must be >= 3");
  RSLO_CHECK_ARG(counts, "voxel_downsample: counts is null");
  if (N == 0) {
    RSLO_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(int32_t), s));
    return RSLO_OK;
  }
  RSLO_CHECK_ARG(points && out && ws, "voxel_downsample: null pointer");
  if (ws_bytes < rslo_voxel_downsample_ws_bytes(N)) {
    rslo_set_error("voxel_downsample: workspace too small");
    return RSLO_EWS;
  }
  unsigned char *w = (unsigned char *)(((uintptr_t)ws + 255) & ~(uintptr_t)255);      // every section on a 256-byte boundary
  auto take = [&](size_t bytes) { unsigned char *p = w; w += (bytes + 255) / 256 * 256; return p; };
  const size_t n = (size_t)N;
  DsState *st = (DsState *)take(256);
  ds_u64 *keys = (ds_u64 *)take(n * 8);
  ds_u64 *skeys = (ds_u64 *)take(n * 8);
  int32_t *vals = (int32_t *)take(n * 4);
  int32_t *sidx = (int32_t *)take(n * 4);
  int32_t *head = (int32_t *)take(n * 4);
  int32_t *row = (int32_t *)take(n * 4);
  int32_t *start = (int32_t *)take((n + 1) * 4);
  int32_t *long_list = (int32_t *)take((n / DS_WAVE + 1) * 4);
  size_t sort_tmp = ds_sort_tmp_bytes(N), scan_tmp = ds_scan_tmp_bytes(N);
  void *sort_ws = take(sort_tmp);
  void *scan_ws = take(scan_tmp);
  const unsigned nb = (unsigned)rslo_cdiv(N, 256);

  hipLaunchKernelGGL(k_ds_init, dim3(1), dim3(64), 0, s, st);
  hipLaunchKernelGGL(k_ds_min, dim3(nb < 1024u ? nb : 1024u), dim3(256), 0, s, points, stride_floats, N, st);
  hipLaunchKernelGGL(k_ds_keys, dim3(nb), dim3(256), 0, s, points, stride_floats, N, voxel_size, st, keys, vals);
  RSLO_CHECK_LAUNCH("voxel_downsample(keys)");
  RSLO_HIP(rocprim::radix_sort_pairs(sort_ws, sort_tmp, keys, skeys, vals, sidx, n, 0u, 64u, s));
  hipLaunchKernelGGL(k_ds_heads, dim3(nb), dim3(256), 0, s, (const ds_u64 *)skeys, N, head);
  RSLO_CHECK_LAUNCH("voxel_downsample(heads)");
  RSLO_HIP(rocprim::inclusive_scan(scan_ws, scan_tmp, head, row, n, rocprim::plus<int32_t>(), s));
  hipLaunchKernelGGL(k_ds_rows, dim3(nb), dim3(256), 0, s, (const ds_u64 *)skeys, (const int32_t *)sidx,
                     (const int32_t *)row, N, (const DsState *)st, start, voxel_of_point, counts);
  if (normals) {
    hipLaunchKernelGGL(k_ds_reduce<true>, dim3(nb), dim3(256), 0, s, points, stride_floats, normals, nstride_floats,
                       (const int32_t *)sidx, (const int32_t *)row, (const int32_t *)start, N, st, out, npts, long_list);
    hipLaunchKernelGGL(k_ds_reduce_long<true>, dim3(DS_LONG_BLOCKS), dim3(DS_WAVE), 0, s, points, stride_floats, normals,
                       nstride_floats, (const int32_t *)sidx, (const int32_t *)start, (const DsState *)st,
                       (const int32_t *)long_list, out);
  } else {
    hipLaunchKernelGGL(k_ds_reduce<false>, dim3(nb), dim3(256), 0, s, points, stride_floats, normals, nstride_floats,
                       (const int32_t *)sidx, (const int32_t *)row, (const int32_t *)start, N, st, out, npts, long_list);
    hipLaunchKernelGGL(k_ds_reduce_long<false>, dim3(DS_LONG_BLOCKS), dim3(DS_WAVE), 0, s, points, stride_floats, normals,
                       nstride_floats, (const int32_t *)sidx, (const int32_t *)start, (const DsState *)st,
                       (const int32_t *)long_list, out);
  }
  RSLO_CHECK_LAUNCH("voxel_downsample(reduce)");
  return RSLO_OK;
}
