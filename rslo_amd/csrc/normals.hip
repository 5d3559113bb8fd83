// Point normals of one cloud: the offline step of the reference's script/create_hdf5.py:130-147
//     pcd.estimate_normals(KDTreeSearchParamHybrid(radius=0.6, max_nn=30))
//     pcd.orient_normals_towards_camera_location((0, 0, 0))
// plus, optionally, the rule its reader applies on load (rslo/data/kitti_dataset_hdf5.py:197-198).
//
// Open3D is not part of the reference tree and was not available when this was written: the rules below are RECALLED
// from its EstimateNormals / OrientNormalsTowardsCameraLocation / KDTreeFlann::SearchHybrid and could not be checked
// against it.  The arbiter of the tests is the float64 restatement rslo_amd/normals.py of exactly these rules.
//   1. S_i = points j of the cloud with |p_j - p_i|^2 < radius^2 (strict; i itself included); if more than max_nn
//      qualify, the max_nn with the smallest squared distance, ties to the lower original index.  count_i = |S_i|.
//   2. count_i >= 3: covariance of S_i (mean of outer products about the neighbourhood mean), accumulated from the
//      offsets p_j - p_i; n_i = unit eigenvector of the smallest eigenvalue.  count_i < 3, or an eigenvector of zero /
//      non-finite norm: n_i = (0, 0, 1).
//   3. v = viewpoint - p_i; n_i is flipped when n_i . v < 0.
//   4. zero_vertical: a component of n_i whose absolute value equals the same component of (0, 0, 1) becomes 0.
//   5. a point with a non-finite coordinate is nobody's neighbour and gets count 0 and a zero normal.
//
// Structure.  The cloud is bucketed by a uniform cell grid of edge >= radius (counting sort: histogram that also hands
// every point its rank inside its cell, scan, scatter; points outside the key range are clamped into border cells, a
// clamp is monotone and 1-Lipschitz so neighbours still sit in adjacent cells).  The key is x-fastest, so the three
// x-adjacent cells of a row are ONE contiguous range of the sorted array.  A wave owns 64 consecutive sorted queries;
// its lanes are grouped by grid row (cy, cz) and a window of NM_WIN cells along x (a sparse row may spread a wave over
// metres, with dense rows beside it), and for every group the nine neighbouring rows are streamed over the window
// +-1 cell through the wave's LDS slot in tiles of 64 candidates (broadcast reads), every candidate
// exactly once.  Each lane keeps its 32 best (d^2 bits << 32 | original index) keys as a sorted register list: a
// candidate is merged by a min/max chain, and only when some lane of the wave has a candidate inside the radius that
// beats its current worst.  The key order IS the tie rule, so the selected set does not depend on the order in which
// candidates arrive: the sort affects speed only, never the answer.  The sums of the selected set are then formed in
// key order (gathered from the caller's array), which makes the result independent of the atomics' arrival order:
// two calls give identical bits.  The 3x3 eigenproblem is solved per lane by cyclic Jacobi sweeps on the
// trace-scaled covariance.
#include "rslo_common.h"

#pragma clang fp contract(off)   /* the neighbour set must not depend on FMA formation */

#define NM_NX 256
#define NM_NY 256
#define NM_NZ 8
#define NM_BINS (NM_NX * NM_NY * NM_NZ)
#define NM_ORG_XY 80.0f       /* 256 cells of >= 0.625 m from -80 m */
#define NM_ORG_Z 10.0f        /* 8 cells of >= 2.5 m from -10 m */
#define NM_MIN_CELL_XY 0.625f
#define NM_MIN_CELL_Z 2.5f
#define NM_CHUNK 1024
#define NM_NCHUNK (NM_BINS / NM_CHUNK)
#define NM_K 32               /* list length = the largest max_nn */
#define NM_TILE 64
#define NM_WIN 2              /* cells along x that one group of a wave's lanes may span */

typedef unsigned long long nm_u64;
#define NM_KEY_NONE (~(nm_u64)0)

__device__ __forceinline__ int nm_cell1(float v, float org, float inv, int n) {
  // NaN -> 0 (fmaxf drops it), +-inf and anything outside the range -> a border cell: the key is only a sort hint
  return (int)fminf(fmaxf(floorf((v + org) * inv), 0.0f), (float)(n - 1));
}

__device__ __forceinline__ int nm_key(int cx, int cy, int cz) { return (cz * NM_NY + cy) * NM_NX + cx; }

// hist[key] += 1; the value the atomic returns is the point's rank inside its cell
__global__ void k_nm_hist(const float *__restrict__ points, int stride, int N, float inv_xy, float inv_z,
                          int32_t *__restrict__ hist, int32_t *__restrict__ rank) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const float *p = points + (int64_t)i * stride;
  const int key = nm_key(nm_cell1(p[0], NM_ORG_XY, inv_xy, NM_NX), nm_cell1(p[1], NM_ORG_XY, inv_xy, NM_NY),
                         nm_cell1(p[2], NM_ORG_Z, inv_z, NM_NZ));
  rank[i] = atomicAdd(&hist[key], 1);
}

// exclusive scan of the NM_BINS counters in place (the two launches of chamfer_grid.hip, one segment)
__global__ __launch_bounds__(256) void k_nm_chunk_sums(const int32_t *__restrict__ hist, int32_t *__restrict__ sums) {
  __shared__ int32_t red[4];
  const int32_t *h = hist + (int64_t)blockIdx.x * NM_CHUNK;
  int32_t s = h[threadIdx.x] + h[threadIdx.x + 256] + h[threadIdx.x + 512] + h[threadIdx.x + 768];
  for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) sums[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(256) void k_nm_scan(int32_t *__restrict__ hist, const int32_t *__restrict__ sums) {
  __shared__ int32_t wsum[4];
  __shared__ int32_t carry_s;
  int32_t *h = hist + (int64_t)blockIdx.x * NM_CHUNK;
  int32_t c = 0;
  for (int k = threadIdx.x; k < (int)blockIdx.x; k += 256) c += sums[k];
  for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) carry_s = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  __syncthreads();
  const int4 v = *reinterpret_cast<const int4 *>(h + threadIdx.x * 4);
  const int32_t tot = v.x + v.y + v.z + v.w;
  int32_t inc = tot;
  const int lane = threadIdx.x & 63;
  for (int d = 1; d < 64; d <<= 1) {
    const int32_t t = __shfl_up(inc, d, 64);
    if (lane >= d) inc += t;
  }
  __syncthreads();
  if (lane == 63) wsum[threadIdx.x >> 6] = inc;
  __syncthreads();
  int32_t base = carry_s + inc - tot;
  for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) base += wsum[w];
  *reinterpret_cast<int4 *>(h + threadIdx.x * 4) = make_int4(base, base + v.x, base + v.x + v.y, base + v.x + v.y + v.z);
}

// sorted[off[key] + rank] = (x, y, z, original index); slots [N, Npad) get +inf / index -1
__global__ void k_nm_scatter(const float *__restrict__ points, int stride, int N, int Npad, float inv_xy, float inv_z,
                             const int32_t *__restrict__ off, const int32_t *__restrict__ rank,
                             float4 *__restrict__ sorted) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Npad) return;
  if (i >= N) {
    const float inf = __builtin_inff();
    sorted[i] = make_float4(inf, inf, inf, __int_as_float(-1));
    return;
  }
  const float *p = points + (int64_t)i * stride;
  const float x = p[0], y = p[1], z = p[2];
  const int key = nm_key(nm_cell1(x, NM_ORG_XY, inv_xy, NM_NX), nm_cell1(y, NM_ORG_XY, inv_xy, NM_NY),
                         nm_cell1(z, NM_ORG_Z, inv_z, NM_NZ));
  sorted[off[key] + rank[i]] = make_float4(x, y, z, __int_as_float(i));
}

// merge `key` into the ascending list (NM_KEY_NONE: no-op, every entry is <= it)
__device__ __forceinline__ void nm_insert(nm_u64 (&L)[NM_K], nm_u64 key) {
#pragma unroll
  for (int j = 0; j < NM_K; ++j) {
    const nm_u64 a = L[j];
    const bool lt = key < a;
    L[j] = lt ? key : a;
    key = lt ? a : key;
  }
}

// one cyclic-Jacobi rotation that annihilates a_pq of a symmetric 3x3 (r is the third index); V's columns follow
__device__ __forceinline__ void nm_rot(float &app, float &aqq, float &apq, float &arp, float &arq, float &v0p, float &v0q,
                                       float &v1p, float &v1q, float &v2p, float &v2q) {
  if (apq == 0.0f) return;
  const float theta = (aqq - app) / (2.0f * apq);
  const float t = copysignf(1.0f, theta) / (fabsf(theta) + sqrtf(theta * theta + 1.0f));   // |theta| huge: t -> 0
  const float c = 1.0f / sqrtf(t * t + 1.0f), s = t * c;
  app = app - t * apq;
  aqq = aqq + t * apq;
  apq = 0.0f;
  float u = arp;
  arp = c * u - s * arq;
  arq = s * u + c * arq;
  u = v0p; v0p = c * u - s * v0q; v0q = s * u + c * v0q;
  u = v1p; v1p = c * u - s * v1q; v1q = s * u + c * v1q;
  u = v2p; v2p = c * u - s * v2q; v2q = s * u + c * v2q;
}

__global__ __launch_bounds__(256) void k_nm_normals(const float4 *__restrict__ sorted, const int32_t *__restrict__ off,
                                                    const float *__restrict__ points, int stride, int N, int Npad,
                                                    float r2, int max_nn, float inv_xy, float inv_z, float vx, float vy,
                                                    float vz, int zero_vertical, float *__restrict__ normals,
                                                    int32_t *__restrict__ counts) {
  __shared__ float4 slots[4][NM_TILE];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int qt = blockIdx.x * 4 + wid;
  if (qt * NM_TILE >= Npad) return;      // whole waves leave; the waves of a block never meet at a barrier
  const float4 q = sorted[qt * NM_TILE + lane];
  const int qi = __float_as_int(q.w);
  const float inf = __builtin_inff();
  const bool fin = qi >= 0 && fabsf(q.x) < inf && fabsf(q.y) < inf && fabsf(q.z) < inf;   // NaN compares false
  const int cx = nm_cell1(q.x, NM_ORG_XY, inv_xy, NM_NX);
  const int row = nm_cell1(q.z, NM_ORG_Z, inv_z, NM_NZ) * NM_NY + nm_cell1(q.y, NM_ORG_XY, inv_xy, NM_NY);
  float4 *slot = slots[wid];

  nm_u64 L[NM_K];
#pragma unroll
  for (int j = 0; j < NM_K; ++j) L[j] = NM_KEY_NONE;

  nm_u64 todo = __ballot(fin);
  while (todo) {
    // the lanes are in key order: the first one left has the smallest cx of its row
    const int first = __builtin_ctzll(todo);
    const int r = __builtin_amdgcn_readlane(row, first), c = __builtin_amdgcn_readlane(cx, first);
    const bool mine = fin && row == r && (unsigned)(cx - c) < (unsigned)NM_WIN;
    todo &= ~__ballot(mine);
    const int lo = c > 0 ? c - 1 : 0;
    const int hi = c + NM_WIN < NM_NX ? c + NM_WIN : NM_NX - 1;
    const int rz = r / NM_NY, ry = r % NM_NY;
    for (int dz = -1; dz <= 1; ++dz) {
      const int z = rz + dz;
      if (z < 0 || z >= NM_NZ) continue;
      for (int dy = -1; dy <= 1; ++dy) {
        const int y = ry + dy;
        if (y < 0 || y >= NM_NY) continue;
        const int k0 = nm_key(lo, y, z), k1 = nm_key(hi, y, z) + 1;
        const int beg = off[k0];
        const int end = k1 < NM_BINS ? off[k1] : N;
        for (int t = beg; t < end; t += NM_TILE) {
          const int n = end - t < NM_TILE ? end - t : NM_TILE;
          slot[lane] = lane < n ? sorted[t + lane] : make_float4(inf, inf, inf, __int_as_float(-1));
          __builtin_amdgcn_wave_barrier();
          for (int j = 0; j < n; ++j) {
            const float4 p = slot[j];
            const float dx = p.x - q.x, dy2 = p.y - q.y, dz2 = p.z - q.z;
            const float d2 = (dx * dx + dy2 * dy2) + dz2 * dz2;
            const nm_u64 key = ((nm_u64)(unsigned)__float_as_int(d2) << 32) | (unsigned)__float_as_int(p.w);
            const bool ok = mine && d2 < r2 && key < L[NM_K - 1];     // NaN / inf distances never qualify
            if (__ballot(ok) != 0ull) nm_insert(L, ok ? key : NM_KEY_NONE);
          }
          __builtin_amdgcn_wave_barrier();
        }
      }
    }
  }
  if (qi < 0) return;

  // sums over the selected set in key order, about the query
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, m00 = 0.f, m01 = 0.f, m02 = 0.f, m11 = 0.f, m12 = 0.f, m22 = 0.f;
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < NM_K; ++j) {
    if (j < max_nn && L[j] != NM_KEY_NONE) {
      const float *p = points + (int64_t)(unsigned)L[j] * stride;
      const float ox = p[0] - q.x, oy = p[1] - q.y, oz = p[2] - q.z;
      s0 += ox; s1 += oy; s2 += oz;
      m00 += ox * ox; m01 += ox * oy; m02 += ox * oz;
      m11 += oy * oy; m12 += oy * oz; m22 += oz * oz;
      ++cnt;
    }
  }
  float nx = 0.f, ny = 0.f, nz = 1.f;
  if (cnt >= 3) {
    const float ic = 1.0f / (float)cnt;
    const float mx = s0 * ic, my = s1 * ic, mz = s2 * ic;
    float a00 = m00 * ic - mx * mx, a01 = m01 * ic - mx * my, a02 = m02 * ic - mx * mz;
    float a11 = m11 * ic - my * my, a12 = m12 * ic - my * mz, a22 = m22 * ic - mz * mz;
    const float tr = a00 + a11 + a22;
    if (tr > 0.0f && tr < inf) {
      const float sc = 1.0f / tr;
      a00 *= sc; a01 *= sc; a02 *= sc; a11 *= sc; a12 *= sc; a22 *= sc;
      float v00 = 1.f, v01 = 0.f, v02 = 0.f, v10 = 0.f, v11 = 1.f, v12 = 0.f, v20 = 0.f, v21 = 0.f, v22 = 1.f;
      for (int sweep = 0; sweep < 6; ++sweep) {
        nm_rot(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);     // (p, q, r) = (0, 1, 2)
        nm_rot(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);     // (0, 2, 1)
        nm_rot(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);     // (1, 2, 0)
      }
      const bool c1 = a11 < a00;                       // smallest eigenvalue, ties to the lower index
      const bool c2 = a22 < (c1 ? a11 : a00);
      const float ex = c2 ? v02 : (c1 ? v01 : v00), ey = c2 ? v12 : (c1 ? v11 : v10), ez = c2 ? v22 : (c1 ? v21 : v20);
      const float nn = sqrtf((ex * ex + ey * ey) + ez * ez);
      if (nn > 0.0f && nn < inf) {
        nx = ex / nn; ny = ey / nn; nz = ez / nn;
      }
    }
  }
  if ((nx * (vx - q.x) + ny * (vy - q.y)) + nz * (vz - q.z) < 0.0f) {
    nx = -nx; ny = -ny; nz = -nz;
  }
  if (zero_vertical) {
    if (nx == 0.0f) nx = 0.0f;      // -0 -> +0, what the comparison with |(0, 0, 1)| does
    if (ny == 0.0f) ny = 0.0f;
    if (fabsf(nz) == 1.0f) nz = 0.0f;
  }
  if (!fin) {
    nx = ny = nz = 0.0f;
    cnt = 0;
  }
  normals[(int64_t)qi * 3 + 0] = nx;
  normals[(int64_t)qi * 3 + 1] = ny;
  normals[(int64_t)qi * 3 + 2] = nz;
  if (counts) counts[qi] = cnt;
}

static inline size_t nm_pad(int n) { return (size_t)rslo_cdiv(n > 0 ? n : 1, NM_TILE) * NM_TILE; }

extern "C" size_t rslo_normals_ws_bytes(int N) {
  return ((size_t)NM_BINS + NM_NCHUNK) * sizeof(int32_t) + nm_pad(N) * (sizeof(int32_t) + sizeof(float4)) + 256;
}

extern "C" int rslo_estimate_normals(const float *points, int stride_floats, int N, float radius, int max_nn,
                                     const float *viewpoint3, int zero_vertical, float *normals, int32_t *counts,
                                     void *ws, size_t ws_bytes, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  RSLO_CHECK_ARG(N >= 0, "estimate_normals: N < 0");
  RSLO_CHECK_ARG(max_nn >= 3 && max_nn <= NM_K, "estimate_normals: max_nn must be in 3..32, got %d", max_nn);
  RSLO_CHECK_ARG(radius > 0.0f && radius < __builtin_inff(), "estimate_normals: radius must be positive and finite");
  RSLO_CHECK_ARG(stride_floats >= 3, "estimate_normals: stride_floats must be >= 3");
  if (N == 0) return RSLO_OK;
  RSLO_CHECK_ARG(points && normals && ws, "estimate_normals: null pointer");
  if (ws_bytes < rslo_normals_ws_bytes(N)) {
    rslo_set_error("estimate_normals: workspace too small");
    return RSLO_EWS;
  }
  const int Npad = (int)nm_pad(N);
  int32_t *hist = (int32_t *)ws;
  int32_t *sums = hist + NM_BINS;
  int32_t *rank = sums + NM_NCHUNK;
  float4 *sorted = (float4 *)(((uintptr_t)(rank + Npad) + 15) & ~(uintptr_t)15);
  // cells a little larger than the radius: neighbours stay in adjacent cells whatever the rounding of the cell index
  const float cell_xy = fmaxf(NM_MIN_CELL_XY, radius * 1.0625f), cell_z = fmaxf(NM_MIN_CELL_Z, radius * 1.0625f);
  const float inv_xy = 1.0f / cell_xy, inv_z = 1.0f / cell_z;
  const float vx = viewpoint3 ? viewpoint3[0] : 0.0f, vy = viewpoint3 ? viewpoint3[1] : 0.0f,
              vz = viewpoint3 ? viewpoint3[2] : 0.0f;
  RSLO_HIP(hipMemsetAsync(hist, 0, (size_t)NM_BINS * sizeof(int32_t), s));
  hipLaunchKernelGGL(k_nm_hist, dim3((unsigned)rslo_cdiv(N, 256)), dim3(256), 0, s, points, stride_floats, N, inv_xy,
                     inv_z, hist, rank);
  hipLaunchKernelGGL(k_nm_chunk_sums, dim3(NM_NCHUNK), dim3(256), 0, s, hist, sums);
  hipLaunchKernelGGL(k_nm_scan, dim3(NM_NCHUNK), dim3(256), 0, s, hist, sums);
  hipLaunchKernelGGL(k_nm_scatter, dim3((unsigned)rslo_cdiv(Npad, 256)), dim3(256), 0, s, points, stride_floats, N,
                     Npad, inv_xy, inv_z, hist, rank, sorted);
  hipLaunchKernelGGL(k_nm_normals, dim3((unsigned)rslo_cdiv(Npad / NM_TILE, 4)), dim3(256), 0, s, sorted, hist, points,
                     stride_floats, N, Npad, radius * radius, max_nn, inv_xy, inv_z, vx, vy, vz, zero_vertical, normals,
                     counts);
  RSLO_CHECK_LAUNCH("estimate_normals");
  return RSLO_OK;
}
