// Surfel map: a voxel hash whose cells hold the integer moments of every point ever inserted into them, and the plane
// (mean, normal, variance along the normal) those moments give; a registration target for the plane metric that needs
// no scan normals (rules: include/rslo_hip.h "Surfel map"; float64 restatement: rslo_amd/surfels.py SurfelMapRef).
//
// One caller-owned allocation: header (256 bytes) | keys u64 [cap] | moments i64 [cap, 10] | rows f64 [cap, 8] |
// dirty i32 [cap].  The table is the world voxel map's (map_table.h: map_point, map_mix, the bounded probe; map_core.h:
// the claim probe, the insert_frames scaffold and the rebuild's re-insert pass).
//
// Order freedom.  A point adds fixed-point INTEGERS to its cell -- count, the three first and the six second moments of
// its position inside the cell in units of voxel / 16384 -- by 64-bit integer atomics (the lanes of a wave that follow
// one another into the same slot add up first: sf_add).  Integer sums do not depend on the order or the grouping of
// the adds, so the moments of a cell are a function of the SET of points inserted; the row of a cell is a function of
// its moments, its key and the header, computed by one thread in a fixed order of IEEE double operations.
// No floating-point atomic anywhere.
//
// Visibility: inside the moments kernel every decision rests on the return value of an atomic (the CAS on the key);
// moments are only added to, never read.  The derive kernel is a kernel boundary later: there the moments are final for
// the call, and the one thread that takes a slot's dirty word (atomicExch per scan point, or the slot's own thread in
// the per-slot pass of rslo_surfel_insert_frames) reads them and writes the row.  The search kernels only READ the
// table.  Nothing communicates across workgroups except through integer atomics and kernel boundaries.
#include "rslo_common.h"

#include <cstddef>
#include <math.h>

#include "map_table.h"

#pragma clang fp contract(off)   /* every rule is stated operation by operation */

#include "map_core.h"            /* the table's write side, shared with csrc/map.hip */
#include "gauss_newton.h"        /* after the pragma and after map_table.h's se3.h */
#include "gn_register.h"         /* the registration scaffold: workspace, accumulate and finish kernels, shared rules */

#define SF_MAGIC 0x52534c4f53524631ull   /* "RSLOSRF1" */
#define SF_HDR_BYTES 256
#define SF_SLOT_BYTES 156                /* key 8 + moments 80 + row 64 + dirty 4 */
#define SF_Q 16384.0                     /* fixed-point steps per cell edge */

struct SurfHdr {      // int64 words: 0 magic, 1 capacity, 2-4 map parameters, 5-7 plane parameters, 8-14 counters, 15-17 prune
  map_u64 magic;
  long long capacity;
  double voxel, min_range, max_range;
  long long min_points;
  double planar_ratio, line_ratio;
  map_u64 n_scans, n_cells, n_points, dropped_invalid, dropped_range, dropped_full, n_planar;
  map_u64 n_prunes, n_evicted, n_lost;
};
static_assert(sizeof(SurfHdr) <= SF_HDR_BYTES, "surfel header");
static_assert(offsetof(SurfHdr, n_prunes) == 8 * RSLO_SURFEL_HDR_PRUNE, "the prune counters are header words 15 .. 17");
static_assert(table_tally_mirrors<SurfHdr>(), "InsertTally mirrors the header's counters");

struct SurfView {
  SurfHdr *hdr;
  map_u64 *keys;
  long long *mom;
  double *rows;
  int32_t *dirty;
};

__device__ __forceinline__ bool sf_view(void *map, long long cap_max, SurfView &v) {
  SurfHdr *h = (SurfHdr *)map;
  const long long cap = h->capacity;
  if (h->magic != SF_MAGIC || cap < MAP_MIN_CAP || cap > cap_max || (cap & (cap - 1))) return false;
  unsigned char *p = (unsigned char *)map + SF_HDR_BYTES;
  v.hdr = h;
  v.keys = (map_u64 *)p;
  v.mom = (long long *)(p + (size_t)cap * 8);
  v.rows = (double *)(p + (size_t)cap * 88);
  v.dirty = (int32_t *)(p + (size_t)cap * 152);
  return true;
}
__device__ __forceinline__ bool table_view(void *map, long long cap_max, SurfView &v) { return sf_view(map, cap_max, v); }

extern "C" size_t rslo_surfel_bytes(int64_t capacity) {
  if (capacity < MAP_MIN_CAP || capacity > ((int64_t)1 << 31) || (capacity & (capacity - 1))) return 0;
  return (size_t)SF_HDR_BYTES + (size_t)SF_SLOT_BYTES * (size_t)capacity;
}

static long long sf_cap_of_bytes(size_t bytes) { return table_cap_of_bytes(bytes, SF_HDR_BYTES, SF_SLOT_BYTES); }

__global__ __launch_bounds__(256) void k_surfel_reset(void *map, long long cap, double voxel, double min_range,
                                                      double max_range, int min_points, double planar_ratio,
                                                      double line_ratio) {
  unsigned char *p = (unsigned char *)map + SF_HDR_BYTES;
  map_u64 *keys = (map_u64 *)p;
  long long *mom = (long long *)(p + (size_t)cap * 8);
  double *rows = (double *)(p + (size_t)cap * 88);
  int32_t *dirty = (int32_t *)(p + (size_t)cap * 152);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    SurfHdr *h = (SurfHdr *)map;
    h->magic = SF_MAGIC;
    h->capacity = cap;
    h->voxel = voxel;
    h->min_range = min_range;
    h->max_range = max_range;
    h->min_points = min_points;
    h->planar_ratio = planar_ratio;
    h->line_ratio = line_ratio;
    h->n_scans = h->n_cells = h->n_points = h->dropped_invalid = h->dropped_range = h->dropped_full = h->n_planar = 0;
    h->n_prunes = h->n_evicted = h->n_lost = 0;
  }
  for (long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x; s < cap; s += (long long)gridDim.x * blockDim.x) {
    keys[s] = MAP_KEY_NONE;
    for (int k = 0; k < 10; ++k) mom[s * 10 + k] = 0;
    for (int k = 0; k < 8; ++k) rows[s * 8 + k] = 0.0;
    dirty[s] = 0;
  }
}

// One point (p: x, y, z) under `pose` into the table, by table_slot (map_core.h); counters go to `c`, the header itself
// or a workgroup's tally in LDS.  -> the slot and the point's fixed-point position q in its cell, or -1 for a point
// that was dropped.  The one probe of both calls.
template <class Counters>
__device__ __forceinline__ int32_t sf_slot(const SurfView &m, Counters *c, const float *__restrict__ p,
                                           const double *__restrict__ pose, long long *q) {
  double w[3];
  const double voxel = m.hdr->voxel;
  const int32_t s = table_slot(m, c, p, pose, w);
  if (s < 0) return -1;
  for (int a = 0; a < 3; ++a) {
    const double sc = w[a] / voxel;
    const double f = sc - floor(sc);                     // 1.0 for a tiny negative sc: the clamp below is part of the rule
    long long v = (long long)floor(f * SF_Q);
    q[a] = v < 0 ? 0 : (v > 16383 ? 16383 : v);
  }
  atomicAdd(&c->n_points, (map_u64)1);
  return s;
}

// The ten adds of a wave's points, called by EVERY lane of the wave (s = -1: nothing to add).  Consecutive points of a
// scan mostly share a cell (a beam sweeps 3 cm per point at 10 m), and adds to one address are served one after the
// other on the memory side: measured, the plain ten atomics per point took 110 us per 119k-point scan at 0.4 m cells
// and 193 us at 0.8 m, against 30 us for the voxel map's insert -- the time grew with the cell, not with the bytes.  So
// the lanes of a RUN of equal slots (adjacent lanes only) add up inside the wave, by a segmented inclusive scan, and
// the last lane of a run issues the run's ten atomics.  Integer sums: no bit of the table depends on the grouping.
__device__ __forceinline__ void sf_add(const SurfView &m, int32_t s, const long long *q) {
  const int lane = threadIdx.x & 63;
  const int32_t before = __shfl_up(s, 1, 64);
  const map_u64 heads = __ballot(lane == 0 || before != s);             // bit l: lane l starts a run (bit 0 always)
  const int start = 63 - __builtin_clzll(heads & (~(map_u64)0 >> (63 - lane)));      // first lane of this lane's run
  map_u64 v[10] = {1, (map_u64)q[0], (map_u64)q[1], (map_u64)q[2], (map_u64)(q[0] * q[0]), (map_u64)(q[0] * q[1]),
                   (map_u64)(q[0] * q[2]), (map_u64)(q[1] * q[1]), (map_u64)(q[1] * q[2]), (map_u64)(q[2] * q[2])};
  for (int off = 1; off < 64; off <<= 1) {
    const bool take = lane - off >= start;
#pragma unroll
    for (int k = 0; k < 10; ++k) {
      const map_u64 t = __shfl_up(v[k], off, 64);
      if (take) v[k] += t;
    }
  }
  const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1);
  if (tail && s >= 0) {
    map_u64 *mo = (map_u64 *)(m.mom + (size_t)s * 10);      // two's complement: the unsigned add is the signed add
#pragma unroll
    for (int k = 0; k < 10; ++k) atomicAdd(mo + k, v[k]);
    m.dirty[s] = 1;      // every writer stores the same word; the kernel boundary publishes it
  }
}

// nm_rot of csrc/normals.hip in double: one cyclic-Jacobi rotation that annihilates a_pq (r is the third index)
__device__ __forceinline__ void sf_rot(double &app, double &aqq, double &apq, double &arp, double &arq, double &v0p,
                                       double &v0q, double &v1p, double &v1q, double &v2p, double &v2q) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  app = app - t * apq;
  aqq = aqq + t * apq;
  apq = 0.0;
  double u = arp;
  arp = c * u - s * arq;
  arq = s * u + c * arq;
  u = v0p; v0p = c * u - s * v0q; v0q = s * u + c * v0q;
  u = v1p; v1p = c * u - s * v1q; v1q = s * u + c * v1q;
  u = v2p; v2p = c * u - s * v2q; v2q = s * u + c * v2q;
}

// The row of slot s from its moments, its key and the header (rules: "Derive"), written in place.  -> the change of
// the slot's "planar" bit (new flag == 2) - (old flag == 2).  Shared by the per-scan and the per-slot pass.
__device__ __forceinline__ int sf_derive(const SurfView &m, size_t s) {
  const long long *mo = m.mom + s * 10;
  double *row = m.rows + s * 8;
  const int was = row[7] == 2.0;
  const long long N = mo[0];
  const double n = (double)N;
  const double mu0 = (double)mo[1] / n, mu1 = (double)mo[2] / n, mu2 = (double)mo[3] / n;
  double a00 = (double)mo[4] / n - mu0 * mu0, a01 = (double)mo[5] / n - mu0 * mu1, a02 = (double)mo[6] / n - mu0 * mu2;
  double a11 = (double)mo[7] / n - mu1 * mu1, a12 = (double)mo[8] / n - mu1 * mu2, a22 = (double)mo[9] / n - mu2 * mu2;
  const double tr = (a00 + a11) + a22;
  if (N < m.hdr->min_points || !(tr > 0.0 && tr < (double)__builtin_inff())) {
    for (int k = 0; k < 8; ++k) row[k] = 0.0;
    return 0 - was;
  }
  a00 = a00 / tr; a01 = a01 / tr; a02 = a02 / tr; a11 = a11 / tr; a12 = a12 / tr; a22 = a22 / tr;
  double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
  for (int sweep = 0; sweep < 6; ++sweep) {
    sf_rot(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);     // (p, q, r) = (0, 1, 2)
    sf_rot(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);     // (0, 2, 1)
    sf_rot(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);     // (1, 2, 0)
  }
  const bool c1 = a11 < a00;                       // smallest eigenvalue, ties to the lower index (k_nm_normals)
  const bool c2 = a22 < (c1 ? a11 : a00);
  const double l0 = c2 ? a22 : (c1 ? a11 : a00);
  const double ra = c2 ? a00 : (c1 ? a00 : a11), rb = c2 ? a11 : a22;      // the other two, lower index first
  const bool c3 = rb < ra;
  const double l1 = c3 ? rb : ra, l2 = c3 ? ra : rb;
  const double ex = c2 ? v02 : (c1 ? v01 : v00), ey = c2 ? v12 : (c1 ? v11 : v10), ez = c2 ? v22 : (c1 ? v21 : v20);
  const double nn = sqrt((ex * ex + ey * ey) + ez * ez);
  double nx = ex / nn, ny = ey / nn, nz = ez / nn;
  double big = nx;                                 // the component of largest magnitude, ties to the lower axis
  if (fabs(ny) > fabs(big)) big = ny;
  if (fabs(nz) > fabs(big)) big = nz;
  if (big < 0.0) {
    nx = -nx; ny = -ny; nz = -nz;
  }
  const map_u64 key = m.keys[s];
  const double voxel = m.hdr->voxel;
  const double cx = (double)((long long)((key >> 42) & 0x1fffff) - 1048576);
  const double cy = (double)((long long)((key >> 21) & 0x1fffff) - 1048576);
  const double cz = (double)((long long)(key & 0x1fffff) - 1048576);
  const double u = voxel / SF_Q;
  const int planar = l0 <= m.hdr->planar_ratio * l1 && l1 >= m.hdr->line_ratio * l2;
  row[0] = (cx + (mu0 + 0.5) / SF_Q) * voxel;
  row[1] = (cy + (mu1 + 0.5) / SF_Q) * voxel;
  row[2] = (cz + (mu2 + 0.5) / SF_Q) * voxel;
  row[3] = nx;
  row[4] = ny;
  row[5] = nz;
  row[6] = ((l0 * tr) * u) * u;
  row[7] = planar ? 2.0 : 1.0;
  return planar - was;
}

__global__ __launch_bounds__(256) void k_surfel_moments(void *map, long long cap_max, const float *__restrict__ points,
                                                        int stride, int N, const double *__restrict__ pose,
                                                        int32_t *__restrict__ slot_of) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  SurfView m;
  if (!sf_view(map, cap_max, m)) {      // uniform over the grid
    if (i < N) slot_of[i] = -1;
    return;
  }
  int32_t s = -1;
  long long q[3] = {0, 0, 0};
  if (i < N) {
    s = sf_slot(m, m.hdr, points + (int64_t)i * stride, pose, q);
    slot_of[i] = s;
  }
  sf_add(m, s, q);      // every lane of the wave, the ones past N included
}

// behind the kernel boundary the moments are final for this scan: whoever takes a slot's dirty word derives its row.
// n_planar moves by the workgroup's integer sum, one add per workgroup.
__global__ __launch_bounds__(256) void k_surfel_derive_scan(void *map, long long cap_max, int N,
                                                            const int32_t *__restrict__ slot_of) {
  __shared__ int moved;
  if (threadIdx.x == 0) moved = 0;
  __syncthreads();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  SurfView m;
  const bool ok = sf_view(map, cap_max, m);      // uniform over the grid
  if (ok && i < N) {
    const int32_t s = slot_of[i];
    // (a plain pre-read of the dirty word in front of the exchange was tried: 28 us per 119k-point scan with and without)
    if (s >= 0 && (long long)s < m.hdr->capacity && atomicExch(&m.dirty[s], 0) == 1) {
      const int d = sf_derive(m, (size_t)s);
      if (d) atomicAdd(&moved, d);
    }
  }
  __syncthreads();
  if (ok && threadIdx.x == 0 && moved) atomicAdd(&m.hdr->n_planar, (map_u64)(long long)moved);
}

// ---------------------------------------------------------------------------------------------------------------------
// rslo_surfel_insert_frames: every frame of a keyframe store under its own pose.  Three launches whatever the data.
// ---------------------------------------------------------------------------------------------------------------------
// pass 1 is k_table_frames_points (map_core.h) with this body, which every lane of the wave enters.  Pass 3,
// k_table_frames_done, is map_core.h's as well; table_insert_frames launches the three.
struct SfFramesBody {
  static __device__ __forceinline__ void point(const SurfView &m, InsertTally *tally, bool valid, const float *p,
                                               const double *pose, map_u64, uint32_t) {
    int32_t s = -1;
    long long q[3] = {0, 0, 0};
    if (valid) s = sf_slot(m, tally, p, pose, q);
    sf_add(m, s, q);      // every lane of the wave
  }
};

// pass 2, over the SLOTS: a slot belongs to one thread, which clears its dirty word and derives its row
__global__ __launch_bounds__(256) void k_surfel_derive_slots(void *map, long long cap_max) {
  __shared__ int moved;
  if (threadIdx.x == 0) moved = 0;
  __syncthreads();
  SurfView m;
  const bool ok = sf_view(map, cap_max, m);      // uniform over the grid
  if (ok) {
    const long long cap = m.hdr->capacity;
    for (long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x; s < cap; s += (long long)gridDim.x * blockDim.x) {
      if (m.dirty[s] == 0) continue;
      m.dirty[s] = 0;
      const int d = sf_derive(m, (size_t)s);
      if (d) atomicAdd(&moved, d);
    }
  }
  __syncthreads();
  if (ok && threadIdx.x == 0 && moved) atomicAdd(&m.hdr->n_planar, (map_u64)(long long)moved);
}

__global__ __launch_bounds__(256) void k_surfel_export(void *map, long long cap_max, int min_flag,
                                                       const double *__restrict__ center, double radius,
                                                       map_u64 *__restrict__ keys, long long *__restrict__ moments,
                                                       double *__restrict__ rows, long long max_rows,
                                                       map_u64 *__restrict__ counts) {
  SurfView m;
  if (!sf_view(map, cap_max, m)) return;
  const long long cap = m.hdr->capacity;
  for (long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x; s < cap; s += (long long)gridDim.x * blockDim.x) {
    const map_u64 key = m.keys[s];
    if (key == MAP_KEY_NONE) continue;
    const double *row = m.rows + (size_t)s * 8;
    if (!(row[7] >= (double)min_flag)) continue;
    if (center) {
      const double dx = row[0] - center[0], dy = row[1] - center[1], dz = row[2] - center[2];
      if (!(dx * dx + dy * dy + dz * dz < radius * radius)) continue;
    }
    const map_u64 o = atomicAdd(&counts[0], (map_u64)1);
    if ((long long)o < max_rows) {
      atomicAdd(&counts[1], (map_u64)1);
      keys[o] = key;
      for (int k = 0; k < 10; ++k) moments[o * 10 + k] = m.mom[(size_t)s * 10 + k];
      for (int k = 0; k < 8; ++k) rows[o * 8 + k] = row[k];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// rslo_surfel_prune: evict far and sparse cells by rebuilding the table (rules: "Rolling local surfel map").  Five
// launches whatever the data.  Workspace: control block (256 bytes, zeroed by the first, one-thread launch) | staged
// keys u64 [cap] | moments i64 [cap, 10] | rows f64 [cap, 8] -- the table's own section layout without the dirty words.
// Rows are copied as 64-bit words, never re-derived.
// ---------------------------------------------------------------------------------------------------------------------
#define SF_STAGE_BYTES 152               /* key 8 + moments 80 + row 64 */
struct SfStage {
  RebuildCtl *ctl;
  map_u64 *keys, *mom, *rows;
};

__device__ __forceinline__ SfStage sf_stage(void *ws, long long cap) {
  unsigned char *p = (unsigned char *)ws + PRUNE_CTL_BYTES;
  SfStage st;
  st.ctl = (RebuildCtl *)ws;
  st.keys = (map_u64 *)p;
  st.mom = (map_u64 *)(p + (size_t)cap * 8);
  st.rows = (map_u64 *)(p + (size_t)cap * 88);
  return st;
}

// pass 1: keep or evict every stored cell from its key and its count alone; the other 144 bytes are read for kept cells
// only.  A wave walks SF_PRUNE_STEP * 64 consecutive slots at a time, SF_PRUNE_STEP per lane (the capacity is a
// multiple of that, so every lane of the wave is in range and takes part in the ballots).  The staging cursor moves
// ONCE per wave and step, by the number of kept slots among those 512: adds to one address are served one after the
// other, about 13 ns each (measured: one add per 64 slots made this launch 211 us at 2^20 slots, and a second add per
// wave for the evictions 77 us more), so the evictions are summed over the workgroup in LDS and added once.
#define SF_PRUNE_STEP 8
static_assert(MAP_MIN_CAP % (SF_PRUNE_STEP * 64) == 0, "a wave's step divides every capacity");

__global__ __launch_bounds__(256) void k_surfel_prune_scan(void *map, long long cap_max, const double *__restrict__ center,
                                                           double radius, double inner_radius, int min_count, void *ws) {
  __shared__ unsigned int gone_wg;
  if (threadIdx.x == 0) gone_wg = 0;
  __syncthreads();
  SurfView m;
  if (!sf_view(map, cap_max, m)) return;      // uniform over the grid
  const long long cap = m.hdr->capacity;
  const SfStage st = sf_stage(ws, cap);
  const double voxel = m.hdr->voxel;
  double c[3] = {0.0, 0.0, 0.0};
  if (center) c[0] = center[0], c[1] = center[1], c[2] = center[2];
  const int lane = threadIdx.x & 63;
  const map_u64 below = ((map_u64)1 << lane) - 1;      // the lanes in front of this one
  unsigned int gone = 0;
  for (long long s0 = ((long long)blockIdx.x * blockDim.x + (threadIdx.x & ~63u)) * SF_PRUNE_STEP; s0 < cap;
       s0 += (long long)gridDim.x * blockDim.x * SF_PRUNE_STEP) {
    map_u64 key[SF_PRUNE_STEP], kept[SF_PRUNE_STEP];
    long long N[SF_PRUNE_STEP];
#pragma unroll
    for (int j = 0; j < SF_PRUNE_STEP; ++j) key[j] = m.keys[(size_t)s0 + j * 64 + lane];
#pragma unroll
    for (int j = 0; j < SF_PRUNE_STEP; ++j) N[j] = key[j] != MAP_KEY_NONE ? m.mom[((size_t)s0 + j * 64 + lane) * 10] : 0;
    unsigned int total = 0;
#pragma unroll
    for (int j = 0; j < SF_PRUNE_STEP; ++j) {
      const bool stored = key[j] != MAP_KEY_NONE;
      bool keep = stored && N[j] >= (long long)min_count;
      if (stored && center) {      // the cell's centre, not the row's mean: a comparison that is false evicts
        const double cx = ((double)((long long)((key[j] >> 42) & 0x1fffff) - 1048576) + 0.5) * voxel;
        const double cy = ((double)((long long)((key[j] >> 21) & 0x1fffff) - 1048576) + 0.5) * voxel;
        const double cz = ((double)((long long)(key[j] & 0x1fffff) - 1048576) + 0.5) * voxel;
        const double dx = cx - c[0], dy = cy - c[1], dz = cz - c[2];
        const double d2 = dx * dx + dy * dy + dz * dz;
        keep = (keep || d2 < inner_radius * inner_radius) && d2 < radius * radius;
      }
      kept[j] = __ballot(keep);
      total += (unsigned int)__popcll(kept[j]);
      gone += (unsigned int)__popcll(__ballot(stored && !keep));
    }
    if (total == 0) continue;      // uniform over the wave
    map_u64 base = 0;
    if (lane == 0) base = atomicAdd(&st.ctl->kept, (map_u64)total);
    base = __shfl(base, 0, 64);
#pragma unroll
    for (int j = 0; j < SF_PRUNE_STEP; ++j) {
      const map_u64 o = base + (map_u64)__popcll(kept[j] & below);
      base += (map_u64)__popcll(kept[j]);
      if (((kept[j] >> lane) & 1) && o < (map_u64)cap) {      // always: one record per slot at most, the cursor starts at 0
        const size_t s = (size_t)s0 + j * 64 + lane;
        const map_u64 *mo = (const map_u64 *)m.mom + s * 10, *row = (const map_u64 *)m.rows + s * 8;
        st.keys[o] = key[j];
        st.mom[o * 10] = (map_u64)N[j];
        for (int k = 1; k < 10; ++k) st.mom[o * 10 + k] = mo[k];
        for (int k = 0; k < 8; ++k) st.rows[o * 8 + k] = row[k];
      }
    }
  }
  if (lane == 0 && gone) atomicAdd(&gone_wg, gone);      // every wave counted the same slots on all its lanes
  __syncthreads();
  if (threadIdx.x == 0 && gone_wg) atomicAdd(&st.ctl->evicted, (map_u64)gone_wg);
}

// pass 2: the state k_surfel_reset leaves in the sections.  An empty slot is in that state already (a slot gets moments,
// a row or a dirty word only behind its key), so only the stored slots are written: the pass reads the keys and
// writes 156 bytes per stored cell.  Nothing evicted: the table stays as it is, to the byte.
__global__ __launch_bounds__(256) void k_surfel_prune_clear(void *map, long long cap_max, const void *ws) {
  SurfView m;
  if (!sf_view(map, cap_max, m)) return;
  if (((const RebuildCtl *)ws)->evicted == 0) return;
  const long long cap = m.hdr->capacity;
  for (long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x; s < cap; s += (long long)gridDim.x * blockDim.x) {
    if (m.keys[s] == MAP_KEY_NONE) continue;
    m.keys[s] = MAP_KEY_NONE;
    for (int k = 0; k < 10; ++k) m.mom[s * 10 + k] = 0;
    for (int k = 0; k < 8; ++k) m.rows[s * 8 + k] = 0.0;
    m.dirty[s] = 0;
  }
}

// pass 3 is k_table_reinsert (map_core.h) over these records: the CAS winner writes moments and row as 64-bit words
struct SfRecords {
  static __device__ __forceinline__ SfStage stage(void *ws, long long cap) { return sf_stage(ws, cap); }
  static __device__ __forceinline__ unsigned put(const SurfView &m, const SfStage &st, size_t i, size_t s) {
    map_u64 *mo = (map_u64 *)m.mom + s * 10, *row = (map_u64 *)m.rows + s * 8;
    for (int k = 0; k < 10; ++k) mo[k] = st.mom[i * 10 + k];
    for (int k = 0; k < 8; ++k) row[k] = st.rows[i * 8 + k];
    return st.rows[i * 8 + 7] == 0x4000000000000000ull;      // the bits of 2.0
  }
};

__global__ void k_surfel_prune_done(void *map, long long cap_max, const void *ws) {
  SurfView m;
  if (threadIdx.x != 0 || !sf_view(map, cap_max, m)) return;
  const RebuildCtl *ctl = (const RebuildCtl *)ws;
  m.hdr->n_prunes = m.hdr->n_prunes + 1;
  if (ctl->evicted == 0) return;
  m.hdr->n_cells = ctl->kept - ctl->lost;
  m.hdr->n_planar = ctl->planar;
  m.hdr->n_evicted = m.hdr->n_evicted + ctl->evicted;
  m.hdr->n_lost = m.hdr->n_lost + ctl->lost;
}

// ---------------------------------------------------------------------------------------------------------------------
// Search and registration (rules: "Nearest", "Normal equations", "Register").  Read-only on the table.
// ---------------------------------------------------------------------------------------------------------------------
// The cell whose mean is nearest to w among the cells key + {-1,0,1}^3: slot, key and d2 of the winner (smallest d2, then
// smallest key), d = w - mean.  Rows are read for matching cells only.  PLANAR (the plane calls): the candidates are the
// rows with flag 2.0 and min_flag is not read; otherwise (the distribution calls) the rows with flag >= min_flag.
template <bool PLANAR>
__device__ __forceinline__ bool sf_nearest(const SurfView &m, map_u64 key, const double *w, double min_flag,
                                           uint32_t &bslot, map_u64 &bkey, double &bd2, double *d) {
  bool found = false;
  map_neighbours(m.keys, m.hdr->capacity, key, [&](uint32_t s, map_u64 nk) {
    const double *row = m.rows + (size_t)s * 8;
    if (PLANAR ? row[7] != 2.0 : !(row[7] >= min_flag)) return;
    const double dx = w[0] - row[0], dy = w[1] - row[1], dz = w[2] - row[2];
    const double d2 = dx * dx + dy * dy + dz * dz;
    if (!found || d2 < bd2 || (d2 == bd2 && nk < bkey)) {
      found = true;
      bslot = s;
      bkey = nk;
      bd2 = d2;
      d[0] = dx;
      d[1] = dy;
      d[2] = dz;
    }
  });
  return found;
}

// The match of scan point p under `pose` in the map as the search calls accept it (reset, and with the cell edge the
// caller was checked against): world position w, slot s, key and d = w - mean of the nearest candidate, closer than max_dist
template <bool PLANAR>
__device__ __forceinline__ bool sf_match(const void *map, long long cap_max, double voxel, const float *p, const double *pose,
                                         double max_dist, double min_flag, SurfView &m, double *w, uint32_t &s,
                                         map_u64 &bkey, double &bd2, double *d) {
  map_u64 key;
  return sf_view((void *)map, cap_max, m) && m.hdr->voxel == voxel &&
         !map_point(p, pose, m.hdr->voxel, m.hdr->min_range, m.hdr->max_range, key, w) &&
         sf_nearest<PLANAR>(m, key, w, min_flag, s, bkey, bd2, d) && bd2 < max_dist * max_dist;
}

// The parameters of the distribution cost (rules: "Distribution cost"): the matched cell's covariance, regularised and
// inverted, weighs the whole residual d = w - mean.  The candidates are the rows with flag >= min_flag.
struct SfDist {
  double min_flag, reg_rel, reg_abs;
};

// The information matrix M6 (00 01 02 11 12 22) of a slot from its ten moments mo: the derive pass's covariance in
// metres plus lam on the diagonal, inverted by the adjugate.  -> whether the pair is usable (det > 0 && det < inf).
__device__ __forceinline__ bool sf_information(const long long *__restrict__ mo, double voxel, const SfDist &dd, double *M6,
                                               double &det, double &lam) {
  long long q[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) q[k] = mo[k];      // the 80 contiguous bytes of the slot
  const double n = (double)q[0];
  const double mu0 = (double)q[1] / n, mu1 = (double)q[2] / n, mu2 = (double)q[3] / n;
  const double c00 = (double)q[4] / n - mu0 * mu0, c01 = (double)q[5] / n - mu0 * mu1, c02 = (double)q[6] / n - mu0 * mu2;
  const double c11 = (double)q[7] / n - mu1 * mu1, c12 = (double)q[8] / n - mu1 * mu2, c22 = (double)q[9] / n - mu2 * mu2;
  const double u = voxel / SF_Q;
  const double C00 = (c00 * u) * u, C01 = (c01 * u) * u, C02 = (c02 * u) * u;
  const double C11 = (c11 * u) * u, C12 = (c12 * u) * u, C22 = (c22 * u) * u;
  lam = dd.reg_rel * ((C00 + C11) + C22) + dd.reg_abs * dd.reg_abs;
  const double S00 = C00 + lam, S01 = C01, S02 = C02, S11 = C11 + lam, S12 = C12, S22 = C22 + lam;
  const double A00 = S11 * S22 - S12 * S12, A01 = S02 * S12 - S01 * S22, A02 = S01 * S12 - S02 * S11;
  const double A11 = S00 * S22 - S02 * S02, A12 = S01 * S02 - S00 * S12, A22 = S00 * S11 - S01 * S01;
  det = (S00 * A00 + S01 * A01) + S02 * A02;
  M6[0] = A00 / det; M6[1] = A01 / det; M6[2] = A02 / det;
  M6[3] = A11 / det; M6[4] = A12 / det; M6[5] = A22 / det;
  return det > 0.0 && det < (double)__builtin_inff();
}

// PLANAR: the plane calls' search; dd and info_out are not read.  Otherwise the distribution calls', with
// info_out row = {M00, M01, M02, M11, M12, M22, det, lam} of the matched cell (M as zeros for an unusable pair)
template <bool PLANAR>
__global__ __launch_bounds__(GN_BLOCK) void k_surfel_nearest(const void *map, long long cap_max, double voxel,
                                                             const float *__restrict__ points, int stride, int N,
                                                             const double *__restrict__ pose, double max_dist, SfDist dd,
                                                             long long *__restrict__ keys_out, double *__restrict__ d2_out,
                                                             double *__restrict__ rows_out, double *__restrict__ info_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  SurfView m;
  long long kout = -1;
  double d2 = -1.0;
  map_u64 bkey;
  double w[3], d[3], bd2;
  uint32_t s = 0;
  bool got = false;
  if (sf_match<PLANAR>(map, cap_max, voxel, points + (int64_t)i * stride, pose, max_dist, dd.min_flag, m, w, s, bkey, bd2, d)) {
    kout = (long long)bkey;
    d2 = bd2;
    got = true;
  }
  keys_out[i] = kout;
  d2_out[i] = d2;
  if (rows_out) {
    const double *row = got ? m.rows + (size_t)s * 8 : nullptr;
    for (int k = 0; k < 8; ++k) rows_out[(size_t)i * 8 + k] = row ? row[k] : 0.0;
  }
  if (!PLANAR && info_out) {
    double v[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (got) {
      const bool usable = sf_information(m.mom + (size_t)s * 10, m.hdr->voxel, dd, v, v[6], v[7]);
      if (!usable)
        for (int k = 0; k < 6; ++k) v[k] = 0.0;
    }
    for (int k = 0; k < 8; ++k) info_out[(size_t)i * 8 + k] = v[k];
  }
}

// The plane cost: one plane term with the matched planar cell's normal, e = r*r
struct SfPlaneCost {
  const void *map;
  long long cap_max;
  double voxel;

  __device__ __forceinline__ bool terms(const float *p, const double *pose, double max_dist, double *acc) const {
    SurfView m;
    map_u64 bkey;
    double w[3], d[3], bd2;
    uint32_t s;
    if (!sf_match<true>(map, cap_max, voxel, p, pose, max_dist, 2.0, m, w, s, bkey, bd2, d)) return false;
    const double *row = m.rows + (size_t)s * 8;
    const double n[3] = {row[3], row[4], row[5]};      // already in the world frame
    double wn[3];
    se3_cross(w, n, wn);
    gn_plane_terms(n, wn, n[0] * d[0] + n[1] * d[1] + n[2] * d[2], acc);
    return true;
  }
};

// The distribution cost, e = d^T M d.  The match comes first and leaves slot and d; only then are the winner's moments
// read, so the 27-key arrays of the search are dead while M and the 3 x 6 product M J are live.  An unusable pair adds
// nothing and is not counted.
struct SfDistCost {
  const void *map;
  long long cap_max;
  double voxel;
  SfDist dd;

  __device__ __forceinline__ bool terms(const float *p, const double *pose, double max_dist, double *acc) const {
    SurfView m;
    map_u64 bkey;
    double w[3], d[3], bd2;
    uint32_t s;
    if (!sf_match<false>(map, cap_max, voxel, p, pose, max_dist, dd.min_flag, m, w, s, bkey, bd2, d)) return false;
    double M6[6], det, lam;
    if (!sf_information(m.mom + (size_t)s * 10, m.hdr->voxel, dd, M6, det, lam)) return false;
    gn_info_terms(w, d, M6, acc);
    return true;
  }
};

// ---------------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------------
extern "C" int rslo_surfel_reset(void *map, size_t map_bytes, int64_t capacity, double voxel_size, double min_range,
                                 double max_range, int min_points, double planar_ratio, double line_ratio, void *stream) {
  RSLO_CHECK_ARG(map && ((uintptr_t)map & 7) == 0, "surfel_reset: map is null or not 8-byte aligned");
  RSLO_CHECK_ARG(rslo_surfel_bytes(capacity) != 0, "surfel_reset: capacity must be a power of two in 1024 .. 2^31");
  RSLO_CHECK_ARG(map_bytes >= rslo_surfel_bytes(capacity), "surfel_reset: map_bytes is smaller than rslo_surfel_bytes(capacity)");
  RSLO_CHECK_ARG(voxel_size > 0.0 && voxel_size < (double)__builtin_inff(),
                 "surfel_reset: voxel_size must be positive and finite");
  RSLO_CHECK_ARG(min_range >= 0.0 && min_range < max_range, "surfel_reset: need 0 <= min_range < max_range");
  RSLO_CHECK_ARG(min_points >= 3, "surfel_reset: min_points must be >= 3");
  RSLO_CHECK_ARG(planar_ratio >= 0.0 && planar_ratio < (double)__builtin_inff() && line_ratio >= 0.0 &&
                     line_ratio < (double)__builtin_inff(),
                 "surfel_reset: planar_ratio and line_ratio must be >= 0 and finite (NaN is refused)");
  const unsigned nb = (unsigned)(capacity / 256 < 4096 ? capacity / 256 : 4096);
  hipLaunchKernelGGL(k_surfel_reset, dim3(nb), dim3(256), 0, (hipStream_t)stream, map, (long long)capacity, voxel_size,
                     min_range, max_range, min_points, planar_ratio, line_ratio);
  RSLO_CHECK_LAUNCH("surfel_reset");
  return RSLO_OK;
}

extern "C" size_t rslo_surfel_insert_ws_bytes(int N) {
  return N < 0 ? 0 : 256 + ((size_t)N * 4 + 255) / 256 * 256;
}

extern "C" int rslo_surfel_insert(void *map, size_t map_bytes, const float *points, int stride_floats, int N,
                                  const double *pose7, void *ws, size_t ws_bytes, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  const long long cap_max = sf_cap_of_bytes(map_bytes);
  RSLO_CHECK_ARG(map && cap_max > 0, "surfel_insert: no map (map_bytes below rslo_surfel_bytes(1024))");
  RSLO_CHECK_ARG(N >= 0 && stride_floats >= 3, "surfel_insert: N < 0 or stride_floats < 3");
  RSLO_CHECK_ARG(pose7, "surfel_insert: pose7 is null");
  if (N > 0) {
    RSLO_CHECK_ARG(points && ws, "surfel_insert: null pointer");
    if (ws_bytes < rslo_surfel_insert_ws_bytes(N)) {
      rslo_set_error("surfel_insert: workspace too small");
      return RSLO_EWS;
    }
    int32_t *slot_of = table_slot_of(ws);
    const unsigned nb = (unsigned)rslo_cdiv(N, 256);
    hipLaunchKernelGGL(k_surfel_moments, dim3(nb), dim3(256), 0, s, map, cap_max, points, stride_floats, N, pose7, slot_of);
    hipLaunchKernelGGL(k_surfel_derive_scan, dim3(nb), dim3(256), 0, s, map, cap_max, N, (const int32_t *)slot_of);
  }
  hipLaunchKernelGGL(k_table_scan_done<SurfView>, dim3(1), dim3(64), 0, s, map, cap_max);      // N == 0 still counts as a scan
  RSLO_CHECK_LAUNCH("surfel_insert");
  return RSLO_OK;
}

extern "C" int rslo_surfel_insert_frames(void *map, size_t map_bytes, const void *store, size_t store_bytes,
                                         int64_t capacity, int K, const double *poses, int n_poses, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  const long long cap_max = sf_cap_of_bytes(map_bytes);
  return table_insert_frames<SurfView, SfFramesBody>(
      "surfel_insert_frames", "rslo_surfel_bytes", map, cap_max, store, store_bytes, capacity, K, poses, n_poses, s,
      [&](unsigned nb) { hipLaunchKernelGGL(k_surfel_derive_slots, dim3(nb), dim3(256), 0, s, map, cap_max); });
}

extern "C" int rslo_surfel_export(const void *map, size_t map_bytes, int min_flag, const double *center3, double radius,
                                  uint64_t *keys, int64_t *moments, double *rows, int64_t max_rows, int64_t *counts,
                                  void *stream) {
  hipStream_t s = (hipStream_t)stream;
  const long long cap_max = sf_cap_of_bytes(map_bytes);
  RSLO_CHECK_ARG(map && cap_max > 0, "surfel_export: no map (map_bytes below rslo_surfel_bytes(1024))");
  RSLO_CHECK_ARG(min_flag >= 0 && min_flag <= 2, "surfel_export: min_flag must be 0, 1 or 2");
  RSLO_CHECK_ARG(counts && max_rows >= 0, "surfel_export: counts is null or max_rows < 0");
  RSLO_CHECK_ARG(max_rows == 0 || (keys && moments && rows), "surfel_export: null output");
  RSLO_CHECK_ARG(!center3 || radius >= 0.0, "surfel_export: radius must be >= 0 (NaN is refused)");
  RSLO_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), s));
  const unsigned nb = table_blocks(cap_max);
  hipLaunchKernelGGL(k_surfel_export, dim3(nb), dim3(256), 0, s, (void *)map, cap_max, min_flag, center3, radius,
                     (map_u64 *)keys, (long long *)moments, rows, (long long)max_rows, (map_u64 *)counts);
  RSLO_CHECK_LAUNCH("surfel_export");
  return RSLO_OK;
}

extern "C" size_t rslo_surfel_prune_ws_bytes(int64_t capacity) {
  if (rslo_surfel_bytes(capacity) == 0) return 0;
  return (size_t)PRUNE_CTL_BYTES + (size_t)SF_STAGE_BYTES * (size_t)capacity;
}

extern "C" int rslo_surfel_prune(void *map, size_t map_bytes, const double *center3, double radius, double inner_radius,
                                 int min_count, void *ws, size_t ws_bytes, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  const long long cap_max = sf_cap_of_bytes(map_bytes);
  RSLO_CHECK_ARG(map && cap_max > 0, "surfel_prune: no map (map_bytes below rslo_surfel_bytes(1024))");
  RSLO_CHECK_ARG(!center3 || radius >= 0.0, "surfel_prune: radius must be >= 0 (NaN is refused)");
  RSLO_CHECK_ARG(!center3 || (inner_radius >= 0.0 && inner_radius <= radius),
                 "surfel_prune: need 0 <= inner_radius <= radius (NaN is refused)");
  RSLO_CHECK_ARG(min_count >= 1, "surfel_prune: min_count must be >= 1");
  RSLO_CHECK_ARG(ws && ((uintptr_t)ws & 15) == 0, "surfel_prune: the workspace is null or not 16-byte aligned");
  if (ws_bytes < rslo_surfel_prune_ws_bytes(cap_max)) {      // the header's capacity is at most cap_max
    rslo_set_error("surfel_prune: workspace too small");
    return RSLO_EWS;
  }
  const unsigned nb = table_blocks(cap_max);
  const long long scan_wg = cap_max / (256 * SF_PRUNE_STEP);      // a workgroup of the scan pass takes 2048 slots per step
  const unsigned nb_scan = (unsigned)(scan_wg < 1 ? 1 : (scan_wg < 256 ? scan_wg : 256));
  map_rebuild_begin(ws, s);
  hipLaunchKernelGGL(k_surfel_prune_scan, dim3(nb_scan), dim3(256), 0, s, map, cap_max, center3, radius, inner_radius,
                     min_count, ws);
  hipLaunchKernelGGL(k_surfel_prune_clear, dim3(nb), dim3(256), 0, s, map, cap_max, (const void *)ws);
  hipLaunchKernelGGL((k_table_reinsert<SurfView, SfRecords>), dim3(nb), dim3(256), 0, s, map, cap_max, ws);
  hipLaunchKernelGGL(k_surfel_prune_done, dim3(1), dim3(64), 0, s, map, cap_max, (const void *)ws);
  RSLO_CHECK_LAUNCH("surfel_prune");
  return RSLO_OK;
}

static int sf_check(const char *name, const void *map, long long cap_max, double voxel, int stride, int N,
                    const double *pose7, double max_dist) {
  return gn_check(name, "rslo_surfel_bytes", map, cap_max, voxel, stride, N, pose7, max_dist);
}

static int sf_check_dist(const char *name, int min_flag, double reg_rel, double reg_abs) {
  const double inf = (double)__builtin_inff();
  RSLO_CHECK_ARG(min_flag == 1 || min_flag == 2, "%s: min_flag must be 1 or 2", name);
  RSLO_CHECK_ARG(reg_rel >= 0.0 && reg_rel < inf && reg_abs >= 0.0 && reg_abs < inf && (reg_rel > 0.0 || reg_abs > 0.0),
                 "%s: reg_rel and reg_abs must be >= 0, finite and not both zero (NaN is refused)", name);
  return RSLO_OK;
}

extern "C" size_t rslo_surfel_register_ws_bytes(int N) { return N < 0 ? 0 : gn_ws_bytes(N); }

static int sf_check_sums(const char *name, const float *points, int N, double scale, void *ws, size_t ws_bytes) {
  RSLO_CHECK_ARG(gn_scale_ok(scale), "%s: " GN_SCALE_TEXT, name);
  return gn_check_ws(name, points, N, ws, ws_bytes);
}

// What the plane and the distribution calls share behind sf_check (and sf_check_dist): the remaining checks, the launches
template <bool PLANAR>
static int sf_nearest_call(const char *name, const void *map, long long cap_max, double voxel, const float *points,
                           int stride, int N, const double *pose7, double max_dist, const SfDist &dd, int64_t *keys_out,
                           double *d2_out, double *rows_out, double *info_out, void *stream) {
  if (N == 0) return RSLO_OK;
  RSLO_CHECK_ARG(points && keys_out && d2_out, "%s: null pointer", name);
  hipLaunchKernelGGL(k_surfel_nearest<PLANAR>, dim3((unsigned)rslo_cdiv(N, GN_BLOCK)), dim3(GN_BLOCK), 0, (hipStream_t)stream,
                     map, cap_max, voxel, points, stride, N, pose7, max_dist, dd, (long long *)keys_out, d2_out, rows_out,
                     info_out);
  RSLO_CHECK_LAUNCH(name);
  return RSLO_OK;
}

template <class Cost>
static int sf_normal_eq(const char *name, const Cost &cost, const float *points, int stride, int N, const double *pose7,
                        double max_dist, double scale, double *out29, void *ws, size_t ws_bytes, void *stream) {
  RSLO_CHECK_ARG(out29, "%s: out29 is null", name);
  const int rc = sf_check_sums(name, points, N, scale, ws, ws_bytes);
  if (rc) return rc;
  gn_normal_eq(cost, points, stride, N, pose7, max_dist, scale, out29, ws, (hipStream_t)stream);
  RSLO_CHECK_LAUNCH(name);
  return RSLO_OK;
}

template <class Cost>
static int sf_register(const char *name, const Cost &cost, const float *points, int stride, int N, double *pose7, int iters,
                       double max_dist, double damping, int min_pairs, double tol_t, double tol_r, double scale,
                       double *info, void *ws, size_t ws_bytes, void *stream) {
  int rc = gn_check_iters(name, iters, tol_t, tol_r);
  if (rc) return rc;
  RSLO_CHECK_ARG(info, "%s: info is null", name);
  rc = sf_check_sums(name, points, N, scale, ws, ws_bytes);
  if (rc) return rc;
  const GnSolve sp = {min_pairs, damping, tol_t, tol_r, 0, 0.0, 0.0};
  gn_iterate(cost, points, stride, N, pose7, iters, max_dist, scale, sp, info, ws, (hipStream_t)stream);
  RSLO_CHECK_LAUNCH(name);
  return RSLO_OK;
}

extern "C" int rslo_surfel_nearest(const void *map, size_t map_bytes, double voxel_size, const float *points,
                                   int stride_floats, int N, const double *pose7, double max_dist, int64_t *keys_out,
                                   double *d2_out, double *rows_out, void *stream) {
  const char *name = "surfel_nearest";
  const long long cap_max = sf_cap_of_bytes(map_bytes);
  const int rc = sf_check(name, map, cap_max, voxel_size, stride_floats, N, pose7, max_dist);
  if (rc) return rc;
  return sf_nearest_call<true>(name, map, cap_max, voxel_size, points, stride_floats, N, pose7, max_dist, SfDist{2.0, 0.0, 0.0},
                               keys_out, d2_out, rows_out, nullptr, stream);
}

extern "C" int rslo_surfel_normal_eq(const void *map, size_t map_bytes, double voxel_size, const float *points,
                                     int stride_floats, int N, const double *pose7, double max_dist, double robust_scale,
                                     double *out29, void *ws, size_t ws_bytes, void *stream) {
  const char *name = "surfel_normal_eq";
  const SfPlaneCost cost = {map, sf_cap_of_bytes(map_bytes), voxel_size};
  const int rc = sf_check(name, map, cost.cap_max, voxel_size, stride_floats, N, pose7, max_dist);
  if (rc) return rc;
  return sf_normal_eq(name, cost, points, stride_floats, N, pose7, max_dist, robust_scale, out29, ws, ws_bytes, stream);
}

extern "C" int rslo_surfel_register(const void *map, size_t map_bytes, double voxel_size, const float *points,
                                    int stride_floats, int N, double *pose7, int iters, double max_dist, double damping,
                                    int min_pairs, double tol_t, double tol_r, double robust_scale, double *info, void *ws,
                                    size_t ws_bytes, void *stream) {
  const char *name = "surfel_register";
  const SfPlaneCost cost = {map, sf_cap_of_bytes(map_bytes), voxel_size};
  const int rc = sf_check(name, map, cost.cap_max, voxel_size, stride_floats, N, pose7, max_dist);
  if (rc) return rc;
  return sf_register(name, cost, points, stride_floats, N, pose7, iters, max_dist, damping, min_pairs, tol_t, tol_r,
                     robust_scale, info, ws, ws_bytes, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// Distribution cost: the three calls above with candidates of flag >= min_flag and the cell's information matrix
// ---------------------------------------------------------------------------------------------------------------------
extern "C" int rslo_surfel_nearest_d(const void *map, size_t map_bytes, double voxel_size, const float *points,
                                     int stride_floats, int N, const double *pose7, double max_dist, int min_flag,
                                     double reg_rel, double reg_abs, int64_t *keys_out, double *d2_out, double *rows_out,
                                     double *info_out, void *stream) {
  const char *name = "surfel_nearest_d";
  const long long cap_max = sf_cap_of_bytes(map_bytes);
  int rc = sf_check(name, map, cap_max, voxel_size, stride_floats, N, pose7, max_dist);
  if (rc) return rc;
  rc = sf_check_dist(name, min_flag, reg_rel, reg_abs);
  if (rc) return rc;
  return sf_nearest_call<false>(name, map, cap_max, voxel_size, points, stride_floats, N, pose7, max_dist,
                                SfDist{(double)min_flag, reg_rel, reg_abs}, keys_out, d2_out, rows_out, info_out, stream);
}

extern "C" int rslo_surfel_normal_eq_d(const void *map, size_t map_bytes, double voxel_size, const float *points,
                                       int stride_floats, int N, const double *pose7, double max_dist, int min_flag,
                                       double reg_rel, double reg_abs, double robust_scale, double *out29, void *ws,
                                       size_t ws_bytes, void *stream) {
  const char *name = "surfel_normal_eq_d";
  const SfDistCost cost = {map, sf_cap_of_bytes(map_bytes), voxel_size, {(double)min_flag, reg_rel, reg_abs}};
  int rc = sf_check(name, map, cost.cap_max, voxel_size, stride_floats, N, pose7, max_dist);
  if (rc) return rc;
  rc = sf_check_dist(name, min_flag, reg_rel, reg_abs);
  if (rc) return rc;
  return sf_normal_eq(name, cost, points, stride_floats, N, pose7, max_dist, robust_scale, out29, ws, ws_bytes, stream);
}

extern "C" int rslo_surfel_register_d(const void *map, size_t map_bytes, double voxel_size, const float *points,
                                      int stride_floats, int N, double *pose7, int iters, double max_dist, double damping,
                                      int min_pairs, double tol_t, double tol_r, double robust_scale, int min_flag,
                                      double reg_rel, double reg_abs, double *info, void *ws, size_t ws_bytes, void *stream) {
  const char *name = "surfel_register_d";
  const SfDistCost cost = {map, sf_cap_of_bytes(map_bytes), voxel_size, {(double)min_flag, reg_rel, reg_abs}};
  int rc = sf_check(name, map, cost.cap_max, voxel_size, stride_floats, N, pose7, max_dist);
  if (rc) return rc;
  rc = sf_check_dist(name, min_flag, reg_rel, reg_abs);
  if (rc) return rc;
  return sf_register(name, cost, points, stride_floats, N, pose7, iters, max_dist, damping, min_pairs, tol_t, tol_r,
                     robust_scale, info, ws, ws_bytes, stream);
}
