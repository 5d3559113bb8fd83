// World voxel map of a streamed trajectory: a persistent, incrementally filled voxel hash in the frame of scan 0
// (rules: include/rslo_hip.h "World voxel map"; float64 restatement: rslo_amd/mapping.py VoxelMapRef).  Nothing of the
// reference corresponds to it: evaluate.py:363-408 writes poses only.
//
// One caller-owned allocation: header (256 bytes) | keys u64 [cap] | tags u64 [cap] | rows f32 [cap, 4] | hits i32 [cap].
// Open addressing, linear probing from a 64-bit mix of the key, at most RSLO_MAP_MAX_PROBE slots examined: no loop here
// depends on the table having room.  Between two prunes slots only fill and keys never move; rslo_map_prune (below)
// is the one call that removes cells, and it does so by REBUILDING the table in launches of its own.
//
// Visibility (eight XCDs with separate L2s): inside the insert kernel every decision rests on the return value of an
// atomic (atomicCAS on the key, atomicMin on the tag, atomicAdd on the hits).  The non-temporal pre-reads only skip an
// atomic that cannot change anything: inside that kernel a key never changes once set, so a stale read can only show
// "empty" (then the CAS decides); a tag only decreases, so a stale read can only be too large (then the atomicMin is
// issued needlessly).  The row of a new cell is written by the owner of its tag in the NEXT kernel of the call (slot
// kept in the workspace), the scan counter is bumped by a third kernel after every reader of it has run.
// rslo_map_insert_frames keeps that order for many scans at once: its second kernel walks the slots and finds the owner
// in the tag itself, so it needs no workspace.
// Keys DO change in a prune, but only in prune's own launches, each of which is a kernel boundary away from every other
// user of the table: one launch reads the table and stages the kept records (the cursor is an atomic whose return value
// is the record's place), the next empties every slot, the next re-inserts the staged records -- there, again, a key
// only goes from empty to set, by atomicCAS, and the CAS winner alone writes tag / row / hits of its slot -- and the
// last one writes the header.  Nothing here communicates across workgroups except through atomics and kernel
// boundaries.
#include "rslo_common.h"

#include <cstddef>

#include "map_table.h"

#pragma clang fp contract(off)   /* the cell of a point must not depend on FMA formation */

#include "map_core.h"            /* the table's write side, shared with csrc/surfel.hip; the rebuild rslo_map_carve shares */

// filled in one launch: the header by thread 0, the sections by everybody
__global__ __launch_bounds__(256) void k_map_reset(void *map, long long cap, double voxel, double min_range,
                                                   double max_range) {
  unsigned char *p = (unsigned char *)map + MAP_HDR_BYTES;
  map_u64 *keys = (map_u64 *)p, *tags = (map_u64 *)(p + (size_t)cap * 8);
  float4 *rows = (float4 *)(p + (size_t)cap * 16);
  int32_t *hits = (int32_t *)(p + (size_t)cap * 32);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    MapHdr *h = (MapHdr *)map;
    h->magic = MAP_MAGIC;
    h->capacity = cap;
    h->voxel = voxel;
    h->min_range = min_range;
    h->max_range = max_range;
    h->n_prunes = h->n_evicted = h->n_lost = 0;
    h->n_carves = h->n_carved = 0;
    h->n_scans = h->n_cells = h->n_points = h->dropped_invalid = h->dropped_range = h->dropped_full = 0;
  }
  for (long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x; s < cap; s += (long long)gridDim.x * blockDim.x) {
    keys[s] = MAP_KEY_NONE;
    tags[s] = MAP_KEY_NONE;
    rows[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    hits[s] = 0;
  }
}

// Point i of scan number `scan` (p: its x, y, z) under `pose` into the table: the slot's key, tag and hits, and the
// five counters n_cells .. dropped_full of `c` -- the map's header itself (rslo_map_insert), or a workgroup's tally in
// LDS that is added to the header once (rslo_map_insert_frames).  -> the slot, or -1 for a point that was dropped.
// The one insert of both calls; the probe is table_slot's (map_core.h).
template <class Counters>
__device__ __forceinline__ int32_t map_put(const MapView &m, Counters *c, const float *__restrict__ p,
                                           const double *__restrict__ pose, map_u64 scan, uint32_t i) {
  double w[3];
  const int32_t s = table_slot(m, c, p, pose, w);
  if (s < 0) return -1;
  const map_u64 tag = (scan << 32) | (map_u64)i;
  if (__builtin_nontemporal_load(&m.tags[s]) > tag) atomicMin(&m.tags[s], tag);
  atomicAdd(&m.hits[s], 1);
  atomicAdd(&c->n_points, (map_u64)1);
  return s;
}

__global__ __launch_bounds__(256) void k_map_insert(void *map, long long cap_max, const float *__restrict__ points,
                                                    int stride, int N, const double *__restrict__ pose,
                                                    int32_t *__restrict__ slot_of) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  MapView m;
  if (!map_view(map, cap_max, m)) {
    slot_of[i] = -1;
    return;
  }
  slot_of[i] = map_put(m, m.hdr, points + (int64_t)i * stride, pose, m.hdr->n_scans, (uint32_t)i);
}

// behind the kernel boundary the tags are final for this scan: the owner of a cell's tag writes its row
__global__ __launch_bounds__(256) void k_map_rows(void *map, long long cap_max, const float *__restrict__ points,
                                                  int stride, int width, int N, const double *__restrict__ pose,
                                                  const int32_t *__restrict__ slot_of) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int32_t s = slot_of[i];
  MapView m;
  if (s < 0 || !map_view(map, cap_max, m)) return;
  const map_u64 tag = (m.hdr->n_scans << 32) | (map_u64)(uint32_t)i;
  if (m.tags[s] != tag) return;
  const float *p = points + (int64_t)i * stride;
  map_u64 key;
  double w[3];
  if (map_point(p, pose, m.hdr->voxel, m.hdr->min_range, m.hdr->max_range, key, w)) return;
  *(float4 *)(m.rows + (size_t)s * 4) = make_float4((float)w[0], (float)w[1], (float)w[2], width >= 4 ? p[3] : 0.f);
}

// ---------------------------------------------------------------------------------------------------------------------
// rslo_map_insert_frames: every frame of a keyframe store under its own pose, as n successive inserts would leave the
// map (rules: include/rslo_hip.h "World voxel map").  Three launches whatever the data, no workspace.
// ---------------------------------------------------------------------------------------------------------------------
// pass 1 is k_table_frames_points (map_core.h) with this body: a valid point is put, the other lanes have nothing to do.
// Pass 3, k_table_frames_done, is map_core.h's as well; table_insert_frames launches the three.
struct MapFramesBody {
  static __device__ __forceinline__ void point(const MapView &m, InsertTally *tally, bool valid, const float *p,
                                               const double *pose, map_u64 scan, uint32_t i) {
    if (valid) map_put(m, tally, p, pose, scan, i);
  }
};

// pass 2, over the SLOTS: behind the kernel boundary the tags are final.  A tag whose scan number lies in
// [n_scans, n_scans + n) was set by pass 1 (older cells carry smaller scan numbers and are never re-owned) and names
// the point that owns the cell: frame (tag >> 32) - n_scans, row tag & 0xffffffff.  Its world position is recomputed
// from the store by the same function that chose its cell.
__global__ __launch_bounds__(256) void k_map_frames_rows(void *map, long long cap_max, void *store, size_t store_bytes,
                                                         long long kf_cap, int K, const double *__restrict__ poses,
                                                         int n_poses) {
  MapView m;
  KfView v;
  if (!map_view(map, cap_max, m) || !kf_view(store, store_bytes, kf_cap, K, v)) return;
  const map_u64 n = (map_u64)table_frames_n(v, n_poses), s0 = m.hdr->n_scans;
  const long long cap = m.hdr->capacity;
  for (long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x; s < cap; s += (long long)gridDim.x * blockDim.x) {
    if (m.keys[s] == MAP_KEY_NONE) continue;
    const map_u64 tag = m.tags[s];
    const map_u64 scan = tag >> 32, i = tag & 0xffffffffull;
    if (scan < s0 || scan - s0 >= n || i >= (map_u64)K) continue;      // (tag all-ones: a scan number no call reaches)
    const map_u64 e = scan - s0;
    const float4 r = *(const float4 *)(v.rows + ((size_t)e * K + i) * 4);
    const float p[3] = {r.x, r.y, r.z};
    map_u64 key;
    double w[3];
    if (map_point(p, poses + (size_t)e * 7, m.hdr->voxel, m.hdr->min_range, m.hdr->max_range, key, w)) continue;
    *(float4 *)(m.rows + (size_t)s * 4) = make_float4((float)w[0], (float)w[1], (float)w[2], r.w);
  }
}

__global__ __launch_bounds__(256) void k_map_lookup(void *map, long long cap_max, const float *__restrict__ points,
                                                    int stride, int N, const double *__restrict__ pose,
                                                    int32_t *__restrict__ hits_out, map_u64 *__restrict__ tags_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  MapView m;
  int32_t h = -1;
  map_u64 tag = MAP_KEY_NONE;
  map_u64 key;
  double w[3];
  if (map_view(map, cap_max, m) &&
      !map_point(points + (int64_t)i * stride, pose, m.hdr->voxel, m.hdr->min_range, m.hdr->max_range, key, w)) {
    const map_u64 mask = (map_u64)m.hdr->capacity - 1;
    map_u64 s = map_mix(key) & mask;
    h = 0;
    for (int probe = 0; probe < RSLO_MAP_MAX_PROBE; ++probe) {
      const map_u64 k = m.keys[s];
      if (k == key) {
        h = m.hits[s];
        tag = m.tags[s];
        break;
      }
      if (k == MAP_KEY_NONE) break;
      s = (s + 1) & mask;
    }
  }
  hits_out[i] = h;
  if (tags_out) tags_out[i] = tag;
}

__global__ __launch_bounds__(256) void k_map_export(void *map, long long cap_max, int min_hits,
                                                    const double *__restrict__ center, double radius,
                                                    float *__restrict__ rows, map_u64 *__restrict__ tags,
                                                    int32_t *__restrict__ hits, long long max_rows,
                                                    map_u64 *__restrict__ counts) {
  MapView m;
  if (!map_view(map, cap_max, m)) return;
  const long long cap = m.hdr->capacity;
  for (long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x; s < cap; s += (long long)gridDim.x * blockDim.x) {
    if (m.keys[s] == MAP_KEY_NONE) continue;
    const int32_t h = m.hits[s];
    if (h < min_hits) continue;
    const float4 r = *(const float4 *)(m.rows + (size_t)s * 4);
    if (center) {
      const double dx = (double)r.x - center[0], dy = (double)r.y - center[1], dz = (double)r.z - center[2];
      if (!(dx * dx + dy * dy + dz * dz < radius * radius)) continue;
    }
    const map_u64 o = atomicAdd(&counts[0], (map_u64)1);
    if ((long long)o < max_rows) {
      atomicAdd(&counts[1], (map_u64)1);
      *(float4 *)(rows + (size_t)o * 4) = r;
      tags[o] = m.tags[s];
      hits[o] = h;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// rslo_map_prune: evict far and sparse cells by rebuilding the table (rules: include/rslo_hip.h "Rolling local map").
// Workspace: control block (256 bytes, zeroed by the first, one-thread launch) | staged keys u64 [cap] |
// tags u64 [cap] | rows f32 [cap, 4] | hits i32 [cap] -- the map's own section layout (map_core.h).
// ---------------------------------------------------------------------------------------------------------------------
// the control block starts every call at zero
__global__ void k_table_rebuild_begin(void *ws) {
  if (threadIdx.x == 0) {
    RebuildCtl *ctl = (RebuildCtl *)ws;
    ctl->kept = ctl->evicted = ctl->lost = ctl->planar = 0;
  }
}

// pass 1: keep or evict every stored cell; the kept records go to the staging area through one cursor
__global__ __launch_bounds__(256) void k_map_prune_scan(void *map, long long cap_max, const double *__restrict__ center,
                                                        double radius, int min_hits, int grace, void *ws) {
  MapView m;
  if (!map_view(map, cap_max, m)) return;
  const long long cap = m.hdr->capacity;
  const PruneStage st = prune_stage(ws, cap);
  const long long last_scan = (long long)m.hdr->n_scans - 1;
  double c[3] = {0.0, 0.0, 0.0};
  if (center) c[0] = center[0], c[1] = center[1], c[2] = center[2];
  for (long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x; s < cap; s += (long long)gridDim.x * blockDim.x) {
    const map_u64 key = m.keys[s];
    if (key == MAP_KEY_NONE) continue;
    const int32_t h = m.hits[s];
    const map_u64 tag = m.tags[s];
    const float4 r = *(const float4 *)(m.rows + (size_t)s * 4);
    bool keep = h >= min_hits || last_scan - (long long)(tag >> 32) < (long long)grace;
    if (center) {      // the test of k_map_export, character for character: a comparison that is false evicts
      const double dx = (double)r.x - c[0], dy = (double)r.y - c[1], dz = (double)r.z - c[2];
      if (!(dx * dx + dy * dy + dz * dz < radius * radius)) keep = false;
    }
    // both adds to ONE address each, the first by every lane of an occupied slot (see k_map_insert): one add per wave
    atomicAdd(&st.ctl->evicted, (map_u64)(!keep));
    if (keep) {
      const map_u64 o = atomicAdd(&st.ctl->kept, (map_u64)1);
      if (o < (map_u64)cap) {      // always: one record per slot at most, and the cursor starts at 0
        st.keys[o] = key;
        st.tags[o] = tag;
        st.rows[o] = r;
        st.hits[o] = h;
      }
    }
  }
}

// pass 2: the state k_map_reset leaves in the sections.  Nothing evicted: the table stays as it is, to the byte.
__global__ __launch_bounds__(256) void k_map_prune_clear(void *map, long long cap_max, const void *ws) {
  MapView m;
  if (!map_view(map, cap_max, m)) return;
  if (((const RebuildCtl *)ws)->evicted == 0) return;
  const long long cap = m.hdr->capacity;
  for (long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x; s < cap; s += (long long)gridDim.x * blockDim.x) {
    m.keys[s] = MAP_KEY_NONE;
    m.tags[s] = MAP_KEY_NONE;
    *(float4 *)(m.rows + (size_t)s * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
    m.hits[s] = 0;
  }
}

// pass 3 is k_table_reinsert (map_core.h) over these records: the CAS winner alone writes tag / row / hits of its slot
struct MapRecords {
  static __device__ __forceinline__ PruneStage stage(void *ws, long long cap) { return prune_stage(ws, cap); }
  static __device__ __forceinline__ unsigned put(const MapView &m, const PruneStage &st, size_t i, size_t s) {
    m.tags[s] = st.tags[i];
    *(float4 *)(m.rows + s * 4) = st.rows[i];
    m.hits[s] = st.hits[i];
    return 0;
  }
};

__global__ void k_map_prune_done(void *map, long long cap_max, const void *ws) {
  MapView m;
  if (threadIdx.x != 0 || !map_view(map, cap_max, m)) return;
  const RebuildCtl *ctl = (const RebuildCtl *)ws;
  m.hdr->n_prunes = m.hdr->n_prunes + 1;
  if (ctl->evicted == 0) return;
  m.hdr->n_cells = ctl->kept - ctl->lost;
  m.hdr->n_evicted = m.hdr->n_evicted + ctl->evicted;
  m.hdr->n_lost = m.hdr->n_lost + ctl->lost;
}

extern "C" size_t rslo_map_bytes(int64_t capacity) {
  if (capacity < MAP_MIN_CAP || capacity > ((int64_t)1 << 31) || (capacity & (capacity - 1))) return 0;
  return (size_t)MAP_HDR_BYTES + (size_t)MAP_SLOT_BYTES * (size_t)capacity;
}

extern "C" int rslo_map_reset(void *map, size_t map_bytes, int64_t capacity, double voxel_size, double min_range,
                              double max_range, void *stream) {
  RSLO_CHECK_ARG(map, "map_reset: map is null");
  RSLO_CHECK_ARG(rslo_map_bytes(capacity) != 0, "map_reset: capacity must be a power of two in 1024 .. 2^31");
  RSLO_CHECK_ARG(map_bytes >= rslo_map_bytes(capacity), "map_reset: map_bytes is smaller than rslo_map_bytes(capacity)");
  RSLO_CHECK_ARG(voxel_size > 0.0 && voxel_size < (double)__builtin_inff(),
                 "map_reset: voxel_size must be positive and finite");
  RSLO_CHECK_ARG(min_range >= 0.0 && min_range < max_range, "map_reset: need 0 <= min_range < max_range");
  const unsigned nb = (unsigned)(capacity / 256 < 4096 ? capacity / 256 : 4096);
  hipLaunchKernelGGL(k_map_reset, dim3(nb), dim3(256), 0, (hipStream_t)stream, map, (long long)capacity, voxel_size,
                     min_range, max_range);
  RSLO_CHECK_LAUNCH("map_reset");
  return RSLO_OK;
}

extern "C" size_t rslo_map_insert_ws_bytes(int N) { return 256 + (N > 0 ? ((size_t)N * 4 + 255) / 256 * 256 : 0); }

extern "C" int rslo_map_insert(void *map, size_t map_bytes, const float *points, int stride_floats, int width, int N,
                               const double *pose7, void *ws, size_t ws_bytes, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  const long long cap_max = map_cap_of_bytes(map_bytes);
  RSLO_CHECK_ARG(map && cap_max > 0, "map_insert: no map (map_bytes below rslo_map_bytes(1024))");
  RSLO_CHECK_ARG(N >= 0, "map_insert: N < 0");
  RSLO_CHECK_ARG(stride_floats >= 3 && width >= 3 && (width < 4 || stride_floats >= 4),
                 "map_insert: stride_floats and width must be >= 3 (>= 4 to read an intensity)");
  RSLO_CHECK_ARG(pose7, "map_insert: pose7 is null");
  if (N > 0) {
    RSLO_CHECK_ARG(points && ws, "map_insert: null pointer");
    if (ws_bytes < rslo_map_insert_ws_bytes(N)) {
      rslo_set_error("map_insert: workspace too small");
      return RSLO_EWS;
    }
    int32_t *slot_of = table_slot_of(ws);
    const unsigned nb = (unsigned)rslo_cdiv(N, 256);
    hipLaunchKernelGGL(k_map_insert, dim3(nb), dim3(256), 0, s, map, cap_max, points, stride_floats, N, pose7, slot_of);
    hipLaunchKernelGGL(k_map_rows, dim3(nb), dim3(256), 0, s, map, cap_max, points, stride_floats, width, N, pose7,
                       (const int32_t *)slot_of);
  }
  hipLaunchKernelGGL(k_table_scan_done<MapView>, dim3(1), dim3(64), 0, s, map, cap_max);      // N == 0 still counts as a scan
  RSLO_CHECK_LAUNCH("map_insert");
  return RSLO_OK;
}

extern "C" int rslo_map_insert_frames(void *map, size_t map_bytes, const void *store, size_t store_bytes, int64_t capacity,
                                      int K, const double *poses, int n_poses, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  const long long cap_max = map_cap_of_bytes(map_bytes);
  return table_insert_frames<MapView, MapFramesBody>(
      "map_insert_frames", "rslo_map_bytes", map, cap_max, store, store_bytes, capacity, K, poses, n_poses, s, [&](unsigned nb) {
        hipLaunchKernelGGL(k_map_frames_rows, dim3(nb), dim3(256), 0, s, map, cap_max, (void *)store, store_bytes,
                           (long long)capacity, K, poses, n_poses);
      });
}

extern "C" int rslo_map_lookup(const void *map, size_t map_bytes, const float *points, int stride_floats, int N,
                               const double *pose7, int32_t *hits_out, uint64_t *tags_out, void *stream) {
  const long long cap_max = map_cap_of_bytes(map_bytes);
  RSLO_CHECK_ARG(map && cap_max > 0, "map_lookup: no map (map_bytes below rslo_map_bytes(1024))");
  RSLO_CHECK_ARG(N >= 0 && stride_floats >= 3, "map_lookup: N < 0 or stride_floats < 3");
  RSLO_CHECK_ARG(pose7, "map_lookup: pose7 is null");
  if (N == 0) return RSLO_OK;
  RSLO_CHECK_ARG(points && hits_out, "map_lookup: null pointer");
  hipLaunchKernelGGL(k_map_lookup, dim3((unsigned)rslo_cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, (void *)map,
                     cap_max, points, stride_floats, N, pose7, hits_out, (map_u64 *)tags_out);
  RSLO_CHECK_LAUNCH("map_lookup");
  return RSLO_OK;
}

extern "C" int rslo_map_export(const void *map, size_t map_bytes, int min_hits, const double *center3, double radius,
                               float *rows, uint64_t *tags, int32_t *hits, int64_t max_rows, int64_t *counts,
                               void *stream) {
  hipStream_t s = (hipStream_t)stream;
  const long long cap_max = map_cap_of_bytes(map_bytes);
  RSLO_CHECK_ARG(map && cap_max > 0, "map_export: no map (map_bytes below rslo_map_bytes(1024))");
  RSLO_CHECK_ARG(counts && max_rows >= 0, "map_export: counts is null or max_rows < 0");
  RSLO_CHECK_ARG(max_rows == 0 || (rows && tags && hits), "map_export: null output");
  RSLO_CHECK_ARG(!center3 || radius >= 0.0, "map_export: radius must be >= 0 (NaN is refused)");
  RSLO_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), s));
  const unsigned nb = table_blocks(cap_max);
  hipLaunchKernelGGL(k_map_export, dim3(nb), dim3(256), 0, s, (void *)map, cap_max, min_hits, center3, radius, rows,
                     (map_u64 *)tags, hits, (long long)max_rows, (map_u64 *)counts);
  RSLO_CHECK_LAUNCH("map_export");
  return RSLO_OK;
}

// the launches of a rebuild that do not depend on who removes the cells (map_core.h)
void map_rebuild_begin(void *ws, hipStream_t s) { hipLaunchKernelGGL(k_table_rebuild_begin, dim3(1), dim3(64), 0, s, ws); }

void map_rebuild_table(void *map, long long cap_max, void *ws, hipStream_t s) {
  const unsigned nb = table_blocks(cap_max);
  hipLaunchKernelGGL(k_map_prune_clear, dim3(nb), dim3(256), 0, s, map, cap_max, (const void *)ws);
  hipLaunchKernelGGL((k_table_reinsert<MapView, MapRecords>), dim3(nb), dim3(256), 0, s, map, cap_max, ws);
}

extern "C" size_t rslo_map_prune_ws_bytes(int64_t capacity) {
  if (rslo_map_bytes(capacity) == 0) return 0;
  return (size_t)PRUNE_CTL_BYTES + (size_t)MAP_SLOT_BYTES * (size_t)capacity;
}

extern "C" int rslo_map_prune(void *map, size_t map_bytes, const double *center3, double radius, int min_hits, int grace,
                              void *ws, size_t ws_bytes, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  const long long cap_max = map_cap_of_bytes(map_bytes);
  RSLO_CHECK_ARG(map && cap_max > 0, "map_prune: no map (map_bytes below rslo_map_bytes(1024))");
  RSLO_CHECK_ARG(!center3 || radius >= 0.0, "map_prune: radius must be >= 0 (NaN is refused)");
  RSLO_CHECK_ARG(min_hits >= 1 && grace >= 0, "map_prune: need min_hits >= 1 and grace >= 0");
  RSLO_CHECK_ARG(ws && ((uintptr_t)ws & 15) == 0, "map_prune: the workspace is null or not 16-byte aligned");
  if (ws_bytes < rslo_map_prune_ws_bytes(cap_max)) {      // the header's capacity is at most cap_max
    rslo_set_error("map_prune: workspace too small");
    return RSLO_EWS;
  }
  const unsigned nb = table_blocks(cap_max);
  map_rebuild_begin(ws, s);
  hipLaunchKernelGGL(k_map_prune_scan, dim3(nb), dim3(256), 0, s, map, cap_max, center3, radius, min_hits, grace, ws);
  map_rebuild_table(map, cap_max, ws, s);
  hipLaunchKernelGGL(k_map_prune_done, dim3(1), dim3(64), 0, s, map, cap_max, (const void *)ws);
  RSLO_CHECK_LAUNCH("map_prune");
  return RSLO_OK;
}
