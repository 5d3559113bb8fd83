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
#include "map_rebuild.h"         /* the staging area and the rebuild launches rslo_map_carve shares (csrc/carve.hip) */
#include "kf_store.h"            /* rslo_map_insert_frames reads a keyframe store */

#pragma clang fp contract(off)   /* the cell of a point must not depend on FMA formation */

#define MAP_FRAMES_BLOCKS 2048u          /* workgroups of rslo_map_insert_frames' points pass: eight per CU */

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
// The one insert of both calls.
template <class Counters>
__device__ __forceinline__ int32_t map_put(const MapView &m, Counters *c, const float *__restrict__ p,
                                           const double *__restrict__ pose, map_u64 scan, uint32_t i) {
  map_u64 key;
  double w[3];
  const int why = map_point(p, pose, m.hdr->voxel, m.hdr->min_range, m.hdr->max_range, key, w);
  if (why) {
    // both adds by every dropped lane, each to ONE address: the compiler then folds an add into one per wave.  (Given
    // `if (why == 1) add(a, 1); else add(b, 1);` it merges the two into one add whose address differs per lane, which
    // is issued lane by lane: 1.4 ms for a scan whose points are all dropped.)
    atomicAdd(&c->dropped_invalid, (map_u64)(why == 1));
    atomicAdd(&c->dropped_range, (map_u64)(why == 2));
    return -1;
  }
  const map_u64 mask = (map_u64)m.hdr->capacity - 1;
  map_u64 s = map_mix(key) & mask;
  int found = 0;
  for (int probe = 0; probe < RSLO_MAP_MAX_PROBE; ++probe) {
    map_u64 prev = __builtin_nontemporal_load(&m.keys[s]);
    if (prev == MAP_KEY_NONE) {
      prev = atomicCAS(&m.keys[s], MAP_KEY_NONE, key);
      if (prev == MAP_KEY_NONE) {
        atomicAdd(&c->n_cells, (map_u64)1);
        prev = key;
      }
    }
    if (prev == key) {
      found = 1;
      break;
    }
    s = (s + 1) & mask;
  }
  if (!found) {
    atomicAdd(&c->dropped_full, (map_u64)1);
    return -1;
  }
  const map_u64 tag = (scan << 32) | (map_u64)i;
  if (__builtin_nontemporal_load(&m.tags[s]) > tag) atomicMin(&m.tags[s], tag);
  atomicAdd(&m.hits[s], 1);
  atomicAdd(&c->n_points, (map_u64)1);
  return (int32_t)s;      // capacity <= 2^31 slots (rslo_map_bytes)
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

__global__ void k_map_scan_done(void *map, long long cap_max) {
  MapView m;
  if (threadIdx.x == 0 && map_view(map, cap_max, m)) m.hdr->n_scans = m.hdr->n_scans + 1;
}

// ---------------------------------------------------------------------------------------------------------------------
// rslo_map_insert_frames: every frame of a keyframe store under its own pose, as n successive inserts would leave the
// map (rules: include/rslo_hip.h "World voxel map").  Three launches whatever the data, no workspace.
// ---------------------------------------------------------------------------------------------------------------------
// n = min(the store's entry count, read here and held to the store's capacity; n_poses)
__device__ __forceinline__ long long map_frames_n(const KfView &v, int n_poses) {
  long long n = v.hdr->n_entries;
  n = n < 0 ? 0 : (n > v.hdr->capacity ? v.hdr->capacity : n);
  return n < (long long)n_poses ? n : (long long)n_poses;
}

// the five header counters an insert adds to, in the header's order (n_cells .. dropped_full)
struct MapTally {
  map_u64 n_cells, n_points, dropped_invalid, dropped_range, dropped_full;
};
static_assert(offsetof(MapHdr, n_points) == offsetof(MapHdr, n_cells) + 8 &&
              offsetof(MapHdr, dropped_invalid) == offsetof(MapHdr, n_cells) + 16 &&
              offsetof(MapHdr, dropped_range) == offsetof(MapHdr, n_cells) + 24 &&
              offsetof(MapHdr, dropped_full) == offsetof(MapHdr, n_cells) + 32, "MapTally mirrors the header's counters");

// pass 1: one thread per (frame, row) in tiles of 256 rows, bpf tiles per frame; frame, pose and count are uniform over
// a tile.  A workgroup takes tiles blockIdx.x, blockIdx.x + gridDim.x, ... and counts in LDS: with the header as the
// sink every WAVE would add to the same few words, and adds to one address are served one after the other on the
// memory side -- measured at 0.8 us per wave, 45 ms for 4096 frames -- so the header gets one add per workgroup and
// non-zero counter.  The scan number of frame e is n_scans + e: the header's n_scans does not change before pass 3.
__global__ __launch_bounds__(256) void k_map_frames_points(void *map, long long cap_max, void *store, size_t store_bytes,
                                                           long long kf_cap, int K, const double *__restrict__ poses,
                                                           int n_poses, int bpf) {
  __shared__ MapTally tally;
  if (threadIdx.x < 5) ((map_u64 *)&tally)[threadIdx.x] = 0;
  __syncthreads();
  MapView m;
  KfView v;
  if (!map_view(map, cap_max, m) || !kf_view(store, store_bytes, kf_cap, K, v)) return;      // uniform over the grid
  const long long tiles = map_frames_n(v, n_poses) * bpf;
  const map_u64 s0 = m.hdr->n_scans;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long e = tile / bpf;
    const int i = (int)(tile % bpf) * 256 + (int)threadIdx.x;
    int count = v.counts[e];
    count = count < 0 ? 0 : (count > K ? K : count);
    if (i >= count) continue;
    const float4 r = *(const float4 *)(v.rows + ((size_t)e * K + i) * 4);
    const float p[3] = {r.x, r.y, r.z};
    map_put(m, &tally, p, poses + (size_t)e * 7, s0 + (map_u64)e, (uint32_t)i);
  }
  __syncthreads();
  if (threadIdx.x < 5) {
    const map_u64 add = ((map_u64 *)&tally)[threadIdx.x];
    if (add) atomicAdd(&m.hdr->n_cells + threadIdx.x, add);
  }
}

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
  const map_u64 n = (map_u64)map_frames_n(v, n_poses), s0 = m.hdr->n_scans;
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

// pass 3: an empty frame still counts as a scan
__global__ void k_map_frames_done(void *map, long long cap_max, void *store, size_t store_bytes, long long kf_cap, int K,
                                  int n_poses) {
  MapView m;
  KfView v;
  if (threadIdx.x != 0 || !map_view(map, cap_max, m) || !kf_view(store, store_bytes, kf_cap, K, v)) return;
  m.hdr->n_scans = m.hdr->n_scans + (map_u64)map_frames_n(v, n_poses);
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
// tags u64 [cap] | rows f32 [cap, 4] | hits i32 [cap] -- the map's own section layout (map_rebuild.h).
// ---------------------------------------------------------------------------------------------------------------------
// the control block starts every call at zero
__global__ void k_map_prune_begin(void *ws) {
  if (threadIdx.x == 0) {
    PruneCtl *ctl = (PruneCtl *)ws;
    ctl->kept = ctl->evicted = ctl->lost = 0;
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
  if (((const PruneCtl *)ws)->evicted == 0) return;
  const long long cap = m.hdr->capacity;
  for (long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x; s < cap; s += (long long)gridDim.x * blockDim.x) {
    m.keys[s] = MAP_KEY_NONE;
    m.tags[s] = MAP_KEY_NONE;
    *(float4 *)(m.rows + (size_t)s * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
    m.hits[s] = 0;
  }
}

// pass 3: the staged keys are distinct, so whoever wins the CAS on a slot owns it and writes the rest with plain
// stores; the kernel boundary publishes them.  The same bounded probe as the insert: a record without a slot is lost whole.
__global__ __launch_bounds__(256) void k_map_prune_reinsert(void *map, long long cap_max, void *ws) {
  MapView m;
  if (!map_view(map, cap_max, m)) return;
  const long long cap = m.hdr->capacity;
  const PruneStage st = prune_stage(ws, cap);
  if (st.ctl->evicted == 0) return;
  const long long n = (long long)st.ctl->kept < cap ? (long long)st.ctl->kept : cap;
  const map_u64 mask = (map_u64)cap - 1;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const map_u64 key = st.keys[i];
    map_u64 s = map_mix(key) & mask;
    bool found = false;
    for (int probe = 0; probe < RSLO_MAP_MAX_PROBE; ++probe) {
      // a stale read can only show "empty": in this launch a key goes from empty to set and never back
      if (__builtin_nontemporal_load(&m.keys[s]) == MAP_KEY_NONE &&
          atomicCAS(&m.keys[s], MAP_KEY_NONE, key) == MAP_KEY_NONE) {
        found = true;
        break;
      }
      s = (s + 1) & mask;
    }
    if (found) {
      m.tags[s] = st.tags[i];
      *(float4 *)(m.rows + (size_t)s * 4) = st.rows[i];
      m.hits[s] = st.hits[i];
    }
    atomicAdd(&st.ctl->lost, (map_u64)(!found));
  }
}

__global__ void k_map_prune_done(void *map, long long cap_max, const void *ws) {
  MapView m;
  if (threadIdx.x != 0 || !map_view(map, cap_max, m)) return;
  const PruneCtl *ctl = (const PruneCtl *)ws;
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
    int32_t *slot_of = (int32_t *)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    const unsigned nb = (unsigned)rslo_cdiv(N, 256);
    hipLaunchKernelGGL(k_map_insert, dim3(nb), dim3(256), 0, s, map, cap_max, points, stride_floats, N, pose7, slot_of);
    hipLaunchKernelGGL(k_map_rows, dim3(nb), dim3(256), 0, s, map, cap_max, points, stride_floats, width, N, pose7,
                       (const int32_t *)slot_of);
  }
  hipLaunchKernelGGL(k_map_scan_done, dim3(1), dim3(64), 0, s, map, cap_max);      // N == 0 still counts as a scan
  RSLO_CHECK_LAUNCH("map_insert");
  return RSLO_OK;
}

extern "C" int rslo_map_insert_frames(void *map, size_t map_bytes, const void *store, size_t store_bytes, int64_t capacity,
                                      int K, const double *poses, int n_poses, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  const long long cap_max = map_cap_of_bytes(map_bytes);
  RSLO_CHECK_ARG(map && cap_max > 0, "map_insert_frames: no map (map_bytes below rslo_map_bytes(1024))");
  RSLO_CHECK_ARG(store && ((uintptr_t)store & 15) == 0, "map_insert_frames: store is null or not 16-byte aligned");
  RSLO_CHECK_ARG(kf_shape_ok(capacity, K),
                 "map_insert_frames: need capacity in 1 .. 2^16 and K a multiple of 64 in 64 .. 4096");
  RSLO_CHECK_ARG(store_bytes >= kf_bytes_of(capacity, K), "map_insert_frames: store_bytes is smaller than rslo_keyframe_bytes");
  RSLO_CHECK_ARG(poses, "map_insert_frames: poses is null");
  RSLO_CHECK_ARG(n_poses >= 0, "map_insert_frames: n_poses < 0");
  if (n_poses == 0) return RSLO_OK;
  const int frames = n_poses < capacity ? n_poses : (int)capacity;      // the store holds no more
  const int bpf = rslo_cdiv(K, 256);
  const unsigned nb = (unsigned)(cap_max / 256 < 2048 ? cap_max / 256 : 2048);
  const unsigned tiles = (unsigned)frames * (unsigned)bpf;      // <= 2^16 * 16
  hipLaunchKernelGGL(k_map_frames_points, dim3(tiles < MAP_FRAMES_BLOCKS ? tiles : MAP_FRAMES_BLOCKS), dim3(256), 0, s, map,
                     cap_max, (void *)store, store_bytes, (long long)capacity, K, poses, n_poses, bpf);
  hipLaunchKernelGGL(k_map_frames_rows, dim3(nb), dim3(256), 0, s, map, cap_max, (void *)store, store_bytes,
                     (long long)capacity, K, poses, n_poses);
  hipLaunchKernelGGL(k_map_frames_done, dim3(1), dim3(64), 0, s, map, cap_max, (void *)store, store_bytes, (long long)capacity,
                     K, n_poses);
  RSLO_CHECK_LAUNCH("map_insert_frames");
  return RSLO_OK;
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
  const unsigned nb = (unsigned)(cap_max / 256 < 2048 ? cap_max / 256 : 2048);
  hipLaunchKernelGGL(k_map_export, dim3(nb), dim3(256), 0, s, (void *)map, cap_max, min_hits, center3, radius, rows,
                     (map_u64 *)tags, hits, (long long)max_rows, (map_u64 *)counts);
  RSLO_CHECK_LAUNCH("map_export");
  return RSLO_OK;
}

// the launches of a rebuild that do not depend on who removes the cells (map_rebuild.h)
void map_rebuild_begin(void *ws, hipStream_t s) { hipLaunchKernelGGL(k_map_prune_begin, dim3(1), dim3(64), 0, s, ws); }

void map_rebuild_table(void *map, long long cap_max, void *ws, hipStream_t s) {
  const unsigned nb = map_rebuild_blocks(cap_max);
  hipLaunchKernelGGL(k_map_prune_clear, dim3(nb), dim3(256), 0, s, map, cap_max, (const void *)ws);
  hipLaunchKernelGGL(k_map_prune_reinsert, dim3(nb), dim3(256), 0, s, map, cap_max, ws);
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
  const unsigned nb = map_rebuild_blocks(cap_max);
  map_rebuild_begin(ws, s);
  hipLaunchKernelGGL(k_map_prune_scan, dim3(nb), dim3(256), 0, s, map, cap_max, center3, radius, min_hits, grace, ws);
  map_rebuild_table(map, cap_max, ws, s);
  hipLaunchKernelGGL(k_map_prune_done, dim3(1), dim3(64), 0, s, map, cap_max, (const void *)ws);
  RSLO_CHECK_LAUNCH("map_prune");
  return RSLO_OK;
}
