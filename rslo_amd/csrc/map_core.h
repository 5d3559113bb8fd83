// The write side of the voxel-hash table that the world voxel map (csrc/map.hip, csrc/carve.hip) and the surfel map
// (csrc/surfel.hip) share: the claim probe, the front half of an insert, the points pass of insert_frames, the re-insert
// pass of a rebuild, and the host helpers of those calls.  A table is a View {hdr, keys, ...} whose header carries
// capacity, voxel, min_range, max_range and the counters n_scans, n_cells .. dropped_full in this order; table_view()
// is overloaded on the View (map_table.h has the voxel map's, surfel.hip the surfel map's).  The read side (map_point,
// map_neighbours) is map_table.h's.  Included under the includer's `#pragma clang fp contract(off)`.
#pragma once
#include <cstddef>

#include "map_table.h"
#include "kf_store.h"            /* insert_frames reads a keyframe store */

#define TABLE_FRAMES_BLOCKS 2048u        /* workgroups of an insert_frames points pass: eight per CU */
#define PRUNE_CTL_BYTES 256

// ---------------------------------------------------------------------------------------------------------------------
// Device
// ---------------------------------------------------------------------------------------------------------------------
// The slot of `key` in keys[mask + 1], claimed if the key is not stored yet, or -1 when the bounded probe finds neither
// the key nor room; created() is called, inside the loop, by a caller that has just created the cell.  (A flag handed
// back and an n_cells add behind the loop were measured: the 4096-frame insert_frames 2.8 % slower, profiles/NOTES.md.)
// Every decision rests on the return value of the atomicCAS.  The non-temporal pre-read only skips a CAS that cannot
// change anything: in a launch that calls this, a key goes from empty to set and never back, so a stale read can only
// show "empty" -- then the CAS decides.  In a rebuild the staged keys are distinct: "found an equal key" never happens
// there, and a slot returned was always created by the caller.
template <class Created>
__device__ __forceinline__ int32_t table_claim(map_u64 *keys, map_u64 mask, map_u64 key, Created created) {
  map_u64 s = map_mix(key) & mask;
  for (int probe = 0; probe < RSLO_MAP_MAX_PROBE; ++probe) {
    map_u64 prev = __builtin_nontemporal_load(&keys[s]);
    if (prev == MAP_KEY_NONE) {
      prev = atomicCAS(&keys[s], MAP_KEY_NONE, key);
      if (prev == MAP_KEY_NONE) {
        created();
        prev = key;
      }
    }
    if (prev == key) return (int32_t)s;      // capacity <= 2^31 slots
    s = (s + 1) & mask;
  }
  return -1;
}

// the five header counters an insert adds to, in the header's order (n_cells .. dropped_full)
struct InsertTally {
  map_u64 n_cells, n_points, dropped_invalid, dropped_range, dropped_full;
};
template <class Hdr>
constexpr bool table_tally_mirrors() {
  return offsetof(Hdr, n_points) == offsetof(Hdr, n_cells) + 8 && offsetof(Hdr, dropped_invalid) == offsetof(Hdr, n_cells) + 16 &&
         offsetof(Hdr, dropped_range) == offsetof(Hdr, n_cells) + 24 && offsetof(Hdr, dropped_full) == offsetof(Hdr, n_cells) + 32;
}
static_assert(table_tally_mirrors<MapHdr>(), "InsertTally mirrors the header's counters");

// The front half of every insert: point p (x, y, z) under `pose` to its slot and its world position w.  The counters
// dropped_invalid, dropped_range, n_cells and dropped_full go to `c` -- the table's header itself (one scan), or a
// workgroup's InsertTally in LDS that is added to the header once (insert_frames).  -> the slot, or -1 for a point that
// was dropped; n_points is the caller's to count, behind whatever it does with the slot.
template <class View, class Counters>
__device__ __forceinline__ int32_t table_slot(const View &m, Counters *c, const float *__restrict__ p,
                                              const double *__restrict__ pose, double *w) {
  map_u64 key;
  const int why = map_point(p, pose, m.hdr->voxel, m.hdr->min_range, m.hdr->max_range, key, w);
  if (why) {
    // both adds by every dropped lane, each to ONE address: the compiler then folds an add into one per wave.  (Given
    // `if (why == 1) add(a, 1); else add(b, 1);` it merges the two into one add whose address differs per lane, which
    // is issued lane by lane: 1.4 ms for a scan whose points are all dropped.)  The empty statement behind them keeps
    // it from doing the same to the second add and the dropped_full add below, which also end a path that returns -1.
    atomicAdd(&c->dropped_invalid, (map_u64)(why == 1));
    atomicAdd(&c->dropped_range, (map_u64)(why == 2));
    asm volatile("");
    return -1;
  }
  const int32_t s = table_claim(m.keys, (map_u64)m.hdr->capacity - 1, key, [&] { atomicAdd(&c->n_cells, (map_u64)1); });
  if (s < 0) atomicAdd(&c->dropped_full, (map_u64)1);
  return s;
}

template <class View>
__global__ void k_table_scan_done(void *map, long long cap_max) {
  View m;
  if (threadIdx.x == 0 && table_view(map, cap_max, m)) m.hdr->n_scans = m.hdr->n_scans + 1;
}

// n = min(the store's entry count, read here and held to the store's capacity; n_poses)
__device__ __forceinline__ long long table_frames_n(const KfView &v, int n_poses) {
  long long n = v.hdr->n_entries;
  n = n < 0 ? 0 : (n > v.hdr->capacity ? v.hdr->capacity : n);
  return n < (long long)n_poses ? n : (long long)n_poses;
}

// insert_frames, pass 1: one thread per (frame, row) in tiles of 256 rows, bpf tiles per frame; frame, pose and count
// are uniform over a tile.  A workgroup takes tiles blockIdx.x, blockIdx.x + gridDim.x, ... and counts in LDS: with the
// header as the sink every WAVE would add to the same few words, and adds to one address are served one after the other
// on the memory side -- measured at 0.8 us per wave, 45 ms for 4096 frames -- so the header gets one add per workgroup
// and non-zero counter.  The scan number of frame e is n_scans + e: the header's n_scans does not change before pass 3.
// Body::point(m, tally, valid, p, pose, scan, i) is entered by EVERY lane of every tile, the ones past the frame's count
// included (valid == false, p zeros): a body may ballot and shuffle across the full wave.
template <class View, class Body>
__global__ __launch_bounds__(256) void k_table_frames_points(void *map, long long cap_max, void *store, size_t store_bytes,
                                                             long long kf_cap, int K, const double *__restrict__ poses,
                                                             int n_poses, int bpf) {
  __shared__ InsertTally tally;
  if (threadIdx.x < 5) ((map_u64 *)&tally)[threadIdx.x] = 0;
  __syncthreads();
  View m;
  KfView v;
  if (!table_view(map, cap_max, m) || !kf_view(store, store_bytes, kf_cap, K, v)) return;      // uniform over the grid
  const long long tiles = table_frames_n(v, n_poses) * bpf;
  const map_u64 s0 = m.hdr->n_scans;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long e = tile / bpf;
    const int i = (int)(tile % bpf) * 256 + (int)threadIdx.x;
    int count = v.counts[e];
    count = count < 0 ? 0 : (count > K ? K : count);
    const bool valid = i < count;
    float p[3] = {0.f, 0.f, 0.f};
    if (valid) {
      const float4 r = *(const float4 *)(v.rows + ((size_t)e * K + i) * 4);
      p[0] = r.x, p[1] = r.y, p[2] = r.z;
    }
    Body::point(m, &tally, valid, p, poses + (size_t)e * 7, s0 + (map_u64)e, (uint32_t)i);
  }
  __syncthreads();
  if (threadIdx.x < 5) {
    const map_u64 add = ((map_u64 *)&tally)[threadIdx.x];
    if (add) atomicAdd(&m.hdr->n_cells + threadIdx.x, add);
  }
}

// insert_frames, pass 3: an empty frame still counts as a scan
template <class View>
__global__ void k_table_frames_done(void *map, long long cap_max, void *store, size_t store_bytes, long long kf_cap, int K,
                                    int n_poses) {
  View m;
  KfView v;
  if (threadIdx.x != 0 || !table_view(map, cap_max, m) || !kf_view(store, store_bytes, kf_cap, K, v)) return;
  m.hdr->n_scans = m.hdr->n_scans + (map_u64)table_frames_n(v, n_poses);
}

// The control block of a rebuild (prune, carve), the first 256 bytes of its workspace; zeroed by the first, one-thread
// launch.  `planar` is the surfel map's.
struct RebuildCtl {
  map_u64 kept, evicted, lost, planar;
};

// A rebuild's pass 3: the staged keys are distinct, so whoever wins the CAS on a slot owns it and writes the rest of the
// record with plain stores; the kernel boundary publishes them.  The insert's bounded probe: a record without a slot is
// lost whole.  Records: stage(ws, cap) -> the staging area {keys, ...}; put(m, st, i, s) copies staged record i into
// slot s and says whether it is planar.  The lost records and the planar rows are counted per thread, summed in LDS
// and added once per workgroup.
template <class View, class Records>
__global__ __launch_bounds__(256) void k_table_reinsert(void *map, long long cap_max, void *ws) {
  __shared__ unsigned int tally[2];      // lost, planar
  if (threadIdx.x < 2) tally[threadIdx.x] = 0;
  __syncthreads();
  View m;
  if (!table_view(map, cap_max, m)) return;      // uniform over the grid
  const long long cap = m.hdr->capacity;
  const auto st = Records::stage(ws, cap);
  RebuildCtl *ctl = (RebuildCtl *)ws;
  if (ctl->evicted == 0) return;                 // uniform over the grid
  const long long n = (long long)ctl->kept < cap ? (long long)ctl->kept : cap;
  const map_u64 mask = (map_u64)cap - 1;
  unsigned int lost = 0, planar = 0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int32_t s = table_claim(m.keys, mask, st.keys[i], [] {});
    if (s < 0) {
      ++lost;
      continue;
    }
    planar += Records::put(m, st, (size_t)i, (size_t)s);
  }
  if (lost) atomicAdd(&tally[0], lost);
  if (planar) atomicAdd(&tally[1], planar);
  __syncthreads();
  if (threadIdx.x == 0 && tally[0]) atomicAdd(&ctl->lost, (map_u64)tally[0]);
  if (threadIdx.x == 1 && tally[1]) atomicAdd(&ctl->planar, (map_u64)tally[1]);
}

// The staging area of the voxel map's rebuilds, shared by rslo_map_prune (csrc/map.hip) and rslo_map_carve
// (csrc/carve.hip): control block | staged keys u64 [cap] | tags u64 [cap] | rows f32 [cap, 4] | hits i32 [cap] -- the
// map's own section layout.  Each call brings its own scan kernel, which stages the kept records, and its own last
// launch, which writes the header.
struct PruneStage {
  RebuildCtl *ctl;
  map_u64 *keys, *tags;
  float4 *rows;
  int32_t *hits;
};

__device__ __forceinline__ PruneStage prune_stage(void *ws, long long cap) {
  unsigned char *p = (unsigned char *)ws + PRUNE_CTL_BYTES;
  PruneStage st;
  st.ctl = (RebuildCtl *)ws;
  st.keys = (map_u64 *)p;
  st.tags = (map_u64 *)(p + (size_t)cap * 8);
  st.rows = (float4 *)(p + (size_t)cap * 16);
  st.hits = (int32_t *)(p + (size_t)cap * 32);
  return st;
}

// ---------------------------------------------------------------------------------------------------------------------
// Host
// ---------------------------------------------------------------------------------------------------------------------
// the grid of every pass over the slots of a table that map_bytes can hold
static inline unsigned table_blocks(long long cap_max) { return (unsigned)(cap_max / 256 < 2048 ? cap_max / 256 : 2048); }

// slot_of, the int32 [N] of an insert's workspace: its first 256-byte boundary
static inline int32_t *table_slot_of(void *ws) { return (int32_t *)(((uintptr_t)ws + 255) & ~(uintptr_t)255); }

// defined in map.hip
void map_rebuild_begin(void *ws, hipStream_t s);                                 // one launch: the control block to zero
void map_rebuild_table(void *map, long long cap_max, void *ws, hipStream_t s);   // two launches: clear, re-insert (voxel map)

// insert_frames of both tables: the argument rules (`name` is the call's, `bytes_fn` the table's rslo_*_bytes) and the
// three launches, of which the middle one is the table's own: rows(nb) launches it over nb workgroups of 256.
template <class View, class Body, class Rows>
static int table_insert_frames(const char *name, const char *bytes_fn, void *map, long long cap_max, const void *store,
                               size_t store_bytes, int64_t capacity, int K, const double *poses, int n_poses, hipStream_t s,
                               Rows rows) {
  RSLO_CHECK_ARG(map && cap_max > 0, "%s: no map (map_bytes below %s(1024))", name, bytes_fn);
  RSLO_CHECK_ARG(store && ((uintptr_t)store & 15) == 0, "%s: store is null or not 16-byte aligned", name);
  RSLO_CHECK_ARG(kf_shape_ok(capacity, K), "%s: need capacity in 1 .. 2^16 and K a multiple of 64 in 64 .. 4096", name);
  RSLO_CHECK_ARG(store_bytes >= kf_bytes_of(capacity, K), "%s: store_bytes is smaller than rslo_keyframe_bytes", name);
  RSLO_CHECK_ARG(poses, "%s: poses is null", name);
  RSLO_CHECK_ARG(n_poses >= 0, "%s: n_poses < 0", name);
  if (n_poses == 0) return RSLO_OK;
  const int frames = n_poses < capacity ? n_poses : (int)capacity;      // the store holds no more
  const int bpf = rslo_cdiv(K, 256);
  const unsigned tiles = (unsigned)frames * (unsigned)bpf;      // <= 2^16 * 16
  hipLaunchKernelGGL((k_table_frames_points<View, Body>), dim3(tiles < TABLE_FRAMES_BLOCKS ? tiles : TABLE_FRAMES_BLOCKS),
                     dim3(256), 0, s, map, cap_max, (void *)store, store_bytes, (long long)capacity, K, poses, n_poses, bpf);
  rows(table_blocks(cap_max));
  hipLaunchKernelGGL(k_table_frames_done<View>, dim3(1), dim3(64), 0, s, map, cap_max, (void *)store, store_bytes,
                     (long long)capacity, K, n_poses);
  RSLO_CHECK_LAUNCH(name);
  return RSLO_OK;
}
