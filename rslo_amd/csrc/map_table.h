// The table of the world voxel map as its kernels see it (csrc/map.hip, csrc/mapreg.hip; csrc/surfel.hip shares the hash,
// the point function and the search): header and section layout, the hash, the one function that turns a point into its
// world position and cell, and the 27-cell neighbour search.  The write side of the table, which the surfel map shares
// too, is map_core.h.  Rules: include/rslo_hip.h "World voxel map".
#pragma once
#include "rslo_common.h"

#pragma clang fp contract(off)   /* the cell of a point must not depend on FMA formation */

#include "se3.h"                 /* after the pragma: the pose algebra takes this file's contraction state */

typedef unsigned long long map_u64;
#define MAP_KEY_NONE (~(map_u64)0)
#define MAP_MAGIC 0x52534c4f4d415031ull /* "RSLOMAP1" */
#define MAP_HDR_BYTES 256
#define MAP_MAXC 1048576.0               /* 2^20: |cell| of a stored point is below it */
#define MAP_MIN_CAP 1024
#define MAP_SLOT_BYTES 36                /* key 8 + tag 8 + row 16 + hits 4 */

// host: the largest capacity that an allocation of `bytes` can hold of a table with this header and slot size (0: none)
static inline long long table_cap_of_bytes(size_t bytes, size_t hdr_bytes, size_t slot_bytes) {
  if (bytes < hdr_bytes + slot_bytes * MAP_MIN_CAP) return 0;
  const size_t slots = (bytes - hdr_bytes) / slot_bytes;
  long long cap = MAP_MIN_CAP;
  while ((size_t)cap * 2 <= slots && cap < ((long long)1 << 31)) cap *= 2;
  return cap;
}
static inline long long map_cap_of_bytes(size_t bytes) { return table_cap_of_bytes(bytes, MAP_HDR_BYTES, MAP_SLOT_BYTES); }

struct MapHdr {                          // int64 words: 0 magic, 1 capacity, 2-4 parameters, 5-7 prune counters, 8-13 counters,
  map_u64 magic;                         // 14-15 carve counters
  long long capacity;
  double voxel, min_range, max_range;
  map_u64 n_prunes, n_evicted, n_lost;   // written by rslo_map_prune's last launch only (n_lost: by rslo_map_carve's too)
  map_u64 n_scans, n_cells, n_points, dropped_invalid, dropped_range, dropped_full;
  map_u64 n_carves, n_carved;            // written by rslo_map_carve's last launch only
};
static_assert(sizeof(MapHdr) <= MAP_HDR_BYTES, "map header");

struct MapView {
  MapHdr *hdr;
  map_u64 *keys, *tags;
  float *rows;
  int32_t *hits;
};

// the sections of a map of `cap` slots (cap from the header, checked against what the allocation holds)
__device__ __forceinline__ bool map_view(void *map, long long cap_max, MapView &v) {
  MapHdr *h = (MapHdr *)map;
  const long long cap = h->capacity;
  if (h->magic != MAP_MAGIC || cap < MAP_MIN_CAP || cap > cap_max || (cap & (cap - 1))) return false;
  unsigned char *p = (unsigned char *)map + MAP_HDR_BYTES;
  v.hdr = h;
  v.keys = (map_u64 *)p;
  v.tags = (map_u64 *)(p + (size_t)cap * 8);
  v.rows = (float *)(p + (size_t)cap * 16);
  v.hits = (int32_t *)(p + (size_t)cap * 32);
  return true;
}
__device__ __forceinline__ bool table_view(void *map, long long cap_max, MapView &v) { return map_view(map, cap_max, v); }

__device__ __forceinline__ map_u64 map_mix(map_u64 x) {      // splitmix64 finaliser
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}

// The stored cells among key + {-1,0,1}^3 in a table of `capacity` (<= 2^31) slots: visit(slot, neighbour key) for each,
// in the order j = 9 (dx + 1) + 3 (dy + 1) + (dz + 1).  The 27 probe chains are independent 8-byte gathers into a table
// far larger than L2, so the first-slot keys of all 27 are loaded before any of them is examined (27 loads in flight
// per lane); a chain goes on alone, up to the bounded probe, only when its first slot held another cell's key.
template <class Visit>
__device__ __forceinline__ void map_neighbours(const map_u64 *keys, long long capacity, map_u64 key, Visit visit) {
  const uint32_t mask = (uint32_t)((map_u64)capacity - 1);
  const int c[3] = {(int)(key >> 42) & 0x1fffff, (int)(key >> 21) & 0x1fffff, (int)key & 0x1fffff};
  map_u64 k0[27];
  uint32_t s0[27];
#pragma unroll
  for (int j = 0; j < 27; ++j) {
    const int x = c[0] + j / 9 - 1, y = c[1] + (j / 3) % 3 - 1, z = c[2] + j % 3 - 1;
    const map_u64 nk = ((map_u64)(uint32_t)x << 42) | ((map_u64)(uint32_t)y << 21) | (map_u64)(uint32_t)z;
    s0[j] = (uint32_t)map_mix(nk) & mask;      // (a neighbour outside the key space is not examined below; its slot is in range)
    k0[j] = keys[s0[j]];
  }
#pragma unroll
  for (int j = 0; j < 27; ++j) {
    const int x = c[0] + j / 9 - 1, y = c[1] + (j / 3) % 3 - 1, z = c[2] + j % 3 - 1;
    if (x < 1 || x > 0x1fffff || y < 1 || y > 0x1fffff || z < 1 || z > 0x1fffff) continue;      // |cell| >= 2^20
    const map_u64 nk = ((map_u64)(uint32_t)x << 42) | ((map_u64)(uint32_t)y << 21) | (map_u64)(uint32_t)z;
    map_u64 k = k0[j];
    uint32_t s = s0[j];
    for (int probe = 1; k != nk && k != MAP_KEY_NONE && probe < RSLO_MAP_MAX_PROBE; ++probe) {
      s = (s + 1) & mask;
      k = keys[s];
    }
    if (k == nk) visit(s, nk);
  }
}

// 0: key and world position valid; 1: skipped (not finite, or outside the range gate); 2: cell outside +-2^20
__device__ __forceinline__ int map_point(const float *__restrict__ p, const double *__restrict__ pose, double voxel,
                                         double min_range, double max_range, map_u64 &key, double *w) {
  const float fx = p[0], fy = p[1], fz = p[2];
  const float inf = __builtin_inff();
  if (!(fabsf(fx) < inf && fabsf(fy) < inf && fabsf(fz) < inf)) return 1;      // NaN compares false
  const double x[3] = {(double)fx, (double)fy, (double)fz};
  const double d2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
  if (!(d2 >= min_range * min_range && d2 < max_range * max_range)) return 1;
  const double t[3] = {pose[0], pose[1], pose[2]}, q[4] = {pose[3], pose[4], pose[5], pose[6]};
  double r[3];
  se3_rotate(q, x, r);      // form A, uncontracted; the pose's quaternion is used as it is, not renormalised
  map_u64 k = 0;
  for (int a = 0; a < 3; ++a) {
    w[a] = t[a] + r[a];
    const double cell = floor(w[a] / voxel);
    if (!(fabs(cell) < MAP_MAXC)) return 2;                      // also a NaN or infinite world coordinate
    k = (k << 21) | (map_u64)((long long)cell + 1048576);
  }
  key = k;
  return 0;
}
