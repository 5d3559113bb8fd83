// The in-place rebuild of the world voxel map's table, shared by the two calls that remove cells: rslo_map_prune
// (csrc/map.hip) and rslo_map_carve (csrc/carve.hip).  Each brings its own scan kernel, which stages the kept records,
// and its own last launch, which writes the header; the launches between them -- zero the control block, empty every
// slot, re-insert the staged records -- are the kernels of map.hip, launched through the two host functions below.
// Workspace: control block (256 bytes) | staged keys u64 [cap] | tags u64 [cap] | rows f32 [cap, 4] | hits i32 [cap]
// -- the map's own section layout.
#pragma once
#include "map_table.h"

#define MAP_SLOT_BYTES 36                /* key 8 + tag 8 + row 16 + hits 4 */
#define PRUNE_CTL_BYTES 256

static inline long long map_cap_of_bytes(size_t bytes) {      // the largest capacity the allocation can hold (0: none)
  if (bytes < (size_t)MAP_HDR_BYTES + (size_t)MAP_SLOT_BYTES * MAP_MIN_CAP) return 0;
  const size_t slots = (bytes - MAP_HDR_BYTES) / MAP_SLOT_BYTES;
  long long cap = MAP_MIN_CAP;
  while ((size_t)cap * 2 <= slots && cap < ((long long)1 << 40)) cap *= 2;
  return cap;
}

struct PruneCtl {
  map_u64 kept, evicted, lost;
};

struct PruneStage {
  PruneCtl *ctl;
  map_u64 *keys, *tags;
  float4 *rows;
  int32_t *hits;
};

__device__ __forceinline__ PruneStage prune_stage(void *ws, long long cap) {
  unsigned char *p = (unsigned char *)ws + PRUNE_CTL_BYTES;
  PruneStage st;
  st.ctl = (PruneCtl *)ws;
  st.keys = (map_u64 *)p;
  st.tags = (map_u64 *)(p + (size_t)cap * 8);
  st.rows = (float4 *)(p + (size_t)cap * 16);
  st.hits = (int32_t *)(p + (size_t)cap * 32);
  return st;
}

// host, defined in map.hip.  The grid of every pass over the slots of a table that map_bytes can hold:
static inline unsigned map_rebuild_blocks(long long cap_max) { return (unsigned)(cap_max / 256 < 2048 ? cap_max / 256 : 2048); }
void map_rebuild_begin(void *ws, hipStream_t s);                                 // one launch: the control block to zero
void map_rebuild_table(void *map, long long cap_max, void *ws, hipStream_t s);   // two launches: clear, re-insert
