// The keyframe store as its kernels see it (csrc/loopverify.hip fills and verifies against it, csrc/map.hip rebuilds a map
// from it): header and section layout.  Rules: include/rslo_hip.h "Loop verification".
//
// One caller-owned allocation, header (256 bytes) | counts i32 [capacity] | rows f32 [capacity, K, 4], every section
// padded to 256 bytes.  Entries are only appended; the entry counter lives in the header and is read on the device.
#pragma once
#include "rslo_common.h"

typedef unsigned long long kf_u64;

#define KF_MAGIC 0x52534c4f4b465231ull   /* "RSLOKFR1" */
#define KF_HDR_BYTES 256
#define KF_MAX_CAP ((int64_t)1 << 16)

struct KfHdr {
  kf_u64 magic;
  long long capacity, K, reserved;
  long long n_entries, dropped_full;
};

struct KfView {
  KfHdr *hdr;
  int32_t *counts;
  float *rows;
};

static __host__ __device__ inline size_t kf_pad(size_t b) { return (b + 255) / 256 * 256; }

static __host__ __device__ inline size_t kf_bytes_of(long long cap, int K) {
  return (size_t)KF_HDR_BYTES + kf_pad((size_t)cap * 4) + kf_pad((size_t)cap * K * 16);
}

static inline bool kf_shape_ok(int64_t cap, int K) { return cap >= 1 && cap <= KF_MAX_CAP && K >= 64 && K <= 4096 && K % 64 == 0; }

// the store the caller says it is (capacity and K as handed to reset), or nothing at all
__device__ __forceinline__ bool kf_view(void *st, size_t st_bytes, long long cap, int K, KfView &v) {
  KfHdr *h = (KfHdr *)st;
  if (st_bytes < kf_bytes_of(cap, K)) return false;
  if (h->magic != KF_MAGIC || h->capacity != cap || h->K != K) return false;
  unsigned char *p = (unsigned char *)st + KF_HDR_BYTES;
  v.hdr = h;
  v.counts = (int32_t *)p;
  p += kf_pad((size_t)cap * 4);
  v.rows = (float *)p;
  return true;
}
