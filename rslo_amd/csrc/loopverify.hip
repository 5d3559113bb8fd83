// Loop verification: a device-resident store of down-sampled keyframes, a geometric check of the loop candidates of a
// place search in ONE launch, and a device edge list the pose graph reads (rules: include/rslo_hip.h "Loop
// verification"; float64 restatement: rslo_amd/loops.py KeyframeStoreRef / LoopVerifierRef).  Nothing of the reference
// corresponds to it.
//
// Store: one caller-owned allocation, header (256 bytes) | counts i32 [capacity] | rows f32 [capacity, K, 4], every
// section padded to 256 bytes.  Entries are only appended; the entry counter lives in the header and is read on the
// device, exactly as in places.hip.
//
// Verification (k_loop_verify): one workgroup per candidate row, the whole Gauss-Newton schedule and the fitness pass
// inside the launch.  The candidate's target frame is staged once into LDS as three float planes (12 bytes a point,
// 48 KiB at K = 4096), and every source point scans ALL of it: the exact nearest point by construction, ties to the
// lowest index because the scan ascends and replaces on a strict `<` only.  All lanes of a wave read the same target
// word at the same time (an LDS broadcast, no bank conflict).  The 28 sums and the pair count are reduced in a fixed
// order -- a thread's own points by ascending index, a shuffle tree inside each wave, the waves in wave order -- with
// no floating-point atomic: two calls give the same bits.  Thread 0 takes the step on the pose kept in LDS.  The
// addends, the reduction and the step are gauss_newton.h's, shared with scan-to-map registration (mapreg.hip).
#include "rslo_common.h"

#include <math.h>

#pragma clang fp contract(off)   /* every sum is specified operation by operation */

#include "se3.h"
#include "gauss_newton.h"                /* after the pragma and after se3.h */
#include "kf_store.h"                    /* the store's layout, shared with csrc/map.hip (rslo_map_insert_frames) */

#define LV_MAX_STAGES 8
#define LV_MAX_ITERS 64
#define LV_MAX_TOPK 16
#define LV_MAX_EDGES 4096

// ---------------------------------------------------------------------------------------------------------------------
// store
// ---------------------------------------------------------------------------------------------------------------------
__global__ void k_kf_reset(void *st, long long cap, int K) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    KfHdr *h = (KfHdr *)st;
    h->magic = KF_MAGIC;
    h->capacity = cap;
    h->K = K;
    h->reserved = 0;
    h->n_entries = 0;
    h->dropped_full = 0;
  }
}

__global__ void k_kf_zero(int32_t *__restrict__ gated) {
  if (threadIdx.x == 0) *gated = 0;
}

// the gate: kept points are copied, gated points become NaN rows (the down-sample skips what is not finite)
__global__ __launch_bounds__(256) void k_kf_gate(const float *__restrict__ points, int stride, int N, double min_z,
                                                 double max_range, float *__restrict__ kept, int32_t *__restrict__ gated) {
  __shared__ int n_block;
  if (threadIdx.x == 0) n_block = 0;
  __syncthreads();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) {
    const float *p = points + (int64_t)i * stride;
    const float fx = p[0], fy = p[1], fz = p[2];
    const float inf = __builtin_inff();
    const double x = (double)fx, y = (double)fy, z = (double)fz;
    const bool keep = fabsf(fx) < inf && fabsf(fy) < inf && fabsf(fz) < inf && z > min_z &&
                      x * x + y * y + z * z < max_range * max_range;
    const float nan = __builtin_nanf("");
    kept[(size_t)i * 3 + 0] = keep ? fx : nan;
    kept[(size_t)i * 3 + 1] = keep ? fy : nan;
    kept[(size_t)i * 3 + 2] = keep ? fz : nan;
    if (!keep) atomicAdd(&n_block, 1);
  }
  __syncthreads();
  if (threadIdx.x == 0 && n_block) atomicAdd(gated, n_block);
}

// frame row k = down-sample row (k * Q) / K when Q > K, else row k; rows >= count are zero
__global__ __launch_bounds__(256) void k_kf_select(const float *__restrict__ ds_rows, const int32_t *__restrict__ ds_counts,
                                                   const int32_t *__restrict__ gated, int N, int K,
                                                   float *__restrict__ frame, int32_t *__restrict__ info) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const int flags = ds_counts[1] & 1;
  long long Q = flags ? 0 : ds_counts[0];
  Q = Q < 0 ? 0 : (Q > N ? N : Q);
  const int count = (int)(Q < K ? Q : K);
  if (k == 0) {
    info[0] = count;
    info[1] = (int32_t)Q;
    info[2] = flags;
    info[3] = N > 0 ? *gated : 0;
  }
  if (k >= K) return;
  float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
  if (k < count) {
    const long long src = Q > K ? ((long long)k * Q) / K : k;
    r.x = ds_rows[src * 3 + 0];
    r.y = ds_rows[src * 3 + 1];
    r.z = ds_rows[src * 3 + 2];
  }
  *(float4 *)(frame + (size_t)k * 4) = r;
}

__global__ __launch_bounds__(256) void k_kf_add(void *st, size_t st_bytes, long long cap, int K,
                                                const float *__restrict__ frame, const int32_t *__restrict__ info) {
  KfView v;
  if (!kf_view(st, st_bytes, cap, K, v)) return;
  const long long n = v.hdr->n_entries;      // constant during this launch: k_kf_add_done bumps it
  if (n < 0 || n >= cap) return;
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < K) *(float4 *)(v.rows + ((size_t)n * K + k) * 4) = *(const float4 *)(frame + (size_t)k * 4);
  if (k == 0) {
    const int c = info[0];
    v.counts[n] = c < 0 ? 0 : (c > K ? K : c);
  }
}

__global__ void k_kf_add_done(void *st, size_t st_bytes, long long cap, int K) {
  KfView v;
  if (threadIdx.x != 0 || !kf_view(st, st_bytes, cap, K, v)) return;
  const long long n = v.hdr->n_entries;
  if (n >= 0 && n < cap) v.hdr->n_entries = n + 1;
  else v.hdr->dropped_full = v.hdr->dropped_full + 1;
}

// ---------------------------------------------------------------------------------------------------------------------
// verification
// ---------------------------------------------------------------------------------------------------------------------
struct LvParams {
  int n_stages, total_iters;
  int iters[LV_MAX_STAGES];
  double max_dist[LV_MAX_STAGES];
  double max_distance, inlier_dist, min_overlap, max_rms, damping;
  int min_pairs;
};

// the exact nearest of the nt staged target points to w: smallest d2, ties to the lowest index (-1: none is comparable)
__device__ __forceinline__ int lv_nearest(const float *__restrict__ tx, const float *__restrict__ ty,
                                          const float *__restrict__ tz, int nt, const double *w, double &bd2, double *m) {
  int bj = -1;
  bd2 = (double)__builtin_inff();
  for (int j = 0; j < nt; ++j) {
    const double mx = (double)tx[j], my = (double)ty[j], mz = (double)tz[j];
    const double dx = w[0] - mx, dy = w[1] - my, dz = w[2] - mz;
    const double d2 = dx * dx + dy * dy + dz * dz;
    if (d2 < bd2) {
      bd2 = d2;
      bj = j;
      m[0] = mx;
      m[1] = my;
      m[2] = mz;
    }
  }
  return bj;
}

// dynamic LDS: tx f32 [K] | ty f32 [K] | tz f32 [K] | part f64 [waves, GN_NSUM] | tot f64 [GN_NSUM] | pose f64 [7] |
// flag i32 [2]
__global__ __launch_bounds__(1024) void k_loop_verify(void *st, size_t st_bytes, long long cap, int K,
                                                      const float *__restrict__ frame, const int32_t *__restrict__ frame_info,
                                                      const double *__restrict__ cands, const double *__restrict__ start,
                                                      LvParams P, double *__restrict__ out, double *__restrict__ info,
                                                      int32_t *__restrict__ matches) {
  extern __shared__ double lv_lds[];
  const int b = blockIdx.x, t = threadIdx.x, n_waves = blockDim.x >> 6;
  double *part = lv_lds;
  double *tot = part + (size_t)n_waves * GN_NSUM;
  double *pose = tot + GN_NSUM;
  int32_t *flag = (int32_t *)(pose + 8);
  float *tx = (float *)(pose + 10), *ty = tx + K, *tz = ty + K;

  double *o16 = out + (size_t)b * 16;
  double *irows = info ? info + (size_t)b * P.total_iters * 8 : nullptr;
  int32_t *mrow = matches ? matches + (size_t)b * K : nullptr;
  const double entry_d = cands[b * 4 + 0], distance = cands[b * 4 + 1], heading = cands[b * 4 + 3];

  KfView v;
  const bool have = kf_view(st, st_bytes, cap, K, v);
  long long n_entries = have ? v.hdr->n_entries : 0;
  n_entries = n_entries < 0 ? 0 : (n_entries > cap ? cap : n_entries);
  int nq = frame_info[0];
  nq = nq < 0 ? 0 : (nq > K ? K : nq);
  int status = 0, nt = 0;
  long long entry = -1;
  if (!(entry_d >= 0.0 && entry_d < (double)n_entries)) {
    status = 1;
  } else if (!(distance < P.max_distance)) {
    status = 2;
  } else {
    entry = (long long)entry_d;
    nt = v.counts[entry];
    nt = nt < 0 ? 0 : (nt > K ? K : nt);
    if (nq < P.min_pairs || nt < P.min_pairs) status = 3;
  }
  if (status) {      // uniform over the workgroup: nothing below runs
    if (t == 0) {
      for (int a = 0; a < 16; ++a) o16[a] = 0.0;
      o16[0] = (double)status;
      o16[1] = entry_d;
      o16[9] = 1.0;
    }
    if (irows)
      for (int a = t; a < P.total_iters * 8; a += blockDim.x) irows[a] = (a & 7) == 0 ? (double)status : 0.0;
    if (mrow)
      for (int a = t; a < K; a += blockDim.x) mrow[a] = -1;
    return;
  }

  const float *rows = v.rows + (size_t)entry * K * 4;
  for (int j = t; j < nt; j += blockDim.x) {
    const float4 r = *(const float4 *)(rows + (size_t)j * 4);
    tx[j] = r.x;
    ty[j] = r.y;
    tz[j] = r.z;
  }
  if (t == 0) {
    if (start) {
      for (int a = 0; a < 7; ++a) pose[a] = start[b * 7 + a];
    } else {
      pose[0] = pose[1] = pose[2] = 0.0;
      pose[3] = cos(heading / 2.0);
      pose[4] = pose[5] = 0.0;
      pose[6] = sin(heading / 2.0);
    }
    flag[0] = 0;
  }
  __syncthreads();

  double last_pairs = 0.0;
  int row = 0;
  bool failed = false;
  for (int s = 0; s < P.n_stages; ++s) {
    const double gate2 = P.max_dist[s] * P.max_dist[s];
    for (int it = 0; it < P.iters[s]; ++it, ++row) {
      if (failed) {      // the remaining iterations are skipped
        if (irows && t < 8) irows[row * 8 + t] = t == 0 ? 4.0 : t == 5 ? (double)s : 0.0;
        continue;
      }
      double Z[7];
      for (int a = 0; a < 7; ++a) Z[a] = pose[a];
      double acc[GN_NSUM];
#pragma unroll
      for (int k = 0; k < GN_NSUM; ++k) acc[k] = 0.0;
      for (int i = t; i < nq; i += blockDim.x) {      // a thread's points by ascending index
        const float4 p4 = *(const float4 *)(frame + (size_t)i * 4);
        const double p[3] = {(double)p4.x, (double)p4.y, (double)p4.z};
        double w[3], m[3], d2;
        se3_rotate(Z + 3, p, w);
        for (int a = 0; a < 3; ++a) w[a] = w[a] + Z[a];
        const int j = lv_nearest(tx, ty, tz, nt, w, d2, m);
        if (j >= 0 && d2 < gate2) {
          const double d[3] = {w[0] - m[0], w[1] - m[1], w[2] - m[2]};
          gn_point_terms(w, d, acc, true);      // a point term, residual d, added to the thread's running sums
          acc[GN_NSUM - 1] = acc[GN_NSUM - 1] + 1.0;
        }
      }
      gn_block_reduce(acc, part, n_waves, tot);
      __syncthreads();
      if (t == 0) {
        double nts = 0.0, th = 0.0;
        bool ok = tot[28] >= (double)P.min_pairs;
        if (ok) {
          double np[7];
          for (int a = 0; a < 7; ++a) np[a] = pose[a];
          ok = gn_step(tot, P.damping, np, nts, th);
          bool fin = ok;
          for (int a = 0; a < 7; ++a) fin = fin && fabs(np[a]) < (double)__builtin_inff();
          ok = fin;
          if (ok)
            for (int a = 0; a < 7; ++a) pose[a] = np[a];
          else
            nts = th = 0.0;
        }
        flag[0] = ok ? 0 : 1;
        if (irows) {
          double *r = irows + row * 8;
          r[0] = ok ? 0.0 : 4.0;
          r[1] = tot[28];
          r[2] = tot[27];
          r[3] = nts;
          r[4] = th;
          r[5] = (double)s;
          r[6] = 0.0;
          r[7] = 0.0;
        }
      }
      __syncthreads();
      last_pairs = tot[28];
      failed = flag[0] != 0;
      __syncthreads();      // tot and flag are read before the next iteration rewrites them
    }
  }

  // fitness at the final Z
  double Z[7];
  for (int a = 0; a < 7; ++a) Z[a] = pose[a];
  double n_in = 0.0, sum_d2 = 0.0;
  if (!failed) {
    const double gate2 = P.inlier_dist * P.inlier_dist;
    for (int i = t; i < K; i += blockDim.x) {
      int mj = -1;
      if (i < nq) {
        const float4 p4 = *(const float4 *)(frame + (size_t)i * 4);
        const double p[3] = {(double)p4.x, (double)p4.y, (double)p4.z};
        double w[3], m[3], d2;
        se3_rotate(Z + 3, p, w);
        for (int a = 0; a < 3; ++a) w[a] = w[a] + Z[a];
        const int j = lv_nearest(tx, ty, tz, nt, w, d2, m);
        if (j >= 0 && d2 < gate2) {
          mj = j;
          n_in = n_in + 1.0;
          sum_d2 = sum_d2 + d2;
        }
      }
      if (mrow) mrow[i] = mj;
    }
  } else if (mrow) {
    for (int i = t; i < K; i += blockDim.x) mrow[i] = -1;
  }
  n_in = gn_block_sum(n_in, part, n_waves);
  sum_d2 = gn_block_sum(sum_d2, part, n_waves);
  if (t == 0) {
    double overlap = 0.0, rms = 0.0;
    int st_out = 4;
    if (!failed) {
      st_out = 5;
      if (n_in > 0.0) {
        overlap = n_in / (double)nq;
        rms = sqrt(sum_d2 / n_in);
        if (overlap >= P.min_overlap && rms <= P.max_rms) st_out = 0;
      }
    }
    o16[0] = (double)st_out;
    o16[1] = (double)entry;
    o16[2] = last_pairs;
    o16[3] = overlap;
    o16[4] = rms;
    o16[5] = (double)nq;
    for (int a = 0; a < 7; ++a) o16[6 + a] = Z[a];
    o16[13] = distance;
    o16[14] = heading;
    o16[15] = 0.0;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// edge list
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_loop_edges_reset(int32_t *__restrict__ ij, double *__restrict__ Z,
                                                          double *__restrict__ w, long long *__restrict__ counters, int E) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e == 0) counters[0] = counters[1] = 0;
  if (e >= E) return;
  ij[e * 2] = ij[e * 2 + 1] = -1;
  for (int a = 0; a < 7; ++a) Z[(size_t)e * 7 + a] = a == 3 ? 1.0 : 0.0;
  w[e * 2] = w[e * 2 + 1] = 0.0;
}

__global__ void k_loop_emit(const double *__restrict__ out, int top_k, void *st, size_t st_bytes, long long cap, int K,
                            int32_t *__restrict__ ij, double *__restrict__ Z, double *__restrict__ w,
                            long long *__restrict__ counters, int E, double w_t, double w_r) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  KfView v;
  if (!kf_view(st, st_bytes, cap, K, v)) return;
  int best = -1;
  double best_overlap = 0.0;
  for (int r = 0; r < top_k; ++r) {      // the accepted row with the largest overlap, ties to the lowest row
    const double *o = out + (size_t)r * 16;
    if (o[0] == 0.0 && (best < 0 || o[3] > best_overlap)) {
      best = r;
      best_overlap = o[3];
    }
  }
  if (best < 0) return;
  const long long n = counters[0];
  if (n < 0 || n >= E) {
    counters[1] = counters[1] + 1;
    return;
  }
  const double *o = out + (size_t)best * 16;
  ij[n * 2] = (int32_t)o[1];
  ij[n * 2 + 1] = (int32_t)v.hdr->n_entries;
  for (int a = 0; a < 7; ++a) Z[n * 7 + a] = o[6 + a];
  w[n * 2] = w_t;
  w[n * 2 + 1] = w_r;
  counters[0] = n + 1;
}

// ---------------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------------
extern "C" size_t rslo_keyframe_bytes(int64_t capacity, int K) {
  if (!kf_shape_ok(capacity, K)) return 0;
  return kf_bytes_of(capacity, K);
}

#define KF_CHECK_STORE(name)                                                                                    \
  RSLO_CHECK_ARG(store && ((uintptr_t)store & 15) == 0 && rslo_keyframe_bytes(capacity, K) != 0 && store_bytes >= rslo_keyframe_bytes(capacity, K), \
                 name ": no 16-byte aligned store of this capacity and K (store_bytes below rslo_keyframe_bytes)")

extern "C" int rslo_keyframe_reset(void *store, size_t store_bytes, int64_t capacity, int K, void *stream) {
  RSLO_CHECK_ARG(store && ((uintptr_t)store & 15) == 0, "keyframe_reset: store is null or not 16-byte aligned");
  RSLO_CHECK_ARG(rslo_keyframe_bytes(capacity, K) != 0,
                 "keyframe_reset: need capacity in 1 .. 2^16 and K a multiple of 64 in 64 .. 4096");
  RSLO_CHECK_ARG(store_bytes >= rslo_keyframe_bytes(capacity, K), "keyframe_reset: store_bytes is smaller than rslo_keyframe_bytes");
  hipLaunchKernelGGL(k_kf_reset, dim3(1), dim3(64), 0, (hipStream_t)stream, store, (long long)capacity, K);
  RSLO_CHECK_LAUNCH("keyframe_reset");
  return RSLO_OK;
}

// workspace: control block (256 bytes: gated, down-sample counts) | kept f32 [N, 3] | down-sample rows f32 [N, 3] |
// the down-sample's own workspace
static size_t kf_ws_rows(int N) { return kf_pad((size_t)(N > 0 ? N : 0) * 12); }

extern "C" size_t rslo_keyframe_prepare_ws_bytes(int N) {
  if (N < 0) return 0;
  return 256 + 2 * kf_ws_rows(N) + rslo_voxel_downsample_ws_bytes(N) + 256;
}

extern "C" int rslo_keyframe_prepare(const float *points, int stride_floats, int N, int K, double voxel_size, double min_z,
                                     double max_range, float *frame, int32_t *frame_info, void *ws, size_t ws_bytes,
                                     void *stream) {
  hipStream_t s = (hipStream_t)stream;
  RSLO_CHECK_ARG(K >= 64 && K <= 4096 && K % 64 == 0, "keyframe_prepare: K must be a multiple of 64 in 64 .. 4096");
  RSLO_CHECK_ARG(N >= 0 && stride_floats >= 3, "keyframe_prepare: N < 0 or stride_floats < 3");
  RSLO_CHECK_ARG(N == 0 || points, "keyframe_prepare: points is null");
  RSLO_CHECK_ARG(voxel_size > 0.0 && voxel_size < (double)__builtin_inff(),
                 "keyframe_prepare: voxel_size must be positive and finite");
  RSLO_CHECK_ARG(min_z == min_z && max_range > 0.0, "keyframe_prepare: min_z is NaN, or max_range is not positive");
  RSLO_CHECK_ARG(frame && ((uintptr_t)frame & 15) == 0 && frame_info, "keyframe_prepare: frame (16-byte aligned) or frame_info is null");
  RSLO_CHECK_ARG(ws && ((uintptr_t)ws & 255) == 0, "keyframe_prepare: the workspace is null or not 256-byte aligned");
  if (ws_bytes < rslo_keyframe_prepare_ws_bytes(N)) {
    rslo_set_error("keyframe_prepare: workspace too small");
    return RSLO_EWS;
  }
  unsigned char *p = (unsigned char *)ws;
  int32_t *gated = (int32_t *)p, *ds_counts = gated + 4;
  float *kept = (float *)(p + 256);
  float *ds_rows = (float *)(p + 256 + kf_ws_rows(N));
  void *ds_ws = p + 256 + 2 * kf_ws_rows(N);
  if (N > 0) {
    hipLaunchKernelGGL(k_kf_zero, dim3(1), dim3(64), 0, s, gated);
    hipLaunchKernelGGL(k_kf_gate, dim3((unsigned)rslo_cdiv(N, 256)), dim3(256), 0, s, points, stride_floats, N, min_z,
                       max_range, kept, gated);
  }
  const int rc = rslo_voxel_downsample(kept, 3, nullptr, 0, N, voxel_size, ds_rows, nullptr, nullptr, ds_counts, ds_ws,
                                       ws_bytes - 256 - 2 * kf_ws_rows(N), stream);
  if (rc) return rc;
  hipLaunchKernelGGL(k_kf_select, dim3((unsigned)rslo_cdiv(K, 256)), dim3(256), 0, s, (const float *)ds_rows,
                     (const int32_t *)ds_counts, (const int32_t *)gated, N, K, frame, frame_info);
  RSLO_CHECK_LAUNCH("keyframe_prepare");
  return RSLO_OK;
}

extern "C" int rslo_keyframe_add(void *store, size_t store_bytes, int64_t capacity, int K, const float *frame,
                                 const int32_t *frame_info, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  KF_CHECK_STORE("keyframe_add");
  RSLO_CHECK_ARG(frame && ((uintptr_t)frame & 15) == 0 && frame_info, "keyframe_add: frame (16-byte aligned) or frame_info is null");
  hipLaunchKernelGGL(k_kf_add, dim3((unsigned)rslo_cdiv(K, 256)), dim3(256), 0, s, store, store_bytes, (long long)capacity, K,
                     frame, frame_info);
  hipLaunchKernelGGL(k_kf_add_done, dim3(1), dim3(64), 0, s, store, store_bytes, (long long)capacity, K);
  RSLO_CHECK_LAUNCH("keyframe_add");
  return RSLO_OK;
}

static size_t lv_lds_bytes(int K, int threads) {
  return ((size_t)(threads / 64) * GN_NSUM + GN_NSUM + 10) * 8 + (size_t)K * 12;
}

extern "C" int rslo_loop_verify(const void *store, size_t store_bytes, int64_t capacity, int K, const float *frame,
                                const int32_t *frame_info, const double *cands, int top_k, const double *start,
                                const double *stages, int n_stages, double max_distance, double inlier_dist,
                                double min_overlap, double max_rms, int min_pairs, double damping, double *out,
                                double *info, int32_t *matches, void *stream) {
  KF_CHECK_STORE("loop_verify");
  RSLO_CHECK_ARG(frame && ((uintptr_t)frame & 15) == 0 && frame_info && cands && out && stages,
                 "loop_verify: null pointer (frame must be 16-byte aligned)");
  RSLO_CHECK_ARG(top_k >= 1 && top_k <= LV_MAX_TOPK, "loop_verify: top_k must be in 1..16");
  RSLO_CHECK_ARG(n_stages >= 1 && n_stages <= LV_MAX_STAGES, "loop_verify: n_stages must be in 1..8");
  LvParams P;
  P.n_stages = n_stages;
  P.total_iters = 0;
  for (int k = 0; k < LV_MAX_STAGES; ++k) {
    P.iters[k] = 0;
    P.max_dist[k] = 0.0;
  }
  for (int k = 0; k < n_stages; ++k) {
    const double md = stages[2 * k], it = stages[2 * k + 1];
    RSLO_CHECK_ARG(md > 0.0 && md * md < (double)__builtin_inff(),
                   "loop_verify: stage %d: max_dist must be positive with a finite square (NaN is refused)", k);
    RSLO_CHECK_ARG(it >= 1.0 && it <= (double)LV_MAX_ITERS && it == (double)(int)it,
                   "loop_verify: stage %d: iters must be an integer >= 1 (all stages together: at most 64)", k);
    P.max_dist[k] = md;
    P.iters[k] = (int)it;
    P.total_iters += (int)it;
    RSLO_CHECK_ARG(P.total_iters <= LV_MAX_ITERS, "loop_verify: the iterations of all stages must sum to 1 .. 64");
  }
  RSLO_CHECK_ARG(max_distance == max_distance, "loop_verify: max_distance is NaN");
  RSLO_CHECK_ARG(inlier_dist > 0.0 && inlier_dist * inlier_dist < (double)__builtin_inff(),
                 "loop_verify: inlier_dist must be positive with a finite square (NaN is refused)");
  RSLO_CHECK_ARG(min_overlap >= 0.0 && min_overlap <= 1.0, "loop_verify: min_overlap must be in 0..1 (NaN is refused)");
  RSLO_CHECK_ARG(max_rms >= 0.0, "loop_verify: max_rms must be >= 0 (NaN is refused)");
  RSLO_CHECK_ARG(min_pairs >= 1, "loop_verify: min_pairs must be >= 1");
  RSLO_CHECK_ARG(damping == damping, "loop_verify: damping is NaN");
  P.max_distance = max_distance;
  P.inlier_dist = inlier_dist;
  P.min_overlap = min_overlap;
  P.max_rms = max_rms;
  P.damping = damping;
  P.min_pairs = min_pairs;
  const int threads = K < 1024 ? K : 1024;      // K is a multiple of 64: whole waves
  hipLaunchKernelGGL(k_loop_verify, dim3((unsigned)top_k), dim3((unsigned)threads), lv_lds_bytes(K, threads),
                     (hipStream_t)stream, (void *)store, store_bytes, (long long)capacity, K, frame, frame_info, cands, start, P,
                     out, info, matches);
  RSLO_CHECK_LAUNCH("loop_verify");
  return RSLO_OK;
}

extern "C" int rslo_loop_edges_reset(int32_t *ij, double *Z, double *w, int64_t *counters2, int max_edges, void *stream) {
  RSLO_CHECK_ARG(ij && Z && w && counters2, "loop_edges_reset: null pointer");
  RSLO_CHECK_ARG(max_edges >= 1 && max_edges <= LV_MAX_EDGES, "loop_edges_reset: max_edges must be in 1..4096");
  hipLaunchKernelGGL(k_loop_edges_reset, dim3((unsigned)rslo_cdiv(max_edges, 256)), dim3(256), 0, (hipStream_t)stream, ij, Z, w,
                     (long long *)counters2, max_edges);
  RSLO_CHECK_LAUNCH("loop_edges_reset");
  return RSLO_OK;
}

extern "C" int rslo_loop_emit(const double *out, int top_k, const void *store, size_t store_bytes, int64_t capacity, int K,
                              int32_t *ij, double *Z, double *w, int64_t *counters2, int max_edges, double w_t, double w_r,
                              void *stream) {
  KF_CHECK_STORE("loop_emit");
  RSLO_CHECK_ARG(out && ij && Z && w && counters2, "loop_emit: null pointer");
  RSLO_CHECK_ARG(top_k >= 1 && top_k <= LV_MAX_TOPK, "loop_emit: top_k must be in 1..16");
  RSLO_CHECK_ARG(max_edges >= 1 && max_edges <= LV_MAX_EDGES, "loop_emit: max_edges must be in 1..4096");
  RSLO_CHECK_ARG(w_t >= 0.0 && w_r >= 0.0 && w_t < (double)__builtin_inff() && w_r < (double)__builtin_inff(),
                 "loop_emit: the edge weights must be finite and >= 0");
  hipLaunchKernelGGL(k_loop_emit, dim3(1), dim3(64), 0, (hipStream_t)stream, out, top_k, (void *)store, store_bytes,
                     (long long)capacity, K, ij, Z, w, (long long *)counters2, max_edges, w_t, w_r);
  RSLO_CHECK_LAUNCH("loop_emit");
  return RSLO_OK;
}
