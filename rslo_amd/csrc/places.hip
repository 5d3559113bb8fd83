// Place recognition: a Scan Context descriptor per scan (Kim & Kim, IROS 2018), a device-resident database of them and
// a two-stage search (rules: include/rslo_hip.h "Place recognition"; float64 restatement: rslo_amd/places.py
// ScanContextRef / PlaceDBRef).  Nothing of the reference corresponds to it.
//
// One caller-owned allocation: header (256 bytes) | D f32 [N, R, S] | norm f64 [N, S] | key i32 [N, R], every section
// padded to 256 bytes.  Entries are only appended; the entry counter lives in the header and is read on the device.
//
// Reproducibility: a bin of the descriptor is a MAXIMUM of positive floats, taken as an integer maximum of their bit
// patterns (first in LDS, then into the zeroed global grid), so it does not depend on arrival order.  No transcendental
// function decides a bin: atan2f only guesses the sector, the two sign conditions on the cross products c_k decide it.
// Every sum of the search is a loop in the rule's order on one thread; selection compares integers (the ordered bit
// pattern of a distance, then the entry index), never floats of two threads in a race.
//
// Visibility: nothing here communicates across workgroups except through atomics on the descriptor grid / the counters
// and through kernel boundaries; a call is a fixed sequence of launches in stream order, without a host read.
#include "rslo_common.h"

#pragma clang fp contract(off)   /* the bin of a point and every distance must not depend on FMA formation */

typedef unsigned long long place_u64;

#define PLACE_MAGIC 0x52534c4f504c4331ull   /* "RSLOPLC1" */
#define PLACE_HDR_BYTES 256
#define PLACE_MAX_CAP ((int64_t)1 << 24)
#define PLACE_JC 16                          /* query columns per pass of the distance kernel */
#define PLACE_KEY_NONE 0xFFFFFFFFFFFFFFFFull
#define PLACE_TWO_PI 6.283185307179586

struct PlaceHdr {
  place_u64 magic;
  long long capacity, R, S;
  long long n_entries, dropped_full;
};

struct PlaceView {
  PlaceHdr *hdr;
  float *D;
  double *norm;
  int32_t *key;
};

static __host__ __device__ inline size_t place_pad(size_t b) { return (b + 255) / 256 * 256; }

static __host__ __device__ inline size_t place_bytes_of(long long cap, int R, int S) {
  return (size_t)PLACE_HDR_BYTES + place_pad((size_t)cap * R * S * 4) + place_pad((size_t)cap * S * 8) +
         place_pad((size_t)cap * R * 4);
}

// the database the caller says it is (capacity, R, S as handed to reset), or nothing at all
__device__ __forceinline__ bool place_view(void *db, size_t db_bytes, long long cap, int R, int S, PlaceView &v) {
  PlaceHdr *h = (PlaceHdr *)db;
  if (db_bytes < place_bytes_of(cap, R, S)) return false;
  if (h->magic != PLACE_MAGIC || h->capacity != cap || h->R != R || h->S != S) return false;
  unsigned char *p = (unsigned char *)db + PLACE_HDR_BYTES;
  v.hdr = h;
  v.D = (float *)p;
  p += place_pad((size_t)cap * R * S * 4);
  v.norm = (double *)p;
  p += place_pad((size_t)cap * S * 8);
  v.key = (int32_t *)p;
  return true;
}

// a double as an unsigned integer of the same order (-0.0 below +0.0; no NaN reaches it)
__device__ __forceinline__ place_u64 place_ordered(double d) {
  const place_u64 b = (place_u64)__double_as_longlong(d);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double place_unordered(place_u64 k) {
  const place_u64 b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
  return __longlong_as_double((long long)b);
}

// ---------------------------------------------------------------------------------------------------------------------
// describe
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_place_zero(uint32_t *__restrict__ D, int cells, place_u64 *__restrict__ counters) {
  for (int i = threadIdx.x; i < cells; i += blockDim.x) D[i] = 0u;
  if (threadIdx.x < 4) counters[threadIdx.x] = 0;
}

// dynamic LDS: dirs f64 [S + 1, 2] | edge2 f64 [R + 1] | grid u32 [R * S] | counts u32 [4]
__global__ __launch_bounds__(256) void k_place_describe(const float *__restrict__ points, int stride, int N, int R, int S,
                                                        const double *__restrict__ tables, float z_offset,
                                                        uint32_t *__restrict__ D, place_u64 *__restrict__ counters) {
  extern __shared__ double place_lds[];
  double *dirs = place_lds;
  double *edge2 = dirs + 2 * (S + 1);
  uint32_t *grid = (uint32_t *)(edge2 + (R + 1));
  uint32_t *counts = grid + R * S;
  const int n_tab = 2 * (S + 1) + (R + 1), cells = R * S;
  for (int i = threadIdx.x; i < n_tab; i += blockDim.x) place_lds[i] = tables[i];
  for (int i = threadIdx.x; i < cells; i += blockDim.x) grid[i] = 0u;
  if (threadIdx.x < 4) counts[threadIdx.x] = 0u;
  __syncthreads();
  const double r2_max = edge2[R];
  const float k_of_angle = (float)S * 0.15915494f;      // S / 2 pi: the guess only
  unsigned n_ok = 0, n_invalid = 0, n_range = 0, n_low = 0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
    const float *p = points + (int64_t)i * stride;
    const float fx = p[0], fy = p[1], fz = p[2];
    if (!(isfinite(fx) && isfinite(fy) && isfinite(fz))) {
      ++n_invalid;
      continue;
    }
    const double x = (double)fx, y = (double)fy;
    const double r2 = x * x + y * y;
    if (!(r2 > 0.0 && r2 < r2_max)) {
      ++n_range;
      continue;
    }
    int ring = 0;
    for (int k = 1; k < R; ++k) ring += (r2 >= edge2[k]) ? 1 : 0;
    // sector: the smallest k with c_k >= 0 and c_{k+1} < 0.  The guess and its two neighbours are tried first; each is
    // confirmed on the same c values as the scan over k would compute.
    float ang = atan2f(fy, fx);
    if (ang < 0.f) ang += 6.2831853f;
    int k0 = (int)(ang * k_of_angle);
    k0 = k0 < 0 ? 0 : (k0 > S - 1 ? S - 1 : k0);
    int sector = -1;
    {      // c at S is c at 0 (dirs[S] = dirs[0]), so a wrapped neighbour reads the same values as the scan would
      const int km = k0 == 0 ? S - 1 : k0 - 1, kp = k0 == S - 1 ? 0 : k0 + 1;
      const double cm = dirs[2 * km] * y - dirs[2 * km + 1] * x;
      const double c0 = dirs[2 * k0] * y - dirs[2 * k0 + 1] * x;
      const double c1 = dirs[2 * k0 + 2] * y - dirs[2 * k0 + 3] * x;
      const double c2 = dirs[2 * kp + 2] * y - dirs[2 * kp + 3] * x;
      if (c0 >= 0.0 && c1 < 0.0) sector = k0;
      else if (cm >= 0.0 && c0 < 0.0) sector = km;
      else if (c1 >= 0.0 && c2 < 0.0) sector = kp;
    }
    if (sector < 0) {      // the guess was not confirmed: the scan over k
      double ca = dirs[0] * y - dirs[1] * x;
      for (int k = 0; k < S; ++k) {
        const double cb = dirs[2 * k + 2] * y - dirs[2 * k + 3] * x;
        if (ca >= 0.0 && cb < 0.0) {
          sector = k;
          break;
        }
        ca = cb;
      }
    }
    if (sector < 0) {
      ++n_range;
      continue;
    }
    const float v = fz + z_offset;
    if (!(v > 0.f)) {
      ++n_low;
      continue;
    }
    ++n_ok;
    atomicMax(&grid[ring * S + sector], __float_as_uint(v));      // positive floats order as their bit patterns
  }
  atomicAdd(&counts[0], n_ok);
  atomicAdd(&counts[1], n_invalid);
  atomicAdd(&counts[2], n_range);
  atomicAdd(&counts[3], n_low);
  __syncthreads();
  for (int i = threadIdx.x; i < cells; i += blockDim.x) {
    const uint32_t v = grid[i];
    if (v) atomicMax(&D[i], v);
  }
  if (threadIdx.x < 4 && counts[threadIdx.x]) atomicAdd(&counters[threadIdx.x], (place_u64)counts[threadIdx.x]);
}

// behind the kernel boundary the grid is final: ring key and column norms, one thread per ring / per column
__global__ __launch_bounds__(128) void k_place_finish(const float *__restrict__ D, int R, int S, int32_t *__restrict__ key,
                                                      double *__restrict__ norm) {
  const int t = threadIdx.x;
  if (t < R) {
    int n = 0;
    for (int j = 0; j < S; ++j) n += D[t * S + j] > 0.f ? 1 : 0;
    key[t] = n;
  }
  if (t < S) {
    double acc = 0.0;
    for (int r = 0; r < R; ++r) {
      const double d = (double)D[r * S + t];
      acc = acc + d * d;
    }
    norm[t] = __dsqrt_rn(acc);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// database
// ---------------------------------------------------------------------------------------------------------------------
__global__ void k_place_reset(void *db, long long cap, int R, int S) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    PlaceHdr *h = (PlaceHdr *)db;
    h->magic = PLACE_MAGIC;
    h->capacity = cap;
    h->R = R;
    h->S = S;
    h->n_entries = 0;
    h->dropped_full = 0;
  }
}

__global__ __launch_bounds__(256) void k_place_add(void *db, size_t db_bytes, long long cap, int R, int S,
                                                   const float *__restrict__ D, const int32_t *__restrict__ key,
                                                   const double *__restrict__ norm) {
  PlaceView v;
  if (!place_view(db, db_bytes, cap, R, S, v)) return;
  const long long n = v.hdr->n_entries;      // constant during this launch: k_place_add_done bumps it
  if (n < 0 || n >= cap) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < R * S) v.D[(size_t)n * R * S + i] = D[i];
  if (i < S) v.norm[(size_t)n * S + i] = norm[i];
  if (i < R) v.key[(size_t)n * R + i] = key[i];
}

__global__ void k_place_add_done(void *db, size_t db_bytes, long long cap, int R, int S) {
  PlaceView v;
  if (threadIdx.x != 0 || !place_view(db, db_bytes, cap, R, S, v)) return;
  const long long n = v.hdr->n_entries;
  if (n >= 0 && n < cap) v.hdr->n_entries = n + 1;
  else v.hdr->dropped_full = v.hdr->dropped_full + 1;
}

// ---------------------------------------------------------------------------------------------------------------------
// query.  Workspace: control block (256 bytes: n_cand) | ring-key distances u64 [N] | candidates i32 [256] |
// distance keys u64 [N] | shifts i32 [N], every section padded to 256 bytes.
// ---------------------------------------------------------------------------------------------------------------------
#define PLACE_CTL_BYTES 256
struct PlaceWs {
  int32_t *n_cand;
  place_u64 *kd;
  int32_t *cand;
  place_u64 *dkey;
  int32_t *shift;
};

static __host__ __device__ inline size_t place_ws_bytes_of(long long cap) {
  return (size_t)PLACE_CTL_BYTES + place_pad((size_t)cap * 8) + 1024 + place_pad((size_t)cap * 8) + place_pad((size_t)cap * 4);
}

__device__ __forceinline__ PlaceWs place_ws(void *ws, long long cap) {
  unsigned char *p = (unsigned char *)ws;
  PlaceWs w;
  w.n_cand = (int32_t *)p;
  p += PLACE_CTL_BYTES;
  w.kd = (place_u64 *)p;
  p += place_pad((size_t)cap * 8);
  w.cand = (int32_t *)p;
  p += 1024;
  w.dkey = (place_u64 *)p;
  p += place_pad((size_t)cap * 8);
  w.shift = (int32_t *)p;
  return w;
}

__device__ __forceinline__ long long place_eligible(const PlaceHdr *h, long long exclude_recent) {
  const long long e = h->n_entries - exclude_recent;
  return e < 0 ? 0 : (e > h->capacity ? h->capacity : e);
}

// stage 1a: (kd << 32 | index) of every eligible entry
// kd = min(sum of squares, 2^32 - 1) for ANY int32 keys: |d| <= 2^32 - 1; a term of |d| >= 2^16 alone reaches the clamp
__global__ __launch_bounds__(256) void k_place_keys(void *db, size_t db_bytes, long long cap, int R, int S,
                                                    const int32_t *__restrict__ keyq, long long exclude_recent, void *ws) {
  PlaceView v;
  if (!place_view(db, db_bytes, cap, R, S, v)) return;
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= place_eligible(v.hdr, exclude_recent)) return;
  place_u64 kd = 0;
  for (int r = 0; r < R; ++r) {
    const long long d = (long long)keyq[r] - (long long)v.key[(size_t)e * R + r];
    const place_u64 a = (place_u64)(d < 0 ? -d : d);
    kd += a >= 65536ull ? 0x100000000ull : a * a;      // every term <= 2^32 and R <= 64: the sum stays < 2^39
  }
  if (kd > 0xFFFFFFFFull) kd = 0xFFFFFFFFull;      // a key is a count 0..S of an honest descriptor: kd <= R * S * S < 2^21
  place_ws(ws, cap).kd[e] = (kd << 32) | (place_u64)e;
}

// stage 1b: the C smallest composite keys, in order; one workgroup, one pass over the keys per candidate
__global__ __launch_bounds__(1024) void k_place_select(void *db, size_t db_bytes, long long cap, int R, int S,
                                                       long long exclude_recent, int C, void *ws) {
  __shared__ place_u64 red[1024];
  PlaceView v;
  if (!place_view(db, db_bytes, cap, R, S, v)) return;
  const PlaceWs w = place_ws(ws, cap);
  const long long E = place_eligible(v.hdr, exclude_recent);
  const int n_cand = (long long)C < E ? C : (int)E;
  place_u64 last = 0;
  for (int c = 0; c < n_cand; ++c) {
    place_u64 best = PLACE_KEY_NONE;
    for (long long e = threadIdx.x; e < E; e += blockDim.x) {
      const place_u64 k = w.kd[e];
      if ((c == 0 || k > last) && k < best) best = k;
    }
    red[threadIdx.x] = best;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s && red[threadIdx.x + s] < red[threadIdx.x]) red[threadIdx.x] = red[threadIdx.x + s];
      __syncthreads();
    }
    last = red[0];
    __syncthreads();
    if (threadIdx.x == 0) w.cand[c] = (int32_t)(last & 0xFFFFFFFFull);      // n_cand <= E: one is always found
  }
  if (threadIdx.x == 0) *w.n_cand = n_cand;
}

// stage 2: one workgroup per entry.  dynamic LDS: nq f64 [S] | ne f64 [S] | cosines f64 [JC, S] | red u64 [256] |
// De f32 [R, S] | Dq columns f32 [R, JC] | red shifts i32 [256]
__global__ __launch_bounds__(256) void k_place_dist(void *db, size_t db_bytes, long long cap, int R, int S,
                                                    const float *__restrict__ Dq, const double *__restrict__ normq,
                                                    long long exclude_recent, int C, void *ws) {
  extern __shared__ double place_lds[];
  PlaceView v;
  if (!place_view(db, db_bytes, cap, R, S, v)) return;
  const PlaceWs w = place_ws(ws, cap);
  long long e;
  if (C > 0) {
    if ((int)blockIdx.x >= *w.n_cand) return;
    e = w.cand[blockIdx.x];
  } else {
    e = blockIdx.x;
    if (e >= place_eligible(v.hdr, exclude_recent)) return;
  }
  double *nq = place_lds, *ne = nq + S, *cosm = ne + S;
  place_u64 *red = (place_u64 *)(cosm + PLACE_JC * S);
  float *De = (float *)(red + 256), *Dqc = De + R * S;
  int32_t *reds = (int32_t *)(Dqc + R * PLACE_JC);
  const int t = threadIdx.x;
  for (int i = t; i < R * S; i += 256) De[i] = v.D[(size_t)e * R * S + i];
  for (int i = t; i < S; i += 256) {
    nq[i] = normq[i];
    ne[i] = v.norm[(size_t)e * S + i];
  }
  double sum = 0.0;
  int n_valid = 0;
  for (int j0 = 0; j0 < S; j0 += PLACE_JC) {
    const int jc = S - j0 < PLACE_JC ? S - j0 : PLACE_JC;
    __syncthreads();      // the staging above; the previous pass's readers of cosm / Dqc
    for (int i = t; i < R * jc; i += 256) {
      const int r = i / jc, jj = i - r * jc;
      Dqc[r * PLACE_JC + jj] = Dq[r * S + j0 + jj];
    }
    __syncthreads();
    for (int i = t; i < jc * S; i += 256) {
      const int jj = i / S, jp = i - jj * S;
      double dot = 0.0;
      for (int r = 0; r < R; ++r) dot = dot + (double)Dqc[r * PLACE_JC + jj] * (double)De[r * S + jp];
      cosm[jj * S + jp] = dot / (nq[j0 + jj] * ne[jp]);      // read only where both norms are positive
    }
    __syncthreads();
    if (t < S) {      // shift t: its wrapped diagonal, j ascending
      for (int jj = 0; jj < jc; ++jj) {
        const int j = j0 + jj;
        int jp = j + t;
        jp = jp >= S ? jp - S : jp;
        if (nq[j] > 0.0 && ne[jp] > 0.0) {
          sum = sum + cosm[jj * S + jp];
          ++n_valid;
        }
      }
    }
  }
  place_u64 k = PLACE_KEY_NONE;
  if (t < S) k = place_ordered(n_valid > 0 ? 1.0 - sum / (double)n_valid : (double)__builtin_inff());
  red[t] = k;
  reds[t] = t;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {      // smallest distance, then smallest shift
    if (t < s) {
      const place_u64 ko = red[t + s];
      const int so = reds[t + s];
      if (ko < red[t] || (ko == red[t] && so < reds[t])) {
        red[t] = ko;
        reds[t] = so;
      }
    }
    __syncthreads();
  }
  if (t == 0) {
    w.dkey[e] = red[0];
    w.shift[e] = reds[0];
  }
}

// result: top_k rounds of "the smallest (distance, index) above the last one" over the stage-2 entries; one workgroup
__global__ __launch_bounds__(256) void k_place_topk(void *db, size_t db_bytes, long long cap, int R, int S,
                                                    long long exclude_recent, int C, int top_k, void *ws,
                                                    double *__restrict__ out) {
  __shared__ place_u64 red[256];
  __shared__ long long redi[256];
  PlaceView v;
  if (!place_view(db, db_bytes, cap, R, S, v)) return;
  const PlaceWs w = place_ws(ws, cap);
  const long long L = C > 0 ? (long long)*w.n_cand : place_eligible(v.hdr, exclude_recent);
  const place_u64 k_inf = place_ordered((double)__builtin_inff());
  const int t = threadIdx.x;
  place_u64 last_k = 0;
  long long last_i = -1;
  bool have = false, done = false;
  for (int row = 0; row < top_k; ++row) {
    place_u64 bk = PLACE_KEY_NONE;
    long long bi = -1;
    if (!done) {
      for (long long i = t; i < L; i += 256) {
        const long long e = C > 0 ? (long long)w.cand[i] : i;
        const place_u64 k = w.dkey[e];
        if (k >= k_inf) continue;
        if (have && (k < last_k || (k == last_k && e <= last_i))) continue;
        if (k < bk || (k == bk && e < bi)) {
          bk = k;
          bi = e;
        }
      }
    }
    red[t] = bk;
    redi[t] = bi;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (t < s) {
        const place_u64 ko = red[t + s];
        const long long io = redi[t + s];
        if (io >= 0 && (redi[t] < 0 || ko < red[t] || (ko == red[t] && io < redi[t]))) {
          red[t] = ko;
          redi[t] = io;
        }
      }
      __syncthreads();
    }
    bk = red[0];
    bi = redi[0];
    __syncthreads();
    if (bi < 0) {
      done = true;
      if (t == 0) {
        out[row * 4 + 0] = -1.0;
        out[row * 4 + 1] = (double)__builtin_inff();
        out[row * 4 + 2] = -1.0;
        out[row * 4 + 3] = 0.0;
      }
    } else {
      have = true;
      last_k = bk;
      last_i = bi;
      if (t == 0) {
        const int s = w.shift[bi];
        out[row * 4 + 0] = (double)bi;
        out[row * 4 + 1] = place_unordered(bk);
        out[row * 4 + 2] = (double)s;
        out[row * 4 + 3] = ((double)s * PLACE_TWO_PI) / (double)S;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------------
static inline bool place_shape_ok(int R, int S) { return R >= 1 && R <= 64 && S >= 3 && S <= 128; }

extern "C" size_t rslo_place_bytes(int64_t capacity, int R, int S) {
  if (capacity < 1 || capacity > PLACE_MAX_CAP || !place_shape_ok(R, S)) return 0;
  return place_bytes_of(capacity, R, S);
}

extern "C" int rslo_place_reset(void *db, size_t db_bytes, int64_t capacity, int R, int S, void *stream) {
  RSLO_CHECK_ARG(db && ((uintptr_t)db & 7) == 0, "place_reset: db is null or not 8-byte aligned");
  RSLO_CHECK_ARG(rslo_place_bytes(capacity, R, S) != 0, "place_reset: need capacity in 1 .. 2^24, R in 1..64, S in 3..128");
  RSLO_CHECK_ARG(db_bytes >= rslo_place_bytes(capacity, R, S), "place_reset: db_bytes is smaller than rslo_place_bytes");
  hipLaunchKernelGGL(k_place_reset, dim3(1), dim3(64), 0, (hipStream_t)stream, db, (long long)capacity, R, S);
  RSLO_CHECK_LAUNCH("place_reset");
  return RSLO_OK;
}

extern "C" int rslo_place_describe(const float *points, int stride_floats, int N, int R, int S, const double *tables,
                                   float z_offset, float *D, int32_t *key, double *norm, int64_t *counters4,
                                   void *stream) {
  hipStream_t s = (hipStream_t)stream;
  RSLO_CHECK_ARG(place_shape_ok(R, S), "place_describe: need R in 1..64 and S in 3..128");
  RSLO_CHECK_ARG(N >= 0 && stride_floats >= 3, "place_describe: N < 0 or stride_floats < 3");
  RSLO_CHECK_ARG(N == 0 || points, "place_describe: points is null");
  RSLO_CHECK_ARG(tables && D && key && norm && counters4, "place_describe: null pointer");
  RSLO_CHECK_ARG(z_offset == z_offset && z_offset > -__builtin_inff() && z_offset < __builtin_inff(),
                 "place_describe: z_offset must be finite");
  hipLaunchKernelGGL(k_place_zero, dim3(1), dim3(256), 0, s, (uint32_t *)D, R * S, (place_u64 *)counters4);
  if (N > 0) {
    int64_t nb = rslo_cdiv(N, 2048);
    nb = nb > 256 ? 256 : nb;
    const size_t lds = (size_t)(2 * (S + 1) + (R + 1)) * 8 + (size_t)(R * S + 4) * 4;
    hipLaunchKernelGGL(k_place_describe, dim3((unsigned)nb), dim3(256), lds, s, points, stride_floats, N, R, S, tables,
                       z_offset, (uint32_t *)D, (place_u64 *)counters4);
  }
  hipLaunchKernelGGL(k_place_finish, dim3(1), dim3(128), 0, s, (const float *)D, R, S, key, norm);
  RSLO_CHECK_LAUNCH("place_describe");
  return RSLO_OK;
}

extern "C" int rslo_place_add(void *db, size_t db_bytes, int64_t capacity, int R, int S, const float *D,
                              const int32_t *key, const double *norm, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  RSLO_CHECK_ARG(db && rslo_place_bytes(capacity, R, S) != 0 && db_bytes >= rslo_place_bytes(capacity, R, S),
                 "place_add: no database of this capacity, R and S (db_bytes below rslo_place_bytes)");
  RSLO_CHECK_ARG(D && key && norm, "place_add: null pointer");
  hipLaunchKernelGGL(k_place_add, dim3((unsigned)rslo_cdiv(R * S, 256)), dim3(256), 0, s, db, db_bytes, (long long)capacity,
                     R, S, D, key, norm);
  hipLaunchKernelGGL(k_place_add_done, dim3(1), dim3(64), 0, s, db, db_bytes, (long long)capacity, R, S);
  RSLO_CHECK_LAUNCH("place_add");
  return RSLO_OK;
}

extern "C" size_t rslo_place_query_ws_bytes(int64_t capacity) {
  if (capacity < 1 || capacity > PLACE_MAX_CAP) return 0;
  return place_ws_bytes_of(capacity);
}

extern "C" int rslo_place_query(const void *db, size_t db_bytes, int64_t capacity, int R, int S, const float *Dq,
                                const int32_t *keyq, const double *normq, int64_t exclude_recent, int num_candidates,
                                int top_k, double *out, void *ws, size_t ws_bytes, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  RSLO_CHECK_ARG(db && rslo_place_bytes(capacity, R, S) != 0 && db_bytes >= rslo_place_bytes(capacity, R, S),
                 "place_query: no database of this capacity, R and S (db_bytes below rslo_place_bytes)");
  RSLO_CHECK_ARG(Dq && keyq && normq && out, "place_query: null pointer");
  RSLO_CHECK_ARG(exclude_recent >= 0, "place_query: exclude_recent < 0");
  RSLO_CHECK_ARG(num_candidates >= 0 && num_candidates <= 256, "place_query: num_candidates must be in 0..256");
  RSLO_CHECK_ARG(top_k >= 1 && top_k <= 16, "place_query: top_k must be in 1..16");
  RSLO_CHECK_ARG(ws && ((uintptr_t)ws & 7) == 0, "place_query: the workspace is null or not 8-byte aligned");
  if (ws_bytes < rslo_place_query_ws_bytes(capacity)) {
    rslo_set_error("place_query: workspace too small");
    return RSLO_EWS;
  }
  void *d = (void *)db;
  const long long cap = capacity, ex = exclude_recent;
  const int C = num_candidates;
  if (C > 0) {
    hipLaunchKernelGGL(k_place_keys, dim3((unsigned)rslo_cdiv(cap, 256)), dim3(256), 0, s, d, db_bytes, cap, R, S, keyq, ex, ws);
    hipLaunchKernelGGL(k_place_select, dim3(1), dim3(1024), 0, s, d, db_bytes, cap, R, S, ex, C, ws);
  }
  const size_t lds = (size_t)(2 * S + PLACE_JC * S + 256) * 8 + (size_t)(R * S + R * PLACE_JC + 256) * 4;
  hipLaunchKernelGGL(k_place_dist, dim3((unsigned)(C > 0 ? C : cap)), dim3(256), lds, s, d, db_bytes, cap, R, S, Dq, normq,
                     ex, C, ws);
  hipLaunchKernelGGL(k_place_topk, dim3(1), dim3(256), 0, s, d, db_bytes, cap, R, S, ex, C, top_k, ws, out);
  RSLO_CHECK_LAUNCH("place_query");
  return RSLO_OK;
}
