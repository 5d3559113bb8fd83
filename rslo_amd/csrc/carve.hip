// Free-space carving of the world voxel map (rules: include/rslo_hip.h "Free-space carving"; float64 restatement:
// rslo_amd/carve.py range_image_ref and rslo_amd/mapping.py VoxelMapRef.carve): a stored cell that the current scan looks
// straight THROUGH is evicted, which is what removes the trail a moving object leaves in a map that otherwise only fills.
//
// rslo_range_image bins a scan into an H x W image of the nearest range per pixel -- columns by azimuth (the reproducible
// arctangent of azimuth.h), rows by the TANGENT of the elevation, so no second arctangent is needed.  A pixel is the
// minimum, as uint32, of the bit patterns of float(r): positive floats order as their bits, and a minimum does not depend
// on arrival order, so the image is the restatement's to the bit.
// rslo_map_carve moves every stored cell into the sensor frame, finds its pixel by the same function, and evicts it when
// the nearest return in a small window about that pixel lies further than the cell by a margin.  The table is then
// rebuilt in place by the launches of rslo_map_prune (map_core.h): this file adds only the scan pass and the header
// update.  All arithmetic is IEEE double without contraction, in the order the header states.
#include "rslo_common.h"

#include <math.h>

#include "map_table.h"

#pragma clang fp contract(off)

#include "map_core.h"     /* the staging area and the rebuild launches of rslo_map_prune */
#include "azimuth.h"      /* after the pragma: uncontracted here, as in deskew.hip */

#define CARVE_EMPTY 0xFFFFFFFFu
#define CARVE_MAX_H 256
#define CARVE_MAX_W 4096
#define CARVE_MAX_WIN_ROWS 4
#define CARVE_MAX_WIN_COLS 8

// the pixel of a sensor-frame position with rho2 = x*x + y*y > 0 (the caller has it): false when its row is outside
// the image.  A NaN anywhere makes a comparison false, which is "no pixel".
__device__ __forceinline__ bool carve_pixel(double x, double y, double z, double rho2, int H, int W, double tan_lo,
                                            double tan_hi, int &row, int &col) {
  const double e = z / sqrt(rho2);
  const double u = ((e - tan_lo) / (tan_hi - tan_lo)) * (double)H;
  if (!(u >= 0.0 && u < (double)H)) return false;
  const double f = az_fraction(x, y, -0.5, 0);
  const int c = (int)floor(f * (double)W);
  col = c < W - 1 ? (c < 0 ? 0 : c) : W - 1;      // f can round to exactly 1 (and is never negative: the index stays inside)
  row = (int)floor(u);
  return true;
}

__global__ __launch_bounds__(256) void k_range_image_fill(uint32_t *__restrict__ img, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) img[i] = CARVE_EMPTY;
}

__global__ __launch_bounds__(256) void k_range_image(const float *__restrict__ points, int stride, int N, int H, int W,
                                                     double tan_lo, double tan_hi, uint32_t *__restrict__ img) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const float *p = points + (int64_t)i * stride;
  const float fx = p[0], fy = p[1], fz = p[2];
  const float inf = __builtin_inff();
  if (!(fabsf(fx) < inf && fabsf(fy) < inf && fabsf(fz) < inf)) return;      // NaN compares false
  const double x = (double)fx, y = (double)fy, z = (double)fz;
  const double rho2 = x * x + y * y;
  if (rho2 == 0.0) return;
  const double r = sqrt(rho2 + z * z);
  int row, col;
  if (!carve_pixel(x, y, z, rho2, H, W, tan_lo, tan_hi, row, col)) return;
  atomicMin(&img[row * W + col], __float_as_uint((float)r));
}

struct CarveArgs {
  int H, W, win_rows, win_cols, grace;
  double tan_lo, tan_hi, margin_abs, margin_rel, max_range;
};

// the rule, on one stored cell: true = evict.  Every comparison that is false keeps the cell.
__device__ __forceinline__ bool carve_evicts(const float4 r, map_u64 tag, long long last_scan, const double *t,
                                             const double *qc, const uint32_t *__restrict__ img, const CarveArgs &a) {
  if (!(last_scan - (long long)(tag >> 32) >= (long long)a.grace)) return false;
  const double d[3] = {(double)r.x - t[0], (double)r.y - t[1], (double)r.z - t[2]};
  double p[3];
  se3_rotate(qc, d, p);
  const double rho2 = p[0] * p[0] + p[1] * p[1];
  if (!(rho2 > 0.0)) return false;
  const double r_m = sqrt(rho2 + p[2] * p[2]);
  if (!(r_m < a.max_range)) return false;
  int row, col;
  if (!carve_pixel(p[0], p[1], p[2], rho2, a.H, a.W, a.tan_lo, a.tan_hi, row, col)) return false;
  if (img[row * a.W + col] == CARVE_EMPTY) return false;
  const int r0 = row - a.win_rows < 0 ? 0 : row - a.win_rows;
  const int r1 = row + a.win_rows > a.H - 1 ? a.H - 1 : row + a.win_rows;
  uint32_t m = CARVE_EMPTY;      // an empty pixel is the largest word: the minimum skips it by itself
  for (int rr = r0; rr <= r1; ++rr)
    for (int dc = -a.win_cols; dc <= a.win_cols; ++dc) {
      int cc = (col + dc) % a.W;      // |dc| <= 8 <= W
      cc = cc < 0 ? cc + a.W : cc;
      const uint32_t v = img[rr * a.W + cc];
      m = v < m ? v : m;
    }
  return (double)__uint_as_float(m) - r_m > a.margin_abs + a.margin_rel * r_m;
}

// pass 1 of the rebuild: keep or evict every stored cell.  A wave walks 64 adjacent slots at a time; the kept records of
// the 64 reach the staging area through a ballot, with ONE move of the cursor per wave (the scheme of
// k_surfel_prune_scan); the evicted ones are counted per workgroup and added to the control block once.
__global__ __launch_bounds__(256) void k_map_carve_scan(void *map, long long cap_max, const uint32_t *__restrict__ img,
                                                        const double *__restrict__ pose, CarveArgs a, void *ws) {
  __shared__ unsigned int gone_wg;
  if (threadIdx.x == 0) gone_wg = 0;
  __syncthreads();
  MapView m;
  if (!map_view(map, cap_max, m)) return;      // uniform over the grid
  const long long cap = m.hdr->capacity;       // a power of two >= 1024: every wave's 64 slots exist
  const PruneStage st = prune_stage(ws, cap);
  const long long last_scan = (long long)m.hdr->n_scans - 1;
  const double t[3] = {pose[0], pose[1], pose[2]};
  const double qc[4] = {pose[3], -pose[4], -pose[5], -pose[6]};      // the inverse rotation; q is not renormalised
  const int lane = threadIdx.x & 63;
  const map_u64 below = ((map_u64)1 << lane) - 1;      // the lanes in front of this one
  unsigned int gone = 0;
  for (long long s0 = (long long)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); s0 < cap;
       s0 += (long long)gridDim.x * blockDim.x) {
    const size_t s = (size_t)s0 + lane;
    const map_u64 key = m.keys[s];
    const bool stored = key != MAP_KEY_NONE;
    map_u64 tag = 0;
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    int32_t h = 0;
    bool evict = false;
    if (stored) {
      tag = m.tags[s];
      r = *(const float4 *)(m.rows + s * 4);
      h = m.hits[s];
      evict = carve_evicts(r, tag, last_scan, t, qc, img, a);
    }
    const bool keep = stored && !evict;
    const map_u64 kept = __ballot(keep);
    gone += (unsigned int)__popcll(__ballot(evict));
    if (kept == 0) continue;      // uniform over the wave
    map_u64 base = 0;
    if (lane == 0) base = atomicAdd(&st.ctl->kept, (map_u64)__popcll(kept));
    base = __shfl(base, 0, 64);
    const map_u64 o = base + (map_u64)__popcll(kept & below);
    if (keep && o < (map_u64)cap) {      // always: one record per slot at most, and the cursor starts at 0
      st.keys[o] = key;
      st.tags[o] = tag;
      st.rows[o] = r;
      st.hits[o] = h;
    }
  }
  if (lane == 0 && gone) atomicAdd(&gone_wg, gone);      // every lane of a wave counted the same slots
  __syncthreads();
  if (threadIdx.x == 0 && gone_wg) atomicAdd(&st.ctl->evicted, (map_u64)gone_wg);
}

__global__ void k_map_carve_done(void *map, long long cap_max, const void *ws) {
  MapView m;
  if (threadIdx.x != 0 || !map_view(map, cap_max, m)) return;
  const RebuildCtl *ctl = (const RebuildCtl *)ws;
  m.hdr->n_carves = m.hdr->n_carves + 1;
  if (ctl->evicted == 0) return;
  m.hdr->n_cells = ctl->kept - ctl->lost;
  m.hdr->n_carved = m.hdr->n_carved + ctl->evicted;
  m.hdr->n_lost = m.hdr->n_lost + ctl->lost;
}

static inline bool carve_finite(double v) { return fabs(v) < (double)__builtin_inff(); }

// the image arguments both calls share
static int carve_check_image(const char *name, int H, int W, double tan_lo, double tan_hi) {
  RSLO_CHECK_ARG(H >= 1 && H <= CARVE_MAX_H, "%s: H = %d must lie in 1 .. %d", name, H, CARVE_MAX_H);
  RSLO_CHECK_ARG(W >= 8 && W <= CARVE_MAX_W, "%s: W = %d must lie in 8 .. %d", name, W, CARVE_MAX_W);
  RSLO_CHECK_ARG(carve_finite(tan_lo) && carve_finite(tan_hi) && tan_lo < tan_hi,
                 "%s: need finite tan_lo < tan_hi", name);
  return RSLO_OK;
}

extern "C" int rslo_range_image(const float *points, int stride_floats, int N, int H, int W, double tan_lo, double tan_hi,
                                uint32_t *img, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  const int rc = carve_check_image("range_image", H, W, tan_lo, tan_hi);
  if (rc) return rc;
  RSLO_CHECK_ARG(stride_floats >= 3, "range_image: stride_floats < 3");
  RSLO_CHECK_ARG(N >= 0, "range_image: N < 0");
  RSLO_CHECK_ARG(img && (N == 0 || points), "range_image: null pointer");
  hipLaunchKernelGGL(k_range_image_fill, dim3((unsigned)rslo_cdiv(H * W, 256)), dim3(256), 0, s, img, H * W);
  // (N == 0: a grid of one workgroup whose threads all return -- two launches whatever the data)
  hipLaunchKernelGGL(k_range_image, dim3(N == 0 ? 1u : (unsigned)rslo_cdiv(N, 256)), dim3(256), 0, s, points, stride_floats,
                     N, H, W, tan_lo, tan_hi, img);
  RSLO_CHECK_LAUNCH("range_image");
  return RSLO_OK;
}

extern "C" size_t rslo_map_carve_ws_bytes(int64_t capacity) { return rslo_map_prune_ws_bytes(capacity); }

extern "C" int rslo_map_carve(void *map, size_t map_bytes, const uint32_t *img, int H, int W, double tan_lo, double tan_hi,
                              const double *pose7, int win_rows, int win_cols, double margin_abs, double margin_rel,
                              double max_range, int grace, void *ws, size_t ws_bytes, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  const long long cap_max = map_cap_of_bytes(map_bytes);
  RSLO_CHECK_ARG(map && cap_max > 0, "map_carve: no map (map_bytes below rslo_map_bytes(1024))");
  const int rc = carve_check_image("map_carve", H, W, tan_lo, tan_hi);
  if (rc) return rc;
  RSLO_CHECK_ARG(win_rows >= 0 && win_rows <= CARVE_MAX_WIN_ROWS && win_cols >= 0 && win_cols <= CARVE_MAX_WIN_COLS,
                 "map_carve: win_rows must lie in 0 .. %d and win_cols in 0 .. %d", CARVE_MAX_WIN_ROWS, CARVE_MAX_WIN_COLS);
  RSLO_CHECK_ARG(margin_abs >= 0.0 && margin_rel >= 0.0, "map_carve: the margins must be >= 0 (NaN is refused)");
  RSLO_CHECK_ARG(max_range > 0.0, "map_carve: max_range must be > 0 (NaN is refused)");
  RSLO_CHECK_ARG(grace >= 0, "map_carve: grace < 0");
  RSLO_CHECK_ARG(img && pose7, "map_carve: img or pose7 is null");
  RSLO_CHECK_ARG(ws && ((uintptr_t)ws & 15) == 0, "map_carve: the workspace is null or not 16-byte aligned");
  if (ws_bytes < rslo_map_carve_ws_bytes(cap_max)) {      // the header's capacity is at most cap_max
    rslo_set_error("map_carve: workspace too small");
    return RSLO_EWS;
  }
  CarveArgs a;
  a.H = H, a.W = W, a.win_rows = win_rows, a.win_cols = win_cols, a.grace = grace;
  a.tan_lo = tan_lo, a.tan_hi = tan_hi, a.margin_abs = margin_abs, a.margin_rel = margin_rel, a.max_range = max_range;
  map_rebuild_begin(ws, s);
  hipLaunchKernelGGL(k_map_carve_scan, dim3(table_blocks(cap_max)), dim3(256), 0, s, map, cap_max, img, pose7, a, ws);
  map_rebuild_table(map, cap_max, ws, s);
  hipLaunchKernelGGL(k_map_carve_done, dim3(1), dim3(64), 0, s, map, cap_max, (const void *)ws);
  RSLO_CHECK_LAUNCH("map_carve");
  return RSLO_OK;
}
