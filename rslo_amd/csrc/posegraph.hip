// Pose-graph optimisation (rules: include/rslo_hip.h "Pose graph"; float64 restatement: rslo_amd/posegraph.py
// PoseGraphRef): Gauss-Newton over a chain of N poses with L loop edges, each step solved by conjugate gradients
// preconditioned with the chain's own Hessian.
//
// Launches of one Gauss-Newton iteration:
//   k_pg_edges   parallel over the N-1+L edges: residual, Jacobian blocks, robust weight, per-edge gradient parts and, for
//                a chain edge, the closed-form inverse of B_k, into one record of PG_EREC doubles per edge; for a loop
//                edge also its cleaned (i, j) and its rank among the earlier valid loops at the same node;
//   k_pg_solve   ONE workgroup of 1024 threads: gradient per node, the segment transfer matrices of the chain scan and
//                the whole preconditioned CG, with its loop and its early stop inside the kernel; writes the info row;
//   k_pg_update  parallel over the nodes: T' = T o (rho, phi) when the solve produced a step.
//
// Inside the solve every vector lives in the workspace (6N doubles do not fit LDS at the top sizes) and is handed
// between threads of the one workgroup through __syncthreads(), which orders global writes inside a workgroup.  Sums
// into a node come in a fixed order: chain edge n-1, chain edge n, then the loops at that node by ascending index (one
// barrier-separated round per rank).  Dot products are one fixed tree: a strided partial per thread, a shuffle tree per
// wave, the 16 waves in order.  No floating-point atomic anywhere: two runs give the same bits.
//
// Applying M^-1 = J_c^-1 J_c^-T is two block-bidiagonal solves, each a linear recurrence v' = T_k v + c_k over 6-vectors.
// Thread s owns a contiguous segment of the chain: a local pass with zero input gives the segment's offset, a
// Kogge-Stone scan over the <= 1024 (transfer matrix, offset) summaries gives every segment's input, a second local pass
// runs the recurrence with it.  The transfer matrices and their per-level products depend on the linearisation alone:
// they are made once per Gauss-Newton iteration.  Dependent depth: 2 * segment length + log2(segments) levels.
#include "rslo_common.h"

#include <math.h>

#pragma clang fp contract(off)

#include "se3.h"      /* the pose algebra, after the pragma: uncontracted here */
#include "gauss_newton.h"      /* gn_block_sum: the fixed-order workgroup sum, after the pragma and after se3.h */

#define PG_THREADS 1024
#define PG_EREC 84                       /* doubles per edge record (RSLO_PG_EDGE_DOUBLES) */
#define PG_HDR 256                       /* bytes: int32 words, see below */
#define PG_MAX_NODES 65536
#define PG_MAX_LOOPS 4096
#define PG_MAX_GN 32
#define PG_MAX_CG 256

// record: r[6] | rho | flag (1 used, 0 skipped, 2 singular chain edge) | Att Atr Arr Btt Brr (3 x 3 each, row-major)
//         | gi[6] gj[6] | e | Binv_tt Binv_rr (chain edges)
#define PG_R 0
#define PG_RHO 6
#define PG_FLAG 7
#define PG_ATT 8
#define PG_ATR 17
#define PG_ARR 26
#define PG_BTT 35
#define PG_BRR 44
#define PG_GI 53
#define PG_GJ 59
#define PG_E 65
#define PG_BITT 66
#define PG_BIRR 75

// header words
#define PG_H_CONV 0                      /* an earlier iteration met the tolerances */
#define PG_H_OK 1                        /* the solve of this iteration produced a step */
#define PG_H_N 2                         /* N and L of the linearisation the workspace holds */
#define PG_H_L 3
#define PG_H_MAXRANK 4

struct PgWs {
  int N, L, E, len, nseg, nlev;
  int32_t *hdr, *lij, *rank;
  double *rec, *g, *x, *r, *z, *p, *Ap, *y, *Pf, *Pb;
};

static size_t pg_pad(size_t b) { return (b + 255) / 256 * 256; }

// carve the workspace; returns the bytes needed
static size_t pg_layout(int N, int L, void *ws, PgWs *o) {
  PgWs w;
  w.N = N, w.L = L, w.E = N - 1;
  w.len = (int)rslo_cdiv(w.E, PG_THREADS);
  w.nseg = (int)rslo_cdiv(w.E, w.len);
  w.nlev = rslo_log2_i64(w.nseg);
  unsigned char *b = (unsigned char *)ws;
  size_t off = 0;
  w.hdr = (int32_t *)(b + off), off += PG_HDR;
  w.lij = (int32_t *)(b + off), off += pg_pad((size_t)2 * (L + 1) * 4);
  w.rank = (int32_t *)(b + off), off += pg_pad((size_t)2 * (L + 1) * 4);
  w.rec = (double *)(b + off), off += pg_pad((size_t)(w.E + L) * PG_EREC * 8);
  double **vecs[7] = {&w.g, &w.x, &w.r, &w.z, &w.p, &w.Ap, &w.y};
  for (int k = 0; k < 7; ++k) *vecs[k] = (double *)(b + off), off += pg_pad((size_t)N * 6 * 8);
  const size_t lev = pg_pad((size_t)(w.nlev + 1) * w.nseg * 36 * 8);
  w.Pf = (double *)(b + off), off += lev;
  w.Pb = (double *)(b + off), off += lev;
  if (o) *o = w;
  return off;
}

__device__ __forceinline__ bool pg_finite(double v) { return fabs(v) < (double)__builtin_inff(); }

// o = M v, o = M^T v for a row-major 3 x 3 in memory
__device__ __forceinline__ void pg_mv3(const double *M, const double *v, double *o) {
  for (int a = 0; a < 3; ++a) o[a] = M[a * 3] * v[0] + M[a * 3 + 1] * v[1] + M[a * 3 + 2] * v[2];
}
__device__ __forceinline__ void pg_mtv3(const double *M, const double *v, double *o) {
  for (int a = 0; a < 3; ++a) o[a] = M[a] * v[0] + M[3 + a] * v[1] + M[6 + a] * v[2];
}

// the four products with the blocks of a record: A x, A^T u, B x, B^T u (A = [[Att, Atr], [0, Arr]], B = diag(Btt, Brr))
__device__ __forceinline__ void pg_A(const double *rec, const double *x, double *o) {
  double a[3], b[3];
  pg_mv3(rec + PG_ATT, x, a);
  pg_mv3(rec + PG_ATR, x + 3, b);
  for (int i = 0; i < 3; ++i) o[i] = a[i] + b[i];
  pg_mv3(rec + PG_ARR, x + 3, o + 3);
}
__device__ __forceinline__ void pg_At(const double *rec, const double *u, double *o) {
  double a[3], b[3];
  pg_mtv3(rec + PG_ATT, u, o);
  pg_mtv3(rec + PG_ATR, u, a);
  pg_mtv3(rec + PG_ARR, u + 3, b);
  for (int i = 0; i < 3; ++i) o[3 + i] = a[i] + b[i];
}
__device__ __forceinline__ void pg_B(const double *rec, const double *x, double *o) {
  pg_mv3(rec + PG_BTT, x, o);
  pg_mv3(rec + PG_BRR, x + 3, o + 3);
}
__device__ __forceinline__ void pg_Bt(const double *rec, const double *u, double *o) {
  pg_mtv3(rec + PG_BTT, u, o);
  pg_mtv3(rec + PG_BRR, u + 3, o + 3);
}

// ---------------------------------------------------------------------------------------------------------------------
// edges
// ---------------------------------------------------------------------------------------------------------------------
// a loop row is used when i, j are nodes, differ, every value is finite, the quaternion is not zero, no weight negative
__device__ __forceinline__ bool pg_loop_valid(const int32_t *ij, const double *Z, const double *w, int l, int N) {
  const int i = ij[2 * l], j = ij[2 * l + 1];
  if (i < 0 || j < 0 || i >= N || j >= N || i == j) return false;
  const double *z = Z + (size_t)l * 7, *ww = w + (size_t)l * 2;
  for (int a = 0; a < 7; ++a)
    if (!pg_finite(z[a])) return false;
  const double n2 = z[3] * z[3] + z[4] * z[4] + z[5] * z[5] + z[6] * z[6];
  if (!(n2 > 0.0) || !pg_finite(n2)) return false;
  return pg_finite(ww[0]) && pg_finite(ww[1]) && ww[0] >= 0.0 && ww[1] >= 0.0;
}

__global__ __launch_bounds__(256) void k_pg_edges(const double *__restrict__ traj0, const double *__restrict__ poses,
                                                  PgWs ws, double cwt, double cwr, const double *__restrict__ cw_dev,
                                                  const int32_t *__restrict__ ij, const double *__restrict__ Zl,
                                                  const double *__restrict__ wl, double s2, int iter) {
  if (iter > 0 && ws.hdr[PG_H_CONV]) return;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= ws.E + ws.L) return;
  double *rec = ws.rec + (size_t)e * PG_EREC;
  const bool chain = e < ws.E;
  int i, j;
  double Z[7], wt, wr;
  bool valid = true;
  if (chain) {
    i = e, j = e + 1;
    se3_between(traj0 + (size_t)i * 7, traj0 + (size_t)j * 7, Z);
    wt = cw_dev ? cw_dev[2 * e] : cwt;
    wr = cw_dev ? cw_dev[2 * e + 1] : cwr;
  } else {
    const int l = e - ws.E;
    valid = pg_loop_valid(ij, Zl, wl, l, ws.N);
    int rk[2] = {-1, -1};
    if (valid) {
      i = ij[2 * l], j = ij[2 * l + 1];
      const double *z = Zl + (size_t)l * 7;
      const double nz = sqrt(z[3] * z[3] + z[4] * z[4] + z[5] * z[5] + z[6] * z[6]);
      for (int a = 0; a < 3; ++a) Z[a] = z[a];
      for (int a = 0; a < 4; ++a) Z[3 + a] = z[3 + a] / nz;
      wt = wl[2 * l], wr = wl[2 * l + 1];
      // rank of this loop at each of its nodes among the earlier valid loops (the order of the sums into a node)
      // (the fixed node receives no sum: its side keeps rank -1 and costs no round)
      rk[0] = i > 0 ? 0 : -1, rk[1] = j > 0 ? 0 : -1;
      for (int m = 0; m < l; ++m) {
        const int mi = ij[2 * m], mj = ij[2 * m + 1];
        const bool hi = i > 0 && (mi == i || mj == i), hj = j > 0 && (mi == j || mj == j);
        if ((hi || hj) && pg_loop_valid(ij, Zl, wl, m, ws.N)) rk[0] += hi, rk[1] += hj;
      }
    }
    ws.lij[2 * l] = valid ? i : -1, ws.lij[2 * l + 1] = valid ? j : -1;
    ws.rank[2 * l] = rk[0], ws.rank[2 * l + 1] = rk[1];
    if (!valid) {
      for (int a = 0; a < PG_EREC; ++a) rec[a] = 0.0;
      return;
    }
  }
  double A[7], E[7], RZ[9], RA[9], RE[9];
  se3_between(poses + (size_t)i * 7, poses + (size_t)j * 7, A);
  se3_between(Z, A, E);
  const double s = E[3] >= 0.0 ? 1.0 : -1.0;
  se3_rotmat(Z + 3, RZ);
  se3_rotmat(A + 3, RA);
  se3_rotmat(E + 3, RE);
  const double G[9] = {s * E[3], s * -E[6], s * E[5], s * E[6], s * E[3], s * -E[4], s * -E[5], s * E[4], s * E[3]};
  const double S[9] = {0.0, -A[2], A[1], A[2], 0.0, -A[0], -A[1], A[0], 0.0};      // [t_A]x
  double r[6];
  for (int a = 0; a < 3; ++a) {
    r[a] = wt * E[a];
    r[3 + a] = wr * (2.0 * s * E[4 + a]);
  }
  const double e2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3] + r[4] * r[4] + r[5] * r[5];
  double rho = 1.0;
  if (!chain && s2 > 0.0) {
    const double u = s2 / (s2 + e2);
    rho = u * u;
  }
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      // R_Z^T [t_A]x and G R_A^T
      const double zs = RZ[0 * 3 + a] * S[0 * 3 + b] + RZ[1 * 3 + a] * S[1 * 3 + b] + RZ[2 * 3 + a] * S[2 * 3 + b];
      const double ga = G[a * 3 + 0] * RA[b * 3 + 0] + G[a * 3 + 1] * RA[b * 3 + 1] + G[a * 3 + 2] * RA[b * 3 + 2];
      rec[PG_ATT + a * 3 + b] = -wt * RZ[b * 3 + a];
      rec[PG_ATR + a * 3 + b] = wt * zs;
      rec[PG_ARR + a * 3 + b] = -wr * ga;
      rec[PG_BTT + a * 3 + b] = wt * RE[a * 3 + b];
      rec[PG_BRR + a * 3 + b] = wr * G[a * 3 + b];
    }
  double gi[6], gj[6];
  pg_At(rec, r, gi);
  pg_Bt(rec, r, gj);
  for (int a = 0; a < 6; ++a) {
    rec[PG_R + a] = r[a];
    rec[PG_GI + a] = rho * gi[a];
    rec[PG_GJ + a] = rho * gj[a];
  }
  rec[PG_RHO] = rho;
  rec[PG_E] = e2;
  double flag = 1.0;
  if (chain) {
    // B_k^-1 = diag(R_E^T / w_t, G^-1 / w_r), G^-1 = (w w I - w [v]x + v v^T) / (s w (w w + v.v))
    const double w = E[3], *v = E + 4;
    const double den = s * w * (w * w + (v[0] * v[0] + v[1] * v[1] + v[2] * v[2]));
    const double V[9] = {0.0, -v[2], v[1], v[2], 0.0, -v[0], -v[1], v[0], 0.0};
    bool ok = pg_finite(e2);
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) {
        const double it = RE[b * 3 + a] / wt;
        const double ir = ((a == b ? w * w : 0.0) - w * V[a * 3 + b] + v[a] * v[b]) / den / wr;
        ok = ok && pg_finite(it) && pg_finite(ir);
        rec[PG_BITT + a * 3 + b] = it;
        rec[PG_BIRR + a * 3 + b] = ir;
      }
    if (!ok) flag = 2.0;
  } else {
    for (int a = PG_BITT; a < PG_EREC; ++a) rec[a] = 0.0;
  }
  rec[PG_FLAG] = flag;
}

// ---------------------------------------------------------------------------------------------------------------------
// the pieces of the one-workgroup solve.  Every piece starts with a barrier, so that what other threads wrote before
// it is visible, and all of them are called by all 1024 threads in uniform control flow.
// ---------------------------------------------------------------------------------------------------------------------
struct PgShared {
  double v[6][PG_THREADS];               // the scan's segment summaries, component-major
  double red[PG_THREADS / 64];
  int imax;
};

__device__ double pg_block_sum(double v, PgShared &sh) { return gn_block_sum(v, sh.red, PG_THREADS / 64); }

__device__ double pg_block_max(double v, PgShared &sh) {
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh.red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = sh.red[0];
  for (int q = 1; q < PG_THREADS / 64; ++q) t = fmax(t, sh.red[q]);
  return t;
}

__device__ double pg_dot(const PgWs &ws, const double *a, const double *b, PgShared &sh) {
  __syncthreads();
  double acc = 0.0;
  for (int k = threadIdx.x; k < ws.N * 6; k += PG_THREADS) acc = acc + a[k] * b[k];
  return pg_block_sum(acc, sh);
}

// the loops' additions into out[node]: entry 2l + side of a used loop adds in the round of its rank at that node
template <typename F>
__device__ void pg_loop_rounds(const PgWs &ws, double *out, F contribution) {
  const int maxrank = ws.hdr[PG_H_MAXRANK];
  for (int round = 0; round <= maxrank; ++round) {
    __syncthreads();
    for (int en = threadIdx.x; en < 2 * ws.L; en += PG_THREADS) {
      if (ws.rank[en] != round) continue;
      const int node = ws.lij[en];
      if (node <= 0) continue;             // a skipped loop, or the fixed node
      double c[6];
      contribution(en >> 1, en & 1, c);
      for (int a = 0; a < 6; ++a) out[(size_t)node * 6 + a] = out[(size_t)node * 6 + a] + c[a];
    }
  }
}

// y = (H_chain + H_loops + damping I) x; row 0 of x is taken as zero, row 0 of y is written zero
__device__ void pg_matvec(const PgWs &ws, const double *x, double *y, double damping) {
  __syncthreads();
  for (int n = threadIdx.x; n < ws.N; n += PG_THREADS) {
    double o[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (n > 0) {
      double xn[6], u[6], t[6];
      for (int a = 0; a < 6; ++a) xn[a] = x[(size_t)n * 6 + a], o[a] = damping * xn[a];
      const double *rk = ws.rec + (size_t)(n - 1) * PG_EREC;      // chain edge n-1: node n is its j
      pg_B(rk, xn, u);
      if (n > 1) {
        pg_A(rk, x + (size_t)(n - 1) * 6, t);
        for (int a = 0; a < 6; ++a) u[a] = t[a] + u[a];
      }
      pg_Bt(rk, u, t);
      for (int a = 0; a < 6; ++a) o[a] = o[a] + t[a];
      if (n < ws.E) {                                              // chain edge n: node n is its i
        const double *rn = ws.rec + (size_t)n * PG_EREC;
        pg_A(rn, xn, u);
        pg_B(rn, x + (size_t)(n + 1) * 6, t);
        for (int a = 0; a < 6; ++a) u[a] = u[a] + t[a];
        pg_At(rn, u, t);
        for (int a = 0; a < 6; ++a) o[a] = o[a] + t[a];
      }
    }
    for (int a = 0; a < 6; ++a) y[(size_t)n * 6 + a] = o[a];
  }
  pg_loop_rounds(ws, y, [&](int l, int side, double *c) {
    const double *rl = ws.rec + (size_t)(ws.E + l) * PG_EREC;
    const int i = ws.lij[2 * l], j = ws.lij[2 * l + 1];
    double u[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, t[6];
    if (i > 0) pg_A(rl, x + (size_t)i * 6, u);
    if (j > 0) {
      pg_B(rl, x + (size_t)j * 6, t);
      for (int a = 0; a < 6; ++a) u[a] = u[a] + t[a];
    }
    if (side == 0) pg_At(rl, u, t); else pg_Bt(rl, u, t);
    for (int a = 0; a < 6; ++a) c[a] = rl[PG_RHO] * t[a];
  });
}

// one Kogge-Stone scan over the summaries in sh.v with the per-level matrices P [nlev+1][nseg][36]: afterwards sh.v[.][s]
// is the recurrence's value at the end of segment s given zero input to segment 0
__device__ void pg_scan(const PgWs &ws, const double *P, PgShared &sh) {
  const int s = threadIdx.x;
  for (int d = 0; d < ws.nlev; ++d) {
    const int off = 1 << d;
    double o[6];
    __syncthreads();
    const bool act = s < ws.nseg && s >= off;
    if (act) {
      const double *M = P + ((size_t)d * ws.nseg + s) * 36;
      double in[6];
      for (int a = 0; a < 6; ++a) in[a] = sh.v[a][s - off];
      for (int a = 0; a < 6; ++a) {
        double acc = M[a * 6] * in[0];
        for (int b = 1; b < 6; ++b) acc = acc + M[a * 6 + b] * in[b];
        o[a] = acc + sh.v[a][s];
      }
    }
    __syncthreads();
    if (act)
      for (int a = 0; a < 6; ++a) sh.v[a][s] = o[a];
  }
  __syncthreads();
}

// y_k from y_{k+1}:  B_k^-T (r_{k+1} - A_{k+1}^T y_{k+1}), the A term absent for the last edge
__device__ __forceinline__ void pg_back(const PgWs &ws, const double *r, int k, double *cur) {
  const double *rk = ws.rec + (size_t)k * PG_EREC;
  double rhs[6], t[6];
  for (int a = 0; a < 6; ++a) rhs[a] = r[(size_t)(k + 1) * 6 + a];
  if (k + 1 < ws.E) {
    pg_At(rk + PG_EREC, cur, t);
    for (int a = 0; a < 6; ++a) rhs[a] = rhs[a] - t[a];
  }
  pg_mtv3(rk + PG_BITT, rhs, cur);
  pg_mtv3(rk + PG_BIRR, rhs + 3, cur + 3);
}

// z_{k+1} from z_k:  B_k^-1 (y_k - A_k z_k), the A term absent for edge 0 (node 0 is fixed)
__device__ __forceinline__ void pg_fwd(const PgWs &ws, const double *y, int k, double *cur) {
  const double *rk = ws.rec + (size_t)k * PG_EREC;
  double rhs[6], t[6];
  for (int a = 0; a < 6; ++a) rhs[a] = y[(size_t)k * 6 + a];
  if (k > 0) {
    pg_A(rk, cur, t);
    for (int a = 0; a < 6; ++a) rhs[a] = rhs[a] - t[a];
  }
  pg_mv3(rk + PG_BITT, rhs, cur);
  pg_mv3(rk + PG_BIRR, rhs + 3, cur + 3);
}

// z = M^-1 r (rows 1..N-1; row 0 of z is written zero).  ws.y holds the intermediate, one row per chain edge.
__device__ void pg_chain_solve(const PgWs &ws, const double *r, double *z, PgShared &sh) {
  const int s = threadIdx.x;
  const bool own = s < ws.nseg;
  const int k0 = s * ws.len, k1 = min(ws.E, k0 + ws.len);
  const int sr = ws.nseg - 1 - s;          // the backward scan runs from the last segment down
  double cur[6];
  __syncthreads();
  if (own) {
    for (int a = 0; a < 6; ++a) cur[a] = 0.0;
    for (int k = k1 - 1; k >= k0; --k) pg_back(ws, r, k, cur);
    for (int a = 0; a < 6; ++a) sh.v[a][sr] = cur[a];
  }
  pg_scan(ws, ws.Pb, sh);
  if (own)
    for (int a = 0; a < 6; ++a) cur[a] = sr > 0 ? sh.v[a][sr - 1] : 0.0;
  __syncthreads();
  if (own) {
    for (int k = k1 - 1; k >= k0; --k) {
      pg_back(ws, r, k, cur);
      for (int a = 0; a < 6; ++a) ws.y[(size_t)k * 6 + a] = cur[a];
    }
    // forward: the y rows of this segment are this thread's own
    for (int a = 0; a < 6; ++a) cur[a] = 0.0;
    for (int k = k0; k < k1; ++k) pg_fwd(ws, ws.y, k, cur);
    for (int a = 0; a < 6; ++a) sh.v[a][s] = cur[a];
  }
  pg_scan(ws, ws.Pf, sh);
  if (own)
    for (int a = 0; a < 6; ++a) cur[a] = s > 0 ? sh.v[a][s - 1] : 0.0;
  __syncthreads();
  if (own)
    for (int k = k0; k < k1; ++k) {
      pg_fwd(ws, ws.y, k, cur);
      for (int a = 0; a < 6; ++a) z[(size_t)(k + 1) * 6 + a] = cur[a];
    }
  if (s < 6) z[s] = 0.0;
}

// M (row-major 6 x 6 in memory) <- T M, column by column
__device__ __forceinline__ void pg_left_mul(const double *T, double *M) {
  for (int c = 0; c < 6; ++c) {
    double col[6], o[6];
    for (int a = 0; a < 6; ++a) col[a] = M[a * 6 + c];
    for (int a = 0; a < 6; ++a) {
      double acc = T[a * 6] * col[0];
      for (int b = 1; b < 6; ++b) acc = acc + T[a * 6 + b] * col[b];
      o[a] = acc;
    }
    for (int a = 0; a < 6; ++a) M[a * 6 + c] = o[a];
  }
}

// everything that depends on the linearisation alone: the loops' largest rank, the gradient per node, the sums and the
// scan's matrices.  sums4 = {cost, chain part, loops used, loops skipped}; returns true when a chain edge is singular.
__device__ bool pg_prepare(const PgWs &ws, PgShared &sh, double *sums4, bool matrices) {
  const int tid = threadIdx.x;
  if (tid == 0) sh.imax = 0;
  __syncthreads();
  int used = 0, mr = 0;
  for (int en = tid; en < 2 * ws.L; en += PG_THREADS) {
    mr = max(mr, ws.rank[en]);
    used += (en & 1) == 0 && ws.lij[en] >= 0;
  }
  if (mr > 0) atomicMax(&sh.imax, mr);
  __syncthreads();
  // the words that say "this workspace holds a linearisation of (N, L)" are cleared here and set again only at the end,
  // once the scan's matrices exist: rslo_posegraph_cost and a singular chain leave them cleared
  if (tid == 0) ws.hdr[PG_H_MAXRANK] = sh.imax, ws.hdr[PG_H_N] = 0, ws.hdr[PG_H_L] = 0;
  // sums in a fixed order: a strided partial per thread over the edges, then the block tree
  double cost = 0.0, chain = 0.0, bad = 0.0;
  for (int e = tid; e < ws.E + ws.L; e += PG_THREADS) {
    const double *rec = ws.rec + (size_t)e * PG_EREC;
    if (rec[PG_FLAG] == 0.0) continue;
    const double c = rec[PG_RHO] * rec[PG_E];
    cost = cost + c;
    if (e < ws.E) chain = chain + c;
    if (rec[PG_FLAG] == 2.0) bad = 1.0;
  }
  cost = pg_block_sum(cost, sh);
  chain = pg_block_sum(chain, sh);
  bad = pg_block_max(bad, sh);
  const double usedd = pg_block_sum((double)used, sh);      // small integers: exact
  if (sums4) {
    sums4[0] = cost, sums4[1] = chain, sums4[2] = usedd, sums4[3] = (double)ws.L - usedd;
  }
  // gradient: chain edge n-1 (as j), chain edge n (as i), then the loops by rank
  for (int n = tid; n < ws.N; n += PG_THREADS) {
    double o[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (n > 0) {
      const double *rk = ws.rec + (size_t)(n - 1) * PG_EREC;
      for (int a = 0; a < 6; ++a) o[a] = rk[PG_GJ + a];
      if (n < ws.E)
        for (int a = 0; a < 6; ++a) o[a] = o[a] + rk[PG_EREC + PG_GI + a];
    }
    for (int a = 0; a < 6; ++a) ws.g[(size_t)n * 6 + a] = o[a];
  }
  pg_loop_rounds(ws, ws.g, [&](int l, int side, double *c) {
    const double *rl = ws.rec + (size_t)(ws.E + l) * PG_EREC + (side ? PG_GJ : PG_GI);
    for (int a = 0; a < 6; ++a) c[a] = rl[a];
  });
  __syncthreads();
  if (!matrices || bad != 0.0) return bad != 0.0;
  // level 0: the transfer matrix of each segment, forward F_k = -B_k^-1 A_k (k ascending) and backward
  // G_k = -B_k^-T A_{k+1}^T (k descending, stored at the reversed segment index)
  if (tid < ws.nseg) {
    const int k0 = tid * ws.len, k1 = min(ws.E, k0 + ws.len);
    double *Pf = ws.Pf + (size_t)tid * 36, *Pb = ws.Pb + (size_t)(ws.nseg - 1 - tid) * 36;
    for (int a = 0; a < 36; ++a) Pf[a] = Pb[a] = (a % 7 == 0) ? 1.0 : 0.0;
    double T[36];
    for (int k = k0; k < k1; ++k) {
      const double *rk = ws.rec + (size_t)k * PG_EREC;
      for (int c = 0; c < 6; ++c) {          // column c of -B^-1 A
        double ec[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, t[6], o[6];
        ec[c] = 1.0;
        pg_A(rk, ec, t);
        pg_mv3(rk + PG_BITT, t, o);
        pg_mv3(rk + PG_BIRR, t + 3, o + 3);
        for (int a = 0; a < 6; ++a) T[a * 6 + c] = k > 0 ? -o[a] : 0.0;
      }
      pg_left_mul(T, Pf);
    }
    for (int k = k1 - 1; k >= k0; --k) {
      const double *rk = ws.rec + (size_t)k * PG_EREC;
      for (int c = 0; c < 6; ++c) {          // column c of -B^-T A_{k+1}^T
        double ec[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, t[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, o[6];
        ec[c] = 1.0;
        if (k + 1 < ws.E) pg_At(rk + PG_EREC, ec, t);
        pg_mtv3(rk + PG_BITT, t, o);
        pg_mtv3(rk + PG_BIRR, t + 3, o + 3);
        for (int a = 0; a < 6; ++a) T[a * 6 + c] = -o[a];
      }
      pg_left_mul(T, Pb);
    }
  }
  // level d + 1: P_s <- P_s P_{s - 2^d} for s >= 2^d (what the scan's later levels multiply with)
  for (int d = 0; d < ws.nlev; ++d) {
    __syncthreads();
    const int off = 1 << d;
    if (tid < ws.nseg)
      for (int dir = 0; dir < 2; ++dir) {
        const double *src = (dir ? ws.Pb : ws.Pf) + (size_t)d * ws.nseg * 36;
        double *dst = (dir ? ws.Pb : ws.Pf) + (size_t)(d + 1) * ws.nseg * 36 + (size_t)tid * 36;
        if (tid >= off) {
          for (int a = 0; a < 36; ++a) dst[a] = src[(size_t)(tid - off) * 36 + a];
          pg_left_mul(src + (size_t)tid * 36, dst);
        } else {
          for (int a = 0; a < 36; ++a) dst[a] = src[(size_t)tid * 36 + a];
        }
      }
  }
  __syncthreads();
  if (tid == 0) ws.hdr[PG_H_N] = ws.N, ws.hdr[PG_H_L] = ws.L;
  return false;
}

struct PgSolve {
  int iter, cg_iters;
  double cg_tol, damping, tol_t, tol_r;
};

__global__ __launch_bounds__(PG_THREADS) void k_pg_solve(PgWs ws, PgSolve sp, double *__restrict__ info) {
  __shared__ PgShared sh;
  const int tid = threadIdx.x;
  double *row = info + (size_t)sp.iter * 8;
  if (sp.iter > 0 && ws.hdr[PG_H_CONV]) {      // uniform: every thread reads the same word before anyone writes it
    if (tid < 8) row[tid] = tid == 0 ? 3.0 : 0.0;
    __syncthreads();
    if (tid == 0) ws.hdr[PG_H_OK] = 0;
    return;
  }
  __shared__ double sums[4];
  const bool singular = pg_prepare(ws, sh, tid == 0 ? sums : nullptr, true);
  __syncthreads();
  const int n6 = ws.N * 6;
  int status = 0, iters = 0;
  double rz0 = 0.0, rz = 0.0;
  for (int k = tid; k < n6; k += PG_THREADS) ws.x[k] = 0.0, ws.r[k] = -ws.g[k];
  if (singular) {
    status = 2;
  } else {
    pg_chain_solve(ws, ws.r, ws.z, sh);
    rz0 = rz = pg_dot(ws, ws.r, ws.z, sh);
    if (rz0 == 0.0) {
      status = 0;                              // g == 0: a zero step
    } else if (!(rz0 > 0.0 && pg_finite(rz0))) {
      status = 2;
    } else {
      for (int k = tid; k < n6; k += PG_THREADS) ws.p[k] = ws.z[k];
      for (int it = 0; it < sp.cg_iters; ++it) {
        pg_matvec(ws, ws.p, ws.Ap, sp.damping);
        const double pAp = pg_dot(ws, ws.p, ws.Ap, sh);
        if (!(pAp > 0.0 && pg_finite(pAp))) break;
        const double alpha = rz / pAp;
        for (int k = tid; k < n6; k += PG_THREADS) {
          ws.x[k] = ws.x[k] + alpha * ws.p[k];
          ws.r[k] = ws.r[k] - alpha * ws.Ap[k];
        }
        ++iters;
        pg_chain_solve(ws, ws.r, ws.z, sh);
        const double rzn = pg_dot(ws, ws.r, ws.z, sh);
        if (rzn <= sp.cg_tol * sp.cg_tol * rz0) {
          rz = rzn;
          break;
        }
        const double beta = rzn / rz;
        for (int k = tid; k < n6; k += PG_THREADS) ws.p[k] = ws.z[k] + beta * ws.p[k];
        rz = rzn;
      }
      if (iters == 0) status = 2;
    }
  }
  __syncthreads();
  // the largest |rho| and |phi| of the step; a step that is not finite is no step
  double mt = 0.0, mr = 0.0, bad = 0.0;
  for (int n = tid; n < ws.N; n += PG_THREADS) {
    const double *x = ws.x + (size_t)n * 6;
    const double a = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]), b = sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5]);
    if (!(pg_finite(a) && pg_finite(b))) bad = 1.0;
    else mt = fmax(mt, a), mr = fmax(mr, b);
  }
  mt = pg_block_max(mt, sh);
  mr = pg_block_max(mr, sh);
  bad = pg_block_max(bad, sh);
  if (bad != 0.0) status = 2;
  if (status != 0) mt = mr = 0.0;
  if (tid == 0) {
    ws.hdr[PG_H_OK] = status == 0;
    ws.hdr[PG_H_CONV] = (status == 0 && mt < sp.tol_t && mr < sp.tol_r) ? 1 : 0;
    row[0] = (double)status;
    row[1] = sums[2];
    row[2] = sums[0];
    row[3] = (double)iters;
    row[4] = rz0 > 0.0 ? sqrt(fmax(rz, 0.0) / rz0) : 0.0;
    row[5] = mt;
    row[6] = mr;
    row[7] = sums[3];
  }
}

__global__ __launch_bounds__(256) void k_pg_update(PgWs ws, double *__restrict__ poses) {
  if (!ws.hdr[PG_H_OK]) return;
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n < 1 || n >= ws.N) return;
  const double *x = ws.x + (size_t)n * 6;
  double *T = poses + (size_t)n * 7;
  const double th = sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5]);
  double dq[4], d[3], q[4];
  se3_dquat(x + 3, th, dq);
  se3_rotate(T + 3, x, d);
  se3_qmul(T + 3, dq, q);
  const double nr = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int a = 0; a < 3; ++a) T[a] = T[a] + d[a];
  for (int a = 0; a < 4; ++a) T[3 + a] = q[a] / nr;
}

// the pieces alone (rslo_posegraph_linearize / _cost / _matvec / _chain_solve): the same device functions, one workgroup
__global__ __launch_bounds__(PG_THREADS) void k_pg_prepare(PgWs ws, double *__restrict__ sums4, double *__restrict__ g_out,
                                                           int matrices) {
  __shared__ PgShared sh;
  __shared__ double sums[4];
  pg_prepare(ws, sh, threadIdx.x == 0 ? sums : nullptr, matrices != 0);
  __syncthreads();
  if (threadIdx.x < 4) sums4[threadIdx.x] = sums[threadIdx.x];
  if (g_out)
    for (int k = threadIdx.x; k < ws.N * 6; k += PG_THREADS) g_out[k] = ws.g[k];
}

__global__ __launch_bounds__(PG_THREADS) void k_pg_matvec(PgWs ws, const double *__restrict__ x, double *__restrict__ y,
                                                          double damping) {
  if (ws.hdr[PG_H_N] != ws.N || ws.hdr[PG_H_L] != ws.L) return;      // no linearisation of this graph in the workspace
  pg_matvec(ws, x, y, damping);
}

__global__ __launch_bounds__(PG_THREADS) void k_pg_chain(PgWs ws, const double *__restrict__ r, double *__restrict__ z) {
  __shared__ PgShared sh;
  if (ws.hdr[PG_H_N] != ws.N || ws.hdr[PG_H_L] != ws.L) return;
  pg_chain_solve(ws, r, z, sh);
}

__global__ void k_pose_between(const double *__restrict__ A, const double *__restrict__ B, int n, double *__restrict__ out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  double o[7];
  se3_between(A + (size_t)k * 7, B + (size_t)k * 7, o);
  for (int a = 0; a < 7; ++a) out[(size_t)k * 7 + a] = o[a];
}

// ---------------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------------
extern "C" size_t rslo_posegraph_ws_bytes(int N, int L) {
  if (N < 2 || N > PG_MAX_NODES || L < 0 || L > PG_MAX_LOOPS) return 0;
  return pg_layout(N, L, nullptr, nullptr);
}

struct PgGraph {      // the arguments every call shares
  const double *traj0, *poses;
  int N;
  const double *cw_host, *cw_dev;
  const int32_t *ij;
  const double *Z, *w;
  int L;
  double scale;
};

static int pg_check(const char *name, const PgGraph &g, void *ws, size_t ws_bytes, PgWs *lay) {
  RSLO_CHECK_ARG(g.N >= 2 && g.N <= PG_MAX_NODES, "%s: N must be in 2 .. 65536", name);
  RSLO_CHECK_ARG(g.L >= 0 && g.L <= PG_MAX_LOOPS, "%s: L must be in 0 .. 4096", name);
  RSLO_CHECK_ARG(g.traj0 && g.poses, "%s: traj0 or poses is null", name);
  RSLO_CHECK_ARG(g.cw_dev || g.cw_host, "%s: no chain weights (a host pair or a device [N-1,2] array)", name);
  RSLO_CHECK_ARG(g.cw_dev || (g.cw_host[0] > 0.0 && g.cw_host[1] > 0.0 && g.cw_host[0] < (double)__builtin_inff() &&
                              g.cw_host[1] < (double)__builtin_inff()),
                 "%s: the chain weights must be positive and finite", name);
  RSLO_CHECK_ARG(g.L == 0 || (g.ij && g.Z && g.w), "%s: L > 0 with a null loop array", name);
  const double s2 = g.scale * g.scale;
  RSLO_CHECK_ARG(g.scale == 0.0 || (g.scale > 0.0 && s2 > 0.0 && s2 < (double)__builtin_inff()),
                 "%s: robust_scale must be 0 (no weights) or positive with a finite, non-zero square", name);
  RSLO_CHECK_ARG(ws && !((uintptr_t)ws & 7), "%s: the workspace is null or not 8-byte aligned", name);
  if (ws_bytes < pg_layout(g.N, g.L, ws, lay)) {
    rslo_set_error("%s: workspace too small", name);
    return RSLO_EWS;
  }
  return RSLO_OK;
}

static void pg_launch_edges(const PgGraph &g, const PgWs &ws, int iter, hipStream_t s) {
  const int n = ws.E + ws.L;
  hipLaunchKernelGGL(k_pg_edges, dim3((unsigned)rslo_cdiv(n, 256)), dim3(256), 0, s, g.traj0, g.poses, ws,
                     g.cw_host ? g.cw_host[0] : 0.0, g.cw_host ? g.cw_host[1] : 0.0, g.cw_dev, g.ij, g.Z, g.w,
                     g.scale * g.scale, iter);
}

extern "C" int rslo_posegraph_optimize(const double *traj0, double *poses, int N, const double *chain_w2_host,
                                       const double *chain_w_dev, const int32_t *loops_ij, const double *loops_Z,
                                       const double *loops_w, int L, int gn_iters, int cg_iters, double cg_tol,
                                       double robust_scale, double damping, double tol_t, double tol_r, double *info,
                                       void *ws, size_t ws_bytes, void *stream) {
  const char *name = "posegraph_optimize";
  const PgGraph g = {traj0, poses, N, chain_w2_host, chain_w_dev, loops_ij, loops_Z, loops_w, L, robust_scale};
  PgWs lay;
  RSLO_CHECK_ARG(gn_iters >= 1 && gn_iters <= PG_MAX_GN, "%s: gn_iters must be in 1 .. 32", name);
  RSLO_CHECK_ARG(cg_iters >= 1 && cg_iters <= PG_MAX_CG, "%s: cg_iters must be in 1 .. 256", name);
  RSLO_CHECK_ARG(cg_tol >= 0.0 && cg_tol < (double)__builtin_inff(), "%s: cg_tol must be >= 0 and finite", name);
  RSLO_CHECK_ARG(damping >= 0.0 && damping < (double)__builtin_inff(), "%s: damping must be >= 0 and finite", name);
  RSLO_CHECK_ARG(tol_t >= 0.0 && tol_r >= 0.0, "%s: tol_t and tol_r must be >= 0 (NaN is refused)", name);
  RSLO_CHECK_ARG(info, "%s: info is null", name);
  const int rc = pg_check(name, g, ws, ws_bytes, &lay);
  if (rc) return rc;
  for (int it = 0; it < gn_iters; ++it) {
    pg_launch_edges(g, lay, it, (hipStream_t)stream);
    const PgSolve sp = {it, cg_iters, cg_tol, damping, tol_t, tol_r};
    hipLaunchKernelGGL(k_pg_solve, dim3(1), dim3(PG_THREADS), 0, (hipStream_t)stream, lay, sp, info);
    hipLaunchKernelGGL(k_pg_update, dim3((unsigned)rslo_cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, lay, poses);
  }
  RSLO_CHECK_LAUNCH(name);
  return RSLO_OK;
}

extern "C" int rslo_posegraph_linearize(const double *traj0, const double *poses, int N, const double *chain_w2_host,
                                        const double *chain_w_dev, const int32_t *loops_ij, const double *loops_Z,
                                        const double *loops_w, int L, double robust_scale, double *edges_out,
                                        double *g_out, double *sums4, void *ws, size_t ws_bytes, void *stream) {
  const char *name = "posegraph_linearize";
  const PgGraph g = {traj0, poses, N, chain_w2_host, chain_w_dev, loops_ij, loops_Z, loops_w, L, robust_scale};
  PgWs lay;
  RSLO_CHECK_ARG(sums4, "%s: sums4 is null", name);
  const int rc = pg_check(name, g, ws, ws_bytes, &lay);
  if (rc) return rc;
  pg_launch_edges(g, lay, 0, (hipStream_t)stream);
  hipLaunchKernelGGL(k_pg_prepare, dim3(1), dim3(PG_THREADS), 0, (hipStream_t)stream, lay, sums4, g_out, 1);
  if (edges_out)
    RSLO_HIP(hipMemcpyAsync(edges_out, lay.rec, (size_t)(lay.E + L) * PG_EREC * 8, hipMemcpyDeviceToDevice,
                            (hipStream_t)stream));
  RSLO_CHECK_LAUNCH(name);
  return RSLO_OK;
}

extern "C" int rslo_posegraph_cost(const double *traj0, const double *poses, int N, const double *chain_w2_host,
                                   const double *chain_w_dev, const int32_t *loops_ij, const double *loops_Z,
                                   const double *loops_w, int L, double robust_scale, double *out4, void *ws,
                                   size_t ws_bytes, void *stream) {
  const char *name = "posegraph_cost";
  const PgGraph g = {traj0, poses, N, chain_w2_host, chain_w_dev, loops_ij, loops_Z, loops_w, L, robust_scale};
  PgWs lay;
  RSLO_CHECK_ARG(out4, "%s: out4 is null", name);
  const int rc = pg_check(name, g, ws, ws_bytes, &lay);
  if (rc) return rc;
  pg_launch_edges(g, lay, 0, (hipStream_t)stream);
  hipLaunchKernelGGL(k_pg_prepare, dim3(1), dim3(PG_THREADS), 0, (hipStream_t)stream, lay, out4, (double *)nullptr, 0);
  RSLO_CHECK_LAUNCH(name);
  return RSLO_OK;
}

static int pg_check_piece(const char *name, int N, int L, const void *a, const void *b, void *ws, size_t ws_bytes,
                          PgWs *lay) {
  RSLO_CHECK_ARG(N >= 2 && N <= PG_MAX_NODES && L >= 0 && L <= PG_MAX_LOOPS, "%s: N must be in 2 .. 65536, L in 0 .. 4096",
                 name);
  RSLO_CHECK_ARG(a && b, "%s: null pointer", name);
  RSLO_CHECK_ARG(ws && !((uintptr_t)ws & 7), "%s: the workspace is null or not 8-byte aligned", name);
  if (ws_bytes < pg_layout(N, L, ws, lay)) {
    rslo_set_error("%s: workspace too small", name);
    return RSLO_EWS;
  }
  return RSLO_OK;
}

extern "C" int rslo_posegraph_matvec(const double *x, double *y, int N, int L, double damping, void *ws, size_t ws_bytes,
                                     void *stream) {
  PgWs lay;
  RSLO_CHECK_ARG(damping >= 0.0 && damping < (double)__builtin_inff(), "posegraph_matvec: damping must be >= 0 and finite");
  RSLO_CHECK_ARG(x != y, "posegraph_matvec: x and y must not alias");
  const int rc = pg_check_piece("posegraph_matvec", N, L, x, y, ws, ws_bytes, &lay);
  if (rc) return rc;
  hipLaunchKernelGGL(k_pg_matvec, dim3(1), dim3(PG_THREADS), 0, (hipStream_t)stream, lay, x, y, damping);
  RSLO_CHECK_LAUNCH("posegraph_matvec");
  return RSLO_OK;
}

extern "C" int rslo_posegraph_chain_solve(const double *r, double *z, int N, int L, void *ws, size_t ws_bytes,
                                          void *stream) {
  PgWs lay;
  RSLO_CHECK_ARG(r != z, "posegraph_chain_solve: r and z must not alias");
  const int rc = pg_check_piece("posegraph_chain_solve", N, L, r, z, ws, ws_bytes, &lay);
  if (rc) return rc;
  hipLaunchKernelGGL(k_pg_chain, dim3(1), dim3(PG_THREADS), 0, (hipStream_t)stream, lay, r, z);
  RSLO_CHECK_LAUNCH("posegraph_chain_solve");
  return RSLO_OK;
}

extern "C" int rslo_pose_between(const double *A, const double *B, int n, double *out, void *stream) {
  RSLO_CHECK_ARG(A && B && out && n >= 0, "rslo_pose_between: bad arguments");
  if (n == 0) return RSLO_OK;
  hipLaunchKernelGGL(k_pose_between, dim3((unsigned)rslo_cdiv(n, 64)), dim3(64), 0, (hipStream_t)stream, A, B, n, out);
  RSLO_CHECK_LAUNCH("rslo_pose_between");
  return RSLO_OK;
}
