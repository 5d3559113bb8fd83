"""Pose-graph optimisation: close loops over a trajectory.

    pg = PoseGraph(capacity=8192, max_loops=256)
    Z = pg.between(traj[i_rows], registered)                     # loop measurements without a host trip
    poses, info = pg.optimize(traj0, loops_ij, loops_Z, loops_w, gn_iters=6, robust_scale=3.0)
    runner = inference.OdometryRunner(net, pose_graph=pg)
    runner.close_loops(loops_ij, loops_Z); runner.optimized_trajectory()

PoseGraph is the device side (csrc/posegraph.hip); PoseGraphRef restates the rules of include/rslo_hip.h "Pose graph"
in float64 numpy on host arrays and is the arbiter of the tests.  The rules in one place:

  * poses and their algebra (compose, between, rotate, retract ...) are those of rslo_amd/se3.py, re-exported here;
  * N nodes, node 0 fixed; chain edge k joins k and k + 1 with Z_k = traj0[k]^-1 o traj0[k+1] and weights (w_t, w_r), one
    pair or [N-1, 2]; loop edge l = (i, j, Z, (w_t, w_r)) with Z the pose of j in the frame of i, its quaternion divided
    by its norm on read.  A loop row is skipped and counted when i < 0, i or j >= N, i == j, a value is not finite, the
    quaternion is zero or a weight is negative;
  * residual of (i, j, Z): A = T_i^-1 o T_j, E = Z^-1 o A, s = +1 if q_E.w >= 0 else -1,
    r = (w_t t_E, w_r 2 s vec(q_E));
  * local parametrisation T' = T o (rho, phi): t' = t + rotate(q, rho), q' = (q (x) dq(phi)) / |.|,
    dq = (1, phi / 2) when |phi| < 1e-12, else (cos(|phi| / 2), sin(|phi| / 2) / |phi| * phi);
  * Jacobians, with G = s (q_E.w I + [vec q_E]x): d r_t / d rho_j = R_E, d r_r / d phi_j = G, d r_t / d rho_i = -R_Z^T,
    d r_t / d phi_i = R_Z^T [t_A]x, d r_r / d phi_i = -G R_A^T, rows scaled by the weights;
  * robust weight of a loop edge: e = r.r, u = s2 / (s2 + e), rho = u u (scale 0: rho = 1); H += rho J^T J,
    g += rho J^T r, cost += rho e.  Chain edges always have rho = 1;
  * a Gauss-Newton iteration solves (H_chain + H_loops + damping I) x = -g over nodes 1..N-1 by conjugate gradients
    preconditioned with M = H_chain = J_c^T J_c, J_c block lower-bidiagonal: M^-1 is a backward and a forward block
    recurrence.  CG stops when r.z <= cg_tol^2 (r.z)_0, after cg_iters iterations, or without applying the iteration
    when p.Ap is not a positive finite number.

Vectors over the nodes are [N, 6] with row 0 (the fixed node) zero.

Loop measurements come from the caller or from rslo_amd/loops.py (a keyframe store and a geometric check whose edge list
this optimiser reads as it is).  Feeding the corrected poses back into a runner's refined chain and voxel map is
OdometryRunner.adopt_loop_closure() / rebuild_map() (rslo_amd/inference.py, over VoxelMap.insert_frames).
"""
import numpy as np

INFO_COLS = ("status", "loops_used", "cost", "cg_iters", "cg_residual", "max_rho", "max_phi", "loops_skipped")
MAX_NODES, MAX_LOOPS, MAX_GN, MAX_CG = 65536, 4096, 32, 256
SEGMENTS = 1024                 # threads of the solve kernel = segments of the chain scan


from .se3 import qmul, qconj, rotate, rotmat, skew, compose, inverse, between, dquat, retract  # noqa: F401


def residual(Ti, Tj, Z, w):
    """weighted residual [..., 6] of edges (T_i, T_j, Z) with weights w [..., 2]"""
    E = between(Z, between(Ti, Tj))
    s = np.where(E[..., 3:4] >= 0.0, 1.0, -1.0)
    return np.concatenate([w[..., :1] * E[..., :3], w[..., 1:2] * (2.0 * s * E[..., 4:])], -1)


def jacobians(Ti, Tj, Z, w):
    """(r [..., 6], Ji [..., 6, 6], Jj [..., 6, 6]): the weighted residual and its derivatives with respect to the local
    increments of node i and node j"""
    A = between(Ti, Tj)
    E = between(Z, A)
    s = np.where(E[..., 3] >= 0.0, 1.0, -1.0)[..., None, None]
    wt, wr = w[..., 0, None, None], w[..., 1, None, None]
    RZt = np.swapaxes(rotmat(Z[..., 3:]), -1, -2)
    RA, RE = rotmat(A[..., 3:]), rotmat(E[..., 3:])
    G = s * (E[..., 3, None, None] * np.eye(3) + skew(E[..., 4:]))
    Ji = np.zeros(A.shape[:-1] + (6, 6))
    Jj = np.zeros(A.shape[:-1] + (6, 6))
    Ji[..., :3, :3] = -wt * RZt
    Ji[..., :3, 3:] = wt * (RZt @ skew(A[..., :3]))
    Ji[..., 3:, 3:] = -wr * (G @ np.swapaxes(RA, -1, -2))
    Jj[..., :3, :3] = wt * RE
    Jj[..., 3:, 3:] = wr * G
    r = np.concatenate([w[..., :1] * E[..., :3], w[..., 1:2] * (2.0 * s[..., 0] * E[..., 4:])], -1)
    return r, Ji, Jj


def gj_inverse(qE, s):
    """closed-form inverse of G = s (w I + [v]x): (w w I - w [v]x + v v^T) / (s w (w w + v.v)); inf / nan when w == 0"""
    w, v = qE[..., 0, None, None], qE[..., 1:]
    vv = v[..., :, None] * v[..., None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        return (w * w * np.eye(3) - w * skew(v) + vv) / (s * w * (w * w + (v * v).sum(-1)[..., None, None]))


def check_scale(scale):
    s2 = float(scale) * float(scale)
    if not (scale == 0.0 or (scale > 0.0 and s2 > 0.0 and np.isfinite(s2))):
        raise ValueError("posegraph: robust_scale must be 0 (no weights) or positive with a finite, non-zero square")
    return float(scale)


def check_sizes(N, L):
    if int(N) != N or not 2 <= N <= MAX_NODES:
        raise ValueError("posegraph: N must be an integer in 2..65536, got %r" % (N,))
    if int(L) != L or not 0 <= L <= MAX_LOOPS:
        raise ValueError("posegraph: L must be an integer in 0..4096, got %r" % (L,))
    return int(N), int(L)


def check_options(gn_iters, cg_iters, cg_tol, robust_scale, damping, tol_t, tol_r):
    if int(gn_iters) != gn_iters or not 1 <= gn_iters <= MAX_GN:
        raise ValueError("posegraph: gn_iters must be an integer in 1..32")
    if int(cg_iters) != cg_iters or not 1 <= cg_iters <= MAX_CG:
        raise ValueError("posegraph: cg_iters must be an integer in 1..256")
    if not (cg_tol >= 0.0 and np.isfinite(cg_tol)):
        raise ValueError("posegraph: cg_tol must be >= 0 and finite")
    check_scale(robust_scale)
    if not (damping >= 0.0 and np.isfinite(damping)):
        raise ValueError("posegraph: damping must be >= 0 and finite")
    if not (tol_t >= 0.0 and tol_r >= 0.0):
        raise ValueError("posegraph: tol_t and tol_r must be >= 0 (NaN is refused)")


def segment_length(n_edges, segments=SEGMENTS):
    """edges per segment of the chain scan: the smallest length with which `segments` segments cover the chain"""
    return max(1, -(-int(n_edges) // int(segments)))


class Linearization:
    """What one linearisation holds.  Edges are numbered chain 0..N-2, then loops N-1..N-2+L.
    r [E, 6] weighted residuals, rho [E], valid [E] bool, Ji / Jj [E, 6, 6], i / j [E], g [N, 6], cost, chain_cost,
    loops_used, loops_skipped, singular (a chain edge with q_E.w == 0 or a zero weight), Binv [N-1, 6, 6]."""


class PoseGraphRef:
    """The rules on host arrays.  Methods mirror PoseGraph's; dense() and synthetic_graph() are for the tests."""

    def __init__(self, capacity=MAX_NODES, max_loops=MAX_LOOPS):
        self.capacity, self.max_loops = check_sizes(capacity, max_loops)

    between = staticmethod(between)

    # -- edges -----------------------------------------------------------------------------------------------------
    @staticmethod
    def _loops(N, loops_ij, loops_Z, loops_w):
        ij = np.zeros((0, 2), np.int32) if loops_ij is None else np.asarray(loops_ij, np.int32).reshape(-1, 2)
        L = len(ij)
        Z = np.zeros((0, 7)) if loops_Z is None else np.asarray(loops_Z, np.float64).reshape(-1, 7)
        w = np.ones((L, 2)) if loops_w is None else np.asarray(loops_w, np.float64).reshape(-1, 2)
        if len(Z) != L or len(w) != L:
            raise ValueError("posegraph: loops_ij, loops_Z and loops_w must have the same number of rows")
        check_sizes(N, L)
        i, j = ij[:, 0].astype(np.int64), ij[:, 1].astype(np.int64)
        with np.errstate(invalid="ignore", over="ignore"):
            n2 = (Z[:, 3:] * Z[:, 3:]).sum(1)
            valid = (i >= 0) & (j >= 0) & (i < N) & (j < N) & (i != j) & np.isfinite(Z).all(1) & np.isfinite(w).all(1) \
                & (w >= 0.0).all(1) & (n2 > 0.0) & np.isfinite(n2)
            Zn = Z.copy()
            Zn[valid, 3:] = Z[valid, 3:] / np.sqrt(n2[valid])[:, None]
        Zn[~valid] = (0, 0, 0, 1, 0, 0, 0)
        return np.where(valid, i, 0), np.where(valid, j, 1), Zn, np.where(valid[:, None], w, 0.0), valid

    @staticmethod
    def _chain_w(N, chain_w):
        w = np.asarray((1.0, 1.0) if chain_w is None else chain_w, np.float64)
        if w.shape == (2,):
            w = np.tile(w, (N - 1, 1))
        if w.shape != (N - 1, 2):
            raise ValueError("posegraph: chain_w must be a pair or [N-1, 2]")
        return w

    def linearize(self, traj0, poses, chain_w=None, loops_ij=None, loops_Z=None, loops_w=None, robust_scale=0.0):
        traj0, poses = np.asarray(traj0, np.float64), np.asarray(poses, np.float64)
        N = len(traj0)
        check_sizes(N, 0)
        scale = check_scale(robust_scale)
        li, lj, lZ, lw, lvalid = self._loops(N, loops_ij, loops_Z, loops_w)
        cw = self._chain_w(N, chain_w)
        lin = Linearization()
        lin.N, lin.L = N, len(li)
        k = np.arange(N - 1)
        lin.i = np.concatenate([k, li])
        lin.j = np.concatenate([k + 1, lj])
        Z = np.concatenate([between(traj0[:-1], traj0[1:]), lZ])
        w = np.concatenate([cw, lw])
        lin.valid = np.concatenate([np.ones(N - 1, bool), lvalid])
        with np.errstate(invalid="ignore", over="ignore"):
            lin.r, lin.Ji, lin.Jj = jacobians(poses[lin.i], poses[lin.j], Z, w)
            e = (lin.r * lin.r).sum(1)
            rho = np.ones(len(e))
            if scale > 0.0:
                s2 = scale * scale
                u = s2 / (s2 + e[N - 1:])
                rho[N - 1:] = u * u
        rho[~lin.valid] = 0.0
        lin.r[~lin.valid] = 0.0
        lin.Ji[~lin.valid] = 0.0
        lin.Jj[~lin.valid] = 0.0
        lin.rho, lin.e = rho, np.where(lin.valid, e, 0.0)
        lin.gi = rho[:, None] * np.einsum("eab,ea->eb", lin.Ji, lin.r)
        lin.gj = rho[:, None] * np.einsum("eab,ea->eb", lin.Jj, lin.r)
        g = np.zeros((N, 6))
        g[1:] += lin.gj[:N - 1]                       # chain edge n-1, then chain edge n, then the loops by index
        g[:-1] += lin.gi[:N - 1]
        for l in np.nonzero(lvalid)[0]:
            g[li[l]] += lin.gi[N - 1 + l]
            g[lj[l]] += lin.gj[N - 1 + l]
        g[0] = 0.0
        lin.g = g
        lin.cost = float((rho * lin.e).sum())
        lin.chain_cost = float(lin.e[:N - 1].sum())
        lin.loops_used, lin.loops_skipped = int(lvalid.sum()), int((~lvalid).sum())
        # B_k^-1 of the chain edges, closed form
        E = between(Z[:N - 1], between(poses[:-1], poses[1:]))
        s = np.where(E[:, 3] >= 0.0, 1.0, -1.0)[:, None, None]
        Binv = np.zeros((N - 1, 6, 6))
        with np.errstate(divide="ignore", invalid="ignore"):
            Binv[:, :3, :3] = np.swapaxes(rotmat(E[:, 3:]), -1, -2) / cw[:, 0, None, None]
            Binv[:, 3:, 3:] = gj_inverse(E[:, 3:], s) / cw[:, 1, None, None]
        lin.singular = bool((~np.isfinite(Binv).all((1, 2))).any() or (~np.isfinite(lin.r[:N - 1])).any())
        lin.Binv = Binv
        return lin

    def cost(self, traj0, poses, chain_w=None, loops_ij=None, loops_Z=None, loops_w=None, robust_scale=0.0):
        """[4]: cost, chain part, loops used, loops skipped"""
        lin = self.linearize(traj0, poses, chain_w, loops_ij, loops_Z, loops_w, robust_scale)
        return np.array([lin.cost, lin.chain_cost, lin.loops_used, lin.loops_skipped], np.float64)

    # -- the three pieces ------------------------------------------------------------------------------------------
    @staticmethod
    def matvec(lin, x, damping=0.0):
        """y = (H_chain + H_loops + damping I) x over nodes 1..N-1; x, y [N, 6], row 0 taken as / left zero"""
        x = np.array(x, np.float64)
        x[0] = 0.0
        u = np.einsum("eab,eb->ea", lin.Ji, x[lin.i]) + np.einsum("eab,eb->ea", lin.Jj, x[lin.j])
        yi = lin.rho[:, None] * np.einsum("eab,ea->eb", lin.Ji, u)
        yj = lin.rho[:, None] * np.einsum("eab,ea->eb", lin.Jj, u)
        N = lin.N
        y = damping * x
        y[1:] += yj[:N - 1]
        y[:-1] += yi[:N - 1]
        for e in range(N - 1, len(lin.i)):
            if lin.valid[e]:
                y[lin.i[e]] += yi[e]
                y[lin.j[e]] += yj[e]
        y[0] = 0.0
        return y

    @staticmethod
    def chain_solve(lin, r, segment=None):
        """z = M^-1 r = J_c^-1 J_c^-T r by the two block recurrences; r, z [N, 6] with row 0 zero.  segment=None: the
        plain sequential recurrences.  segment=n: the device's formulation -- segments of n edges, a local pass with
        zero input, a scan over the segment summaries with the segments' transfer matrices, a local pass with the
        right input."""
        N = lin.N
        E = N - 1
        A, Binv = lin.Ji[:E], lin.Binv                # A_k acts on node k (A_0 on the fixed node: never used)
        r = np.asarray(r, np.float64)
        y = np.zeros((E + 1, 6))                      # y[E] = 0: the input of the last edge
        z = np.zeros((N, 6))

        def back(k, y_next):                          # y_k from y_{k+1}
            rhs = r[k + 1] - (A[k + 1].T @ y_next if k + 1 < E else 0.0)
            return Binv[k].T @ rhs

        def fwd(k, z_k):                              # z_{k+1} from z_k
            return Binv[k] @ (y[k] - (A[k] @ z_k if k > 0 else 0.0))

        if segment is None:
            for k in range(E - 1, -1, -1):
                y[k] = back(k, y[k + 1])
            for k in range(E):
                z[k + 1] = fwd(k, z[k])
            return z
        n = int(segment)
        starts = list(range(0, E, n))
        S = len(starts)
        ends = [min(E, s + n) for s in starts]
        # backward: segment s runs k = end-1 .. start; its input is y[end]
        Q, v = [], []
        for s in range(S):
            P = np.eye(6)
            acc = np.zeros(6)
            for k in range(ends[s] - 1, starts[s] - 1, -1):
                Gk = -Binv[k].T @ A[k + 1].T if k + 1 < E else np.zeros((6, 6))
                acc = back(k, acc)
                P = Gk @ P
            Q.append(P)
            v.append(acc)
        inp = np.zeros(6)                             # scan from the last segment down
        ins = [None] * S
        for s in range(S - 1, -1, -1):
            ins[s] = inp
            inp = Q[s] @ inp + v[s]
        for s in range(S):
            cur = ins[s]
            for k in range(ends[s] - 1, starts[s] - 1, -1):
                cur = back(k, cur)
                y[k] = cur
        # forward: segment s runs k = start .. end-1; its input is z[start]
        P_, v = [], []
        for s in range(S):
            P = np.eye(6)
            acc = np.zeros(6)
            for k in range(starts[s], ends[s]):
                Fk = -Binv[k] @ A[k] if k > 0 else np.zeros((6, 6))
                acc = fwd(k, acc)
                P = Fk @ P
            P_.append(P)
            v.append(acc)
        inp = np.zeros(6)
        for s in range(S):
            ins[s] = inp
            inp = P_[s] @ inp + v[s]
        for s in range(S):
            cur = ins[s]
            for k in range(starts[s], ends[s]):
                cur = fwd(k, cur)
                z[k + 1] = cur
        return z

    @staticmethod
    def dense(lin, damping=0.0):
        """(H, g, H_chain, J_c) as dense matrices over the 6 (N-1) unknowns of nodes 1..N-1 (small N only)"""
        N = lin.N
        n = 6 * (N - 1)
        J = np.zeros((len(lin.i), 6, n + 6))          # six leading columns for node 0, cut below
        for e in range(len(lin.i)):
            J[e, :, 6 * lin.i[e]:6 * lin.i[e] + 6] += lin.Ji[e]
            J[e, :, 6 * lin.j[e]:6 * lin.j[e] + 6] += lin.Jj[e]
        J = J[:, :, 6:]
        Jc = J[:N - 1].reshape(n, n)
        Hc = Jc.T @ Jc
        Jl = (np.sqrt(lin.rho[N - 1:])[:, None, None] * J[N - 1:]).reshape(-1, n)
        H = Hc + Jl.T @ Jl + damping * np.eye(n)
        return H, lin.g[1:].reshape(-1).copy(), Hc, Jc

    # -- Gauss-Newton ----------------------------------------------------------------------------------------------
    def pcg(self, lin, cg_iters=64, cg_tol=1e-8, damping=0.0, segment=None):
        """(x [N, 6], status, iterations, sqrt(r.z / (r.z)_0) at the stop) of H x = -g"""
        N = lin.N
        x = np.zeros((N, 6))
        if lin.singular:
            return x, 2, 0, 0.0
        r = -lin.g
        z = self.chain_solve(lin, r, segment)
        rz0 = rz = float((r * z).sum())
        if rz0 == 0.0:
            return x, 0, 0, 0.0
        if not (rz0 > 0.0 and np.isfinite(rz0)):
            return x, 2, 0, 0.0
        p = z.copy()
        it = 0
        for _ in range(int(cg_iters)):
            Ap = self.matvec(lin, p, damping)
            pAp = float((p * Ap).sum())
            if not (pAp > 0.0 and np.isfinite(pAp)):
                break
            a = rz / pAp
            x = x + a * p
            r = r - a * Ap
            it += 1
            z = self.chain_solve(lin, r, segment)
            rzn = float((r * z).sum())
            if rzn <= cg_tol * cg_tol * rz0:
                rz = rzn
                break
            p = z + (rzn / rz) * p
            rz = rzn
        res = float(np.sqrt(max(rz, 0.0) / rz0)) if np.isfinite(rz) else float("nan")
        if it == 0 or not np.isfinite(x).all():
            return np.zeros((N, 6)), 2, it, res
        return x, 0, it, res

    def optimize(self, traj0, loops_ij=None, loops_Z=None, loops_w=None, poses=None, chain_w=None, gn_iters=6,
                 cg_iters=64, cg_tol=1e-8, robust_scale=0.0, damping=0.0, tol_t=0.0, tol_r=0.0, exact=False,
                 segment=None):
        """(poses [N, 7], info [gn_iters, 8]).  exact=True takes each step from numpy.linalg.solve on dense()."""
        check_options(gn_iters, cg_iters, cg_tol, robust_scale, damping, tol_t, tol_r)
        traj0 = np.asarray(traj0, np.float64)
        poses = traj0.copy() if poses is None else np.array(poses, np.float64)
        info = np.zeros((int(gn_iters), 8))
        done = False
        for it in range(int(gn_iters)):
            if done:
                info[it, 0] = 3.0
                continue
            lin = self.linearize(traj0, poses, chain_w, loops_ij, loops_Z, loops_w, robust_scale)
            if exact:
                H, g, _, _ = self.dense(lin, damping)
                x = np.zeros((lin.N, 6))
                x[1:] = np.linalg.solve(H, -g).reshape(-1, 6)
                status, cg, res = 0, 0, 0.0
            else:
                x, status, cg, res = self.pcg(lin, cg_iters, cg_tol, damping, segment)
            mt = float(np.sqrt((x[:, :3] ** 2).sum(1)).max())
            mr = float(np.sqrt((x[:, 3:] ** 2).sum(1)).max())
            if status == 0:
                poses = retract(poses, x)
                done = mt < tol_t and mr < tol_r
            else:
                mt = mr = 0.0
            info[it] = (status, lin.loops_used, lin.cost, cg, res, mt, mr, lin.loops_skipped)
        return poses, info


def synthetic_graph(N, laps=2, loops=4, seed=0, sigma_t=0.02, sigma_r=np.deg2rad(0.1), falsify=False):
    """A drive of `laps` turns round a circle of 20 m radius with a small z wave and roll / pitch: dict with truth
    [N, 7], traj0 [N, 7] (noisy odometry chained from the true first pose), loops_ij int32 [loops, 2], loops_Z
    [loops, 7] (the TRUE relative pose between a node of the last lap and the node one lap earlier, spread over that
    lap), loops_w, chain_w (see the comment at the end for the weights).  falsify: loop number loops // 2 has
    (5, -3, 0.5) m added to its translation; its index is under "falsified"."""
    rng = np.random.default_rng(seed)
    per_lap = N // laps
    a = 2.0 * np.pi * np.arange(N) / per_lap
    t = np.stack([20.0 * np.cos(a), 20.0 * np.sin(a), 0.3 * np.sin(3.0 * a)], 1)
    yaw, roll, pitch = a + np.pi / 2.0, 0.03 * np.sin(2.0 * a), 0.02 * np.cos(5.0 * a)

    def axis_q(ang, ax):
        q = np.zeros((len(ang), 4))
        q[:, 0], q[:, 1 + ax] = np.cos(ang / 2.0), np.sin(ang / 2.0)
        return q
    q = qmul(qmul(axis_q(yaw, 2), axis_q(pitch, 1)), axis_q(roll, 0))
    truth = np.concatenate([t, q], 1)
    rel = between(truth[:-1], truth[1:])
    noise = np.concatenate([sigma_t * rng.standard_normal((N - 1, 3)), sigma_r * rng.standard_normal((N - 1, 3))], 1)
    rel = retract(rel, noise)
    traj0 = np.empty((N, 7))
    traj0[0] = truth[0]
    for k in range(N - 1):
        traj0[k + 1] = compose(traj0[k], rel[k])
        traj0[k + 1, 3:] /= np.sqrt((traj0[k + 1, 3:] ** 2).sum())
    first = (laps - 1) * per_lap
    j = (first + (np.arange(loops) + 0.5) * (N - first) / max(loops, 1)).astype(np.int64) if loops else np.zeros(0, np.int64)
    i = j - per_lap
    Z = between(truth[i], truth[j])
    if falsify and loops:
        Z[loops // 2, :3] += (5.0, -3.0, 0.5)
    # weights: the chain's are 1 / sigma up to a common factor that makes w_t = 1 per metre (so that a robust scale is
    # in metres of translation); a loop measurement, a registration against a map of many scans, is taken to be ten times
    # as precise as one odometry step
    chain_w = np.array([1.0, sigma_t / sigma_r])
    return {"truth": truth, "traj0": traj0, "loops_ij": np.stack([i, j], 1).astype(np.int32), "loops_Z": Z,
            "loops_w": np.tile(10.0 * chain_w[None, :], (loops, 1)), "chain_w": chain_w,
            "falsified": (loops // 2) if (falsify and loops) else None}


PoseGraphRef.synthetic_graph = staticmethod(synthetic_graph)


# the edge record of rslo_posegraph_linearize (include/rslo_hip.h): offsets in doubles
REC = {"r": 0, "rho": 6, "flag": 7, "Att": 8, "Atr": 17, "Arr": 26, "Btt": 35, "Brr": 44, "gi": 53, "gj": 59, "e": 65,
       "Binv_tt": 66, "Binv_rr": 75}
REC_DOUBLES = 84


class PoseGraph:
    """The device optimiser: owns a workspace for graphs of up to `capacity` nodes and `max_loops` loop edges.  Every
    method enqueues on the current stream, reads nothing on the host and -- when the caller passes poses=, info= (and
    loops_w) -- allocates nothing, so a call can be captured.  All tensors are float64 CUDA, contiguous; loops_ij int32.

    Feeding the corrected poses back into a runner's chain state and voxel map is OdometryRunner.adopt_loop_closure() /
    rebuild_map().  (Verifying a loop candidate and the keyframe store are rslo_amd/loops.py.)"""

    def __init__(self, capacity=8192, max_loops=256, device="cuda"):
        import torch
        from rslo_amd import capi
        try:
            self.capacity, self.max_loops = check_sizes(capacity, max_loops)
        except ValueError as e:
            raise capi.RsloHipError(str(e))
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._ws = torch.zeros((capi.posegraph_ws_bytes(self.capacity, self.max_loops) // 8,), dtype=torch.int64,
                               device=self.device)
        self._lin = None      # (N, L) of the linearisation the workspace holds

    def reference(self):
        return PoseGraphRef(self.capacity, self.max_loops)

    def _loops(self, loops_ij, loops_Z, loops_w):
        import torch
        if loops_ij is None or loops_ij.shape[0] == 0:
            return None, None, None
        if loops_w is None:
            loops_w = torch.ones((loops_ij.shape[0], 2), dtype=torch.float64, device=self.device)
        return loops_ij, loops_Z, loops_w

    def _fits(self, N, L, name):
        from rslo_amd import capi
        if N > self.capacity or L > self.max_loops:
            raise capi.RsloHipError("PoseGraph.%s: N = %d, L = %d exceed capacity = %d, max_loops = %d"
                                    % (name, N, L, self.capacity, self.max_loops))

    def optimize(self, traj0, loops_ij=None, loops_Z=None, loops_w=None, poses=None, chain_w=(1.0, 1.0), gn_iters=6,
                 cg_iters=64, cg_tol=1e-8, robust_scale=0.0, damping=0.0, tol_t=0.0, tol_r=0.0, info=None):
        """(poses [N, 7], info [gn_iters, 8]).  poses=None starts from a copy of traj0; a given poses is updated in
        place.  chain_w: a pair, or a [N-1, 2] tensor."""
        import torch
        from rslo_amd import capi
        loops_ij, loops_Z, loops_w = self._loops(loops_ij, loops_Z, loops_w)
        self._fits(int(traj0.shape[0]), 0 if loops_ij is None else int(loops_ij.shape[0]), "optimize")
        if poses is None:
            poses = traj0.clone()
        if info is None:
            info = torch.empty((int(gn_iters), 8), dtype=torch.float64, device=self.device)
        capi.posegraph_optimize(traj0, poses, chain_w, loops_ij, loops_Z, loops_w, gn_iters, cg_iters, cg_tol, robust_scale,
                                damping, tol_t, tol_r, info, self._ws)
        self._lin = None
        return poses, info

    def cost(self, traj0, poses, loops_ij=None, loops_Z=None, loops_w=None, chain_w=(1.0, 1.0), robust_scale=0.0, out=None):
        """float64 [4] on the device: cost, chain part, loops used, loops skipped"""
        import torch
        from rslo_amd import capi
        loops_ij, loops_Z, loops_w = self._loops(loops_ij, loops_Z, loops_w)
        self._fits(int(traj0.shape[0]), 0 if loops_ij is None else int(loops_ij.shape[0]), "cost")
        if out is None:
            out = torch.empty((4,), dtype=torch.float64, device=self.device)
        capi.posegraph_cost(traj0, poses, chain_w, loops_ij, loops_Z, loops_w, robust_scale, out, self._ws)
        self._lin = None
        return out

    def linearize(self, traj0, poses, loops_ij=None, loops_Z=None, loops_w=None, chain_w=(1.0, 1.0), robust_scale=0.0):
        """{"edges": [(N-1+L), 84] records (offsets: posegraph.REC), "g": [N, 6], "sums": [4]}; the workspace keeps the
        linearisation for matvec() and chain_solve()."""
        import torch
        from rslo_amd import capi
        loops_ij, loops_Z, loops_w = self._loops(loops_ij, loops_Z, loops_w)
        N, L = int(traj0.shape[0]), 0 if loops_ij is None else int(loops_ij.shape[0])
        self._fits(N, L, "linearize")
        edges = torch.empty((N - 1 + L, REC_DOUBLES), dtype=torch.float64, device=self.device)
        g = torch.empty((N, 6), dtype=torch.float64, device=self.device)
        sums = torch.empty((4,), dtype=torch.float64, device=self.device)
        capi.posegraph_linearize(traj0, poses, chain_w, loops_ij, loops_Z, loops_w, robust_scale, edges, g, sums, self._ws)
        self._lin = (N, L)
        return {"edges": edges, "g": g, "sums": sums}

    def _held(self, name):
        from rslo_amd import capi
        if self._lin is None:
            raise capi.RsloHipError("PoseGraph.%s: call linearize() first (optimize() and cost() overwrite it)" % name)
        return self._lin

    def matvec(self, x, damping=0.0, out=None):
        """y = (H_chain + H_loops + damping I) x on the last linearize(); [N, 6], row 0 read as zero"""
        import torch
        from rslo_amd import capi
        N, L = self._held("matvec")
        y = torch.empty_like(x) if out is None else out
        capi.posegraph_matvec(x, y, N, L, damping, self._ws)
        return y

    def chain_solve(self, r, out=None):
        """z = H_chain^-1 r on the last linearize(); [N, 6]"""
        import torch
        from rslo_amd import capi
        N, L = self._held("chain_solve")
        z = torch.empty_like(r) if out is None else out
        capi.posegraph_chain_solve(r, z, N, L, self._ws)
        return z

    def between(self, A, B, out=None):
        """A[k]^-1 o B[k] for [n, 7] rows: a registered pose and the pose it was registered against become a loop
        measurement without a host trip"""
        from rslo_amd import capi
        return capi.pose_between(A, B, out)
