"""The Gauss-Newton core of scan-to-map registration and loop verification on the host, numpy float64 (device twin:
csrc/gauss_newton.h).  The 28 sums of a set of matched points are the upper triangle of H = sum J^T J (21, row-major),
g = sum J^T r (6) and the cost sum r.r, for the world-frame twist (dt, dtheta).  terms_of gives their addends row by row
in the operand order of gn_point_terms / gn_plane_terms, info_terms those of gn_info_terms (H = sum J^T M J with a
cell's information matrix M); robust_weighted is the Geman-McClure block of k_gn_accum; gauss_newton_step is gn_step,
scalar float64 in the order of the device's one thread; register_loop is the iteration loop of the register calls."""
import math

import numpy as np


def point_jacobian(w):
    """[n, 3, 6]: the rows J = [I | -[w]x] of the points at world positions w [n, 3]"""
    J = np.zeros((len(w), 3, 6), np.float64)
    for a in range(3):
        J[:, a, a] = 1.0
    J[:, 0, 4], J[:, 0, 5] = w[:, 2], -w[:, 1]
    J[:, 1, 3], J[:, 1, 5] = -w[:, 2], w[:, 0]
    J[:, 2, 3], J[:, 2, 4] = w[:, 1], -w[:, 0]
    return J


def terms_of(J, r):
    """[K, 28]: the addends from the Jacobian rows J [K, 3, 6] and residuals r [K, 3] (rows a term lacks are zero)"""
    terms = np.zeros((len(J), 28), np.float64)
    o = 0
    for a in range(6):
        for b in range(a, 6):
            terms[:, o] = J[:, 0, a] * J[:, 0, b] + J[:, 1, a] * J[:, 1, b] + J[:, 2, a] * J[:, 2, b]
            o += 1
    for a in range(6):
        terms[:, 21 + a] = J[:, 0, a] * r[:, 0] + J[:, 1, a] * r[:, 1] + J[:, 2, a] * r[:, 2]
    terms[:, 27] = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2]
    return terms


def point_terms(w, d):
    """[n, 28]: the addends of the 28 sums of matched points at world positions w with residuals d (J = [I | -[w]x])"""
    return terms_of(point_jacobian(w), d)


def info_terms(w, d, M6):
    """[n, 28]: the addends of point-to-distribution terms (gn_info_terms): rows J = [I | -[w]x] of the points at world
    positions w [n, 3], residuals d [n, 3], information matrices M6 [n, 6] in the order 00 01 02 11 12 22.  m = M d,
    B = M J; H(k, l) = J0[k] B0[l] + J1[k] B1[l] + J2[k] B2[l], g(k) = J0[k] m0 + J1[k] m1 + J2[k] m2, cost = d . m,
    every sum left to right."""
    w, d, M6 = (np.asarray(x, np.float64) for x in (w, d, M6))
    J = point_jacobian(w)
    M = [[M6[:, 0], M6[:, 1], M6[:, 2]], [M6[:, 1], M6[:, 3], M6[:, 4]], [M6[:, 2], M6[:, 4], M6[:, 5]]]
    terms = np.zeros((len(w), 28), np.float64)
    with np.errstate(all="ignore"):
        m = [M[a][0] * d[:, 0] + M[a][1] * d[:, 1] + M[a][2] * d[:, 2] for a in range(3)]
        B = [[M[a][0] * J[:, 0, k] + M[a][1] * J[:, 1, k] + M[a][2] * J[:, 2, k] for k in range(6)] for a in range(3)]
        o = 0
        for k in range(6):
            for l in range(k, 6):
                terms[:, o] = J[:, 0, k] * B[0][l] + J[:, 1, k] * B[1][l] + J[:, 2, k] * B[2][l]
                o += 1
        for k in range(6):
            terms[:, 21 + k] = J[:, 0, k] * m[0] + J[:, 1, k] * m[1] + J[:, 2, k] * m[2]
        terms[:, 27] = d[:, 0] * m[0] + d[:, 1] * m[1] + d[:, 2] * m[2]
    return terms


def _cross3(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def gauss_newton_step(sums, pose, damping=0.0):
    """The step from the 28 sums (H upper triangle, g, cost) at pose [7]: -> (new pose [7], |dt|, theta), or None when
    M = H + damping * I is not positive definite or the step overflows.  Scalar float64 in the order of the device's one
    thread; the translation update is form B: see se3.py."""
    f = [float(v) for v in sums]
    M = [[0.0] * 6 for _ in range(6)]
    o = 0
    for a in range(6):
        for b in range(a, 6):
            M[a][b] = M[b][a] = f[o]
            o += 1
    for a in range(6):
        M[a][a] = M[a][a] + float(damping)
    L = [[0.0] * 6 for _ in range(6)]
    for a in range(6):
        for b in range(a + 1):
            acc = M[a][b]
            for k in range(b):
                acc = acc - L[a][k] * L[b][k]
            if a == b:
                if not (0.0 < acc < float("inf")):
                    return None
                L[a][a] = math.sqrt(acc)
            else:
                L[a][b] = acc / L[b][b]
    y, x = [0.0] * 6, [0.0] * 6
    for a in range(6):
        acc = f[21 + a]
        for k in range(a):
            acc = acc - L[a][k] * y[k]
        y[a] = acc / L[a][a]
    for a in range(5, -1, -1):
        acc = y[a]
        for k in range(a + 1, 6):
            acc = acc - L[k][a] * x[k]
        x[a] = acc / L[a][a]
    dt, dr = [-x[0], -x[1], -x[2]], [-x[3], -x[4], -x[5]]
    nt = math.sqrt(dt[0] * dt[0] + dt[1] * dt[1] + dt[2] * dt[2])
    th = math.sqrt(dr[0] * dr[0] + dr[1] * dr[1] + dr[2] * dr[2])
    if not (nt < float("inf") and th < float("inf")):
        return None
    if th < 1e-12:
        dq = [1.0] + [v / 2.0 for v in dr]
    else:
        fac = math.sin(th / 2.0) / th
        dq = [math.cos(th / 2.0)] + [fac * v for v in dr]
    t, q = [float(v) for v in pose[:3]], [float(v) for v in pose[3:7]]
    b = _cross3(dq[1:], t)
    c = _cross3(dq[1:], b)
    tn = [dt[a] + (t[a] + 2.0 * b[a] * dq[0] + 2.0 * c[a]) for a in range(3)]
    vx = _cross3(dq[1:], q[1:])
    r = [dq[0] * q[0] - (dq[1] * q[1] + dq[2] * q[2] + dq[3] * q[3])]
    r += [dq[1 + a] * q[0] + q[1 + a] * dq[0] + vx[a] for a in range(3)]
    nr = math.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3])
    return np.array(tn + [v / nr for v in r], np.float64), nt, th


def robust_weighted(terms, scale):
    """terms [K, 28] with every row multiplied by its Geman-McClure weight rho = u * u, u = s2 / (s2 + e), e the row's
    cost addend and s2 = scale * scale; scale 0: the terms as they are"""
    if scale == 0.0:
        return terms
    s2 = scale * scale
    with np.errstate(all="ignore"):
        u = s2 / (s2 + terms[:, 27])
        rho = u * u
        return terms * rho[:, None]


def register_loop(normal_equations, pose, iters, damping, min_pairs, tol_t, tol_r):
    """-> (pose [7] float64, info [iters, 8]): Gauss-Newton iterations on the 29 sums normal_equations(pose) returns.
    Row = (status, pairs, cost, |dt|, theta, 0, 0, 0); status 1 (fewer than min_pairs pairs) and 2 (no step: not positive
    definite, or overflowed) leave the pose as it is, status 3 marks the iterations after a step below both tolerances."""
    pose = np.array(pose, dtype=np.float64).reshape(7)
    info = np.zeros((int(iters), 8), np.float64)
    done = False
    for it in range(int(iters)):
        if done:
            info[it, 0] = 3.0
            continue
        sums = normal_equations(pose)
        info[it, 1], info[it, 2] = sums[28], sums[27]
        if sums[28] < min_pairs:
            info[it, 0] = 1.0
            continue
        step = gauss_newton_step(sums[:28], pose, damping)
        if step is None:
            info[it, 0] = 2.0
            continue
        pose, info[it, 3], info[it, 4] = step
        done = bool(info[it, 3] < tol_t and info[it, 4] < tol_r)
    return pose, info
