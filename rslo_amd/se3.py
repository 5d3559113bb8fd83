"""The pose algebra of the streaming back end on the host, numpy float64 (device twin: csrc/se3.h).

The rule: poses are [7] float64 rows (t, q wxyz).  compose(A, B) = (t_A + rotate(q_A, t_B), q_A (x) q_B), rotate(q, v) =
v + 2 w (u x v) + 2 u x (u x v) with u = vec(q); the inverse of a unit pose is (-rotate(q*, t), q*).  Products are not
renormalised; only the update divides by the norm.  The local parametrisation is T' = T o (rho, phi):
t' = t + rotate(q, rho), q' = (q (x) dq(phi)) / |.|, dq = (1, phi / 2) when |phi| < 1e-12, else
(cos(|phi| / 2), sin(|phi| / 2) / |phi| * phi).

rotate sums v + (2 b w + 2 c) with b = u x v, c = u x b ("form A"), as se3_rotate of csrc/se3.h does: the two agree bit
for bit.  The scalar restatements of one device thread, inference.pose_chain_host and gauss_newton.gauss_newton_step, sum
(v + 2 b w) + 2 c ("form B") as their kernels do; the two forms differ in the last bit and both are pinned by
bit-equality tests (tests/test_se3_host.py holds them apart).

Every function works row by row on [..., 7] / [..., 4] / [..., 3] float64 arrays.
"""
import numpy as np


def qmul(a, b):
    aw, av, bw, bv = a[..., :1], a[..., 1:], b[..., :1], b[..., 1:]
    w = aw * bw - (av * bv).sum(-1, keepdims=True)
    v = av * bw + bv * aw + np.cross(av, bv)
    return np.concatenate([w, v], -1)


def qconj(q):
    return np.concatenate([q[..., :1], -q[..., 1:]], -1)


def rotate(q, v):
    u = q[..., 1:]
    b = np.cross(u, v)
    c = np.cross(u, b)
    return v + (2.0 * b * q[..., :1] + 2.0 * c)


def rotmat(q):
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0] = 1.0 - 2.0 * (y * y + z * z)
    R[..., 0, 1] = 2.0 * (x * y - w * z)
    R[..., 0, 2] = 2.0 * (x * z + w * y)
    R[..., 1, 0] = 2.0 * (x * y + w * z)
    R[..., 1, 1] = 1.0 - 2.0 * (x * x + z * z)
    R[..., 1, 2] = 2.0 * (y * z - w * x)
    R[..., 2, 0] = 2.0 * (x * z - w * y)
    R[..., 2, 1] = 2.0 * (y * z + w * x)
    R[..., 2, 2] = 1.0 - 2.0 * (x * x + y * y)
    return R


def skew(v):
    S = np.zeros(v.shape[:-1] + (3, 3))
    S[..., 0, 1], S[..., 0, 2] = -v[..., 2], v[..., 1]
    S[..., 1, 0], S[..., 1, 2] = v[..., 2], -v[..., 0]
    S[..., 2, 0], S[..., 2, 1] = -v[..., 1], v[..., 0]
    return S


def compose(A, B):
    return np.concatenate([A[..., :3] + rotate(A[..., 3:], B[..., :3]), qmul(A[..., 3:], B[..., 3:])], -1)


def inverse(A):
    qc = qconj(A[..., 3:])
    return np.concatenate([-rotate(qc, A[..., :3]), qc], -1)


def between(A, B):
    """A^-1 o B row by row: the pose of B in the frame of A."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    qc = qconj(A[..., 3:])
    return np.concatenate([rotate(qc, B[..., :3] - A[..., :3]), qmul(qc, B[..., 3:])], -1)


def dquat(phi):
    th = np.sqrt((phi * phi).sum(-1, keepdims=True))
    small = th < 1e-12
    ths = np.where(small, 1.0, th)
    f = np.where(small, 0.5, np.sin(ths / 2.0) / ths)
    return np.concatenate([np.where(small, 1.0, np.cos(ths / 2.0)), f * phi], -1)


def retract(T, delta):
    """T o (rho, phi) row by row"""
    t = T[..., :3] + rotate(T[..., 3:], delta[..., :3])
    q = qmul(T[..., 3:], dquat(delta[..., 3:]))
    return np.concatenate([t, q / np.sqrt((q * q).sum(-1, keepdims=True))], -1)
