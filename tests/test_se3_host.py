"""rslo_amd/se3.py, the host pose algebra: its identities on random poses, its agreement with the numpy port of the
reference's pose helpers, and the two summation orders of the rotation held apart.

Bounds: 1e-14 absolute on poses whose translation components are standard normal draws (|t| < 5 over the 1 000 draws): a
compose / inverse / rotate is a few dozen float64 roundings of values of that size, a few 1e-16 each."""
import numpy as np

from rslo_amd import se3

N = 1000
IDENT = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)


def _poses(seed):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((N, 4))
    return np.concatenate([rng.standard_normal((N, 3)), q / np.linalg.norm(q, axis=1, keepdims=True)], 1)


def test_identities():
    A, B = _poses(11), _poses(12)
    ident = np.broadcast_to(IDENT, A.shape)
    assert np.abs(se3.compose(A, se3.inverse(A)) - ident).max() <= 1e-14
    assert np.abs(se3.compose(se3.inverse(A), A) - ident).max() <= 1e-14
    assert np.abs(se3.between(A, A) - ident).max() <= 1e-14
    assert np.abs(se3.between(A, B) - se3.compose(se3.inverse(A), B)).max() <= 1e-14
    kept = se3.retract(A, np.zeros((N, 6)))      # retract divides the quaternion by its norm: A's is a unit one already
    assert np.abs(kept - A).max() <= 1e-14 and np.abs(np.linalg.norm(kept[:, 3:], axis=1) - 1.0).max() <= 1e-15
    v = np.random.default_rng(13).standard_normal((N, 3))
    assert np.abs((se3.rotmat(A[:, 3:]) @ v[:, :, None])[:, :, 0] - se3.rotate(A[:, 3:], v)).max() <= 1e-14
    assert np.abs(se3.skew(v) @ B[:, :3, None] - np.cross(v, B[:, :3])[:, :, None]).max() <= 1e-14
    assert np.abs(se3.qmul(A[:, 3:], se3.qconj(A[:, 3:])) - IDENT[3:]).max() <= 1e-14


def test_against_the_reference_port():
    """compose / inverse against rslo.utils.pose_utils_np.  The port's qmult divides its product by (norm + 1e-6), the
    reference's own rule (a unit quaternion comes back shorter by 1e-6), where se3 does not renormalise: the port's
    quaternion is compared after that one known factor is taken out again, every component to 1e-14."""
    from rslo.utils import pose_utils_np as ref
    A, B = _poses(21), _poses(22)
    want = ref.compose_pose_quaternion(A, B)
    got = se3.compose(A, B)
    assert np.abs(got[:, :3] - want[:, :3]).max() <= 1e-14
    assert np.abs(got[:, 3:] - want[:, 3:] * (1.0 + 1e-6)).max() <= 1e-14
    assert np.abs(se3.inverse(A) - ref.invert_pose_quaternion(A)).max() <= 1e-14


def test_the_two_forms_stay_apart():
    """form A, v + (2 b w + 2 c), is se3.rotate (and se3_rotate of csrc/se3.h, map_point, the pose graph); form B,
    (v + 2 b w) + 2 c, is the translation update of k_pose_chain / gn_step and of their scalar restatements
    (inference.pose_chain_host, gauss_newton.gauss_newton_step).  Both are right (within 4 ulp of R(q) v, component by
    component); they are NOT the same bits, and each is pinned by bit-equality tests of its kernels: whoever makes
    se3.rotate form B, or this point's two forms equal, fails here first.  (Seed 2: a point where the forms differ.)"""
    rng = np.random.default_rng(2)
    q = rng.standard_normal(4)
    q /= np.linalg.norm(q)
    v = rng.standard_normal(3) * 10
    b = np.cross(q[1:], v)
    c = np.cross(q[1:], b)
    form_a = v + (2.0 * b * q[0] + 2.0 * c)
    form_b = (v + 2.0 * b * q[0]) + 2.0 * c
    want = se3.rotmat(q) @ v
    assert (np.abs(form_a - want) <= 4 * np.spacing(np.abs(want))).all()
    assert (np.abs(form_b - want) <= 4 * np.spacing(np.abs(want))).all()
    assert not np.array_equal(form_a, form_b)
    assert np.array_equal(se3.rotate(q, v).view(np.int64), form_a.view(np.int64))


def test_posegraph_re_exports_the_algebra():
    from rslo_amd import posegraph
    for name in ("qmul", "qconj", "rotate", "rotmat", "skew", "compose", "inverse", "between", "dquat", "retract"):
        assert getattr(posegraph, name) is getattr(se3, name)
