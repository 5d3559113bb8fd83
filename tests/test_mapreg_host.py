"""Scan-to-map registration, the float64 restatement (rslo_amd/mapping.py VoxelMapRef.nearest / normal_equations /
register; rules: include/rslo_hip.h "Scan-to-map registration").  No GPU: the restatement is the arbiter of
tests/test_gpu_mapreg.py, so it is held here against things that do not share its code -- hand-made cells, an all-pairs
search, finite differences of the cost, and the drive's true poses."""
import numpy as np
import pytest

IDENT = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
POSE_YAW = np.array([1.0, -0.5, 0.1, np.cos(0.15), 0.0, 0.0, np.sin(0.15)], np.float64)
_CACHE = {}


def _cloud(seed):
    from rslo_amd import synthetic
    if ("cloud", seed) not in _CACHE:
        _CACHE["cloud", seed] = synthetic.small_cloud(4000, seed=seed)
    return _CACHE["cloud", seed]


def _pts(*xyz):
    return np.array(xyz, np.float32).reshape(-1, 3)


def test_hand_made_cells():
    from rslo_amd.mapping import VoxelMapRef
    ref = VoxelMapRef(1.0)
    # one scan; cells (0,0,0), (1,0,0), (0,2,0); the third point raises the hits of cell (0,0,0) to 2
    ref.insert(_pts((0.75, 0.5, 0.5), (1.25, 0.5, 0.5), (0.5, 0.25, 0.5), (0.5, 2.5, 0.5)))
    assert ref.points()[1].tolist() == [0, 1, 3] and ref.points()[2].tolist() == [2, 1, 1]
    # (1.0, 0.5, 0.5) is 0.25 from the rows of tags 0 and 1, exactly: the tie goes to the smaller tag, from either cell
    tags, d2 = ref.nearest(_pts((1.0, 0.5, 0.5)), IDENT)
    assert tags.tolist() == [0] and d2.tolist() == [0.0625]
    tags, d2, rows = ref.nearest(_pts((1.0, 0.5, 0.5), (1.125, 0.5, 0.5)), IDENT, return_rows=True)
    assert tags.tolist() == [0, 1] and d2.tolist() == [0.0625, 0.015625]
    assert rows.dtype == np.float32 and rows[:, :3].tolist() == [[0.75, 0.5, 0.5], [1.25, 0.5, 0.5]]
    # min_hits = 2 leaves only the cell of tag 0
    tags, d2 = ref.nearest(_pts((1.125, 0.5, 0.5), (0.5, 2.5, 0.5)), IDENT, min_hits=2)
    assert tags.tolist() == [0, -1] and d2.tolist() == [0.140625, -1.0]
    # the edge d2 < max_dist^2 is exclusive: the point is exactly 0.5 from tag 3's row
    q = _pts((0.5, 3.0, 0.5))
    assert ref.nearest(q, IDENT, max_dist=0.5)[0].tolist() == [-1]
    assert ref.nearest(q, IDENT, max_dist=0.5000001)[0].tolist() == [3]
    assert ref.nearest(q, IDENT, max_dist=0.5, return_rows=True)[2].tolist() == [[0.0] * 4]
    # two cells away: not a candidate, whatever max_dist (which may not exceed the cell edge)
    assert ref.nearest(_pts((0.5, 4.1, 0.5)), IDENT)[0].tolist() == [-1]
    for bad in (1.5, 0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            ref.nearest(q, IDENT, max_dist=bad)
    # an invalid or gated query
    tags, d2 = ref.nearest(_pts((np.nan, 0.5, 0.5), (np.inf, 0.5, 0.5), (3e6, 0.5, 0.5)), IDENT)
    assert tags.tolist() == [-1] * 3 and d2.tolist() == [-1.0] * 3
    gated = VoxelMapRef(1.0, min_range=0.5, max_range=2.0)
    gated.insert(_pts((0.75, 0.5, 0.5), (1.25, 0.5, 0.5)))
    tags, _ = gated.nearest(_pts((0.25, 0.25, 0.25), (1.0, 0.5, 0.5), (2.0, 0.5, 0.5)), IDENT)
    assert tags.tolist() == [-1, 0, -1]
    # an empty map
    empty = VoxelMapRef(1.0)
    tags, d2, rows = empty.nearest(_pts((0.5, 0.5, 0.5)), IDENT, return_rows=True)
    assert tags.tolist() == [-1] and d2.tolist() == [-1.0] and not rows.any()
    assert empty.normal_equations(_pts((0.5, 0.5, 0.5)), IDENT, "point").tolist() == [0.0] * 29
    pose, info = empty.register(_pts((0.5, 0.5, 0.5)), POSE_YAW, iters=2)
    assert pose.tobytes() == POSE_YAW.tobytes() and info[:, 0].tolist() == [1.0, 1.0]


def test_nearest_equals_brute_force():
    from rslo_amd.mapping import VoxelMapRef
    voxel = 0.4
    ref = VoxelMapRef(voxel)
    ref.insert(_cloud(0), IDENT)
    q = _cloud(5)
    md = 0.9 * voxel
    tags, d2 = ref.nearest(q, POSE_YAW, max_dist=md)
    rows, rtags, _ = ref.points()
    status, _, w = ref._cells(q, POSE_YAW)
    assert (status == 0).all()
    m = rows[:, :3].astype(np.float64)
    d = w[:, None, :] - m[None, :, :]
    all2 = d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1] + d[:, :, 2] * d[:, :, 2]      # [P, M]
    want_tags = np.full((len(q),), -1, np.int64)
    want_d2 = np.full((len(q),), -1.0)
    for i in range(len(q)):
        j = np.lexsort((rtags, all2[i]))[0]          # by d2, then by tag
        if all2[i, j] < md * md:
            want_tags[i], want_d2[i] = rtags[j], all2[i, j]
    assert (want_tags >= 0).sum() > 100 and (want_tags < 0).sum() > 100
    assert (tags == want_tags).all() and d2.tobytes() == want_d2.tobytes()


def _perturbed(pose, delta):
    """pose moved by the world-frame twist delta = (dt, dtheta): the update of register"""
    dt, dr = delta[:3], delta[3:]
    th = np.linalg.norm(dr)
    dq = np.concatenate([[np.cos(th / 2)], (np.sin(th / 2) / th if th > 0 else 0.5) * dr])
    t, q = pose[:3], pose[3:]
    b = np.cross(dq[1:], t)
    tn = dt + t + 2 * dq[0] * b + 2 * np.cross(dq[1:], b)
    qn = np.concatenate([[dq[0] * q[0] - dq[1:] @ q[1:]], dq[0] * q[1:] + q[0] * dq[1:] + np.cross(dq[1:], q[1:])])
    return np.concatenate([tn, qn / np.linalg.norm(qn)])


def _rotmat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


@pytest.mark.parametrize("metric", ["point", "plane"])
def test_jacobian_against_finite_differences(metric):
    """g = d(cost/2)/d(delta) and H = J^T J with J the residuals' Jacobian, both by central differences of residuals
    written here from the definition (rotation matrices, no shared code), over the correspondences of the base pose
    and with the plane normals held at the base pose, as the Gauss-Newton step holds them."""
    from rslo_amd.mapping import VoxelMapRef
    ref = VoxelMapRef(0.4)
    ref.insert(_cloud(0), IDENT)
    q = _cloud(5)
    tags, _, rows = ref.nearest(q, POSE_YAW, return_rows=True)
    sel = tags >= 0
    assert sel.sum() > 100
    p = q[sel, :3].astype(np.float64)
    m = rows[sel, :3].astype(np.float64)
    n0 = q[sel, 4:7].astype(np.float64) @ _rotmat(POSE_YAW[3:]).T

    def residuals(delta):
        pose = _perturbed(POSE_YAW, delta)
        d = p @ _rotmat(pose[3:]).T + pose[:3] - m
        return (n0 * d).sum(axis=1) if metric == "plane" else d.reshape(-1)

    eps = 1e-6
    r0 = residuals(np.zeros(6))
    J = np.stack([(residuals(eps * e) - residuals(-eps * e)) / (2 * eps) for e in np.eye(6)], axis=1)
    g_fd = np.array([(0.5 * (residuals(eps * e) ** 2).sum() - 0.5 * (residuals(-eps * e) ** 2).sum()) / (2 * eps)
                     for e in np.eye(6)])
    out = ref.normal_equations(q, POSE_YAW, metric)
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = out[:21]
    H = H + np.triu(H, 1).T
    assert out[28] == sel.sum()
    assert abs(out[27] - r0 @ r0) <= 1e-12 * (r0 @ r0)
    assert np.abs(out[21:27] - g_fd).max() <= 1e-6 * np.abs(g_fd).max()
    assert np.abs(H - J.T @ J).max() <= 1e-6 * np.abs(H).max()
    terms, plane = ref._pair_terms(q, POSE_YAW, metric, return_plane=True)
    assert terms.shape == (sel.sum(), 28) and plane.all() == (metric == "plane")      # small_cloud's normals are unit vectors


def _drive():
    """scans 0..2 of the drive of seed 3 (16 beams, about 7.4k points), the map of scans 0 and 1 under the true poses"""
    from rslo_amd import synthetic
    from rslo_amd.mapping import VoxelMapRef
    if "drive" not in _CACHE:
        scans = [synthetic.sequence_scan(i, seed=3, n_el=16, n_az=520) for i in range(3)]
        poses = [synthetic.sequence_pose(i, seed=3) for i in range(3)]
        ref = VoxelMapRef(0.4, min_range=2.5, max_range=80.0)
        ref.insert(scans[0], poses[0])
        ref.insert(scans[1], poses[1])
        _CACHE["drive"] = scans, poses, ref
    return _CACHE["drive"]


def drive_start(true_pose):
    """the true pose of scan 2 with its translation moved by 0.1 * (0.6, -0.5, 0.2) m and its rotation followed by 0.15
    degrees about a fixed oblique axis"""
    axis = np.array([0.3, -0.4, 0.866])
    turned = _perturbed(np.concatenate([np.zeros(3), true_pose[3:]]),
                        np.concatenate([np.zeros(3), np.deg2rad(0.15) * axis / np.linalg.norm(axis)]))
    return np.concatenate([true_pose[:3] + 0.1 * np.array([0.6, -0.5, 0.2]), turned[3:]])


@pytest.mark.parametrize("metric,ratio", [("plane", 0.25), ("point", 0.5)])
def test_register_converges_on_the_drive(metric, ratio):
    scans, poses, ref = _drive()
    assert 7000 < len(scans[2]) < 8000
    start = drive_start(poses[2])
    e0 = np.linalg.norm(start[:3] - poses[2][:3])
    assert 0.08 < e0 < 0.083
    pose, info = ref.register(scans[2], start, iters=8, metric=metric)
    e1 = np.linalg.norm(pose[:3] - poses[2][:3])
    print("%s: translation error %.4f -> %.4f m (ratio %.3f), pairs %d, cost %.3f -> %.3f" % (
        metric, e0, e1, e1 / e0, info[-1, 1], info[0, 2], info[-1, 2]))
    assert (info[:, 0] == 0).all() and info[-1, 1] > 1000
    assert e1 <= ratio * e0
    assert abs(np.linalg.norm(pose[3:]) - 1.0) < 1e-12


def test_plane_metric_needs_the_point_fallback():
    """The drive's ground is level and the reader zeroes exactly vertical normals: the plane terms alone leave z, roll
    and pitch unobserved.  The matched points without a usable normal enter as point terms and make H definite."""
    scans, poses, ref = _drive()
    start = drive_start(poses[2])
    terms, plane = ref._pair_terms(scans[2], start, "plane", return_plane=True)
    assert plane.sum() > 500 and (~plane).sum() > 500

    def H_of(t):
        H = np.zeros((6, 6))
        H[np.triu_indices(6)] = t[:, :21].sum(axis=0)
        return H + np.triu(H, 1).T
    ev_plane = np.linalg.eigvalsh(H_of(terms[plane]))
    ev_all = np.linalg.eigvalsh(H_of(terms))
    print("eigenvalues, plane terms only:", ev_plane, "with the point terms:", ev_all)
    assert ev_plane[0] <= 1e-9 * ev_plane[-1]          # singular
    assert ev_all[0] > 1e-6 * ev_all[-1]               # definite
    assert ref.normal_equations(scans[2], start, "plane")[:28].tobytes() == terms.sum(axis=0).tobytes()
    # and every point term of the plane metric is a point whose normal the rule rejects
    w, idx, _ = ref._match(scans[2], start, None, 1)
    ns = scans[2][idx >= 0, 4:7].astype(np.float64)
    assert ((ns * ns).sum(axis=1)[~plane] < 0.25).all()


def test_argument_checks():
    from rslo_amd.mapping import VoxelMapRef
    ref = VoxelMapRef(0.4)
    ref.insert(_cloud(0), IDENT)
    with pytest.raises(ValueError):
        ref.normal_equations(_cloud(5)[:, :4], IDENT, "plane")      # no normals
    with pytest.raises(ValueError):
        ref.normal_equations(_cloud(5), IDENT, "surface")
    for iters in (0, 33):
        with pytest.raises(ValueError):
            ref.register(_cloud(5), IDENT, iters=iters)
    with pytest.raises(ValueError):
        ref.register(_cloud(5), IDENT, tol_t=-1.0)
    # status 2 and status 3
    pose, info = ref.register(_cloud(5), POSE_YAW, iters=2, damping=-1e30)
    assert info[:, 0].tolist() == [2.0, 2.0] and pose.tobytes() == POSE_YAW.tobytes()
    one, _ = ref.register(_cloud(5), POSE_YAW, iters=1)
    pose, info = ref.register(_cloud(5), POSE_YAW, iters=3, tol_t=1e9, tol_r=1e9)
    assert info[:, 0].tolist() == [0.0, 3.0, 3.0] and pose.tobytes() == one.tobytes()
    assert ref.register(_cloud(5)[:, :4], POSE_YAW, iters=1)[1][0, 0] == 0.0      # metric None: point for a [P, 4] cloud
