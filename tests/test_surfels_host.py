"""Surfel map, the float64 restatement (rslo_amd/surfels.py SurfelMapRef; rules: include/rslo_hip.h "Surfel map").  No
GPU: the restatement is the arbiter of tests/test_gpu_surfels.py, so it is held here against things that do not share
its code -- hand-computed integer moments, numpy.linalg.eigh, an all-pairs search, finite differences of the cost, and
the drive's true poses."""
import numpy as np
import pytest
from test_mapreg_host import IDENT, POSE_YAW, _cloud, _perturbed, _pts, _rotmat, drive_start

_CACHE = {}
DRIVE_ARGS = dict(min_range=2.5, max_range=80.0)


def drive_scans(n=3):
    """scans and true poses 0 .. n-1 of the 16-beam drive of seed 3 (tests/test_mapreg_host.py::_drive)"""
    from rslo_amd import synthetic
    if ("scans", n) not in _CACHE:
        _CACHE["scans", n] = ([synthetic.sequence_scan(i, seed=3, n_el=16, n_az=520) for i in range(n)],
                              [synthetic.sequence_pose(i, seed=3) for i in range(n)])
    return _CACHE["scans", n]


def drive_ref(voxel, n_scans, **kw):
    """SurfelMapRef of the drive's first n_scans scans under their true poses; made once, never modified"""
    from rslo_amd.surfels import SurfelMapRef
    key = ("ref", voxel, n_scans, tuple(sorted(kw.items())))
    if key not in _CACHE:
        scans, poses = drive_scans()
        ref = SurfelMapRef(voxel, **dict(DRIVE_ARGS, **kw))
        for s, p in zip(scans[:n_scans], poses[:n_scans]):
            ref.insert(s, p)
        _CACHE[key] = ref
    return _CACHE[key]


def lattice():
    """5 x 5 points on the plane z = 0.25 x inside the cell (0, 0, 0) of a 1 m grid; every coordinate a multiple of 1/32"""
    g = np.arange(1, 6) * 0.125
    x, y = np.meshgrid(g, g, indexing="ij")
    return _pts(*zip(x.ravel(), y.ravel(), 0.25 * x.ravel()))


def test_hand_made_plane():
    from rslo_amd.surfels import SurfelMapRef
    ref = SurfelMapRef(1.0)
    ref.insert(lattice(), IDENT)
    keys, mom, rows = ref.cells(min_flag=0)
    assert keys.tolist() == [(1 << 20 << 42) | (1 << 20 << 21) | (1 << 20)]
    # q = 2048 k along x and y, 512 k along z, k = 1 .. 5: sum k = 15, sum k^2 = 55, each value five times
    a, b = 2048, 512
    want = [25, 5 * a * 15, 5 * a * 15, 5 * b * 15, 5 * a * a * 55, (a * 15) * (a * 15), 5 * a * b * 55, 5 * a * a * 55,
            (a * 15) * (b * 15), 5 * b * b * 55]
    assert mom.tolist() == [want]
    mean = np.array([0.375, 0.375, 0.09375]) + 0.5 / 16384
    assert np.abs(rows[0, :3] - mean).max() < 1e-15
    n = np.array([-0.25, 0.0, 1.0]) / np.sqrt(1.0625)            # the largest component is made positive
    assert np.abs(rows[0, 3:6] - n).max() < 1e-12 and rows[0, 5] > 0
    assert rows[0, 7] == 2.0 and abs(rows[0, 6]) < 1e-12         # planar; no spread along the normal
    assert ref.stats() == dict(n_scans=1, n_cells=1, n_points=25, dropped_invalid=0, dropped_range=0, dropped_full=0,
                               n_planar=1)
    # the mirrored plane z = 0.75 - 0.25 x: the same rule gives (+0.25, 0, 1) / |.|
    mir = lattice()
    mir[:, 2] = 0.75 - mir[:, 2]
    ref2 = SurfelMapRef(1.0)
    ref2.insert(mir, IDENT)
    assert np.abs(ref2.cells()[2][0, 3:6] - np.array([0.25, 0.0, 1.0]) / np.sqrt(1.0625)).max() < 1e-12
    # a plane whose largest normal component would be negative is flipped: x = 0.5 + 0.25 z has normal +-(1, 0, -0.25)
    g = np.arange(1, 6) * 0.125
    z, y = np.meshgrid(g, g, indexing="ij")
    ref3 = SurfelMapRef(1.0)
    ref3.insert(_pts(*zip(0.5 + 0.25 * z.ravel(), y.ravel(), z.ravel())), IDENT)
    assert np.abs(ref3.cells()[2][0, 3:6] - np.array([1.0, 0.0, -0.25]) / np.sqrt(1.0625)).max() < 1e-12


def test_hand_made_line_few_points_clamp_and_face():
    from rslo_amd.surfels import SurfelMapRef
    ref = SurfelMapRef(1.0)
    k = np.arange(1, 7)
    ref.insert(_pts(*zip(0.125 * k, 0.0625 * k + 0.25, 0.03125 * k + 0.5)), IDENT)      # six points on one oblique line
    _, mom, rows = ref.cells(min_flag=0)
    assert mom[0, 0] == 6 and rows[0, 7] == 1.0 and ref.stats()["n_planar"] == 0 and len(ref.cells(min_flag=2)[0]) == 0
    # four points with min_points = 5: flag 0, a row of zeros; the fifth makes a plane of them
    ref = SurfelMapRef(1.0)
    four = _pts((0.25, 0.25, 0.5), (0.75, 0.25, 0.5), (0.25, 0.75, 0.5), (0.75, 0.75, 0.5))
    ref.insert(four, IDENT)
    assert ref.cells(min_flag=0)[1][0, 0] == 4 and not ref.cells(min_flag=0)[2].any() and len(ref.cells()[0]) == 0
    ref.insert(_pts((0.5, 0.5, 0.5)), IDENT)
    assert ref.cells()[2][0].tolist() == [0.5 + 0.5 / 16384] * 3 + [0.0, 0.0, 1.0, 0.0, 2.0]
    with_three = SurfelMapRef(1.0, min_points=3)
    with_three.insert(four, IDENT)
    assert with_three.cells()[2][0, 7] == 2.0
    # a tiny negative coordinate: s - floor(s) rounds to 1.0, the clamp holds q at 16383, the cell is -1
    ref = SurfelMapRef(1.0)
    ref.insert(_pts((-1e-30, 0.5, 0.5)), IDENT)
    keys, mom, _ = ref.cells(min_flag=0)
    assert ((keys[0] >> 42) & 0x1fffff) - (1 << 20) == -1 and mom[0, :4].tolist() == [1, 16383, 8192, 8192]
    assert mom[0, 4] == 16383 * 16383
    # a point exactly on a cell face goes to the upper cell, with q = 0
    ref = SurfelMapRef(1.0)
    ref.insert(_pts((1.0, 0.5, 0.5), (-1.0, 0.5, 0.5)), IDENT)
    keys, mom, _ = ref.cells(min_flag=0)
    assert (((keys >> 42) & 0x1fffff) - (1 << 20)).tolist() == [-1, 1] and mom[:, 1].tolist() == [0, 0]
    # invalid, gated and out-of-range points are counted, not stored
    ref = SurfelMapRef(1.0, min_range=1.0, max_range=10.0)
    ref.insert(_pts((np.nan, 0, 0), (0.5, 0, 0), (20.0, 0, 0), (2.0, 0, 0)), IDENT)
    ref.insert(_pts((3.0, 0, 0)), np.array([3e6, 0, 0, 1, 0, 0, 0.0]))
    assert ref.stats() == dict(n_scans=2, n_cells=1, n_points=1, dropped_invalid=3, dropped_range=1, dropped_full=0,
                               n_planar=0)


def test_order_freedom():
    from rslo_amd.surfels import SurfelMapRef
    A, B = _cloud(0), _cloud(5)
    B = B + np.array([0.3, -0.2, 0.05, 0, 0, 0, 0], np.float32)
    ab, ba, one = SurfelMapRef(2.0), SurfelMapRef(2.0), SurfelMapRef(2.0)
    ab.insert(A, POSE_YAW), ab.insert(B, POSE_YAW)
    ba.insert(B, POSE_YAW), ba.insert(A, POSE_YAW)
    one.insert(np.concatenate([A, B])[np.random.RandomState(0).permutation(len(A) + len(B))], POSE_YAW)
    assert len(ab.keys) > 50 and ab.stats()["n_planar"] > 10
    for other in (ba, one):
        assert ab.keys.tobytes() == other.keys.tobytes() and ab.moments.tobytes() == other.moments.tobytes()
        assert ab.rows.tobytes() == other.rows.tobytes()
    assert ab.stats() == ba.stats()
    assert ab.stats()["n_scans"] == 2 and one.stats() == dict(ab.stats(), n_scans=1)
    # and the rows are a function of the moments alone
    assert ab.derive_rows().tobytes() == ab.rows.tobytes()


@pytest.mark.parametrize("voxel", [0.4, 1.6])
def test_jacobi_twin_against_eigh(voxel):
    """The normal of EVERY planar cell of the 3-scan drive within 1e-4 degrees of numpy.linalg.eigh's eigenvector: the
    planar rule itself keeps the gap l1 - l0 >= 0.9 l1 >= 0.045 l2, so no cell is excluded."""
    from rslo_amd import surfels
    ref = drive_ref(voxel, 3)
    keys, mom, rows = ref.cells(min_flag=1)
    mu, c, tr = surfels.covariances(mom)
    C = np.zeros((len(keys), 3, 3))
    for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        C[:, a, b] = C[:, b, a] = c[:, k]
    planar = rows[:, 7] == 2.0
    assert planar.sum() > (500 if voxel == 0.4 else 150)
    ev, vec = np.linalg.eigh(C[planar])
    dots = np.abs((vec[:, :, 0] * rows[planar, 3:6]).sum(axis=1))
    sin = np.linalg.norm(np.cross(vec[:, :, 0], rows[planar, 3:6]), axis=1)
    ang = np.degrees(np.arctan2(sin, dots))
    print("voxel %.1f: %d cells, %d planar; worst angle to eigh %.3g deg" % (voxel, len(keys), planar.sum(), ang.max()))
    assert ang.max() <= 1e-4
    assert np.abs(np.linalg.norm(rows[planar, 3:6], axis=1) - 1.0).max() < 1e-15
    # sigma2 is the smallest eigenvalue in m^2
    u = voxel / 16384.0
    assert np.abs(rows[planar, 6] - ev[:, 0] * u * u).max() <= 1e-12 * (ev[:, -1] * u * u).max()
    # the off-diagonal residue after six sweeps is exactly zero on every cell with a row
    a = [c[:, k] / tr for k in range(6)]
    _, off, _ = surfels.jacobi_eig(*a)
    assert all((o == 0.0).all() for o in off)


def test_nearest_equals_brute_force():
    ref = drive_ref(0.4, 2)
    scans, poses = drive_scans()
    start = drive_start(poses[2])
    md = 0.9 * 0.4
    keys, d2, rows = ref.nearest(scans[2], start, max_dist=md, return_rows=True)
    pk, _, prow = ref.cells(min_flag=2)
    status, _, w = ref._cells(scans[2], start)
    want_keys = np.full((len(w),), -1, np.int64)
    want_d2 = np.full((len(w),), -1.0)
    for lo in range(0, len(w), 1024):
        d = w[lo:lo + 1024, None, :] - prow[None, :, :3]
        all2 = d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1] + d[:, :, 2] * d[:, :, 2]
        for i in range(len(all2)):
            if status[lo + i]:
                continue
            j = np.lexsort((pk, all2[i]))[0]          # by d2, then by key
            if all2[i, j] < md * md:
                want_keys[lo + i], want_d2[lo + i] = pk[j], all2[i, j]
    assert (want_keys >= 0).sum() > 1000 and (want_keys < 0).sum() > 1000
    assert (keys == want_keys).all() and d2.tobytes() == want_d2.tobytes()
    got = keys >= 0
    assert (rows[got] == prow[np.searchsorted(pk, keys[got])]).all() and not rows[~got].any()


def test_jacobian_against_finite_differences():
    """g and H by central differences of residuals written here from the definition, over the correspondences of the
    base pose; the bars of tests/test_mapreg_host.py."""
    ref = drive_ref(0.4, 2)
    scans, poses = drive_scans()
    q, base = scans[2][:, :4], drive_start(poses[2])
    keys, _, rows = ref.nearest(q, base, return_rows=True)
    sel = keys >= 0
    assert sel.sum() > 1000
    p, m, n0 = q[sel, :3].astype(np.float64), rows[sel, :3], rows[sel, 3:6]

    def residuals(delta):
        pose = _perturbed(base, delta)
        return (n0 * (p @ _rotmat(pose[3:]).T + pose[:3] - m)).sum(axis=1)

    eps = 1e-6
    r0 = residuals(np.zeros(6))
    J = np.stack([(residuals(eps * e) - residuals(-eps * e)) / (2 * eps) for e in np.eye(6)], axis=1)
    g_fd = np.array([(0.5 * (residuals(eps * e) ** 2).sum() - 0.5 * (residuals(-eps * e) ** 2).sum()) / (2 * eps)
                     for e in np.eye(6)])
    out = ref.normal_equations(q, base)
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = out[:21]
    H = H + np.triu(H, 1).T
    assert out[28] == sel.sum()
    assert abs(out[27] - r0 @ r0) <= 1e-12 * (r0 @ r0)
    assert np.abs(out[21:27] - g_fd).max() <= 1e-6 * np.abs(g_fd).max()
    assert np.abs(H - J.T @ J).max() <= 1e-6 * np.abs(H).max()
    # the weighted sums are the weighted addends
    terms = ref._pair_terms(q, base)
    rho = (0.04 / (0.04 + terms[:, 27])) ** 2
    assert np.allclose(ref.normal_equations(q, base, robust_scale=0.2)[:28], (terms * rho[:, None]).sum(axis=0), rtol=1e-12)
    assert ref.normal_equations(q, base, robust_scale=0.2)[28] == len(terms)


def test_register_converges_on_the_drive():
    ref = drive_ref(0.4, 2)
    scans, poses = drive_scans()
    start = drive_start(poses[2])
    e0 = np.linalg.norm(start[:3] - poses[2][:3])
    assert 0.08 < e0 < 0.083
    pose, info = ref.register(scans[2][:, :3], start, iters=8)           # [P, 3]: no normal, no intensity
    e1 = np.linalg.norm(pose[:3] - poses[2][:3])
    print("surfels: translation error %.4f -> %.4f m (ratio %.3f), pairs %d, cost %.3f -> %.3f; %d of %d cells planar" % (
        e0, e1, e1 / e0, info[-1, 1], info[0, 2], info[-1, 2], ref.stats()["n_planar"], ref.stats()["n_cells"]))
    assert (info[:, 0] == 0).all() and info[-1, 1] > 1000
    assert e1 <= 0.25 * e0
    assert abs(np.linalg.norm(pose[3:]) - 1.0) < 1e-12


def test_save_ply(tmp_path):
    ref = drive_ref(1.6, 3)
    path = tmp_path / "surfels.ply"
    ref.save_ply(str(path))
    raw = path.read_bytes()
    head, body = raw.split(b"end_header\n", 1)
    rows = ref.cells(min_flag=2)[2]
    assert b"element vertex %d\n" % len(rows) in head and b"property float nz" in head and len(rows) > 100
    got = np.frombuffer(body, "<f4").reshape(-1, 6)
    assert got.tobytes() == rows[:, :6].astype("<f4").tobytes()


def test_argument_checks():
    from rslo_amd.surfels import SurfelMapRef
    ref = drive_ref(0.4, 2)
    scans, poses = drive_scans()
    start = drive_start(poses[2])
    for iters in (0, 33):
        with pytest.raises(ValueError):
            ref.register(scans[2], start, iters=iters)
    with pytest.raises(ValueError):
        ref.register(scans[2], start, tol_t=-1.0)
    for bad in (0.5, 0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            ref.nearest(scans[2], start, max_dist=bad)
        with pytest.raises(ValueError):
            ref.register(scans[2], start, max_dist=bad)
    for bad in (-0.1, float("nan"), float("inf"), 1e200):
        with pytest.raises(ValueError):
            ref.normal_equations(scans[2], start, robust_scale=bad)
    for kw in (dict(min_points=2), dict(min_points=5.5), dict(planar_ratio=-1.0), dict(line_ratio=float("nan")),
               dict(voxel_size=0.0), dict(min_range=2.0, max_range=1.0)):
        with pytest.raises(ValueError):
            SurfelMapRef(**kw)
    # statuses 1 (an empty map), 2 and 3
    empty = SurfelMapRef(0.4)
    pose, info = empty.register(scans[2], start, iters=2)
    assert pose.tobytes() == start.tobytes() and info[:, 0].tolist() == [1.0, 1.0] and info[:, 1].tolist() == [0.0, 0.0]
    assert empty.normal_equations(scans[2], start).tolist() == [0.0] * 29
    pose, info = ref.register(scans[2], start, iters=2, damping=-1e30)
    assert info[:, 0].tolist() == [2.0, 2.0] and pose.tobytes() == start.tobytes()
    one, _ = ref.register(scans[2], start, iters=1)
    pose, info = ref.register(scans[2], start, iters=3, tol_t=1e9, tol_r=1e9)
    assert info[:, 0].tolist() == [0.0, 3.0, 3.0] and pose.tobytes() == one.tobytes()
    # points on one plane only: the system is singular without damping
    flat = SurfelMapRef(1.0)
    g = (np.arange(40) + 0.5) * 0.125
    x, y = np.meshgrid(g, g, indexing="ij")
    floor = _pts(*zip(x.ravel(), y.ravel(), np.full(x.size, 0.5)))
    flat.insert(floor, IDENT)
    assert flat.stats()["n_planar"] == 25
    pose, info = flat.register(floor, IDENT, iters=1)
    assert info[0, 0] == 2.0 and info[0, 1] == 1600
