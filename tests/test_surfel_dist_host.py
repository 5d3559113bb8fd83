"""The point-to-distribution cost of the surfel map, float64 restatement (rslo_amd/surfels.py SurfelMapRef with
cost="distribution"; rules: include/rslo_hip.h "Distribution cost").  No GPU: the restatement is the arbiter of
tests/test_gpu_surfel_dist.py, so it is held here against things that do not share its code -- numpy.linalg.inv, a cell
whose information matrix is written out by hand, finite differences of the cost, the drive's true poses and a scene
without planes."""
import numpy as np
import pytest
from test_mapreg_host import IDENT, _perturbed, _rotmat, drive_start
from test_surfels_host import drive_ref, drive_scans, lattice

_CACHE = {}
PAIRS6 = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
POLE_START = np.array([0.06, -0.04, 0.03, np.cos(0.005), 0.0, 0.0, np.sin(0.005)])      # yaw 0.01 rad


def sym3(v6):
    """[n, 3, 3] symmetric matrices of rows [n, 6] in the order 00 01 02 11 12 22"""
    out = np.zeros((len(v6), 3, 3))
    for k, (a, b) in enumerate(PAIRS6):
        out[:, a, b] = out[:, b, a] = v6[:, k]
    return out


def pole_scene(seed=0):
    """A scene without planes at voxel 0.4: 24 poles (60 points each, z uniform in [-1, 2], x and y within 0.03 of the
    axis) and 24 blobs (60 points uniform in a cube of half-edge 0.15), axes and centres snapped to cell centres
    (k + 0.5) * 0.4 on rings of radius 5 .. 12 m.  -> (SurfelMapRef of all points under the identity, the points fp32
    [2880, 3], the scan: a random half of them); made once, never modified."""
    from rslo_amd.surfels import SurfelMapRef
    if ("poles", seed) not in _CACHE:
        rng = np.random.default_rng(seed)

        def centres(n):
            r, a = rng.uniform(5.0, 12.0, n), rng.uniform(0.0, 2 * np.pi, n)
            return (np.floor(np.stack([r * np.cos(a), r * np.sin(a)], axis=1) / 0.4) + 0.5) * 0.4
        pts = []
        for c in centres(24):
            pts.append(np.concatenate([c + rng.uniform(-0.03, 0.03, (60, 2)), rng.uniform(-1.0, 2.0, (60, 1))], axis=1))
        for c in centres(24):
            c3 = np.array([c[0], c[1], (np.floor(rng.uniform(-1.0, 2.0) / 0.4) + 0.5) * 0.4])
            pts.append(c3 + rng.uniform(-0.15, 0.15, (60, 3)))
        pts = np.concatenate(pts).astype(np.float32)
        ref = SurfelMapRef(0.4)
        ref.insert(pts, IDENT)
        scan = np.ascontiguousarray(pts[np.sort(rng.permutation(len(pts))[:len(pts) // 2])])
        _CACHE["poles", seed] = (ref, pts, scan)
    return _CACHE["poles", seed]


def test_information_against_numpy_inverse():
    from rslo_amd import surfels
    ref = drive_ref(0.4, 3)
    idx = np.nonzero(ref.rows[:, 7] >= 1.0)[0]
    assert len(idx) > 1000 and (ref.rows[idx, 7] == 1.0).sum() > 400 and (ref.rows[idx, 7] == 2.0).sum() > 500
    _, c, tr = surfels.covariances(ref.moments[idx])
    u = 0.4 / 16384.0
    C = sym3(c) * u * u
    for reg_rel, reg_abs in ((0.01, 0.02), (0.01, 0.01), (0.0, 0.02), (0.05, 0.0)):
        info = ref.information(idx, reg_rel, reg_abs)
        lam = reg_rel * np.trace(C, axis1=1, axis2=2) + reg_abs * reg_abs
        S = C + lam[:, None, None] * np.eye(3)
        want, cond = np.linalg.inv(S), np.linalg.cond(S)
        rel = np.abs(sym3(info[:, :6]) - want).max(axis=(1, 2)) / np.abs(want).max(axis=(1, 2))
        print("reg %g %g: %d cells, cond <= %.3g, worst relative error / (1e-9 cond) %.3g" % (
            reg_rel, reg_abs, len(idx), cond.max(), (rel / (1e-9 * cond)).max()))
        assert (rel <= 1e-9 * cond).all()
        assert (info[:, 6] > 0).all() and np.isfinite(info[:, 6]).all()
        assert np.abs(info[:, 6] - np.linalg.det(S)).max() <= 1e-9 * np.abs(info[:, 6]).max()
        assert np.abs(info[:, 7] - lam).max() <= 1e-15 * lam.max()
    # by key and by index: the same rows
    assert ref.information(ref.keys[idx]).tobytes() == ref.information(idx).tobytes()
    with pytest.raises(ValueError):
        ref.information([1 << 62])                          # a key that is not in the map


def test_hand_made_cell():
    """The lattice of test_hand_made_plane in one cell of a 1 m grid: x and y are k/8, z = x/4, k = 1 .. 5.  The variance
    of k is 2, so C = [[1/32, 0, 1/128], [0, 1/32, 0], [1/128, 0, 1/512]] exactly.  reg_rel = 0, reg_abs = 1/16 give
    lam = 1/256 and, in units of 1/256, S = [[9, 0, 2], [0, 9, 0], [2, 0, 1.5]]: adj = [[13.5, 0, -18], [0, 9.5, 0],
    [-18, 0, 81]], det = 9 * 13.5 - 2 * 18 = 85.5.  Every product is exact in binary, so M = 256 * adj / 85.5 to the bit."""
    from rslo_amd.surfels import SurfelMapRef
    ref = SurfelMapRef(1.0)
    ref.insert(lattice(), IDENT)
    info = ref.information([0], reg_rel=0.0, reg_abs=0.0625)
    want = [768.0 / 19.0, 0.0, -1024.0 / 19.0, 256.0 / 9.0, 0.0, 4608.0 / 19.0, 85.5 / 256.0 ** 3, 1.0 / 256.0]
    assert info[0].tolist() == want
    # reg_rel alone: trace = 33/512, reg_rel = 1/4 -> lam = 33/2048; S in units of 1/2048: [[97, 0, 16], [0, 97, 0], [16, 0, 37]]
    info = ref.information(ref.keys[:1], reg_rel=0.25, reg_abs=0.0)
    det = 97.0 * (97.0 * 37.0) - 16.0 * (16.0 * 97.0)
    want = [2048.0 * 97.0 * 37.0 / det, 0.0, -2048.0 * 16.0 * 97.0 / det, 2048.0 * (97.0 * 37.0 - 256.0) / det, 0.0,
            2048.0 * 97.0 * 97.0 / det, det / 2048.0 ** 3, 33.0 / 2048.0]
    assert info[0].tolist() == want
    # the cost of a point one cell-sigma above the mean along y is 1 / (1 + lam / C11)
    keys, d2, rows, inf = ref.nearest(np.array([[0.375, 0.375 + np.sqrt(1 / 32), 0.09375]], np.float32), IDENT, return_rows=True,
                                      cost="distribution", reg_rel=0.0, reg_abs=0.0625, return_info=True)
    assert keys[0] == ref.keys[0] and rows[0, 7] == 2.0 and inf[0].tolist() == ref.information([0], 0.0, 0.0625)[0].tolist()
    out = ref.normal_equations(np.array([[0.375, 0.375 + np.sqrt(1 / 32), 0.09375]], np.float32), IDENT, cost="distribution",
                               reg_rel=0.0, reg_abs=0.0625)
    assert out[28] == 1.0 and abs(out[27] - 1.0 / (1.0 + 32.0 / 256.0)) < 1e-3


def test_jacobian_against_finite_differences():
    """g and H by central differences of e = d^T M d written here from the definition (rotation matrices,
    numpy.linalg.inv), over the correspondences of the base pose; the construction and the bars of
    tests/test_surfels_host.py::test_jacobian_against_finite_differences."""
    from rslo_amd import surfels
    ref = drive_ref(0.4, 2)
    scans, poses = drive_scans()
    q, base = scans[2][:, :4], drive_start(poses[2])
    keys, _, rows = ref.nearest(q, base, return_rows=True, cost="distribution")
    sel = keys >= 0
    assert sel.sum() > 4000 and (rows[sel, 7] == 1.0).sum() > 500
    p, mean = q[sel, :3].astype(np.float64), rows[sel, :3]
    _, c, tr = surfels.covariances(ref.moments[np.searchsorted(ref.keys, keys[sel])])
    u = 0.4 / 16384.0
    C = sym3(c) * u * u
    M = np.linalg.inv(C + (0.01 * np.trace(C, axis1=1, axis2=2) + 0.02 * 0.02)[:, None, None] * np.eye(3))

    def residuals(delta):
        pose = _perturbed(base, delta)
        return p @ _rotmat(pose[3:]).T + pose[:3] - mean

    def costs(delta):
        d = residuals(delta)
        return np.einsum("na,nab,nb->n", d, M, d)

    eps = 1e-6
    e0 = costs(np.zeros(6))
    J = np.stack([(residuals(eps * e) - residuals(-eps * e)) / (2 * eps) for e in np.eye(6)], axis=2)      # [n, 3, 6]
    g_fd = np.array([(0.5 * costs(eps * e).sum() - 0.5 * costs(-eps * e).sum()) / (2 * eps) for e in np.eye(6)])
    H_fd = np.einsum("nak,nab,nbl->kl", J, M, J)
    out = ref.normal_equations(q, base, cost="distribution")
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = out[:21]
    H = H + np.triu(H, 1).T
    assert out[28] == sel.sum()
    assert abs(out[27] - e0.sum()) <= 1e-12 * e0.sum()
    assert np.abs(out[21:27] - g_fd).max() <= 1e-6 * np.abs(g_fd).max()
    assert np.abs(H - H_fd).max() <= 1e-6 * np.abs(H).max()
    # the weighted sums are the weighted addends
    terms = ref._pair_terms(q, base, dist=(1, 0.01, 0.02))
    rho = (9.0 / (9.0 + terms[:, 27])) ** 2
    got = ref.normal_equations(q, base, robust_scale=3.0, cost="distribution")
    assert np.allclose(got[:28], (terms * rho[:, None]).sum(axis=0), rtol=1e-12) and got[28] == len(terms)
    assert np.abs(terms[:, 27] - e0).max() <= 1e-12 * e0.max()


def test_register_converges_on_the_drive():
    ref = drive_ref(0.4, 2)
    assert (ref.rows[:, 7] == 2.0).sum() == 600 and (ref.rows[:, 7] == 1.0).sum() == 534
    scans, poses = drive_scans()
    start = drive_start(poses[2])
    e0 = np.linalg.norm(start[:3] - poses[2][:3])
    plane, pinfo = ref.register(scans[2][:, :3], start, iters=8)
    pose, info = ref.register(scans[2][:, :3], start, iters=8, cost="distribution", robust_scale=3.0)
    e1, ep = np.linalg.norm(pose[:3] - poses[2][:3]), np.linalg.norm(plane[:3] - poses[2][:3])
    print("distribution: translation error %.4f -> %.4f m (ratio %.3f), pairs %d; plane: -> %.4f m, pairs %d" % (
        e0, e1, e1 / e0, info[-1, 1], ep, pinfo[-1, 1]))
    assert (info[:, 0] == 0).all() and e1 <= 0.25 * e0
    assert (info[:, 1] > pinfo[:, 1]).all()                 # strictly more pairs than the plane cost, in every iteration
    assert abs(np.linalg.norm(pose[3:]) - 1.0) < 1e-12
    # min_flag=2 restricts the distribution cost to the plane cost's cells
    k2, d2 = ref.nearest(scans[2], start, cost="distribution", min_flag=2)
    kp, dp = ref.nearest(scans[2], start)
    assert k2.tobytes() == kp.tobytes() and d2.tobytes() == dp.tobytes()


def test_scene_without_planes():
    ref, _, scan = pole_scene()
    flags = [int((ref.rows[:, 7] == f).sum()) for f in (0.0, 1.0, 2.0)]
    e0 = np.linalg.norm(POLE_START[:3])
    _, pinfo = ref.register(scan, POLE_START, iters=8, damping=1e-6)
    pose, info = ref.register(scan, POLE_START, iters=8, damping=1e-6, cost="distribution", robust_scale=3.0)
    e1, ang = np.linalg.norm(pose[:3]), 2 * np.arccos(min(1.0, abs(pose[3])))
    print("flags 0/1/2 %s; plane: status %s pairs %s; distribution: status %s pairs %d of %d, %.4f -> %.4f m (ratio %.3f), "
          "angle 0.01 -> %.4f rad" % (flags, pinfo[:, 0].tolist(), pinfo[:, 1].tolist(), info[:, 0].tolist(), info[-1, 1],
                                      len(scan), e0, e1, e1 / e0, ang))
    assert len(scan) == 1440 and flags[1] > 100 and flags[2] < 10
    assert (pinfo[:, 0] == 1).all() and (pinfo[:, 1] <= 49).all()       # fewer than min_pairs = 50: not refined at all
    assert (info[:, 0] == 0).all() and info[-1, 1] > 1000
    assert e1 <= 0.25 * e0


def test_argument_checks():
    from rslo_amd import surfels
    ref = drive_ref(0.4, 2)
    scans, poses = drive_scans()
    pts, start = scans[2][:200], drive_start(poses[2])
    nan = float("nan")
    bad = [dict(min_flag=0), dict(min_flag=3), dict(reg_rel=0.0, reg_abs=0.0), dict(reg_rel=-0.01), dict(reg_abs=-0.02),
           dict(reg_rel=nan), dict(reg_abs=nan), dict(reg_abs=float("inf"))]
    for kw in bad:
        for call in (ref.nearest, ref.normal_equations, ref.register):
            with pytest.raises(ValueError):
                call(pts, start, cost="distribution", **kw)
    with pytest.raises(ValueError):
        ref.information([0], 0.0, 0.0)
    with pytest.raises(ValueError):
        ref.nearest(pts, start, cost="ndt")
    # the new options together with cost="plane"
    for kw in (dict(min_flag=1), dict(reg_rel=0.01), dict(reg_abs=0.02)):
        for call in (ref.nearest, ref.normal_equations, ref.register):
            with pytest.raises(ValueError):
                call(pts, start, **kw)
            with pytest.raises(ValueError):
                call(pts, start, cost="plane", **kw)
    with pytest.raises(ValueError):
        ref.nearest(pts, start, return_info=True)
    # surfel_refine options
    plane = surfels.check_surfel_refine({}, ref)
    assert plane == surfels.SURFEL_REFINE_DEFAULTS and surfels.check_surfel_refine(dict(cost="plane"), ref) == plane
    assert surfels.SURFEL_REFINE_DEFAULTS == dict(iters=4, max_dist=None, robust_scale=0.2, damping=1e-6, min_pairs=50,
                                                  tol_t=0.0, tol_r=0.0)
    dist = surfels.check_surfel_refine(dict(cost="distribution"), ref)
    assert dist == dict(plane, robust_scale=3.0, cost="distribution", min_flag=1, reg_rel=0.01, reg_abs=0.02)
    assert surfels.check_surfel_refine(dict(cost="distribution", robust_scale=2.0, reg_abs=0.01, iters=2), ref) == dict(
        dist, robust_scale=2.0, reg_abs=0.01, iters=2)
    for opts in (dict(metric="plane"), dict(cost="distribution", lam=1.0), dict(cost="ndt"), dict(reg_abs=0.01),
                 dict(cost="plane", min_flag=1), dict(cost="distribution", min_flag=0),
                 dict(cost="distribution", reg_rel=0.0, reg_abs=0.0)):
        with pytest.raises(ValueError):
            surfels.check_surfel_refine(opts, ref)
    # the options reach register: a dict from check_surfel_refine is its keyword arguments
    a, ia = ref.register(pts, start, **dist)
    b, ib = ref.register(pts, start, iters=4, damping=1e-6, robust_scale=3.0, cost="distribution")
    assert a.tobytes() == b.tobytes() and ia.tobytes() == ib.tobytes()


def test_plane_cost_is_untouched():
    """cost="plane" returns the bytes of a call without the keyword."""
    ref = drive_ref(0.4, 2)
    scans, poses = drive_scans()
    pts, start = scans[2], drive_start(poses[2])
    for a, b in zip(ref.nearest(pts, start, return_rows=True), ref.nearest(pts, start, return_rows=True, cost="plane")):
        assert a.tobytes() == b.tobytes()
    assert len(ref.nearest(pts, start, cost="plane", min_flag=2)) == 2
    for scale in (0.0, 0.2):
        assert ref.normal_equations(pts, start, robust_scale=scale).tobytes() == ref.normal_equations(
            pts, start, robust_scale=scale, cost="plane").tobytes()
        a, ia = ref.register(pts, start, iters=3, robust_scale=scale)
        b, ib = ref.register(pts, start, iters=3, robust_scale=scale, cost="plane")
        assert a.tobytes() == b.tobytes() and ia.tobytes() == ib.tobytes()
    # and the distribution cost is another result
    assert ref.normal_equations(pts, start, cost="distribution").tobytes() != ref.normal_equations(pts, start).tobytes()
