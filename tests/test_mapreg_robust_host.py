"""Coarse-to-fine robust scan-to-map registration, the float64 restatement (rslo_amd/mapping.py VoxelMapRef robust_scale=,
MapPyramidRef; rules: include/rslo_hip.h "Robust weight" and "Scheduled register").  No GPU: the restatement is the
arbiter of tests/test_gpu_mapreg_robust.py, so it is held here against a scalar evaluation of the formula on hand-made
cells, against today's unweighted outputs, and against the basin figures the pyramid was proposed with."""
import math

import numpy as np
import pytest
from stream_support import disturbed, turned

IDENT = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
POSE_YAW = np.array([1.0, -0.5, 0.1, np.cos(0.15), 0.0, 0.0, np.sin(0.15)], np.float64)
PYRAMID = (1.6, 0.8, 0.4)
GATE = dict(min_range=2.5, max_range=80.0)
_CACHE = {}


def _cloud(seed):
    from rslo_amd import synthetic
    if ("cloud", seed) not in _CACHE:
        _CACHE["cloud", seed] = synthetic.small_cloud(4000, seed=seed)
    return _CACHE["cloud", seed]


def _drive():
    """scans 0..2 of the drive of seed 3 (16 beams), scans 0 and 1 under their true poses in a pyramid (1.6, 0.8, 0.4);
    made once and never modified"""
    from rslo_amd import synthetic
    from rslo_amd.mapping import MapPyramidRef
    if "drive" not in _CACHE:
        scans = [synthetic.sequence_scan(i, seed=3, n_el=16, n_az=520) for i in range(3)]
        poses = [synthetic.sequence_pose(i, seed=3) for i in range(3)]
        pyr = MapPyramidRef(PYRAMID, **GATE)
        for s, p in zip(scans[:2], poses[:2]):
            pyr.insert(s, p)
        _CACHE["drive"] = scans, poses, pyr
    return _CACHE["drive"]


def _err(pose, true):
    return float(np.linalg.norm(pose[:3] - true[:3]))


# ---------------------------------------------------------------------------------------------------------------------
# the weight
# ---------------------------------------------------------------------------------------------------------------------
def _unweighted_today(ref, pts, pose, metric):
    """normal_equations as it was before robust_scale existed: the column sums of _pair_terms and the pair count"""
    terms = ref._pair_terms(pts, pose, metric)
    return np.concatenate([terms.sum(axis=0), [float(len(terms))]])


@pytest.mark.parametrize("metric", ["point", "plane"])
def test_scale_zero_keeps_todays_bits(metric):
    from rslo_amd.mapping import VoxelMapRef
    ref = VoxelMapRef(0.4)
    ref.insert(_cloud(0), IDENT)
    q = _cloud(5)
    want = _unweighted_today(ref, q, POSE_YAW, metric)
    assert want[28] > 100
    assert ref.normal_equations(q, POSE_YAW, metric).tobytes() == want.tobytes()
    assert ref.normal_equations(q, POSE_YAW, metric, robust_scale=0).tobytes() == want.tobytes()
    assert ref.normal_equations(q, POSE_YAW, metric, robust_scale=0.0).tobytes() == want.tobytes()
    # register: today's loop, written out with today's pieces
    from rslo_amd.gauss_newton import gauss_newton_step
    pose = POSE_YAW.copy()
    rows = []
    for _ in range(3):
        sums = _unweighted_today(ref, q, pose, metric)
        pose, nt, th = gauss_newton_step(sums[:28], pose, 0.0)
        rows.append([0.0, sums[28], sums[27], nt, th, 0.0, 0.0, 0.0])
    for kw in ({}, dict(robust_scale=0), dict(robust_scale=0.0)):
        got, info = ref.register(q, POSE_YAW, iters=3, metric=metric, **kw)
        assert got.tobytes() == pose.tobytes() and info.tobytes() == np.array(rows).tobytes()


def _hand_map():
    """a 5 x 5 patch of the plane z = 0.5 with one stored point per cell of edge 1, and a scan of 60 points hovering up
    to 0.2 above and below it with unit normals near +z; (map, scan [60, 7])"""
    from rslo_amd.mapping import VoxelMapRef
    ref = VoxelMapRef(1.0)
    g = np.arange(5, dtype=np.float32) + np.float32(0.5)
    cells = np.stack([np.repeat(g, 5), np.tile(g, 5), np.full((25,), 0.5, np.float32)], axis=1)
    ref.insert(cells)
    assert len(ref.keys) == 25
    rng = np.random.RandomState(11)
    scan = np.zeros((60, 7), np.float32)
    scan[:, 0:2] = rng.uniform(0.6, 4.4, (60, 2))
    scan[:, 2] = 0.5 + rng.uniform(-0.2, 0.2, 60)
    n = np.array([0.0, 0.0, 1.0]) + rng.uniform(-0.2, 0.2, (60, 3))
    scan[:, 4:7] = n / np.linalg.norm(n, axis=1, keepdims=True)
    scan[7, 4:7] = 0.0                                  # a zeroed normal: a point term under the plane metric
    return ref, scan


def _scalar_sums(ref, scan, pose, metric, scale):
    """The rules evaluated point by point in scalar Python floats: nearest stored row by exhaustive search, the term's
    addends from the definition, the Geman-McClure weight, sums in input order.  Shares no code with _pair_terms."""
    t, qw, v = [float(x) for x in pose[:3]], float(pose[3]), [float(x) for x in pose[4:7]]

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

    def rot(p):
        b = cross(v, p)
        c = cross(v, b)
        return [p[a] + (2.0 * b[a] * qw + 2.0 * c[a]) for a in range(3)]
    rows = [[float(x) for x in r[:3]] for r in ref.rows]
    sums = [0.0] * 28
    pairs = 0
    s2 = scale * scale
    for pt in scan:
        w = [t[a] + x for a, x in enumerate(rot([float(x) for x in pt[:3]]))]
        best, bd2 = None, None
        for m in rows:
            d = [w[a] - m[a] for a in range(3)]
            d2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
            if bd2 is None or d2 < bd2:
                best, bd2 = d, d2
        if not bd2 < 1.0:                               # max_dist = voxel = 1
            continue
        d = best
        ns = [float(x) for x in pt[4:7]]
        if metric == "plane" and ns[0] * ns[0] + ns[1] * ns[1] + ns[2] * ns[2] >= 0.25:
            n = rot(ns)
            J = [n + cross(w, n)]
            r = [n[0] * d[0] + n[1] * d[1] + n[2] * d[2]]
        else:
            J = [[1.0, 0.0, 0.0, 0.0, w[2], -w[1]], [0.0, 1.0, 0.0, -w[2], 0.0, w[0]], [0.0, 0.0, 1.0, w[1], -w[0], 0.0]]
            r = d
        e = sum(x * x for x in r)
        u = s2 / (s2 + e) if scale else 1.0
        rho = u * u
        o = 0
        for a in range(6):
            for b in range(a, 6):
                sums[o] += rho * sum(Jk[a] * Jk[b] for Jk in J)
                o += 1
        for a in range(6):
            sums[21 + a] += rho * sum(Jk[a] * rk for Jk, rk in zip(J, r))
        sums[27] += rho * e
        pairs += 1
    return np.array(sums + [float(pairs)])


@pytest.mark.parametrize("metric", ["point", "plane"])
@pytest.mark.parametrize("scale", [0.0, 0.05, 0.2, 1.0])
def test_weight_follows_the_formula(metric, scale):
    ref, scan = _hand_map()
    pose = np.concatenate([[0.02, -0.03, 0.01], turned(IDENT[3:], np.array([0.004, -0.003, 0.01]))])
    got = ref.normal_equations(scan, pose, metric, robust_scale=scale)
    want = _scalar_sums(ref, scan, pose, metric, scale)
    assert got[28] == want[28] == 60
    # 1e-12 of the sum's own scale: sum |addend| for a sum whose addends change sign
    mag = np.abs(ref._weighted_terms(scan, pose, metric, robust_scale=scale)).sum(axis=0)
    assert (np.abs(got[:28] - want[:28]) <= 1e-12 * mag).all()
    if scale:
        plain = ref.normal_equations(scan, pose, metric)
        assert got[27] < plain[27] and got[0] < plain[0]          # rho < 1 wherever e > 0
        terms, wterms = ref._pair_terms(scan, pose, metric), ref._weighted_terms(scan, pose, metric, robust_scale=scale)
        e = terms[:, 27]
        rho = (scale * scale / (scale * scale + e)) ** 2
        assert wterms.tobytes() == (terms * rho[:, None]).tobytes()


def test_outliers_lose_their_pull():
    """The scan is the hand-made scan put flat on the plane; 10 % of its points are then lifted by 0.3 m (inside
    max_dist = 1).  From a start 0.05 m below the truth one unweighted step is dragged up by the outliers' mean; the
    weighted step lands nearer the true pose.  (A level plane leaves x, y and yaw unobserved: a damping of 1e-6 keeps M
    definite and the step in the observed directions.)"""
    ref, scan = _hand_map()
    scan = scan.copy()
    scan[:, 2] = 0.5
    scan[:, 4:7] = [0.0, 0.0, 1.0]
    scan[::10, 2] += np.float32(0.3)
    start = np.array([0.0, 0.0, -0.05, 1.0, 0.0, 0.0, 0.0])
    plain, _ = ref.register(scan, start, iters=1, metric="plane", damping=1e-6)
    robust, info = ref.register(scan, start, iters=1, metric="plane", damping=1e-6, robust_scale=0.1)
    e_plain, e_robust = _err(plain, IDENT), _err(robust, IDENT)
    print("one step from 0.05 m: unweighted %.4f m, weighted %.4f m" % (e_plain, e_robust))
    assert info[0, 0] == 0.0 and info[0, 1] == 60
    assert e_robust < e_plain and e_robust < 0.5 * e_plain
    # the same after the iterations have settled
    plain, _ = ref.register(scan, start, iters=8, metric="plane", damping=1e-6)
    robust, _ = ref.register(scan, start, iters=8, metric="plane", damping=1e-6, robust_scale=0.1)
    print("eight steps: unweighted %.4f m, weighted %.4f m" % (_err(plain, IDENT), _err(robust, IDENT)))
    assert _err(robust, IDENT) < 0.5 * _err(plain, IDENT)


# ---------------------------------------------------------------------------------------------------------------------
# the basin
# ---------------------------------------------------------------------------------------------------------------------
def test_basin_pyramid_without_weights():
    scans, poses, pyr = _drive()
    assert len(scans[2]) == 7374
    start = disturbed(poses[2], 1.00, 2.0)
    assert abs(_err(start, poses[2]) - 1.0) < 1e-12
    pose, info = pyr.register(scans[2], start, [(0, 4, None, 0), (1, 4, None, 0), (2, 4, None, 0)], metric="plane")
    fine, _ = pyr.levels[2].register(scans[2], start, iters=12, metric="plane")
    print("start 1.00 m, 2.0 deg: pyramid %.4f m, fine map alone %.4f m" % (_err(pose, poses[2]), _err(fine, poses[2])))
    assert info.shape == (12, 8) and (info[:, 0] == 0).all()
    assert info[:, 5].tolist() == [0.0] * 4 + [1.0] * 4 + [2.0] * 4 and info[:, 6].tolist() == info[:, 5].tolist()
    assert _err(pose, poses[2]) <= 0.05
    assert _err(fine, poses[2]) > 0.5


def test_basin_robust_schedule():
    scans, poses, pyr = _drive()
    start = disturbed(poses[2], 0.60, 1.0)
    sched = [(k, 4, None, 0.5 * v) for k, v in enumerate(PYRAMID)]
    pose, info = pyr.register(scans[2], start, sched, metric="plane")
    fine, _ = pyr.levels[2].register(scans[2], start, iters=12, metric="plane")
    print("start 0.60 m, 1.0 deg: robust pyramid %.4f m, fine map alone %.4f m" % (_err(pose, poses[2]), _err(fine, poses[2])))
    assert (info[:, 0] == 0).all()
    assert _err(pose, poses[2]) <= 0.02
    assert _err(fine, poses[2]) > 0.05


# ---------------------------------------------------------------------------------------------------------------------
# the pyramid
# ---------------------------------------------------------------------------------------------------------------------
def test_pyramid_agrees_with_its_levels():
    from rslo_amd.mapping import MapPyramidRef, VoxelMapRef
    scans, poses, _ = _drive()
    pyr = MapPyramidRef(PYRAMID, **GATE)
    alone = [VoxelMapRef(v, **GATE) for v in PYRAMID]
    for s, p in zip(scans[:2], poses[:2]):
        pyr.insert(s, p)
        for m in alone:
            m.insert(s, p)

    def same(a, b):
        return (a.keys.tobytes() == b.keys.tobytes() and a.tags.tobytes() == b.tags.tobytes()
                and a.hits.tobytes() == b.hits.tobytes() and a.rows.tobytes() == b.rows.tobytes() and a.stats() == b.stats()
                and a.prune_stats() == b.prune_stats())
    assert len(pyr.levels) == 3 and [m.voxel_size for m in pyr.levels] == list(PYRAMID)
    assert all(same(a, b) for a, b in zip(pyr.levels, alone))
    assert pyr.stats() == [m.stats() for m in alone] and pyr.stats()[0]["n_cells"] < pyr.stats()[2]["n_cells"]
    # the finest level answers points / lookup / overlap
    assert pyr.points()[1].tobytes() == alone[2].points()[1].tobytes()
    assert pyr.lookup(scans[2], poses[2]).tobytes() == alone[2].lookup(scans[2], poses[2]).tobytes()
    assert pyr.overlap(scans[2], poses[2]) == alone[2].overlap(scans[2], poses[2])
    # prune reaches every level
    pyr.prune(center=poses[1][:3], radius=20.0, min_hits=2, grace=1)
    for m in alone:
        m.prune(center=poses[1][:3], radius=20.0, min_hits=2, grace=1)
    assert all(same(a, b) for a, b in zip(pyr.levels, alone))
    assert all(st["n_prunes"] == 1 and st["n_evicted"] > 0 for st in pyr.prune_stats())
    # a stage is the level's own register; the schedule chains them on one pose
    start = disturbed(poses[2], 0.3, 0.5)
    sched = [(0, 2, None, 0.0), (2, 3, 0.3, 0.2)]
    pose, info = pyr.register(scans[2], start, sched, metric="plane")
    p0, i0 = alone[0].register(scans[2], start, iters=2, metric="plane")
    p1, i1 = alone[2].register(scans[2], p0, iters=3, metric="plane", max_dist=0.3, robust_scale=0.2)
    assert pose.tobytes() == p1.tobytes()
    assert info[:, :5].tobytes() == np.concatenate([i0, i1])[:, :5].tobytes()
    assert info[:, 5].tolist() == [0, 0, 1, 1, 1] and info[:, 6].tolist() == [0, 0, 2, 2, 2] and not info[:, 7].any()
    # a met tolerance ends its own stage only
    pose, info = pyr.register(scans[2], start, [(0, 3, None, 0.0), (1, 2, None, 0.0)], metric="plane", tol_t=1e9, tol_r=1e9)
    assert info[:, 0].tolist() == [0.0, 3.0, 3.0, 0.0, 3.0]
    pyr.reset()
    assert all(set(st.values()) == {0} for st in pyr.stats())
    # the default schedule: coarse to fine, no weights on the coarsest level, scale = factor * voxel below it
    sch = pyr.default_schedule(3, robust_factor=0.5)
    assert sch == [(0, 3, None, 0.0), (1, 3, None, 0.4), (2, 3, None, 0.2)]
    assert pyr.default_schedule() == pyr.default_schedule(4, None) and len(pyr.default_schedule()) == 3


def test_argument_errors():
    from rslo_amd.mapping import MapPyramidRef, VoxelMapRef
    scans, poses, pyr = _drive()
    before = [m.keys.copy() for m in pyr.levels]
    nan = float("nan")
    for sched in ([(3, 4, None, 0.0)], [(-1, 4, None, 0.0)],                    # a bad level
                  [(0, 4, None, 0.0), (1, 0, None, 0.0)],                        # zero iterations in a stage
                  [(2, 4, 0.41, 0.0)], [(0, 4, 0.0, 0.0)], [(0, 4, nan, 0.0)],   # max_dist > voxel, 0, NaN
                  [(0, 4, None, -0.1)], [(0, 4, None, nan)], [(0, 4, None, float("inf"))], [(0, 4, None, 1e-200)],
                  [(0, 33, None, 0.0), (1, 32, None, 0.0)], []):                 # 65 iterations, none
        with pytest.raises(ValueError):
            pyr.register(scans[2], poses[2], sched)
    with pytest.raises(TypeError):
        pyr.register(scans[2], poses[2], iters=3, schedule=[(0, 1, None, 0.0)])      # iters together with a schedule
    # the refine= options of an OdometryRunner are checked by the same rules, before a runner is built
    from rslo_amd.mapping import check_refine
    with pytest.raises(ValueError):
        check_refine(dict(iters=3, schedule=[(0, 1, None, 0.0)]), pyr)               # iters together with a schedule
    with pytest.raises(ValueError):
        check_refine(dict(schedule=[(0, 1, None, 0.0)]), pyr.levels[2])              # a schedule without a pyramid
    with pytest.raises(ValueError):
        check_refine(dict(iters=3), pyr)
    with pytest.raises(ValueError):
        check_refine(dict(schedule=[(0, 0, None, 0.0)]), pyr)
    with pytest.raises(ValueError):
        check_refine(dict(metric="point"), pyr.levels[2])
    assert check_refine(dict(iters=3, tol_t=0.01), pyr.levels[2]) == (dict(iters=3, tol_t=0.01), 3)
    assert check_refine({}, pyr.levels[2]) == (dict(iters=5), 5) and check_refine({}, pyr)[1] == 12
    kw, rows = check_refine(dict(schedule=[(0, 2, None, 0.0), (2, 3, 0.3, 0.1)], min_pairs=10), pyr)
    assert rows == 5 and kw == dict(schedule=[(0, 2, 1.6, 0.0), (2, 3, 0.3, 0.1)], min_pairs=10)
    ref = pyr.levels[2]
    for bad in (-0.1, nan, float("inf"), 1e-200, 1e200):
        with pytest.raises(ValueError):
            ref.normal_equations(scans[2], poses[2], "plane", robust_scale=bad)
        with pytest.raises(ValueError):
            ref.register(scans[2], poses[2], iters=1, robust_scale=bad)
    with pytest.raises(ValueError):
        MapPyramidRef((0.4, 0.8))                                                # fine to coarse
    with pytest.raises(ValueError):
        MapPyramidRef(())
    with pytest.raises(ValueError):
        MapPyramidRef(tuple(2.0 ** -k for k in range(9)))                        # nine levels
    assert all(a.tobytes() == m.keys.tobytes() for a, m in zip(before, pyr.levels))
    # a weight that underflows is no poison: rho == 0 for every e > 0
    out = ref.normal_equations(scans[2], disturbed(poses[2], 0.1, 0.15), "plane", robust_scale=1e-150)
    assert np.isfinite(out).all() and out[28] > 1000 and out[27] == 0.0
    assert math.isclose(VoxelMapRef(0.4).normal_equations(scans[2], poses[2], "plane", robust_scale=0.1)[28], 0.0)
