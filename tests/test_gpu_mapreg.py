"""Scan-to-map registration on the GPU (csrc/mapreg.hip, VoxelMap.nearest / normal_equations / register) against the float64
restatement VoxelMapRef run on the same fp32 inputs, and the refined chain of an OdometryRunner.

The bars follow from the formats, not from what the kernels return:
  * nearest: BIT equality of tags, d2 and rows.  World position, d2 and the comparison are IEEE double operations on
    exactly-converted fp32 inputs in one fixed order; the candidates are found by integer keys.
  * normal equations: the pair count is exact; the device sums the same addends in another order than numpy, so each of
    the 28 sums is held to |dev - ref| <= K * 2^-50 * sum|addend| over the K addends of VoxelMapRef._pair_terms: four
    times the classical any-order bound (K - 1) * 2^-53 * sum|x|, the margin absorbing a last-bit difference in an addend.
  * one Gauss-Newton step from the same pose: 1e4 * cond2(H) * 2^-52 * (1 + |t|), Cholesky's backward error and the
    summation order at cond ~ 1e2: about 1e-9 m against corrections of about 1e-2 m.
"""
import numpy as np
import pytest
import torch
from stream_support import cond_of, dev, odom_fixture, same_bits, seed_poses, stream, turned

pytestmark = pytest.mark.gpu

IDENT = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
POSE_YAW = np.array([1.0, -0.5, 0.1, np.cos(0.15), 0.0, 0.0, np.sin(0.15)], np.float64)
_q = np.array([0.9, 0.1, -0.3, 0.25])
POSE_FULL = np.concatenate([[-2.0, 3.0, 0.4], _q / np.linalg.norm(_q)])
_CLOUD = {}
_REF = {}


def _cloud(seed):
    from rslo_amd import synthetic
    if seed not in _CLOUD:
        _CLOUD[seed] = synthetic.small_cloud(4000, seed=seed)
    return _CLOUD[seed]


def _ref(voxel, **kw):
    """VoxelMapRef holding small_cloud(seed 0) under the identity, made once and never modified"""
    from rslo_amd.mapping import VoxelMapRef
    key = (voxel, tuple(sorted(kw.items())))
    if key not in _REF:
        _REF[key] = VoxelMapRef(voxel, **kw)
        _REF[key].insert(_cloud(0), IDENT)
    return _REF[key]


def _map_of(voxel, capacity=1 << 14, **kw):
    from rslo_amd.mapping import VoxelMap
    vmap = VoxelMap(voxel, capacity, **kw)
    vmap.insert(dev(_cloud(0)), IDENT)
    return vmap


def _same_nearest(vmap, ref, q, pose, label="", dev_q=None, **kw):
    tags, d2, rows = vmap.nearest(dev(q) if dev_q is None else dev_q, dev(pose), return_rows=True, **kw)
    wt, wd, wr = ref.nearest(q, pose, return_rows=True, **kw)
    tags, d2, rows = tags.cpu().numpy(), d2.cpu().numpy(), rows.cpu().numpy()
    print("%s: %d queries, %d matched (reference %d)" % (label, len(q), int((tags >= 0).sum()), int((wt >= 0).sum())))
    assert tags.dtype == np.int64 and d2.dtype == np.float64 and rows.dtype == np.float32
    assert (tags == wt).all()
    assert (d2.view(np.int64) == wd.view(np.int64)).all()
    assert (rows.view(np.int32) == wr.view(np.int32)).all()
    return wt


# ---------------------------------------------------------------------------------------------------------------------
# nearest
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("voxel", [0.1, 0.4, 2.0])
def test_nearest_small_cloud(voxel):
    ref = _ref(voxel)
    vmap = _map_of(voxel)
    before = vmap._buf.clone()
    q = _cloud(5)
    _same_nearest(vmap, ref, q, POSE_FULL, "voxel %.1f, full rotation" % voxel)      # (tilts the cloud out of the surface: few matches)
    wt = _same_nearest(vmap, ref, q, POSE_YAW, "voxel %.1f" % voxel)
    if voxel >= 0.4:
        assert (wt >= 0).sum() > 1000
    if voxel == 0.4:
        assert (wt < 0).sum() > 1000
    _same_nearest(vmap, ref, q, POSE_YAW, "voxel %.1f, max_dist 0.9 voxel" % voxel, max_dist=0.9 * voxel)
    w2 = _same_nearest(vmap, ref, q, POSE_YAW, "voxel %.1f, min_hits 2" % voxel, min_hits=2)
    if voxel == 2.0:
        assert (w2 >= 0).sum() > 100 and (w2 != ref.nearest(q, POSE_YAW)[0]).sum() > 0      # the filter changes matches
    _same_nearest(vmap, ref, _cloud(0), IDENT, "voxel %.1f, the map's own points" % voxel)
    assert torch.equal(before, vmap._buf)            # read-only: every bit of the table and its header


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 1025])
def test_nearest_sizes(N):
    sentinel = torch.full((N + 3,), -7, dtype=torch.int64, device="cuda")
    from rslo_amd import capi
    vmap = _map_of(2.0)
    q = _cloud(5)[:N]
    _same_nearest(vmap, _ref(2.0), q, POSE_FULL, "N %d, full rotation" % N)
    wt = _same_nearest(vmap, _ref(2.0), q, POSE_YAW, "N %d" % N)
    assert (wt >= 0).sum() >= (1 if N < 63 else N // 2)
    capi.map_nearest(vmap._buf, dev(q), dev(POSE_YAW), 2.0, tags=sentinel[:N])       # nothing behind row N - 1
    assert (sentinel[N:] == -7).all() and (sentinel[:N].cpu().numpy() == wt).all()


def test_nearest_negative_and_far_coordinates():
    """Cells at both ends of the key space: a stored cell with index 2^20 - 1 (its +1 neighbour does not exist) and one
    with index -(2^20 - 1)."""
    from rslo_amd.mapping import VoxelMap, VoxelMapRef
    c = _cloud(0).copy()
    c[:, :3] += np.array([-1234.5, 987.6, -3.2], np.float32)
    c[10, 0] = np.float32(104857.55)
    c[11, 0] = np.float32(-104857.45)
    c[12, 1] = np.float32(104857.55)
    ref = VoxelMapRef(0.1)
    ref.insert(c, IDENT)
    cx, cy = (ref.keys >> 42) & 0x1fffff, (ref.keys >> 21) & 0x1fffff
    assert cx.max() == (1 << 21) - 1 and cx.min() == 1 and cy.max() == (1 << 21) - 1 and ref.stats()["dropped_range"] == 0
    vmap = VoxelMap(0.1, 1 << 14)
    vmap.insert(dev(c), IDENT)
    q = c.copy()
    q[:, :3] += np.float32(0.03)
    q[13, 0] = np.float32(2.0e5)                   # out of range itself
    wt = _same_nearest(vmap, ref, q, IDENT, "far cells")
    assert wt[10] >= 0 and wt[11] >= 0 and wt[12] >= 0 and wt[13] == -1 and (wt >= 0).sum() > 3000


def test_nearest_invalid_and_gated_queries():
    ref = _ref(0.4, min_range=5.0, max_range=15.0)
    vmap = _map_of(0.4, min_range=5.0, max_range=15.0)
    q = _cloud(5).copy()
    q[100, 1] = np.nan
    q[200, 2] = np.inf
    q[300, 0] = -np.inf
    wt = _same_nearest(vmap, ref, q, IDENT, "gate 5 .. 15 m")
    rng = np.linalg.norm(q[:, :3].astype(np.float64), axis=1)
    gated = ~((rng >= 5.0) & (rng < 15.0))
    assert gated.sum() > 100 and (wt[gated] == -1).all() and (wt >= 0).sum() > 100
    assert wt[100] == -1 and wt[200] == -1 and wt[300] == -1


def test_nearest_strided_views():
    ref = _ref(0.4)
    vmap = _map_of(0.4)
    q7 = dev(_cloud(5))
    for view in (q7, q7[:, :4], q7[:, :3], q7[:, :3].contiguous()):
        _same_nearest(vmap, ref, _cloud(5), POSE_YAW, "stride %d" % view.stride(0), dev_q=view)


def test_nearest_long_probe_chains():
    ref = _ref(0.4)
    assert len(ref.keys) / 4096.0 > 0.7
    vmap = _map_of(0.4, 4096)
    assert vmap.stats()["dropped_full"] == 0
    _same_nearest(vmap, ref, _cloud(5), POSE_YAW, "load 0.72")
    _same_nearest(vmap, ref, _cloud(0), IDENT, "load 0.72, own points")


def test_nearest_overflowed_table():
    """1024 slots for 2947 cells: which cells are stored is open, but the table then IS a map of exactly those cells, and
    nearest is exact on it: every returned tag is a stored cell, and tags / d2 / rows equal the restatement restricted to
    the stored cells."""
    from rslo_amd.mapping import VoxelMapRef
    ref = _ref(0.4)
    vmap = _map_of(0.4, 1024)
    assert vmap.stats()["dropped_full"] > 0
    stored = vmap.points()[1].cpu().numpy()
    keep = np.isin(ref.tags, stored)
    assert keep.sum() == len(stored) > 500
    sub = VoxelMapRef(0.4)
    sub.keys, sub.tags, sub.hits, sub.rows = ref.keys[keep], ref.tags[keep], ref.hits[keep], ref.rows[keep]
    for q, pose in ((_cloud(5), POSE_YAW), (_cloud(0), IDENT)):
        wt = _same_nearest(vmap, sub, q, pose, "overflowed table")
        assert np.isin(wt[wt >= 0], stored).all() and (wt >= 0).sum() > 100
        # d2 is exact for the returned cell: recomputed here from the exported row
        tags, d2 = (t.cpu().numpy() for t in vmap.nearest(dev(q), dev(pose)))
        rows = vmap.points()[0].cpu().numpy()[np.searchsorted(stored, tags[tags >= 0])]
        d = ref._cells(q, pose)[2][tags >= 0] - rows[:, :3].astype(np.float64)
        assert ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).tobytes() == d2[tags >= 0].tobytes())


# ---------------------------------------------------------------------------------------------------------------------
# the drive: scans 0 and 1 in the map under the true poses, scan 2 to be registered
# ---------------------------------------------------------------------------------------------------------------------
DRIVE_MAP = dict(voxel_size=0.4, min_range=2.5, max_range=80.0)


@pytest.fixture(scope="module")
def drive():
    from rslo_amd import synthetic
    from rslo_amd.mapping import VoxelMap, VoxelMapRef
    scans = [synthetic.sequence_scan(i, seed=3, n_el=16, n_az=520) for i in range(3)]
    poses = [synthetic.sequence_pose(i, seed=3) for i in range(3)]
    ref = VoxelMapRef(**DRIVE_MAP)
    vmap = VoxelMap(capacity=1 << 16, **DRIVE_MAP)
    for s, p in zip(scans[:2], poses[:2]):
        ref.insert(s, p)
        vmap.insert(dev(s), p)
    axis = np.array([0.3, -0.4, 0.866])
    start = np.concatenate([poses[2][:3] + 0.1 * np.array([0.6, -0.5, 0.2]),
                            turned(poses[2][3:], np.deg2rad(0.15) * axis / np.linalg.norm(axis))])
    tiled = np.concatenate([scans[2] + np.array([0.01 * k, -0.01 * k, 0, 0, 0, 0, 0], np.float32) for k in range(9)])
    assert vmap.stats()["dropped_full"] == 0 and vmap.stats() == ref.stats()
    return dict(scans=scans, poses=poses, ref=ref, vmap=vmap, start=start, tiled=tiled, dev2=dev(scans[2]))


@pytest.mark.parametrize("metric", ["point", "plane"])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 1025, 7374, 66366])
def test_normal_equations(drive, N, metric):
    ref, vmap = drive["ref"], drive["vmap"]
    src = drive["tiled"] if N > len(drive["scans"][2]) else drive["scans"][2]
    assert N <= len(src) and (N < 60000 or N > 256 * 256)      # the largest: more block partials than one 256-wide pass
    pts = src[:N]
    terms = ref._pair_terms(pts, drive["start"], metric)
    K = len(terms)
    want = ref.normal_equations(pts, drive["start"], metric)
    dpts, dpose = dev(pts), dev(drive["start"])
    got = vmap.normal_equations(dpts, dpose, metric).cpu().numpy()
    again = vmap.normal_equations(dpts, dpose, metric).cpu().numpy()
    bound = K * 2.0 ** -50 * np.abs(terms).sum(axis=0)
    err = np.abs(got[:28] - want[:28])
    with np.errstate(all="ignore"):
        print("N %d %s: %d pairs; worst |dev - ref| / bound %.3g" % (N, metric, K, np.nanmax(np.where(bound > 0, err / bound, 0.0))))
    assert got.shape == (29,) and got[28] == K == want[28]
    if N >= 1025:
        assert K > N // 2
    assert (err <= bound).all()
    assert got.tobytes() == again.tobytes()


@pytest.mark.parametrize("metric", ["plane", "point"])
def test_one_step_teacher_forced(drive, metric):
    """Six successive iterations; both implementations start every one of them from the DEVICE's current pose."""
    ref, vmap, pts = drive["ref"], drive["vmap"], drive["scans"][2]
    pose = dev(drive["start"])
    worst = 0.0
    for it in range(6):
        cur = pose.cpu().numpy().copy()
        want, winfo = ref.register(pts, cur, iters=1, metric=metric)
        out, info = vmap.register(drive["dev2"], pose, iters=1, metric=metric)
        assert out is pose                           # in place
        got, info = pose.cpu().numpy(), info.cpu().numpy()
        assert info.shape == (1, 8) and info[0, 0] == winfo[0, 0] == 0.0 and info[0, 1] == winfo[0, 1]
        bound = 1e4 * cond_of(ref.normal_equations(pts, cur, metric)) * 2.0 ** -52 * (1.0 + np.linalg.norm(cur[:3]))
        err = np.abs(got - want).max()
        worst = max(worst, err / bound)
        print("%s iteration %d: step %.3e m, |dev - ref| %.3e, bound %.3e, pairs %d" % (
            metric, it, np.linalg.norm(got[:3] - cur[:3]), err, bound, info[0, 1]))
        assert err <= bound
        assert abs(info[0, 3] - winfo[0, 3]) <= bound and abs(info[0, 4] - winfo[0, 4]) <= bound
    print("%s: largest |dev - ref| / bound over six steps %.3g" % (metric, worst))


@pytest.mark.parametrize("metric,ratio", [("plane", 0.25), ("point", 0.5)])
def test_whole_call(drive, metric, ratio):
    vmap, pts, true = drive["vmap"], drive["dev2"], drive["poses"][2]
    pose6 = dev(drive["start"])
    _, info6 = vmap.register(pts, pose6, iters=6, metric=metric)
    pose1 = dev(drive["start"])
    rows = [vmap.register(pts, pose1, iters=1, metric=metric)[1] for _ in range(6)]
    after_one = None
    assert torch.equal(pose6.view(torch.int64), pose1.view(torch.int64))
    assert torch.equal(info6.view(torch.int64), torch.cat(rows).view(torch.int64))
    e0 = np.linalg.norm(drive["start"][:3] - true[:3])
    e1 = np.linalg.norm(pose6.cpu().numpy()[:3] - true[:3])
    print("%s: translation error %.4f -> %.4f m (ratio %.3f)" % (metric, e0, e1, e1 / e0))
    assert (info6[:, 0] == 0).all() and e1 <= ratio * e0
    # tolerances that the first step meets: the later iterations are skipped
    after_one = dev(drive["start"])
    vmap.register(pts, after_one, iters=1, metric=metric)
    pose = dev(drive["start"])
    _, info = vmap.register(pts, pose, iters=4, metric=metric, tol_t=10.0, tol_r=10.0)
    assert info[:, 0].tolist() == [0.0, 3.0, 3.0, 3.0] and not info[1:, 1:].any()
    assert torch.equal(pose.view(torch.int64), after_one.view(torch.int64))
    # ... and a tolerance that is never met skips nothing, whatever the flag held before
    pose = dev(drive["start"])
    _, info = vmap.register(pts, pose, iters=6, metric=metric, tol_t=1e-30, tol_r=1e-30)
    assert torch.equal(pose.view(torch.int64), pose6.view(torch.int64)) and (info[:, 0] == 0).all()


def test_register_leaves_the_pose_alone(drive):
    from rslo_amd.mapping import VoxelMap
    start = dev(drive["start"])
    bits = start.view(torch.int64).clone()
    empty = VoxelMap(capacity=1024, **DRIVE_MAP)
    pose, info = empty.register(drive["dev2"], start, iters=2)
    assert info[:, 0].tolist() == [1.0, 1.0] and info[:, 1].tolist() == [0.0, 0.0] and torch.equal(pose.view(torch.int64), bits)
    pose, info = drive["vmap"].register(drive["dev2"][:0], start, iters=2)              # N = 0
    assert info[:, 0].tolist() == [1.0, 1.0] and torch.equal(pose.view(torch.int64), bits)
    pose, info = drive["vmap"].register(drive["dev2"], start, iters=2, min_pairs=10 ** 6)
    assert info[:, 0].tolist() == [1.0, 1.0] and info[0, 1] > 1000 and torch.equal(pose.view(torch.int64), bits)
    pose, info = drive["vmap"].register(drive["dev2"], start, iters=2, damping=-1e30)
    assert info[:, 0].tolist() == [2.0, 2.0] and torch.equal(pose.view(torch.int64), bits)
    # a host pose is copied, not written
    host = drive["start"].copy()
    pose, _ = drive["vmap"].register(drive["dev2"], host, iters=1)
    assert pose.is_cuda and host.tobytes() == drive["start"].tobytes() and not torch.equal(pose.view(torch.int64), bits)


def test_argument_errors_write_nothing(drive):
    from rslo_amd import capi
    lib = capi.lib()
    vmap, pts = drive["vmap"], drive["dev2"]
    N = 500
    p, nbytes = vmap._buf.data_ptr(), vmap._buf.numel() * 8
    before = vmap._buf.clone()
    pose = dev(drive["start"])
    S = -7.0
    tags = torch.full((N,), -7, dtype=torch.int64, device="cuda")
    d2 = torch.full((N,), S, dtype=torch.float64, device="cuda")
    rows = torch.full((N, 4), S, device="cuda")
    out = torch.full((29,), S, dtype=torch.float64, device="cuda")
    info = torch.full((33, 8), S, dtype=torch.float64, device="cuda")
    ws = torch.full((lib.rslo_map_register_ws_bytes(N) // 8,), -7, dtype=torch.int64, device="cuda")
    wsb = ws.numel() * 8
    raw4 = pts[:, :4].contiguous()
    nan = float("nan")

    def nearest(md):
        return lib.rslo_map_nearest(p, nbytes, 0.4, pts.data_ptr(), 7, N, pose.data_ptr(), md, 1, tags.data_ptr(),
                                    d2.data_ptr(), rows.data_ptr(), None)

    def normal_eq(md, metric=1, src=pts, stride=7, width=7, wsb=wsb, voxel=0.4):
        return lib.rslo_map_normal_eq(p, nbytes, voxel, src.data_ptr(), stride, width, N, pose.data_ptr(), metric, md, 1,
                                      out.data_ptr(), ws.data_ptr(), wsb, None)

    def register(md, iters=3, metric=1, src=pts, stride=7, width=7, wsb=wsb, tol=0.0):
        return lib.rslo_map_register(p, nbytes, 0.4, src.data_ptr(), stride, width, N, pose.data_ptr(), iters, metric, md, 1,
                                     0.0, 50, tol, tol, info.data_ptr(), ws.data_ptr(), wsb, None)
    rcs = [f(md) for f in (nearest, normal_eq, register) for md in (0.41, 0.0, -0.1, nan)]      # max_dist > voxel, 0, < 0, NaN
    rcs += [register(0.4, iters=0), register(0.4, iters=33), register(0.4, tol=nan), register(0.4, tol=-1.0)]
    rcs += [normal_eq(0.4, src=raw4, stride=4, width=4), register(0.4, src=raw4, stride=4, width=4)]      # plane on [P, 4]
    rcs += [normal_eq(0.4, metric=2), register(0.4, metric=-1)]
    rcs += [normal_eq(0.4, wsb=wsb - 256), register(0.4, wsb=16)]                                # a short workspace
    rcs += [normal_eq(0.4, voxel=nan), normal_eq(0.4, voxel=0.0)]
    print("return codes:", rcs, lib.rslo_last_error().decode())
    assert all(rc != 0 for rc in rcs)
    torch.cuda.synchronize()
    assert (tags == -7).all() and (d2 == S).all() and (rows == S).all() and (out == S).all() and (info == S).all()
    assert (ws == -7).all() and torch.equal(pose.cpu(), torch.from_numpy(drive["start"])) and torch.equal(before, vmap._buf)
    # a voxel_size that is not the map's passes the host check; the kernels then see no map: nothing matches
    assert lib.rslo_map_nearest(p, nbytes, 0.5, pts.data_ptr(), 7, N, pose.data_ptr(), 0.45, 1, tags.data_ptr(),
                                d2.data_ptr(), rows.data_ptr(), None) == 0
    assert (tags == -1).all() and (d2 == -1.0).all() and not rows.any()
    assert capi.map_params(vmap._buf) == (0.4, 2.5, 80.0)
    for kw in (dict(max_dist=0.5), dict(max_dist=0.0), dict(iters=0), dict(iters=33), dict(metric="surface")):
        with pytest.raises(ValueError):
            vmap.register(pts, pose, **kw)
    with pytest.raises(ValueError):
        vmap.register(raw4, pose, metric="plane")
    with pytest.raises(capi.RsloHipError):
        vmap.nearest(pts.cpu(), pose)


def test_capture_and_replay(drive):
    """One graph holding register over a static cloud, pose and info buffer; replayed for two scans it equals the eager
    calls: the iteration state lives on the device and nothing reads the host."""
    vmap = drive["vmap"]
    n = min(len(drive["scans"][1]), len(drive["scans"][2]))
    clouds = [dev(drive["scans"][2][:n]), dev(drive["scans"][1][:n])]
    starts = [dev(drive["start"]), dev(np.concatenate([drive["poses"][1][:3] + [0.05, 0.03, -0.02], drive["poses"][1][3:]]))]
    eager = []
    for c, s in zip(clouds, starts):
        pose = s.clone()
        _, info = vmap.register(c, pose, iters=4, tol_t=0.01, tol_r=0.01)      # (also the kernels' first launches)
        eager.append((pose, info))
    vmap.reserve(n)
    static_pts, static_pose = torch.zeros_like(clouds[0]), torch.zeros(7, dtype=torch.float64, device="cuda")
    static_info = torch.zeros((4, 8), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        vmap.register(static_pts, static_pose, iters=4, tol_t=0.01, tol_r=0.01, info=static_info)
    assert not static_pose.any()                    # captured, not run
    for c, s, (pose, info) in zip(clouds, starts, eager):
        static_pts.copy_(c)
        static_pose.copy_(s)
        g.replay()
        assert torch.equal(static_pose.view(torch.int64), pose.view(torch.int64))
        assert torch.equal(static_info.view(torch.int64), info.view(torch.int64))
        assert static_info[:, 0].tolist() == [0.0, 0.0, 0.0, 3.0] and static_info[0, 1] > 1000      # the fourth iteration is skipped


# ---------------------------------------------------------------------------------------------------------------------
# the runner's refined chain
# ---------------------------------------------------------------------------------------------------------------------
N_SCANS = 3
MAP_ARGS = dict(voxel_size=0.2, capacity=1 << 21, min_range=2.5, max_range=80.0)
REFINE = dict(iters=3)


odom = odom_fixture(21, 3, N_SCANS)


def _seed(vmap, scans, seeds):
    for i in range(1, len(scans)):
        vmap.insert(scans[i], seeds[i])


def _replay_by_hand(scans, rel, refine, seeds=None):
    """The refined chain issued call by call into a fresh map: pose_chain on scratch buffers, register, the state copy,
    insert (seeds: the map is seeded behind scan 0, as _stream_seeded does).  -> (map, trajectory [n, 7], info [n, iters, 8])"""
    from rslo_amd import capi
    from rslo_amd.mapping import VoxelMap
    vmap = VoxelMap(**MAP_ARGS)
    n = len(scans)
    state = torch.zeros(7, dtype=torch.float64, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    rel2 = torch.zeros((n, 7), dtype=torch.float32, device="cuda")
    traj = torch.zeros((n, 7), dtype=torch.float64, device="cuda")
    infos = []
    for i, s in enumerate(scans):
        capi.pose_chain(rel[i, :3], rel[i, 3:], state, count, rel2, traj)
        infos.append(vmap.register(s, traj[i], **refine)[1])
        state.copy_(traj[i])
        vmap.insert(s, traj[i])
        if i == 0 and seeds is not None:
            _seed(vmap, scans, seeds)
    return vmap, traj, torch.stack(infos)


def _stream_seeded(runner, vmap, scans, seeds):
    runner.reset()
    runner.run(runner.submit(scans[0]))
    _seed(vmap, scans, seeds)
    stream(runner, scans[1:])


def _same_map(a, b):
    return all(torch.equal(x, y) for x, y in zip(a.points(), b.points())) and a.stats() == b.stats()


def _check_refined_chain(runner, vmap, scans, hand_refine):
    """after one plain pass of `scans` through a refining runner: the chain against its replay by hand, reset(), and the
    same with a seeded map, where the registration has pairs to work on"""
    refined, info = runner.refined_trajectory(), runner.refine_info()
    assert refined.shape == (N_SCANS, 7) and refined.dtype == torch.float64 and refined.is_cuda
    assert info.shape == (N_SCANS, 3, 8) and info.is_cuda
    assert refined[0].tolist() == IDENT.tolist()
    assert info[0, :, 0].tolist() == [1.0] * 3 and info[0, :, 1].tolist() == [0.0] * 3      # scan 0 meets an empty map
    assert not torch.equal(refined[1:], runner.trajectory()[1:])
    rel = runner.relative().clone()
    hand_map, hand_traj, hand_info = _replay_by_hand(scans, rel, hand_refine)
    assert same_bits(refined, hand_traj) and same_bits(info, hand_info)
    assert _same_map(vmap, hand_map) and vmap.stats()["n_scans"] == N_SCANS and vmap.stats()["dropped_full"] == 0
    runner.reset()                                  # a new sequence: both chains and the map restart
    assert len(runner.refined_trajectory()) == 0 and len(runner.refine_info()) == 0 and set(vmap.stats().values()) == {0}
    seeds = seed_poses(rel)
    _stream_seeded(runner, vmap, scans, seeds)
    assert same_bits(runner.relative(), rel)
    refined, info = runner.refined_trajectory(), runner.refine_info()
    print("seeded map: status\n%s\npairs\n%s\n|dt|\n%s" % tuple(info[:, :, k].cpu().numpy() for k in (0, 1, 3)))
    assert refined[0].tolist() == IDENT.tolist() and info[0, :, 0].tolist() == [1.0] * 3
    assert (info[1:, :, 0] == 0).all() and (info[1:, :, 1] > 10000).all() and (info[1:, 0, 3] > 1e-3).all()
    hand_map, hand_traj, hand_info = _replay_by_hand(scans, rel, hand_refine, seeds)
    assert same_bits(refined, hand_traj) and same_bits(info, hand_info)
    assert _same_map(vmap, hand_map) and vmap.stats()["n_scans"] == 2 * N_SCANS - 1


def test_runner_refines_against_its_map(odom):
    from rslo_amd import capi, inference
    from rslo_amd.mapping import VoxelMap
    net, scans = odom
    plain = inference.OdometryRunner(net)
    try:
        rel0, traj0 = stream(plain, scans)
        keys0 = set(plain.stats)
        with pytest.raises(capi.RsloHipError):
            plain.refined_trajectory()
    finally:
        plain.close()
    with pytest.raises(capi.RsloHipError):
        inference.OdometryRunner(net, refine=REFINE)                         # no map to register against
    with pytest.raises(capi.RsloHipError):
        inference.OdometryRunner(net, voxel_map=VoxelMap(**MAP_ARGS), refine=dict(metric="point"))
    vmap = VoxelMap(**MAP_ARGS)
    runner = inference.OdometryRunner(net, voxel_map=vmap, refine=REFINE)
    try:
        rel, traj = stream(runner, scans)
        assert set(runner.stats) == keys0
        assert rel.tobytes() == rel0.tobytes() and traj.tobytes() == traj0.tobytes()      # the open-loop chain is untouched
        _check_refined_chain(runner, vmap, scans, REFINE)
    finally:
        runner.close()


def test_runner_refines_raw_scans(odom):
    """[P, 4] scans with normals="estimate": the registration reads the submitted tensor, so it uses the point metric."""
    from rslo_amd import inference
    from rslo_amd.mapping import VoxelMap
    net, scans = odom
    raw_scans = [s[:, :4].contiguous() for s in scans]
    vmap = VoxelMap(**MAP_ARGS)
    runner = inference.OdometryRunner(net, normals="estimate", voxel_map=vmap, refine=REFINE)
    try:
        stream(runner, raw_scans)
        _check_refined_chain(runner, vmap, raw_scans, dict(REFINE, metric="point"))
    finally:
        runner.close()
