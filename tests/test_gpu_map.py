"""World voxel map on the GPU (csrc/map.hip, rslo_amd/mapping.py VoxelMap) against the float64 restatement VoxelMapRef run on
the same fp32 inputs, and the map an OdometryRunner fills while it streams.

The bar is BIT equality after sorting by tag -- rows (viewed as int32), tags, hits and all six counters -- with no
tolerance and no excluded cell: the cell of a point and its row are IEEE double operations on exactly-converted fp32
inputs in a fixed order, rounded once to fp32; tags, hits and counters are integers.  It follows from the formats, not
from what the kernels return.  Only a map that overflowed (dropped_full > 0) leaves the choice of the stored cells open;
each stored cell is still exact.
"""
import ctypes

import numpy as np
import pytest
import torch
from stream_support import dev, odom_fixture, stream

pytestmark = pytest.mark.gpu

IDENT = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
POSE_YAW = np.array([1.0, -0.5, 0.1, np.cos(0.15), 0.0, 0.0, np.sin(0.15)], np.float64)
_q = np.array([0.9, 0.1, -0.3, 0.25])
POSE_FULL = np.concatenate([[-2.0, 3.0, 0.4], _q / np.linalg.norm(_q)])      # all four quaternion components non-zero
_CLOUD = {}
_REF = {}


def _cloud(seed):
    from rslo_amd import synthetic
    if seed not in _CLOUD:
        _CLOUD[seed] = synthetic.small_cloud(4000, seed=seed)
    return _CLOUD[seed]


def _ref(voxel, scans, **kw):
    """VoxelMapRef filled with scans = ((cloud seed, pose), ...) of full [P, 7] clouds, made once and never modified"""
    from rslo_amd.mapping import VoxelMapRef
    key = (voxel, tuple((s, tuple(p)) for s, p in scans), tuple(sorted(kw.items())))
    if key not in _REF:
        ref = VoxelMapRef(voxel, **kw)
        for seed, pose in scans:
            ref.insert(_cloud(seed), pose)
        _REF[key] = ref
    return _REF[key]


def _got(vmap, **kw):
    rows, tags, hits = vmap.points(**kw)
    return rows.cpu().numpy(), tags.cpu().numpy(), hits.cpu().numpy()


def _assert_same(vmap, ref, label=""):
    rows, tags, hits = _got(vmap)
    rrows, rtags, rhits = ref.points()
    st, rst = vmap.stats(), ref.stats()
    print("%s: cells kernel %d, reference %d; %d cells with >= 2 points, most hits %d; counters %s" % (
        label, len(tags), len(rtags), int((rhits >= 2).sum()), int(rhits.max()) if len(rhits) else 0, st))
    assert st == rst
    assert len(tags) == len(rtags) and (tags == rtags).all()
    assert (hits == rhits).all()
    assert rows.dtype == np.float32 and (rows.view(np.int32) == rrows.view(np.int32)).all()


@pytest.mark.parametrize("voxel", [0.1, 0.4, 2.0])
def test_small_cloud(voxel):
    from rslo_amd.mapping import VoxelMap
    ref = _ref(voxel, ((0, IDENT),))
    rhits = ref.points()[2]
    if voxel == 0.1:
        assert (rhits >= 2).sum() >= 50
    if voxel == 2.0:
        assert rhits.max() > 32
    assert (ref.points()[0][:, 3] != 0).all()      # the intensities are real
    pts = dev(_cloud(0))
    first = None
    for k in range(2):                             # two fresh maps: the same bits
        vmap = VoxelMap(voxel, 1 << 14)
        vmap.insert(pts, dev(IDENT))
        _assert_same(vmap, ref, "small %.1f run %d" % (voxel, k))
        got = _got(vmap)
        if first is not None:
            assert all(a.tobytes() == b.tobytes() for a, b in zip(first, got))
        first = got


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 1025])
def test_sizes(N):
    """The first N points shrunk by 0.01 (they lie within 0.2 m of the origin), moved by t = (5, 5, 5) so that at a cell
    edge of 10 m all of them share ONE cell (the cells are anchored at the world origin, which would otherwise cut the
    cloud into octants): lane, wave and block boundaries."""
    from rslo_amd.mapping import VoxelMap, VoxelMapRef
    c = _cloud(0)[:N].copy()
    c[:, :3] *= np.float32(0.01)
    pose = np.array([5.0, 5.0, 5.0, 1, 0, 0, 0], np.float64)
    for voxel in (0.1, 10.0):
        ref = VoxelMapRef(voxel)
        ref.insert(c, pose)
        if voxel == 10.0:
            assert ref.points()[2].tolist() == [N]
        vmap = VoxelMap(voxel, 1 << 12)
        vmap.insert(dev(c), pose)
        _assert_same(vmap, ref, "N %d voxel %.1f" % (N, voxel))


@pytest.mark.parametrize("name", ["yaw", "full"])
def test_two_scans(name):
    from rslo_amd.mapping import VoxelMap
    pose = POSE_YAW if name == "yaw" else POSE_FULL
    ref = _ref(0.4, ((0, IDENT), (5, pose)))
    rrows, rtags, rhits = ref.points()
    only0 = _ref(0.4, ((0, IDENT),))
    created_by_1 = int((rtags >> 32 == 1).sum())
    into_old = int(rhits[rtags >> 32 == 0].sum() - only0.points()[2].sum())      # scan-1 points that fell into scan-0 cells
    print("two scans (%s): %d cells, %d created by scan 1, %d scan-1 points in scan-0 cells" % (
        name, len(rtags), created_by_1, into_old))
    assert created_by_1 > 0 and into_old > 0
    n0 = len(only0.points()[1])
    assert rrows[:n0].tobytes() == only0.points()[0].tobytes()      # a later scan never changes an earlier cell's row
    vmap = VoxelMap(0.4, 1 << 14)
    vmap.insert(dev(_cloud(0)), IDENT)
    vmap.insert(dev(_cloud(5)), dev(pose))
    _assert_same(vmap, ref, "two scans " + name)


def test_negative_and_far_coordinates():
    from rslo_amd.mapping import VoxelMap, VoxelMapRef
    c = _cloud(0).copy()
    c[:, :3] += np.array([-1234.5, 987.6, -3.2], np.float32)
    far = c.copy()
    far[1500, 0] = np.float32(2.0e5)               # cell 2e6 >= 2^20 at 0.1 m
    refs = []
    for cloud, dropped in ((c, 0), (far, 1)):
        ref = VoxelMapRef(0.1)
        ref.insert(cloud, IDENT)
        assert ref.stats()["dropped_range"] == dropped and ref.stats()["n_points"] == len(c) - dropped
        assert (ref.points()[0][:, 0] < 0).all() or dropped
        vmap = VoxelMap(0.1, 1 << 14)
        vmap.insert(dev(cloud), IDENT)
        _assert_same(vmap, ref, "far cloud, %d out of range" % dropped)
        assert vmap.stats()["dropped_range"] == dropped
        refs.append(ref)
    # the rest is unchanged: every cell of the second map is a cell of the first with the same row
    a = dict(zip(refs[0].points()[1].tolist(), (r.tobytes() for r in refs[0].points()[0])))
    assert all(a[t] == r.tobytes() for t, r in zip(refs[1].points()[1].tolist(), refs[1].points()[0]) if t in a)


def test_invalid_and_gated_points():
    from rslo_amd import synthetic
    from rslo_amd.mapping import VoxelMap, VoxelMapRef
    c = _cloud(0).copy()
    c[100, 1] = np.nan
    c[200, 2] = np.inf
    ref = VoxelMapRef(0.4)
    ref.insert(c, POSE_YAW)
    assert ref.stats()["dropped_invalid"] == 2
    vmap = VoxelMap(0.4, 1 << 14)
    vmap.insert(dev(c), POSE_YAW)
    _assert_same(vmap, ref, "NaN / inf")
    s = synthetic.scan(n_az=520, n_el=16)
    rng = np.linalg.norm(s[:, :3].astype(np.float64), axis=1)
    assert rng.min() < 10 and rng.max() > 40       # both ends of the gate cut
    ref = VoxelMapRef(0.4, min_range=10.0, max_range=40.0)
    ref.insert(s, POSE_YAW)
    st = ref.stats()
    assert 0 < st["dropped_invalid"] < len(s) and st["n_points"] + st["dropped_invalid"] == len(s)
    vmap = VoxelMap(0.4, 1 << 14, min_range=10.0, max_range=40.0)
    vmap.insert(dev(s), POSE_YAW)
    _assert_same(vmap, ref, "range gate 10 .. 40 m")


def test_strided_input():
    from rslo_amd.mapping import VoxelMap
    ref = _ref(0.4, ((0, POSE_YAW),))
    c7 = dev(_cloud(0))
    maps = []
    for pts in (c7, c7[:, :4].contiguous(), c7[:, :4], c7[:, :3].contiguous(), c7[:, :3]):      # views are read in place
        vmap = VoxelMap(0.4, 1 << 14)
        vmap.insert(pts, POSE_YAW)
        maps.append(_got(vmap))
    for k in (0, 1, 2):
        rows, tags, hits = maps[k]
        assert rows.tobytes() == ref.points()[0].tobytes() and (tags == ref.points()[1]).all() and (hits == ref.points()[2]).all()
    for k in (3, 4):
        rows, tags, hits = maps[k]
        assert (tags == ref.points()[1]).all() and (hits == ref.points()[2]).all()
        assert rows[:, :3].tobytes() == ref.points()[0][:, :3].tobytes() and (rows[:, 3] == 0).all()


def test_full_table_is_a_counter_not_a_hang():
    """2947 cells offered to 1024 slots: the bounded probe drops what finds no slot.  Every stored cell is complete."""
    from rslo_amd.mapping import VoxelMap
    ref = _ref(0.4, ((0, IDENT),))
    rrows, rtags, rhits = ref.points()
    assert len(rtags) > 2 * 1024
    vmap = VoxelMap(0.4, 1024)
    pts = dev(_cloud(0))
    vmap.insert(pts, IDENT)
    rows, tags, hits = _got(vmap)
    st = vmap.stats()
    print("full table: %d of %d cells stored, counters %s" % (len(tags), len(rtags), st))
    assert st["dropped_full"] > 0 and st["n_cells"] <= 1024 and st["n_cells"] == len(tags)
    pos = np.searchsorted(rtags, tags)
    assert (pos < len(rtags)).all() and (rtags[pos] == tags).all() and len(np.unique(tags)) == len(tags)
    assert (hits == rhits[pos]).all() and rows.tobytes() == rrows[pos].tobytes()
    assert st["dropped_full"] == ref.stats()["n_points"] - int(hits.sum())
    assert st["n_points"] == int(hits.sum()) and st["dropped_invalid"] == 0 and st["dropped_range"] == 0
    # lookup of the same points: a stored cell reads its hits, a dropped cell reads 0
    got = vmap.lookup(pts, IDENT).cpu().numpy()
    want = ref.lookup(_cloud(0), IDENT)
    assert ((got == want) | (got == 0)).all() and int((got == 0).sum()) == st["dropped_full"]
    assert abs(float(vmap.overlap(pts, IDENT)) - float((got > 0).sum()) / len(got)) < 1e-6


def test_long_probe_chains_without_overflow():
    from rslo_amd.mapping import VoxelMap
    ref = _ref(0.4, ((0, IDENT),))
    assert len(ref.points()[1]) / 4096.0 > 0.7
    vmap = VoxelMap(0.4, 4096)
    vmap.insert(dev(_cloud(0)), IDENT)
    _assert_same(vmap, ref, "load 0.72")


def test_lookup_and_overlap():
    from rslo_amd.mapping import VoxelMap
    ref = _ref(0.4, ((0, IDENT),))
    q = _cloud(5).copy()
    q[7, 0] = np.nan
    want, wtags = ref.lookup(q, POSE_YAW, return_tags=True)
    assert (want > 0).sum() > 100 and (want == 0).sum() > 100 and want[7] == -1      # partly new, one invalid point
    vmap = VoxelMap(0.4, 1 << 14)
    vmap.insert(dev(_cloud(0)), IDENT)
    before = _got(vmap)
    hits, tags = vmap.lookup(dev(q), dev(POSE_YAW), return_tags=True)
    assert hits.dtype == torch.int32 and (hits.cpu().numpy() == want).all() and (tags.cpu().numpy() == wtags).all()
    ov = vmap.overlap(dev(q), POSE_YAW)
    assert ov.is_cuda and abs(float(ov) - ref.overlap(q, POSE_YAW)) < 1e-6
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, _got(vmap)))       # read-only
    assert vmap.stats() == ref.stats()
    # a range-gated map: a point outside the gate reads -1
    from rslo_amd.mapping import VoxelMapRef
    gref = VoxelMapRef(0.4, min_range=5.0, max_range=15.0)
    gref.insert(_cloud(0), IDENT)
    gmap = VoxelMap(0.4, 1 << 14, min_range=5.0, max_range=15.0)
    gmap.insert(dev(_cloud(0)), IDENT)
    want = gref.lookup(_cloud(5), IDENT)
    assert (want == -1).sum() > 100 and (gmap.lookup(dev(_cloud(5)), IDENT).cpu().numpy() == want).all()


def test_export():
    from rslo_amd import capi
    from rslo_amd.mapping import VoxelMap
    ref = _ref(0.4, ((0, IDENT), (5, POSE_YAW)))
    vmap = VoxelMap(0.4, 1 << 14)
    vmap.insert(dev(_cloud(0)), IDENT)
    vmap.insert(dev(_cloud(5)), POSE_YAW)
    for min_hits in (1, 2, 3):
        want = ref.points(min_hits=min_hits)
        assert 0 < len(want[1]) and (min_hits == 1 or len(want[1]) < len(ref.points()[1]))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(_got(vmap, min_hits=min_hits), want))
    center = np.array([3.0, -2.0, 0.1])
    want = ref.points(min_hits=2, center=center, radius=4.0)
    assert 10 < len(want[1]) < len(ref.points(min_hits=2)[1])
    for c in (dev(center), center):               # a device row, or host values
        assert all(a.tobytes() == b.tobytes() for a, b in zip(_got(vmap, min_hits=2, center=c, radius=4.0), want))
    # unsorted: the same set
    rows, tags, hits = _got(vmap, sort=False)
    order = np.argsort(tags)
    assert rows[order].tobytes() == ref.points()[0].tobytes() and (hits[order] == ref.points()[2]).all()
    # fewer output rows than matches: counted, not written
    R, M = 100, len(ref.points()[1])
    rows = torch.full((R + 50, 4), -7.0, device="cuda")
    tags = torch.full((R + 50,), -7, dtype=torch.int64, device="cuda")
    hits = torch.full((R + 50,), -7, dtype=torch.int32, device="cuda")
    counts = capi.map_export(vmap._buf, 1, None, 0.0, rows[:R], tags[:R], hits[:R])
    assert counts.tolist() == [M, R]
    assert (rows[R:] == -7).all() and (tags[R:] == -7).all() and (hits[R:] == -7).all()
    t = tags[:R].cpu().numpy()
    pos = np.searchsorted(ref.points()[1], t)
    assert len(np.unique(t)) == R and (ref.points()[1][pos] == t).all()
    assert rows[:R].cpu().numpy().tobytes() == ref.points()[0][pos].tobytes()
    assert (hits[:R].cpu().numpy() == ref.points()[2][pos]).all()
    assert capi.map_export(vmap._buf, 1).tolist() == [M, 0]


def test_reset():
    from rslo_amd.mapping import VoxelMap
    vmap = VoxelMap(0.4, 1 << 14)
    vmap.insert(dev(_cloud(5)), POSE_FULL)
    vmap.insert(dev(_cloud(5)[:0]), POSE_FULL)      # an empty scan still counts
    assert vmap.stats()["n_scans"] == 2 and vmap.stats()["n_cells"] > 0
    vmap.reset()
    assert set(vmap.stats().values()) == {0} and len(vmap.points()[1]) == 0
    assert int((vmap.lookup(dev(_cloud(5)), POSE_FULL) != 0).sum()) == 0
    vmap.insert(dev(_cloud(0)), IDENT)               # the tags start at scan 0 again
    _assert_same(vmap, _ref(0.4, ((0, IDENT),)), "after reset")


def test_argument_errors_write_nothing():
    from rslo_amd import capi
    from rslo_amd.mapping import VoxelMap
    lib = capi.lib()
    nbytes = capi.map_bytes(2048)
    sentinel = 0x5A5A5A5A5A5A5A5A
    buf = torch.full((nbytes // 8,), sentinel, dtype=torch.int64, device="cuda")
    p, inf = buf.data_ptr(), float("inf")
    pts = dev(_cloud(0)[:64, :4])
    pose = dev(IDENT)
    ws = torch.empty((lib.rslo_map_insert_ws_bytes(64),), dtype=torch.uint8, device="cuda")
    rcs = [lib.rslo_map_reset(p, nbytes, 1000, 0.1, 0.0, inf, None),            # not a power of two
           lib.rslo_map_reset(p, nbytes, 1536, 0.1, 0.0, inf, None),
           lib.rslo_map_reset(p, nbytes, 512, 0.1, 0.0, inf, None),             # below 1024
           lib.rslo_map_reset(p, nbytes, 2048, 0.0, 0.0, inf, None),            # voxel_size <= 0
           lib.rslo_map_reset(p, nbytes, 2048, -0.1, 0.0, inf, None),
           lib.rslo_map_reset(p, nbytes, 2048, float("nan"), 0.0, inf, None),
           lib.rslo_map_reset(p, nbytes - 8, 2048, 0.1, 0.0, inf, None),        # a short map_bytes
           lib.rslo_map_reset(p, nbytes, 4096, 0.1, 0.0, inf, None),
           lib.rslo_map_reset(p, nbytes, 2048, 0.1, 5.0, 5.0, None),            # min_range >= max_range
           lib.rslo_map_reset(p, nbytes, 2048, 0.1, -1.0, inf, None),
           lib.rslo_map_insert(p, nbytes, pts.data_ptr(), 2, 3, 64, pose.data_ptr(), ws.data_ptr(), ws.numel(), None),   # stride < 3
           lib.rslo_map_insert(p, 1000, pts.data_ptr(), 4, 4, 64, pose.data_ptr(), ws.data_ptr(), ws.numel(), None),
           lib.rslo_map_insert(p, nbytes, pts.data_ptr(), 4, 4, 64, pose.data_ptr(), ws.data_ptr(), 16, None)]            # workspace
    print("return codes:", rcs, capi.lib().rslo_last_error().decode())
    assert all(rc != 0 for rc in rcs)
    # a buffer that was never reset holds no map: the kernels of a valid call leave it alone
    assert lib.rslo_map_insert(p, nbytes, pts.data_ptr(), 4, 4, 64, pose.data_ptr(), ws.data_ptr(), ws.numel(), None) == 0
    torch.cuda.synchronize()
    assert bool((buf == sentinel).all())
    for bad in (1000, 1536, 0):
        with pytest.raises(capi.RsloHipError):
            VoxelMap(0.1, bad)
    with pytest.raises(ValueError):
        VoxelMap(0.0, 1024)
    with pytest.raises(capi.RsloHipError):
        VoxelMap(0.1, 1024).insert(dev(_cloud(0)).cpu(), IDENT)
    assert ctypes.sizeof(ctypes.c_size_t) == 8


def test_capture_and_replay():
    """One graph holding insert from a static buffer under a static pose row; replayed with two clouds and poses copied in
    it equals two eager inserts: the scan counter lives on the device and nothing reads the host."""
    from rslo_amd.mapping import VoxelMap
    ref = _ref(0.4, ((0, IDENT), (5, POSE_YAW)))
    clouds = [dev(_cloud(0)[:, :4]), dev(_cloud(5)[:, :4])]
    poses = [dev(IDENT), dev(POSE_YAW)]
    eager = VoxelMap(0.4, 1 << 14)
    for c, p in zip(clouds, poses):
        eager.insert(c, p)                          # (also the kernels' first launches, outside the capture)
    vmap = VoxelMap(0.4, 1 << 14)
    vmap.reserve(len(clouds[0]))
    static_pts, static_pose = torch.zeros_like(clouds[0]), torch.zeros(7, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        vmap.insert(static_pts, static_pose)
    assert vmap.stats()["n_scans"] == 0             # captured, not run
    for c, p in zip(clouds, poses):
        static_pts.copy_(c)
        static_pose.copy_(p)
        g.replay()
    _assert_same(vmap, ref, "graph replay")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(_got(vmap), _got(eager)))
    assert vmap.stats() == eager.stats()


# ---------------------------------------------------------------------------------------------------------------------
# the runner's map
# ---------------------------------------------------------------------------------------------------------------------
N_SCANS = 3
MAP_ARGS = dict(voxel_size=0.2, capacity=1 << 21, min_range=2.5, max_range=80.0)


odom = odom_fixture(21, 3, N_SCANS)


def _ref_of(scans, traj):
    from rslo_amd.mapping import VoxelMapRef
    ref = VoxelMapRef(MAP_ARGS["voxel_size"], MAP_ARGS["min_range"], MAP_ARGS["max_range"])
    for s, pose in zip(scans, traj):
        ref.insert(s.cpu().numpy(), pose)
    return ref


def test_runner_fills_the_map(odom):
    from rslo_amd import inference
    from rslo_amd.mapping import VoxelMap, VoxelMapRef
    net, scans = odom
    plain = inference.OdometryRunner(net)
    try:
        rel0, traj0 = stream(plain, scans)
        keys0 = set(plain.stats)
    finally:
        plain.close()
    vmap = VoxelMap(**MAP_ARGS)
    runner = inference.OdometryRunner(net, voxel_map=vmap)
    try:
        rel, traj = stream(runner, scans)
        assert set(runner.stats) == keys0
        assert rel.tobytes() == rel0.tobytes() and traj.tobytes() == traj0.tobytes()      # the map disturbs nothing
        assert traj[0].tolist() == IDENT.tolist() and np.abs(traj[1:] - IDENT).max() > 0
        ref = _ref_of(scans, traj)
        assert ref.stats()["n_scans"] == N_SCANS and ref.stats()["n_points"] > 300000
        _assert_same(vmap, ref, "runner map")
        assert vmap.stats()["dropped_full"] == 0
        again = VoxelMap(**MAP_ARGS)                # filled afterwards from the same scans and trajectory rows
        for s, pose in zip(scans, runner.trajectory()):
            again.insert(s, pose)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(_got(vmap), _got(again))) and vmap.stats() == again.stats()
        first = VoxelMapRef(MAP_ARGS["voxel_size"], MAP_ARGS["min_range"], MAP_ARGS["max_range"])
        first.insert(scans[0].cpu().numpy(), IDENT)
        assert vmap.stats()["n_cells"] >= first.stats()["n_cells"] > 10000
        runner.reset()                              # a new sequence has a new frame
        assert set(vmap.stats().values()) == {0} and len(vmap.points()[1]) == 0
        stream(runner, scans[:1])
        _assert_same(vmap, first, "runner map after reset")
    finally:
        runner.close()
    # raw [P, 4] scans with estimated normals: the map is fed from the submitted tensor, never from the arena's cloud
    raw_scans = [s[:, :4].contiguous() for s in scans]
    rmap = VoxelMap(**MAP_ARGS)
    raw = inference.OdometryRunner(net, normals="estimate", voxel_map=rmap)
    try:
        _, rtraj = stream(raw, raw_scans)
        _assert_same(rmap, _ref_of(raw_scans, rtraj), "runner map, raw scans")
        same_traj = rtraj.tobytes() == traj.tobytes()
        print("raw scans: trajectory %s the [P, 7] run's" % ("equals" if same_traj else "differs from"))
        rows, tags, hits = _got(rmap)
        wrows, wtags, whits = ref.points()
        if same_traj:
            assert rows.tobytes() == wrows.tobytes() and (tags == wtags).all() and (hits == whits).all()
        else:                                       # scan 0 is inserted under the identity whatever the head predicts
            a, b = tags >> 32 == 0, wtags >> 32 == 0
            assert a.sum() == b.sum() > 10000 and (tags[a] == wtags[b]).all() and rows[a].tobytes() == wrows[b].tobytes()
    finally:
        raw.close()
