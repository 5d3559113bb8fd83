"""The surfel map on the GPU (csrc/surfel.hip, rslo_amd/surfels.py SurfelMap) against the float64 restatement SurfelMapRef
run on the same fp32 inputs, and the surfel stage of an OdometryRunner.

The bars follow from the formats, not from what the kernels return:
  * table: after sorting by key, keys, moments (int64), rows (float64, viewed as int64) and all seven counters are EQUAL.
    The cell and the fixed-point position of a point are IEEE double operations on exactly-converted fp32 inputs in one
    fixed order; the moments are integer sums, which do not depend on the order of arrival; a row is a fixed sequence of
    double +, -, *, / and sqrt -- all correctly rounded on both sides -- on those integers.
  * nearest: BIT equality of keys, d2 and rows, for the same reason.
  * normal equations: the pair count is exact; each of the 28 sums is held to K * 2^-50 * sum|addend| over the K addends
    of SurfelMapRef._pair_terms, the bound derived in tests/test_gpu_mapreg.py.
  * one Gauss-Newton step from the same pose: that file's 1e4 * cond2(H) * 2^-52 * (1 + |t|).
"""
import numpy as np
import pytest
import torch
from stream_support import cond_of, dev, odom_fixture, same_bits, seed_poses, stream
from test_gpu_loops import quiet_collector
from test_gpu_mapreg import IDENT, POSE_FULL, POSE_YAW, _cloud
from test_map_frames_host import filled, make_frames, make_poses, store_ref
from test_surfels_host import DRIVE_ARGS, drive_ref, drive_scans, drive_start

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A5A5A5A5A
POSES = {"ident": IDENT, "yaw": POSE_YAW, "full": POSE_FULL}
SIZES = [0, 1, 2, 63, 64, 65, 1025]
_REF = {}


def _ref(voxel, pose="ident", **kw):
    """SurfelMapRef holding small_cloud(seed 0) under the named pose, made once and never modified"""
    from rslo_amd.surfels import SurfelMapRef
    key = (voxel, pose, tuple(sorted(kw.items())))
    if key not in _REF:
        _REF[key] = SurfelMapRef(voxel, **kw)
        _REF[key].insert(_cloud(0), POSES[pose])
    return _REF[key]


def _map_of(voxel, pose="ident", capacity=1 << 14, **kw):
    from rslo_amd.surfels import SurfelMap
    smap = SurfelMap(voxel, capacity, **kw)
    smap.insert(dev(_cloud(0)), POSES[pose])
    return smap


def got_of(smap, min_flag=0):
    return tuple(t.cpu().numpy() for t in smap.cells(min_flag))


def assert_same(smap, ref, label=""):
    keys, mom, rows = got_of(smap)
    rkeys, rmom, rrows = ref.cells(min_flag=0)
    st, rst = smap.stats(), ref.stats()
    print("%s: cells kernel %d, reference %d; flags 0/1/2 = %s; counters %s" % (
        label, len(keys), len(rkeys), [int((rrows[:, 7] == f).sum()) for f in (0.0, 1.0, 2.0)], st))
    assert st == rst
    assert keys.dtype == np.int64 and len(keys) == len(rkeys) and (keys == rkeys).all()
    assert mom.dtype == np.int64 and (mom == rmom).all()
    assert rows.dtype == np.float64 and (rows.view(np.int64) == rrows.view(np.int64)).all()
    assert st["n_planar"] == int((rrows[:, 7] == 2.0).sum())


def same_device_maps(a, b):
    return a.stats() == b.stats() and all(x.tobytes() == y.tobytes() for x, y in zip(got_of(a), got_of(b)))


# ---------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pose", ["ident", "yaw", "full"])
@pytest.mark.parametrize("voxel", [0.1, 0.4, 2.0])
def test_insert_small_cloud(voxel, pose):
    ref = _ref(voxel, pose)
    if voxel == 2.0:
        assert ref.stats()["n_planar"] > 20 and (ref.rows[:, 7] == 1.0).sum() > 0 and (ref.rows[:, 7] == 0.0).sum() > 0
    assert_same(_map_of(voxel, pose), ref, "voxel %.1f, %s" % (voxel, pose))


def test_three_scans_in_sequence():
    from rslo_amd.surfels import SurfelMap, SurfelMapRef
    scans, poses = drive_scans()
    ref = SurfelMapRef(0.4, **DRIVE_ARGS)
    smap = SurfelMap(0.4, 1 << 14, **DRIVE_ARGS)
    for i, (s, p) in enumerate(zip(scans, poses)):
        ref.insert(s, p)
        smap.insert(dev(s), p)
        assert_same(smap, ref, "after scan %d" % i)        # cells of earlier scans are re-derived from the grown moments
    assert ref.stats()["n_planar"] > 500 and ref.stats()["dropped_invalid"] > 0
    for other in (dict(min_points=3), dict(planar_ratio=0.02, line_ratio=0.3)):      # the header's parameters reach the rows
        ref2, smap2 = SurfelMapRef(0.4, **DRIVE_ARGS, **other), SurfelMap(0.4, 1 << 14, **DRIVE_ARGS, **other)
        ref2.insert(scans[0], poses[0])
        smap2.insert(dev(scans[0]), poses[0])
        assert_same(smap2, ref2, str(other))
        assert ref2.stats()["n_planar"] != drive_ref(0.4, 1).stats()["n_planar"]


@pytest.mark.parametrize("N", SIZES)
def test_insert_sizes(N):
    from rslo_amd.surfels import SurfelMap, SurfelMapRef
    ref, smap = SurfelMapRef(2.0), SurfelMap(2.0, 1024)
    for pts in (_cloud(0)[:N], _cloud(5)[:N]):             # the second scan meets the first one's cells
        ref.insert(pts, POSE_YAW)
        smap.insert(dev(pts), POSE_YAW)
    assert_same(smap, ref, "N %d" % N)
    assert smap.stats()["n_scans"] == 2 and smap.stats()["n_points"] == 2 * N


def test_one_cell_contention():
    """5000 points in ONE cell: every thread adds to the same ten addresses"""
    from rslo_amd.surfels import SurfelMap, SurfelMapRef
    rng = np.random.default_rng(3)
    pts = np.zeros((5000, 4), np.float32)
    pts[:, :3] = rng.uniform(0.0, 2.0, (5000, 3)) * np.array([1.0, 1.0, 0.01]) + np.array([4.0, -6.0, 2.5])
    ref, smap = SurfelMapRef(2.0), SurfelMap(2.0, 1024)
    ref.insert(pts, IDENT)
    smap.insert(dev(pts), IDENT)
    assert len(ref.keys) == 1 and ref.moments[0, 0] == 5000 and ref.rows[0, 7] == 2.0
    assert_same(smap, ref, "one cell")


def test_far_negative_invalid_and_gated_points():
    from rslo_amd.surfels import SurfelMap, SurfelMapRef
    c = _cloud(0).copy()
    c[:, :3] += np.array([-1234.5, 987.6, -3.2], np.float32)
    c[10, 0] = np.float32(104857.55)          # cell 2^20 - 1
    c[11, 0] = np.float32(-104857.45)         # cell -(2^20 - 1)
    c[12, 1] = np.float32(104857.55)
    c[13, 0] = np.float32(2.0e5)              # out of range
    c[14, 1] = np.nan
    c[15, 2] = np.inf
    c[16, 0] = -np.inf
    ref, smap = SurfelMapRef(0.1), SurfelMap(0.1, 1 << 14)
    ref.insert(c, IDENT)
    smap.insert(dev(c), IDENT)
    cx = (ref.keys >> 42) & 0x1fffff
    assert cx.max() == (1 << 21) - 1 and cx.min() == 1
    assert ref.stats()["dropped_range"] == 1 and ref.stats()["dropped_invalid"] == 3
    assert_same(smap, ref, "far cells")
    ref, smap = SurfelMapRef(2.0, min_range=5.0, max_range=15.0), SurfelMap(2.0, 1 << 12, min_range=5.0, max_range=15.0)
    ref.insert(_cloud(5), POSE_YAW)
    smap.insert(dev(_cloud(5)), POSE_YAW)
    assert ref.stats()["dropped_invalid"] > 100 and ref.stats()["n_points"] > 100
    assert_same(smap, ref, "gate 5 .. 15 m")
    # a pose of NaN drops every valid point (dropped_range)
    bad = np.full((7,), np.nan)
    ref.insert(_cloud(5), bad)
    smap.insert(dev(_cloud(5)), bad)
    assert_same(smap, ref, "NaN pose")


def test_strided_and_narrow_inputs():
    from rslo_amd.surfels import SurfelMap
    ref = _ref(2.0, "yaw")
    q7 = dev(_cloud(0))
    for view in (q7[:, :4], q7[:, :3], q7[:, :4].contiguous(), q7[:, :3].contiguous()):
        smap = SurfelMap(2.0, 1 << 12)
        smap.insert(view, POSE_YAW)
        assert_same(smap, ref, "width %d stride %d" % (view.shape[1], view.stride(0)))


def test_full_table():
    """1024 slots for 2947 cells: which cells are stored is open, but every STORED cell holds exactly the reference's
    moments and row of that key (a cell is stored completely or not at all), and the call returns."""
    ref = _ref(0.4)
    assert len(ref.keys) > 1024
    smap = _map_of(0.4, capacity=1024)
    st = smap.stats()
    keys, mom, rows = got_of(smap)
    print("full table:", st)
    assert st["dropped_full"] > 0 and st["n_cells"] == len(keys) <= 1024 and len(set(keys.tolist())) == len(keys)
    at = np.searchsorted(ref.keys, keys)
    assert (ref.keys[at] == keys).all()
    assert (mom == ref.moments[at]).all() and (rows.view(np.int64) == ref.rows[at].view(np.int64)).all()
    assert int(mom[:, 0].sum()) == st["n_points"] and st["n_points"] + st["dropped_full"] == ref.stats()["n_points"]
    assert st["n_planar"] == int((rows[:, 7] == 2.0).sum())


def test_order_freedom_and_determinism():
    from rslo_amd.surfels import SurfelMap
    A, B = dev(_cloud(0)), dev(_cloud(5))
    maps = []
    for order in ((A, B), (B, A), (A, B)):
        smap = SurfelMap(2.0, 1 << 12)
        for s in order:
            smap.insert(s, POSE_FULL)
        maps.append(smap)
    assert maps[0].stats()["n_planar"] > 20
    assert same_device_maps(maps[0], maps[1]) and same_device_maps(maps[0], maps[2])


def test_never_reset_allocation_and_argument_errors():
    from rslo_amd import capi
    lib = capi.lib()
    assert lib.rslo_surfel_bytes(1024) == 256 + 156 * 1024 and lib.rslo_surfel_bytes(1000) == 0
    assert lib.rslo_surfel_bytes(512) == 0 and lib.rslo_surfel_bytes(1 << 32) == 0
    assert lib.rslo_surfel_insert_ws_bytes(-1) == 0 and lib.rslo_surfel_insert_ws_bytes(100) >= 400
    assert lib.rslo_surfel_register_ws_bytes(-1) == 0 and lib.rslo_surfel_register_ws_bytes(257) >= 2 * 29 * 8
    pts, pose = dev(_cloud(0)), dev(POSE_YAW)
    raw = torch.full((capi.surfel_bytes(1024) // 8,), SENTINEL, dtype=torch.int64, device="cuda")
    ws = capi.surfel_insert_ws(len(pts), "cuda")
    capi.surfel_insert(raw, pts, pose, ws)                  # never reset: the kernels do nothing
    keys, d2 = capi.surfel_nearest(raw, pts, pose, 0.4)
    torch.cuda.synchronize()
    assert bool((raw == SENTINEL).all()) and bool((keys == -1).all()) and bool((d2 == -1.0).all())
    smap = _map_of(0.4)
    before = smap._buf.clone()
    p, nbytes = smap._buf.data_ptr(), smap._buf.numel() * 8
    N = 500
    S = -7.0
    out = torch.full((29,), S, dtype=torch.float64, device="cuda")
    info = torch.full((33, 8), S, dtype=torch.float64, device="cuda")
    keys = torch.full((N,), -7, dtype=torch.int64, device="cuda")
    d2 = torch.full((N,), S, dtype=torch.float64, device="cuda")
    rws = torch.full((lib.rslo_surfel_register_ws_bytes(N) // 8,), -7, dtype=torch.int64, device="cuda")
    nan = float("nan")

    def nearest(md, voxel=0.4):
        return lib.rslo_surfel_nearest(p, nbytes, voxel, pts.data_ptr(), 7, N, pose.data_ptr(), md, keys.data_ptr(),
                                       d2.data_ptr(), None, None)

    def normal_eq(md, scale=0.0, wsb=rws.numel() * 8, voxel=0.4):
        return lib.rslo_surfel_normal_eq(p, nbytes, voxel, pts.data_ptr(), 7, N, pose.data_ptr(), md, scale, out.data_ptr(),
                                         rws.data_ptr(), wsb, None)

    def register(md, iters=3, scale=0.0, tol=0.0, wsb=rws.numel() * 8):
        return lib.rslo_surfel_register(p, nbytes, 0.4, pts.data_ptr(), 7, N, pose.data_ptr(), iters, md, 0.0, 50, tol, tol,
                                        scale, info.data_ptr(), rws.data_ptr(), wsb, None)

    def reset(**kw):
        a = dict(cap=1 << 14, voxel=0.4, lo=0.0, hi=10.0, mp=5, pr=0.1, lr=0.05)
        a.update(kw)
        return lib.rslo_surfel_reset(p, nbytes, a["cap"], a["voxel"], a["lo"], a["hi"], a["mp"], a["pr"], a["lr"], None)
    rcs = [f(md) for f in (nearest, normal_eq, register) for md in (0.41, 0.0, -0.1, nan)]
    rcs += [register(0.4, iters=0), register(0.4, iters=33), register(0.4, tol=nan), register(0.4, tol=-1.0)]
    rcs += [normal_eq(0.4, scale=-1.0), normal_eq(0.4, scale=nan), register(0.4, scale=1e200)]
    rcs += [normal_eq(0.4, wsb=256), register(0.4, wsb=16), nearest(0.4, voxel=nan), normal_eq(0.4, voxel=0.0)]
    rcs += [reset(cap=1 << 15), reset(cap=1000), reset(voxel=0.0), reset(lo=3.0, hi=2.0), reset(mp=2), reset(pr=-0.1),
            reset(lr=nan)]
    rcs += [lib.rslo_surfel_insert(p, nbytes, pts.data_ptr(), 2, N, pose.data_ptr(), ws.data_ptr(), ws.numel(), None),
            lib.rslo_surfel_insert(p, nbytes, pts.data_ptr(), 7, N, pose.data_ptr(), ws.data_ptr(), 16, None),
            lib.rslo_surfel_insert(p, nbytes, pts.data_ptr(), 7, -1, pose.data_ptr(), ws.data_ptr(), ws.numel(), None)]
    print("return codes:", rcs, lib.rslo_last_error().decode())
    assert all(rc != 0 for rc in rcs)
    torch.cuda.synchronize()
    assert (keys == -7).all() and (d2 == S).all() and (out == S).all() and (info == S).all() and (rws == -7).all()
    assert torch.equal(before, smap._buf) and torch.equal(pose.cpu(), torch.from_numpy(POSE_YAW))
    for kw in (dict(max_dist=0.5), dict(max_dist=0.0), dict(iters=0), dict(iters=33), dict(robust_scale=-1.0)):
        with pytest.raises(ValueError):
            smap.register(pts, pose, **kw)
    with pytest.raises(capi.RsloHipError):
        smap.nearest(pts.cpu(), pose)
    from rslo_amd.surfels import SurfelMap
    with pytest.raises(capi.RsloHipError):
        SurfelMap(0.4, 1000)
    with pytest.raises(ValueError):
        SurfelMap(0.4, 1024, min_points=2)


# ---------------------------------------------------------------------------------------------------------------------
# insert_frames
# ---------------------------------------------------------------------------------------------------------------------
def dev_store(frames, K, capacity=16):
    from rslo_amd import loops
    return filled(loops.KeyframeStore(capacity=capacity, K=K), frames, dev)


@pytest.mark.parametrize("K,voxel", [(64, 0.5), (64, 4.0), (320, 4.0)])
def test_insert_frames_is_the_loop_of_inserts(K, voxel):
    from rslo_amd.surfels import SurfelMap, SurfelMapRef
    counts = (0, 1, 63, 64, K)
    frames, poses = make_frames(K, counts, seed=K), make_poses(5, seed=K)
    sref = store_ref(frames, K)
    ref = SurfelMapRef(voxel)
    ref.insert_frames(sref, poses)
    assert ref.stats()["n_scans"] == 5 and ref.stats()["n_points"] == sum(counts)
    if voxel == 4.0:
        assert (ref.moments[:, 0] >= 5).sum() >= 10                     # cells shared between frames, with rows
    store, poses_d = dev_store(frames, K), dev(poses)
    once = SurfelMap(voxel, 1 << 12)
    once.insert_frames(store, poses_d)
    assert_same(once, ref, "insert_frames K %d voxel %.1f" % (K, voxel))
    rows, _ = store.frames()
    loop = SurfelMap(voxel, 1 << 12)
    for e, c in enumerate(counts):
        loop.insert(rows[e][:c], poses_d[e])
    assert same_device_maps(once, loop)
    # a map that already holds a scan, fewer poses than entries, host poses
    first = dev(_cloud(5))
    a, b = SurfelMap(voxel, 1 << 12), SurfelMap(voxel, 1 << 12)
    a.insert(first, POSE_YAW), b.insert(first, POSE_YAW)
    a.insert_frames(store, poses[:4])
    for e in range(4):
        b.insert(rows[e][:counts[e]], poses_d[e])
    assert same_device_maps(a, b) and a.stats()["n_scans"] == 5


def test_insert_frames_more_tiles_than_workgroups():
    """The points pass launches at most 2048 workgroups, which then take further tiles in a loop: 2100 frames of K = 64
    (one tile each) reach the second round (tests/test_gpu_map_frames.py)."""
    from rslo_amd.surfels import SurfelMap, SurfelMapRef
    K, voxel, F = 64, 2.0, 2100
    frames = make_frames(K, [(0, 1, 3, K)[e % 4] for e in range(F)], seed=13)
    poses = make_poses(F, seed=13)
    ref = SurfelMapRef(voxel)
    ref.insert_frames(store_ref(frames, K, capacity=4096), poses)
    assert ref.stats()["n_scans"] == F and ref.stats()["n_points"] == 525 * 68 and ref.stats()["n_planar"] > 0
    assert sum(int(info[0]) for _, info in frames[2048:]) > 0           # the second round carries points
    smap = SurfelMap(voxel, 1 << 12)
    smap.insert_frames(dev_store(frames, K, capacity=4096), dev(poses))
    assert_same(smap, ref, "2100 frames")


def test_insert_frames_clamps():
    """Fewer poses than entries, more poses than entries, and a pose row of NaN (tests/test_gpu_map_frames.py
    test_clamps): keys, moments, rows and all seven counters are the restatement's."""
    from rslo_amd.surfels import SurfelMap, SurfelMapRef
    K, voxel, counts = 64, 4.0, (0, 1, 63, 64, 64)          # a 4 m cell: frames share cells, and some cells get a row
    frames, poses = make_frames(K, counts, seed=K), make_poses(9, seed=5)
    sref, store = store_ref(frames, K), dev_store(frames, K)
    bad = poses[:5].copy()
    bad[2] = np.nan                                         # the frame of 63 points
    for label, rows, n in (("3 poses", poses[:3], 3), ("9 poses", poses, 5), ("a NaN pose", bad, 5)):
        ref = SurfelMapRef(voxel)
        ref.insert_frames(sref, rows)
        assert ref.stats()["n_scans"] == n and ref.stats()["n_points"] + ref.stats()["dropped_range"] == sum(counts[:n])
        assert ref.stats()["dropped_range"] == (63 if rows is bad else 0)
        assert n == 3 or (ref.moments[:, 0] >= 5).sum() >= 8
        smap = SurfelMap(voxel, 1 << 12)
        smap.insert_frames(store, dev(rows))
        assert_same(smap, ref, label + ", 5 entries")


def test_insert_frames_full_table():
    """40 frames x 64 points in 2560 distinct cells and only 1024 slots (tests/test_gpu_map_frames.py test_overflow):
    dropped_full > 0 is certain by counting.  Slots only fill, so a key that is stored has received all of its points:
    every stored cell holds the reference's moments and row of that key."""
    from rslo_amd.surfels import SurfelMap, SurfelMapRef
    K, voxel, F = 64, 0.1, 40
    frames, poses = make_frames(K, (K,) * F, seed=11, spread=40.0), make_poses(F, seed=11)
    ref = SurfelMapRef(voxel)
    ref.insert_frames(store_ref(frames, K, capacity=64), poses)
    assert len(ref.keys) == F * K == 2560 and ref.stats()["n_cells"] == 2560 and ref.stats()["n_points"] == 2560
    smap = SurfelMap(voxel, 1024)
    smap.insert_frames(dev_store(frames, K, capacity=64), dev(poses))
    st = smap.stats()
    keys, mom, rows = got_of(smap)
    print("insert_frames into a full table:", st)
    assert st["dropped_full"] > 0 and st["n_points"] + st["dropped_full"] == ref.stats()["n_points"]
    assert st["n_scans"] == F
    assert st["n_cells"] == len(keys) <= 1024 and len(set(keys.tolist())) == len(keys)
    at = np.searchsorted(ref.keys, keys)
    assert (at < len(ref.keys)).all() and (ref.keys[at] == keys).all()
    assert (mom == ref.moments[at]).all() and (rows.view(np.int64) == ref.rows[at].view(np.int64)).all()


# ---------------------------------------------------------------------------------------------------------------------
# nearest
# ---------------------------------------------------------------------------------------------------------------------
def _same_nearest(smap, ref, q, pose, label="", dev_q=None, **kw):
    keys, d2, rows = smap.nearest(dev(q) if dev_q is None else dev_q, dev(pose), return_rows=True, **kw)
    wk, wd, wr = ref.nearest(q, pose, return_rows=True, **kw)
    keys, d2, rows = keys.cpu().numpy(), d2.cpu().numpy(), rows.cpu().numpy()
    print("%s: %d queries, %d matched (reference %d)" % (label, len(q), int((keys >= 0).sum()), int((wk >= 0).sum())))
    assert keys.dtype == np.int64 and d2.dtype == np.float64 and rows.dtype == np.float64
    assert (keys == wk).all()
    assert (d2.view(np.int64) == wd.view(np.int64)).all()
    assert (rows.view(np.int64) == wr.view(np.int64)).all()
    return wk


@pytest.fixture(scope="module")
def drive():
    from rslo_amd.surfels import SurfelMap
    scans, poses = drive_scans()
    ref = drive_ref(0.4, 2)
    smap = SurfelMap(0.4, 1 << 14, **DRIVE_ARGS)
    for s, p in zip(scans[:2], poses[:2]):
        smap.insert(dev(s), p)
    start = drive_start(poses[2])
    raw = np.ascontiguousarray(scans[2][:, :4])            # [P, 4]: the registration reads no normal
    hit = ref.nearest(raw, start)[0] >= 0
    n = min(int(hit.sum()), int((~hit).sum()))
    mixed = np.empty((2 * n, 4), np.float32)               # matched and unmatched points in turn, so that a few rows hold both
    mixed[0::2], mixed[1::2] = raw[hit][:n], raw[~hit][:n]
    return dict(scans=scans, poses=poses, ref=ref, smap=smap, start=start, raw=raw, dev2=dev(raw), mixed=mixed)


def test_nearest_on_the_drive(drive):
    ref, smap = drive["ref"], drive["smap"]
    assert_same(smap, ref, "the drive's map")
    before = smap._buf.clone()
    wk = _same_nearest(smap, ref, drive["raw"], drive["start"], "drive")
    assert (wk >= 0).sum() > 1000 and (wk < 0).sum() > 1000
    _same_nearest(smap, ref, drive["raw"], drive["start"], "drive, max_dist 0.25", max_dist=0.25)
    _same_nearest(smap, ref, drive["raw"], POSE_FULL, "drive, tilted")
    q7 = dev(drive["scans"][2])
    for view in (q7, q7[:, :3]):
        _same_nearest(smap, ref, drive["scans"][2], drive["start"], "stride %d" % view.stride(0), dev_q=view)
    assert torch.equal(before, smap._buf)                   # read-only: every bit of the table and its header


@pytest.mark.parametrize("N", SIZES)
def test_nearest_sizes(drive, N):
    from rslo_amd import capi
    ref, smap = drive["ref"], drive["smap"]
    q = drive["mixed"][:N]
    wk = _same_nearest(smap, ref, q, drive["start"], "N %d" % N)
    assert (wk >= 0).sum() == (N + 1) // 2
    sent_k = torch.full((N + 3,), -7, dtype=torch.int64, device="cuda")
    sent_d = torch.full((N + 3,), -7.0, dtype=torch.float64, device="cuda")
    sent_r = torch.full((N + 3, 8), -7.0, dtype=torch.float64, device="cuda")
    capi.surfel_nearest(smap._buf, dev(q), dev(drive["start"]), 0.4, keys=sent_k[:N], d2=sent_d[:N], rows=sent_r[:N])
    assert (sent_k[N:] == -7).all() and (sent_d[N:] == -7.0).all() and (sent_r[N:] == -7.0).all()      # nothing behind row N - 1
    assert (sent_k[:N].cpu().numpy() == wk).all()


def test_nearest_far_cells_and_full_table():
    from rslo_amd.surfels import SurfelMap, SurfelMapRef
    rng = np.random.default_rng(11)

    def patch(x, y):      # 40 points on a tilted plane inside one 1 m cell whose lower corner is (x, y, 0)
        p = np.zeros((40, 4), np.float32)
        p[:, :2] = rng.uniform(0.1, 0.9, (40, 2)) + (x, y)
        p[:, 2] = 0.3 + 0.2 * (p[:, 0] - x)
        return p
    c = np.concatenate([patch(1048574.0, 3.0), patch(-1048575.0, 3.0), patch(5.0, 1048574.0), patch(5.0, 3.0)])
    ref, smap = SurfelMapRef(1.0), SurfelMap(1.0, 1024)
    ref.insert(c, IDENT)
    smap.insert(dev(c), IDENT)
    assert ref.stats()["n_planar"] == 4 and ((ref.keys >> 42) & 0x1fffff).max() == (1 << 21) - 2
    q = c.copy()
    q[:, 2] += np.float32(0.05)
    wk = _same_nearest(smap, ref, q, IDENT, "far cells")
    assert (wk >= 0).sum() > 100
    # a full table IS a map of exactly the stored cells: nearest is exact on it
    full = _map_of(0.4, capacity=1024, min_points=3)
    big = _ref(0.4, min_points=3)
    sub = SurfelMapRef(0.4, min_points=3)
    keys = got_of(full)[0]
    keep = np.isin(big.keys, keys)
    assert full.stats()["dropped_full"] > 0 and keep.sum() == len(keys)
    sub.keys, sub.moments, sub.rows = big.keys[keep], big.moments[keep], big.rows[keep]
    wk = _same_nearest(full, sub, _cloud(5), POSE_YAW, "table of %d cells" % len(keys))
    assert (wk >= 0).sum() >= 10


# ---------------------------------------------------------------------------------------------------------------------
# normal equations and register
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [0.0, 0.2])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 513, 7374])
def test_normal_equations(drive, N, scale):
    ref, smap = drive["ref"], drive["smap"]
    pts = (drive["raw"] if N > 1000 else drive["mixed"])[:N]
    assert len(pts) == N
    terms = ref._weighted_terms(pts, drive["start"], robust_scale=scale)
    K = len(terms)
    want = ref.normal_equations(pts, drive["start"], robust_scale=scale)
    dpts, dpose = dev(pts), dev(drive["start"])
    got = smap.normal_equations(dpts, dpose, robust_scale=scale).cpu().numpy()
    again = smap.normal_equations(dpts, dpose, robust_scale=scale).cpu().numpy()
    bound = K * 2.0 ** -50 * np.abs(terms).sum(axis=0)
    err = np.abs(got[:28] - want[:28])
    with np.errstate(all="ignore"):
        print("N %d scale %.1f: %d pairs; worst |dev - ref| / bound %.3g" % (
            N, scale, K, np.nanmax(np.where(bound > 0, err / bound, 0.0))))
    assert got.shape == (29,) and got[28] == K == want[28]
    assert K > 3000 if N >= 7000 else K == (N + 1) // 2
    assert (err <= bound).all()
    assert got.tobytes() == again.tobytes()
    if scale and K:
        assert got[27] < ref.normal_equations(pts, drive["start"])[27]      # the weights are below one


@pytest.mark.parametrize("scale", [0.0, 0.2])
def test_one_step_teacher_forced(drive, scale):
    """Six successive iterations; both implementations start every one of them from the DEVICE's current pose."""
    ref, smap, pts = drive["ref"], drive["smap"], drive["raw"]
    pose = dev(drive["start"])
    for it in range(6):
        cur = pose.cpu().numpy().copy()
        want, winfo = ref.register(pts, cur, iters=1, robust_scale=scale, damping=1e-6)
        out, info = smap.register(drive["dev2"], pose, iters=1, robust_scale=scale, damping=1e-6)
        assert out is pose                           # in place
        got, info = pose.cpu().numpy(), info.cpu().numpy()
        assert info.shape == (1, 8) and info[0, 0] == winfo[0, 0] == 0.0 and info[0, 1] == winfo[0, 1] > 1000
        assert not info[0, 5:].any()
        bound = 1e4 * cond_of(ref.normal_equations(pts, cur, robust_scale=scale)) * 2.0 ** -52 * (1.0 + np.linalg.norm(cur[:3]))
        err = np.abs(got - want).max()
        print("scale %.1f iteration %d: step %.3e m, |dev - ref| %.3e, bound %.3e, pairs %d" % (
            scale, it, np.linalg.norm(got[:3] - cur[:3]), err, bound, info[0, 1]))
        assert err <= bound
        assert abs(info[0, 2] - winfo[0, 2]) <= 1e-9 * winfo[0, 2]
        assert abs(info[0, 3] - winfo[0, 3]) <= bound and abs(info[0, 4] - winfo[0, 4]) <= bound


def test_whole_call_and_statuses(drive):
    from rslo_amd.surfels import SurfelMap
    smap, pts, true = drive["smap"], drive["dev2"], drive["poses"][2]
    pose8 = dev(drive["start"])
    _, info8 = smap.register(pts, pose8, iters=8)
    pose1 = dev(drive["start"])
    rows = [smap.register(pts, pose1, iters=1)[1] for _ in range(8)]
    assert same_bits(pose8, pose1) and same_bits(info8, torch.cat(rows))      # and two runs give the same bits
    e0 = np.linalg.norm(drive["start"][:3] - true[:3])
    e1 = np.linalg.norm(pose8.cpu().numpy()[:3] - true[:3])
    print("surfels: translation error %.4f -> %.4f m (ratio %.3f)" % (e0, e1, e1 / e0))
    assert (info8[:, 0] == 0).all() and (info8[:, 1] > 1000).all() and e1 <= 0.25 * e0
    # status 3: tolerances that the first step meets
    after_one = dev(drive["start"])
    smap.register(pts, after_one, iters=1)
    pose = dev(drive["start"])
    _, info = smap.register(pts, pose, iters=4, tol_t=10.0, tol_r=10.0)
    assert info[:, 0].tolist() == [0.0, 3.0, 3.0, 3.0] and not info[1:, 1:].any() and same_bits(pose, after_one)
    pose = dev(drive["start"])
    _, info = smap.register(pts, pose, iters=8, tol_t=1e-30, tol_r=1e-30)      # never met: nothing skipped, whatever the flag held
    assert same_bits(pose, pose8) and (info[:, 0] == 0).all()
    # status 1: an empty map, N == 0, min_pairs out of reach; the pose is left alone
    start = dev(drive["start"])
    bits = start.view(torch.int64).clone()
    empty = SurfelMap(0.4, 1024, **DRIVE_ARGS)
    pose, info = empty.register(pts, start, iters=2)
    assert info[:, 0].tolist() == [1.0, 1.0] and info[:, 1].tolist() == [0.0, 0.0] and torch.equal(pose.view(torch.int64), bits)
    pose, info = smap.register(pts[:0], start, iters=2)
    assert info[:, 0].tolist() == [1.0, 1.0] and torch.equal(pose.view(torch.int64), bits)
    pose, info = smap.register(pts, start, iters=2, min_pairs=10 ** 6)
    assert info[:, 0].tolist() == [1.0, 1.0] and info[0, 1] > 1000 and torch.equal(pose.view(torch.int64), bits)
    # status 2: points on one plane only give a singular system
    g = (np.arange(40) + 0.5) * 0.125
    x, y = np.meshgrid(g, g, indexing="ij")
    floor = np.stack([x.ravel(), y.ravel(), np.full(x.size, 0.5)], axis=1).astype(np.float32)
    flat = SurfelMap(1.0, 1024)
    flat.insert(dev(floor), IDENT)
    assert flat.stats()["n_planar"] == 25
    ident = dev(IDENT)
    pose, info = flat.register(dev(floor), ident, iters=2)
    assert info[:, 0].tolist() == [2.0, 2.0] and info[0, 1] == 1600 and pose.cpu().numpy().tobytes() == IDENT.tobytes()
    host = drive["start"].copy()                            # a host pose is copied, not written
    pose, _ = smap.register(pts, host, iters=1)
    assert pose.is_cuda and host.tobytes() == drive["start"].tobytes() and not torch.equal(pose.view(torch.int64), bits)


def test_capture_and_replay(drive):
    """One graph holding insert + register over static buffers, on a single stream; replayed into a reset map it gives
    the eager bits: the launch count does not depend on the data and nothing reads the host."""
    from rslo_amd.surfels import SurfelMap
    scans, poses = drive["scans"], drive["poses"]
    n = min(len(s) for s in scans)
    clouds = [dev(np.ascontiguousarray(s[:n, :4])) for s in scans]

    def eager():
        smap = SurfelMap(0.4, 1 << 14, **DRIVE_ARGS)
        smap.insert(clouds[0], poses[0])
        pose = dev(drive_start(poses[1]))
        smap.insert(clouds[1], poses[1])
        _, info = smap.register(clouds[2], pose, iters=3, robust_scale=0.2, tol_t=1e-4, tol_r=1e-5)
        return smap, pose, info
    want_map, want_pose, want_info = eager()
    assert want_info[0, 0] == 0 and want_info[0, 1] > 1000
    smap = SurfelMap(0.4, 1 << 14, **DRIVE_ARGS)
    smap.reserve(n)
    static_pts, static_ins = torch.zeros_like(clouds[0]), torch.zeros_like(clouds[0])
    static_pose, ins_pose = torch.zeros(7, dtype=torch.float64, device="cuda"), torch.zeros(7, dtype=torch.float64, device="cuda")
    static_info = torch.zeros((3, 8), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with quiet_collector(), torch.cuda.graph(g):
        smap.insert(static_ins, ins_pose)
        smap.register(static_pts, static_pose, iters=3, robust_scale=0.2, tol_t=1e-4, tol_r=1e-5, info=static_info)
    assert smap.stats()["n_scans"] == 0 and not static_pose.any()      # captured, not run
    smap.insert(clouds[0], poses[0])
    static_ins.copy_(clouds[1])
    ins_pose.copy_(dev(poses[1]))
    static_pts.copy_(clouds[2])
    static_pose.copy_(dev(drive_start(poses[1])))
    g.replay()
    torch.cuda.synchronize()
    assert same_device_maps(smap, want_map) and same_bits(static_pose, want_pose) and same_bits(static_info, want_info)


# ---------------------------------------------------------------------------------------------------------------------
# the runner
# ---------------------------------------------------------------------------------------------------------------------
N_SCANS = 3
SURF_ARGS = dict(voxel_size=0.4, capacity=1 << 18, min_range=2.5, max_range=80.0)
SURF_REFINE = dict(iters=3)
odom = odom_fixture(21, 3, N_SCANS)


def test_runner_fills_the_surfel_map(odom):
    from rslo_amd import capi, inference
    from rslo_amd.surfels import SurfelMap, SurfelMapRef
    net, scans = odom
    plain = inference.OdometryRunner(net)
    try:
        rel0, traj0 = stream(plain, scans)
        keys0 = set(plain.stats)
        with pytest.raises(capi.RsloHipError):
            plain.surfel_refine_info()
    finally:
        plain.close()
    with pytest.raises(capi.RsloHipError):
        inference.OdometryRunner(net, surfel_refine=SURF_REFINE)                   # no surfel map to register against
    with pytest.raises(capi.RsloHipError):
        inference.OdometryRunner(net, surfels=SurfelMap(**SURF_ARGS), surfel_refine=dict(metric="plane"))
    with pytest.raises(capi.RsloHipError):
        inference.OdometryRunner(net, surfels=SurfelMap(**SURF_ARGS), surfel_refine=dict(max_dist=0.5))
    smap = SurfelMap(**SURF_ARGS)
    runner = inference.OdometryRunner(net, surfels=smap)
    try:
        rel, traj = stream(runner, scans)
        assert set(runner.stats) == keys0
        assert rel.tobytes() == rel0.tobytes() and traj.tobytes() == traj0.tobytes()
        with pytest.raises(capi.RsloHipError):
            runner.refined_trajectory()                     # surfels alone make no second chain
        ref = SurfelMapRef(**{k: v for k, v in SURF_ARGS.items() if k != "capacity"})
        for s, p in zip(scans, traj):
            ref.insert(s.cpu().numpy(), p)
        assert ref.stats()["n_planar"] > 1000
        assert_same(smap, ref, "runner's surfel map")
        runner.reset()
        assert set(smap.stats().values()) == {0}
    finally:
        runner.close()


def _by_hand(scans, rel, seeds):
    """The refined chain of a surfel_refine runner issued call by call into a fresh map: pose_chain on scratch buffers,
    register, the state copy, insert; the map is seeded behind scan 0.  -> (map, trajectory [n, 7], info [n, iters, 8])"""
    from rslo_amd import capi
    from rslo_amd.surfels import SURFEL_REFINE_DEFAULTS, SurfelMap
    smap = SurfelMap(**SURF_ARGS)
    n = len(scans)
    state = torch.zeros(7, dtype=torch.float64, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    rel2 = torch.zeros((n, 7), dtype=torch.float32, device="cuda")
    traj = torch.zeros((n, 7), dtype=torch.float64, device="cuda")
    infos = []
    for i, s in enumerate(scans):
        capi.pose_chain(rel[i, :3], rel[i, 3:], state, count, rel2, traj)
        infos.append(smap.register(s, traj[i], **dict(SURFEL_REFINE_DEFAULTS, **SURF_REFINE))[1])
        state.copy_(traj[i])
        smap.insert(s, traj[i])
        if i == 0:
            for j in range(1, n):
                smap.insert(scans[j], seeds[j])
    return smap, traj, torch.stack(infos)


@pytest.mark.parametrize("raw", [False, True])
def test_runner_refines_against_the_surfels(odom, raw):
    """Copies of the scans seeded where the chain will predict them (stream_support.seed_poses) give the registration of
    an untrained network's poses something to find.  raw: [P, 4] scans with normals="estimate" get the same plane metric."""
    from rslo_amd import inference
    from rslo_amd.surfels import SurfelMap
    net, scans = odom
    if raw:
        scans = [s[:, :4].contiguous() for s in scans]
    smap = SurfelMap(**SURF_ARGS)
    runner = inference.OdometryRunner(net, surfels=smap, surfel_refine=SURF_REFINE, **(dict(normals="estimate") if raw else {}))
    try:
        stream(runner, scans)
        rel = runner.relative().clone()
        info = runner.surfel_refine_info()
        assert info.shape == (N_SCANS, 3, 8) and info[0, :, 0].tolist() == [1.0] * 3      # scan 0 meets an empty table
        assert runner.refined_trajectory()[0].tolist() == IDENT.tolist()
        runner.reset()
        assert len(runner.refined_trajectory()) == 0 and set(smap.stats().values()) == {0}
        seeds = seed_poses(rel)
        runner.run(runner.submit(scans[0]))
        for j in range(1, N_SCANS):
            smap.insert(scans[j], seeds[j])
        stream(runner, scans[1:])
        assert same_bits(runner.relative(), rel)
        refined, info = runner.refined_trajectory(), runner.surfel_refine_info()
        print("seeded map: status\n%s\npairs\n%s\n|dt|\n%s" % tuple(info[:, :, k].cpu().numpy() for k in (0, 1, 3)))
        assert (info[1:, :, 0] == 0).all() and (info[1:, :, 1] > 10000).all() and (info[1:, 0, 3] > 1e-3).all()
        assert not torch.equal(refined[1:], runner.trajectory()[1:])
        hand_map, hand_traj, hand_info = _by_hand(scans, rel, seeds)
        assert same_bits(refined, hand_traj) and same_bits(info, hand_info)
        assert same_device_maps(smap, hand_map) and smap.stats()["n_scans"] == 2 * N_SCANS - 1
    finally:
        runner.close()


def test_runner_rebuilds_the_surfels_after_loop_closure(odom):
    """The scenario of tests/test_gpu_map_frames.py::test_runner_rebuilds_and_adopts with a surfel map attached: after
    adopt_loop_closure the surfel table is insert_frames of the keyframe store under the optimised rows."""
    from rslo_amd import inference, loops, places, posegraph, synthetic
    from rslo_amd.mapping import VoxelMap
    from rslo_amd.surfels import SurfelMap
    net, scans = odom
    scans = list(scans) + [dev(synthetic.scan(2083, 64, (0.5, 0.4), 0.2, scan_seed=999))]
    store, vmap, smap = loops.KeyframeStore(capacity=16, K=1024), VoxelMap(0.5, 1 << 18), SurfelMap(2.0, 1 << 14)
    runner = inference.OdometryRunner(net, capacity=16, voxel_map=vmap, refine=dict(iters=1, min_pairs=10 ** 9),
                                      surfels=smap, surfel_refine=dict(iters=1, min_pairs=10 ** 9),
                                      places=places.PlaceDB(capacity=16), loop=dict(exclude_recent=1, num_candidates=2, top_k=2),
                                      keyframes=store, verify=dict(max_edges=8),
                                      pose_graph=posegraph.PoseGraph(capacity=16, max_loops=8))
    try:
        with quiet_collector():
            stream(runner, scans)
        assert (runner.surfel_refine_info().cpu().numpy()[:, :, 0] == 1).all()
        assert smap.stats()["n_scans"] == 4 and smap.stats()["n_points"] > 100000
        poses, info = runner.close_verified_loops(gn_iters=3)
        assert int(info.cpu().numpy()[0, 1]) >= 1           # a loop edge was used
        runner.adopt_loop_closure()
        want = SurfelMap(2.0, 1 << 14)
        want.insert_frames(store, poses)
        torch.cuda.synchronize()
        assert want.stats()["n_points"] > 1000 and want.stats()["n_planar"] > 10
        assert same_device_maps(smap, want) and smap.stats()["n_scans"] == 4
        other, own = VoxelMap(0.5, 1 << 14), smap._buf.clone()
        runner.rebuild_map(voxel_map=other)                 # another map: the runner's own surfels stay, to the byte
        torch.cuda.synchronize()
        assert torch.equal(smap._buf, own)
        runner.rebuild_map()                                # the runner's own maps, again: the same table
        assert same_device_maps(smap, want)
    finally:
        runner.close()
