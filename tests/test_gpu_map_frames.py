"""The map after loop closure on the GPU: rslo_map_insert_frames (csrc/map.hip, VoxelMap.insert_frames) against its
definition, VoxelMapRef.insert_frames -- successive inserts of a keyframe store's frames, each under its own pose -- and
against the existing per-scan kernel, and OdometryRunner.rebuild_map / adopt_loop_closure.

The bar is the one of tests/test_gpu_map.py: after sorting by tag, rows (viewed as int32), tags, hits and all six counters
are EQUAL, with no tolerance.  It follows from the rules, not from what the kernels return: the cell and the row of a point
are IEEE double operations on exactly-converted fp32 inputs in a fixed order, tags, hits and counters are integers, and
the content of a map does not depend on the order of insertion (the smallest tag wins, the rest are integer sums).  The
stores are made of hand-built frames, so that every count is chosen: 0, 1, 63, 64 and K rows at K = 64 (one wave, one
partly filled block per frame) and K = 320 (a second, partial block per frame)."""
import numpy as np
import pytest
import torch

from stream_support import dev, odom_fixture, same_bits, stream
from test_gpu_loops import quiet_collector
from test_map_frames_host import filled, frame_points, loop_of_inserts, make_frames, make_poses, store_ref

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A5A5A5A5A
CASES = [(64, 0.1), (64, 2.0), (320, 0.1), (320, 2.0)]
_CASE = {}


def counts_of(K):
    return (0, 1, 63, 64, K)


def case(K, voxel):
    """(frames, poses, the restatement's map): made once per case and never modified"""
    from rslo_amd.mapping import VoxelMapRef
    if (K, voxel) not in _CASE:
        frames, poses = make_frames(K, counts_of(K), seed=K), make_poses(5, seed=K)
        ref = VoxelMapRef(voxel)
        ref.insert_frames(store_ref(frames, K), poses)
        _CASE[(K, voxel)] = (frames, poses, ref)
    return _CASE[(K, voxel)]


def dev_store(frames, K, capacity=16):
    from rslo_amd import loops
    return filled(loops.KeyframeStore(capacity=capacity, K=K), frames, dev)


def got_of(vmap):
    rows, tags, hits = vmap.points()
    return rows.cpu().numpy(), tags.cpu().numpy(), hits.cpu().numpy()


def assert_same(vmap, ref, label=""):
    rows, tags, hits = got_of(vmap)
    rrows, rtags, rhits = ref.points()
    st, rst = vmap.stats(), ref.stats()
    print("%s: cells kernel %d, reference %d; %d cells with >= 2 points; counters %s" % (
        label, len(tags), len(rtags), int((rhits >= 2).sum()), st))
    assert st == rst
    assert len(tags) == len(rtags) and (tags == rtags).all()
    assert (hits == rhits).all()
    assert rows.dtype == np.float32 and (rows.view(np.int32) == rrows.view(np.int32)).all()


def same_device_maps(a, b):
    return a.stats() == b.stats() and all(x.tobytes() == y.tobytes() for x, y in zip(got_of(a), got_of(b)))


@pytest.mark.parametrize("K,voxel", CASES)
def test_against_the_restatement(K, voxel):
    from rslo_amd.mapping import VoxelMap
    frames, poses, ref = case(K, voxel)
    if voxel == 2.0:
        assert (ref.points()[2] >= 2).sum() >= 20           # points of different frames share cells
    assert ref.stats()["n_scans"] == 5 and ref.stats()["n_points"] == sum(counts_of(K))
    vmap = VoxelMap(voxel, 1 << 12)
    vmap.insert_frames(dev_store(frames, K), dev(poses))
    assert_same(vmap, ref, "K %d voxel %.1f" % (K, voxel))
    assert (got_of(vmap)[0][:, 3] != 0).all()               # column 3 of the store's rows travels


@pytest.mark.parametrize("K,voxel", CASES)
def test_against_the_existing_kernel(K, voxel):
    """the same store, frame by frame through VoxelMap.insert on views of its rows: the same map and stats"""
    from rslo_amd.mapping import VoxelMap
    frames, poses, ref = case(K, voxel)
    store, poses_d = dev_store(frames, K), dev(poses)
    rows, _ = store.frames()
    loop = VoxelMap(voxel, 1 << 12)
    for e, c in enumerate(counts_of(K)):
        loop.insert(rows[e][:c], poses_d[e])
    once = VoxelMap(voxel, 1 << 12)
    once.insert_frames(store, poses_d)
    assert same_device_maps(once, loop)
    assert_same(loop, ref, "per-frame loop, K %d voxel %.1f" % (K, voxel))


def test_cells_shared_across_frames():
    """Entries 0 and 3 are the same frame under the same pose, entry 5 is that frame again under a pose shifted by less
    than a voxel: the earliest frame owns every shared cell's tag and row, and the hits add up."""
    from rslo_amd.mapping import VoxelMap, VoxelMapRef
    K, voxel = 320, 0.1
    A, others = make_frames(K, (K,), seed=7)[0], make_frames(K, (K, 100, 17), seed=8)
    frames = [A, others[0], others[1], A, others[2], A]
    poses = make_poses(6, seed=3)
    poses[3] = poses[0]
    poses[5] = poses[0]
    poses[5, :3] += (0.03, -0.02, 0.01)
    sref = store_ref(frames, K)
    ref = VoxelMapRef(voxel)
    ref.insert_frames(sref, poses)
    rhits = ref.points()[2]
    assert (rhits >= 2).sum() >= 50 and (rhits >= 3).sum() >= 50      # 0 + 3 share every cell; most of 5 stay in theirs too
    hits, tags = ref.lookup(A[0], poses[0], return_tags=True)
    assert (hits >= 2).all() and (tags >> 32 == 0).all()              # the earliest frame owns the shared cells
    only0 = VoxelMapRef(voxel)
    only0.insert(A[0], poses[0])
    owned = np.isin(ref.points()[1], only0.points()[1])
    assert ref.points()[0][owned].tobytes() == only0.points()[0].tobytes()      # ... and their rows
    vmap = VoxelMap(voxel, 1 << 12)
    vmap.insert_frames(dev_store(frames, K), dev(poses))
    assert_same(vmap, ref, "shared cells")


def test_non_empty_map_and_continuation():
    """one ordinary insert (S0 = 1), the frames, another ordinary insert: the reference doing the same"""
    from rslo_amd.mapping import VoxelMap, VoxelMapRef
    K, voxel = 320, 0.5
    frames, poses, _ = case(K, 0.1)
    first, last = frame_points(500, 41), frame_points(300, 42)
    first[:, 0] += np.float32(100.0)
    last[:, 1] -= np.float32(100.0)
    p_first, p_last = make_poses(2, seed=9)
    ref = VoxelMapRef(voxel)
    ref.insert(first, p_first)
    ref.insert_frames(store_ref(frames, K), poses)
    ref.insert(last, p_last)
    scans = set((ref.points()[1] >> 32).tolist())
    assert scans == {0, 2, 3, 4, 5, 6}                     # frame 0 (scan 1) is empty; the frames carry scans 1 .. n
    vmap = VoxelMap(voxel, 1 << 12)
    vmap.insert(dev(first), p_first)
    vmap.insert_frames(dev_store(frames, K), dev(poses))
    vmap.insert(dev(last), p_last)
    assert_same(vmap, ref, "continuation")
    tags = got_of(vmap)[1]
    assert set((tags >> 32).tolist()) == scans and vmap.stats()["n_scans"] == 7


def test_clamps():
    from rslo_amd import capi
    from rslo_amd.mapping import VoxelMap, VoxelMapRef
    K, voxel = 64, 0.5
    frames, _, _ = case(K, 0.1)
    sref, store = store_ref(frames, K), dev_store(frames, K)
    poses = make_poses(9, seed=5)
    for m, n in ((3, 3), (9, 5)):                           # fewer poses than entries, more poses than entries
        ref = loop_of_inserts(VoxelMapRef(voxel), sref, poses, n=n)
        vmap = VoxelMap(voxel, 1 << 12)
        vmap.insert_frames(store, dev(poses[:m]))
        assert_same(vmap, ref, "%d poses, 5 entries" % m)
        assert vmap.stats()["n_scans"] == n
    # an empty store, or no poses: the map buffer is unchanged to the byte
    vmap = VoxelMap(voxel, 1 << 12)
    vmap.insert(dev(frame_points(100, 3)), poses[0])
    before = vmap._buf.clone()
    vmap.insert_frames(dev_store([], K), dev(poses))
    vmap.insert_frames(store, dev(poses[:0]))
    ptr, nbytes = vmap._buf.data_ptr(), vmap._buf.numel() * 8
    sptr, sbytes = store._buf.data_ptr(), store._buf.numel() * 8
    poses_d = dev(poses)
    capi._chk(capi.lib().rslo_map_insert_frames(ptr, nbytes, sptr, sbytes, store.capacity, K, poses_d.data_ptr(), 0, None), "n = 0")
    # ... and a store whose header disagrees with (capacity, K) is no store
    capi._chk(capi.lib().rslo_map_insert_frames(ptr, nbytes, sptr, sbytes, 8, K, poses_d.data_ptr(), 5, None), "other shape")
    torch.cuda.synchronize()
    assert torch.equal(vmap._buf, before)
    # a map that was never reset is no map: nothing is written
    raw = torch.full((capi.map_bytes(1024) // 8,), SENTINEL, dtype=torch.int64, device="cuda")
    capi._chk(capi.lib().rslo_map_insert_frames(raw.data_ptr(), raw.numel() * 8, sptr, sbytes, store.capacity, K,
                                                poses_d.data_ptr(), 5, None), "never reset")
    torch.cuda.synchronize()
    assert bool((raw == SENTINEL).all())
    # a pose row of NaN: that frame's valid points are dropped_range, the others are exact
    bad = poses[:5].copy()
    bad[2] = np.nan
    ref = VoxelMapRef(voxel)
    ref.insert_frames(sref, bad)
    assert ref.stats()["dropped_range"] == 63 and ref.stats()["n_points"] == sum(counts_of(K)) - 63
    vmap = VoxelMap(voxel, 1 << 12)
    vmap.insert_frames(store, dev(bad))
    assert_same(vmap, ref, "NaN pose")


def test_overflow():
    """40 frames x 64 points in 2560 distinct cells and only 1024 slots: dropped_full > 0 is certain by counting.  The call
    returns, and every cell that IS stored has the reference's tag, hits and row."""
    from rslo_amd.mapping import VoxelMap, VoxelMapRef
    K, voxel, F = 64, 0.1, 40
    frames, poses = make_frames(K, (K,) * F, seed=11, spread=40.0), make_poses(F, seed=11)
    ref = VoxelMapRef(voxel)
    ref.insert_frames(store_ref(frames, K, capacity=64), poses)
    rrows, rtags, rhits = ref.points()
    assert ref.stats()["n_cells"] == F * K == 2560 and ref.stats()["n_points"] == 2560
    vmap = VoxelMap(voxel, 1024)
    vmap.insert_frames(dev_store(frames, K, capacity=64), dev(poses))
    rows, tags, hits = got_of(vmap)
    st = vmap.stats()
    print("overflow: %s" % st)
    assert st["dropped_full"] > 0 and st["n_points"] + st["dropped_full"] == ref.stats()["n_points"]
    assert st["n_scans"] == F and st["dropped_invalid"] == 0 and st["dropped_range"] == 0
    assert st["n_cells"] == len(tags) <= 1024 and len(set(tags.tolist())) == len(tags)
    at = np.searchsorted(rtags, tags)
    assert (at < len(rtags)).all() and (rtags[at] == tags).all()
    assert (hits == rhits[at]).all() and int(hits.sum()) == st["n_points"]
    assert (rows.view(np.int32) == rrows[at].view(np.int32)).all()


def test_more_tiles_than_workgroups():
    """The points pass launches at most 2048 workgroups, which then take further tiles of 256 rows in a loop: 2100 frames
    of K = 64 (one tile each) reach the second round.  Counts 0, 1, 3 and 64 in turn keep the restatement's 2100 inserts
    quick; at a 2 m voxel most cells are shared between frames."""
    from rslo_amd.mapping import VoxelMap, VoxelMapRef
    K, voxel, F = 64, 2.0, 2100
    frames = make_frames(K, [(0, 1, 3, K)[e % 4] for e in range(F)], seed=13)
    poses = make_poses(F, seed=13)
    ref = VoxelMapRef(voxel)
    ref.insert_frames(store_ref(frames, K, capacity=4096), poses)
    rtags, rhits = ref.points()[1:]
    assert ref.stats()["n_scans"] == F and ref.stats()["n_points"] == 525 * 68
    assert rhits.max() > 20 and sum(int(info[0]) for _, info in frames[2048:]) > 0      # the second round carries points
    vmap = VoxelMap(voxel, 1 << 12)
    vmap.insert_frames(dev_store(frames, K, capacity=4096), dev(poses))
    assert_same(vmap, ref, "2100 frames")


def test_determinism_and_capture():
    from rslo_amd.mapping import VoxelMap
    K, voxel = 320, 2.0
    frames, poses, ref = case(K, voxel)
    store, poses_d = dev_store(frames, K), dev(poses)
    maps = []
    for _ in range(2):                                      # two calls on fresh maps: identical bits
        vmap = VoxelMap(voxel, 1 << 12)
        vmap.insert_frames(store, poses_d)
        maps.append(vmap)
    assert same_device_maps(*maps)
    assert_same(maps[0], ref, "eager")
    vmap = VoxelMap(voxel, 1 << 12)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with quiet_collector(), torch.cuda.graph(g):
        vmap.insert_frames(store, poses_d)
    assert vmap.stats()["n_scans"] == 0                     # captured, not run
    for _ in range(2):                                      # replayed into a reset map: the eager map
        vmap.reset()
        g.replay()
        torch.cuda.synchronize()
        assert same_device_maps(vmap, maps[0])


def test_argument_errors_write_nothing():
    from rslo_amd import capi
    from rslo_amd.mapping import VoxelMap
    K = 64
    frames, poses, _ = case(K, 0.1)
    store, poses_d = dev_store(frames, K), dev(poses)
    vmap = VoxelMap(0.5, 1 << 12)
    vmap.insert(dev(frame_points(100, 3)), poses[0])
    before = vmap._buf.clone()
    good = dict(map=vmap._buf.data_ptr(), map_bytes=vmap._buf.numel() * 8, store=store._buf.data_ptr(),
                store_bytes=store._buf.numel() * 8, capacity=store.capacity, K=K, poses=poses_d.data_ptr(), n=5)
    call = lambda **kw: capi._chk(capi.lib().rslo_map_insert_frames(*[{**good, **kw}[k] for k in (
        "map", "map_bytes", "store", "store_bytes", "capacity", "K", "poses", "n")], None), "rslo_map_insert_frames")
    for bad in (dict(map=None), dict(store=None), dict(poses=None), dict(n=-1), dict(capacity=0), dict(capacity=(1 << 16) + 1),
                dict(K=0), dict(K=100), dict(K=4160), dict(store_bytes=good["store_bytes"] - 8),
                dict(map_bytes=capi.map_bytes(1024) - 8), dict(store=good["store"] + 8)):
        with pytest.raises(capi.RsloHipError):
            call(**bad)
    for bad in (poses_d[:, :6], poses_d.float(), poses_d.reshape(-1), poses[:, :6]):      # the wrong shape or type
        with pytest.raises(capi.RsloHipError):
            vmap.insert_frames(store, bad)
    with pytest.raises(capi.RsloHipError):
        capi.map_insert_frames(vmap._buf, store._buf, store.capacity, K, poses_d.cpu())
    torch.cuda.synchronize()
    assert torch.equal(vmap._buf, before)
    call()                                                  # ... and the good call is one
    torch.cuda.synchronize()
    assert vmap.stats()["n_scans"] == 6


def test_pyramid():
    from rslo_amd.mapping import MapPyramid, MapPyramidRef
    K = 320
    frames, poses, _ = case(K, 0.1)
    ref = MapPyramidRef(voxel_sizes=(2.0, 0.1))
    ref.insert_frames(store_ref(frames, K), poses)
    pyr = MapPyramid(voxel_sizes=(2.0, 0.1), capacity=1 << 12)
    pyr.insert_frames(dev_store(frames, K), poses)          # host poses: copied to the device once
    for k in range(2):
        assert_same(pyr.levels[k], ref.levels[k], "level %d" % k)


# ---------------------------------------------------------------------------------------------------------------------
# the runner
# ---------------------------------------------------------------------------------------------------------------------
LOOP = dict(exclude_recent=1, num_candidates=2, top_k=2)
odom = odom_fixture(21, 3, 3)


def test_runner_rebuilds_and_adopts(odom):
    """Three scans of the drive, the revisit of tests/test_gpu_loops.py and one more scan.  min_pairs = 10^9 makes every
    registration report "too few pairs" and leave the prediction as it is, so every expectation is exact."""
    from rslo_amd import capi, inference, loops, places, posegraph, synthetic
    from rslo_amd.mapping import VoxelMap, VoxelMapRef
    net, scans = odom
    scans = list(scans) + [dev(synthetic.scan(2083, 64, (0.5, 0.4), 0.2, scan_seed=999))]
    extra = dev(synthetic.scan(2083, 64, (1.0, 0.6), 0.25, scan_seed=1000))
    plain = inference.OdometryRunner(net, capacity=16)
    try:
        keys0 = set(plain.stats)
        with pytest.raises(capi.RsloHipError):
            plain.adopt_loop_closure()                      # no refine
        with pytest.raises(capi.RsloHipError):
            plain.rebuild_map()                             # no keyframes
    finally:
        plain.close()
    store, vmap = loops.KeyframeStore(capacity=16, K=1024), VoxelMap(0.5, 1 << 18)
    runner = inference.OdometryRunner(net, capacity=16, voxel_map=vmap, refine=dict(iters=1, min_pairs=10 ** 9),
                                      places=places.PlaceDB(capacity=16), loop=LOOP, keyframes=store,
                                      verify=dict(max_edges=8), pose_graph=posegraph.PoseGraph(capacity=16, max_loops=8))
    try:
        with quiet_collector():
            rel, traj = stream(runner, scans)
        with pytest.raises(capi.RsloHipError):
            runner.adopt_loop_closure()                     # before close_loops()
        with pytest.raises(capi.RsloHipError):
            runner.rebuild_map()                            # no poses to use
        assert (runner.refine_info().cpu().numpy()[:, :, 0] == 1).all()      # every registration: too few pairs
        poses, info = runner.close_verified_loops(gn_iters=3)
        assert int(info.cpu().numpy()[0, 1]) >= 1           # a loop edge was used
        runner.adopt_loop_closure()
        torch.cuda.synchronize()
        assert same_bits(runner.refined_trajectory(), poses) and runner.optimized_trajectory() is poses
        assert runner.trajectory().cpu().numpy().tobytes() == traj.tobytes()
        assert runner.relative().cpu().numpy().tobytes() == rel.tobytes()
        sref = store.reference()
        for s in scans:
            sref.prepare(s.cpu().numpy())
            sref.add()
        got_rows, got_counts = store.entries()
        assert got_rows.tobytes() == sref.entries()[0].tobytes() and got_counts.tolist() == sref.counts
        ref = VoxelMapRef(0.5)
        ref.insert_frames(sref, poses.cpu().numpy())
        assert ref.stats()["n_points"] > 1000
        assert_same(vmap, ref, "adopted map")
        assert vmap.stats()["n_scans"] == 4
        other, own = VoxelMap(0.5, 1 << 14), vmap._buf.clone()
        assert runner.rebuild_map(voxel_map=other) is other
        torch.cuda.synchronize()
        assert torch.equal(vmap._buf, own)                  # the runner's own map: untouched to the byte
        assert_same(other, ref, "rebuilt into a second map")
        with quiet_collector():
            stream(runner, [extra])                         # the next scan composes onto the corrected pose
        state, count = poses[3].clone(), torch.tensor([4], dtype=torch.int32, device="cuda")
        rel_rows = torch.zeros((16, 7), dtype=torch.float32, device="cuda")
        chain = torch.zeros((16, 7), dtype=torch.float64, device="cuda")
        r = runner.relative()[4]
        capi.pose_chain(r[:3], r[3:], state, count, rel_rows, chain)      # the project's existing kernel
        torch.cuda.synchronize()
        assert same_bits(runner.refined_trajectory()[4], chain[4]) and same_bits(runner.refined_trajectory()[:4], poses)
        assert runner.trajectory().cpu().numpy()[:4].tobytes() == traj.tobytes()
        assert vmap.stats()["n_scans"] == 5
        assert set(runner.stats) == keys0
        with pytest.raises(capi.RsloHipError):
            runner.adopt_loop_closure()                     # the correction is one scan old
    finally:
        runner.close()
