"""The map after loop closure, host side: VoxelMapRef.insert_frames (rslo_amd/mapping.py) is DEFINED as successive inserts
of a keyframe store's frames, each under its own pose.  These tests pin that definition on hand-made stores -- the arbiter
of tests/test_gpu_map_frames.py -- and carry the helpers both files build their stores with."""
import numpy as np

K = 64
COUNTS = (0, 1, 37, K, K)


def frame_points(n, seed, spread=6.0):
    """[n, 4] float32: points within +-spread metres, a non-zero intensity in column 3"""
    rng = np.random.default_rng(seed)
    f = np.zeros((n, 4), np.float32)
    f[:, :3] = rng.uniform(-spread, spread, (n, 3))
    f[:, 3] = rng.uniform(0.1, 1.0, n)
    return f


def make_frames(K, counts, seed=0, spread=6.0):
    """[(frame [K, 4], info int32 [4])]: EVERY row of a frame is a real point, so a row >= count that reached the map
    would show"""
    return [(frame_points(K, seed + 100 * e, spread), np.array([c, c, 0, 0], np.int32)) for e, c in enumerate(counts)]


def make_poses(n, seed=0, shift=3.0):
    """[n, 7] float64 (t, q wxyz): all four quaternion components non-zero, unit norm"""
    rng = np.random.default_rng(1000 + seed)
    q = rng.uniform(0.2, 1.0, (n, 4)) * rng.choice([-1.0, 1.0], (n, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    assert (np.abs(q) > 0.05).all()
    return np.concatenate([rng.uniform(-shift, shift, (n, 3)), q], 1)


def filled(store, frames, put=lambda a: a):
    """store (device or restatement) with the frames added in order; put: host array -> what store.add takes"""
    for frame, info in frames:
        store.add(put(frame), put(info))
    return store


def store_ref(frames, K, capacity=16):
    from rslo_amd import loops
    return filled(loops.KeyframeStoreRef(capacity=capacity, K=K), frames)


def loop_of_inserts(ref_map, sref, poses, n=None):
    """the definition, written out"""
    n = min(len(sref.rows), len(poses)) if n is None else n
    for e in range(n):
        ref_map.insert(sref.rows[e][:sref.counts[e]], poses[e])
    return ref_map


def same_maps(a, b):
    return a.stats() == b.stats() and all(x.tobytes() == y.tobytes() for x, y in zip(a.points(), b.points()))


def test_insert_frames_is_the_loop_of_inserts():
    from rslo_amd.mapping import VoxelMapRef
    sref = store_ref(make_frames(K, COUNTS), K)
    assert sref.counts == list(COUNTS)
    poses = make_poses(len(COUNTS))
    for voxel in (0.1, 2.0):
        got = VoxelMapRef(voxel)
        got.insert_frames(sref, poses)
        want = loop_of_inserts(VoxelMapRef(voxel), sref, poses)
        assert same_maps(got, want)
        st = got.stats()
        assert st["n_scans"] == len(COUNTS) and st["n_points"] == sum(COUNTS)      # the empty frame counts as a scan
        rows, tags, hits = got.points()
        assert int(hits.sum()) == sum(COUNTS)
        scans = set((tags >> 32).tolist())
        assert scans <= {1, 2, 3, 4} and 1 in scans and 0 not in scans             # frame 0 is empty
        assert ((tags & 0xffffffff) < np.array(COUNTS)[tags >> 32]).all()           # no row >= count reached the map
        assert (rows[:, 3] != 0).all()                                              # column 3 travels
    shared = VoxelMapRef(2.0)
    shared.insert_frames(sref, poses)
    assert (shared.points()[2] >= 2).sum() >= 5                                     # cells shared between points
    # a map that already holds a scan: the frames continue its scan numbers
    first = frame_points(50, 77)
    got, want = VoxelMapRef(0.5), VoxelMapRef(0.5)
    got.insert(first, poses[0])
    want.insert(first, poses[0])
    got.insert_frames(sref, poses)
    loop_of_inserts(want, sref, poses)
    assert same_maps(got, want) and got.stats()["n_scans"] == 1 + len(COUNTS)


def test_the_shorter_of_entries_and_poses_counts():
    from rslo_amd.mapping import VoxelMapRef
    sref = store_ref(make_frames(K, COUNTS), K)
    more, fewer = make_poses(7), make_poses(7)[:3]
    got = VoxelMapRef(0.5)
    got.insert_frames(sref, more)                        # poses beyond n_entries are ignored
    assert same_maps(got, loop_of_inserts(VoxelMapRef(0.5), sref, more, n=5)) and got.stats()["n_scans"] == 5
    got = VoxelMapRef(0.5)
    got.insert_frames(sref, fewer)                       # entries beyond len(poses) are ignored
    assert same_maps(got, loop_of_inserts(VoxelMapRef(0.5), sref, fewer, n=3)) and got.stats()["n_scans"] == 3
    assert got.stats()["n_points"] == sum(COUNTS[:3])
    got = VoxelMapRef(0.5)
    got.insert_frames(sref, np.zeros((0, 7)))
    assert got.stats()["n_scans"] == 0 and len(got.points()[1]) == 0
    empty = store_ref([], K)
    got.insert_frames(empty, more)
    assert got.stats()["n_scans"] == 0


def test_pyramid_reaches_every_level():
    from rslo_amd.mapping import MapPyramidRef, VoxelMapRef
    sref = store_ref(make_frames(K, COUNTS), K)
    poses = make_poses(len(COUNTS))
    pyr = MapPyramidRef(voxel_sizes=(2.0, 0.5, 0.1))
    pyr.insert_frames(sref, poses)
    for level, voxel in zip(pyr.levels, (2.0, 0.5, 0.1)):
        assert same_maps(level, loop_of_inserts(VoxelMapRef(voxel), sref, poses))
        assert level.stats()["n_scans"] == len(COUNTS) and level.stats()["n_points"] == sum(COUNTS)
    assert len(pyr.levels[0].points()[1]) < len(pyr.levels[2].points()[1])
