"""Rolling local map on the GPU (rslo_map_prune in csrc/map.hip, VoxelMap.prune) against VoxelMapRef.prune on the same inputs,
and the map an OdometryRunner keeps with local_map=.

The bar is that of tests/test_gpu_map.py: BIT equality after sorting by tag -- rows (viewed as int32), tags, hits, the six
counters and the three prune counters -- with no tolerance: the keep / evict rule is an IEEE double comparison on stored
fp32 rows in a fixed order plus integer comparisons, and a kept cell is copied, not recomputed.  The rebuild loses no
cell (n_lost == 0) whenever the survivors' longest run of occupied slots is below the probe limit of 128; the tests
that lean on it restate the map's hash in numpy and assert that as a precondition.
"""
import numpy as np
import pytest
import torch
from stream_support import dev, network_and_scans, stream

pytestmark = pytest.mark.gpu

IDENT = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
POSE_YAW = np.array([1.0, -0.5, 0.1, np.cos(0.15), 0.0, 0.0, np.sin(0.15)], np.float64)
_q = np.array([0.9, 0.1, -0.3, 0.25])
POSE_FULL = np.concatenate([[-2.0, 3.0, 0.4], _q / np.linalg.norm(_q)])
POSE_BACK = np.array([-1.5, 1.0, 0.05, np.cos(0.1), 0.0, 0.0, -np.sin(0.1)], np.float64)
CENTER = np.array([3.0, -2.0, 0.1])
PROBE = 128
_CLOUD = {}


def _cloud(seed, n=4000):
    from rslo_amd import synthetic
    if (seed, n) not in _CLOUD:
        _CLOUD[(seed, n)] = synthetic.small_cloud(n, seed=seed)
    return _CLOUD[(seed, n)]


def _got(vmap, **kw):
    rows, tags, hits = vmap.points(**kw)
    return rows.cpu().numpy(), tags.cpu().numpy(), hits.cpu().numpy()


def _assert_same(vmap, ref, label=""):
    rows, tags, hits = _got(vmap)
    rrows, rtags, rhits = ref.points()
    st, rst, ps, rps = vmap.stats(), ref.stats(), vmap.prune_stats(), ref.prune_stats()
    print("%s: cells kernel %d, reference %d; counters %s; prune %s" % (label, len(tags), len(rtags), st, ps))
    assert st == rst and ps == rps
    assert len(tags) == len(rtags) and (tags == rtags).all()
    assert (hits == rhits).all()
    assert rows.dtype == np.float32 and (rows.view(np.int32) == rrows.view(np.int32)).all()


def _pair(voxel, capacity, scans):
    """(VoxelMap, VoxelMapRef) filled with scans = ((cloud [P, F] numpy, pose), ...)"""
    from rslo_amd.mapping import VoxelMap, VoxelMapRef
    vmap, ref = VoxelMap(voxel, capacity), VoxelMapRef(voxel)
    for cloud, pose in scans:
        vmap.insert(dev(cloud), pose)
        ref.insert(cloud, pose)
    return vmap, ref


# the map's hash (csrc/map_table.h map_mix, the splitmix64 finaliser) and the occupied set of a linear-probing table, which
# does not depend on the insertion order
def _home(keys, cap):
    x = np.asarray(keys).astype(np.uint64)
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint64(30))
        x = x * np.uint64(0xbf58476d1ce4e5b9)
        x = x ^ (x >> np.uint64(27))
        x = x * np.uint64(0x94d049bb133111eb)
        x = x ^ (x >> np.uint64(31))
    return (x & np.uint64(cap - 1)).astype(np.int64)


def _occupied(keys, cap):
    occ = np.zeros((cap,), bool)
    for h in _home(keys, cap).tolist():
        while occ[h]:
            h = (h + 1) & (cap - 1)
        occ[h] = True
    return occ


def _longest_run(occ):
    """longest run of occupied slots, wrap-around included"""
    if occ.all():
        return len(occ)
    r = np.roll(occ, -int(np.nonzero(~occ)[0][0]))
    edges = np.flatnonzero(np.diff(np.concatenate([[0], r.astype(np.int8), [0]])))
    return int((edges[1::2] - edges[::2]).max()) if len(edges) else 0


def _near(rows, center, radius):
    d = rows[:, :3].astype(np.float64) - np.asarray(center, np.float64)[None, :]
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]) < radius * radius


@pytest.mark.parametrize("K", [0, 1, 63, 64, 65, 257, 1000])
def test_survivor_counts(K):
    """1000 cells in a row along x, one point at the centre of each: cell i lies at ((i + 0.5) v, v / 2, v / 2), and
    ((i + 0.5)^2 + 0.5) v^2 < (K v)^2 holds exactly for i < K (all terms are exact in binary at v = 0.5).  The slots of
    the cells are scattered over the table, so the kept ones cross lanes, waves and blocks of the compaction."""
    voxel = 0.5
    pts = np.zeros((1000, 4), np.float32)
    pts[:, 0] = (np.arange(1000) + 0.5) * voxel
    pts[:, 1:3] = 0.5 * voxel
    pts[:, 3] = np.arange(1000) / 1000.0
    vmap, ref = _pair(voxel, 4096, ((pts, IDENT),))
    assert ref.stats()["n_cells"] == 1000
    center = torch.zeros(3, dtype=torch.float64, device="cuda")
    vmap.prune(center, K * voxel)
    ref.prune(np.zeros(3), K * voxel)
    assert ref.stats()["n_cells"] == K and ref.prune_stats() == {"n_prunes": 1, "n_evicted": 1000 - K, "n_lost": 0}
    _assert_same(vmap, ref, "K %d" % K)
    assert (_got(vmap)[1] == np.arange(K)).all()
    hits = vmap.lookup(dev(pts), IDENT).cpu().numpy()
    assert (hits[:K] == 1).all() and (hits[K:] == 0).all()


def test_minimum_table_with_wrap_around():
    vmap, ref = _pair(1.0, 1024, ((_cloud(5, 1000), IDENT),))
    center, radius = np.array([2.0, 1.0, 0.0]), 12.0
    keep = _near(ref.rows, center, radius)
    occ0, occ1 = _occupied(ref.keys, 1024), _occupied(ref.keys[keep], 1024)
    print("cells %d (longest run %d), survivors %d (longest run %d), slots 1023 and 0 occupied: %s" % (
        len(ref.keys), _longest_run(occ0), int(keep.sum()), _longest_run(occ1), bool(occ1[1023] and occ1[0])))
    # preconditions: ~600 cells stored without overflow, a real eviction, survivors within the probe limit, and a run of
    # occupied slots that crosses the end of the table
    assert 560 <= len(ref.keys) <= 614 and _longest_run(occ0) < PROBE
    assert 200 < keep.sum() < len(ref.keys) - 200
    assert _longest_run(occ1) < PROBE and occ1[1023] and occ1[0]
    assert vmap.stats()["dropped_full"] == 0
    vmap.prune(center, radius)
    ref.prune(center, radius)
    assert vmap.prune_stats()["n_lost"] == 0
    _assert_same(vmap, ref, "capacity 1024")
    got = vmap.lookup(dev(_cloud(5, 1000)), IDENT).cpu().numpy()
    assert (got == ref.lookup(_cloud(5, 1000), IDENT)).all() and (got == 0).sum() > 200


def test_nothing_evicted_leaves_the_table_alone():
    vmap, ref = _pair(0.4, 1 << 14, ((_cloud(0), IDENT), (_cloud(5), POSE_YAW)))
    hdr = 256 // 8
    before = vmap._buf.clone()
    for kw in (dict(), dict(center=CENTER, radius=float("inf")), dict(center=dev(POSE_YAW), radius=1.0e4),
               dict(min_hits=3, grace=2)):      # with two scans every cell is younger than 2
        n0 = vmap.prune_stats()["n_prunes"]
        vmap.prune(**kw)
        ref.prune(**{k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in kw.items()})
        assert torch.equal(vmap._buf[hdr:], before[hdr:])            # every slot section, to the byte
        assert vmap.prune_stats() == {"n_prunes": n0 + 1, "n_evicted": 0, "n_lost": 0}
        changed = torch.nonzero(vmap._buf[:hdr] != before[:hdr]).flatten().tolist()
        assert changed == [5]                                        # n_prunes and nothing else in the header
    _assert_same(vmap, ref, "nothing evicted")


def test_life_after_a_prune():
    vmap, ref = _pair(0.4, 1 << 14, ((_cloud(0), IDENT), (_cloud(5), POSE_YAW)))
    third = _cloud(7)
    was = ref.lookup(third, POSE_BACK)
    for m in (vmap, ref):
        m.prune(CENTER, 6.0)
    _assert_same(vmap, ref, "two scans, pruned")
    now = ref.lookup(third, POSE_BACK)
    n_evicted_hit = int(((was > 0) & (now == 0)).sum())
    print("third scan: %d points in kept cells, %d in evicted cells, %d in cells never stored" % (
        int((now > 0).sum()), n_evicted_hit, int((was == 0).sum())))
    assert n_evicted_hit > 50 and (now > 0).sum() > 50 and 100 < ref.stats()["n_cells"] < ref.prune_stats()["n_evicted"]
    hits, tags = vmap.lookup(dev(third), POSE_FULL, return_tags=True)      # an evicted cell reads 0, not its old hits
    whits, wtags = ref.lookup(third, POSE_FULL, return_tags=True)
    assert (hits.cpu().numpy() == whits).all() and (tags.cpu().numpy() == wtags).all()
    vmap.insert(dev(third), POSE_BACK)
    ref.insert(third, POSE_BACK)
    _assert_same(vmap, ref, "third scan after the prune")
    rtags = ref.points()[1]
    assert (rtags >> 32 == 2).sum() > n_evicted_hit // 4                    # evicted cells were created afresh by scan 2
    q = _cloud(9)
    hits, tags = vmap.lookup(dev(q), POSE_YAW, return_tags=True)
    whits, wtags = ref.lookup(q, POSE_YAW, return_tags=True)
    assert (whits > 0).sum() > 100 and (hits.cpu().numpy() == whits).all() and (tags.cpu().numpy() == wtags).all()
    t, d2, rows = vmap.nearest(dev(q), dev(POSE_YAW), return_rows=True)
    wt, wd, wr = ref.nearest(q, POSE_YAW, return_rows=True)
    assert (wt >= 0).sum() > 100 and (t.cpu().numpy() == wt).all()
    assert (d2.cpu().numpy().view(np.int64) == wd.view(np.int64)).all()
    assert (rows.cpu().numpy().view(np.int32) == wr.view(np.int32)).all()
    # and a second prune, about a pose row on the device, with the sparse rule
    vmap.prune(dev(POSE_BACK), 8.0, min_hits=2, grace=1)
    ref.prune(POSE_BACK, 8.0, min_hits=2, grace=1)
    assert ref.prune_stats()["n_prunes"] == 2 and 0 < ref.stats()["n_cells"]
    _assert_same(vmap, ref, "second prune")


def test_overflow_recovery():
    """A table that overflowed holds an unspecified set of complete cells; a prune to a small sphere empties it enough
    for the next scan to be stored whole."""
    from rslo_amd.mapping import VoxelMap, VoxelMapRef
    full = VoxelMapRef(0.4)
    full.insert(_cloud(0), IDENT)
    center, radius = np.array([3.0, -2.0, 0.1]), 3.5
    could = _near(full.rows, center, radius)       # a superset of the survivors, whatever the table stored
    fresh = np.zeros((200, 4), np.float32)
    fresh[:, 0] = 500.2 + 0.4 * np.arange(200)
    fresh[:, 1] = 0.2
    fresh[:, 3] = 0.5
    probe = VoxelMapRef(0.4)
    probe.insert(fresh, IDENT)
    union = np.concatenate([full.keys[could], probe.keys])
    print("at most %d survivors, longest run with the fresh scan %d" % (int(could.sum()), _longest_run(_occupied(union, 1024))))
    assert 50 < could.sum() <= 256 and len(probe.keys) == 200 and _longest_run(_occupied(union, 1024)) < PROBE
    vmap = VoxelMap(0.4, 1024)
    vmap.insert(dev(_cloud(0)), IDENT)
    st0 = vmap.stats()
    assert st0["dropped_full"] > 0
    rows, tags, hits = _got(vmap)
    keep = _near(rows, center, radius)
    assert 0 < keep.sum() <= 256
    vmap.prune(center, radius)
    got = _got(vmap)
    assert got[0].tobytes() == rows[keep].tobytes() and (got[1] == tags[keep]).all() and (got[2] == hits[keep]).all()
    st = vmap.stats()
    assert st == dict(st0, n_cells=int(keep.sum()))
    assert vmap.prune_stats() == {"n_prunes": 1, "n_evicted": len(tags) - int(keep.sum()), "n_lost": 0}
    vmap.insert(dev(fresh), IDENT)
    st2 = vmap.stats()
    assert st2["dropped_full"] == st0["dropped_full"] and st2["n_cells"] == st["n_cells"] + 200
    assert bool((vmap.lookup(dev(fresh), IDENT) > 0).all())


@pytest.mark.parametrize("grace", [0, 1])
def test_sparse_rule(grace):
    vmap, ref = _pair(0.4, 1 << 14, ((_cloud(0), IDENT), (_cloud(5), POSE_YAW), (_cloud(7), POSE_FULL)))
    rtags, rhits = ref.points()[1:]
    single_old = int(((rhits < 2) & (rtags >> 32 < 2)).sum())
    single_last = int(((rhits < 2) & (rtags >> 32 == 2)).sum())
    assert single_old > 100 and single_last > 100 and (rhits >= 2).sum() > 100
    vmap.prune(min_hits=2, grace=grace)
    ref.prune(min_hits=2, grace=grace)
    assert ref.prune_stats()["n_evicted"] == single_old + (single_last if grace == 0 else 0)
    _assert_same(vmap, ref, "min_hits 2, grace %d" % grace)


def test_capture_and_replay():
    """insert + prune captured once; replayed with two scans and two centres copied into the static tensors"""
    from rslo_amd.mapping import VoxelMap, VoxelMapRef
    clouds = [_cloud(0)[:, :4], _cloud(5)[:, :4]]
    poses = [IDENT, POSE_YAW]
    radius = 7.0
    warm = VoxelMap(0.4, 1 << 14)                   # the kernels' first launches, outside the capture
    warm.insert(dev(clouds[0]), IDENT)
    warm.prune(dev(IDENT), radius)
    vmap, ref = VoxelMap(0.4, 1 << 14), VoxelMapRef(0.4)
    vmap.reserve(len(clouds[0]))
    vmap.reserve_prune()
    static_pts = torch.zeros((len(clouds[0]), 4), dtype=torch.float32, device="cuda")
    static_pose = torch.zeros(7, dtype=torch.float64, device="cuda")
    on_dev = [(dev(c), dev(p)) for c, p in zip(clouds, poses)]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        vmap.insert(static_pts, static_pose)
        vmap.prune(static_pose, radius)             # the centre is the pose row's translation, read in place
    assert vmap.stats()["n_scans"] == 0 and vmap.prune_stats()["n_prunes"] == 0      # captured, not run
    torch.cuda.synchronize()
    mem = torch.cuda.memory_allocated()
    for k, (c, p) in enumerate(on_dev):
        static_pts.copy_(c)
        static_pose.copy_(p)
        g.replay()
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == mem
        ref.insert(clouds[k], poses[k])
        ref.prune(poses[k], radius)
        assert ref.prune_stats()["n_evicted"] > 100 * (k + 1) and ref.stats()["n_cells"] > 100
        _assert_same(vmap, ref, "replay %d" % k)
    assert torch.cuda.memory_allocated() == mem


def test_determinism():
    first = None
    for _ in range(2):
        vmap, _ = _pair(0.4, 1 << 14, ((_cloud(0), IDENT), (_cloud(5), POSE_YAW)))
        vmap.prune(CENTER, 6.0)
        vmap.insert(dev(_cloud(7)), POSE_BACK)
        vmap.prune(dev(POSE_BACK), 9.0, min_hits=2, grace=1)
        got = _got(vmap), vmap.stats(), vmap.prune_stats()
        assert len(got[0][1]) > 100 and got[2]["n_prunes"] == 2
        if first is not None:
            assert all(a.tobytes() == b.tobytes() for a, b in zip(first[0], got[0])) and first[1:] == got[1:]
        first = got


def test_argument_errors_write_nothing():
    from rslo_amd import capi
    lib = capi.lib()
    vmap, ref = _pair(0.4, 2048, ((_cloud(0)[:1000], IDENT),))
    vmap.reserve_prune()
    before = vmap._buf.clone()
    buf, ws = vmap._buf, vmap._prune_ws
    c = dev(CENTER)
    nb, wb = buf.numel() * 8, ws.numel() * 8
    assert wb == lib.rslo_map_prune_ws_bytes(2048)
    rcs = [lib.rslo_map_prune(buf.data_ptr(), nb, c.data_ptr(), -1.0, 1, 0, ws.data_ptr(), wb, None),
           lib.rslo_map_prune(buf.data_ptr(), nb, c.data_ptr(), float("nan"), 1, 0, ws.data_ptr(), wb, None),
           lib.rslo_map_prune(buf.data_ptr(), nb, c.data_ptr(), 1.0, 0, 0, ws.data_ptr(), wb, None),
           lib.rslo_map_prune(buf.data_ptr(), nb, c.data_ptr(), 1.0, 1, -1, ws.data_ptr(), wb, None),
           lib.rslo_map_prune(buf.data_ptr(), nb, c.data_ptr(), 1.0, 1, 0, None, wb, None),
           lib.rslo_map_prune(buf.data_ptr(), nb, c.data_ptr(), 1.0, 1, 0, ws.data_ptr() + 8, wb - 8, None),
           lib.rslo_map_prune(buf.data_ptr(), 1000, c.data_ptr(), 1.0, 1, 0, ws.data_ptr(), wb, None),
           lib.rslo_map_prune(buf.data_ptr(), nb, c.data_ptr(), 1.0, 1, 0, ws.data_ptr(), wb - 16, None)]      # RSLO_EWS
    print("return codes:", rcs, lib.rslo_last_error().decode())
    assert all(rc != 0 for rc in rcs) and rcs[-1] != rcs[0]
    for kw in (dict(center=CENTER), dict(center=CENTER, radius=-1.0), dict(center=CENTER, radius=float("nan")),
               dict(min_hits=0), dict(grace=-1)):
        with pytest.raises(ValueError):
            vmap.prune(**kw)
    with pytest.raises(capi.RsloHipError):
        vmap.prune(torch.zeros(3, dtype=torch.float64, device="cuda")[:2], 1.0)
    torch.cuda.synchronize()
    assert torch.equal(vmap._buf, before)
    _assert_same(vmap, ref, "after refused calls")


# ---------------------------------------------------------------------------------------------------------------------
# the runner's local map
# ---------------------------------------------------------------------------------------------------------------------
N_SCANS = 4
MAP_ARGS = dict(voxel_size=0.2, capacity=1 << 21, min_range=2.5, max_range=80.0)
LOCAL = dict(radius=30.0, every=2)


def test_runner_keeps_a_local_map():
    from rslo_amd import capi, inference
    from rslo_amd.mapping import VoxelMap, VoxelMapRef
    net, scans = network_and_scans(21, 3, N_SCANS)
    plain = inference.OdometryRunner(net)
    try:
        rel0, traj0 = stream(plain, scans)
    finally:
        plain.close()
    for bad in (dict(radius=30.0, every=0), dict(radius=30.0, evry=2), dict(every=2), dict(radius=-1.0)):
        with pytest.raises((capi.RsloHipError, ValueError)):
            inference.OdometryRunner(net, voxel_map=VoxelMap(0.2, 1024), local_map=bad)
    with pytest.raises(capi.RsloHipError):
        inference.OdometryRunner(net, local_map=LOCAL)          # needs a voxel_map
    vmap = VoxelMap(**MAP_ARGS)
    runner = inference.OdometryRunner(net, voxel_map=vmap, local_map=LOCAL)
    try:
        assert vmap._prune_ws is not None                       # reserved by the constructor
        rel, traj = stream(runner, scans)
        assert rel.tobytes() == rel0.tobytes() and traj.tobytes() == traj0.tobytes()      # the local map disturbs nothing
        ref = VoxelMapRef(MAP_ARGS["voxel_size"], MAP_ARGS["min_range"], MAP_ARGS["max_range"])
        for n, (s, pose) in enumerate(zip(scans, traj)):
            ref.insert(s.cpu().numpy(), pose)
            if (n + 1) % LOCAL["every"] == 0:
                ref.prune(pose, LOCAL["radius"])
        assert ref.prune_stats()["n_prunes"] == 2 and ref.prune_stats()["n_evicted"] > 1000
        assert ref.stats()["n_cells"] > 10000
        _assert_same(vmap, ref, "runner, local map")
        assert vmap.stats()["dropped_full"] == 0 and vmap.prune_stats()["n_lost"] == 0
    finally:
        runner.close()
    # with refine the prune is about the REFINED chain's row, the one that fed the insert
    rmap = VoxelMap(**MAP_ARGS)
    refined = inference.OdometryRunner(net, voxel_map=rmap, refine=dict(iters=1), local_map=dict(radius=30.0, every=1))
    try:
        assert refined.local_map == dict(radius=30.0, every=1, min_hits=1, grace=0)
        stream(refined, scans[:2])
        traj2 = refined.refined_trajectory().cpu().numpy()
        assert traj2[1].tobytes() != refined.trajectory().cpu().numpy()[1].tobytes()      # the two chains differ
        ref = VoxelMapRef(MAP_ARGS["voxel_size"], MAP_ARGS["min_range"], MAP_ARGS["max_range"])
        for s, pose in zip(scans[:2], traj2):
            ref.insert(s.cpu().numpy(), pose)
            ref.prune(pose, 30.0)
        assert ref.prune_stats()["n_evicted"] > 1000
        _assert_same(rmap, ref, "runner, refine + local map")
    finally:
        refined.close()
