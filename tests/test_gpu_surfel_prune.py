"""Rolling local surfel map on the GPU (rslo_surfel_prune in csrc/surfel.hip, SurfelMap.prune) against SurfelMapRef.prune
on the same inputs, and the surfel map an OdometryRunner keeps with local_map=dict(..., surfels=...).

The bar is that of tests/test_gpu_surfels.py and tests/test_gpu_local_map.py: after sorting by key, keys, moments
(int64), rows (float64 viewed as int64), the seven counters and the three prune counters are EQUAL, with no tolerance:
the keep / evict rule is a fixed sequence of IEEE double operations on integers unpacked from the key plus integer
comparisons, and a kept cell is copied, not derived again.  The rebuild loses no cell (n_lost == 0) whenever the
survivors' longest run of occupied slots is below the probe limit of 128; every test that leans on it asserts that
first, with the numpy restatement of the map's hash (tests/test_gpu_local_map.py) on the reference's surviving keys.
"""
import numpy as np
import pytest
import torch
from stream_support import dev, network_and_scans, stream
from test_gpu_local_map import CENTER, IDENT, POSE_BACK, POSE_FULL, POSE_YAW, PROBE, _cloud, _longest_run, _occupied
from test_gpu_surfels import SENTINEL, _same_nearest, got_of
from test_gpu_surfels import assert_same as assert_same_table
from test_surfel_prune_host import KS, key_of, row_of_cells

pytestmark = pytest.mark.gpu

HDR = 256 // 8                      # the header in int64 words
HDR_USED = 18                       # of which these are defined: the rest is whatever the allocation held
KEY_NONE = -1                       # MAP_KEY_NONE, all bits set, as int64
THREE = ((0, IDENT), (5, POSE_YAW), (7, POSE_FULL))


def _fits(keys, capacity):
    """the precondition of n_lost == 0: the longest run of occupied slots of these keys, wrap-around included"""
    run = _longest_run(_occupied(keys, capacity))
    assert run < PROBE, "longest run %d" % run
    return run


def _sections(smap):
    """(keys [cap], moments [cap, 10], rows [cap, 8] as int64, dirty [cap] int32) of the raw table, on the host"""
    cap, raw = smap.capacity, smap._buf.cpu().numpy()
    body = raw[HDR:]
    return (body[:cap], body[cap:11 * cap].reshape(cap, 10), body[11 * cap:19 * cap].reshape(cap, 8),
            body[19 * cap:].view(np.int32))


def assert_same(smap, ref, label=""):
    assert_same_table(smap, ref, label)
    ps, rps = smap.prune_stats(), ref.prune_stats()
    print("%s: prune %s" % (label, ps))
    assert ps == rps
    assert not _sections(smap)[3].any()                     # all dirty words are 0 between two calls


def _pair(voxel, capacity, scans, **kw):
    """(SurfelMap, SurfelMapRef) filled with scans = ((seed or cloud, pose), ...)"""
    from rslo_amd.surfels import SurfelMap, SurfelMapRef
    smap, ref = SurfelMap(voxel, capacity, **kw), SurfelMapRef(voxel, **kw)
    for cloud, pose in scans:
        cloud = _cloud(cloud) if isinstance(cloud, int) else cloud
        smap.insert(dev(cloud), pose)
        ref.insert(cloud, pose)
    return smap, ref


def _both(smap, ref, center=None, *args, **kw):
    """the same prune on the device map and on the reference; a centre goes to the device as it is given"""
    smap.prune(center, *args, **kw)
    ref.prune(center.cpu().numpy() if torch.is_tensor(center) else center, *args, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_survivor_counts(K):
    """1000 planar cells in a row along x (tests/test_surfel_prune_host.py): exactly the K nearest the origin survive.
    Their slots are scattered over the 4096-slot table, so the kept ones cross lanes, waves and workgroups of the
    wave-aggregated cursor; 0, 1, 63, 64, 65 kept cells are its own boundaries."""
    voxel, pts = 0.5, row_of_cells()
    smap, ref = _pair(voxel, 4096, ((pts, IDENT),))
    assert ref.stats()["n_cells"] == 1000 == ref.stats()["n_planar"]
    _fits(ref.keys, 4096)
    _both(smap, ref, torch.zeros(3, dtype=torch.float64, device="cuda"), K * voxel)
    _fits(ref.keys, 4096)
    assert ref.stats()["n_cells"] == K and ref.prune_stats() == {"n_prunes": 1, "n_evicted": 1000 - K, "n_lost": 0}
    assert_same(smap, ref, "K %d" % K)
    assert (got_of(smap)[0] == key_of(np.arange(K), 0, 0)).all() and smap.stats()["n_planar"] == K
    # the cell centres as queries, within a quarter of a cell: each finds its own cell if that was kept, else nothing
    wk = _same_nearest(smap, ref, pts[:1000], IDENT, "K %d" % K, max_dist=0.5 * voxel)
    assert (wk[:K] == key_of(np.arange(K), 0, 0)).all() and (wk[K:] == -1).all()


def test_minimum_table_with_wrap_around():
    cloud = _cloud(5, 1000)
    smap, ref = _pair(1.0, 1024, ((cloud, IDENT),))
    center, radius, inner, min_count = np.array([2.0, 1.0, 0.0]), 12.0, 6.0, 2
    n0 = len(ref.keys)
    assert 560 <= n0 <= 614 and _fits(ref.keys, 1024) and smap.stats()["dropped_full"] == 0
    _both(smap, ref, center, radius, inner, min_count)
    occ = _occupied(ref.keys, 1024)
    print("cells %d, survivors %d (longest run %d), slots 1023 and 0 occupied: %s" % (
        n0, len(ref.keys), _fits(ref.keys, 1024), bool(occ[1023] and occ[0])))
    assert 100 < len(ref.keys) < n0 - 200 and occ[1023] and occ[0]      # a surviving run crosses the end of the table
    assert smap.prune_stats()["n_lost"] == 0
    assert_same(smap, ref, "capacity 1024")
    _same_nearest(smap, ref, cloud, IDENT, "capacity 1024")


def test_capacity_beyond_one_grid_stride():
    """The slot loops launch at most 2048 workgroups of 256 threads, one slot per thread and round -- the scan pass at
    most 256 workgroups, 2048 slots per workgroup and round: both strides are 2^19 slots, so 2^20 slots give every
    thread two rounds, and the cells of one small cloud lie scattered over both halves of the table."""
    smap, ref = _pair(2.0, 1 << 20, ((0, POSE_YAW),))
    slots = np.flatnonzero(_sections(smap)[0] != KEY_NONE)
    assert (slots < (1 << 19)).sum() > 100 and (slots >= (1 << 19)).sum() > 100
    _both(smap, ref, dev(CENTER), 11.0, 6.0, 6)
    _fits(ref.keys, 1 << 20)
    assert 20 < len(ref.keys) < ref.prune_stats()["n_evicted"] and ref.stats()["n_planar"] > 10
    assert_same(smap, ref, "2^20 slots")
    slots = np.flatnonzero(_sections(smap)[0] != KEY_NONE)
    assert (slots < (1 << 19)).sum() > 5 and (slots >= (1 << 19)).sum() > 5


@pytest.mark.parametrize("min_count", [1, 3, 5])
def test_three_rotated_scans(min_count):
    smap, ref = _pair(0.4, 1 << 14, THREE)
    assert ref.min_points == 5 and smap.stats()["dropped_full"] == 0
    n0, planar0 = len(ref.keys), ref.stats()["n_planar"]
    _fits(ref.keys, 1 << 14)
    assert_same(smap, ref, "three scans")
    _both(smap, ref, dev(CENTER), 9.0, 5.0, min_count)
    _fits(ref.keys, 1 << 14)
    assert 500 < len(ref.keys) < n0 - 500 and 0 < ref.stats()["n_planar"] < planar0
    assert_same(smap, ref, "three scans, min_count %d" % min_count)
    rows = got_of(smap, min_flag=2)[2]
    assert smap.stats()["n_planar"] == len(rows) and (rows[:, 7] == 2.0).all()
    _same_nearest(smap, ref, _cloud(9), POSE_YAW, "after the prune")


def test_prune_insert_prune():
    smap, ref = _pair(2.0, 1 << 12, ((0, IDENT), (5, POSE_YAW)))
    _both(smap, ref, CENTER, 8.0)
    _fits(ref.keys, 1 << 12)
    assert_same(smap, ref, "two scans, pruned")
    kept = ref.keys.copy()
    third = _cloud(7)
    smap.insert(dev(third), POSE_BACK)
    ref.insert(third, POSE_BACK)
    assert len(np.setdiff1d(ref.keys, kept)) > 50           # cells that start from zero, evicted ones among them
    assert_same(smap, ref, "third scan after the prune")
    _same_nearest(smap, ref, _cloud(9), POSE_YAW, "after the third scan")
    _both(smap, ref, dev(POSE_BACK), 10.0, 4.0, 8)          # about a pose row on the device, with the sparse rule
    _fits(ref.keys, 1 << 12)
    assert ref.prune_stats()["n_prunes"] == 2 and 20 < ref.stats()["n_cells"] and ref.stats()["n_planar"] > 10
    assert_same(smap, ref, "second prune")
    smap.reset()
    assert smap.prune_stats() == {"n_prunes": 0, "n_evicted": 0, "n_lost": 0} and set(smap.stats().values()) == {0}


def test_without_a_centre():
    smap, ref = _pair(0.4, 1 << 14, THREE)
    sparse = int((ref.moments[:, 0] < 3).sum())
    assert 1000 < sparse < len(ref.keys) - 500
    _both(smap, ref, min_count=3)
    _fits(ref.keys, 1 << 14)
    assert ref.prune_stats()["n_evicted"] == sparse
    assert_same(smap, ref, "min_count 3, no centre")
    before = smap._buf.clone()
    smap.prune(None, 1.0, 0.5, 3)                           # the radii are ignored without a centre: nothing more goes
    assert torch.equal(smap._buf[HDR:], before[HDR:]) and smap.prune_stats()["n_evicted"] == sparse


def test_nothing_evicted_leaves_the_allocation_alone():
    smap, ref = _pair(0.4, 1 << 14, ((0, IDENT), (5, POSE_YAW)))
    before = smap._buf.clone()
    calls = (dict(), dict(center=CENTER, radius=float("inf")), dict(center=dev(POSE_YAW), radius=float("inf"), min_count=1),
             dict(center=dev(CENTER), radius=1.0e4, inner_radius=1.0e4, min_count=10 ** 6))
    for n, kw in enumerate(calls):
        _both(smap, ref, **kw)
        changed = torch.nonzero(smap._buf != before).flatten().tolist()
        assert changed == [15]                              # n_prunes and nothing else in the whole allocation
        assert smap.prune_stats() == {"n_prunes": n + 1, "n_evicted": 0, "n_lost": 0}
    assert_same(smap, ref, "nothing evicted")


@pytest.mark.parametrize("how", ["radius 0", "NaN centre"])
def test_everything_evicted_is_a_reset_table(how):
    from rslo_amd.surfels import SurfelMap
    smap, ref = _pair(0.4, 1 << 12, ((0, IDENT),))
    n = len(ref.keys)
    assert smap.stats()["dropped_full"] == 0
    if how == "radius 0":
        _both(smap, ref, dev(CENTER), 0.0)
    else:
        _both(smap, ref, dev(np.array([1.0, np.nan, 0.0])), float("inf"), min_count=2)
    assert ref.prune_stats() == {"n_prunes": 1, "n_evicted": n, "n_lost": 0} and ref.stats()["n_cells"] == 0
    assert_same(smap, ref, how)
    keys, mom, rows, dirty = _sections(smap)
    assert (keys == KEY_NONE).all() and not mom.any() and not rows.any() and not dirty.any()
    assert torch.equal(smap._buf[HDR:], SurfelMap(0.4, 1 << 12)._buf[HDR:])
    smap.insert(dev(_cloud(5)), POSE_YAW)                   # and the map lives on
    ref.insert(_cloud(5), POSE_YAW)
    assert_same(smap, ref, how + ", next scan")


def test_full_table_accounting():
    """1024 slots for 2947 cells: the table is full, which cells it holds is open, and a rebuild may lose records.
    Accounting only: n_cells == kept - n_lost == the number of exported cells, and every surviving cell is, to the bit,
    the cell of that key before the call."""
    from rslo_amd.surfels import SurfelMap
    smap = SurfelMap(0.4, 1024)
    smap.insert(dev(_cloud(0)), IDENT)
    st0 = smap.stats()
    keys0, mom0, rows0 = got_of(smap)
    assert st0["dropped_full"] > 0 and st0["n_cells"] == len(keys0) > 900
    before = smap._buf.clone()
    smap.prune(dev(CENTER), float("inf"))                   # keeps everything: no rebuild, nothing can be lost
    assert torch.nonzero(smap._buf != before).flatten().tolist() == [15]
    cell = np.stack([(keys0 >> 42) & 0x1fffff, (keys0 >> 21) & 0x1fffff, keys0 & 0x1fffff], axis=1) - (1 << 20)
    d = (cell.astype(np.float64) + 0.5) * 0.4 - CENTER[None, :]
    d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    radius = float(np.sqrt(np.sort(d2)[-20]))               # about twenty cells go, the table stays crowded
    kept = int((d2 < radius * radius).sum())
    assert len(keys0) - 40 < kept < len(keys0)
    smap.prune(dev(CENTER), radius)
    st, ps = smap.stats(), smap.prune_stats()
    keys, mom, rows = got_of(smap)
    print("full table: %d cells, %d kept by the rule, prune %s" % (len(keys0), kept, ps))
    assert ps["n_prunes"] == 2 and ps["n_evicted"] == len(keys0) - kept
    assert st["n_cells"] == kept - ps["n_lost"] == len(keys) and len(set(keys.tolist())) == len(keys)
    assert st == dict(st0, n_cells=len(keys), n_planar=int((rows[:, 7] == 2.0).sum()))
    at = np.searchsorted(keys0, keys)
    assert (keys0[at] == keys).all() and (d2[at] < radius * radius).all()
    assert mom.tobytes() == mom0[at].tobytes() and rows.tobytes() == rows0[at].tobytes()
    assert not _sections(smap)[3].any()


def test_argument_errors_write_nothing():
    from rslo_amd import capi
    lib = capi.lib()
    assert lib.rslo_surfel_prune_ws_bytes(1024) == 256 + 152 * 1024 and lib.rslo_surfel_prune_ws_bytes(1000) == 0
    assert lib.rslo_surfel_prune_ws_bytes(512) == 0 and lib.rslo_surfel_prune_ws_bytes(1 << 32) == 0
    assert capi.SURFEL_HDR_PRUNE == 15
    smap, ref = _pair(0.4, 2048, ((_cloud(0)[:1000], IDENT),))
    smap.reserve_prune()
    ws = smap._prune_ws
    ws.fill_(SENTINEL)
    before = smap._buf.clone()
    buf, c = smap._buf, dev(CENTER)
    nb, wb = buf.numel() * 8, ws.numel() * 8
    assert wb == lib.rslo_surfel_prune_ws_bytes(2048)
    nan = float("nan")

    def call(map_ptr=buf.data_ptr(), map_bytes=nb, center=c.data_ptr(), radius=5.0, inner=2.0, min_count=1,
             ws_ptr=ws.data_ptr(), ws_bytes=wb):
        return lib.rslo_surfel_prune(map_ptr, map_bytes, center, radius, inner, min_count, ws_ptr, ws_bytes, None)
    einval = [call(map_ptr=None), call(map_bytes=capi.surfel_bytes(1024) - 8), call(radius=-1.0), call(radius=nan),
              call(inner=-0.5), call(inner=nan), call(inner=5.5), call(min_count=0), call(min_count=-2),
              call(ws_ptr=None), call(ws_ptr=ws.data_ptr() + 8, ws_bytes=wb - 8)]
    ews = [call(ws_bytes=wb - 16), call(ws_bytes=0)]
    print("return codes:", einval, ews, lib.rslo_last_error().decode())
    assert einval == [-1] * len(einval) and ews == [-4] * len(ews)      # RSLO_EINVAL, RSLO_EWS
    for kw in (dict(center=CENTER), dict(center=CENTER, radius=-1.0), dict(center=CENTER, radius=nan),
               dict(center=CENTER, radius=5.0, inner_radius=6.0), dict(center=CENTER, radius=5.0, inner_radius=nan),
               dict(min_count=0)):
        with pytest.raises(ValueError):
            smap.prune(**kw)
    with pytest.raises(capi.RsloHipError):
        smap.prune(torch.zeros(3, dtype=torch.float64, device="cuda")[:2], 1.0)
    with pytest.raises(capi.RsloHipError):
        capi.surfel_prune_ws(1000, "cuda")
    torch.cuda.synchronize()
    assert torch.equal(smap._buf, before) and bool((ws == SENTINEL).all())
    assert_same(smap, ref, "after refused calls")
    # without a centre the radii are not looked at
    assert call(center=None, radius=nan, inner=-1.0) == 0
    torch.cuda.synchronize()
    assert torch.nonzero(smap._buf != before).flatten().tolist() == [15]


def test_never_reset_allocation():
    from rslo_amd import capi
    raw = torch.full((capi.surfel_bytes(1024) // 8,), SENTINEL, dtype=torch.int64, device="cuda")
    ws = capi.surfel_prune_ws(1024, "cuda")
    capi.surfel_prune(raw, ws, dev(CENTER), 3.0, 1.0, 2)
    capi.surfel_prune(raw, ws)
    torch.cuda.synchronize()
    assert bool((raw == SENTINEL).all())


def test_determinism():
    first = None
    for _ in range(2):
        smap, _ = _pair(2.0, 1 << 12, ((0, IDENT), (5, POSE_YAW)))
        smap.prune(CENTER, 8.0)
        smap.insert(dev(_cloud(7)), POSE_BACK)
        smap.prune(dev(POSE_BACK), 10.0, 4.0, 8)
        got = got_of(smap), smap.stats(), smap.prune_stats(), smap._buf[:HDR_USED].cpu().numpy().tobytes()
        assert len(got[0][0]) > 20 and got[2]["n_prunes"] == 2 and got[2]["n_lost"] == 0
        if first is not None:
            assert all(a.tobytes() == b.tobytes() for a, b in zip(first[0], got[0])) and first[1:] == got[1:]
        first = got


def test_capture_and_replay():
    """insert + prune captured once on one stream; replayed with two scans and two centres copied into the static
    tensors, it gives the eager bits: the launch count does not depend on the data and nothing reads the host."""
    from rslo_amd.surfels import SurfelMap, SurfelMapRef
    clouds = [_cloud(0)[:, :4], _cloud(5)[:, :4]]
    poses = [IDENT, POSE_YAW]
    args = (9.0, 5.0, 3)
    warm = SurfelMap(0.4, 1 << 14)                  # the kernels' first launches, outside the capture
    warm.insert(dev(clouds[0]), IDENT)
    warm.prune(dev(IDENT), *args)
    smap, ref, eager = SurfelMap(0.4, 1 << 14), SurfelMapRef(0.4), SurfelMap(0.4, 1 << 14)
    for m in (smap, eager):                         # every workspace now: the loop below must allocate nothing
        m.reserve(len(clouds[0]))
        m.reserve_prune()
    static_pts = torch.zeros((len(clouds[0]), 4), dtype=torch.float32, device="cuda")
    static_pose = torch.zeros(7, dtype=torch.float64, device="cuda")
    on_dev = [(dev(c), dev(p)) for c, p in zip(clouds, poses)]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        smap.insert(static_pts, static_pose)
        smap.prune(static_pose, *args)              # the centre is the pose row's translation, read in place
    assert smap.stats()["n_scans"] == 0 and smap.prune_stats()["n_prunes"] == 0      # captured, not run
    torch.cuda.synchronize()
    mem = torch.cuda.memory_allocated()
    for k, (c, p) in enumerate(on_dev):
        static_pts.copy_(c)
        static_pose.copy_(p)
        g.replay()
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == mem
        ref.insert(clouds[k], poses[k])
        ref.prune(poses[k], *args)
        _fits(ref.keys, 1 << 14)
        assert ref.prune_stats()["n_evicted"] > 1000 * (k + 1) and ref.stats()["n_cells"] > 100
        assert_same(smap, ref, "replay %d" % k)
        eager.insert(c, p)
        eager.prune(p, *args)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got_of(smap), got_of(eager)))
        assert torch.equal(smap._buf[:HDR_USED], eager._buf[:HDR_USED])


# ---------------------------------------------------------------------------------------------------------------------
# the runner's local surfel map
# ---------------------------------------------------------------------------------------------------------------------
N_SCANS = 4
SURF_ARGS = dict(voxel_size=0.4, capacity=1 << 18, min_range=2.5, max_range=80.0)
MAP_ARGS = dict(voxel_size=0.2, capacity=1 << 21, min_range=2.5, max_range=80.0)
LOCAL = dict(radius=30.0, every=2, surfels=dict(min_count=2, inner_radius=15.0))


@pytest.fixture(scope="module")
def odom():
    return network_and_scans(21, 3, N_SCANS)


def _ref_of(scans, traj, every=2):
    from rslo_amd.surfels import SurfelMapRef
    ref = SurfelMapRef(**{k: v for k, v in SURF_ARGS.items() if k != "capacity"})
    for n, (s, pose) in enumerate(zip(scans, traj)):
        ref.insert(s.cpu().numpy(), pose)
        if (n + 1) % every == 0:
            ref.prune(pose, LOCAL["radius"], LOCAL["surfels"]["inner_radius"], LOCAL["surfels"]["min_count"])
    return ref


def test_runner_keeps_a_local_surfel_map(odom):
    from rslo_amd import inference
    from rslo_amd.surfels import SurfelMap
    net, scans = odom
    plain = inference.OdometryRunner(net)
    try:
        rel0, traj0 = stream(plain, scans)
    finally:
        plain.close()
    smap = SurfelMap(**SURF_ARGS)
    runner = inference.OdometryRunner(net, surfels=smap, local_map=LOCAL)      # no voxel_map is needed with the key
    try:
        assert smap._prune_ws is not None                       # reserved by the constructor
        assert runner.local_map == dict(radius=30.0, every=2, min_hits=1, grace=0, surfels=dict(min_count=2, inner_radius=15.0))
        rel, traj = stream(runner, scans)
        assert rel.tobytes() == rel0.tobytes() and traj.tobytes() == traj0.tobytes()      # the prune disturbs nothing
        ref = _ref_of(scans, traj)
        _fits(ref.keys, SURF_ARGS["capacity"])
        assert ref.prune_stats()["n_prunes"] == 2 and ref.prune_stats()["n_evicted"] > 0
        assert ref.stats()["n_cells"] > 1000 and ref.stats()["n_planar"] > 100
        assert_same(smap, ref, "runner, local surfel map")
        assert smap.stats()["dropped_full"] == 0 and smap.prune_stats()["n_lost"] == 0
        runner.reset()
        assert smap.prune_stats() == {"n_prunes": 0, "n_evicted": 0, "n_lost": 0}
    finally:
        runner.close()


def test_runner_prunes_about_the_refined_row(odom):
    """with voxel_map= and refine= the centre is the REFINED chain's row, the one that fed both inserts; the voxel map
    is pruned as before"""
    from rslo_amd import inference
    from rslo_amd.mapping import VoxelMap, VoxelMapRef
    from rslo_amd.surfels import SurfelMap
    net, scans = odom
    smap, vmap = SurfelMap(**SURF_ARGS), VoxelMap(**MAP_ARGS)
    runner = inference.OdometryRunner(net, voxel_map=vmap, refine=dict(iters=1), surfels=smap, local_map=LOCAL)
    try:
        assert smap._prune_ws is not None and vmap._prune_ws is not None
        stream(runner, scans)
        traj2 = runner.refined_trajectory().cpu().numpy()
        assert traj2[1].tobytes() != runner.trajectory().cpu().numpy()[1].tobytes()      # the two chains differ
        ref = _ref_of(scans, traj2)
        _fits(ref.keys, SURF_ARGS["capacity"])
        assert ref.prune_stats()["n_prunes"] == 2 and ref.prune_stats()["n_evicted"] > 0
        assert_same(smap, ref, "runner, refine + local surfel map")
        vref = VoxelMapRef(MAP_ARGS["voxel_size"], MAP_ARGS["min_range"], MAP_ARGS["max_range"])
        for n, (s, pose) in enumerate(zip(scans, traj2)):
            vref.insert(s.cpu().numpy(), pose)
            if (n + 1) % 2 == 0:
                vref.prune(pose, 30.0)
        assert vmap.stats() == vref.stats() and vmap.prune_stats() == vref.prune_stats()
    finally:
        runner.close()


def test_runner_without_the_key_and_construction_errors(odom):
    from rslo_amd import capi, inference
    from rslo_amd.mapping import VoxelMap
    from rslo_amd.surfels import SurfelMap
    net, scans = odom
    smap, vmap = SurfelMap(**SURF_ARGS), VoxelMap(**MAP_ARGS)
    runner = inference.OdometryRunner(net, voxel_map=vmap, surfels=smap, local_map=dict(radius=30.0, every=2))
    try:
        assert runner.local_map == dict(radius=30.0, every=2, min_hits=1, grace=0)      # today's four keys
        assert smap._prune_ws is None
        stream(runner, scans[:2])
        assert smap.prune_stats()["n_prunes"] == 0 and vmap.prune_stats()["n_prunes"] == 1
        assert smap.stats()["n_scans"] == 2
    finally:
        runner.close()
    with pytest.raises(capi.RsloHipError):
        inference.OdometryRunner(net, voxel_map=vmap, local_map=LOCAL)                 # the key without surfels=
    with pytest.raises(capi.RsloHipError):
        inference.OdometryRunner(net, surfels=smap, local_map=dict(radius=30.0))       # no key: a voxel_map is needed
    with pytest.raises(capi.RsloHipError):
        inference.OdometryRunner(net, surfels=smap, local_map=dict(radius=30.0, surfels=dict(min_cnt=2)))
    for bad in (dict(inner_radius=31.0), dict(inner_radius=-1.0), dict(min_count=0)):
        with pytest.raises((capi.RsloHipError, ValueError)):
            inference.OdometryRunner(net, surfels=smap, local_map=dict(radius=30.0, surfels=bad))
    ok = inference.OdometryRunner(net, surfels=smap, local_map=dict(radius=30.0, surfels=True))
    try:
        assert ok.local_map == dict(radius=30.0, every=1, min_hits=1, grace=0, surfels=dict(min_count=1, inner_radius=30.0))
    finally:
        ok.close()
