"""Voxel down-sample on the GPU (csrc/downsample.hip) against the float64 restatement rslo_amd/downsample.py run on the
same fp32 inputs, and the store builder rslo_amd/rawstore.py read back through KittiDatasetHDF5.

The bar is BIT equality, with no tolerance and no excluded point: the cell index and the means are IEEE double
operations on exactly-converted fp32 inputs in a fixed order (ascending input index), rounded once to fp32.  It follows
from the formats, not from what the kernel returns.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_CLOUD = {}
_REF = {}


def _dense_far_patch():
    """the 3 000-point patch at (60, -30, 1) of tests/test_gpu_normals.py (plus 64 repeated points), seeded normals"""
    rng = np.random.default_rng(11)
    u = rng.random((3000, 2)) * 0.5 - 0.25
    z = 0.4 * u[:, 0] - 0.25 * u[:, 1] + rng.normal(0, 1e-3, 3000)
    xyz = (np.stack([u[:, 0], u[:, 1], z], 1) + np.array([60.0, -30.0, 1.0])).astype(np.float32)
    xyz = np.concatenate([xyz, xyz[:64]], 0)
    nrm = rng.normal(size=(len(xyz), 3)).astype(np.float32)
    return xyz, nrm


def _cloud(name):
    """(xyz [P, 3], normals [P, 3]) fp32, made once"""
    from rslo_amd import synthetic
    if name not in _CLOUD:
        if name == "small":
            c = synthetic.small_cloud(4000, seed=0)
            _CLOUD[name] = (c[:, :3].copy(), c[:, 4:7].copy())
        elif name == "scan":
            c = synthetic.scan(n_az=520, n_el=16)
            _CLOUD[name] = (c[:, :3].copy(), c[:, 4:7].copy())
        elif name == "patch":
            _CLOUD[name] = _dense_far_patch()
        else:
            raise KeyError(name)
    return _CLOUD[name]


def _ref(name, size):
    """float64 reference of a cloud at a size, computed once per session and never modified"""
    from rslo_amd.downsample import voxel_down_sample_ref
    if (name, size) not in _REF:
        xyz, nrm = _cloud(name)
        _REF[(name, size)] = voxel_down_sample_ref(xyz, nrm, size)
    return _REF[(name, size)]


def _run(xyz, nrm, size):
    """(rows, voxel_of_point, npts) of the kernel as numpy arrays"""
    from rslo_amd import capi
    pts = torch.from_numpy(np.ascontiguousarray(xyz)).cuda()
    nr = None if nrm is None else torch.from_numpy(np.ascontiguousarray(nrm)).cuda()
    rows, vop, npts = capi.voxel_downsample(pts, nr, size, index=True, npts=True)
    return rows.cpu().numpy(), vop.cpu().numpy(), npts.cpu().numpy()


def _assert_same(got, ref, label=""):
    rows, vop, npts = got
    rrows, rvop, rnpts = ref
    print("%s: Q kernel %d, reference %d; %d cells with >= 2 points, longest run %d" % (
        label, len(rows), len(rrows), int((rnpts >= 2).sum()), int(rnpts.max()) if len(rnpts) else 0))
    assert rows.shape == rrows.shape and rows.dtype == np.float32
    assert np.array_equal(vop, rvop)
    assert np.array_equal(npts, rnpts)
    assert np.array_equal(rows.view(np.int32), rrows.view(np.int32))


@pytest.mark.parametrize("size", [0.1, 0.4, 2.0])
@pytest.mark.parametrize("name", ["small", "scan", "patch"])
def test_cloud_against_float64(name, size):
    xyz, nrm = _cloud(name)
    ref = _ref(name, size)
    # the reference itself first, so that nothing below passes vacuously
    if size == 0.1 and name in ("small", "scan"):
        assert (ref[2] >= 2).sum() >= 50
    if size == 2.0 and name == "scan":
        assert ref[2].max() > 64
    if name == "patch":          # every size has runs longer than a wave; at 2.0 the whole patch is one cell
        assert ref[2].max() > 64
    assert ref[2].sum() == len(xyz) and (ref[1] >= 0).all()
    got = _run(xyz, nrm, size)
    _assert_same(got, ref, "%s @ %g" % (name, size))
    again = _run(xyz, nrm, size)
    assert np.array_equal(got[0].view(np.int32), again[0].view(np.int32))
    assert np.array_equal(got[1], again[1]) and np.array_equal(got[2], again[2])


@pytest.mark.parametrize("size", [0.1, 10.0])
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 1025])
def test_sizes(N, size):
    """the first N points shrunk to a few cells: single runs cross the lane, wave and block boundaries"""
    from rslo_amd.downsample import voxel_down_sample_ref
    xyz, nrm = _cloud("small")
    xyz = (xyz[:N] * np.float32(0.01)).astype(np.float32)
    nrm = nrm[:N].copy()
    ref = voxel_down_sample_ref(xyz, nrm, size)
    if size == 10.0:
        assert ref[2].tolist() == [N]          # one run of all N
    elif N >= 63:
        assert 2 <= len(ref[0]) <= N // 2
    _assert_same(_run(xyz, nrm, size), ref, "N=%d @ %g" % (N, size))


def test_invalid_points():
    from rslo_amd import capi
    from rslo_amd.downsample import voxel_down_sample_ref
    xyz, nrm = _cloud("small")
    xyz, nrm = xyz[:502].copy(), nrm[:502].copy()
    xyz[100] = (np.nan, 0.0, 0.0)
    xyz[200, 1] = np.inf
    ref = voxel_down_sample_ref(xyz, nrm, 0.4)
    assert ref[1][100] == -1 and ref[1][200] == -1 and (ref[1] >= 0).sum() == 500
    got = _run(xyz, nrm, 0.4)
    assert got[1][100] == -1 and got[1][200] == -1
    _assert_same(got, ref, "nan + inf")
    # nothing valid: Q = 0, no flag, every point -1
    bad = torch.full((300, 3), float("nan"), device="cuda")
    out, vop, npts, counts = capi.voxel_downsample(bad, None, 0.1, index=True, npts=True, sync=False)
    torch.cuda.synchronize()
    assert counts.tolist() == [0, 0] and (vop == -1).all()
    rows = capi.voxel_downsample(bad, None, 0.1)
    assert rows.shape == (0, 3)


def test_empty_cloud_writes_counts_only():
    from rslo_amd import capi
    out = torch.full((4, 6), 7.0, device="cuda")
    vop = torch.full((4,), 7, dtype=torch.int32, device="cuda")
    npts = torch.full((4,), 7, dtype=torch.int32, device="cuda")
    counts = torch.full((2,), 7, dtype=torch.int32, device="cuda")
    ws = torch.empty((capi.lib().rslo_voxel_downsample_ws_bytes(0),), dtype=torch.uint8, device="cuda")
    pts = torch.zeros((4, 7), device="cuda")
    rc = capi.lib().rslo_voxel_downsample(pts.data_ptr(), 7, pts.data_ptr() + 16, 7, 0, ctypes.c_double(0.1),
                                          out.data_ptr(), vop.data_ptr(), npts.data_ptr(), counts.data_ptr(),
                                          ws.data_ptr(), ws.numel(), capi._stream())
    torch.cuda.synchronize()
    assert rc == 0 and counts.tolist() == [0, 0]
    assert (out == 7.0).all() and (vop == 7).all() and (npts == 7).all()
    rows = capi.voxel_downsample(torch.zeros((0, 4), device="cuda"))
    assert rows.shape == (0, 3)
    # argument errors
    for size, stride in ((0.0, 7), (-1.0, 7), (0.1, 2)):
        rc = capi.lib().rslo_voxel_downsample(pts.data_ptr(), stride, None, 0, 4, ctypes.c_double(size), out.data_ptr(),
                                              None, None, counts.data_ptr(), ws.data_ptr(), ws.numel(), capi._stream())
        assert rc != 0
    torch.cuda.synchronize()
    assert (out == 7.0).all()


def test_overflow_is_flagged_on_the_device():
    from rslo_amd import capi
    from rslo_amd.downsample import voxel_down_sample_ref
    xyz = np.zeros((10, 3), np.float32)
    xyz[:, 0] = np.linspace(-150.0, 150.0, 10)
    with pytest.raises(ValueError):
        voxel_down_sample_ref(xyz, None, 1e-4)
    pts = torch.from_numpy(xyz).cuda()
    out = torch.full((10, 3), 7.0, device="cuda")
    _, _, _, counts = capi.voxel_downsample(pts, None, 1e-4, out=out, sync=False)
    torch.cuda.synchronize()
    Q, flags = counts.tolist()
    assert Q == 0 and flags & 1
    assert (out == 7.0).all()
    with pytest.raises(capi.RsloHipError, match="2\\^21"):
        capi.voxel_downsample(pts, None, 1e-4)
    rows = capi.voxel_downsample(pts, None, 2e-4)           # 1.5e6 cells fit
    assert rows.shape == (10, 3)


def test_strided_input():
    from rslo_amd import capi, synthetic
    cloud = torch.from_numpy(synthetic.small_cloud(4000, seed=0)).cuda()
    r7, i7, n7 = capi.voxel_downsample(cloud, cloud[:, 4:7], 0.4, index=True, npts=True)
    r3, i3, n3 = capi.voxel_downsample(cloud[:, :3].contiguous(), cloud[:, 4:7].contiguous(), 0.4, index=True, npts=True)
    assert r7.shape[1] == 6 and 50 < r7.shape[0] < 4000
    assert torch.equal(r7.view(torch.int32), r3.view(torch.int32)) and torch.equal(i7, i3) and torch.equal(n7, n3)
    rx = capi.voxel_downsample(cloud, None, 0.4)
    assert rx.shape == (r7.shape[0], 3) and torch.equal(rx.view(torch.int32), r7[:, :3].contiguous().view(torch.int32))


def test_capture_and_replay():
    from rslo_amd import capi, synthetic
    a = torch.from_numpy(synthetic.small_cloud(4000, seed=0)).cuda()
    b = torch.from_numpy(synthetic.small_cloud(4000, seed=5)).cuda()
    want_a = [t.clone() for t in capi.voxel_downsample(a, a[:, 4:7], 0.4, index=True, npts=True)]
    want_b = [t.clone() for t in capi.voxel_downsample(b, b[:, 4:7], 0.4, index=True, npts=True)]
    assert want_a[0].shape[0] != want_b[0].shape[0]
    buf = a.clone()
    out = torch.zeros((4000, 6), device="cuda")
    vop = torch.zeros((4000,), dtype=torch.int32, device="cuda")
    npts = torch.zeros((4000,), dtype=torch.int32, device="cuda")
    counts = torch.zeros((2,), dtype=torch.int32, device="cuda")
    ws = torch.empty((capi.lib().rslo_voxel_downsample_ws_bytes(4000),), dtype=torch.uint8, device="cuda")
    kw = dict(out=out, index=vop, npts=npts, counts=counts, ws=ws, sync=False)
    capi.voxel_downsample(buf, buf[:, 4:7], 0.4, **kw)       # first launches outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        capi.voxel_downsample(buf, buf[:, 4:7], 0.4, **kw)
    for src, want in ((a, want_a), (b, want_b)):
        buf.copy_(src)
        g.replay()
        torch.cuda.synchronize()
        Q = int(counts[0])
        assert Q == want[0].shape[0] and int(counts[1]) == 0
        assert torch.equal(out[:Q].view(torch.int32), want[0].view(torch.int32))
        assert torch.equal(vop, want[1]) and torch.equal(npts[:Q], want[2])


def test_store_round_trip(tmp_path):
    """raw scans -> rawstore.build_sequence -> KittiDatasetHDF5, as tests/test_reader.py opens a store"""
    from rslo.data.kitti_dataset_hdf5 import GroupStore, KittiDatasetHDF5, cam_pose_to_lidar
    from rslo.utils.geometric import RT_to_tq
    from rslo_amd import capi, rawstore, synthetic
    from rslo_amd.downsample import voxel_down_sample_ref
    scans = [synthetic.sequence_scan(i, n_el=16, n_az=520)[:, :4].copy() for i in range(3)]
    broken = scans[0][:100].copy()
    broken[7, 2] = np.nan
    scans.append(broken)
    poses = np.zeros((4, 3, 4), np.float32)
    for i in range(4):
        c, s = np.cos(0.01 * i), np.sin(0.01 * i)
        poses[i] = [[c, 0, s, 0.1 * i], [0, 1, 0, 0.02 * i], [-s, 0, c, 1.0 * i]]
    tr = np.array([[0, -1, 0, 0.0], [0, 0, -1, -0.08], [1, 0, 0, -0.27]], np.float32)
    calib = {"P%d" % k: np.arange(12, dtype=np.float32).reshape(3, 4) + k for k in range(4)}
    calib["Tr_velo_to_cam"] = tr
    with pytest.warns(UserWarning, match="NaN"):
        stats = rawstore.build_sequence(str(tmp_path), "00", scans, poses, calib, hier_sizes=(0.1, 0.8))
    assert stats["scans"] == 4 and stats["skipped"] == [3]

    store = str(tmp_path)
    ds = KittiDatasetHDF5(store, store, seq_length=2, skip=1, split="eval_train", num_point_features=7)
    assert len(ds) == 4
    r = ds.get_sensor_data(2)
    for k, i in enumerate((1, 2)):
        dev = torch.from_numpy(scans[i]).cuda()
        want = capi.append_normals(dev).cpu().numpy()
        got = np.ascontiguousarray(r["lidar_seq"][k], dtype=np.float32)
        assert got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32))
        raw_n = capi.estimate_normals(dev, zero_vertical=False)[0].cpu().numpy()
        rows, _, _ = voxel_down_sample_ref(scans[i][:, :3], raw_n, 0.1)
        hier = np.ascontiguousarray(r["hier_points_seq"][k][0], dtype=np.float32)
        assert len(rows) > 1000 and hier.shape == rows.shape and np.array_equal(hier.view(np.int32), rows.view(np.int32))
        want_pose = RT_to_tq(cam_pose_to_lidar(poses[i], tr))
        assert np.array_equal(np.asarray(r["pose_seq"][k]), np.asarray(want_pose))
        assert np.array_equal(np.asarray(r["calib/Tr_velo_to_cam"][k]), tr)
    # the other sizes and the fixed-shape datasets, straight from the store
    grp = GroupStore(store)["00"]
    rows8, _, _ = voxel_down_sample_ref(scans[0][:, :3], np.asarray(grp["lidar_normals"][0]).reshape(-1, 3), 0.8)
    got8 = np.asarray(grp["hier_lidar_points_normals_0.8"][0]).reshape(-1, 6)
    assert np.array_equal(got8.view(np.int32), rows8.view(np.int32))
    assert np.array_equal(np.asarray(grp["poses"][:3]), poses[:3])
    for k in range(4):
        assert np.array_equal(np.asarray(grp["calib.P%d" % k][1]), calib["P%d" % k])
    # the scan with a NaN: empty entries, zero pose and calib rows
    for name in ("lidar_points", "lidar_normals", "hier_lidar_points_normals_0.1", "hier_lidar_points_normals_0.8"):
        assert len(grp[name]) == 4 and len(grp[name][3]) == 0 and len(grp[name][2]) > 0
    assert (np.asarray(grp["poses"][3]) == 0).all() and (np.asarray(grp["calib.Tr_velo_to_cam"][3]) == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# past every grid stride: more long runs than k_ds_reduce_long has workgroups, more points than k_ds_min has threads, and
# the instantiations without normals on runs longer than a wave
# ---------------------------------------------------------------------------------------------------------------------
LONG_BLOCKS = 1024           # DS_LONG_BLOCKS of csrc/downsample.hip
MIN_THREADS = 1024 * 256     # the launch cap of k_ds_min


def _long_run_lattice():
    """11 x 10 x 10 cells of 0.4 m with 65 to 70 jittered points each, shuffled; the last point, alone at the origin, pins
    the minimum, so that the cell centres sit at multiples of the voxel size and the jitter (0.3 of a cell) stays inside"""
    if "lattice" not in _CLOUD:
        rng = np.random.default_rng(41)
        centres = np.stack(np.meshgrid(np.arange(1, 12), np.arange(1, 11), np.arange(1, 11), indexing="ij"), -1).reshape(-1, 3)
        per = rng.integers(65, 71, len(centres))
        pts = np.repeat(centres, per, 0) * 0.4 + rng.uniform(-0.12, 0.12, (int(per.sum()), 3))
        pts = pts[rng.permutation(len(pts))]
        xyz = np.concatenate([pts, np.zeros((1, 3))], 0).astype(np.float32)
        _CLOUD["lattice"] = (xyz, rng.normal(size=xyz.shape).astype(np.float32))
    return _CLOUD["lattice"]


def test_more_long_runs_than_workgroups():
    xyz, nrm = _long_run_lattice()
    ref = _ref("lattice", 0.4)
    assert (ref[2] > 64).sum() >= LONG_BLOCKS + 1 and len(xyz) < 90000
    assert ref[2][0] == 1 and ref[2][1:].min() >= 65 and ref[2].max() <= 70
    _assert_same(_run(xyz, nrm, 0.4), ref, "lattice")
    rows, vop, npts = _run(xyz, None, 0.4)
    _assert_same((rows, vop, npts), (np.ascontiguousarray(ref[0][:, :3]), ref[1], ref[2]), "lattice, no normals")


@pytest.mark.parametrize("size", [0.1, 0.4, 2.0])
def test_no_normals_on_long_runs(size):
    from rslo_amd import capi
    xyz, _ = _cloud("patch")
    ref = _ref("patch", size)
    assert ref[2].max() > 64
    want = (np.ascontiguousarray(ref[0][:, :3]), ref[1], ref[2])
    _assert_same(_run(xyz, None, size), want, "patch without normals @ %g" % size)
    rows = capi.voxel_downsample(torch.from_numpy(xyz).cuda(), None, size)           # neither index nor npts
    assert np.array_equal(rows.cpu().numpy().view(np.int32), want[0].view(np.int32))


def test_minimum_past_the_grid_stride():
    """N = 1024 * 256 + 1: k_ds_min strides, and the point only a second trip reaches holds the minimum of all three axes"""
    from rslo_amd.downsample import voxel_down_sample_ref
    N = MIN_THREADS + 1
    rng = np.random.default_rng(43)
    xyz = rng.uniform(0.0, 20.0, (N, 3)).astype(np.float32)
    xyz[-1] = (-0.13, -0.27, -0.31)
    assert (xyz[:-1].min(0) >= 0).all()
    ref = voxel_down_sample_ref(xyz, None, 0.4)
    without = voxel_down_sample_ref(xyz[:-1], None, 0.4)
    assert (ref[1][:-1] != without[1]).all()          # were the last point missed, every other point would move
    _assert_same(_run(xyz, None, 0.4), ref, "N = %d" % N)
