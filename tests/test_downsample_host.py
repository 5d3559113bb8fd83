"""The float64 restatement of the voxel down-sample rules (rslo_amd/downsample.py, the arbiter of the kernel's tests)
and the KITTI directory parsers of rslo_amd/rawstore.py.  No GPU needed."""
import os

import numpy as np
import pytest

import rslo_amd  # noqa: F401
from rslo_amd.downsample import hier_name, voxel_down_sample_ref


def test_hand_case():
    xyz = np.array([[0.0, 0, 0], [0.04, 0, 0], [0.06, 0, 0]], np.float32)
    rows, vop, npts = voxel_down_sample_ref(xyz, None, 0.1)
    # vmin = -0.05: cells 0, 0, 1
    assert vop.tolist() == [0, 0, 1] and npts.tolist() == [2, 1]
    assert rows.dtype == np.float32 and rows.shape == (2, 3)
    want = np.array([[(np.float64(np.float32(0.0)) + np.float64(np.float32(0.04))) / 2.0, 0, 0],
                     [np.float64(np.float32(0.06)), 0, 0]]).astype(np.float32)
    assert np.array_equal(rows.view(np.int32), want.view(np.int32))
    assert np.allclose(rows, [[0.02, 0, 0], [0.06, 0, 0]], rtol=0, atol=1e-8)


def test_invalid_points_are_dropped():
    xyz = np.array([[0.0, 0, 0], [np.nan, 0, 0], [0.04, 0, 0], [0, np.inf, 0], [0.06, 0, 0], [0, 0, -np.inf]], np.float32)
    rows, vop, npts = voxel_down_sample_ref(xyz, None, 0.1)
    assert vop.tolist() == [0, -1, 0, -1, 1, -1] and npts.tolist() == [2, 1] and rows.shape == (2, 3)
    allbad = np.full((5, 3), np.nan, np.float32)
    rows, vop, npts = voxel_down_sample_ref(allbad, np.zeros((5, 3), np.float32), 0.1)
    assert rows.shape == (0, 6) and (vop == -1).all() and npts.shape == (0,)
    rows, vop, npts = voxel_down_sample_ref(np.zeros((0, 3), np.float32), None, 0.1)
    assert rows.shape == (0, 3) and vop.shape == (0,)


def test_normal_mean_is_not_renormalised():
    xyz = np.array([[0.0, 0, 0], [0.01, 0, 0]], np.float32)
    nrm = np.array([[1.0, 0, 0], [0, 1.0, 0]], np.float32)
    rows, _, npts = voxel_down_sample_ref(xyz, nrm, 0.1)
    assert npts.tolist() == [2] and rows.shape == (1, 6)
    assert rows[0, 3:].tolist() == [0.5, 0.5, 0.0]          # norm 0.707, left as it is


def test_rows_come_in_ascending_cell_order():
    rng = np.random.default_rng(0)
    xyz = (rng.random((500, 3)) * 3.0 - 1.0).astype(np.float32)
    rows, vop, npts = voxel_down_sample_ref(xyz, None, 0.5)
    vmin = xyz.astype(np.float64).min(0) - 0.25
    cell = np.floor((xyz.astype(np.float64) - vmin) / 0.5).astype(np.int64)
    cells = [tuple(cell[np.nonzero(vop == r)[0][0]]) for r in range(len(rows))]
    assert cells == sorted(set(map(tuple, cell))) and len(cells) > 50
    assert npts.sum() == 500 and (np.bincount(vop) == npts).all()
    # sums in ascending input index, one double add at a time
    r = int(np.argmax(npts))
    acc = np.zeros(3)
    for i in np.nonzero(vop == r)[0]:
        acc = acc + xyz[i].astype(np.float64)
    assert npts[r] >= 3 and np.array_equal(rows[r], (acc / float(npts[r])).astype(np.float32))


def test_permuting_the_input_keeps_cells_and_counts():
    rng = np.random.default_rng(1)
    xyz = (rng.random((400, 3)) * 2.0).astype(np.float32)
    rows, vop, npts = voxel_down_sample_ref(xyz, None, 0.25)
    perm = rng.permutation(400)
    rows_p, vop_p, npts_p = voxel_down_sample_ref(xyz[perm], None, 0.25)
    assert np.array_equal(npts, npts_p) and np.array_equal(vop[perm], vop_p)
    assert np.allclose(rows, rows_p, rtol=0, atol=1e-6)      # the order of the adds moves the last bit at most


def test_overflow_raises():
    xyz = np.array([[-150.0, 0, 0], [150.0, 0, 0]], np.float32)
    with pytest.raises(ValueError, match="2\\^21"):
        voxel_down_sample_ref(xyz, None, 1e-4)          # 3e6 cells >= 2^21
    rows, _, _ = voxel_down_sample_ref(xyz, None, 2e-4)  # 1.5e6 cells fit
    assert rows.shape == (2, 3)
    with pytest.raises(ValueError):
        voxel_down_sample_ref(xyz, None, 0.0)


def test_dataset_names():
    assert [hier_name(s) for s in (0.1, 0.2, 0.4, 0.8)] == ["hier_lidar_points_normals_0.1", "hier_lidar_points_normals_0.2",
                                                            "hier_lidar_points_normals_0.4", "hier_lidar_points_normals_0.8"]
    from rslo.data.kitti_dataset_hdf5 import RAGGED
    assert hier_name(0.1) in RAGGED


def test_read_kitti_sequence(tmp_path):
    from rslo_amd import rawstore
    vel = tmp_path / "sequences" / "00" / "velodyne"
    vel.mkdir(parents=True)
    (tmp_path / "poses").mkdir()
    rng = np.random.default_rng(2)
    for name in ("000001.bin", "000000.bin"):
        rng.random((5, 4)).astype(np.float32).tofile(str(vel / name))
    calib = rng.random((5, 12)).astype(np.float32)          # %.9e round-trips an fp32 value exactly
    with open(tmp_path / "sequences" / "00" / "calib.txt", "w") as f:
        for label, row in zip(("P0:", "P1:", "P2:", "P3:", "Tr:"), calib):
            f.write(label + " " + " ".join("%.9e" % v for v in row) + "\n")
    poses = rng.random((2, 12)).astype(np.float32)
    with open(tmp_path / "poses" / "00.txt", "w") as f:
        for row in poses:
            f.write(" ".join("%.9e" % v for v in row) + "\n")
    paths, got_poses, got_calib = rawstore.read_kitti_sequence(str(tmp_path), "00")
    assert [os.path.basename(p) for p in paths] == ["000000.bin", "000001.bin"]
    assert got_poses.shape == (2, 3, 4) and got_poses.dtype == np.float32
    assert np.array_equal(got_poses, poses.reshape(2, 3, 4))
    assert sorted(got_calib) == ["P0", "P1", "P2", "P3", "Tr_velo_to_cam"]
    for k, row in zip(("P0", "P1", "P2", "P3", "Tr_velo_to_cam"), calib):
        assert got_calib[k].shape == (3, 4) and np.array_equal(got_calib[k], row.reshape(3, 4))
    # no pose file (the test sequences): zeros
    os.remove(tmp_path / "poses" / "00.txt")
    _, zero_poses, _ = rawstore.read_kitti_sequence(str(tmp_path), "00")
    assert zero_poses.shape == (2, 3, 4) and (zero_poses == 0).all()
