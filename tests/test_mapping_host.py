"""The world voxel map's float64 restatement (rslo_amd/mapping.py VoxelMapRef) on hand-made cells, the pose convention on a
synthetic drive, the host-only size function of the C ABI and the PLY writer.  No GPU needed."""
import numpy as np
import pytest

IDENT = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)


def _pts(*rows):
    return np.array(rows, np.float32).reshape(len(rows), -1)


def _cell_of(ref, point):
    """integer cell (x, y, z) of one accepted point"""
    status, key, _ = ref._cells(_pts(point), IDENT)
    assert status[0] == 0
    k = int(key[0])
    return tuple(((k >> sh) & ((1 << 21) - 1)) - (1 << 20) for sh in (42, 21, 0))


def test_floor_at_negative_coordinates_and_cell_faces():
    from rslo_amd.mapping import VoxelMapRef
    ref = VoxelMapRef(0.1)
    assert _cell_of(ref, (-0.05, 0.05, -0.15)) == (-1, 0, -2)          # floor, not truncation: -0.05 / 0.1 -> -1
    ref = VoxelMapRef(0.5)                                             # 0.5 and the faces below are exact in binary
    assert _cell_of(ref, (0.0, 0.5, -0.5)) == (0, 1, -1)               # a face belongs to the cell above it
    assert _cell_of(ref, (1.0, -1.0, 1.5)) == (2, -2, 3)
    assert _cell_of(ref, (np.nextafter(np.float32(0.5), np.float32(0)), -0.0, np.nextafter(np.float32(-0.5), np.float32(-1)))) \
        == (0, 0, -2)


def test_two_points_in_one_cell_and_two_scans():
    from rslo_amd.mapping import VoxelMapRef
    ref = VoxelMapRef(1.0)
    ref.insert(_pts((0.2, 0.2, 0.2, 0.5), (5.5, 0.1, 0.1, 0.6), (0.7, 0.7, 0.7, 0.9)), IDENT)
    rows, tags, hits = ref.points()
    assert tags.tolist() == [0, 1] and hits.tolist() == [2, 1]         # the lower index owns the row
    assert rows[0].tolist() == [np.float32(0.2)] * 3 + [0.5] and rows.dtype == np.float32
    # scan 1 hits the same cell: the scan-0 row is kept and the hits add up; its other point opens a cell of scan 1
    ref.insert(_pts((0.9, 0.1, 0.3, 0.1), (0.4, 0.4, 0.4, 0.2), (-3.5, 0.5, 0.5, 0.3)), IDENT)
    rows, tags, hits = ref.points()
    assert tags.tolist() == [0, 1, (1 << 32) | 2] and hits.tolist() == [4, 1, 1]
    assert rows[0].tolist() == [np.float32(0.2)] * 3 + [0.5]
    assert rows[2].tolist() == [-3.5, 0.5, 0.5, np.float32(0.3)]
    assert ref.stats() == {"n_scans": 2, "n_cells": 3, "n_points": 6, "dropped_invalid": 0, "dropped_range": 0,
                           "dropped_full": 0}
    assert ref.points(min_hits=2)[1].tolist() == [0]
    assert ref.points(center=(5.0, 0.0, 0.0), radius=1.0)[1].tolist() == [1]
    assert ref.lookup(_pts((0.5, 0.5, 0.5), (9.5, 9.5, 9.5), (np.nan, 0, 0))).tolist() == [4, 0, -1]
    # a [P, 3] input has intensity 0
    ref3 = VoxelMapRef(1.0)
    ref3.insert(_pts((0.2, 0.2, 0.2)), IDENT)
    assert ref3.points()[0][0].tolist() == [np.float32(0.2)] * 3 + [0.0]
    ref.reset()
    assert len(ref.points()[1]) == 0 and ref.stats()["n_scans"] == 0


def test_range_gate_invalid_points_and_cell_limits():
    from rslo_amd.mapping import VoxelMapRef
    ref = VoxelMapRef(1.0, min_range=2.0, max_range=4.0)
    pts = _pts((2.0, 0, 0), (0, np.nextafter(np.float32(2.0), np.float32(0)), 0), (0, 0, 4.0),
               (np.nextafter(np.float32(4.0), np.float32(0)), 0, 0), (np.nan, 3, 0), (3, np.inf, 0), (3, 0, -np.inf), (0, 3.0, 0))
    ref.insert(pts, IDENT)
    st = ref.stats()
    assert ref.lookup(pts, IDENT).tolist() == [1, -1, -1, 1, -1, -1, -1, 1]      # inclusive below, exclusive above
    assert st["n_points"] == 3 and st["dropped_invalid"] == 5 and st["dropped_range"] == 0
    # |cell| = 2^20 - 1 is accepted, 2^20 is dropped (on either side: the rule is on the absolute value)
    ref = VoxelMapRef(1.0)
    lim = float(1 << 20)
    pts = _pts((lim - 0.5, 0, 0), (lim, 0, 0), (0, -(lim - 1.0), 0), (0, -lim, 0), (0, 0, -(lim + 0.5)), (1, 1, 1))
    ref.insert(pts, IDENT)
    st = ref.stats()
    assert ref.lookup(pts, IDENT).tolist() == [1, -1, 1, -1, -1, 1]
    assert st["n_points"] == 3 and st["dropped_range"] == 3 and st["n_cells"] == 3
    assert st["n_points"] + st["dropped_invalid"] + st["dropped_range"] + st["dropped_full"] == len(pts)
    with pytest.raises(ValueError):
        VoxelMapRef(0.0)
    with pytest.raises(ValueError):
        VoxelMapRef(0.1, min_range=5.0, max_range=5.0)


def test_pose_is_applied_as_in_the_pose_chain():
    """w = T p with rslo_pose_chain's formula: a quarter turn about z plus a translation, checked against a rotation matrix"""
    from rslo_amd.mapping import VoxelMapRef
    from rslo_amd import inference
    h = np.sqrt(0.5)
    pose = np.array([10.0, -2.0, 0.5, h, 0, 0, h])
    ref = VoxelMapRef(0.5)
    ref.insert(_pts((1.0, 0.25, 0.0)), pose)
    assert np.allclose(ref.points()[0][0, :3], [10.0 - 0.25, -2.0 + 1.0, 0.5], atol=1e-6)
    # and against the host pose chain itself: chaining (identity seed, pose, rel) moves rel's translation by pose
    rel = np.array([1.0, 0.25, 0.0, 1, 0, 0, 0])
    chained = inference.pose_chain_host(np.stack([pose, rel]))[1]
    assert np.allclose(chained[:3], pose[:3] + [-0.25, 1.0, 0.0], atol=1e-5)


def test_pose_convention_on_a_synthetic_drive():
    """Structure points only (sensor-frame z > -1.2): ground rings look alike from every pose and would hide a wrong
    convention.  Scan 1 under its own pose overlaps the map of scan 0 more than under the identity or the inverted pose."""
    from rslo_amd import synthetic
    from rslo_amd.mapping import VoxelMapRef
    s0, s1 = (synthetic.sequence_scan(i, seed=3, n_el=16, n_az=520) for i in (0, 1))
    s0, s1 = s0[s0[:, 2] > -1.2], s1[s1[:, 2] > -1.2]
    assert len(s0) > 500 and len(s1) > 500
    p0, p1 = synthetic.sequence_pose(0, 3), synthetic.sequence_pose(1, 3)
    assert p0.dtype == np.float64 and p0.tolist() == [0, 0, 0, 1, 0, 0, 0] and 0.5 < np.linalg.norm(p1[:3]) < 1.5
    # the inverse of (t, q): (-R^T t, conj q)
    yaw = 2.0 * np.arctan2(p1[6], p1[3])
    c, s = np.cos(-yaw), np.sin(-yaw)
    inv = np.array([-(c * p1[0] - s * p1[1]), -(s * p1[0] + c * p1[1]), 0.0, p1[3], 0, 0, -p1[6]])
    for voxel in (0.2, 0.4):
        ref = VoxelMapRef(voxel)
        ref.insert(s0, p0)
        good, ident, wrong = ref.overlap(s1, p1), ref.overlap(s1, IDENT), ref.overlap(s1, inv)
        print("voxel %.1f: overlap under the scan's pose %.3f, identity %.3f, inverted pose %.3f" % (voxel, good, ident, wrong))
        assert good > ident and good > wrong


def test_sequence_scan_is_unchanged_by_sequence_pose():
    from rslo_amd import synthetic
    a = synthetic.sequence_scan(2, seed=3, n_el=4, n_az=40)
    x, y, yaw = synthetic._sequence_xy_yaw(2, 3)
    b = synthetic.scan(40, 4, (x, y), yaw, scan_seed=7 * 3 + 3 * 2 + 1)
    assert a.tobytes() == b.tobytes()
    p = synthetic.sequence_pose(2, 3)
    assert p[:3].tolist() == [x, y, 0.0] and np.isclose(2 * np.arctan2(p[6], p[3]), yaw)


def test_map_bytes():
    from rslo_amd import capi
    for bad in (0, 1000, 1023, 1536, -1024):
        assert capi.map_bytes(bad) == 0
    sizes = [capi.map_bytes(1 << k) for k in range(10, 24)]
    assert sizes[0] > 0 and all(b > a for a, b in zip(sizes, sizes[1:]))
    assert sizes[0] >= 1024 * (8 + 8 + 4 + 16) and all(s % 8 == 0 for s in sizes)
    assert capi.lib().rslo_map_insert_ws_bytes(1000) >= 4000
    assert capi.lib().rslo_abi_version() == 1


def test_write_ply_round_trip(tmp_path):
    from rslo_amd.mapping import VoxelMapRef, write_ply
    rng = np.random.default_rng(0)
    rows = rng.normal(size=(37, 4)).astype(np.float32)
    rows[3, 0] = -0.0
    hits = rng.integers(1, 1000, 37).astype(np.int32)
    path = str(tmp_path / "m.ply")
    write_ply(path, rows, hits)
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and lines[2] == "element vertex 37"
    assert lines[3:8] == ["property float x", "property float y", "property float z", "property float intensity",
                          "property int hits"]
    rec = np.frombuffer(body, dtype=np.dtype([("v", "<f4", (4,)), ("h", "<i4")]))
    assert len(rec) == 37 and len(body) == 37 * 20
    assert rec["v"].tobytes() == rows.tobytes() and rec["h"].tobytes() == hits.tobytes()
    # save_ply of a map: the cells in tag order
    ref = VoxelMapRef(1.0)
    ref.insert(rows, IDENT)
    ref.save_ply(path, min_hits=1)
    body = open(path, "rb").read().split(b"end_header\n", 1)[1]
    rec = np.frombuffer(body, dtype=np.dtype([("v", "<f4", (4,)), ("h", "<i4")]))
    r, _, h = ref.points()
    assert rec["v"].tobytes() == r.tobytes() and rec["h"].tobytes() == h.tobytes()
