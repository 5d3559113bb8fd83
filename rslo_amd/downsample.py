"""Float64 restatement of the voxel down-sample rules of csrc/downsample.hip (numpy only).

The reference down-samples offline with Open3D (script/create_hdf5.py:149-165, called at :337-347 for 0.1 / 0.2 / 0.4 /
0.8 m, each time from the full-resolution cloud):
    pcd.voxel_down_sample(voxel_size)
Open3D is not part of the reference tree and is not a dependency here: the rules are recalled from its
PointCloud::VoxelDownSample and are stated in include/rslo_hip.h.  This module is the arbiter of the kernel's tests and
a utility for scripts.  It is NOT a fallback: capi.voxel_downsample never calls it.

Every operation below is an IEEE double operation on exactly-converted fp32 inputs in a fixed order, rounded once to
fp32, so the kernel is expected to agree with it bit for bit.
"""
import numpy as np

MAX_CELLS = 1 << 21       # cell indices are sorted as three 21-bit fields


def hier_name(voxel_size):
    """Dataset name of one down-sample size: 0.1 -> hier_lidar_points_normals_0.1"""
    return "hier_lidar_points_normals_%s" % repr(float(voxel_size))


def voxel_down_sample_ref(xyz, normals, voxel_size):
    """xyz [P, >=3] and normals [P, 3] or None (read as given, computed in float64).  Returns (rows fp32 [Q, 6] -- or
    [Q, 3] without normals --, voxel_of_point int32 [P] (-1: invalid point), npts int32 [Q]); rows in ascending
    (cx, cy, cz).  Raises ValueError when a cell index reaches 2^21."""
    voxel_size = float(voxel_size)
    if not voxel_size > 0.0:
        raise ValueError("voxel_size must be positive")
    xyz = np.asarray(xyz)[:, :3].astype(np.float64)
    P = len(xyz)
    feats = xyz if normals is None else np.concatenate([xyz, np.asarray(normals)[:, :3].astype(np.float64)], 1)
    width = feats.shape[1]
    voxel_of_point = np.full(P, -1, np.int32)
    ids = np.nonzero(np.isfinite(xyz).all(1))[0]          # ascending input index
    if ids.size == 0:
        return np.zeros((0, width), np.float32), voxel_of_point, np.zeros(0, np.int32)
    pts = xyz[ids]
    vmin = pts.min(0) - 0.5 * voxel_size
    cell = np.floor((pts - vmin) / voxel_size)            # true division, never a multiplication by a reciprocal
    if (cell >= MAX_CELLS).any():
        raise ValueError("the cloud spans %d cells of %g along an axis; at most 2^21 can be told apart"
                         % (int(cell.max()) + 1, voxel_size))
    cell = cell.astype(np.int64)
    key = (cell[:, 0] << 42) | (cell[:, 1] << 21) | cell[:, 2]
    order = np.argsort(key, kind="stable")                # a cell's members stay in ascending input index
    skey = key[order]
    head = np.concatenate([[True], skey[1:] != skey[:-1]])
    start = np.nonzero(head)[0]
    npts = np.diff(np.concatenate([start, [len(skey)]])).astype(np.int32)
    voxel_of_point[ids[order]] = (np.cumsum(head) - 1).astype(np.int32)
    # sequential sums: step k adds the k-th member of every cell that has one, so each cell's sum is formed in
    # ascending input index, one double add at a time
    src = feats[ids[order]]
    acc = np.zeros((len(start), width))
    for k in range(int(npts.max())):
        live = np.nonzero(npts > k)[0]
        acc[live] = acc[live] + src[start[live] + k]
    rows = (acc / npts[:, None].astype(np.float64)).astype(np.float32)
    return rows, voxel_of_point, npts
