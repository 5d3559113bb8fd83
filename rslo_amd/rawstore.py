"""A raw KITTI odometry directory -> the numpy store KittiDatasetHDF5 reads, made on the GPU.

The reference builds its HDF5 store offline with Open3D (script/create_hdf5.py:297-360): per scan the normals
(estimate_normals, :130-147) and four voxel down-samples (:149-165, :337-347).  Here the two steps are
capi.estimate_normals (csrc/normals.hip) and capi.voxel_downsample (csrc/downsample.hip), and the output is the directory
layout of rslo.data.kitti_dataset_hdf5.write_numpy_store / GroupStore:
    <out>/<seq>/lidar_points.{values,offsets}.npy                   flat float32 [P_i * 4] per scan
    <out>/<seq>/lidar_normals.{values,offsets}.npy                  flat float32 [P_i * 3], NOT zeroed (zeroing the vertical
                                                                    ones is the reader's rule)
    <out>/<seq>/hier_lidar_points_normals_<size>.{values,offsets}.npy   flat float32 [Q_i * 6]
    <out>/<seq>/poses.npy, calib.P0..P3.npy, calib.Tr_velo_to_cam.npy   [L, 3, 4]
A scan that contains a NaN is skipped as the reference skips it (:319-323): its ragged entries stay empty and its pose
and calib rows stay zero.
"""
import glob
import os
import time
import warnings

import numpy as np

CALIB_KEYS = ("P0", "P1", "P2", "P3", "Tr_velo_to_cam")


def parse_pose_file(path):
    """One 3x4 row-major pose per line (create_hdf5.py:9-19) -> [L, 3, 4] float32"""
    with open(path) as f:
        rows = [line.split() for line in f if line.strip()]
    return np.array([[np.float32(v) for v in r] for r in rows], np.float32).reshape(-1, 3, 4)


def parse_calib_file(path):
    """calib.txt: a label and twelve numbers per line; the first four lines are P0..P3, the next Tr (create_hdf5.py:22-33)"""
    with open(path) as f:
        lines = [line.strip() for line in f if line.strip()]
    calib = {}
    for i, line in enumerate(lines):
        nums = np.array([np.float32(v) for v in line.split()[1:]], np.float32).reshape(3, 4)
        calib["P%d" % i if i < 4 else "Tr_velo_to_cam"] = nums
    missing = [k for k in CALIB_KEYS if k not in calib]
    if missing:
        raise ValueError("%s lacks %s" % (path, ", ".join(missing)))
    return calib


def read_kitti_sequence(kitti_root, seq):
    """(sorted velodyne/*.bin paths, poses [L, 3, 4] float32, calib {P0..P3, Tr_velo_to_cam: [3, 4]}) of
    <kitti_root>/sequences/<seq>; the poses are zeros when <kitti_root>/poses/<seq>.txt is absent (the test sequences
    11-21, create_hdf5.py:268-272)."""
    seq_dir = os.path.join(str(kitti_root), "sequences", seq)
    paths = sorted(glob.glob(os.path.join(seq_dir, "velodyne", "*.bin")))
    calib = parse_calib_file(os.path.join(seq_dir, "calib.txt"))
    pose_path = os.path.join(str(kitti_root), "poses", seq + ".txt")
    if os.path.exists(pose_path):
        poses = parse_pose_file(pose_path)
        if len(poses) != len(paths):
            raise ValueError("%s has %d poses for %d scans" % (pose_path, len(poses), len(paths)))
    else:
        poses = np.zeros((len(paths), 3, 4), np.float32)
    return paths, poses, calib


def _n_points(scan):
    if isinstance(scan, (str, os.PathLike)):
        return os.path.getsize(scan) // 16
    return len(scan)


def _load(scan):
    if isinstance(scan, (str, os.PathLike)):
        return np.fromfile(scan, dtype=np.float32).reshape(-1, 4)
    a = np.ascontiguousarray(scan, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != 4:
        raise ValueError("a raw scan is [P, 4] (x, y, z, intensity), got %s" % (a.shape,))
    return a


def _save_ragged(d, name, flat):
    np.save(os.path.join(d, name + ".values.npy"), np.concatenate(flat) if flat else np.zeros((0,), np.float32))
    np.save(os.path.join(d, name + ".offsets.npy"), np.cumsum([0] + [len(f) for f in flat]).astype(np.int64))


def build_sequence(out_root, seq, scans, poses, calib, hier_sizes=(0.1,), normal_radius=0.6, normal_max_nn=30,
                   device="cuda"):
    """Write <out_root>/<seq>/.  scans: iterable of [P, 4] float32 host arrays or .bin paths; poses [L, 3, 4] (or 4x4);
    calib: {P0..P3, Tr_velo_to_cam}.  Per scan: upload, normals (not zeroed), one down-sample per size in hier_sizes --
    each over the full-resolution cloud and its normals --, download.  The point and normal values go through memory
    maps sized beforehand from the file sizes / array lengths (a skipped scan leaves its share unused at the end of the
    file; the offsets never reach it).  Returns {"scans", "skipped", "read_ms", "normals_ms", "downsample_ms",
    "write_ms"}: milliseconds per scan, host clock around a device synchronise (normals_ms includes the upload, write_ms
    the downloads)."""
    import torch
    from numpy.lib.format import open_memmap
    from rslo_amd import capi
    from rslo_amd.downsample import hier_name

    scans = list(scans)
    L = len(scans)
    poses = np.asarray(poses, np.float32)
    if poses.shape[0] != L or poses.shape[1:] not in ((3, 4), (4, 4)):
        raise ValueError("poses must be [%d, 3, 4], got %s" % (L, poses.shape))
    missing = [k for k in CALIB_KEYS if k not in calib]
    if missing:
        raise ValueError("calib lacks %s" % ", ".join(missing))
    sizes = [float(s) for s in hier_sizes]
    d = os.path.join(str(out_root), seq)
    os.makedirs(d, exist_ok=True)

    total = sum(_n_points(s) for s in scans)
    if total == 0:          # nothing to map: two empty files
        np.save(os.path.join(d, "lidar_points.values.npy"), np.zeros((0,), np.float32))
        np.save(os.path.join(d, "lidar_normals.values.npy"), np.zeros((0,), np.float32))
        pts_mm = nrm_mm = None
    else:
        pts_mm = open_memmap(os.path.join(d, "lidar_points.values.npy"), mode="w+", dtype=np.float32, shape=(total * 4,))
        nrm_mm = open_memmap(os.path.join(d, "lidar_normals.values.npy"), mode="w+", dtype=np.float32, shape=(total * 3,))
    lens = np.zeros(L, np.int64)
    hier = {s: [] for s in sizes}
    out_poses = np.zeros_like(poses)
    out_calib = {k: np.zeros((L, 3, 4), np.float32) for k in CALIB_KEYS}
    t_read = t_nrm = t_ds = t_write = 0.0
    done = 0          # points written so far
    skipped = []
    for i, scan in enumerate(scans):
        t0 = time.perf_counter()
        pts = _load(scan)
        t1 = time.perf_counter()
        t_read += t1 - t0
        if np.isnan(pts).any():
            warnings.warn("scan %d of sequence %s%s contains NaN: skipped" % (
                i, seq, " (%s)" % scan if isinstance(scan, (str, os.PathLike)) else ""))
            skipped.append(i)
            for s in sizes:
                hier[s].append(np.zeros((0,), np.float32))
            continue
        P = len(pts)
        if done + P > total:
            raise ValueError("scan %d has more points than its size announced" % i)
        dev_pts = torch.from_numpy(pts).to(device)
        nrm, _ = capi.estimate_normals(dev_pts, normal_radius, normal_max_nn, None, False)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        t_nrm += t2 - t1
        rows = [capi.voxel_downsample(dev_pts, nrm, s) for s in sizes]
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        t_ds += t3 - t2
        if P:
            pts_mm[done * 4:(done + P) * 4] = pts.reshape(-1)
            nrm_mm[done * 3:(done + P) * 3] = nrm.cpu().numpy().reshape(-1)
        for s, r in zip(sizes, rows):
            hier[s].append(r.cpu().numpy().reshape(-1))
        lens[i] = P
        done += P
        out_poses[i] = poses[i]
        for k in CALIB_KEYS:
            out_calib[k][i] = np.asarray(calib[k], np.float32).reshape(-1)[:12].reshape(3, 4)
        t_write += time.perf_counter() - t3

    t0 = time.perf_counter()
    if total:
        pts_mm.flush()
        nrm_mm.flush()
    del pts_mm, nrm_mm
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    np.save(os.path.join(d, "lidar_points.offsets.npy"), offs * 4)
    np.save(os.path.join(d, "lidar_normals.offsets.npy"), offs * 3)
    for s in sizes:
        _save_ragged(d, hier_name(s), hier[s])
    np.save(os.path.join(d, "poses.npy"), out_poses)
    for k in CALIB_KEYS:
        np.save(os.path.join(d, "calib.%s.npy" % k), out_calib[k])
    t_write += time.perf_counter() - t0
    n = max(L, 1)
    return {"scans": L, "skipped": skipped, "read_ms": 1e3 * t_read / n, "normals_ms": 1e3 * t_nrm / n,
            "downsample_ms": 1e3 * t_ds / n, "write_ms": 1e3 * t_write / n}
