"""World voxel map of a streamed trajectory: the registered cloud of an OdometryRunner, built on the GPU.

    vmap = VoxelMap(voxel_size=0.2, capacity=1 << 22)
    runner = inference.OdometryRunner(net, voxel_map=vmap)      # every run() inserts its scan under its absolute pose
    rows, tags, hits = vmap.points(min_hits=2)                 # [M, 4] (x, y, z, intensity), sorted by tag
    vmap.save_ply("map.ply", min_hits=2)

VoxelMap is the device map (csrc/map.hip, rules in include/rslo_hip.h); VoxelMapRef is the float64 numpy restatement of
the same rules on host arrays and the arbiter of the tests, which compare bit for bit.  The rules in one place:

  * the map lives in the frame of the trajectory (the frame of scan 0) and is a set of cubic cells of edge voxel_size;
  * scan number s (inserts since the last reset) under pose (t, q wxyz), float64: p = float64(xyz_i); skipped
    (dropped_invalid) when a coordinate is not finite or d2 = p.x*p.x + p.y*p.y + p.z*p.z fails
    d2 >= min_range*min_range and d2 < max_range*max_range;
    w = t + (p + (2.0*b*q.w + 2.0*c)), b = v x p, c = v x b, v = q.xyz -- the arithmetic of rslo_pose_chain, w = T_abs p,
    q not renormalised; cell = floor(w / voxel_size); any |cell| >= 2^20 drops the point (dropped_range);
  * tag = (s << 32) | i.  A cell holds the SMALLEST tag ever inserted into it, hits = the number of points ever inserted
    into it, and row = (float32(w), intensity) of the point that owns the tag: the first point wins, which is what makes
    the map reproducible (float sums would depend on arrival order);
  * the device map probes at most 128 slots: a point that finds neither its cell nor an empty slot is dropped
    (dropped_full) -- a cell is stored completely or not at all.  VoxelMapRef has no capacity: it specifies a map that
    did not overflow.
"""
import numpy as np

COUNTERS = ("n_scans", "n_cells", "n_points", "dropped_invalid", "dropped_range", "dropped_full")
_MAXC = 1 << 20


def write_ply(path, rows, hits):
    """Binary little-endian PLY: vertex x y z intensity (float) and hits (int); numpy only."""
    rows = np.ascontiguousarray(np.asarray(rows, dtype="<f4")).reshape(-1, 4)
    hits = np.asarray(hits, dtype="<i4").reshape(-1)
    if len(hits) != len(rows):
        raise ValueError("write_ply: rows [M, 4] and hits [M] must have the same length")
    rec = np.empty((len(rows),), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4"), ("hits", "<i4")])
    for k, name in enumerate(("x", "y", "z", "intensity")):
        rec[name] = rows[:, k]
    rec["hits"] = hits
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\n"
            "property float z\nproperty float intensity\nproperty int hits\nend_header\n" % len(rows))
    with open(path, "wb") as f:
        f.write(head.encode("ascii"))
        f.write(rec.tobytes())


def _check_params(voxel_size, min_range, max_range):
    voxel_size, min_range, max_range = float(voxel_size), float(min_range), float(max_range)
    if not (0.0 < voxel_size < float("inf")):
        raise ValueError("voxel_size must be positive and finite")
    if not (0.0 <= min_range < max_range):
        raise ValueError("need 0 <= min_range < max_range")
    return voxel_size, min_range, max_range


class VoxelMapRef:
    """The float64 numpy restatement of the map's rules (module docstring), same methods as VoxelMap on host arrays.
    Cells are kept as arrays sorted by packed key; no probe limit, no capacity."""

    def __init__(self, voxel_size=0.2, min_range=0.0, max_range=float("inf")):
        self.voxel_size, self.min_range, self.max_range = _check_params(voxel_size, min_range, max_range)
        self.reset()

    def reset(self):
        self.keys = np.zeros((0,), np.int64)
        self.tags = np.zeros((0,), np.int64)
        self.hits = np.zeros((0,), np.int32)
        self.rows = np.zeros((0, 4), np.float32)
        self.counters = dict.fromkeys(COUNTERS, 0)

    def _cells(self, points, pose):
        """-> (status [P]: 0 accepted, 1 skipped, 2 out of range; key [P] int64; world [P, 3] float64)"""
        pts = np.asarray(points)
        if pts.dtype != np.float32 or pts.ndim != 2 or pts.shape[1] < 3:
            raise ValueError("points must be float32 [P, >= 3]")
        pose = np.asarray([0, 0, 0, 1, 0, 0, 0] if pose is None else pose, dtype=np.float64).reshape(7)
        P = len(pts)
        status = np.zeros((P,), np.int32)
        with np.errstate(all="ignore"):
            p = pts[:, :3].astype(np.float64)
            finite = np.isfinite(pts[:, :3]).all(axis=1)
            d2 = p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1] + p[:, 2] * p[:, 2]
            gate = (d2 >= self.min_range * self.min_range) & (d2 < self.max_range * self.max_range)
            status[~(finite & gate)] = 1
            t, qw, v = pose[:3], pose[3], pose[4:7]

            def cross(a, b):      # a: [3] or [P, 3]
                a = np.broadcast_to(a, b.shape)
                return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                                 a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)
            b = cross(v, p)
            c = cross(v, b)
            w = t[None, :] + (p + (2.0 * b * qw + 2.0 * c))
            cell = np.floor(w / self.voxel_size)
            inside = (np.abs(cell) < float(_MAXC)).all(axis=1)      # False for NaN / inf as well
            status[(status == 0) & ~inside] = 2
            ci = np.where(inside[:, None], cell, 0.0).astype(np.int64) + _MAXC
        key = (ci[:, 0] << 42) | (ci[:, 1] << 21) | ci[:, 2]
        return status, key, w

    def insert(self, points, pose=None):
        pts = np.asarray(points)
        status, key, w = self._cells(pts, pose)
        s = self.counters["n_scans"]
        ok = np.nonzero(status == 0)[0]
        self.counters["n_scans"] = s + 1
        self.counters["n_points"] += len(ok)
        self.counters["dropped_invalid"] += int((status == 1).sum())
        self.counters["dropped_range"] += int((status == 2).sum())
        if len(ok) == 0:
            return
        ukey, first, cnt = np.unique(key[ok], return_index=True, return_counts=True)      # first: lowest index of the cell
        owner = ok[first]
        pos = np.searchsorted(self.keys, ukey)
        old = np.zeros((len(ukey),), bool)
        inb = pos < len(self.keys)
        old[inb] = self.keys[pos[inb]] == ukey[inb]
        self.hits[pos[old]] += cnt[old].astype(np.int32)            # an earlier scan's cell: only the hits change
        new = ~old
        if new.any():
            o = owner[new]
            rows = np.zeros((len(o), 4), np.float32)
            rows[:, :3] = w[o].astype(np.float32)
            if pts.shape[1] >= 4:
                rows[:, 3] = pts[o, 3]
            keys = np.concatenate([self.keys, ukey[new]])
            order = np.argsort(keys, kind="stable")
            self.keys = keys[order]
            self.tags = np.concatenate([self.tags, (np.int64(s) << 32) | o.astype(np.int64)])[order]
            self.hits = np.concatenate([self.hits, cnt[new].astype(np.int32)])[order]
            self.rows = np.concatenate([self.rows, rows])[order]
        self.counters["n_cells"] = len(self.keys)

    def lookup(self, points, pose=None, return_tags=False):
        status, key, _ = self._cells(points, pose)
        hits = np.full((len(status),), -1, np.int32)
        tags = np.full((len(status),), -1, np.int64)
        ok = np.nonzero(status == 0)[0]
        hits[ok] = 0
        pos = np.searchsorted(self.keys, key[ok])
        inb = pos < len(self.keys)
        found = np.zeros((len(ok),), bool)
        found[inb] = self.keys[pos[inb]] == key[ok][inb]
        hits[ok[found]] = self.hits[pos[found]]
        tags[ok[found]] = self.tags[pos[found]]
        return (hits, tags) if return_tags else hits

    def overlap(self, points, pose=None):
        hits = self.lookup(points, pose)
        return float((hits > 0).sum()) / float((hits >= 0).sum())

    def points(self, min_hits=1, center=None, radius=None, sort=True):
        sel = self.hits >= min_hits
        if center is not None:
            c = np.asarray(center, dtype=np.float64).reshape(3)
            r = float(radius)
            d = self.rows[:, :3].astype(np.float64) - c[None, :]
            sel &= (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]) < r * r
        idx = np.nonzero(sel)[0]
        if sort:
            idx = idx[np.argsort(self.tags[idx], kind="stable")]
        return self.rows[idx], self.tags[idx], self.hits[idx]

    def stats(self):
        return dict(self.counters, dropped_full=0)

    def save_ply(self, path, min_hits=1):
        rows, _, hits = self.points(min_hits)
        write_ply(path, rows, hits)


class VoxelMap:
    """The device map: owns the table (one allocation of rslo_map_bytes(capacity) bytes) and an insert workspace that
    grows only when a larger scan arrives.  insert / lookup / overlap enqueue on the current stream and read nothing on
    the host; points() and stats() make one host read each."""

    def __init__(self, voxel_size=0.2, capacity=1 << 22, device="cuda", min_range=0.0, max_range=float("inf")):
        import torch
        from rslo_amd import capi
        self.voxel_size, self.min_range, self.max_range = _check_params(voxel_size, min_range, max_range)
        self.capacity = int(capacity)
        nbytes = capi.map_bytes(self.capacity)
        if nbytes == 0:
            raise capi.RsloHipError("VoxelMap: capacity must be a power of two >= 1024, got %r" % (capacity,))
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._buf = torch.empty((nbytes // 8,), dtype=torch.int64, device=self.device)
        self._ws = None
        self._ws_points = -1
        self._identity = torch.tensor([0, 0, 0, 1, 0, 0, 0], dtype=torch.float64, device=self.device)
        self.reserve(0)
        self.reset()

    def reset(self):
        """Empty the map; the scan counter restarts at 0 (a new sequence has a new frame)."""
        from rslo_amd import capi
        capi.map_reset(self._buf, self.capacity, self.voxel_size, self.min_range, self.max_range)

    def reserve(self, n_points):
        """Size the insert workspace for scans of up to n_points points, so that later inserts allocate nothing."""
        import torch
        from rslo_amd import capi
        if n_points > self._ws_points:
            self._ws = torch.empty((capi.lib().rslo_map_insert_ws_bytes(int(n_points)),), dtype=torch.uint8,
                                   device=self.device)
            self._ws_points = int(n_points)

    def _pose(self, pose):
        """a float64 CUDA [7] tensor as it is (a row of OdometryRunner's trajectory); None = identity; anything else is copied"""
        import torch
        if pose is None:
            return self._identity
        if torch.is_tensor(pose) and pose.is_cuda and pose.dtype == torch.float64:
            return pose
        return torch.as_tensor(np.asarray(pose, dtype=np.float64).reshape(7)).to(self.device)

    def insert(self, points, pose=None):
        """One scan (fp32 CUDA [P, F >= 3], read in place; column 3 is the intensity when F >= 4) under pose (t, q wxyz)."""
        from rslo_amd import capi
        self.reserve(points.shape[0])
        capi.map_insert(self._buf, points, self._pose(pose), self._ws)

    def lookup(self, points, pose=None, return_tags=False):
        """hits int32 [P]: -1 for a skipped or out-of-range point, 0 for a cell that is not in the map, else its hits."""
        from rslo_amd import capi
        return capi.map_lookup(self._buf, points, self._pose(pose), tags=True if return_tags else None)

    def overlap(self, points, pose=None):
        """Share of the scan's valid points that fall into occupied cells: a device scalar, no host read."""
        hits = self.lookup(points, pose)
        return (hits > 0).sum() / (hits >= 0).sum()

    def points(self, min_hits=1, center=None, radius=None, sort=True):
        """(rows [M, 4] fp32, tags [M] int64, hits [M] int32) of the cells with hits >= min_hits, and within radius of
        center when one is given (a sequence, or a float64 CUDA [3] tensor).  One host read (M).  sort=True orders by tag:
        deterministic bit for bit."""
        import torch
        from rslo_amd import capi
        if center is not None:
            if radius is None:
                raise ValueError("points: a center needs a radius")
            if not (torch.is_tensor(center) and center.is_cuda and center.dtype == torch.float64):
                center = torch.as_tensor(np.asarray(center, dtype=np.float64).reshape(3)).to(self.device)
        r = 0.0 if radius is None else float(radius)
        M = int(capi.map_export(self._buf, min_hits, center, r)[0])      # count only; nothing else changes the map meanwhile
        rows = torch.empty((M, 4), dtype=torch.float32, device=self.device)
        tags = torch.empty((M,), dtype=torch.int64, device=self.device)
        hits = torch.empty((M,), dtype=torch.int32, device=self.device)
        if M:
            capi.map_export(self._buf, min_hits, center, r, rows, tags, hits)
            if sort:
                tags, order = torch.sort(tags)
                rows, hits = rows[order], hits[order]
        return rows, tags, hits

    def stats(self):
        """The six counters of the map's header as a dict (one host read)."""
        from rslo_amd import capi
        vals = self._buf[capi.MAP_HDR_COUNTERS:capi.MAP_HDR_COUNTERS + len(COUNTERS)].tolist()
        return dict(zip(COUNTERS, (int(v) for v in vals)))

    def save_ply(self, path, min_hits=1):
        rows, _, hits = self.points(min_hits)
        write_ply(path, rows.cpu().numpy(), hits.cpu().numpy())
