"""Surfel map: per-cell planes from order-free integer moments, and point-to-plane registration against them.

    smap = SurfelMap(voxel_size=0.4, capacity=1 << 20)
    smap.insert(scan, pose)                                     # fp32 CUDA [P, >= 3]: only x, y, z are read
    pose, info = smap.register(scan, pose, iters=4, robust_scale=0.2)
    pose, info = smap.register(scan, pose, iters=4, robust_scale=3.0, cost="distribution")      # every fitted cell
    keys, moments, rows = smap.cells(min_flag=2)                # the planar cells, sorted by key
    runner = inference.OdometryRunner(net, surfels=smap, surfel_refine=dict(iters=4))

SurfelMap is the device map (csrc/surfel.hip, rules in include/rslo_hip.h "Surfel map"); SurfelMapRef is the float64 numpy
restatement of the same rules on host arrays and the arbiter of the tests: keys, moments and rows are compared bit for
bit.  The rules in one place:

  * the cell of a point is the world voxel map's (mapping.VoxelMapRef._cells: validity, range gate, w = T p, cell =
    floor(w / voxel_size), |cell| < 2^20);
  * per axis s = w / voxel, f = s - floor(s), q = int64(floor(f * 16384.0)) clamped to 0 .. 16383; the ten moments of the
    cell grow by (1, qx, qy, qz, qx qx, qx qy, qx qz, qy qy, qy qz, qz qz) -- INTEGERS, so the moments of a cell do not
    depend on the order in which points or scans arrive (the device adds them with 64-bit integer atomics);
  * the row of a cell is a pure function of its moments, key and the parameters (derive_rows): mean, unit normal of the
    smallest eigenvalue of the trace-scaled covariance by six cyclic Jacobi sweeps (the rotation of normals.py / csrc/
    normals.hip, in float64), the variance along the normal, and a flag: 0 fewer than min_points points or no spread,
    2 planar (l0 <= planar_ratio * l1 and l1 >= line_ratio * l2), else 1;
  * nearest: among the PLANAR cells c + {-1,0,1}^3 around a point's cell the one whose mean is nearest (then the
    smallest key), accepted within max_dist <= voxel_size;
  * normal equations: every matched point adds ONE plane row a = (n, w x n), r = n . (w - mean) with the CELL's normal:
    no scan normal is read and there is no point-term fallback; robust weights and the Gauss-Newton step are those of
    mapping.py (gauss_newton.py);
  * cost="distribution" on nearest / normal_equations / register (include/rslo_hip.h "Distribution cost"): the
    candidates are the cells with flag >= min_flag (default 1: every fitted cell, poles and vegetation included), and a
    matched point adds d^T M d with d = w - mean and M = (C + lam I)^-1, C the covariance of the cell's moments in
    metres, lam = reg_rel * trace(C) + reg_abs^2 (SurfelMapRef.information, gauss_newton.info_terms).  The residual is
    in sigmas, and so is robust_scale.  cost="plane", the default, is the rule above and takes none of these options;
  * the device table probes at most 128 slots and drops what finds no slot (dropped_full); SurfelMapRef has no capacity.
    Between two prunes the table only fills: reset() empties it;
  * prune(center=None, radius=None, inner_radius=None, min_count=1) is the one call that removes cells (include/
    rslo_hip.h "Rolling local surfel map").  With cc = (float64(cell) + 0.5) * voxel_size, the cell's centre, d = cc -
    center and d2 = dx*dx + dy*dy + dz*dz, a cell is KEPT iff it is near (center is None, or d2 < radius*radius) and not
    sparse (N = moments[0] >= min_count, or a center is given and d2 < inner_radius*inner_radius; inner_radius=None
    means radius).  A comparison that is false evicts.  Kept cells keep key, moments and row to the bit; n_cells and
    n_planar are recounted, the other counters stay.  prune_stats() -> {n_prunes, n_evicted, n_lost}: calls, cells
    evicted so far, and -- device map only -- kept records that found no slot when the table was rebuilt.
"""
import numpy as np

from .gauss_newton import info_terms, register_loop, robust_weighted, terms_of
from .mapping import VoxelMapRef, _DeviceTable, _check_params, _check_register, _max_dist_of, check_scale

COUNTERS = ("n_scans", "n_cells", "n_points", "dropped_invalid", "dropped_range", "dropped_full", "n_planar")
PRUNE_COUNTERS = ("n_prunes", "n_evicted", "n_lost")
Q = 16384.0
_MAXC = 1 << 20


def _check_plane_params(min_points, planar_ratio, line_ratio):
    if int(min_points) != min_points or min_points < 3:
        raise ValueError("min_points must be an integer >= 3, got %r" % (min_points,))
    planar_ratio, line_ratio = float(planar_ratio), float(line_ratio)
    if not (0.0 <= planar_ratio < float("inf") and 0.0 <= line_ratio < float("inf")):
        raise ValueError("planar_ratio and line_ratio must be >= 0 and finite")
    return int(min_points), planar_ratio, line_ratio


SURFEL_REFINE_DEFAULTS = dict(iters=4, max_dist=None, robust_scale=0.2, damping=1e-6, min_pairs=50, tol_t=0.0, tol_r=0.0)
COSTS = ("plane", "distribution")
DIST_DEFAULTS = dict(min_flag=1, reg_rel=0.01, reg_abs=0.02)
DIST_ROBUST_SCALE = 3.0      # the runner's default for cost="distribution": the residual is in sigmas, a three-sigma soft gate


def check_cost(cost="plane", min_flag=None, reg_rel=None, reg_abs=None):
    """The cost options of nearest / normal_equations / register (ValueError).  -> None for cost="plane", which takes
    none of the others (min_flag=2 says what it does and is accepted); (min_flag, reg_rel, reg_abs) for
    cost="distribution", defaults DIST_DEFAULTS: min_flag 1 or 2, reg_rel and reg_abs >= 0, finite, not both zero."""
    if cost not in COSTS:
        raise ValueError("cost must be one of %s, got %r" % (COSTS, cost))
    if cost == "plane":
        if min_flag not in (None, 2) or reg_rel is not None or reg_abs is not None:
            raise ValueError("cost=\"plane\" matches the planar cells only and takes no min_flag, reg_rel or reg_abs")
        return None
    mf = DIST_DEFAULTS["min_flag"] if min_flag is None else min_flag
    if mf not in (1, 2):
        raise ValueError("min_flag must be 1 or 2, got %r" % (min_flag,))
    rr = float(DIST_DEFAULTS["reg_rel"] if reg_rel is None else reg_rel)
    ra = float(DIST_DEFAULTS["reg_abs"] if reg_abs is None else reg_abs)
    if not (0.0 <= rr < float("inf") and 0.0 <= ra < float("inf") and (rr > 0.0 or ra > 0.0)):
        raise ValueError("reg_rel and reg_abs must be >= 0, finite and not both zero (NaN is refused), got %r and %r"
                         % (reg_rel, reg_abs))
    return int(mf), rr, ra


def _dist_kw(dist):
    return dict(zip(("min_flag", "reg_rel", "reg_abs"), dist))


def check_surfel_refine(options, surfel_map):
    """The surfel_refine= options of an OdometryRunner against the map it was given (ValueError): -> the keyword
    arguments of surfel_map.register, defaults filled in.  cost="plane" (the default): SURFEL_REFINE_DEFAULTS and
    nothing else.  cost="distribution" also takes min_flag, reg_rel and reg_abs (DIST_DEFAULTS), and its default
    robust_scale is DIST_ROBUST_SCALE."""
    known = set(SURFEL_REFINE_DEFAULTS) | {"cost"} | set(DIST_DEFAULTS)
    unknown = set(options) - known
    if unknown:
        raise ValueError("surfel_refine takes %s; got %s" % (", ".join(sorted(known)), sorted(unknown)))
    options = dict(options)
    dist = check_cost(options.pop("cost", "plane"), *(options.pop(k, None) for k in ("min_flag", "reg_rel", "reg_abs")))
    opts = dict(SURFEL_REFINE_DEFAULTS)
    if dist is not None:
        opts["robust_scale"] = DIST_ROBUST_SCALE
    opts.update(options)
    opts["iters"] = int(opts["iters"])
    _check_register(opts["iters"], opts["tol_t"], opts["tol_r"])
    _max_dist_of(opts["max_dist"], surfel_map.voxel_size)
    check_scale(opts["robust_scale"])
    if dist is not None:
        opts.update(cost="distribution", **_dist_kw(dist))
    return opts


def check_surfel_prune(center, radius, inner_radius, min_count, has_center=None):
    """The argument errors of prune (ValueError), raised before anything is written, next to mapping.check_prune; ->
    (radius, inner_radius, min_count) as two floats and an int (radius 0.0 when None, inner_radius = radius when None).
    has_center: whether a centre will be given, for callers that validate before they have one.  Stricter than
    rslo_surfel_prune in one point: the radii are checked without a centre too, where the C call ignores them."""
    if has_center is None:
        has_center = center is not None
    if has_center and radius is None:
        raise ValueError("prune: a center needs a radius")
    r = 0.0 if radius is None else float(radius)
    if not r >= 0.0:
        raise ValueError("prune: radius must be >= 0 (NaN is refused), got %r" % (radius,))
    ri = r if inner_radius is None else float(inner_radius)
    if not 0.0 <= ri <= r:
        raise ValueError("prune: need 0 <= inner_radius <= radius (NaN is refused), got %r and %r" % (inner_radius, radius))
    if int(min_count) != min_count or min_count < 1:
        raise ValueError("prune: min_count must be an integer >= 1, got %r" % (min_count,))
    return r, ri, int(min_count)


def _rot(app, aqq, apq, arp, arq, v0p, v0q, v1p, v1q, v2p, v2q):
    """nm_rot in float64 on arrays: the rotation that annihilates a_pq; rows with a_pq == 0 are left as they are"""
    act = apq != 0.0
    theta = (aqq - app) / (2.0 * np.where(act, apq, 1.0))
    t = np.copysign(1.0, theta) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
    c = 1.0 / np.sqrt(t * t + 1.0)
    s = t * c
    new = (app - t * apq, aqq + t * apq, np.zeros_like(apq), c * arp - s * arq, s * arp + c * arq,
           c * v0p - s * v0q, s * v0p + c * v0q, c * v1p - s * v1q, s * v1p + c * v1q, c * v2p - s * v2q, s * v2p + c * v2q)
    old = (app, aqq, apq, arp, arq, v0p, v0q, v1p, v1q, v2p, v2q)
    return tuple(np.where(act, n, o) for n, o in zip(new, old))


def jacobi_eig(a00, a01, a02, a11, a12, a22):
    """Six cyclic sweeps on symmetric 3 x 3 matrices given as arrays: -> (diagonal (a00, a11, a22), off-diagonal
    (a01, a02, a12), V as v[row][column]); operation by operation the device's loop."""
    one, zero = np.ones_like(a00), np.zeros_like(a00)
    v = [[one, zero, zero], [zero, one, zero], [zero, zero, one]]
    with np.errstate(all="ignore"):
        for _ in range(6):
            a00, a11, a01, a02, a12, v[0][0], v[0][1], v[1][0], v[1][1], v[2][0], v[2][1] = _rot(
                a00, a11, a01, a02, a12, v[0][0], v[0][1], v[1][0], v[1][1], v[2][0], v[2][1])
            a00, a22, a02, a01, a12, v[0][0], v[0][2], v[1][0], v[1][2], v[2][0], v[2][2] = _rot(
                a00, a22, a02, a01, a12, v[0][0], v[0][2], v[1][0], v[1][2], v[2][0], v[2][2])
            a11, a22, a12, a01, a02, v[0][1], v[0][2], v[1][1], v[1][2], v[2][1], v[2][2] = _rot(
                a11, a22, a12, a01, a02, v[0][1], v[0][2], v[1][1], v[1][2], v[2][1], v[2][2])
    return (a00, a11, a22), (a01, a02, a12), v


def covariances(moments):
    """-> (mu [M, 3], c [M, 6] in the order 00 01 02 11 12 22, tr [M]) of moments int64 [M, 10], by the rules"""
    mo = np.asarray(moments, np.int64).reshape(-1, 10)
    n = mo[:, 0].astype(np.float64)
    with np.errstate(all="ignore"):
        mu = mo[:, 1:4].astype(np.float64) / n[:, None]
        pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
        c = np.stack([mo[:, 4 + k].astype(np.float64) / n - mu[:, a] * mu[:, b] for k, (a, b) in enumerate(pairs)], axis=1)
        tr = (c[:, 0] + c[:, 3]) + c[:, 5]
    return mu, c, tr


def derive_rows(keys, moments, voxel_size, min_points=5, planar_ratio=0.1, line_ratio=0.05):
    """rows float64 [M, 8] = {mean (3), normal (3), sigma2, flag} of the cells (keys int64 [M], moments int64 [M, 10]):
    the float64 twin of the device's derive function, vectorised, operation by operation."""
    keys = np.asarray(keys, np.int64).reshape(-1)
    mo = np.asarray(moments, np.int64).reshape(-1, 10)
    voxel = float(voxel_size)
    rows = np.zeros((len(keys), 8), np.float64)
    if len(keys) == 0:
        return rows
    mu, c, tr = covariances(mo)
    with np.errstate(all="ignore"):
        good = (mo[:, 0] >= min_points) & (tr > 0.0) & (tr < np.inf)
        trs = np.where(good, tr, 1.0)
        a = [np.where(good, c[:, k] / trs, 0.0) for k in range(6)]
        (d0, d1, d2), _, v = jacobi_eig(*a)
        c1 = d1 < d0
        c2 = d2 < np.where(c1, d1, d0)
        l0 = np.where(c2, d2, np.where(c1, d1, d0))
        ra = np.where(c2, d0, np.where(c1, d0, d1))
        rb = np.where(c2, d1, d2)
        c3 = rb < ra
        l1, l2 = np.where(c3, rb, ra), np.where(c3, ra, rb)
        e = [np.where(c2, v[r][2], np.where(c1, v[r][1], v[r][0])) for r in range(3)]
        nn = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        nrm = [e[r] / nn for r in range(3)]
        big = nrm[0]
        big = np.where(np.abs(nrm[1]) > np.abs(big), nrm[1], big)
        big = np.where(np.abs(nrm[2]) > np.abs(big), nrm[2], big)
        neg = big < 0.0
        nrm = [np.where(neg, -x, x) for x in nrm]
        cell = np.stack([(keys >> 42) & 0x1fffff, (keys >> 21) & 0x1fffff, keys & 0x1fffff], axis=1) - _MAXC
        u = voxel / Q
        planar = (l0 <= planar_ratio * l1) & (l1 >= line_ratio * l2)
        full = np.empty_like(rows)
        for r in range(3):
            full[:, r] = (cell[:, r].astype(np.float64) + (mu[:, r] + 0.5) / Q) * voxel
            full[:, 3 + r] = nrm[r]
        full[:, 6] = ((l0 * tr) * u) * u
        full[:, 7] = np.where(planar, 2.0, 1.0)
    rows[good] = full[good]
    return rows


def write_surfel_ply(path, rows):
    """Binary little-endian PLY: vertex x y z nx ny nz (float) from rows [M, 8]; numpy only."""
    rows = np.asarray(rows, np.float64).reshape(-1, 8)
    rec = np.ascontiguousarray(rows[:, :6].astype("<f4"))
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\n"
            "property float z\nproperty float nx\nproperty float ny\nproperty float nz\nend_header\n" % len(rec))
    with open(path, "wb") as f:
        f.write(head.encode("ascii"))
        f.write(rec.tobytes())


class SurfelMapRef:
    """The float64 numpy restatement of the surfel map's rules (module docstring), same methods as SurfelMap on host
    arrays.  Cells are kept as arrays sorted by packed key; no probe limit, no capacity."""

    def __init__(self, voxel_size=0.4, min_range=0.0, max_range=float("inf"), min_points=5, planar_ratio=0.1,
                 line_ratio=0.05):
        self.voxel_size, self.min_range, self.max_range = _check_params(voxel_size, min_range, max_range)
        self.min_points, self.planar_ratio, self.line_ratio = _check_plane_params(min_points, planar_ratio, line_ratio)
        self._grid = VoxelMapRef(self.voxel_size, self.min_range, self.max_range)      # the cell of a point is the map's
        self.reset()

    def reset(self):
        self.keys = np.zeros((0,), np.int64)
        self.moments = np.zeros((0, 10), np.int64)
        self.rows = np.zeros((0, 8), np.float64)
        self.counters = dict.fromkeys(COUNTERS, 0)
        self.prune_counters = dict.fromkeys(PRUNE_COUNTERS, 0)

    def _cells(self, points, pose):
        return self._grid._cells(points, pose)

    def quantise(self, w):
        """q int64 [n, 3] of world positions w [n, 3]: rule 2, clamp included"""
        s = w / self.voxel_size
        f = s - np.floor(s)
        return np.clip(np.floor(f * Q), 0.0, Q - 1.0).astype(np.int64)

    def derive_rows(self, keys=None, moments=None):
        """the rows of the given cells (default: all of this map's) from their moments: derive_rows() with this map's parameters"""
        keys = self.keys if keys is None else keys
        moments = self.moments if moments is None else moments
        return derive_rows(keys, moments, self.voxel_size, self.min_points, self.planar_ratio, self.line_ratio)

    def insert(self, points, pose=None):
        status, key, w = self._cells(points, pose)
        ok = np.nonzero(status == 0)[0]
        self.counters["n_scans"] += 1
        self.counters["n_points"] += len(ok)
        self.counters["dropped_invalid"] += int((status == 1).sum())
        self.counters["dropped_range"] += int((status == 2).sum())
        if len(ok) == 0:
            return
        q = self.quantise(w[ok])
        add = np.stack([np.ones((len(ok),), np.int64), q[:, 0], q[:, 1], q[:, 2], q[:, 0] * q[:, 0], q[:, 0] * q[:, 1],
                        q[:, 0] * q[:, 2], q[:, 1] * q[:, 1], q[:, 1] * q[:, 2], q[:, 2] * q[:, 2]], axis=1)
        ukey, inv = np.unique(key[ok], return_inverse=True)
        sums = np.zeros((len(ukey), 10), np.int64)
        np.add.at(sums, inv.reshape(-1), add)
        pos = np.searchsorted(self.keys, ukey)
        old = np.zeros((len(ukey),), bool)
        inb = pos < len(self.keys)
        old[inb] = self.keys[pos[inb]] == ukey[inb]
        self.moments[pos[old]] += sums[old]
        new = ~old
        if new.any():
            keys = np.concatenate([self.keys, ukey[new]])
            order = np.argsort(keys, kind="stable")
            self.keys = keys[order]
            self.moments = np.concatenate([self.moments, sums[new]])[order]
            self.rows = np.concatenate([self.rows, np.zeros((int(new.sum()), 8), np.float64)])[order]
        touched = np.searchsorted(self.keys, ukey)
        self.rows[touched] = self.derive_rows(self.keys[touched], self.moments[touched])
        self.counters["n_cells"] = len(self.keys)
        self.counters["n_planar"] = int((self.rows[:, 7] == 2.0).sum())

    def insert_frames(self, store_ref, poses):
        """Every frame of a loops.KeyframeStoreRef under its own row of poses [m, 7]: literally the loop of inserts."""
        poses = np.asarray(poses, dtype=np.float64).reshape(-1, 7)
        for e in range(min(len(store_ref.rows), len(poses))):
            self.insert(store_ref.rows[e][:store_ref.counts[e]], poses[e])

    def prune(self, center=None, radius=None, inner_radius=None, min_count=1):
        """Evict the cells that are not near or that are sparse (module docstring): the sorted arrays are filtered.
        No probe limit here, so n_lost stays 0."""
        r, ri, mc = check_surfel_prune(center, radius, inner_radius, min_count)
        keep = self.moments[:, 0] >= mc
        if center is not None:
            c = np.asarray(center, dtype=np.float64).reshape(-1)[:3]
            cell = np.stack([(self.keys >> 42) & 0x1fffff, (self.keys >> 21) & 0x1fffff, self.keys & 0x1fffff], axis=1) - _MAXC
            with np.errstate(all="ignore"):
                d = (cell.astype(np.float64) + 0.5) * self.voxel_size - c[None, :]
                d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
                keep = (keep | (d2 < ri * ri)) & (d2 < r * r)
        self.prune_counters["n_prunes"] += 1
        self.prune_counters["n_evicted"] += int((~keep).sum())
        self.keys, self.moments, self.rows = self.keys[keep], self.moments[keep], self.rows[keep]
        self.counters["n_cells"] = len(self.keys)
        self.counters["n_planar"] = int((self.rows[:, 7] == 2.0).sum())

    def prune_stats(self):
        return dict(self.prune_counters)

    def cells(self, min_flag=1):
        """(keys int64 [M], moments int64 [M, 10], rows float64 [M, 8]) of the cells with flag >= min_flag, sorted by key"""
        sel = self.rows[:, 7] >= float(min_flag)
        return self.keys[sel], self.moments[sel], self.rows[sel]

    def _match(self, points, pose, max_dist, min_flag=2):
        """-> (world [P, 3], index [P] into the cell arrays (-1: no match), d2 [P] (-1.0: no match)); the candidates are
        the cells with flag >= min_flag (2: the planar ones)"""
        md = _max_dist_of(max_dist, self.voxel_size)
        status, key, w = self._cells(points, pose)
        P = len(status)
        best = np.full((P,), -1, np.int64)
        bd2 = np.full((P,), np.inf, np.float64)
        bkey = np.full((P,), np.iinfo(np.int64).max, np.int64)
        if len(self.keys):
            ok = status == 0
            c = [(key >> 42) & 0x1fffff, (key >> 21) & 0x1fffff, key & 0x1fffff]
            last = len(self.keys) - 1
            planar = self.rows[:, 7] >= float(min_flag)
            with np.errstate(all="ignore"):
                for dx in (-1, 0, 1):
                    for dy in (-1, 0, 1):
                        for dz in (-1, 0, 1):
                            x, y, z = c[0] + dx, c[1] + dy, c[2] + dz
                            valid = ok & (x >= 1) & (x <= 0x1fffff) & (y >= 1) & (y <= 0x1fffff) & (z >= 1) & (z <= 0x1fffff)
                            nk = (x << 42) | (y << 21) | z
                            pos = np.minimum(np.searchsorted(self.keys, nk), last)
                            hit = valid & (self.keys[pos] == nk) & planar[pos]
                            d = w - self.rows[pos, :3]
                            d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
                            better = hit & ((best < 0) | (d2 < bd2) | ((d2 == bd2) & (nk < bkey)))
                            best[better], bd2[better], bkey[better] = pos[better], d2[better], nk[better]
        with np.errstate(all="ignore"):
            acc = (best >= 0) & (bd2 < md * md)
        return w, np.where(acc, best, -1), np.where(acc, bd2, -1.0)

    def nearest(self, points, pose=None, max_dist=None, return_rows=False, cost="plane", min_flag=None, reg_rel=None,
                reg_abs=None, return_info=False):
        """(keys int64 [P], d2 float64 [P][, rows float64 [P, 8]][, info float64 [P, 8]]) of the nearest planar cell
        within max_dist (None: voxel_size) of every point; -1 / -1.0 / zeros without a match or for a skipped point.
        cost="distribution": the nearest cell with flag >= min_flag (default 1); return_info adds the rows of
        information() of the matched cells, zeros without a match."""
        dist = check_cost(cost, min_flag, reg_rel, reg_abs)
        if dist is None and return_info:
            raise ValueError("return_info needs cost=\"distribution\"")
        _, idx, d2 = self._match(points, pose, max_dist, 2 if dist is None else dist[0])
        got = idx >= 0
        keys = np.full((len(idx),), -1, np.int64)
        keys[got] = self.keys[idx[got]]
        out = [keys, d2]
        if return_rows:
            rows = np.zeros((len(idx), 8), np.float64)
            rows[got] = self.rows[idx[got]]
            out.append(rows)
        if return_info:
            info = np.zeros((len(idx), 8), np.float64)
            info[got] = self.information(idx[got], dist[1], dist[2])
            out.append(info)
        return tuple(out)

    def information(self, idx_or_keys, reg_rel=DIST_DEFAULTS["reg_rel"], reg_abs=DIST_DEFAULTS["reg_abs"]):
        """[n, 8] float64 rows {M00, M01, M02, M11, M12, M22, det, lam} of the given cells -- indices into the cell
        arrays, or packed keys (a key is >= 2^42) -- by the rules of "Distribution cost": the covariance of the cell's
        moments in metres, lam = reg_rel * trace + reg_abs^2 on the diagonal, inverted by the adjugate, operation by
        operation the device's sf_information.  A row whose det fails det > 0 && det < inf is unusable: its six M
        entries are zeros."""
        _, rr, ra = check_cost("distribution", None, reg_rel, reg_abs)
        at = np.asarray(idx_or_keys, np.int64).reshape(-1)
        is_key = at >= (1 << 42)
        if is_key.any():
            pos = np.minimum(np.searchsorted(self.keys, at), max(len(self.keys) - 1, 0))
            if len(self.keys) == 0 or (self.keys[pos] != at)[is_key].any():
                raise ValueError("information: a key that is not in the map")
            at = np.where(is_key, pos, at)
        _, c, _ = covariances(self.moments[at])
        out = np.zeros((len(at), 8), np.float64)
        with np.errstate(all="ignore"):
            u = self.voxel_size / Q
            C = [(c[:, k] * u) * u for k in range(6)]
            lam = rr * ((C[0] + C[3]) + C[5]) + ra * ra
            S00, S01, S02, S11, S12, S22 = C[0] + lam, C[1], C[2], C[3] + lam, C[4], C[5] + lam
            A = [S11 * S22 - S12 * S12, S02 * S12 - S01 * S22, S01 * S12 - S02 * S11,
                 S00 * S22 - S02 * S02, S01 * S02 - S00 * S12, S00 * S11 - S01 * S01]
            det = (S00 * A[0] + S01 * A[1]) + S02 * A[2]
            usable = (det > 0.0) & (det < np.inf)
            for k in range(6):
                out[:, k] = np.where(usable, A[k] / np.where(usable, det, 1.0), 0.0)
        out[:, 6], out[:, 7] = det, lam
        return out

    def _pair_terms(self, points, pose, max_dist=None, dist=None):
        """The addends of normal_equations, one row per matched point in input order: [K, 28] = H upper triangle (21),
        g (6), cost of the plane term with the cell's normal.  dist = (min_flag, reg_rel, reg_abs): of the distribution
        term with the cell's information matrix instead, one row per USABLE pair (gauss_newton.info_terms)."""
        posev = np.asarray([0, 0, 0, 1, 0, 0, 0] if pose is None else pose, dtype=np.float64).reshape(7)
        if dist is not None:
            w, idx, _ = self._match(points, posev, max_dist, dist[0])
            sel = np.nonzero(idx >= 0)[0]
            info = self.information(idx[sel], dist[1], dist[2])
            use = (info[:, 6] > 0.0) & (info[:, 6] < np.inf)
            sel, info = sel[use], info[use]
            return info_terms(w[sel], w[sel] - self.rows[idx[sel], :3], info[:, :6])
        w, idx, _ = self._match(points, posev, max_dist)
        sel = np.nonzero(idx >= 0)[0]
        w = w[sel]
        d = w - self.rows[idx[sel], :3]
        n = self.rows[idx[sel], 3:6]
        J = np.zeros((len(sel), 3, 6), np.float64)
        r = np.zeros((len(sel), 3), np.float64)
        J[:, 0, :3], J[:, 0, 3:] = n, np.cross(w, n)
        r[:, 0] = n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1] + n[:, 2] * d[:, 2]
        return terms_of(J, r)

    def _weighted_terms(self, points, pose, max_dist=None, robust_scale=0.0, dist=None):
        scale = check_scale(robust_scale)
        return robust_weighted(self._pair_terms(points, pose, max_dist, dist), scale)

    def normal_equations(self, points, pose, max_dist=None, robust_scale=0.0, cost="plane", min_flag=None, reg_rel=None,
                         reg_abs=None):
        """[29] float64: the column sums of _pair_terms (weighted when robust_scale > 0), then the number of pairs.
        cost="distribution": of the distribution terms (robust_scale is then in sigmas)."""
        dist = check_cost(cost, min_flag, reg_rel, reg_abs)
        terms = self._weighted_terms(points, pose, max_dist, robust_scale, dist)
        return np.concatenate([terms.sum(axis=0), [float(len(terms))]])

    def register(self, points, pose, iters=4, max_dist=None, damping=0.0, min_pairs=50, tol_t=0.0, tol_r=0.0,
                 robust_scale=0.0, cost="plane", min_flag=None, reg_rel=None, reg_abs=None):
        """-> (pose [7] float64, info [iters, 8]): the loop of mapping.VoxelMapRef.register on the plane terms above, or
        with cost="distribution" on the distribution terms."""
        dist = check_cost(cost, min_flag, reg_rel, reg_abs)
        cost_kw = {} if dist is None else dict(cost="distribution", **_dist_kw(dist))
        _check_register(iters, tol_t, tol_r)
        check_scale(robust_scale)
        _max_dist_of(max_dist, self.voxel_size)
        return register_loop(lambda at: self.normal_equations(points, at, max_dist, robust_scale, **cost_kw), pose, iters,
                             damping, min_pairs, tol_t, tol_r)

    def stats(self):
        return dict(self.counters, dropped_full=0)

    def save_ply(self, path, min_flag=2):
        write_surfel_ply(path, self.cells(min_flag)[2])


class SurfelMap(_DeviceTable):
    """The device surfel map: owns the table (one allocation of rslo_surfel_bytes(capacity) bytes) and the insert and
    registration workspaces, which grow only when a larger scan arrives, and prune's workspace (about one more table),
    allocated by the first prune() or by reserve_prune().  insert / insert_frames / nearest / normal_equations /
    register / prune enqueue on the current stream and read nothing on the host; cells(), stats() and prune_stats()
    make one host read each."""

    _CAPI = "surfel"

    def __init__(self, voxel_size=0.4, capacity=1 << 20, device="cuda", min_range=0.0, max_range=float("inf"),
                 min_points=5, planar_ratio=0.1, line_ratio=0.05):
        super().__init__(voxel_size, capacity, device, min_range, max_range, min_points=min_points,
                         planar_ratio=planar_ratio, line_ratio=line_ratio)

    def _set_params(self, min_points, planar_ratio, line_ratio):
        self.min_points, self.planar_ratio, self.line_ratio = _check_plane_params(min_points, planar_ratio, line_ratio)

    def reset(self):
        """Empty the table; every counter restarts at 0."""
        from rslo_amd import capi
        capi.surfel_reset(self._buf, self.capacity, self.voxel_size, self.min_range, self.max_range, self.min_points,
                          self.planar_ratio, self.line_ratio)

    def reserve(self, n_points):
        """Size the workspaces for scans of up to n_points points, so that later calls allocate nothing."""
        from rslo_amd import capi
        if n_points > self._ws_points:
            self._ws = capi.surfel_insert_ws(int(n_points), self.device)
            self._reg_ws = capi.surfel_register_ws(int(n_points), self.device)
            self._ws_points = int(n_points)

    def insert(self, points, pose=None):
        """One scan (fp32 CUDA [P, F >= 3], read in place; only x, y, z are read) under pose (t, q wxyz)."""
        from rslo_amd import capi
        self.reserve(points.shape[0])
        capi.surfel_insert(self._buf, points, self._pose(pose), self._ws)

    def nearest(self, points, pose=None, max_dist=None, return_rows=False, cost="plane", min_flag=None, reg_rel=None,
                reg_abs=None, return_info=False):
        """(keys int64 [P], d2 float64 [P][, rows float64 [P, 8]][, info float64 [P, 8]]) on the device; -1 / -1.0 /
        zeros without a match.  cost="distribution": among the cells with flag >= min_flag (default 1); return_info adds
        the information-matrix rows {M00, M01, M02, M11, M12, M22, det, lam} of the matched cells."""
        from rslo_amd import capi
        dist = check_cost(cost, min_flag, reg_rel, reg_abs)
        md = _max_dist_of(max_dist, self.voxel_size)
        if dist is None:
            if return_info:
                raise ValueError("return_info needs cost=\"distribution\"")
            return capi.surfel_nearest(self._buf, points, self._pose(pose), self.voxel_size, md,
                                       rows=True if return_rows else None)
        return capi.surfel_nearest_d(self._buf, points, self._pose(pose), self.voxel_size, md, *dist,
                                     rows=True if return_rows else None, info=True if return_info else None)

    def normal_equations(self, points, pose, max_dist=None, robust_scale=0.0, cost="plane", min_flag=None, reg_rel=None,
                         reg_abs=None):
        """float64 CUDA [29]: the upper triangle of H (21), g (6), cost, pairs of the matched points at pose.
        cost="distribution": of the distribution terms (robust_scale is then in sigmas)."""
        from rslo_amd import capi
        dist = check_cost(cost, min_flag, reg_rel, reg_abs)
        md = _max_dist_of(max_dist, self.voxel_size)
        scale = check_scale(robust_scale)
        self.reserve(points.shape[0])
        if dist is None:
            return capi.surfel_normal_eq(self._buf, points, self._pose(pose), self.voxel_size, md, scale, ws=self._reg_ws)
        return capi.surfel_normal_eq_d(self._buf, points, self._pose(pose), self.voxel_size, md, *dist, robust_scale=scale,
                                       ws=self._reg_ws)

    def register(self, points, pose, iters=4, max_dist=None, damping=0.0, min_pairs=50, tol_t=0.0, tol_r=0.0,
                 robust_scale=0.0, info=None, cost="plane", min_flag=None, reg_rel=None, reg_abs=None):
        """`iters` Gauss-Newton iterations of points (fp32 CUDA [P, F >= 3], read in place) against the planar cells, on
        the device; cost="distribution": against every cell with flag >= min_flag (default 1) under the
        point-to-distribution cost (include/rslo_hip.h "Distribution cost"; robust_scale is then in sigmas).  pose: a
        float64 CUDA [7] tensor (a trajectory row) is updated IN PLACE and returned; anything else is copied to the
        device first.  -> (pose [7], info [iters, 8]) device tensors; info may be preallocated.  No host read, nothing
        allocated after a reserve() when info is given."""
        from rslo_amd import capi
        dist = check_cost(cost, min_flag, reg_rel, reg_abs)
        _check_register(iters, tol_t, tol_r)
        md = _max_dist_of(max_dist, self.voxel_size)
        scale = check_scale(robust_scale)
        self.reserve(points.shape[0])
        pose = self._identity.clone() if pose is None else self._pose(pose)
        if dist is None:
            info = capi.surfel_register(self._buf, points, pose, self.voxel_size, iters, md, damping, min_pairs, tol_t,
                                        tol_r, scale, info=info, ws=self._reg_ws)
        else:
            info = capi.surfel_register_d(self._buf, points, pose, self.voxel_size, iters, md, damping, min_pairs, tol_t,
                                          tol_r, scale, *dist, info=info, ws=self._reg_ws)
        return pose, info

    def prune(self, center=None, radius=None, inner_radius=None, min_count=1):
        """Evict the cells whose centre is not within radius of center, or that hold fewer than min_count points and
        lie at least inner_radius (None: radius) from it (module docstring).  center: None, a sequence, or a float64
        CUDA tensor of >= 3 elements that is read in place (a [7] trajectory row).  Enqueued on the current stream; no
        host read, and nothing allocated after reserve_prune() when center is a device tensor (or None): capturable."""
        from rslo_amd import capi
        r, ri, mc = check_surfel_prune(center, radius, inner_radius, min_count)
        self.reserve_prune()
        capi.surfel_prune(self._buf, self._prune_ws, self._center(center, exact=False), r, ri, mc)

    def cells(self, min_flag=1, center=None, radius=None):
        """(keys int64 [M], moments int64 [M, 10], rows float64 [M, 8]) of the cells with flag >= min_flag (and whose mean
        lies within radius of center, when one is given), sorted by key: deterministic bit for bit.  One host read (M)."""
        import torch
        from rslo_amd import capi
        if center is not None and radius is None:
            raise ValueError("cells: a center needs a radius")
        center = self._center(center, exact=True)
        r = 0.0 if radius is None else float(radius)
        M = int(capi.surfel_export(self._buf, min_flag, center, r)[0])      # count only; nothing else changes the map meanwhile
        keys = torch.empty((M,), dtype=torch.int64, device=self.device)
        moments = torch.empty((M, 10), dtype=torch.int64, device=self.device)
        rows = torch.empty((M, 8), dtype=torch.float64, device=self.device)
        if M:
            capi.surfel_export(self._buf, min_flag, center, r, keys, moments, rows)
            keys, order = torch.sort(keys)
            moments, rows = moments[order], rows[order]
        return keys, moments, rows

    def stats(self):
        """The seven counters of the header as a dict (one host read)."""
        from rslo_amd import capi
        return self._header(capi.SURFEL_HDR_COUNTERS, COUNTERS)

    def save_ply(self, path, min_flag=2):
        write_surfel_ply(path, self.cells(min_flag)[2].cpu().numpy())
