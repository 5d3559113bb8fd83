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

The map after loop closure, on both classes and on the pyramids (rslo_map_insert_frames):

    vmap.reset(); vmap.insert_frames(store, poses)             # every keyframe of a loops.KeyframeStore under its own pose

  * insert_frames(store, poses [m, 7]): n = min(the store's entry count, m); the map is left as the n calls
    insert(rows_e[:count_e], poses[e]), e = 0 .. n-1, leave it -- VoxelMapRef.insert_frames IS that loop over a
    KeyframeStoreRef -- so row i of frame e has tag ((S0 + e) << 32) | i with S0 = n_scans before the call, an empty
    frame still counts as a scan, a pose row that is not finite drops its frame's valid points (dropped_range), and the
    map's own range gate applies.  The device does it in three launches with no host read, one thread per (frame,
    row): the content of a map does not depend on the order of insertion (the smallest tag wins, hits and counters are
    integer sums), so the result is the loop's to the bit.  The rebuilt map has the density of the keyframes.

Rolling local map (rules: include/rslo_hip.h "Rolling local map"), on both classes:

    vmap.prune(center=pose, radius=100.0)                      # forget what is not within 100 m of the sensor
    vmap.prune(min_hits=2, grace=5)                            # forget cells hit once that are at least 5 scans old
    runner = inference.OdometryRunner(net, voxel_map=vmap, local_map=dict(radius=100.0, every=10))

  * prune(center=None, radius=None, min_hits=1, grace=0), S = n_scans at the time of the call.  A stored cell with row
    (x, y, z, .), tag and hits is KEPT iff both hold.  Near: center is None, or d2 < radius*radius with
    dx = float64(x) - c[0], dy, dz likewise, d2 = dx*dx + dy*dy + dz*dz summed left to right -- the test of
    points(center=, radius=); a comparison that is false evicts (a NaN centre coordinate, radius == 0), radius = +inf
    keeps every cell; radius < 0 or NaN (here even without a center, where rslo_map_prune ignores the radius), or a
    center without a radius, is a ValueError and writes nothing.  Not sparse:
    hits >= min_hits, or S - 1 - (tag >> 32) < grace (created fewer than `grace` scans ago: still young);
    min_hits >= 1 and grace >= 0 are integers, with min_hits = 1 nothing is sparse;
  * every other cell is EVICTED: key, tag, row and hits are gone, lookup reads 0, nearest does not see it, a later
    insert creates it afresh (new tag, hits from zero).  Kept cells keep tag, row and hits to the bit.  n_cells becomes
    the number of kept cells, the other five counters of stats() are cumulative and do not change;
  * prune_stats() -> {n_prunes, n_evicted, n_lost}: calls, cells evicted so far, and -- device map only -- kept cells
    that found no slot within 128 probes when the table was rebuilt (dropped whole; impossible while the survivors'
    longest run of occupied slots is below 128; VoxelMapRef has no capacity: always 0).  reset() zeroes them.

Free-space carving (csrc/carve.hip; rules: include/rslo_hip.h "Free-space carving"; the image: rslo_amd/carve.py), on
both classes and on the pyramids, which apply the one image to every level:

    ri = carve.RangeImage(rows=64, cols=1024)                  # the range image of a scan, on the device
    vmap.carve(ri(scan), pose)                                 # forget the cells the scan at `pose` sees through
    ref.carve(carve.range_image_ref(scan), pose)               # VoxelMapRef takes the uint32 [H, W] array

  * carve(image, pose, tan_lo=None, tan_hi=None, win_rows=1, win_cols=1, margin_abs=0.3, margin_rel=0.0, max_range=60.0,
    grace=1); tan_lo / tan_hi None: those of a RangeImage, else carve.CARVE_DEFAULTS.  S = n_scans at the time of the
    call.  A stored cell with row (x, y, z, .) and tag is EVICTED iff all of these hold -- a comparison that is false
    keeps the cell, so a NaN pose carves nothing.  Old enough: S - 1 - (tag >> 32) >= grace.  In view:
    d = float64(row.xyz) - t; p = rotate(conj(q), d) with conj(q) = (w, -x, -y, -z), q not renormalised;
    rho2 = p.x*p.x + p.y*p.y > 0; r_m = sqrt(rho2 + p.z*p.z) < max_range (+inf allowed); p has a pixel (row, col) by
    carve.pixel_ref.  Observed: that pixel is not empty.  Seen through: with m the minimum of the non-empty pixels in
    the window rows row +- win_rows (clipped) x columns col +- win_cols (wrapped modulo W),
    float64(float32_of(m)) - r_m > margin_abs + margin_rel * r_m.  The window is what keeps the ground: at grazing
    incidence its range changes by metres across one pixel of elevation, and the nearer return in the row below
    protects the cell;
  * evicted cells are gone exactly as after a prune, kept cells keep tag, row and hits to the bit, n_cells is recounted;
    carve_stats() -> {n_carves, n_carved}; n_lost (prune_stats) is added to as in the prune, n_prunes and n_evicted do
    not move.  A call that evicts nothing leaves the device table as it is, to the byte.  An argument outside its
    range (carve.check_image, carve.check_rule) is a ValueError and writes nothing.

Scan-to-map registration (csrc/mapreg.hip; rules: include/rslo_hip.h "Scan-to-map registration") reads the map back, on
both classes:

    tags, d2 = vmap.nearest(scan, pose, max_dist=0.3)          # the exact nearest stored point within max_dist <= voxel_size
    pose, info = vmap.register(scan, pose, iters=5)            # Gauss-Newton on the device, pose (a trajectory row) in place

  * nearest: the candidates of a point are the stored cells c + {-1,0,1}^3 around its cell with hits >= min_hits;
    d2 = |w - float64(row.xyz)|^2 summed left to right; the smallest d2 wins, then the smallest tag; accepted when
    d2 < max_dist^2.  max_dist <= voxel_size makes the 27 cells sufficient, so this is the exact nearest stored point;
  * normal_equations -> [29]: the upper triangle of H (21), g (6), cost, pairs of the matched points at a pose, for the
    world-frame twist (dt, dtheta).  metric "plane": a point whose scan normal (columns 4..6) has n.n >= 0.25
    contributes one row a = (n, w x n), r = n . (w - m), n = the normal rotated by the pose (held fixed over the
    step); every other matched point -- and every point under metric "point" -- contributes the three rows of
    J = [I | -[w]x] with residual w - m.  The fallback matters: the reader zeroes exactly vertical normals, and a
    world whose ground is level would otherwise leave z, roll and pitch unobserved;
  * register: per iteration M = H + damping * I by row-by-row Cholesky, delta = -M^-1 g, q' = normalize(dq (x) q),
    t' = dt + rotate(dq, t); info rows {status, pairs, cost, |dt|, theta, 0, 0, 0}, status 0 step, 1 fewer than
    min_pairs pairs, 2 not positive definite, 3 skipped after an iteration with |dt| < tol_t and theta < tol_r.
The device sums run in a fixed order but not in numpy's: the sums agree within the bound of a reordered float64 sum,
the matches and the pair count exactly.

Coarse-to-fine robust registration (rules: include/rslo_hip.h "Robust weight" and "Scheduled register"), on both classes
and on the pyramids MapPyramid (device) / MapPyramidRef (numpy):

    pose, info = vmap.register(scan, pose, iters=5, robust_scale=0.2)          # Geman-McClure weights
    pyr = MapPyramid(voxel_sizes=(0.8, 0.4, 0.2), capacity=1 << 22)             # one VoxelMap per level, coarse to fine
    pyr.insert(scan, pose)                                                      # ... every level
    pose, info = pyr.register(scan, pose, schedule=pyr.default_schedule(4))     # stages in order on the one pose

  * robust weight: a matched point whose term (plane or point, as above) has the cost addend e gets
    s2 = scale*scale, u = s2 / (s2 + e), rho = u*u, and each of its 28 addends is the addend above times rho; the pair
    count stays the unweighted count; cost is the weighted cost.  robust_scale = 0: no weights, today's bits.
    scale < 0, NaN, inf, or a positive scale whose square is not a positive finite float64: ValueError;
  * a schedule is a sequence of stages (level, iters, max_dist or None, robust_scale); max_dist None = the level's
    voxel size, and 0 < max_dist <= that voxel size always.  The stages run in order on the one pose; a met tolerance
    skips the rest of its stage only (status 3), the next stage starts afresh.  info [sum of iters, 8], rows
    {status, pairs, cost, |dt|, theta, stage, level, 0}; the iterations of all stages sum to 1 .. 64, at most 8 levels;
  * why a pyramid: the 27-cell search is exact only for max_dist <= voxel_size, so a start further off than one cell
    edge of the fine map finds no correct pair.  A coarser map of the same scans widens the basin at the same 27 probes
    per point; robust weights keep the coarse stages from pulling a good start away.
"""
import numpy as np

from . import se3
from .gauss_newton import point_jacobian, register_loop, robust_weighted, terms_of

COUNTERS = ("n_scans", "n_cells", "n_points", "dropped_invalid", "dropped_range", "dropped_full")
PRUNE_COUNTERS = ("n_prunes", "n_evicted", "n_lost")
CARVE_COUNTERS = ("n_carves", "n_carved")
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


def _metric_of(metric, width):
    """None: "plane" for a cloud that carries normals (>= 7 columns), else "point" """
    if metric is None:
        metric = "plane" if width >= 7 else "point"
    if metric not in ("point", "plane"):
        raise ValueError("metric must be \"point\" or \"plane\", got %r" % (metric,))
    if metric == "plane" and width < 7:
        raise ValueError("metric \"plane\" reads the normals at columns 4..6: the points have %d columns" % width)
    return metric


def _max_dist_of(max_dist, voxel_size):
    md = voxel_size if max_dist is None else float(max_dist)
    if not (0.0 < md <= voxel_size):
        raise ValueError("need 0 < max_dist <= voxel_size = %g, got %r" % (voxel_size, max_dist))
    return md


def check_prune(center, radius, min_hits, grace, has_center=None):
    """The argument errors of prune (ValueError), raised before anything is written; -> radius as a float (0.0 when
    None).  has_center: whether a centre will be given, for callers that validate before they have one (default:
    center is not None).  Stricter than rslo_map_prune in one point: a negative or NaN radius is refused without a
    centre too, where the C call ignores the radius."""
    if has_center is None:
        has_center = center is not None
    if has_center and radius is None:
        raise ValueError("prune: a center needs a radius")
    r = 0.0 if radius is None else float(radius)
    if not r >= 0.0:
        raise ValueError("prune: radius must be >= 0 (NaN is refused), got %r" % (radius,))
    if int(min_hits) != min_hits or int(grace) != grace or min_hits < 1 or grace < 0:
        raise ValueError("prune: min_hits >= 1 and grace >= 0 must be integers, got %r and %r" % (min_hits, grace))
    return r


def check_local_map(options, voxel_map, surfels):
    """The local_map= options of an OdometryRunner against the maps it was given (ValueError): -> dict(radius, every,
    min_hits, grace), plus surfels=dict(min_count, inner_radius) when the surfels key asks for the surfel map to be
    pruned too (True: its defaults).  Without that key a voxel_map is required; with it, surfels is."""
    from .surfels import check_surfel_prune
    o = dict(options)
    surfel_prune = o.pop("surfels", None)
    if surfel_prune is None or surfel_prune is False:
        surfel_prune = None
        if voxel_map is None:
            raise ValueError("local_map needs a voxel_map to prune")
    else:
        if surfels is None:
            raise ValueError("local_map's surfels key needs surfels=SurfelMap(...) to prune")
        surfel_prune = {} if surfel_prune is True else dict(surfel_prune)
        unknown = set(surfel_prune) - {"min_count", "inner_radius"}
        if unknown:
            raise ValueError("local_map surfels takes min_count and inner_radius; got %s" % sorted(unknown))
    unknown = set(o) - {"radius", "every", "min_hits", "grace"}
    if unknown:
        raise ValueError("local_map takes radius, every, min_hits, grace and surfels; got %s" % sorted(unknown))
    if "radius" not in o:
        raise ValueError("local_map needs a radius")
    every, min_hits, grace = o.get("every", 1), o.get("min_hits", 1), o.get("grace", 0)
    if int(every) != every or every < 1:
        raise ValueError("local_map every must be an integer >= 1, got %r" % (every,))
    radius = check_prune(None, o["radius"], min_hits, grace, has_center=True)
    out = dict(radius=radius, every=int(every), min_hits=int(min_hits), grace=int(grace))
    if surfel_prune is not None:
        _, inner, min_count = check_surfel_prune(None, radius, surfel_prune.get("inner_radius"),
                                                 surfel_prune.get("min_count", 1), has_center=True)
        out["surfels"] = dict(min_count=min_count, inner_radius=inner)
    return out


def check_carve_call(image, tan_lo, tan_hi, win_rows, win_cols, margin_abs, margin_rel, max_range, grace):
    """The argument errors of carve (ValueError), raised before anything is written.  image: anything with a 2-D .shape,
    or a carve.RangeImage, whose tangents stand in for tan_lo / tan_hi = None (else carve.CARVE_DEFAULTS).
    -> (H, W, tan_lo, tan_hi, win_rows, win_cols, margin_abs, margin_rel, max_range, grace)"""
    from . import carve as carve_mod
    shape = tuple(getattr(getattr(image, "img", image), "shape", ()))
    if len(shape) != 2:
        raise ValueError("carve: the image must be [rows, cols], got shape %r" % (shape,))
    tan_lo = getattr(image, "tan_lo", carve_mod.CARVE_DEFAULTS["tan_lo"]) if tan_lo is None else tan_lo
    tan_hi = getattr(image, "tan_hi", carve_mod.CARVE_DEFAULTS["tan_hi"]) if tan_hi is None else tan_hi
    return carve_mod.check_image(int(shape[0]), int(shape[1]), tan_lo, tan_hi) + carve_mod.check_rule(
        win_rows, win_cols, margin_abs, margin_rel, max_range, grace)


def _check_register(iters, tol_t, tol_r):
    if not 1 <= int(iters) <= 32:
        raise ValueError("register: iters must be in 1 .. 32")
    if not (float(tol_t) >= 0.0 and float(tol_r) >= 0.0):
        raise ValueError("register: tol_t and tol_r must be >= 0")


def check_scale(scale):
    """robust_scale: 0.0 (no weights) or positive with a positive finite square; -> float (ValueError otherwise)"""
    sc = float(scale)
    s2 = sc * sc
    if not (sc == 0.0 or (sc > 0.0 and 0.0 < s2 < float("inf"))):
        raise ValueError("robust_scale must be 0 (no weights) or positive with a finite, non-zero square, got %r" % (scale,))
    return sc


MAX_LEVELS = 8
MAX_SCHEDULE_ITERS = 64


def check_schedule(schedule, voxel_sizes):
    """-> [(level, iters, max_dist, robust_scale)] with every max_dist a float; ValueError for a level outside the
    pyramid, iters < 1, max_dist outside (0, voxel of the level], a bad scale, or more than 64 iterations in all."""
    stages = []
    total = 0
    for st in schedule:
        if len(st) != 4:
            raise ValueError("schedule: a stage is (level, iters, max_dist or None, robust_scale), got %r" % (st,))
        level, iters, max_dist, scale = st
        if int(level) != level or not 0 <= level < len(voxel_sizes):
            raise ValueError("schedule: level %r is not one of the pyramid's %d levels" % (level, len(voxel_sizes)))
        if int(iters) != iters or iters < 1:
            raise ValueError("schedule: a stage needs iters >= 1, got %r" % (iters,))
        total += int(iters)
        stages.append((int(level), int(iters), _max_dist_of(max_dist, voxel_sizes[int(level)]), check_scale(scale)))
    if not 1 <= total <= MAX_SCHEDULE_ITERS:
        raise ValueError("schedule: the iterations of all stages must sum to 1 .. %d, got %d" % (MAX_SCHEDULE_ITERS, total))
    return stages


def _check_pyramid(voxel_sizes, capacity=None):
    voxel_sizes = tuple(float(v) for v in voxel_sizes)
    if not 1 <= len(voxel_sizes) <= MAX_LEVELS:
        raise ValueError("a pyramid has 1 .. %d levels" % MAX_LEVELS)
    if any(not b < a for a, b in zip(voxel_sizes, voxel_sizes[1:])):
        raise ValueError("voxel_sizes must be ordered coarse to fine (strictly decreasing), got %r" % (voxel_sizes,))
    if capacity is None:
        return voxel_sizes
    caps = [capacity] * len(voxel_sizes) if np.ndim(capacity) == 0 else list(capacity)
    if len(caps) != len(voxel_sizes):
        raise ValueError("capacity is an int or one value per level")
    return voxel_sizes, [int(c) for c in caps]


REFINE_KEYS = ("max_dist", "min_hits", "damping", "min_pairs", "tol_t", "tol_r")


def check_refine(refine, voxel_map):
    """The refine= options of an OdometryRunner against the map it was given (ValueError): -> (keyword arguments of
    voxel_map.register, info rows per scan).  A VoxelMap takes iters= (default 5) and the keywords of VoxelMap.register;
    a pyramid takes schedule= (default: its default_schedule()) and no iters= / max_dist=, which the stages carry."""
    refine = dict(refine)
    pyramid = isinstance(voxel_map, _PyramidBase)
    if "iters" in refine and "schedule" in refine:
        raise ValueError("refine: iters= and schedule= exclude each other (a schedule carries its iterations)")
    if "schedule" in refine and not pyramid:
        raise ValueError("refine: schedule= needs a MapPyramid as voxel_map")
    allowed = set(REFINE_KEYS) | {"robust_scale", "iters"}
    if pyramid:
        allowed = (set(REFINE_KEYS) - {"max_dist"}) | {"schedule"}
    unknown = set(refine) - allowed
    if unknown:
        raise ValueError("refine takes %s (the metric is chosen by the input's width); got %s"
                         % (", ".join(sorted(allowed)), sorted(unknown)))
    if pyramid:
        stages = check_schedule(voxel_map.default_schedule() if refine.get("schedule") is None else refine["schedule"],
                                voxel_map.voxel_sizes)
        refine["schedule"] = stages
        return refine, sum(st[1] for st in stages)
    refine.setdefault("iters", 5)
    return refine, int(refine["iters"])


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
        self.prune_counters = dict.fromkeys(PRUNE_COUNTERS, 0)
        self.carve_counters = dict.fromkeys(CARVE_COUNTERS, 0)

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
            w = pose[None, :3] + se3.rotate(pose[3:], p)
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

    @staticmethod
    def _frame_poses(store_ref, poses):
        return np.asarray(poses, dtype=np.float64).reshape(-1, 7)

    def insert_frames(self, store_ref, poses):
        """Every frame of a loops.KeyframeStoreRef under its own row of poses [m, 7]: the definition (module docstring)."""
        poses = self._frame_poses(store_ref, poses)
        for e in range(min(len(store_ref.rows), len(poses))):
            self.insert(store_ref.rows[e][:store_ref.counts[e]], poses[e])

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

    def prune(self, center=None, radius=None, min_hits=1, grace=0):
        """Evict the cells that are not near or that are sparse (module docstring): the sorted arrays are filtered."""
        r = check_prune(center, radius, min_hits, grace)
        young = (self.counters["n_scans"] - 1 - (self.tags >> 32)) < int(grace)
        keep = (self.hits >= int(min_hits)) | young
        if center is not None:
            c = np.asarray(center, dtype=np.float64).reshape(-1)[:3]
            with np.errstate(all="ignore"):
                d = self.rows[:, :3].astype(np.float64) - c[None, :]
                keep &= (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]) < r * r
        self.prune_counters["n_prunes"] += 1
        self.prune_counters["n_evicted"] += int((~keep).sum())
        self.keys, self.tags, self.hits, self.rows = self.keys[keep], self.tags[keep], self.hits[keep], self.rows[keep]
        self.counters["n_cells"] = len(self.keys)

    def prune_stats(self):
        return dict(self.prune_counters)

    def carve_mask(self, image, pose, tan_lo=None, tan_hi=None, win_rows=1, win_cols=1, margin_abs=0.3, margin_rel=0.0,
                   max_range=60.0, grace=1):
        """bool, one per stored cell in the order of the cell arrays: the cells carve() would evict (module docstring);
        image: uint32 [H, W] (carve.range_image_ref)."""
        from . import carve as carve_mod
        H, W, tan_lo, tan_hi, win_rows, win_cols, margin_abs, margin_rel, max_range, grace = check_carve_call(
            image, tan_lo, tan_hi, win_rows, win_cols, margin_abs, margin_rel, max_range, grace)
        img = np.ascontiguousarray(np.asarray(image)).view(np.uint32).reshape(H, W)
        pose = np.asarray(pose, dtype=np.float64).reshape(7)
        with np.errstate(all="ignore"):
            old = (self.counters["n_scans"] - 1 - (self.tags >> 32)) >= grace
            d = self.rows[:, :3].astype(np.float64) - pose[None, :3]
            qc = np.array([pose[3], -pose[4], -pose[5], -pose[6]])
            p = se3.rotate(qc, d)
            rho2 = p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]
            r_m = np.sqrt(rho2 + p[:, 2] * p[:, 2])
            in_view = (rho2 > 0.0) & (r_m < max_range)
            has, row, col = carve_mod.pixel_ref(p, H, W, tan_lo, tan_hi)
            in_view &= has
            observed = img[row, col] != carve_mod.EMPTY
            m = carve_mod.window_min_ref(img, row, col, win_rows, win_cols)
            through = (m.view(np.float32).astype(np.float64) - r_m) > (margin_abs + margin_rel * r_m)
        return old & in_view & observed & through

    def carve(self, image, pose, **kw):
        """Evict the cells the scan behind `image` sees through from `pose` (module docstring), then rebuild like prune:
        the sorted arrays are filtered."""
        evict = self.carve_mask(image, pose, **kw)
        keep = ~evict
        self.carve_counters["n_carves"] += 1
        self.carve_counters["n_carved"] += int(evict.sum())
        self.keys, self.tags, self.hits, self.rows = self.keys[keep], self.tags[keep], self.hits[keep], self.rows[keep]
        self.counters["n_cells"] = len(self.keys)

    def carve_stats(self):
        return dict(self.carve_counters)

    def _match(self, points, pose, max_dist, min_hits):
        """-> (world [P, 3] float64, index [P] into the cell arrays (-1: no match), d2 [P] (-1.0: no match))"""
        md = _max_dist_of(max_dist, self.voxel_size)
        status, key, w = self._cells(points, pose)
        P = len(status)
        best = np.full((P,), -1, np.int64)
        bd2 = np.full((P,), np.inf, np.float64)
        btag = np.full((P,), np.iinfo(np.int64).max, np.int64)
        if len(self.keys):
            ok = status == 0
            c = [(key >> 42) & 0x1fffff, (key >> 21) & 0x1fffff, key & 0x1fffff]
            last = len(self.keys) - 1
            with np.errstate(all="ignore"):
                for dx in (-1, 0, 1):
                    for dy in (-1, 0, 1):
                        for dz in (-1, 0, 1):
                            x, y, z = c[0] + dx, c[1] + dy, c[2] + dz
                            valid = ok & (x >= 1) & (x <= 0x1fffff) & (y >= 1) & (y <= 0x1fffff) & (z >= 1) & (z <= 0x1fffff)
                            nk = (x << 42) | (y << 21) | z
                            pos = np.minimum(np.searchsorted(self.keys, nk), last)
                            hit = valid & (self.keys[pos] == nk) & (self.hits[pos] >= min_hits)
                            m = self.rows[pos, :3].astype(np.float64)
                            d = w - m
                            d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
                            tag = self.tags[pos]
                            better = hit & ((d2 < bd2) | ((d2 == bd2) & (tag < btag)))
                            best[better], bd2[better], btag[better] = pos[better], d2[better], tag[better]
        acc = (best >= 0) & (bd2 < md * md)
        return w, np.where(acc, best, -1), np.where(acc, bd2, -1.0)

    def nearest(self, points, pose=None, max_dist=None, min_hits=1, return_rows=False):
        """(tags int64 [P], d2 float64 [P][, rows fp32 [P, 4]]) of the nearest stored point within max_dist (None:
        voxel_size) of every point; -1 / -1.0 / zeros without a match or for a skipped point."""
        _, idx, d2 = self._match(points, pose, max_dist, min_hits)
        got = idx >= 0
        tags = np.full((len(idx),), -1, np.int64)
        tags[got] = self.tags[idx[got]]
        if not return_rows:
            return tags, d2
        rows = np.zeros((len(idx), 4), np.float32)
        rows[got] = self.rows[idx[got]]
        return tags, d2, rows

    def _pair_terms(self, points, pose, metric="plane", max_dist=None, min_hits=1, return_plane=False):
        """The addends of normal_equations, one row per matched point in input order: [K, 28] = H upper triangle (21),
        g (6), cost; return_plane=True adds the bool [K] of the rows that are plane terms."""
        pts = np.asarray(points)
        metric = _metric_of(metric, pts.shape[1] if pts.ndim == 2 else 0)
        posev = np.asarray([0, 0, 0, 1, 0, 0, 0] if pose is None else pose, dtype=np.float64).reshape(7)
        w, idx, _ = self._match(pts, posev, max_dist, min_hits)
        sel = np.nonzero(idx >= 0)[0]
        K = len(sel)
        w = w[sel]
        d = w - self.rows[idx[sel], :3].astype(np.float64)
        J = point_jacobian(w)                          # rows of the Jacobian; a plane term uses row 0 only
        r = d.copy()
        plane = np.zeros((K,), bool)
        if metric == "plane":
            with np.errstate(all="ignore"):
                ns = pts[sel, 4:7].astype(np.float64)
                plane = (ns[:, 0] * ns[:, 0] + ns[:, 1] * ns[:, 1] + ns[:, 2] * ns[:, 2]) >= 0.25
            ns, wp, dp = ns[plane], w[plane], d[plane]
            n = se3.rotate(posev[3:], ns)
            J[plane] = 0.0
            J[plane, 0, :3], J[plane, 0, 3:] = n, np.cross(wp, n)
            r[plane] = 0.0
            r[plane, 0] = n[:, 0] * dp[:, 0] + n[:, 1] * dp[:, 1] + n[:, 2] * dp[:, 2]
        terms = terms_of(J, r)
        return (terms, plane) if return_plane else terms

    def _weighted_terms(self, points, pose, metric="plane", max_dist=None, min_hits=1, robust_scale=0.0):
        """_pair_terms with every row multiplied by its Geman-McClure weight rho (module docstring); scale 0: as they are"""
        scale = check_scale(robust_scale)
        return robust_weighted(self._pair_terms(points, pose, metric, max_dist, min_hits), scale)

    def normal_equations(self, points, pose, metric="plane", max_dist=None, min_hits=1, robust_scale=0.0):
        """[29] float64: the column sums of _pair_terms (weighted when robust_scale > 0), then the number of pairs."""
        terms = self._weighted_terms(points, pose, metric, max_dist, min_hits, robust_scale)
        return np.concatenate([terms.sum(axis=0), [float(len(terms))]])

    def register(self, points, pose, iters=5, metric=None, max_dist=None, min_hits=1, damping=0.0, min_pairs=50,
                 tol_t=0.0, tol_r=0.0, robust_scale=0.0):
        """-> (pose [7] float64, info [iters, 8]); metric None: "plane" for points with normals, else "point"."""
        _check_register(iters, tol_t, tol_r)
        check_scale(robust_scale)
        pts = np.asarray(points)
        metric = _metric_of(metric, pts.shape[1] if pts.ndim == 2 else 0)
        return register_loop(lambda at: self.normal_equations(pts, at, metric, max_dist, min_hits, robust_scale), pose, iters,
                             damping, min_pairs, tol_t, tol_r)

    def stats(self):
        return dict(self.counters, dropped_full=0)

    def save_ply(self, path, min_hits=1):
        rows, _, hits = self.points(min_hits)
        write_ply(path, rows, hits)


class _DeviceTable:
    """What the device maps VoxelMap and surfels.SurfelMap share: the table's allocation, the workspace fields, the pose
    and centre arguments, insert_frames, prune's workspace and the header reads.  A subclass names its capi functions
    by their prefix (_CAPI) and brings reserve() and reset()."""

    _CAPI = None      # "map" / "surfel": capi.<_CAPI>_bytes, _insert_frames, _prune_ws and capi.<_CAPI upper>_HDR_PRUNE

    def __init__(self, voxel_size, capacity, device, min_range, max_range, **more):
        import torch
        from rslo_amd import capi
        self.voxel_size, self.min_range, self.max_range = _check_params(voxel_size, min_range, max_range)
        self._set_params(**more)
        self.capacity = int(capacity)
        nbytes = self._capi("bytes")(self.capacity)
        if nbytes == 0:
            raise capi.RsloHipError("%s: capacity must be a power of two >= 1024, got %r" % (type(self).__name__, capacity))
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._buf = torch.empty((nbytes // 8,), dtype=torch.int64, device=self.device)
        self._ws = None
        self._ws_points = -1
        self._prune_ws = None
        self._identity = torch.tensor([0, 0, 0, 1, 0, 0, 0], dtype=torch.float64, device=self.device)
        self.reserve(0)
        self.reset()

    def _set_params(self):
        """the subclass's own parameters, checked behind the three every table has"""

    def _capi(self, name):
        from rslo_amd import capi
        return getattr(capi, "%s_%s" % (self._CAPI, name))

    def _pose(self, pose):
        """a float64 CUDA [7] tensor as it is (a row of OdometryRunner's trajectory); None = identity; anything else is copied"""
        import torch
        if pose is None:
            return self._identity
        if torch.is_tensor(pose) and pose.is_cuda and pose.dtype == torch.float64:
            return pose
        return torch.as_tensor(np.asarray(pose, dtype=np.float64).reshape(7)).to(self.device)

    def _center(self, center, exact):
        """None or a float64 CUDA tensor as it is (read in place); anything else is copied to the device: its 3 values
        (exact: an export) or its first 3 (a prune, which also takes a [7] trajectory row)"""
        import torch
        if center is None or (torch.is_tensor(center) and center.is_cuda and center.dtype == torch.float64):
            return center
        host = np.asarray(center, dtype=np.float64)
        return torch.as_tensor(host.reshape(3) if exact else host.reshape(-1)[:3].copy()).to(self.device)

    def _frame_poses(self, store, poses):
        """a float64 CUDA [m, 7] contiguous tensor on this map's device as it is; anything else that is not a device
        tensor is copied to the device; a wrong device, dtype or shape is an error"""
        import torch
        from rslo_amd import capi
        name = type(self).__name__
        if store.device != self.device:
            raise capi.RsloHipError("%s.insert_frames: the keyframe store lives on %s, the map on %s"
                                    % (name, store.device, self.device))
        if not (torch.is_tensor(poses) and poses.is_cuda):
            host = np.asarray(poses.cpu() if torch.is_tensor(poses) else poses, dtype=np.float64)
            if host.ndim != 2 or host.shape[1] != 7:
                raise capi.RsloHipError("%s.insert_frames: poses must be [m, 7] rows (t, q wxyz), got %s" % (name, host.shape,))
            return torch.as_tensor(np.ascontiguousarray(host)).to(self.device)
        if poses.device != self.device:
            raise capi.RsloHipError("%s.insert_frames: the poses live on %s, the map on %s" % (name, poses.device, self.device))
        if poses.dtype != torch.float64 or poses.dim() != 2 or poses.shape[1] != 7:
            raise capi.RsloHipError("%s.insert_frames: poses must be float64 [m, 7] rows (t, q wxyz), got %s %s"
                                    % (name, poses.dtype, tuple(poses.shape)))
        return poses.contiguous()

    def insert_frames(self, store, poses):
        """Every frame of `store` (a loops.KeyframeStore) under its own row of poses -- float64 CUDA [m, 7], contiguous:
        read in place (optimized_trajectory() will do); anything else is copied -- as min(entries, m) successive insert()
        calls would leave the map (module docstring).  Three launches on the current stream, no host read, nothing
        allocated for a device tensor: capturable."""
        self._capi("insert_frames")(self._buf, store._buf, store.capacity, store.K, self._frame_poses(store, poses))

    def reserve_prune(self):
        """Allocate prune's workspace (about one more table) now, so that a later prune() allocates nothing."""
        if self._prune_ws is None:
            self._prune_ws = self._capi("prune_ws")(self.capacity, self.device)

    def _header(self, first_word, names):
        """the int64 header words first_word .. as a dict under `names` (one host read)"""
        vals = self._buf[first_word:first_word + len(names)].tolist()
        return dict(zip(names, (int(v) for v in vals)))

    def prune_stats(self):
        """{n_prunes, n_evicted, n_lost} of the map's header (one host read)."""
        from rslo_amd import capi
        return self._header(getattr(capi, "%s_HDR_PRUNE" % self._CAPI.upper()), PRUNE_COUNTERS)


class VoxelMap(_DeviceTable):
    """The device map: owns the table (one allocation of rslo_map_bytes(capacity) bytes) and the insert and registration
    workspaces, which grow only when a larger scan arrives, and prune's workspace (about one more table), allocated by
    the first prune() or by reserve_prune().  insert / lookup / overlap / nearest / normal_equations / register / prune
    enqueue on the current stream and read nothing on the host; points(), stats() and prune_stats() make one host read
    each."""

    _CAPI = "map"

    def __init__(self, voxel_size=0.2, capacity=1 << 22, device="cuda", min_range=0.0, max_range=float("inf")):
        super().__init__(voxel_size, capacity, device, min_range, max_range)

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
            self._reg_ws = capi.map_register_ws(int(n_points), self.device)      # normal_equations / register
            self._ws_points = int(n_points)

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

    def nearest(self, points, pose=None, max_dist=None, min_hits=1, return_rows=False):
        """(tags int64 [P], d2 float64 [P][, rows fp32 [P, 4]]) on the device: the exact nearest stored point within
        max_dist (None: voxel_size; at most voxel_size) of every point; -1 / -1.0 / zeros without a match."""
        from rslo_amd import capi
        md = _max_dist_of(max_dist, self.voxel_size)
        return capi.map_nearest(self._buf, points, self._pose(pose), self.voxel_size, md, min_hits,
                                rows=True if return_rows else None)

    def normal_equations(self, points, pose, metric="plane", max_dist=None, min_hits=1, robust_scale=0.0):
        """float64 CUDA [29]: the upper triangle of H (21), g (6), cost, pairs of the matched points at pose; with
        robust_scale > 0 every point's addends carry its Geman-McClure weight (rslo_map_normal_eq_w)."""
        from rslo_amd import capi
        md = _max_dist_of(max_dist, self.voxel_size)
        scale = check_scale(robust_scale)
        self.reserve(points.shape[0])
        return capi.map_normal_eq(self._buf, points, self._pose(pose), self.voxel_size, _metric_of(metric, points.shape[1]),
                                  md, min_hits, ws=self._reg_ws, robust_scale=scale if scale else None)

    def register(self, points, pose, iters=5, metric=None, max_dist=None, min_hits=1, damping=0.0, min_pairs=50,
                 tol_t=0.0, tol_r=0.0, info=None, robust_scale=0.0):
        """`iters` Gauss-Newton iterations of points (fp32 CUDA [P, F], read in place) against the map, on the device.
        pose: a float64 CUDA [7] tensor (a trajectory row) is updated IN PLACE and returned; anything else is copied to
        the device first.  -> (pose [7], info [iters, 8]) device tensors; info may be preallocated.  metric None:
        "plane" for points with normals (F >= 7), else "point".  robust_scale > 0: Geman-McClure weights
        (rslo_map_register_w).  No host read, nothing allocated after a reserve() when info is given."""
        from rslo_amd import capi
        _check_register(iters, tol_t, tol_r)
        md = _max_dist_of(max_dist, self.voxel_size)
        scale = check_scale(robust_scale)
        self.reserve(points.shape[0])
        pose = self._identity.clone() if pose is None else self._pose(pose)
        info = capi.map_register(self._buf, points, pose, self.voxel_size, iters, _metric_of(metric, points.shape[1]), md,
                                 min_hits, damping, min_pairs, tol_t, tol_r, info=info, ws=self._reg_ws,
                                 robust_scale=scale if scale else None)
        return pose, info

    def prune(self, center=None, radius=None, min_hits=1, grace=0):
        """Evict the cells that are not within radius of center, or that have fewer than min_hits hits and were created
        at least `grace` scans ago (module docstring).  center: None, a sequence, or a float64 CUDA tensor of >= 3
        elements that is read in place (a [7] trajectory row).  Enqueued on the current stream; no host read, and
        nothing allocated after reserve_prune() when center is a device tensor (or None): capturable."""
        from rslo_amd import capi
        r = check_prune(center, radius, min_hits, grace)
        self.reserve_prune()
        capi.map_prune(self._buf, self._prune_ws, self._center(center, exact=False), r, int(min_hits), int(grace))

    def carve(self, image, pose, tan_lo=None, tan_hi=None, win_rows=1, win_cols=1, margin_abs=0.3, margin_rel=0.0,
              max_range=60.0, grace=1):
        """Evict the cells that the scan behind `image` sees through from `pose` (module docstring).  image: a
        carve.RangeImage, or its int32 CUDA [H, W] tensor with tan_lo= / tan_hi=; pose: a float64 CUDA [7] tensor is read
        in place (a trajectory row), anything else is copied.  Enqueued on the current stream, five launches; no host
        read, and nothing allocated after reserve_prune() (the rebuild shares prune's workspace) when the pose is a
        device tensor: capturable."""
        from rslo_amd import capi
        _, _, tan_lo, tan_hi, win_rows, win_cols, margin_abs, margin_rel, max_range, grace = check_carve_call(
            image, tan_lo, tan_hi, win_rows, win_cols, margin_abs, margin_rel, max_range, grace)
        self.reserve_prune()
        capi.map_carve(self._buf, self._prune_ws, getattr(image, "img", image), tan_lo, tan_hi, self._pose(pose), win_rows,
                       win_cols, margin_abs, margin_rel, max_range, grace)

    def carve_stats(self):
        """{n_carves, n_carved} of the map's header (one host read)."""
        from rslo_amd import capi
        return self._header(capi.MAP_HDR_CARVE, CARVE_COUNTERS)

    def points(self, min_hits=1, center=None, radius=None, sort=True):
        """(rows [M, 4] fp32, tags [M] int64, hits [M] int32) of the cells with hits >= min_hits, and within radius of
        center when one is given (a sequence, or a float64 CUDA [3] tensor).  One host read (M).  sort=True orders by tag:
        deterministic bit for bit."""
        import torch
        from rslo_amd import capi
        if center is not None and radius is None:
            raise ValueError("points: a center needs a radius")
        center = self._center(center, exact=True)
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
        return self._header(capi.MAP_HDR_COUNTERS, COUNTERS)

    def save_ply(self, path, min_hits=1):
        rows, _, hits = self.points(min_hits)
        write_ply(path, rows.cpu().numpy(), hits.cpu().numpy())


# The default robust factor of default_schedule: scale = factor * voxel of the stage, no weights on the coarsest level.
# Chosen from the registration-alone pass of profiles/NOTES.md "Coarse-to-fine robust registration".
DEFAULT_ROBUST_FACTOR = 0.5


_CARVE_KW = (("tan_lo", None), ("tan_hi", None), ("win_rows", 1), ("win_cols", 1), ("margin_abs", 0.3), ("margin_rel", 0.0),
             ("max_range", 60.0), ("grace", 1))      # carve's keywords and defaults, in check_carve_call's order


class _PyramidBase:
    """What MapPyramidRef and MapPyramid share: a list of maps, coarse to fine, that receive the same calls."""

    def _each(self, name, *args, **kw):
        return [getattr(m, name)(*args, **kw) for m in self.levels]

    def insert(self, points, pose=None):
        self._each("insert", points, pose)

    def insert_frames(self, store, poses):
        """every level gets every frame of the keyframe store (the poses are checked, and copied if need be, once)"""
        self._each("insert_frames", store, self.levels[-1]._frame_poses(store, poses))

    def reset(self):
        self._each("reset")

    def prune(self, center=None, radius=None, min_hits=1, grace=0):
        check_prune(center, radius, min_hits, grace)      # before any level is written
        self._each("prune", center, radius, min_hits, grace)

    def stats(self):
        return self._each("stats")

    def prune_stats(self):
        return self._each("prune_stats")

    def carve(self, image, pose, **kw):
        """the one image carves every level (MapPyramid: the pose is copied to the device once, if need be)"""
        check_carve_call(image, *[kw.get(k, d) for k, d in _CARVE_KW])      # before any level is written
        self._each("carve", image, self._carve_pose(pose), **kw)

    def _carve_pose(self, pose):
        return pose

    def carve_stats(self):
        return self._each("carve_stats")

    def points(self, *args, **kw):
        return self.levels[-1].points(*args, **kw)

    def save_ply(self, path, min_hits=1):
        self.levels[-1].save_ply(path, min_hits)

    def lookup(self, points, pose=None, return_tags=False):
        return self.levels[-1].lookup(points, pose, return_tags)

    def overlap(self, points, pose=None):
        return self.levels[-1].overlap(points, pose)

    def default_schedule(self, iters_per_level=4, robust_factor=None):
        """One stage per level, coarse to fine: (level, iters_per_level, None, scale) with scale = robust_factor * voxel
        of the level, and no weights (0.0) on the coarsest level of a pyramid of more than one level: far from the
        answer the weights shut out the very pairs that pull the pose in.  robust_factor None: DEFAULT_ROBUST_FACTOR."""
        f = DEFAULT_ROBUST_FACTOR if robust_factor is None else float(robust_factor)
        n = len(self.levels)
        return [(k, int(iters_per_level), None, 0.0 if (k == 0 and n > 1) else f * self.voxel_sizes[k]) for k in range(n)]

    def _stages(self, schedule):
        return check_schedule(self.default_schedule() if schedule is None else schedule, self.voxel_sizes)


class MapPyramidRef(_PyramidBase):
    """The numpy restatement of a pyramid: one VoxelMapRef per voxel size, ordered coarse to fine (.levels[k]).
    insert / insert_frames / reset / prune / stats / prune_stats go to every level (stats: lists), points / save_ply / lookup / overlap
    address the finest; register runs a schedule (module docstring)."""

    def __init__(self, voxel_sizes=(0.8, 0.4, 0.2), capacity=None, min_range=0.0, max_range=float("inf")):
        self.voxel_sizes = _check_pyramid(voxel_sizes)      # (capacity: accepted for symmetry; the restatement has none)
        self.levels = [VoxelMapRef(v, min_range, max_range) for v in self.voxel_sizes]

    def reserve(self, n_points):
        pass

    def reserve_prune(self):
        pass

    def register(self, points, pose, schedule=None, metric=None, min_hits=1, damping=0.0, min_pairs=50, tol_t=0.0,
                 tol_r=0.0, info=None):
        """-> (pose [7] float64, info [sum of iters, 8]): the stages as successive VoxelMapRef.register calls."""
        stages = self._stages(schedule)
        _check_register(1, tol_t, tol_r)
        pose = np.array(pose, dtype=np.float64).reshape(7)
        rows = []
        for k, (level, iters, md, scale) in enumerate(stages):
            pose, part = self.levels[level].register(points, pose, iters, metric, md, min_hits, damping, min_pairs,
                                                     tol_t, tol_r, robust_scale=scale)
            part[:, 5], part[:, 6] = float(k), float(level)
            rows.append(part)
        rows = np.concatenate(rows)
        if info is not None:
            info[...] = rows
            rows = info
        return pose, rows


class MapPyramid(_PyramidBase):
    """The device pyramid: one VoxelMap per voxel size, ordered coarse to fine (.levels[k]); capacity is an int or one
    value per level.  Every level is filled by the existing insert and pruned by the existing prune (one call per
    level); register is ONE call of rslo_map_register_sched over all levels: no host read, nothing allocated after
    reserve() when info is given, a launch count fixed by the schedule."""

    def __init__(self, voxel_sizes=(0.8, 0.4, 0.2), capacity=1 << 22, device="cuda", min_range=0.0,
                 max_range=float("inf")):
        self.voxel_sizes, caps = _check_pyramid(voxel_sizes, capacity)
        self.levels = [VoxelMap(v, c, device, min_range, max_range) for v, c in zip(self.voxel_sizes, caps)]
        self.device = self.levels[-1].device

    def reserve(self, n_points):
        self._each("reserve", n_points)

    def reserve_prune(self):
        self._each("reserve_prune")

    def prune(self, center=None, radius=None, min_hits=1, grace=0):
        import torch
        check_prune(center, radius, min_hits, grace)
        if center is not None and not (torch.is_tensor(center) and center.is_cuda and center.dtype == torch.float64):
            center = torch.as_tensor(np.asarray(center, dtype=np.float64).reshape(-1)[:3].copy()).to(self.device)
        self._each("prune", center, radius, min_hits, grace)

    def _carve_pose(self, pose):
        return self.levels[-1]._pose(pose)

    def register(self, points, pose, schedule=None, metric=None, min_hits=1, damping=0.0, min_pairs=50, tol_t=0.0,
                 tol_r=0.0, info=None):
        """The stages of `schedule` (None: default_schedule()) in order, on the device.  pose: a float64 CUDA [7] tensor
        is updated IN PLACE and returned, anything else is copied to the device first.  -> (pose [7], info [sum of
        iters, 8]) device tensors; info may be preallocated."""
        from rslo_amd import capi
        stages = self._stages(schedule)
        _check_register(1, tol_t, tol_r)
        fine = self.levels[-1]
        self.reserve(points.shape[0])
        pose = fine._identity.clone() if pose is None else fine._pose(pose)
        info = capi.map_register_sched([m._buf for m in self.levels], self.voxel_sizes, stages, points, pose,
                                       _metric_of(metric, points.shape[1]), min_hits, damping, min_pairs, tol_t, tol_r,
                                       info=info, ws=fine._reg_ws)
        return pose, info
