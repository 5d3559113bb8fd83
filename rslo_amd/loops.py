"""Loop verification: a keyframe store, a geometric check of loop candidates in one launch, and a device edge list.

    store = KeyframeStore(capacity=8192, K=2048)                # voxel_size 0.5, min_z -1.4 (sensor frame), max_range 80
    frame, info = store.prepare(scan)                           # fp32 CUDA [P, F >= 3], sensor frame, read in place
    rows = db.query(...)                                        # PlaceDB: [top_k, 4] (entry, distance, shift, heading)
    ver = LoopVerifier(store)                                   # the options of check_verify
    out = ver.verify(rows)                                      # [top_k, 16], one workgroup per candidate
    edges = EdgeList(max_edges=256); edges.emit(out, store)     # at most one (i, j, Z, w) edge per query
    store.add()                                                 # AFTER emit: j is the store's n_entries at that moment
    runner = inference.OdometryRunner(net, places=db, loop=..., keyframes=store, verify=dict(), pose_graph=pg)
    runner.loop_checks(); runner.loop_edges(); runner.close_verified_loops()

KeyframeStore / LoopVerifier / EdgeList are the device side (csrc/loopverify.hip); KeyframeStoreRef / LoopVerifierRef /
EdgeListRef restate the rules of include/rslo_hip.h "Loop verification" in float64 numpy on host arrays and are the
arbiter of the tests: the store bit for bit, the matching exactly, the sums within rounding bounds.  The rules in one
place (all arithmetic IEEE double, no fused multiply-add; the pose algebra is se3.py's):

  * prepare(scan) -> frame float32 [K, 4], frame_info int32 [4] = {count, Q, flags, gated}.  A point is gated out when
    a coordinate is not finite, when double(z) > min_z is false, or when x*x + y*y + z*z < max_range*max_range is false.
    The kept points are voxel down-sampled (downsample.voxel_down_sample_ref's rules, no normals) at voxel_size: Q
    centroid rows in its cell order; its overflow is flags bit 0 and then Q = count = 0.  count = min(Q, K); frame row k
    is down-sample row (k * Q) // K when Q > K, else row k; column 3 is 0; rows >= count are zero;
  * add() appends the staged frame as entry n_entries; a full store drops it and counts dropped_full;
  * verify, per candidate row (entry, distance, shift, heading): status 1 unless 0 <= entry < n_entries; status 2
    unless distance < max_distance; status 3 when the query's or the entry's count is below min_pairs; these rows are
    {status, entry, 0, 0, 0, 0, identity, 0, 0, 0}.  Otherwise Z, the pose of the query in the frame of the entry
    (p_e = Z p_q: the Z of a PoseGraph loop edge (i = entry, j = query)), starts at t = 0,
    q = (cos(h/2), 0, 0, sin(h/2)), h = heading, or at the given start row.  Match of source point i: w = rotate(q, p_i)
    + t; d2 to every target point as dx*dx + dy*dy + dz*dz; the smallest d2 wins, ties to the lowest index; accepted
    iff d2 < max_dist*max_dist.  stages [(max_dist, iters), ...]: every iteration adds the point terms
    (J = [I | -[w]x], residual d; gauss_newton.point_terms) of the matched points to the 28 sums and takes
    gauss_newton.gauss_newton_step; fewer than min_pairs pairs, a matrix that is not positive definite or a step that
    is not finite is status 4: Z stays, the rest is skipped, no fitness.  Fitness at the final Z: match again within inlier_dist; overlap = inliers / query count,
    rms = sqrt(sum of d2 / inliers); status 0 iff inliers > 0, overlap >= min_overlap and rms <= max_rms, else 5.
    out row = {status, entry, pairs of the last iteration, overlap, rms, query count, Z (7), distance, heading, 0};
  * emit: among the rows with status 0 the one with the largest overlap, ties to the lowest row, is appended to the
    edge list as (i = entry, j = the store's n_entries, Z, (w_t, w_r)); a full list counts dropped_full.  Unused rows
    hold i = j = -1, which PoseGraph skips and counts.

The nearest-neighbour search of the device is an exhaustive scan of the entry's frame held in LDS (exact by
construction).  The store is also what a consistent map is rebuilt from after loop closure: VoxelMap.insert_frames
(rslo_amd/mapping.py) inserts every stored frame under its corrected pose in one call, and OdometryRunner.rebuild_map() /
adopt_loop_closure() (rslo_amd/inference.py) feed the correction back into the map and the refined chain.  Out of scope
here: evicting keyframes.
"""
import numpy as np

from rslo_amd import se3
from rslo_amd.downsample import voxel_down_sample_ref
from rslo_amd.gauss_newton import gauss_newton_step, point_terms

OUT_COLS = 16
STATUS = {0: "accepted", 1: "no candidate", 2: "gated", 3: "too few points", 4: "failed", 5: "rejected"}
DEFAULT_STAGES = ((3.0, 5), (1.5, 5), (0.75, 10))
VERIFY_DEFAULTS = dict(stages=DEFAULT_STAGES, max_distance=float("inf"), inlier_dist=0.5, min_overlap=0.5,
                       max_rms=float("inf"), min_pairs=50, damping=0.0)
IDENTITY = (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)


def check_store(capacity, K, voxel_size, min_z, max_range):
    if int(capacity) != capacity or not 1 <= capacity <= 1 << 16:
        raise ValueError("loops: capacity must be an integer in 1..2^16, got %r" % (capacity,))
    if int(K) != K or not 64 <= K <= 4096 or K % 64:
        raise ValueError("loops: K must be a multiple of 64 in 64..4096, got %r" % (K,))
    voxel_size, min_z, max_range = float(voxel_size), float(min_z), float(max_range)
    if not (voxel_size > 0.0 and np.isfinite(voxel_size)):
        raise ValueError("loops: voxel_size must be positive and finite, got %r" % (voxel_size,))
    if np.isnan(min_z) or not max_range > 0.0:
        raise ValueError("loops: min_z must not be NaN and max_range must be positive, got %r, %r" % (min_z, max_range))
    return int(capacity), int(K), voxel_size, min_z, max_range


def check_verify(options):
    """the verify options with their defaults filled in; ValueError for an unknown key or a value out of range"""
    options = dict(options or {})
    unknown = set(options) - set(VERIFY_DEFAULTS)
    if unknown:
        raise ValueError("loops: verify takes %s; got %s" % (", ".join(sorted(VERIFY_DEFAULTS)), sorted(unknown)))
    o = dict(VERIFY_DEFAULTS, **options)
    try:
        stages = [(float(md), it) for md, it in o["stages"]]
    except (TypeError, ValueError):
        raise ValueError("loops: stages must be rows (max_dist, iters), got %r" % (o["stages"],))
    if not 1 <= len(stages) <= 8:
        raise ValueError("loops: 1..8 stages, got %d" % len(stages))
    total = 0
    for md, it in stages:
        if not (md > 0.0 and np.isfinite(md * md)):
            raise ValueError("loops: a stage's max_dist must be positive with a finite square, got %r" % (md,))
        if int(it) != it or it < 1:
            raise ValueError("loops: a stage's iters must be an integer >= 1, got %r" % (it,))
        total += int(it)
    if total > 64:
        raise ValueError("loops: the iterations of all stages must sum to 1..64, got %d" % total)
    o["stages"] = tuple((md, int(it)) for md, it in stages)
    for name in ("max_distance", "inlier_dist", "min_overlap", "max_rms", "damping"):
        o[name] = float(o[name])
        if np.isnan(o[name]):
            raise ValueError("loops: %s is NaN" % name)
    if not (o["inlier_dist"] > 0.0 and np.isfinite(o["inlier_dist"] * o["inlier_dist"])):
        raise ValueError("loops: inlier_dist must be positive with a finite square, got %r" % (o["inlier_dist"],))
    if not 0.0 <= o["min_overlap"] <= 1.0:
        raise ValueError("loops: min_overlap must be in 0..1, got %r" % (o["min_overlap"],))
    if not o["max_rms"] >= 0.0:
        raise ValueError("loops: max_rms must be >= 0, got %r" % (o["max_rms"],))
    if int(o["min_pairs"]) != o["min_pairs"] or o["min_pairs"] < 1:
        raise ValueError("loops: min_pairs must be an integer >= 1, got %r" % (o["min_pairs"],))
    o["min_pairs"] = int(o["min_pairs"])
    return o


def check_top_k(top_k):
    if int(top_k) != top_k or not 1 <= top_k <= 16:
        raise ValueError("loops: top_k must be an integer in 1..16, got %r" % (top_k,))
    return int(top_k)


def check_edges(max_edges, edge_w):
    if int(max_edges) != max_edges or not 1 <= max_edges <= 4096:
        raise ValueError("loops: max_edges must be an integer in 1..4096, got %r" % (max_edges,))
    try:
        w_t, w_r = float(edge_w[0]), float(edge_w[1])
        ok = len(edge_w) == 2
    except (TypeError, ValueError, IndexError):
        ok = False
    if not ok or not (0.0 <= w_t < float("inf") and 0.0 <= w_r < float("inf")):
        raise ValueError("loops: edge_w must be two finite weights >= 0, got %r" % (edge_w,))
    return int(max_edges), (w_t, w_r)


def heading_pose(heading):
    """the start of a verification from a place search's heading: t = 0, a rotation by `heading` about z"""
    h = float(heading)
    return np.array([0.0, 0.0, 0.0, np.cos(h / 2.0), 0.0, 0.0, np.sin(h / 2.0)], np.float64)


class KeyframeStoreRef:
    """The store's rules on host arrays."""

    def __init__(self, capacity=8192, K=2048, voxel_size=0.5, min_z=-1.4, max_range=80.0):
        self.capacity, self.K, self.voxel_size, self.min_z, self.max_range = check_store(capacity, K, voxel_size, min_z,
                                                                                         max_range)
        self.frame = np.zeros((self.K, 4), np.float32)
        self.info = np.zeros(4, np.int32)
        self.reset()

    def reset(self):
        self.rows, self.counts = [], []
        self.dropped_full = 0

    def gate(self, points):
        """bool [N]: the points that are kept"""
        p = np.asarray(points, np.float32)[:, :3]
        x, y, z = (p[:, a].astype(np.float64) for a in range(3))
        with np.errstate(invalid="ignore", over="ignore"):
            return np.isfinite(p).all(1) & (z > self.min_z) & (x * x + y * y + z * z < self.max_range * self.max_range)

    def downsampled(self, points):
        """(rows float32 [Q, 3], flags, gated) of steps 1 and 2"""
        p = np.asarray(points, np.float32)
        p = p[:, :3] if len(p) else np.zeros((0, 3), np.float32)
        keep = self.gate(p) if len(p) else np.zeros(0, bool)
        kept = np.where(keep[:, None], p, np.float32(np.nan))
        try:
            rows = voxel_down_sample_ref(kept, None, self.voxel_size)[0]
            flags = 0
        except ValueError:
            rows, flags = np.zeros((0, 3), np.float32), 1
        return rows, flags, int((~keep).sum())

    def prepare(self, points):
        rows, flags, gated = self.downsampled(points)
        Q, K = len(rows), self.K
        count = min(Q, K)
        frame = np.zeros((K, 4), np.float32)
        k = np.arange(count, dtype=np.int64)
        frame[:count, :3] = rows[(k * Q) // K if Q > K else k]
        self.frame, self.info = frame, np.array([count, Q, flags, gated], np.int32)
        return self.frame, self.info

    def add(self, frame=None, info=None):
        if frame is None:
            frame, info = self.frame, self.info
        if len(self.rows) >= self.capacity:
            self.dropped_full += 1
            return
        self.rows.append(np.array(frame, np.float32))
        self.counts.append(int(min(max(int(info[0]), 0), self.K)))

    def stats(self):
        s = {"n_entries": len(self.rows), "dropped_full": self.dropped_full}
        s.update(zip(("count", "Q", "flags", "gated"), (int(v) for v in self.info)))
        return s

    def entries(self):
        n = len(self.rows)
        return (np.stack(self.rows) if n else np.zeros((0, self.K, 4), np.float32)), np.array(self.counts, np.int32)


def nearest_exact(w, target, chunk=256):
    """(index int64 [n] (-1: none comparable), d2 float64 [n]) of the target point [m, 3] nearest to every row of w:
    the smallest d2 = dx*dx + dy*dy + dz*dz, ties to the lowest index; brute force"""
    n, m = len(w), len(target)
    idx, best = np.full(n, -1, np.int64), np.full(n, np.inf)
    if m == 0:
        return idx, best
    t = np.ascontiguousarray(np.asarray(target, np.float64).T).T
    w = np.ascontiguousarray(np.asarray(w, np.float64).T).T
    for s in range(0, n, chunk):
        with np.errstate(invalid="ignore", over="ignore"):
            d = w[s:s + chunk, 0, None] - t[None, :, 0]
            d2 = d * d
            for a in (1, 2):                     # (dx*dx + dy*dy) + dz*dz
                d = w[s:s + chunk, a, None] - t[None, :, a]
                d2 = d2 + d * d
        d2 = np.where(np.isnan(d2), np.inf, d2)
        j = d2.argmin(1)                         # the first of equal minima: the lowest index
        b = d2[np.arange(len(j)), j]
        idx[s:s + chunk] = np.where(b < np.inf, j, -1)
        best[s:s + chunk] = b
    return idx, best


class LoopVerifierRef:
    """The verification rules on host arrays, against a KeyframeStoreRef."""

    def __init__(self, store, **options):
        self.store = store
        self.options = check_verify(options)

    def match(self, frame, info, entry, Z, max_dist):
        """(w [nq, 3], index int64 [nq] of the accepted match or -1, d2 [nq]) at the pose Z"""
        nq = int(min(max(int(info[0]), 0), self.store.K))
        nt = self.store.counts[entry]
        p = np.asarray(frame, np.float32)[:nq, :3].astype(np.float64)
        Z = np.asarray(Z, np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            w = se3.rotate(Z[3:], p) + Z[:3]
        idx, d2 = nearest_exact(w, self.store.rows[entry][:nt, :3])
        with np.errstate(invalid="ignore"):
            idx = np.where(d2 < max_dist * max_dist, idx, -1)
        return w, idx, d2

    def terms(self, frame, info, entry, Z, max_dist):
        """[pairs, 28]: the addends of the matched points in input order"""
        w, idx, _ = self.match(frame, info, entry, Z, max_dist)
        sel = idx >= 0
        m = self.store.rows[entry][idx[sel], :3].astype(np.float64)
        return point_terms(w[sel], w[sel] - m)

    def verify_row(self, frame, info, row, start=None):
        """-> (out [16], info [sum of iters, 8], matches int32 [K]) of one candidate row"""
        o, K = self.options, self.store.K
        total = sum(it for _, it in o["stages"])
        out, rows, matches = np.zeros(OUT_COLS), np.zeros((total, 8)), np.full(K, -1, np.int32)
        entry_d, distance, heading = float(row[0]), float(row[1]), float(row[3])
        nq = int(min(max(int(info[0]), 0), K))
        status = 0
        if not (entry_d >= 0.0 and entry_d < len(self.store.rows)):
            status = 1
        elif not distance < o["max_distance"]:
            status = 2
        elif nq < o["min_pairs"] or self.store.counts[int(entry_d)] < o["min_pairs"]:
            status = 3
        if status:
            out[0], out[1], out[6:13] = status, entry_d, IDENTITY
            rows[:, 0] = status
            return out, rows, matches
        entry = int(entry_d)
        Z = heading_pose(heading) if start is None else np.array(start, np.float64).reshape(7)
        failed, r, pairs = False, 0, 0.0
        for s, (max_dist, iters) in enumerate(o["stages"]):
            for _ in range(iters):
                rows[r, 5] = s
                if failed:
                    rows[r, 0] = 4.0
                    r += 1
                    continue
                terms = self.terms(frame, info, entry, Z, max_dist)
                pairs = float(len(terms))
                sums = terms.sum(axis=0)
                rows[r, 1], rows[r, 2] = pairs, sums[27]
                step = None
                if pairs >= o["min_pairs"]:
                    with np.errstate(all="ignore"):
                        step = gauss_newton_step(sums, Z, o["damping"])
                    if step is not None and not np.isfinite(step[0]).all():
                        step = None
                if step is None:
                    failed, rows[r, 0] = True, 4.0
                else:
                    Z, rows[r, 3], rows[r, 4] = step
                r += 1
        out[0], out[1], out[2], out[5], out[6:13], out[13], out[14] = 4.0, entry, pairs, nq, Z, distance, heading
        if failed:
            return out, rows, matches
        _, idx, d2 = self.match(frame, info, entry, Z, o["inlier_dist"])
        matches[:nq] = idx
        n_in = int((idx >= 0).sum())
        out[0] = 5.0
        if n_in:
            out[3] = n_in / float(nq)
            out[4] = np.sqrt(d2[idx >= 0].sum() / float(n_in))
            if out[3] >= o["min_overlap"] and out[4] <= o["max_rms"]:
                out[0] = 0.0
        return out, rows, matches

    def verify(self, cands, frame=None, info=None, start=None):
        """-> (out [top_k, 16], info [top_k, sum of iters, 8], matches int32 [top_k, K]); the staged frame by default"""
        if frame is None:
            frame, info = self.store.frame, self.store.info
        cands = np.asarray(cands, np.float64).reshape(-1, 4)
        check_top_k(len(cands))
        res = [self.verify_row(frame, info, row, None if start is None else np.asarray(start).reshape(-1, 7)[b])
               for b, row in enumerate(cands)]
        return tuple(np.stack([r[a] for r in res]) for a in range(3))


class EdgeListRef:
    """The edge list's rules on host arrays."""

    def __init__(self, max_edges=256, edge_w=(1.0, 1.0)):
        self.max_edges, self.edge_w = check_edges(max_edges, edge_w)
        self.reset()

    def reset(self):
        E = self.max_edges
        self.ij = np.full((E, 2), -1, np.int32)
        self.Z = np.tile(np.array(IDENTITY), (E, 1))
        self.w = np.zeros((E, 2))
        self.counters = np.zeros(2, np.int64)

    def emit(self, out, n_entries):
        out = np.asarray(out, np.float64).reshape(-1, OUT_COLS)
        best = -1
        for r in range(len(out)):
            if out[r, 0] == 0.0 and (best < 0 or out[r, 3] > out[best, 3]):
                best = r
        if best < 0:
            return
        n = int(self.counters[0])
        if n >= self.max_edges:
            self.counters[1] += 1
            return
        self.ij[n] = (int(out[best, 1]), int(n_entries))
        self.Z[n], self.w[n] = out[best, 6:13], self.edge_w
        self.counters[0] = n + 1


def _hip_error(fn, *args):
    from rslo_amd import capi
    try:
        return fn(*args)
    except ValueError as e:
        raise capi.RsloHipError(str(e))


class KeyframeStore:
    """The device store: owns the allocation (rslo_keyframe_bytes bytes), one staged frame with its info and the
    prepare workspace.  prepare / add / reset enqueue on the current stream, read nothing on the host and allocate
    nothing once reserve(n_points) has covered the scan size (prepare grows the workspace otherwise, outside capture
    only); stats() makes one host read."""

    def __init__(self, capacity=8192, K=2048, voxel_size=0.5, min_z=-1.4, max_range=80.0, device="cuda"):
        import torch
        from rslo_amd import capi
        self.capacity, self.K, self.voxel_size, self.min_z, self.max_range = _hip_error(check_store, capacity, K, voxel_size,
                                                                                         min_z, max_range)
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        dev = self.device
        self._buf = torch.empty((capi.keyframe_bytes(self.capacity, self.K) // 8,), dtype=torch.int64, device=dev)
        self._frame = torch.zeros((self.K, 4), dtype=torch.float32, device=dev)
        self._info = torch.zeros((4,), dtype=torch.int32, device=dev)
        self._ws, self._ws_points = None, -1
        self.reserve(0)
        self.reset()

    def reference(self, capacity=None):
        """a KeyframeStoreRef with this store's parameters"""
        return KeyframeStoreRef(self.capacity if capacity is None else capacity, self.K, self.voxel_size, self.min_z,
                                self.max_range)

    def reset(self):
        """Empty the store (a new sequence)."""
        from rslo_amd import capi
        capi.keyframe_reset(self._buf, self.capacity, self.K)

    def reserve(self, n_points=0):
        """Allocate the prepare workspace for scans of up to n_points points, once: prepare() then allocates nothing."""
        from rslo_amd import capi
        if int(n_points) > self._ws_points:
            self._ws = capi.keyframe_prepare_ws(int(n_points), self.device)
            self._ws_points = int(n_points)

    def prepare(self, points, out=None):
        """(frame fp32 [K, 4], frame_info int32 [4]) of one scan (fp32 CUDA [P, F >= 3], read in place).  Without out=
        they are the store's own staging buffers, overwritten by the next prepare()."""
        from rslo_amd import capi
        frame, info = (self._frame, self._info) if out is None else out
        self.reserve(int(points.shape[0]))
        capi.keyframe_prepare(points, self.K, self.voxel_size, self.min_z, self.max_range, frame, info, self._ws)
        return frame, info

    def add(self, frame=None, info=None):
        """Append a frame (default: the one prepare() staged last)."""
        from rslo_amd import capi
        if frame is None:
            frame, info = self._frame, self._info
        capi.keyframe_add(self._buf, self.capacity, self.K, frame, info)

    def stats(self):
        """{n_entries, dropped_full} of the store and {count, Q, flags, gated} of the staged frame: one host read."""
        import torch
        from rslo_amd import capi
        h = torch.cat([self._buf[capi.KF_HDR_ENTRIES:capi.KF_HDR_ENTRIES + 2], self._info.to(torch.int64)]).tolist()
        return dict(zip(("n_entries", "dropped_full", "count", "Q", "flags", "gated"), h))

    def frames(self):
        """(rows fp32 [capacity, K, 4], counts int32 [capacity]): device VIEWS of the store's sections, no copy and no
        host read; entries >= n_entries are unspecified."""
        import torch
        N, K = self.capacity, self.K
        raw = self._buf.view(torch.uint8)
        o = 256 + (N * 4 + 255) // 256 * 256
        return raw[o:o + N * K * 16].view(torch.float32).view(N, K, 4), raw[256:256 + N * 4].view(torch.int32)

    def entries(self):
        """(rows [n, K, 4], counts int32 [n]) of the stored frames, copied to the host (tests, tools)."""
        n = self.stats()["n_entries"]
        N, K = self.capacity, self.K
        pad = lambda b: (b + 255) // 256 * 256
        raw = self._buf.cpu().numpy().view(np.uint8)
        o = 256
        counts = raw[o:o + N * 4].view(np.int32)[:n].copy()
        o += pad(N * 4)
        rows = raw[o:o + N * K * 16].view(np.float32).reshape(N, K, 4)[:n].copy()
        return rows, counts


class LoopVerifier:
    """rslo_loop_verify with a fixed set of options against one KeyframeStore.  verify() enqueues ONE launch on the
    current stream, reads nothing on the host and allocates nothing when out= (and info= / matches=) are given."""

    def __init__(self, store, **options):
        self.store = store
        self.options = _hip_error(check_verify, options)
        self.total_iters = sum(it for _, it in self.options["stages"])

    def reference(self, store_ref):
        return LoopVerifierRef(store_ref, **self.options)

    def verify(self, cands, frame=None, info_q=None, start=None, out=None, info=None, matches=None):
        """cands: float64 CUDA [top_k, 4], the rows of PlaceDB.query -> out float64 [top_k, 16].  info=True / matches=True
        allocate the optional outputs (or pass preallocated tensors) and the result is the tuple (out, info, matches)
        with None where not asked for."""
        import torch
        from rslo_amd import capi
        st, o = self.store, self.options
        if frame is None:
            frame, info_q = st._frame, st._info
        if cands.dim() != 2 or cands.shape[1] != 4:
            raise capi.RsloHipError("LoopVerifier.verify: cands must be [top_k, 4] float64")
        top_k = _hip_error(check_top_k, int(cands.shape[0]))
        dev = st.device
        if out is None:
            out = torch.empty((top_k, OUT_COLS), dtype=torch.float64, device=dev)
        plain = info is None and matches is None
        if info is True:
            info = torch.empty((top_k, self.total_iters, 8), dtype=torch.float64, device=dev)
        if matches is True:
            matches = torch.empty((top_k, st.K), dtype=torch.int32, device=dev)
        capi.loop_verify(st._buf, st.capacity, st.K, frame, info_q, cands, top_k, start, o["stages"], o["max_distance"],
                         o["inlier_dist"], o["min_overlap"], o["max_rms"], o["min_pairs"], o["damping"], out, info, matches)
        return out if plain else (out, info, matches)


class EdgeList:
    """The device edge list: ij int32 [E, 2], Z float64 [E, 7], w float64 [E, 2], counters int64 [2] = {n_edges,
    dropped_full}.  Unused rows hold i = j = -1, so PoseGraph.optimize takes the whole list without a host read."""

    def __init__(self, max_edges=256, edge_w=(1.0, 1.0), device="cuda"):
        import torch
        self.max_edges, self.edge_w = _hip_error(check_edges, max_edges, edge_w)
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        E, dev = self.max_edges, self.device
        self.ij = torch.empty((E, 2), dtype=torch.int32, device=dev)
        self.Z = torch.empty((E, 7), dtype=torch.float64, device=dev)
        self.w = torch.empty((E, 2), dtype=torch.float64, device=dev)
        self.counters = torch.empty((2,), dtype=torch.int64, device=dev)
        self.reset()

    def reset(self):
        from rslo_amd import capi
        capi.loop_edges_reset(self.ij, self.Z, self.w, self.counters)

    def emit(self, out, store):
        """Append the best accepted row of out [top_k, 16] as (entry, store's n_entries, Z, edge_w): before store.add()."""
        from rslo_amd import capi
        capi.loop_emit(out, int(out.shape[0]), store._buf, store.capacity, store.K, self.ij, self.Z, self.w, self.counters,
                       self.edge_w[0], self.edge_w[1])

    def tensors(self):
        return self.ij, self.Z, self.w, self.counters
