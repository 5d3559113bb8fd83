"""Place recognition: Scan Context descriptors (Kim & Kim, IROS 2018), a device-resident database and a loop search.

    db = PlaceDB(capacity=8192)                                 # R = 20 rings, S = 60 sectors, 80 m, z_offset 2.0
    D, key, norm = db.describe(scan)                            # fp32 CUDA [P, F >= 3], sensor frame, read in place
    rows = db.query(D, key, norm, exclude_recent=50, num_candidates=10, top_k=1)
    db.add(D, key, norm)
    runner = inference.OdometryRunner(net, places=db, loop=dict(exclude_recent=50, num_candidates=10, top_k=1))
    runner.loop_candidates()                                    # [n, top_k, 4]: (entry, distance, shift, heading)

PlaceDB is the device side (csrc/places.hip); ScanContextRef / PlaceDBRef restate the rules of include/rslo_hip.h
"Place recognition" in float64 numpy on host arrays and are the arbiter of the tests, which compare bit for bit.  The
rules in one place (all arithmetic IEEE double, no fused multiply-add, unless it says float):

  * tables(R, S, max_range), made once and handed to both sides: dirs[k] = (cos, sin)(2 pi k / S) for k = 0..S with
    dirs[S] = dirs[0], and edge2[k] = (k * max_range / R)^2 for k = 0..R.  No transcendental function decides a bin;
  * descriptor D float32 [R, S] of a scan in the sensor frame, per point: x, y = double(p.x), double(p.y); a coordinate of
    xyz that is not finite drops it (dropped_invalid); r2 = x*x + y*y must be > 0 and < edge2[R] (dropped_range);
    ring = #{k in 1..R-1: r2 >= edge2[k]}; c_k = dirs[k].x*y - dirs[k].y*x, sector = the smallest k in 0..S-1 with
    c_k >= 0 and c_{k+1} < 0 (none: dropped_range); v = p.z + z_offset in float must be > 0 (dropped_low);
    D[ring, sector] = max(D[ring, sector], v); empty bins are 0;
  * key[r] int32 = #{j: D[r, j] > 0}; norm[j] = sqrt(sum over r ascending of double(D[r, j])^2);
  * the database appends entries; a full one drops the entry and counts it (dropped_full);
  * query: eligible = entries with index < n_entries - exclude_recent.  Stage 1 (num_candidates C > 0): the C eligible
    entries with the smallest kd = min(sum_r (key_q[r] - key_e[r])^2, 2^32 - 1), the sum exact for any int32 keys,
    ties to the lower index; C = 0: all of them.  Stage 2:
    for every shift s, j' = (j + s) % S, column j valid when norm_q[j] > 0 and norm_e[j'] > 0,
    cos_j = (sum over r ascending of double(Dq[r,j]) * double(De[r,j'])) / (norm_q[j] * norm_e[j']),
    d(s) = 1 - (sum of cos_j over valid j ascending) / n_valid (+inf without a valid column); the entry's distance is
    min_s d(s), ties to the lowest s.  Result [top_k, 4] float64 rows (entry, distance, shift, (shift * 2 pi) / S) by
    distance, then index; entries at +inf are not returned; unused rows are (-1, +inf, -1, 0).  Column 3 is the
    query's heading relative to the entry.  No threshold: acceptance is the caller's comparison.

Verifying a candidate geometrically is rslo_amd/loops.py (KeyframeStore, LoopVerifier); pose-graph optimisation is
rslo_amd/posegraph.py.  Out of scope here: correcting the map, evicting entries.
"""
import numpy as np

TWO_PI = 2.0 * np.pi
UNUSED_ROW = (-1.0, float("inf"), -1.0, 0.0)
KD_MAX = (1 << 32) - 1      # the bound of a stage-1 ring-key distance


def check_params(R, S, max_range, z_offset):
    if int(R) != R or not 1 <= R <= 64:
        raise ValueError("places: R (rings) must be an integer in 1..64, got %r" % (R,))
    if int(S) != S or not 3 <= S <= 128:
        raise ValueError("places: S (sectors) must be an integer in 3..128, got %r" % (S,))
    max_range, z_offset = float(max_range), float(z_offset)
    if not (max_range > 0.0 and np.isfinite(max_range)):
        raise ValueError("places: max_range must be positive and finite, got %r" % (max_range,))
    if not np.isfinite(np.float32(z_offset)):
        raise ValueError("places: z_offset must be a finite float, got %r" % (z_offset,))
    return int(R), int(S), max_range, z_offset


def check_query(exclude_recent, num_candidates, top_k):
    for name, v, lo, hi in (("exclude_recent", exclude_recent, 0, None), ("num_candidates", num_candidates, 0, 256),
                            ("top_k", top_k, 1, 16)):
        if int(v) != v or v < lo or (hi is not None and v > hi):
            raise ValueError("places: %s must be an integer in %d..%s, got %r" % (name, lo, "" if hi is None else hi, v))
    return int(exclude_recent), int(num_candidates), int(top_k)


LOOP_DEFAULTS = dict(exclude_recent=50, num_candidates=10, top_k=1)


def check_loop(options):
    """The loop= options of an OdometryRunner (ValueError): -> the keyword arguments of PlaceDB.query, LOOP_DEFAULTS
    filled in.  None: the defaults."""
    o = dict(LOOP_DEFAULTS, **(options or {}))
    unknown = set(o) - set(LOOP_DEFAULTS)
    if unknown:
        raise ValueError("loop takes exclude_recent, num_candidates and top_k; got %s" % sorted(unknown))
    return dict(zip(LOOP_DEFAULTS, check_query(**o)))


def tables(R, S, max_range):
    """float64 [2*(S+1) + R+1]: dirs [S+1, 2] flattened, then edge2 [R+1].  Made once; both sides read these values."""
    R, S, max_range, _ = check_params(R, S, max_range, 0.0)
    k = np.arange(S + 1, dtype=np.float64)
    dirs = np.stack([np.cos(TWO_PI * k / S), np.sin(TWO_PI * k / S)], 1)
    dirs[S] = dirs[0]
    e = np.arange(R + 1, dtype=np.float64) * max_range / R
    return np.concatenate([dirs.reshape(-1), e * e])


class ScanContextRef:
    """The descriptor rules on host arrays."""

    def __init__(self, R=20, S=60, max_range=80.0, z_offset=2.0, tables_=None):
        self.R, self.S, self.max_range, self.z_offset = check_params(R, S, max_range, z_offset)
        t = tables(self.R, self.S, self.max_range) if tables_ is None else np.asarray(tables_, np.float64)
        self.dirs = t[:2 * (self.S + 1)].reshape(self.S + 1, 2)
        self.edge2 = t[2 * (self.S + 1):]
        self.no_sector = 0      # points of the last describe() that no k satisfied (part of dropped_range)

    def bins(self, points):
        """(ring, sector, v, why) per point; why: 0 kept, 1 invalid, 2 range (or no sector), 3 low"""
        R, S = self.R, self.S
        p = np.asarray(points, np.float32)[:, :3]
        why = np.zeros(len(p), np.int32)
        x, y = p[:, 0].astype(np.float64), p[:, 1].astype(np.float64)
        finite = np.isfinite(p).all(1)
        with np.errstate(invalid="ignore", over="ignore"):
            r2 = x * x + y * y
            in_range = (r2 > 0.0) & (r2 < self.edge2[R])
            ring = (r2[:, None] >= self.edge2[None, 1:R]).sum(1).astype(np.int64)
            c = self.dirs[None, :, 0] * y[:, None] - self.dirs[None, :, 1] * x[:, None]      # two rounded products, one subtraction
            ok = (c[:, :-1] >= 0.0) & (c[:, 1:] < 0.0)
            sector = ok.argmax(1)
            has = ok.any(1)
            v = p[:, 2] + np.float32(self.z_offset)
            low = ~(v > np.float32(0))
        why[low] = 3
        self.no_sector = int((finite & in_range & ~has).sum())
        why[~has] = 2
        why[~in_range] = 2
        why[~finite] = 1
        return ring, sector, v.astype(np.float32), why

    def describe(self, points):
        """(D float32 [R, S], key int32 [R], norm float64 [S], counters dict)"""
        R, S = self.R, self.S
        ring, sector, v, why = self.bins(points)
        keep = why == 0
        D = np.zeros((R, S), np.float32)
        np.maximum.at(D, (ring[keep], sector[keep]), v[keep])
        key, norm = key_and_norm(D)
        counters = {"n_points": int(keep.sum()), "dropped_invalid": int((why == 1).sum()),
                    "dropped_range": int((why == 2).sum()), "dropped_low": int((why == 3).sum())}
        return D, key, norm, counters


def key_and_norm(D):
    D = np.asarray(D, np.float32)
    key = (D > 0).sum(1).astype(np.int32)
    acc = np.zeros(D.shape[1], np.float64)
    for r in range(D.shape[0]):                  # r ascending
        d = D[r].astype(np.float64)
        acc = acc + d * d
    return key, np.sqrt(acc)


class PlaceDBRef:
    """The database and the query rules on host arrays.  describe() is ScanContextRef's."""

    def __init__(self, capacity=8192, R=20, S=60, max_range=80.0, z_offset=2.0, tables_=None):
        self.sc = ScanContextRef(R, S, max_range, z_offset, tables_)
        self.R, self.S = self.sc.R, self.sc.S
        if int(capacity) != capacity or not 1 <= capacity <= 1 << 24:
            raise ValueError("places: capacity must be an integer in 1..2^24, got %r" % (capacity,))
        self.capacity = int(capacity)
        self.reset()

    def reset(self):
        self.D, self.key, self.norm = [], [], []
        self.dropped_full = 0
        self._last = None

    def describe(self, points):
        D, key, norm, counters = self.sc.describe(points)
        self._last = counters
        return D, key, norm

    def add(self, D, key, norm):
        if len(self.D) >= self.capacity:
            self.dropped_full += 1
            return
        self.D.append(np.array(D, np.float32))
        self.key.append(np.array(key, np.int32))
        self.norm.append(np.array(norm, np.float64))

    def stats(self):
        s = {"n_entries": len(self.D), "dropped_full": self.dropped_full}
        s.update(self._last or dict.fromkeys(("n_points", "dropped_invalid", "dropped_range", "dropped_low"), 0))
        return s

    def distances(self, D, norm, entries):
        """(distance float64 [len(entries)], shift int64 [len(entries)]) of stage 2.  The sums over r and over j are
        explicit loops, in the rule's order; numpy only runs them for every (entry, column pair) side by side."""
        R, S = self.R, self.S
        entries = np.asarray(entries, np.int64)
        if len(entries) == 0:
            return np.zeros(0, np.float64), np.zeros(0, np.int64)
        Dq = np.asarray(D, np.float32).astype(np.float64)
        nq = np.asarray(norm, np.float64)
        De = np.stack([self.D[e] for e in entries]).astype(np.float64)      # [E, R, S]
        ne = np.stack([self.norm[e] for e in entries])                       # [E, S]
        dot = np.zeros((len(entries), S, S), np.float64)                     # [e, j, j']
        for r in range(R):
            dot = dot + Dq[r][None, :, None] * De[:, r, None, :]
        valid = (nq[None, :, None] > 0.0) & (ne[:, None, :] > 0.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            cos = dot / (nq[None, :, None] * ne[:, None, :])
        total = np.zeros((len(entries), S), np.float64)                      # [e, s]
        n_valid = np.zeros((len(entries), S), np.int64)
        s_all = np.arange(S)
        for j in range(S):                                                   # j ascending
            jp = (j + s_all) % S
            ok = valid[:, j, jp]
            total = np.where(ok, total + np.where(ok, cos[:, j, jp], 0.0), total)
            n_valid += ok
        with np.errstate(invalid="ignore", divide="ignore"):
            d = np.where(n_valid > 0, 1.0 - total / np.maximum(n_valid, 1).astype(np.float64), np.inf)
        shift = d.argmin(1)                                                  # the first of equal minima: the lowest s
        return d[np.arange(len(entries)), shift], shift.astype(np.int64)

    def candidates(self, key, exclude_recent, num_candidates):
        """the stage-2 entries, in stage-1 order"""
        E = max(len(self.D) - int(exclude_recent), 0)
        if num_candidates == 0 or E == 0:
            return np.arange(E, dtype=np.int64)
        a = np.abs(np.asarray(key, np.int64)[None, :] - np.stack(self.key[:E]).astype(np.int64))
        kd = np.minimum((np.minimum(a, 65536) ** 2).sum(1), KD_MAX)      # |d| >= 2^16 reaches the bound alone: nothing wraps
        order = np.lexsort((np.arange(E), kd))
        return order[:num_candidates].astype(np.int64)

    def query(self, D, key, norm, exclude_recent=0, num_candidates=10, top_k=1):
        exclude_recent, num_candidates, top_k = check_query(exclude_recent, num_candidates, top_k)
        cand = self.candidates(key, exclude_recent, num_candidates)
        d, shift = self.distances(D, norm, cand)
        out = np.tile(np.array(UNUSED_ROW, np.float64), (top_k, 1))
        keep = np.isfinite(d)
        cand, d, shift = cand[keep], d[keep], shift[keep]
        order = np.lexsort((cand, d))[:top_k]
        for row, i in enumerate(order):
            out[row] = (float(cand[i]), d[i], float(shift[i]), (float(shift[i]) * TWO_PI) / float(self.S))
        return out


class PlaceDB:
    """The device database: owns the allocation (rslo_place_bytes bytes), the tables, the query workspace and one set of
    descriptor buffers.  describe / add / query / reset enqueue on the current stream, read nothing on the host and
    allocate nothing (query's result excepted, unless out= is given); stats() makes one host read.  add() and query()
    take key and norm as the caller gives them: any int32 key has a defined stage-1 distance (clamped at 2^32 - 1)."""

    def __init__(self, capacity=8192, R=20, S=60, max_range=80.0, z_offset=2.0, device="cuda"):
        import torch
        from rslo_amd import capi
        self.R, self.S, self.max_range, self.z_offset = check_params(R, S, max_range, z_offset)
        self.capacity = int(capacity)
        nbytes = capi.place_bytes(self.capacity, self.R, self.S)
        if nbytes == 0:
            raise capi.RsloHipError("PlaceDB: capacity must be in 1..2^24, got %r" % (capacity,))
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        dev = self.device
        self.tables_host = tables(self.R, self.S, self.max_range)
        self.tables = torch.from_numpy(self.tables_host).to(dev)
        self._buf = torch.empty((nbytes // 8,), dtype=torch.int64, device=dev)
        self._ws = capi.place_query_ws(self.capacity, dev)
        self._D = torch.zeros((self.R, self.S), dtype=torch.float32, device=dev)
        self._key = torch.zeros((self.R,), dtype=torch.int32, device=dev)
        self._norm = torch.zeros((self.S,), dtype=torch.float64, device=dev)
        self._counters = torch.zeros((4,), dtype=torch.int64, device=dev)
        self.reset()

    def reference(self, capacity=None):
        """a PlaceDBRef with this database's parameters and tables"""
        return PlaceDBRef(self.capacity if capacity is None else capacity, self.R, self.S, self.max_range, self.z_offset,
                          self.tables_host)

    def reset(self):
        """Empty the database (a new sequence)."""
        from rslo_amd import capi
        capi.place_reset(self._buf, self.capacity, self.R, self.S)

    def reserve(self, n_points=0):
        """Everything describe / add / query need is allocated at construction, whatever the scan size: nothing to do.
        Kept so that a runner can ask, as it asks a VoxelMap."""

    def describe(self, points, out=None):
        """(D fp32 [R, S], key int32 [R], norm float64 [S]) of one scan (fp32 CUDA [P, F >= 3], read in place).  Without
        out= they are the database's own buffers, overwritten by the next describe(); out=(D, key, norm) are the
        caller's.  The counters of the scan are in stats()."""
        from rslo_amd import capi
        D, key, norm = (self._D, self._key, self._norm) if out is None else out
        capi.place_describe(points, self.R, self.S, self.tables, self.z_offset, D, key, norm, self._counters)
        return D, key, norm

    def add(self, D=None, key=None, norm=None):
        """Append a descriptor (default: the one describe() made last)."""
        from rslo_amd import capi
        if D is None:
            D, key, norm = self._D, self._key, self._norm
        capi.place_add(self._buf, self.capacity, self.R, self.S, D, key, norm)

    def query(self, D=None, key=None, norm=None, exclude_recent=0, num_candidates=10, top_k=1, out=None):
        """[top_k, 4] float64 on the device: (entry, distance, shift, heading) rows, best first; unused rows are
        (-1, inf, -1, 0).  out: a preallocated contiguous [top_k, 4] float64 CUDA tensor (a row of a runner's buffer)."""
        import torch
        from rslo_amd import capi
        try:
            exclude_recent, num_candidates, top_k = check_query(exclude_recent, num_candidates, top_k)
        except ValueError as e:
            raise capi.RsloHipError(str(e))
        if D is None:
            D, key, norm = self._D, self._key, self._norm
        if out is None:
            out = torch.empty((top_k, 4), dtype=torch.float64, device=self.device)
        capi.place_query(self._buf, self.capacity, self.R, self.S, D, key, norm, exclude_recent, num_candidates, top_k,
                         out, self._ws)
        return out

    def stats(self):
        """{n_entries, dropped_full} of the database and the four counters of the last describe(): one host read."""
        import torch
        from rslo_amd import capi
        h = torch.cat([self._buf[capi.PLACE_HDR_ENTRIES:capi.PLACE_HDR_ENTRIES + 2], self._counters]).tolist()
        return dict(zip(("n_entries", "dropped_full") + capi.PLACE_COUNTERS, h))

    def entries(self):
        """(D [n, R, S], norm [n, S], key [n, R]) of the stored entries, copied to the host (tests, tools)."""
        n = self.stats()["n_entries"]
        R, S, N = self.R, self.S, self.capacity
        pad = lambda b: (b + 255) // 256 * 256
        raw = self._buf.cpu().numpy().view(np.uint8)
        o = 256
        D = raw[o:o + N * R * S * 4].view(np.float32).reshape(N, R, S)[:n].copy()
        o += pad(N * R * S * 4)
        norm = raw[o:o + N * S * 8].view(np.float64).reshape(N, S)[:n].copy()
        o += pad(N * S * 8)
        key = raw[o:o + N * R * 4].view(np.int32).reshape(N, R)[:n].copy()
        return D, norm, key
