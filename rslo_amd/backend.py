"""The streaming back end: what happens to a scan behind the network's pose, and to what has been streamed.

PoseChain is the four tensors of rslo_pose_chain; BackEnd owns the stages that OdometryRunner.run() issues behind the
head replay (de-skewing, the refined chain, both registrations, carving, both maps and their pruning, place search, the
keyframe store, loop verification) and the work on what has been streamed (the pose graph, the map rebuild).  It knows
no network, no encoder and no handle: step(source, times) takes the tensor the caller submitted.  check() is every
option's validation, with no side effect, so that a caller can refuse a configuration before it builds anything.
"""
import torch

from rslo_amd import capi


def _device(device):
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


class PoseChain:
    """One streamed pose chain on the device: state [7] fp64, count [1] int32, rel [capacity, 7] fp32 (the odometry rows
    pushed) and traj [capacity, 7] fp64 (their composition).  push() is ONE launch of rslo_pose_chain on the current
    stream: row *count of rel and traj is written, then *count += 1; it may be captured into a graph."""

    def __init__(self, capacity, device):
        self.capacity = int(capacity)
        self.state = torch.zeros((7,), dtype=torch.float64, device=device)
        self.count = torch.zeros((1,), dtype=torch.int32, device=device)
        self.rel = torch.zeros((self.capacity, 7), dtype=torch.float32, device=device)
        self.traj = torch.zeros((self.capacity, 7), dtype=torch.float64, device=device)

    def push(self, t, q):
        capi.pose_chain(t, q, self.state, self.count, self.rel, self.traj)

    def reset(self):
        """A new sequence: the next push seeds the state and writes row 0."""
        self.count.zero_()

    def set_state(self, row):
        """The next push composes onto `row` ([7] fp64 on the device)."""
        self.state.copy_(row)

    def rows(self, n):
        """(rel [n, 7], traj [n, 7]) views of the first n rows"""
        return self.rel[:n], self.traj[:n]


def check(capacity, device, voxel_map=None, refine=None, local_map=None, places=None, loop=None, pose_graph=None,
          keyframes=None, verify=None, surfels=None, surfel_refine=None, deskew=None, carve=None):
    """Every back-end option of an OdometryRunner / a BackEnd, normalised (ValueError otherwise): -> dict(refine,
    info_rows, surfel_refine, local_map, loop, verify, edges, deskew, carve), None where the option is off.  Nothing is
    built, reserved or started: the collaborators are only read (.device, .capacity, .max_loops and what their own
    check_* read)."""
    from rslo_amd import carve as carve_mod, deskew as deskew_mod, loops, mapping, places as places_mod, surfels as surfels_mod
    out = dict(refine=None, info_rows=0, surfel_refine=None, local_map=None, loop=None, verify=None, edges=None,
               deskew=None, carve=None)
    if carve is not None:
        if voxel_map is None:
            raise ValueError("carve needs a voxel_map to carve")
        out["carve"] = carve_mod.check_carve(carve)
    if refine is not None:
        if voxel_map is None:
            raise ValueError("refine needs a voxel_map to register against")
        out["refine"], out["info_rows"] = mapping.check_refine(refine, voxel_map)
    if surfel_refine is not None:
        if surfels is None:
            raise ValueError("surfel_refine needs surfels=SurfelMap(...) to register against")
        out["surfel_refine"] = surfels_mod.check_surfel_refine(surfel_refine, surfels)
    if deskew is not None:
        out["deskew"] = deskew_mod.check_deskew(deskew)
        if out["deskew"]["motion"] == "refined" and refine is None and surfel_refine is None:
            raise ValueError("deskew motion=\"refined\" needs refine= or surfel_refine= (the chain it reads)")
    if loop is not None and places is None:
        raise ValueError("loop needs places=PlaceDB(...) to search")
    if places is not None:
        out["loop"] = places_mod.check_loop(loop)
    if verify is not None:
        if places is None or keyframes is None:
            raise ValueError("verify needs places=PlaceDB(...) and keyframes=KeyframeStore(...)")
        verify = dict(verify)
        edge_w, max_edges = verify.pop("edge_w", (1.0, 1.0)), verify.pop("max_edges", 256)
        out["verify"], out["edges"] = loops.check_verify(verify), loops.check_edges(max_edges, edge_w)
        if pose_graph is not None and out["edges"][0] > pose_graph.max_loops:
            raise ValueError("verify max_edges = %d exceeds pose_graph.max_loops = %d" % (out["edges"][0], pose_graph.max_loops))
    for name, owner in (("places", places if verify is not None else None), ("keyframes", keyframes)):
        if owner is not None and owner.capacity < int(capacity):
            raise ValueError("the %s capacity %d is below the runner's capacity %d (an entry's index must equal its scan's "
                             "index)" % (name, owner.capacity, int(capacity)))
    if local_map is not None:
        out["local_map"] = mapping.check_local_map(local_map, voxel_map, surfels)
    for name, owner in (("voxel map", voxel_map), ("surfel map", surfels), ("place database", places),
                        ("keyframe store", keyframes), ("pose graph", pose_graph)):
        if owner is not None and owner.device != _device(device):
            raise ValueError("the %s lives on %s, the runner on %s" % (name, owner.device, _device(device)))
    return out


class BackEnd:
    """Everything a streamed scan meets behind the network's pose, in one explicit sequence:

        chain = PoseChain(capacity, device)                    # the open-loop chain: the caller pushes rel[n] ...
        back = BackEnd(chain, capacity=..., point_capacity=..., device=..., voxel_map=..., refine=..., ...)
        back.step(cloud)                                       # ... then hands over scan n = back.n, the step's own count

    OdometryRunner builds one over its open-loop chain and calls step() behind every head replay; its public methods
    and attributes of the same names delegate here.  step() enqueues on the caller's stream, reads nothing on the host,
    allocates nothing and opens no stream; what is issued when is decided by the host's own scan count n (counted from 0
    since reset()).  The open-loop chain is only read: its rel / traj rows stay bit for bit whatever is switched on
    here, and with every option None step() issues nothing at all.

    * World map: voxel_map=VoxelMap(...) (rslo_amd/mapping.py, csrc/map.hip) registers every scan: step() inserts the
      tensor the caller submitted (its first four columns are x, y, z, intensity in both input forms) under row n of
      the trajectory, behind the pose chain of that scan: at most three launches, no synchronisation.  The caller keeps
      the submitted tensor unmodified until the step has been consumed on the device.  reset() also resets the map (a
      new sequence has a new frame); its figures come from voxel_map.stats().  None (the default): no map.
    * Refinement: refine=dict(iters=3, ...) (keyword arguments of VoxelMap.register except metric; needs voxel_map)
      registers every scan against the map before inserting it (csrc/mapreg.hip).  The back end then keeps a SECOND
      chain beside the open-loop one, driven by the same rslo_pose_chain: push(rel[n]) on it writes the prediction
      refined[n-1] o rel[n] into row n, voxel_map.register corrects that row in place (metric "plane" for [P, >= 7]
      input, "point" for raw scans), the chain's state is set to the corrected row so that the next scan composes onto
      it, and the scan is inserted under it.  refined_trajectory() is the second chain and refine_info() the
      [n, iters, 8] info rows of register, both on the device.  A fixed number of launches per scan.  None (the
      default): no second chain.
    * Coarse-to-fine refinement: voxel_map=MapPyramid(...) (one VoxelMap per voxel size) with
      refine=dict(schedule=[(level, iters, max_dist or None, robust_scale), ...]) -- or refine=dict(): the pyramid's
      default_schedule() -- runs MapPyramid.register (rslo_map_register_sched, one call) where VoxelMap.register runs
      above; insert, reset and prune reach every level; refine_info() is [n, sum of iters, 8] with stage and level in
      columns 5 and 6.  refine=dict(robust_scale=s) on a plain VoxelMap weights its iterations.  schedule= with a plain
      VoxelMap, or together with iters=, is an error at construction.
    * Rolling local map: local_map=dict(radius=R, every=K, min_hits=1, grace=0) (needs voxel_map) keeps the map near the
      sensor: behind the insert of scan n, when (n + 1) % K == 0, step() calls voxel_map.prune(center=row n of the
      chain that fed the insert, radius=R, min_hits=, grace=) -- the refined chain when there is one, else the
      open-loop one (VoxelMap.prune; include/rslo_hip.h "Rolling local map").  The workspace (about one more table) is
      reserved at construction.  None (the default): the map only grows.  One more, optional key, surfels=True or
      surfels=dict(min_count=1, inner_radius=None) (needs surfels=; a voxel_map is then no longer required), prunes
      the surfel map too: behind the surfel insert of the same scans step() calls surfels.prune(the same row, R,
      inner_radius, min_count) (SurfelMap.prune; "Rolling local surfel map"), with its workspace reserved at
      construction as well.  Without the key the surfel map is never pruned.
    * Place recognition: places=PlaceDB(...) (rslo_amd/places.py, csrc/places.hip) with
      loop=dict(exclude_recent=50, num_candidates=10, top_k=1) (these defaults; keyword arguments of PlaceDB.query):
      behind everything above, step() describes the scan (sensor frame, its first three columns), queries the database
      with that descriptor into row n of loop_candidates() ([n, top_k, 4] float64 on the device: entry, distance,
      shift, heading), then adds it -- in that order, so a scan never finds itself; exclude_recent keeps its neighbours
      out.  Nine launches with candidates (seven with num_candidates=0).  No threshold is applied and nothing is
      corrected: verification and the pose graph are the caller's.  reset() empties the database.  Unknown keys, or
      loop without places, are errors at construction.  None (the default): no database.
    * Pose graph: pose_graph=PoseGraph(...) (rslo_amd/posegraph.py, csrc/posegraph.hip) lets the caller close loops over
      what has been streamed: close_loops(loops_ij, loops_Z, loops_w=None, **options) optimises a COPY of
      refined_trajectory() when there is a refined chain, else of the open-loop trajectory, with PoseGraph.optimize's
      options, on the caller's stream; optimized_trajectory() and pose_graph_info() return the result.  Both chains
      stay what they are, bit for bit, and step() does not change.  Feeding the corrected poses back is rebuild_map()
      / adopt_loop_closure() (below), both opt-in.  The loop measurements are the caller's, or the back end's own with
      verify= (next).  None (the default): close_loops raises.
    * Loop verification: keyframes=KeyframeStore(...) (rslo_amd/loops.py, csrc/loopverify.hip) with verify=dict(...)
      (the options of loops.check_verify -- stages, max_distance, inlier_dist, min_overlap, max_rms, min_pairs, damping
      -- plus edge_w=(1.0, 1.0) and max_edges=256; needs places) turns the candidates into measured loop edges on the
      device: behind places.describe / query and before places.add, step() calls keyframes.prepare(the scan), verifies
      row n of loop_candidates() into row n of loop_checks() ([n, top_k, 16]: status, entry, pairs, overlap, rms,
      query count, Z, distance, heading, 0) in ONE launch, emits the best accepted row into the edge list
      loop_edges() = (ij, Z, w, counters) and then keyframes.add().  A fixed number of launches.
      close_verified_loops(**options) is close_loops on that edge list (its unused rows hold i = j = -1, which the
      pose graph skips), with no host read.  The capacities of places and keyframes must reach `capacity` (an entry's
      index is its scan's index), and max_edges must not exceed pose_graph.max_loops.  keyframes= without verify= only
      stores the frames.  reset() empties the store and the edge list.  Unknown keys are an error at construction.
    * The map after loop closure (needs keyframes=): rebuild_map(voxel_map=None, poses=None) resets the given VoxelMap
      or MapPyramid (default: the back end's own) and fills it with every stored keyframe under its own row of poses
      (default: optimized_trajectory()) in ONE call per level (VoxelMap.insert_frames, rslo_map_insert_frames: three
      launches whatever the number of scans), on the caller's stream, with no host read.  The rebuilt map has the
      density of the KEYFRAMES, not of the scans: voxel_size centroids of the store, at most K per scan, about one hit
      per cell per frame.  A caller who refines with min_hits > 1, or wants a 0.2 m map, builds the store with
      voxel_size=0.2, K=4096.  adopt_loop_closure() (with a refined chain, after close_loops() /
      close_verified_loops() of everything streamed so far) takes the correction into the refined chain: the optimised
      rows replace rows 0 .. n-1 of refined_trajectory() (a later close_loops() would otherwise read the correction as
      one huge odometry edge between n-1 and n), the chain's state becomes optimised row n-1, so that the next scan's
      prediction composes onto the corrected pose, and rebuild_map() makes the back end's own map consistent before
      that scan is registered against it: n is unchanged, so the next insert is scan n and local_map's grace keeps its
      meaning.  The open-loop chain, the place database, the keyframe store and the edge list are untouched.  Evicting
      keyframes is out of scope.  Neither method is called by step().
    * Surfel map: surfels=SurfelMap(...) (rslo_amd/surfels.py, csrc/surfel.hip) receives every scan beside the voxel map
      (or alone): step() inserts the scan under the row the voxel map uses -- the refined chain when there is one, else
      the open-loop chain.  surfel_refine=dict(iters=4, max_dist=None, robust_scale=0.2, damping=1e-6, min_pairs=50,
      tol_t=0.0, tol_r=0.0) (these defaults; needs surfels) adds a registration stage against the surfel map's planes
      (SurfelMap.register: no scan normal is read, so raw scans get a plane metric): it creates the refined chain when
      refine= is absent, and corrects row n of it in place behind refine's own stage (if any); then the chain state is
      set and both maps are filled.  Scan 0 meets an empty table (status 1) and stays the identity.  With
      cost="distribution" among the options (then also min_flag=1, reg_rel=0.01, reg_abs=0.02, and robust_scale
      defaults to 3.0 sigmas) the stage is the point-to-distribution cost over every fitted cell
      (SurfelMap.register(cost="distribution")), which also refines where the map holds no planes.
      surfel_refine_info() is the [n, iters, 8] info.  reset() empties the surfel map; rebuild_map() on the back end's
      own maps and adopt_loop_closure() also reset it and refill it from the keyframe store under the same poses
      (SurfelMap.insert_frames).  The table only fills unless local_map= carries the surfels key (above): then it is
      pruned about the sensor every K scans and a long drive runs in a fixed table.
    * De-skewing: deskew=dict(motion="network", times="azimuth", stamp=0.5, az_start_turn=-0.5, az_clockwise=False,
      max_angle=pi/2) (these defaults; rslo_amd/deskew.py, csrc/deskew.hip) motion-compensates every sweep before the
      other stages see it: first of all, step() de-skews the scan into its own [point_capacity, F] buffer -- the
      normals are rotated when F >= 7, the caller's tensor is not written -- and both register stages, both map
      inserts, places.describe and keyframes.prepare read that buffer instead of the submitted tensor.  One launch per
      scan (the buffer is made by the first check_scan(), which fixes F).  The motion of the sweep: motion="network"
      uses rel[n] of the open-loop chain, and none for n == 0 (the pair is the scan with itself); motion="refined"
      (needs refine= or surfel_refine=, whose chain starts at the identity) uses between(refined[n-2], refined[n-1]),
      the constant-velocity model on the corrected chain, and none for n < 2.  times="azimuth" dates a return by its
      azimuth (a sweep from az_start_turn, in turns, counter-clockwise unless az_clockwise); times="input" takes
      step(cloud, times): one contiguous fp32 CUDA [P] tensor of sweep fractions per scan.  deskew_info() is the [n, 8]
      motion blocks {axis, angle, t', status} on the device, deskewed() the view of the last scan.  Unknown keys are
      errors at construction.
    * Free-space carving: carve=dict(every=1, rows=64, cols=1024, tan_lo=tan(-25 deg), tan_hi=tan(3 deg), win_rows=1,
      win_cols=1, margin_abs=0.3, margin_rel=0.0, max_range=60.0, grace=1) (these defaults; rslo_amd/carve.py,
      csrc/carve.hip; needs voxel_map) removes what moves: when (n + 1) % every == 0, behind the registration of scan n
      and in FRONT of its insert, step() builds the range image of the scan the stages read (the de-skewed buffer with
      deskew=; `range_image` holds it) and calls voxel_map.carve(image, row n of the chain that feeds the insert) -- a
      VoxelMap, or every level of a MapPyramid (VoxelMap.carve; include/rslo_hip.h "Free-space carving").  Two
      launches for the image and five per map level (the image and the rebuild's workspace are made at construction).
      The surfel map is not carved.  Unknown keys are errors at construction.
    Every option's default is None: nothing of it is built and none of its launches is issued."""

    def __init__(self, chain, capacity=8192, point_capacity=160000, device="cuda", voxel_map=None, refine=None,
                 local_map=None, places=None, loop=None, pose_graph=None, keyframes=None, verify=None, surfels=None,
                 surfel_refine=None, deskew=None, carve=None):
        from rslo_amd import carve as carve_mod, loops
        opts = check(capacity, device, voxel_map=voxel_map, refine=refine, local_map=local_map, places=places, loop=loop,
                     pose_graph=pose_graph, keyframes=keyframes, verify=verify, surfels=surfels, surfel_refine=surfel_refine,
                     deskew=deskew, carve=carve)
        self.chain, self.capacity, self.point_capacity = chain, int(capacity), int(point_capacity)
        self.device = dev = _device(device)
        self.n = 0                 # scans of the current sequence (host mirror of the chains' device counters)
        self.voxel_map, self.surfels, self.places, self.keyframes, self.pose_graph = voxel_map, surfels, places, keyframes, pose_graph
        self.refine, self.surfel_refine, self.local_map = opts["refine"], opts["surfel_refine"], opts["local_map"]
        self.loop, self.verify, self.deskew, self.carve = opts["loop"], opts["verify"], opts["deskew"], opts["carve"]
        for owner in (voxel_map, surfels, places, keyframes):
            if owner is not None:
                owner.reserve(self.point_capacity)      # step() must not allocate
        info = lambda *shape: torch.zeros((self.capacity,) + shape, dtype=torch.float64, device=dev)
        self.refined = None        # the second chain
        if self.refine is not None or self.surfel_refine is not None:
            self.refined = PoseChain(self.capacity, dev)
        self._refine_info = None if self.refine is None else info(opts["info_rows"], 8)
        self._surfel_info = None if self.surfel_refine is None else info(self.surfel_refine["iters"], 8)
        if self.local_map is not None:
            if "surfels" in self.local_map:
                surfels.reserve_prune()                 # step() must not allocate
            if voxel_map is not None:
                voxel_map.reserve_prune()
        self.range_image = None
        if self.carve is not None:
            c = self.carve
            self.range_image = carve_mod.RangeImage(c["rows"], c["cols"], c["tan_lo"], c["tan_hi"], dev)
            self._carve_kw = {k: c[k] for k in ("win_rows", "win_cols", "margin_abs", "margin_rel", "max_range", "grace")}
            voxel_map.reserve_prune()                   # the rebuild shares prune's workspace
        self._candidates = None if places is None else info(self.loop["top_k"], 4)
        self._verifier = self._edges = self._checks = None
        if self.verify is not None:
            self._verifier = loops.LoopVerifier(keyframes, **self.verify)
            self._edges = loops.EdgeList(opts["edges"][0], opts["edges"][1], device=dev)
            self._checks = info(self.loop["top_k"], loops.OUT_COLS)
        self._deskewer = self._deskewed = None      # the stage is built by the first check_scan(), which fixes F
        self._deskew_info = None if self.deskew is None else info(8)
        self._optimized = self._pg_info = None

    @property
    def reads_scans(self):
        """whether step() reads its source at all: the caller may drop the tensor otherwise"""
        return any(x is not None for x in (self.voxel_map, self.places, self.keyframes, self.surfels, self.deskew))

    def check_scan(self, cloud, times=None):
        """What a scan must be for step() to read it (ValueError), checked when the caller takes it in; the first scan
        of a de-skewing back end fixes the width of the buffer, which is allocated here."""
        on_device = lambda t: torch.is_tensor(t) and t.device.type == self.device.type
        if self.reads_scans and not (on_device(cloud) and cloud.dtype == torch.float32 and cloud.dim() == 2):
            raise ValueError("a back end that reads the scans (a map, a place database, a keyframe store or de-skewing) "
                             "takes one fp32 CUDA [P, F] tensor")
        if times is not None and (self.deskew is None or self.deskew["times"] != "input"):
            raise ValueError("a times tensor needs deskew=dict(times=\"input\")")
        if self.deskew is None:
            return
        P, F = cloud.shape
        if self.deskew["times"] == "input" and not (on_device(times) and times.shape == (P,)
                                                    and times.dtype == torch.float32 and times.is_contiguous()):
            raise ValueError("deskew times=\"input\" takes a contiguous fp32 CUDA [P] tensor of sweep fractions with every scan")
        if P > self.point_capacity:
            raise ValueError("the scan exceeds point_capacity = %d" % self.point_capacity)
        if self._deskewer is None:
            from rslo_amd import deskew as deskew_mod
            self._deskewer = deskew_mod.Deskewer(self.point_capacity, F, self.device, **self.deskew)
        elif self._deskewer.n_cols != F:
            raise ValueError("the de-skewing buffer holds [P, %d] scans, got [P, %d]" % (self._deskewer.n_cols, F))

    def step(self, source, times=None):
        """Scan n = self.n behind its push onto the open-loop chain: `source` is the tensor the caller submitted (None
        when reads_scans is False), `times` its sweep fractions with deskew=dict(times="input")."""
        n = self.n
        if n >= self.capacity:
            raise capi.RsloHipError("BackEnd: more than %d scans in one sequence (capacity); reset() or a larger capacity"
                                    % self.capacity)
        if self.deskew is not None:         # behind the head (rel[n] is written), before the second chain: one launch
            if self._deskewer is None:
                self.check_scan(source, times)
            if self.deskew["motion"] == "network":
                motion = dict(rel7=self.chain.rel[n]) if n >= 1 else {}
            else:                           # constant velocity on the corrected chain, whose rows below n are final
                motion = dict(pose_a=self.refined.traj[n - 2], pose_b=self.refined.traj[n - 1]) if n >= 2 else {}
            source = self._deskewed = self._deskewer(source, times, motion_out=self._deskew_info[n], **motion)
        row = (self.chain if self.refined is None else self.refined).traj[n]      # places this scan in the maps
        if self.refined is not None:        # the second chain: predict from the refined pose, register, compose onto the result
            rel = self.chain.rel[n]
            self.refined.push(rel[:3], rel[3:])
            if self.refine is not None:
                self.voxel_map.register(source, row, info=self._refine_info[n], **self.refine)
            if self.surfel_refine is not None:      # behind refine's own stage, on the same row
                self.surfels.register(source, row, info=self._surfel_info[n], **self.surfel_refine)
            self.refined.set_state(row)
        if self.carve is not None and (n + 1) % self.carve["every"] == 0:      # behind the registration, in front of the insert
            self.voxel_map.carve(self.range_image(source), row, **self._carve_kw)
        if self.voxel_map is not None:      # behind the pose chain (and the registration) that wrote row n, on this stream
            self.voxel_map.insert(source, row)
        if self.surfels is not None:
            self.surfels.insert(source, row)
        if self.local_map is not None and (n + 1) % self.local_map["every"] == 0:
            lm = self.local_map
            if self.voxel_map is not None:
                self.voxel_map.prune(row, lm["radius"], lm["min_hits"], lm["grace"])
            if "surfels" in lm:                 # the same row and the same radius
                self.surfels.prune(row, lm["radius"], lm["surfels"]["inner_radius"], lm["surfels"]["min_count"])
        if self.places is not None:         # describe -> query -> add: the scan is searched for before it is stored
            self.places.describe(source)
            self.places.query(out=self._candidates[n], **self.loop)
            if self.keyframes is not None:  # prepare -> verify -> emit -> add: an edge's j is the store's count before add
                self.keyframes.prepare(source)
                if self._verifier is not None:
                    self._verifier.verify(self._candidates[n], out=self._checks[n])
                    self._edges.emit(self._checks[n], self.keyframes)
                self.keyframes.add()
            self.places.add()
        elif self.keyframes is not None:
            self.keyframes.prepare(source)
            self.keyframes.add()
        self.n += 1

    def reset(self):
        """A new sequence: every map, the database, the store and the edge list are emptied, the refined chain restarts.
        The open-loop chain is its owner's to reset."""
        self.n = 0
        self._deskewed = self._optimized = self._pg_info = None
        for owner in (self.voxel_map, self.surfels, self.refined, self.places, self.keyframes, self._edges):
            if owner is not None:
                owner.reset()

    def close_loops(self, loops_ij, loops_Z, loops_w=None, **options):
        """Optimise a copy of the streamed trajectory (the refined chain when there is one) under the loop edges
        (loops_ij int32 [L, 2] scan indices, loops_Z float64 [L, 7] the pose of j in the frame of i, loops_w [L, 2] or
        None for ones; options: PoseGraph.optimize's).  Returns (poses, info), also kept for optimized_trajectory() and
        pose_graph_info().  Nothing that is streamed is changed."""
        if self.pose_graph is None:
            raise capi.RsloHipError("close_loops: built without pose_graph")
        if "poses" in options:
            raise capi.RsloHipError("close_loops: the start is the streamed trajectory itself")
        traj0 = (self.chain if self.refined is None else self.refined).traj[:self.n]
        self._optimized, self._pg_info = self.pose_graph.optimize(traj0, loops_ij, loops_Z, loops_w, **options)
        return self._optimized, self._pg_info

    def close_verified_loops(self, **options):
        """close_loops() on the back end's own edge list (verify=...): the whole fixed-size list goes to the pose graph,
        which skips its unused rows; nothing is read on the host."""
        e = self._need(self._edges, "close_verified_loops: built without verify")
        return self.close_loops(e.ij, e.Z, e.w, **options)

    def rebuild_map(self, voxel_map=None, poses=None):
        """Reset voxel_map (a VoxelMap or MapPyramid; default: the back end's own) and insert every stored keyframe under
        its own row of poses (float64 CUDA [m, 7]; default: optimized_trajectory()): the map the corrected trajectory
        implies, at the density of the keyframes.  On the caller's stream, no host read.  Returns the map.  With the
        back end's own map as the target (voxel_map=None) an attached SurfelMap is reset and refilled the same way; a
        back end with surfels= and no voxel_map rebuilds the surfel map alone (and returns None)."""
        if self.keyframes is None:
            raise capi.RsloHipError("rebuild_map: built without keyframes")
        vmap = self.voxel_map if voxel_map is None else voxel_map
        own_surfels = self.surfels if voxel_map is None else None      # the back end's own maps are rebuilt together
        if vmap is None and own_surfels is None:
            raise capi.RsloHipError("rebuild_map: no voxel_map given and none was built in")
        if poses is None:
            poses = self._need(self._optimized, "rebuild_map: no poses given and close_loops() has not run")
        for m in (vmap, own_surfels):
            if m is not None:
                m.reset()
                m.insert_frames(self.keyframes, poses)
        return vmap

    def adopt_loop_closure(self):
        """Take the last close_loops() into the refined chain (class docstring): its rows, its state, and the back end's
        own map rebuilt from the keyframes.  The open-loop chain and everything else that is streamed stay."""
        if self.refined is None or self.keyframes is None:
            raise capi.RsloHipError("adopt_loop_closure: needs refine= (or surfel_refine=) and keyframes=")
        poses = self._need(self._optimized, "adopt_loop_closure: close_loops() has not run")
        n = int(poses.shape[0])
        if n != self.n:
            raise capi.RsloHipError("adopt_loop_closure: close_loops() optimised %d scans, %d have been streamed; close the "
                                    "loops again first" % (n, self.n))
        self.refined.traj[:n].copy_(poses)
        self.refined.set_state(poses[n - 1])
        self.rebuild_map()

    @staticmethod
    def _need(value, message):
        if value is None:
            raise capi.RsloHipError(message)
        return value

    def _rows(self, buf, name, option):
        """rows 0 .. n-1 of a per-scan buffer that exists only with `option`"""
        if buf is None:
            raise capi.RsloHipError("%s: built without %s" % (name, option))
        return buf[:self.n]

    def refined_trajectory(self):
        """[n, 7] fp64 device rows of the refined chain (refine=...): row i = register(refined[i-1] o rel[i])."""
        return self._rows(None if self.refined is None else self.refined.traj, "refined_trajectory", "refine")

    def refine_info(self):
        """[n, iters, 8] fp64 device rows: VoxelMap.register's info of every scan."""
        return self._rows(self._refine_info, "refine_info", "refine")

    def surfel_refine_info(self):
        """[n, iters, 8] fp64 device rows (surfel_refine=...): SurfelMap.register's info of every scan."""
        return self._rows(self._surfel_info, "surfel_refine_info", "surfel_refine")

    def deskew_info(self):
        """[n, 8] fp64 device rows (deskew=...): the motion block {axis, angle, t', status} every scan was de-skewed with."""
        return self._rows(self._deskew_info, "deskew_info", "deskew")

    def loop_candidates(self):
        """[n, top_k, 4] fp64 device rows (places=...): PlaceDB.query's result of every scan against the scans before it."""
        return self._rows(self._candidates, "loop_candidates", "places")

    def loop_checks(self):
        """[n, top_k, 16] fp64 device rows (verify=...): LoopVerifier.verify's result of every scan's candidates."""
        return self._rows(self._checks, "loop_checks", "verify")

    def loop_edges(self):
        """(ij int32 [E, 2], Z fp64 [E, 7], w fp64 [E, 2], counters int64 [2] = {n_edges, dropped_full}) on the device
        (verify=...): the edges emitted so far; unused rows hold i = j = -1."""
        return self._need(self._edges, "loop_edges: built without verify").tensors()

    def deskewed(self):
        """The [P, F] fp32 view of the buffer that holds the last scan de-skewed (deskew=...); the next step()
        overwrites it."""
        if self.deskew is None:
            raise capi.RsloHipError("deskewed: built without deskew")
        return self._need(self._deskewed, "deskewed: no scan has been stepped since reset()")

    def optimized_trajectory(self):
        """[n, 7] fp64 device rows: the result of the last close_loops()."""
        return self._need(self._optimized, "optimized_trajectory: close_loops() has not run (or built "
                                                        "without pose_graph)")

    def pose_graph_info(self):
        """[gn_iters, 8] fp64 device rows: PoseGraph.optimize's info of the last close_loops()."""
        return self._need(self._pg_info, "pose_graph_info: close_loops() has not run (or built without "
                                                      "pose_graph)")
