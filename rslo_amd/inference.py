"""Frame-after-frame inference of the sparse GU encoder from ONE hipGraph per plan arena.

evaluate.py:363-408 runs the same eval-mode forward for every frame of a sequence (rslo/models/middle.py:219-245 for the
encoder).  Issued eagerly that pass is ~40 dependent launches on levels of 2.6 k .. 31 k rows: 0.6 ms of launch chain for
54 us of roofline work, plus the interpreter time of building a plan's tensor views for every frame.  Here

  * the structure work of a frame (voxelization + every rulebook: rslo_plan_encoder, one foreign call) goes into a
    CAPACITY-laid-out arena whose rows past each level's count are padding rows (rslo_plan_encoder_pad_tails), so every
    pointer and every shape the encoder's kernels see depends on the arena only, not on the scan;
  * VFE + all convolutions + dense() of an arena are captured once into a hipGraph (torch.cuda.graph over the same modules,
    the same kernels: capi launches go to the capture stream) and REPLAYED for every later frame planned into that arena:
    one launch of the graph per frame, counts stay on the device, no host read anywhere;
  * the coming frames' structure work is issued by a helper thread on a side stream while the current frame's graph runs.

Outputs of the VALID rows (and the whole BEV map: padding rows are never scattered) equal the eager pass bit for bit:
same kernels, and the tilings that depend on a level's size are pinned to what the eager pass of a single scan picks
(`capi.tuning(spconv_rbw=1, spconv_ks=4)`: 16-row tiles shared by four waves, csrc/spconv.hip).
"""
import queue
import threading

import torch

from rslo_amd import capi
from rslo_amd.plan import EncoderPlanner


class _Handle:
    __slots__ = ("slot", "job", "error", "issued", "source", "times")

    def __init__(self, slot):
        self.slot, self.job, self.error, self.issued = slot, None, None, threading.Event()
        self.source = None      # OdometryRunner with a voxel map: the tensor the caller passed to submit()
        self.times = None       # OdometryRunner with deskew=dict(times="input"): the scan's sweep fractions


class EncoderGraphRunner:
    """runner = EncoderGraphRunner(net_like)       # .middle_feature_extractor (eval mode), .voxel_generator
       job = runner.submit(cloud)                   # structure work of one scan, on the runner's side stream
       bev, cov, n_rows = runner.run(job)           # graph replay on the current stream; cov[:n_rows] are the valid rows
    `bev` / `cov` are static tensors of the job's arena: consume (or copy) them before that arena's next run()."""

    def __init__(self, net_like, max_voxels, device="cuda", point_capacity=160000, arenas=4, frames_per_job=1,
                 with_cov=True, pre_plan=None):
        self.net = net_like
        # optional hook of the helper thread: pre_plan(cloud, arena, k) -> the [P,F] cloud to plan, issued on the plan stream
        # immediately in front of the structure work of frame k of a job (behind the wait for the arena's previous frame), so
        # it may write per-arena buffers.  It must not synchronise, allocate per call or open a stream.  None: off.
        self.pre_plan = pre_plan
        self.with_cov = bool(with_cov)      # False: the covariance branch is not issued (run() returns cov = None)
        self.enc = net_like.middle_feature_extractor
        if self.enc.training:
            raise capi.RsloHipError("EncoderGraphRunner is an inference path: put the encoder in eval() mode")
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.planner = EncoderPlanner(net_like, max_voxels, arenas=arenas)
        self.point_capacity = int(point_capacity)
        self.frames = int(frames_per_job)
        # structure stream(s), used round-robin.  One is the measured choice: a plan alone takes 0.43 ms per scan on one stream and
        # 0.26 on two alternating ones, but beside the replayed pass two or three streams change nothing (0.75-0.77 ms per scan)
        import os
        prio = os.environ.get("RSLO_INFER_PLAN_PRIORITY", "")
        self.sides = [torch.cuda.Stream(self.device, **({"priority": int(prio)} if prio else {}))
                      for _ in range(int(os.environ.get("RSLO_INFER_PLAN_STREAMS", "1")))]
        self._exact_planner = EncoderPlanner(net_like, max_voxels, arenas=2)
        self.fallbacks = 0
        self._seq = 0
        self._queue = queue.Queue()
        self._thread = threading.Thread(target=self._work, daemon=True)
        self._thread.start()
        self.stats = {"plans": 0, "helper_s": 0.0, "ready_wait_s": 0.0, "runs": 0}      # host-side time split (bench.py c2)
        self._graphs = {}          # arena slot -> (graph, bev, cov, rows_dev0, arena data_ptr)
        self._last_use = {}        # arena slot -> event recorded behind the last replay that read the arena
        self._pending = {}         # arena slot -> scan submitted into it and not yet run()

    def submit(self, clouds):
        """clouds: one CUDA fp32 [P,F] tensor (or a list of `frames_per_job` of them).  Returns a handle for run().  The
        structure work is issued by the runner's helper thread (one foreign call of ~60 launches: 0.3-0.5 ms of host time
        that would otherwise sit in front of every replay on the calling thread)."""
        if torch.is_tensor(clouds):
            clouds = [clouds]
        slot = self._seq
        a = slot % self.planner.n_arenas
        if a in self._pending:
            # the plan of this scan would overwrite tables the pending replay of handle `self._pending[a]` still has to read
            raise capi.RsloHipError("EncoderGraphRunner.submit: arena %d still holds scan %d, which has not been run(); keep fewer "
                                    "than %d handles outstanding" % (a, self._pending[a], self.planner.n_arenas))
        self._seq += 1
        self._pending[a] = slot
        h = _Handle(slot)
        prev = self._last_use.get(a)
        self._queue.put((h, clouds, prev))
        return h

    def _work(self):
        torch.cuda.set_device(self.device)
        while True:
            item = self._queue.get()
            if item is None:
                return
            h, clouds, prev = item
            import time as _t
            t0 = _t.perf_counter()
            try:
                side = self.sides[h.slot % len(self.sides)]
                with torch.cuda.stream(side):
                    if prev is not None:
                        side.wait_event(prev)               # the arena's previous frame has been consumed on the GPU
                    if self.pre_plan is not None:
                        a = h.slot % self.planner.n_arenas
                        clouds = [self.pre_plan(c, a, k) for k, c in enumerate(clouds)]
                    h.job = self.planner.submit([[c] for c in clouds], with_pairs=False, slot=h.slot,
                                                point_capacity=self.point_capacity)
            except Exception as e:      # surfaces in run()
                h.error = e
            self.stats["plans"] += 1
            self.stats["helper_s"] += _t.perf_counter() - t0
            h.issued.set()

    def close(self):
        self._queue.put(None)
        self._thread.join(timeout=10)

    def _forward(self, job):
        vox, num, plan, rows_dev = self.planner.finish_static(job)
        x = capi.vfe_mean(vox, num)
        bev, cov = self.enc(x, plan.indices, job.n_clouds, plan=plan, defer_cov=not self.with_cov)
        return bev, cov if self.with_cov else None, rows_dev[0]

    def _exact(self, job):
        """Exact-size plan + eager pass of a scan whose static plan overflowed a level's capacity (fresh tensors, no graph)."""
        ex = self._exact_planner.finish(self._exact_planner.submit(job.clouds, with_pairs=False))
        vox, num = ex["_frame_major"]
        with torch.no_grad():
            bev, cov = self.enc(capi.vfe_mean(vox, num), ex["sparse_plan"].indices, job.n_clouds, plan=ex["sparse_plan"],
                                defer_cov=not self.with_cov)
        if not self.with_cov:
            return bev, None, torch.tensor([vox.shape[0]], dtype=torch.int32, device=bev.device)
        return bev, cov, torch.tensor([cov.shape[0]], dtype=torch.int32, device=cov.device)

    def _capture(self, job, cur):
        """Warm up on a side stream (lazy initialisation inside the modules must not be captured), then capture the pass over
        the job's arena.  The tilings that depend on a level's size are pinned to the single-scan choice (module docstring)."""
        with torch.no_grad(), capi.tuning(spconv_rbw=1, spconv_ks=4):
            s = torch.cuda.Stream(self.device)
            s.wait_stream(cur)
            with torch.cuda.stream(s):
                for _ in range(2):
                    self._forward(job)
            cur.wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                bev, cov, n0 = self._forward(job)
        return g, bev, cov, n0, job.arena.data_ptr()

    def run(self, handle, graph=True):
        """The encoder pass of a submitted scan on the current stream: a replay of its arena's graph (captured on first use),
        or, graph=False, the same modules issued eagerly over the same capacity-laid-out plan."""
        if not handle.issued.wait(timeout=60.0):
            raise capi.RsloHipError("EncoderGraphRunner: the helper thread did not issue the scan's structure work")
        if handle.error is not None:
            raise handle.error
        job = handle.job
        if self._pending.get(handle.slot % self.planner.n_arenas) == handle.slot:
            del self._pending[handle.slot % self.planner.n_arenas]
        cur = torch.cuda.current_stream(self.device)
        # the counts block of the job reached pinned memory behind job.ready; it was submitted `depth` scans ago, so the event has
        # normally passed and this is a read of host memory, not a wait.  A level that outgrew its capacity (not a LiDAR-shaped
        # scan) cannot be replayed: that scan takes the exact-size eager pass.
        import time as _t
        t0 = _t.perf_counter()
        job.ready.synchronize()
        self.stats["ready_wait_s"] += _t.perf_counter() - t0
        self.stats["runs"] += 1
        if int(job.counts[capi.PLAN_CNT_OVERFLOW]) != 0:
            self.fallbacks += 1
            return self._exact(job)
        a = job.slot % self.planner.n_arenas
        if graph:
            ent = self._graphs.get(a)
            if ent is None or ent[4] != job.arena.data_ptr():
                ent = self._graphs[a] = self._capture(job, cur)
            ent[0].replay()
            out = ent[1], ent[2], ent[3]
        else:
            with torch.no_grad(), capi.tuning(spconv_rbw=1, spconv_ks=4):
                out = self._forward(job)
        ev = torch.cuda.Event()
        ev.record(cur)
        self._last_use[a] = ev
        return out


def pose_chain_host(rows):
    """The recurrence of rslo_pose_chain on the host, one scan at a time, float64: rows [N,7] (t, q wxyz) -> poses [N,7].
    Scan 0 seeds the state with its own odometry and is the identity (the quirk of geometric.odom_to_abs_pose).  The
    translation update is form B: see se3.py."""
    import numpy as np
    rows = np.asarray(rows, dtype=np.float64)
    out = np.zeros_like(rows)
    t = q = None
    for i, r in enumerate(rows):
        if i == 0:
            t, q = r[:3].copy(), r[3:].copy()
            out[0] = (0, 0, 0, 1, 0, 0, 0)
            continue
        ti, qi = r[:3], r[3:]
        b = np.cross(q[1:], ti)
        t = t + (ti + 2.0 * b * q[0] + 2.0 * np.cross(q[1:], b))
        p = np.concatenate([[q[0] * qi[0] - np.dot(q[1:], qi[1:])], q[1:] * qi[0] + qi[1:] * q[0] + np.cross(q[1:], qi[1:])])
        q = p / (np.linalg.norm(p) + 1e-6)
        out[i, :3], out[i, 3:] = t, q
    return out


class OdometryRunner:
    """Streaming odometry of the whole network in eval mode (evaluate.py:363-408 fed one scan at a time):

        runner = OdometryRunner(net)        # UnVoxelOdomNetICP3 in eval(), CUDA, fp32
        h = runner.submit(cloud)            # [P, 7] fp32 CUDA scan, in sequence order
        rel, pose = runner.run(h)           # [7] (t, q) each: odometry of (previous, this) and absolute pose
        traj = runner.trajectory()          # [N, 7] fp64 device tensor = odom_to_abs_pose of the rel rows
        runner.reset()                      # new sequence: the next scan pairs with itself, the trajectory restarts
        runner.feed(clouds)                 # THE way to drive a runner over a list of scans: submit one ahead, run

    * Encoder: an EncoderGraphRunner with one frame per job and no covariance branch (poses do not depend on it): every
      scan is voxelized, planned and encoded ONCE.  (The dataset builds example i from frames (max(i-1, 0), i), so an
      eager loop encodes every scan twice; in eval mode a frame's encoding does not depend on its partner.)
    * Pair map: the head's static input [1, 2C, H, W] = [previous | current], the channel order of
      voxel_odom_net.network_forward: per scan the current half moves to the previous half and the scan's BEV map is
      copied in (two device copies of C*H*W floats); the first scan of a sequence is paired with itself.
    * Head: the eval forward without autograd (odom_pred._forward_eval_fused: every conv -> BN -> activation one launch of
      a hand-written kernel) plus the pose chain (rslo_pose_chain, float64 state, row n of the trajectory) captured
      once into a hipGraph over that static input and replayed once per scan on the caller's stream.  Both graphs are
      single-stream captures; no stream is opened beyond the encoder runner's plan stream.
    * Weights: split operands and folded BatchNorms are derived outside the graph (hip_conv2d.EvalOperands) and
      re-derived before the next replay when a parameter or running statistic of the head changed in place
      (load_state_dict, an optimizer step, bn.running_var.mul_(...)); a storage that moved is re-planned and the head
      graph captured again.  A replaced parameter object, or a write through `.data` (it bumps no version counter):
      call refresh_weights(force=True).
    * Handles: the outstanding-handle rule of EncoderGraphRunner (fewer than `arenas` submitted and not yet run).  feed()
      keeps it for the caller: it submits scan i + 1, then runs scan i, so two handles are outstanding at the most and the
      helper thread plans one scan ahead of the device.  submit() / run() by hand are for callers that read `rel` / `pose`.
    * Raw scans: normals="estimate" takes what a LiDAR produces, [P, 4] (x, y, z, intensity; or [P, 3], intensity 0):
      the helper thread builds the [P, 7] cloud with capi.append_normals (csrc/normals.hip: the offline step of
      script/create_hdf5.py:130-147 with normal_radius / normal_max_nn, plus the reader's zero_vertical rule) on the plan
      stream immediately in front of the scan's structure work, into buffers allocated once per arena.  No stream is
      added and nothing synchronises.  normals="input" (the default) is the path above, unchanged.
    * World map: voxel_map=VoxelMap(...) (rslo_amd/mapping.py, csrc/map.hip) registers every scan: run() inserts the tensor
      the caller passed to submit() (its first four columns are x, y, z, intensity in both input forms) under row n of
      the trajectory, on the caller's stream behind the head and pose chain of that scan: at most three launches, no
      synchronisation.  The encoder job's cloud is NOT read: with normals="estimate" it is an arena buffer the helper
      thread may overwrite as soon as the event recorded by EncoderGraphRunner.run has passed.  The caller keeps the
      submitted tensor unmodified until run() of its handle has been consumed on the device.  reset() also resets the
      map (a new sequence has a new frame); its figures come from voxel_map.stats().  None (the default): no map.
    * Refinement: refine=dict(iters=3, ...) (keyword arguments of VoxelMap.register except metric; needs voxel_map)
      registers every scan against the map before inserting it (csrc/mapreg.hip).  The runner then keeps a SECOND chain
      beside the open-loop one, driven by the same rslo_pose_chain outside the head graph: behind the head replay,
      pose_chain(rel[n]) on it writes the prediction refined[n-1] o rel[n] into row n, voxel_map.register corrects that
      row in place (metric "plane" for [P, >= 7] input, "point" for raw scans), the chain's state is set to the
      corrected row so that the next scan composes onto it, and the scan is inserted under it.  trajectory() and
      relative() stay the open-loop chain, bit for bit; refined_trajectory() is the second chain and refine_info() the
      [n, iters, 8] info rows of register, both on the device.  A fixed number of launches per scan, no
      synchronisation, no stream.  None (the default): today's behaviour to the bit.
    * Coarse-to-fine refinement: voxel_map=MapPyramid(...) (one VoxelMap per voxel size) with
      refine=dict(schedule=[(level, iters, max_dist or None, robust_scale), ...]) -- or refine=dict(): the pyramid's
      default_schedule() -- runs MapPyramid.register (rslo_map_register_sched, one call) where VoxelMap.register runs
      above; insert, reset and prune reach every level; refine_info() is [n, sum of iters, 8] with stage and level in
      columns 5 and 6.  refine=dict(robust_scale=s) on a plain VoxelMap weights its iterations.  schedule= with a plain
      VoxelMap, or together with iters=, is an error at construction.
    * Rolling local map: local_map=dict(radius=R, every=K, min_hits=1, grace=0) (needs voxel_map) keeps the map near the
      sensor: behind the insert of scan n (counted from 0 since reset()), when (n + 1) % K == 0, run() calls
      voxel_map.prune(center=row n of the chain that fed the insert, radius=R, min_hits=, grace=) -- the refined chain
      with refine, else the open-loop one (VoxelMap.prune; include/rslo_hip.h "Rolling local map").  The decision is
      the host's own scan count: no device read.  The workspace (about one more table) is reserved here, so run()
      allocates nothing.  trajectory() / relative() are untouched.  None (the default): the map only grows.  One more,
      optional key, surfels=True or surfels=dict(min_count=1, inner_radius=None) (needs surfels=; a voxel_map is then
      no longer required), prunes the surfel map too: behind the surfel insert of the same scans run() calls
      surfels.prune(the same row, R, inner_radius, min_count) (SurfelMap.prune; "Rolling local surfel map"), with its
      workspace reserved here as well.  Without the key the surfel map is never pruned and the launches are today's.
    * Place recognition: places=PlaceDB(...) (rslo_amd/places.py, csrc/places.hip) with
      loop=dict(exclude_recent=50, num_candidates=10, top_k=1) (these defaults; keyword arguments of PlaceDB.query):
      behind everything above, run() describes the tensor passed to submit() (sensor frame, its first three columns),
      queries the database with that descriptor into row n of loop_candidates() ([n, top_k, 4] float64 on the device:
      entry, distance, shift, heading), then adds it -- in that order, so a scan never finds itself; exclude_recent
      keeps its neighbours out.  Nine launches with candidates (seven with num_candidates=0) on the caller's stream, no
      synchronisation, nothing allocated.  No threshold is applied and nothing is corrected: verification and the pose
      graph are the caller's.  reset() empties the database.  Unknown keys, or loop without places, are errors at
      construction.  None (the default): no database, today's bits.
    * Pose graph: pose_graph=PoseGraph(...) (rslo_amd/posegraph.py, csrc/posegraph.hip) lets the caller close loops over
      what has been streamed: close_loops(loops_ij, loops_Z, loops_w=None, **options) optimises a COPY of
      refined_trajectory() when the runner refines, else of trajectory(), with PoseGraph.optimize's options, on the
      caller's stream; optimized_trajectory() and pose_graph_info() return the result.  trajectory(), relative() and
      refined_trajectory() stay what they are, bit for bit, and run() does not change.  Feeding the corrected poses
      back is rebuild_map() / adopt_loop_closure() (below), both opt-in.  The loop measurements are the caller's, or
      the runner's own with verify= (next).  None (the default): close_loops raises.
    * Loop verification: keyframes=KeyframeStore(...) (rslo_amd/loops.py, csrc/loopverify.hip) with verify=dict(...)
      (the options of loops.check_verify -- stages, max_distance, inlier_dist, min_overlap, max_rms, min_pairs, damping
      -- plus edge_w=(1.0, 1.0) and max_edges=256; needs places) turns the candidates into measured loop edges on the
      device: behind places.describe / query and before places.add, run() calls keyframes.prepare(the submitted
      tensor), verifies row n of loop_candidates() into row n of loop_checks() ([n, top_k, 16]: status, entry, pairs,
      overlap, rms, query count, Z, distance, heading, 0) in ONE launch, emits the best accepted row into the edge list
      loop_edges() = (ij, Z, w, counters) and then keyframes.add().  A fixed number of launches, no synchronisation,
      nothing allocated.  close_verified_loops(**options) is close_loops on that edge list (its unused rows hold
      i = j = -1, which the pose graph skips), with no host read.  The capacities of places and keyframes must reach
      the runner's capacity (an entry's index is its scan's index), and max_edges must not exceed
      pose_graph.max_loops.  keyframes= without verify= only stores the frames.  reset() empties the store and the
      edge list.  Unknown keys are an error at construction.  verify=None (the default): today's bits.
    * The map after loop closure (needs keyframes=): rebuild_map(voxel_map=None, poses=None) resets the given VoxelMap
      or MapPyramid (default: the runner's own) and fills it with every stored keyframe under its own row of poses
      (default: optimized_trajectory()) in ONE call per level (VoxelMap.insert_frames, rslo_map_insert_frames: three
      launches whatever the number of scans), on the caller's stream, with no host read.  The rebuilt map has the
      density of the KEYFRAMES, not of the scans: voxel_size centroids of the store, at most K per scan, about one hit
      per cell per frame.  A caller who refines with min_hits > 1, or wants a 0.2 m map, builds the store with
      voxel_size=0.2, K=4096.  adopt_loop_closure() (refining runners, after close_loops() / close_verified_loops() of
      everything streamed so far) takes the correction into the refined chain: the optimised rows replace rows
      0 .. n-1 of refined_trajectory() (a later close_loops() would otherwise read the correction as one huge odometry
      edge between n-1 and n), the chain's state becomes optimised row n-1, so that the next scan's prediction composes
      onto the corrected pose, and rebuild_map() makes the runner's own map consistent before that scan is registered
      against it: n_scans is n again, so the next insert is scan n and local_map's grace keeps its meaning.
      trajectory(), relative(), the head graph, the place database, the keyframe store and the edge list are untouched.
      Evicting keyframes is out of scope.  Neither method is called by run(): without them, today's bits.
    * Surfel map: surfels=SurfelMap(...) (rslo_amd/surfels.py, csrc/surfel.hip) receives every scan beside the voxel map
      (or alone): run() inserts the tensor passed to submit() under the row the voxel map uses -- the refined chain
      when there is one, else the open-loop chain.  surfel_refine=dict(iters=4, max_dist=None, robust_scale=0.2,
      damping=1e-6, min_pairs=50, tol_t=0.0, tol_r=0.0) (these defaults; needs surfels) adds a registration stage
      against the surfel map's planes (SurfelMap.register: no scan normal is read, so raw scans get a plane metric): it
      creates the refined chain when refine= is absent, and corrects row n of it in place behind refine's own stage
      (if any); then the chain state is set and both maps are filled.  Scan 0 meets an empty table (status 1) and
      stays the identity.  With cost="distribution" among the options (then also min_flag=1, reg_rel=0.01, reg_abs=0.02,
      and robust_scale defaults to 3.0 sigmas) the stage is the point-to-distribution cost over every fitted cell
      (SurfelMap.register(cost="distribution")), which also refines where the map holds no planes; nothing else in the
      runner changes.  surfel_refine_info() is the [n, iters, 8] info.  reset() empties the surfel map;
      rebuild_map() on the runner's own maps and adopt_loop_closure() also reset it and refill it from the keyframe
      store under the same poses (SurfelMap.insert_frames).  The table only fills unless local_map= carries the
      surfels key (above): then it is pruned about the sensor every K scans and a long drive runs in a fixed table.
      trajectory() and relative() are untouched.  None (the default): the launches of before.
    * De-skewing: deskew=dict(motion="network", times="azimuth", stamp=0.5, az_start_turn=-0.5, az_clockwise=False,
      max_angle=pi/2) (these defaults; rslo_amd/deskew.py, csrc/deskew.hip) motion-compensates every sweep before the
      back end sees it: behind the head replay (or the eager head) and before the second chain, run() de-skews the
      tensor passed to submit() into a runner-owned [point_capacity, F] buffer -- the normals are rotated when F >= 7,
      the caller's tensor is not written, the encoder's arena cloud is not read -- and both register stages, both map
      inserts, places.describe and keyframes.prepare read that buffer instead of the submitted tensor.  One launch per
      scan, no synchronisation, nothing allocated (the buffer is made by the first submit(), which fixes F).  The
      motion of the sweep: motion="network" uses rel[n], and none for n == 0 (the pair is the scan with itself);
      motion="refined" (needs refine= or surfel_refine=, whose chain starts at the identity) uses
      between(refined[n-2], refined[n-1]), the constant-velocity model on the corrected chain, and none for n < 2.
      Whether a motion is given is decided by the host's own scan count.  times="azimuth" dates a return by its
      azimuth (a sweep from az_start_turn, in turns, counter-clockwise unless az_clockwise); times="input" takes
      submit(cloud, times) / feed(scans, times): one contiguous fp32 CUDA [P] tensor of sweep fractions per scan.
      deskew_info() is the [n, 8] motion blocks {axis, angle, t', status} on the device, deskewed() the view of the
      last scan.  The ENCODER's input is deliberately not de-skewed: its job is planned one scan ahead on the helper
      thread, before any motion for that scan exists.  trajectory() and relative() stay bit for bit.  Unknown keys
      are errors at construction.  None (the default): every launch and every bit of before.
    * Free-space carving: carve=dict(every=1, rows=64, cols=1024, tan_lo=tan(-25 deg), tan_hi=tan(3 deg), win_rows=1,
      win_cols=1, margin_abs=0.3, margin_rel=0.0, max_range=60.0, grace=1) (these defaults; rslo_amd/carve.py,
      csrc/carve.hip; needs voxel_map) removes what moves: when (n + 1) % every == 0, behind the registration of scan n
      and in FRONT of its insert, run() builds the range image of the scan the back end reads (the de-skewed buffer
      with deskew=) and calls voxel_map.carve(image, row n of the chain that feeds the insert) -- a VoxelMap, or every
      level of a MapPyramid (VoxelMap.carve; include/rslo_hip.h "Free-space carving").  Two launches for the image and
      five per map level, no synchronisation, nothing allocated (the image and the rebuild's workspace are made here).  The surfel map
      is not carved.  trajectory() and relative() are untouched.  Unknown keys are errors at construction.  None (the
      default): every launch and every bit of before.
    `rel` and `pose` are rows of the runner's device buffers [capacity, 7]; they stay valid until reset()."""

    def __init__(self, net, max_voxels=None, device="cuda", capacity=8192, arenas=4, point_capacity=160000,
                 normals="input", normal_radius=0.6, normal_max_nn=30, voxel_map=None, refine=None, local_map=None,
                 places=None, loop=None, pose_graph=None, keyframes=None, verify=None, surfels=None, surfel_refine=None,
                 deskew=None, carve=None):
        from rslo_amd import synthetic
        if carve is not None:
            from rslo_amd import carve as carve_mod
            if voxel_map is None:
                raise capi.RsloHipError("OdometryRunner: carve needs a voxel_map to carve")
            try:
                carve = carve_mod.check_carve(carve)
            except ValueError as e:
                raise capi.RsloHipError("OdometryRunner: %s" % e)
        if normals not in ("input", "estimate"):
            raise capi.RsloHipError("OdometryRunner: normals must be \"input\" or \"estimate\", got %r" % (normals,))
        if refine is not None and voxel_map is not None:      # (before anything is built: a refused option leaves nothing behind)
            from rslo_amd import mapping
            try:
                refine, info_rows = mapping.check_refine(refine, voxel_map)
            except ValueError as e:
                raise capi.RsloHipError("OdometryRunner: %s" % e)
        if surfel_refine is not None:
            from rslo_amd import surfels as surfels_mod
            if surfels is None:
                raise capi.RsloHipError("OdometryRunner: surfel_refine needs surfels=SurfelMap(...) to register against")
            try:
                surfel_refine = surfels_mod.check_surfel_refine(surfel_refine, surfels)
            except ValueError as e:
                raise capi.RsloHipError("OdometryRunner: %s" % e)
        if deskew is not None:
            from rslo_amd import deskew as deskew_mod
            try:
                deskew = deskew_mod.check_deskew(deskew)
            except ValueError as e:
                raise capi.RsloHipError("OdometryRunner: %s" % e)
            if deskew["motion"] == "refined" and refine is None and surfel_refine is None:
                raise capi.RsloHipError("OdometryRunner: deskew motion=\"refined\" needs refine= or surfel_refine= (the "
                                        "chain it reads)")
        if loop is not None and places is None:
            raise capi.RsloHipError("OdometryRunner: loop needs places=PlaceDB(...) to search")
        if places is not None:
            from rslo_amd import places as places_mod
            loop = dict(loop or {})
            unknown = set(loop) - {"exclude_recent", "num_candidates", "top_k"}
            if unknown:
                raise capi.RsloHipError("OdometryRunner: loop takes exclude_recent, num_candidates and top_k; got %s"
                                        % sorted(unknown))
            try:
                ex, nc, tk = places_mod.check_query(loop.get("exclude_recent", 50), loop.get("num_candidates", 10),
                                                    loop.get("top_k", 1))
            except ValueError as e:
                raise capi.RsloHipError("OdometryRunner: %s" % e)
            loop = dict(exclude_recent=ex, num_candidates=nc, top_k=tk)
        edge_opts = None
        if verify is not None:
            from rslo_amd import loops as loops_mod
            if places is None or keyframes is None:
                raise capi.RsloHipError("OdometryRunner: verify needs places=PlaceDB(...) and keyframes=KeyframeStore(...)")
            verify = dict(verify)
            edge_w, max_edges = verify.pop("edge_w", (1.0, 1.0)), verify.pop("max_edges", 256)
            try:
                verify = loops_mod.check_verify(verify)
                edge_opts = loops_mod.check_edges(max_edges, edge_w)
            except ValueError as e:
                raise capi.RsloHipError("OdometryRunner: %s" % e)
            if pose_graph is not None and edge_opts[0] > pose_graph.max_loops:
                raise capi.RsloHipError("OdometryRunner: verify max_edges = %d exceeds pose_graph.max_loops = %d"
                                        % (edge_opts[0], pose_graph.max_loops))
        for name, owner in (("places", places if verify is not None else None), ("keyframes", keyframes)):
            if owner is not None and owner.capacity < int(capacity):
                raise capi.RsloHipError("OdometryRunner: the %s capacity %d is below the runner's capacity %d (an entry's "
                                        "index must equal its scan's index)" % (name, owner.capacity, int(capacity)))
        self.normals = normals
        self.normal_radius, self.normal_max_nn = float(normal_radius), int(normal_max_nn)
        if normals == "estimate" and not (3 <= self.normal_max_nn <= 32 and self.normal_radius > 0):
            raise capi.RsloHipError("OdometryRunner: normal_max_nn must be in 3..32 and normal_radius positive")
        self.net = net
        self.head = net.odom_predictor
        if net.training or self.head.training:
            raise capi.RsloHipError("OdometryRunner is an inference path: put the network in eval() mode")
        why = self.head.eval_fused_unsupported()
        if why is not None:
            raise capi.RsloHipError("OdometryRunner: unsupported configuration: " + why)
        p = next(self.head.parameters())
        if not p.is_cuda:
            raise capi.RsloHipError("OdometryRunner: the network must live on the GPU")
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        from rslo.layers import hip_conv2d
        self.operands = hip_conv2d.EvalOperands(self.head)
        self.encoder = EncoderGraphRunner(net, synthetic.MAX_VOXELS if max_voxels is None else max_voxels, self.device,
                                          point_capacity=point_capacity, arenas=arenas, with_cov=False,
                                          pre_plan=self._append_normals if normals == "estimate" else None)
        self.capacity = int(capacity)
        dev = self.device
        self._raw = []             # normals="estimate": per arena (cloud [cap,7], normals [cap,3], counts [cap], workspace)
        if normals == "estimate":
            cap = int(point_capacity)
            wsb = capi.lib().rslo_normals_ws_bytes(cap)
            for _ in range(self.encoder.planner.n_arenas):
                self._raw.append((torch.zeros((cap, 7), dtype=torch.float32, device=dev),
                                  torch.zeros((cap, 3), dtype=torch.float32, device=dev),
                                  torch.zeros((cap,), dtype=torch.int32, device=dev),
                                  torch.empty((wsb,), dtype=torch.uint8, device=dev)))
        self._state = torch.zeros((7,), dtype=torch.float64, device=dev)
        self._count = torch.zeros((1,), dtype=torch.int32, device=dev)
        self._rel = torch.zeros((self.capacity, 7), dtype=torch.float32, device=dev)
        self._traj = torch.zeros((self.capacity, 7), dtype=torch.float64, device=dev)
        self._pair = None          # [1, 2C, H, W] static input of the head graph
        self._graph = None
        self._n = 0                # scans of the current sequence (host mirror of the device counter)
        self.voxel_map = voxel_map
        if voxel_map is not None:
            if voxel_map.device != dev:
                raise capi.RsloHipError("OdometryRunner: the voxel map lives on %s, the runner on %s" % (voxel_map.device, dev))
            voxel_map.reserve(int(point_capacity))      # run() must not allocate
        self.surfels, self.surfel_refine = surfels, surfel_refine
        if surfels is not None:
            if surfels.device != dev:
                raise capi.RsloHipError("OdometryRunner: the surfel map lives on %s, the runner on %s" % (surfels.device, dev))
            surfels.reserve(int(point_capacity))        # run() must not allocate
        self.refine = None
        if refine is not None and voxel_map is None:
            raise capi.RsloHipError("OdometryRunner: refine needs a voxel_map to register against")
        self._refined = refine is not None or surfel_refine is not None      # the second chain exists
        if self._refined:
            self._state2 = torch.zeros((7,), dtype=torch.float64, device=dev)
            self._count2 = torch.zeros((1,), dtype=torch.int32, device=dev)
            self._rel2 = torch.zeros((self.capacity, 7), dtype=torch.float32, device=dev)
            self._traj2 = torch.zeros((self.capacity, 7), dtype=torch.float64, device=dev)
        if refine is not None:
            self.refine = refine
            self._info2 = torch.zeros((self.capacity, info_rows, 8), dtype=torch.float64, device=dev)
        if surfel_refine is not None:
            self._info3 = torch.zeros((self.capacity, surfel_refine["iters"], 8), dtype=torch.float64, device=dev)
        self.local_map = None
        if local_map is not None:
            local_map = dict(local_map)
            surfel_prune = local_map.pop("surfels", None)
            if surfel_prune is None or surfel_prune is False:
                surfel_prune = None
                if voxel_map is None:
                    raise capi.RsloHipError("OdometryRunner: local_map needs a voxel_map to prune")
            else:
                if surfels is None:
                    raise capi.RsloHipError("OdometryRunner: local_map's surfels key needs surfels=SurfelMap(...) to prune")
                surfel_prune = {} if surfel_prune is True else dict(surfel_prune)
                unknown = set(surfel_prune) - {"min_count", "inner_radius"}
                if unknown:
                    raise capi.RsloHipError("OdometryRunner: local_map surfels takes min_count and inner_radius; got %s"
                                            % sorted(unknown))
            unknown = set(local_map) - {"radius", "every", "min_hits", "grace"}
            if unknown:
                raise capi.RsloHipError("OdometryRunner: local_map takes radius, every, min_hits, grace and surfels; got %s"
                                        % sorted(unknown))
            if "radius" not in local_map:
                raise capi.RsloHipError("OdometryRunner: local_map needs a radius")
            every = local_map.get("every", 1)
            if int(every) != every or every < 1:
                raise capi.RsloHipError("OdometryRunner: local_map every must be an integer >= 1, got %r" % (every,))
            from rslo_amd import mapping
            radius = mapping.check_prune(None, local_map["radius"], local_map.get("min_hits", 1), local_map.get("grace", 0),
                                         has_center=True)
            local_map = dict(radius=radius, every=int(every), min_hits=int(local_map.get("min_hits", 1)),
                             grace=int(local_map.get("grace", 0)))
            if surfel_prune is not None:
                from rslo_amd import surfels as surfels_mod
                _, inner, min_count = surfels_mod.check_surfel_prune(None, radius, surfel_prune.get("inner_radius"),
                                                                     surfel_prune.get("min_count", 1), has_center=True)
                local_map["surfels"] = dict(min_count=min_count, inner_radius=inner)
                surfels.reserve_prune()                 # run() must not allocate
            self.local_map = local_map
            if voxel_map is not None:
                voxel_map.reserve_prune()               # run() must not allocate
        self.carve = carve
        self._range_image = None
        if carve is not None:
            from rslo_amd import carve as carve_mod
            self._range_image = carve_mod.RangeImage(carve["rows"], carve["cols"], carve["tan_lo"], carve["tan_hi"], dev)
            self._carve_kw = {k: carve[k] for k in ("win_rows", "win_cols", "margin_abs", "margin_rel", "max_range", "grace")}
            voxel_map.reserve_prune()                   # the rebuild shares prune's workspace: run() must not allocate
        self.places, self.loop = places, loop
        if places is not None:
            if places.device != dev:
                raise capi.RsloHipError("OdometryRunner: the place database lives on %s, the runner on %s" % (places.device, dev))
            places.reserve(int(point_capacity))         # run() must not allocate
            self._loop = torch.zeros((self.capacity, loop["top_k"], 4), dtype=torch.float64, device=dev)
        self.keyframes, self.verify = keyframes, verify
        self._verifier = self._edges = None
        if keyframes is not None:
            if keyframes.device != dev:
                raise capi.RsloHipError("OdometryRunner: the keyframe store lives on %s, the runner on %s" % (keyframes.device, dev))
            keyframes.reserve(int(point_capacity))      # run() must not allocate
        if verify is not None:
            from rslo_amd import loops as loops_mod
            self._verifier = loops_mod.LoopVerifier(keyframes, **verify)
            self._edges = loops_mod.EdgeList(edge_opts[0], edge_opts[1], device=dev)
            self._checks = torch.zeros((self.capacity, loop["top_k"], loops_mod.OUT_COLS), dtype=torch.float64, device=dev)
        self.deskew = deskew
        self._deskewer = self._deskewed = None      # the stage is built by the first submit(), which fixes F
        if deskew is not None:
            self._dk_info = torch.zeros((self.capacity, 8), dtype=torch.float64, device=dev)
        self.pose_graph = pose_graph
        self._optimized = self._pg_info = None
        if pose_graph is not None and pose_graph.device != dev:
            raise capi.RsloHipError("OdometryRunner: the pose graph lives on %s, the runner on %s" % (pose_graph.device, dev))
        self.stats = {"scans": 0, "encoder_runs": 0, "head_replays": 0, "head_eager": 0, "captures": 0,
                      "weight_refreshes": 0}

    def submit(self, cloud, times=None):
        raw = torch.is_tensor(cloud) and cloud.dim() == 2 and cloud.shape[1] in (3, 4)
        if self.normals == "input" and raw:
            raise capi.RsloHipError("OdometryRunner.submit: a [P, %d] scan has no normals; this runner takes [P, 7] clouds -- "
                                    "build it with normals=\"estimate\" to feed raw scans" % cloud.shape[1])
        if self.normals == "estimate":
            if not (raw and cloud.is_cuda and cloud.dtype == torch.float32 and cloud.is_contiguous()):
                raise capi.RsloHipError("OdometryRunner.submit: normals=\"estimate\" takes contiguous fp32 CUDA [P, 4] (or "
                                        "[P, 3]) scans, got %s" % (tuple(cloud.shape) if torch.is_tensor(cloud) else type(cloud),))
            if cloud.shape[0] > self.encoder.point_capacity:
                raise capi.RsloHipError("OdometryRunner.submit: the scan exceeds point_capacity = %d"
                                        % self.encoder.point_capacity)
        keep = (self.voxel_map is not None or self.places is not None or self.keyframes is not None
                or self.surfels is not None or self.deskew is not None)
        if keep and not (torch.is_tensor(cloud) and cloud.is_cuda and cloud.dtype == torch.float32 and cloud.dim() == 2):
            raise capi.RsloHipError("OdometryRunner.submit: a runner with a voxel map%s takes one fp32 CUDA [P, F] tensor"
                                    % ("" if self.places is None else " or a place database"))
        if times is not None and (self.deskew is None or self.deskew["times"] != "input"):
            raise capi.RsloHipError("OdometryRunner.submit: a times tensor needs deskew=dict(times=\"input\")")
        if self.deskew is not None:
            P, F = cloud.shape
            if self.deskew["times"] == "input" and not (torch.is_tensor(times) and times.is_cuda and times.shape == (P,)
                                                        and times.dtype == torch.float32 and times.is_contiguous()):
                raise capi.RsloHipError("OdometryRunner.submit: deskew times=\"input\" takes a contiguous fp32 CUDA [P] "
                                        "tensor of sweep fractions with every scan")
            if P > self.encoder.point_capacity:
                raise capi.RsloHipError("OdometryRunner.submit: the scan exceeds point_capacity = %d"
                                        % self.encoder.point_capacity)
            if self._deskewer is None:
                from rslo_amd import deskew as deskew_mod
                self._deskewer = deskew_mod.Deskewer(self.encoder.point_capacity, F, self.device, **self.deskew)
            elif self._deskewer.n_cols != F:
                raise capi.RsloHipError("OdometryRunner.submit: the de-skewing buffer holds [P, %d] scans, got [P, %d]"
                                        % (self._deskewer.n_cols, F))
        h = self.encoder.submit(cloud)
        h.source = cloud if keep else None
        h.times = times
        return h

    def feed(self, scans, times=None):
        """Drive the runner over the sequence `scans` in order: scan i + 1 is submitted before scan i is run, so the
        helper thread plans the next scan while the device works on this one.  times: one sweep-fraction tensor per scan
        (deskew=dict(times="input")), else None.  Nothing is read back and nothing is
        returned (trajectory(), relative() ... hold the results); never more than two handles are outstanding."""
        if len(scans) == 0:
            return
        if times is not None and len(times) != len(scans):
            raise capi.RsloHipError("OdometryRunner.feed: %d scans and %d times tensors" % (len(scans), len(times)))
        submit = (lambda i: self.submit(scans[i])) if times is None else (lambda i: self.submit(scans[i], times[i]))
        h = submit(0)
        for i in range(1, len(scans)):
            ahead = submit(i)
            self.run(h)
            h = ahead
        self.run(h)

    def _append_normals(self, scan, arena, k):
        """pre-plan hook (helper thread, plan stream): raw scan -> the arena's [P, 7] cloud"""
        cloud, nrm, cnt, ws = self._raw[arena]
        return capi.append_normals(scan, self.normal_radius, self.normal_max_nn, None, out=cloud, counts=cnt, ws=ws,
                                   normals=nrm)

    def close(self):
        self.encoder.close()

    def reset(self):
        """A new sequence: the next scan is paired with itself and seeds a new trajectory."""
        self._count.zero_()
        self._n = 0
        self._deskewed = None
        if self.voxel_map is not None:
            self.voxel_map.reset()
        if self.surfels is not None:
            self.surfels.reset()
        if self._refined:
            self._count2.zero_()
        if self.places is not None:
            self.places.reset()
        if self.keyframes is not None:
            self.keyframes.reset()
        if self._edges is not None:
            self._edges.reset()
        self._optimized = self._pg_info = None

    def close_loops(self, loops_ij, loops_Z, loops_w=None, **options):
        """Optimise a copy of the streamed trajectory (the refined chain when the runner refines) under the loop edges
        (loops_ij int32 [L, 2] scan indices, loops_Z float64 [L, 7] the pose of j in the frame of i, loops_w [L, 2] or
        None for ones; options: PoseGraph.optimize's).  Returns (poses, info), also kept for optimized_trajectory() and
        pose_graph_info().  Nothing the runner streams is changed."""
        if self.pose_graph is None:
            raise capi.RsloHipError("OdometryRunner.close_loops: the runner was built without pose_graph")
        if "poses" in options:
            raise capi.RsloHipError("OdometryRunner.close_loops: the start is the runner's own trajectory")
        traj0 = self.refined_trajectory() if self._refined else self.trajectory()
        self._optimized, self._pg_info = self.pose_graph.optimize(traj0, loops_ij, loops_Z, loops_w, **options)
        return self._optimized, self._pg_info

    def close_verified_loops(self, **options):
        """close_loops() on the runner's own edge list (verify=...): the whole fixed-size list goes to the pose graph,
        which skips its unused rows; nothing is read on the host."""
        if self._edges is None:
            raise capi.RsloHipError("OdometryRunner.close_verified_loops: the runner was built without verify")
        return self.close_loops(self._edges.ij, self._edges.Z, self._edges.w, **options)

    def rebuild_map(self, voxel_map=None, poses=None):
        """Reset voxel_map (a VoxelMap or MapPyramid; default: the runner's own) and insert every stored keyframe under
        its own row of poses (float64 CUDA [m, 7]; default: optimized_trajectory()): the map the corrected trajectory
        implies, at the density of the keyframes.  On the caller's stream, no host read.  Returns the map.  With the
        runner's own map as the target (voxel_map=None) an attached SurfelMap is reset and refilled the same way; a
        runner with surfels= and no voxel_map rebuilds the surfel map alone (and returns None)."""
        if self.keyframes is None:
            raise capi.RsloHipError("OdometryRunner.rebuild_map: the runner was built without keyframes")
        vmap = self.voxel_map if voxel_map is None else voxel_map
        own_surfels = self.surfels if voxel_map is None else None      # the runner's own maps are rebuilt together
        if vmap is None and own_surfels is None:
            raise capi.RsloHipError("OdometryRunner.rebuild_map: no voxel_map given and the runner was built without one")
        if poses is None:
            if self._optimized is None:
                raise capi.RsloHipError("OdometryRunner.rebuild_map: no poses given and close_loops() has not run")
            poses = self._optimized
        if vmap is not None:
            vmap.reset()
            vmap.insert_frames(self.keyframes, poses)
        if own_surfels is not None:
            own_surfels.reset()
            own_surfels.insert_frames(self.keyframes, poses)
        return vmap

    def adopt_loop_closure(self):
        """Take the last close_loops() into the refined chain (class docstring): its rows, its state, and the runner's
        own map rebuilt from the keyframes.  The open-loop chain and everything else the runner streams stay."""
        if not self._refined or self.keyframes is None:
            raise capi.RsloHipError("OdometryRunner.adopt_loop_closure: needs a runner built with refine= and keyframes=")
        if self._optimized is None:
            raise capi.RsloHipError("OdometryRunner.adopt_loop_closure: close_loops() has not run")
        n = int(self._optimized.shape[0])
        if n != self._n:
            raise capi.RsloHipError("OdometryRunner.adopt_loop_closure: close_loops() optimised %d scans, %d have been "
                                    "streamed; close the loops again first" % (n, self._n))
        self._traj2[:n].copy_(self._optimized)
        self._state2.copy_(self._optimized[n - 1])
        self.rebuild_map()

    def loop_checks(self):
        """[n, top_k, 16] fp64 device rows (verify=...): LoopVerifier.verify's result of every scan's candidates."""
        if self._verifier is None:
            raise capi.RsloHipError("OdometryRunner.loop_checks: the runner was built without verify")
        return self._checks[:min(self._n, self.capacity)]

    def loop_edges(self):
        """(ij int32 [E, 2], Z fp64 [E, 7], w fp64 [E, 2], counters int64 [2] = {n_edges, dropped_full}) on the device
        (verify=...): the edges emitted so far; unused rows hold i = j = -1."""
        if self._edges is None:
            raise capi.RsloHipError("OdometryRunner.loop_edges: the runner was built without verify")
        return self._edges.tensors()

    def optimized_trajectory(self):
        """[n, 7] fp64 device rows: the result of the last close_loops()."""
        if self._optimized is None:
            raise capi.RsloHipError("OdometryRunner.optimized_trajectory: close_loops() has not run "
                                    "(or the runner was built without pose_graph)")
        return self._optimized

    def pose_graph_info(self):
        """[gn_iters, 8] fp64 device rows: PoseGraph.optimize's info of the last close_loops()."""
        if self._pg_info is None:
            raise capi.RsloHipError("OdometryRunner.pose_graph_info: close_loops() has not run "
                                    "(or the runner was built without pose_graph)")
        return self._pg_info

    def loop_candidates(self):
        """[n, top_k, 4] fp64 device rows (places=...): PlaceDB.query's result of every scan against the scans before it."""
        if self.places is None:
            raise capi.RsloHipError("OdometryRunner.loop_candidates: the runner was built without places")
        return self._loop[:min(self._n, self.capacity)]

    def refined_trajectory(self):
        """[n, 7] fp64 device rows of the refined chain (refine=...): row i = register(refined[i-1] o rel[i])."""
        if not self._refined:
            raise capi.RsloHipError("OdometryRunner.refined_trajectory: the runner was built without refine")
        return self._traj2[:min(self._n, self.capacity)]

    def surfel_refine_info(self):
        """[n, iters, 8] fp64 device rows (surfel_refine=...): SurfelMap.register's info of every scan."""
        if self.surfel_refine is None:
            raise capi.RsloHipError("OdometryRunner.surfel_refine_info: the runner was built without surfel_refine")
        return self._info3[:min(self._n, self.capacity)]

    def deskew_info(self):
        """[n, 8] fp64 device rows (deskew=...): the motion block {axis, angle, t', status} every scan was de-skewed with."""
        if self.deskew is None:
            raise capi.RsloHipError("OdometryRunner.deskew_info: the runner was built without deskew")
        return self._dk_info[:min(self._n, self.capacity)]

    def deskewed(self):
        """The [P, F] fp32 view of the runner's buffer that holds the last scan de-skewed (deskew=...); the next run()
        overwrites it."""
        if self.deskew is None:
            raise capi.RsloHipError("OdometryRunner.deskewed: the runner was built without deskew")
        if self._deskewed is None:
            raise capi.RsloHipError("OdometryRunner.deskewed: no scan has been run since reset()")
        return self._deskewed

    def refine_info(self):
        """[n, iters, 8] fp64 device rows: VoxelMap.register's info of every scan."""
        if self.refine is None:
            raise capi.RsloHipError("OdometryRunner.refine_info: the runner was built without refine")
        return self._info2[:min(self._n, self.capacity)]

    def trajectory(self):
        return self._traj[:min(self._n, self.capacity)]

    def relative(self):
        return self._rel[:min(self._n, self.capacity)]

    def refresh_weights(self, force=False):
        """Re-derive the head's split operands and folded BatchNorms if a parameter / running statistic changed (or
        always, force=True); a storage that moved invalidates the captured head graph."""
        if force:           # the tensors are collected again: a parameter object may have been replaced
            from rslo.layers import hip_conv2d
            self.operands = hip_conv2d.EvalOperands(self.head)
        n0 = self.operands.refreshes
        if self.operands.refresh():
            self._graph = None
        self.stats["weight_refreshes"] += self.operands.refreshes - n0

    def _head(self):
        self.head.__dict__["_eval_fused"] = True
        try:
            with torch.no_grad():
                out = self.head(self._pair)
        finally:
            self.head.__dict__.pop("_eval_fused", None)
        return out["translation_preds"][0], out["rotation_preds"][0]

    def _head_and_chain(self):
        t, r = self._head()
        capi.pose_chain(t[0], r[0], self._state, self._count, self._rel, self._traj)

    def run(self, handle, graph=True):
        """Encoder pass of the submitted scan, pair map, head + pose chain (a replay of the head graph, or with
        graph=False the same kernels issued eagerly).  Returns (rel [7] fp32, pose [7] fp64) device rows."""
        if self._n >= self.capacity:
            raise capi.RsloHipError("OdometryRunner: more than %d scans in one sequence (capacity); reset() or a larger "
                                    "capacity" % self.capacity)
        bev, _, _ = self.encoder.run(handle, graph=graph)
        self.stats["encoder_runs"] += 1
        C = bev.shape[1]
        if self._pair is None or self._pair.shape[1] != 2 * C or self._pair.shape[2:] != bev.shape[2:]:
            self._pair = torch.empty((1, 2 * C) + tuple(bev.shape[2:]), dtype=torch.float32, device=self.device)
            self._graph = None
        prev, cur = self._pair[:, :C], self._pair[:, C:]
        if self._n == 0:
            prev.copy_(bev[:1])
        else:
            prev.copy_(cur)
        cur.copy_(bev[:1])
        self.refresh_weights()
        if graph:
            if self._graph is None:
                self._capture()
            self._graph.replay()
            self.stats["head_replays"] += 1
        else:
            self._head_and_chain()
            self.stats["head_eager"] += 1
        n = self._n
        source = handle.source              # what the back end reads: the submitted tensor, or its de-skewed copy
        if self.deskew is not None:         # behind the head (rel[n] is written), before the second chain: one launch
            if self.deskew["motion"] == "network":
                motion = dict(rel7=self._rel[n]) if n >= 1 else {}
            else:                           # constant velocity on the corrected chain, whose rows below n are final
                motion = dict(pose_a=self._traj2[n - 2], pose_b=self._traj2[n - 1]) if n >= 2 else {}
            source = self._deskewed = self._deskewer(handle.source, handle.times, motion_out=self._dk_info[n], **motion)
        chain = self._traj2 if self._refined else self._traj      # the chain whose row n places this scan in the maps
        if self._refined:                   # the second chain: predict from the refined pose, register, compose onto the result
            rel = self._rel[n]
            capi.pose_chain(rel[:3], rel[3:], self._state2, self._count2, self._rel2, self._traj2)
            if self.refine is not None:
                self.voxel_map.register(source, self._traj2[n], info=self._info2[n], **self.refine)
            if self.surfel_refine is not None:      # behind refine's own stage, on the same row
                self.surfels.register(source, self._traj2[n], info=self._info3[n], **self.surfel_refine)
            self._state2.copy_(self._traj2[n])
        if self.carve is not None and (n + 1) % self.carve["every"] == 0:      # behind the registration, in front of the insert
            self.voxel_map.carve(self._range_image(source), chain[n], **self._carve_kw)
        if self.voxel_map is not None:      # behind the pose chain (and the registration) that wrote row n, on this stream
            self.voxel_map.insert(source, chain[n])
        if self.surfels is not None:
            self.surfels.insert(source, chain[n])
        if self.local_map is not None and (n + 1) % self.local_map["every"] == 0:
            lm = self.local_map
            if self.voxel_map is not None:
                self.voxel_map.prune(chain[n], lm["radius"], lm["min_hits"], lm["grace"])
            if "surfels" in lm:                 # the same row and the same radius
                self.surfels.prune(chain[n], lm["radius"], lm["surfels"]["inner_radius"], lm["surfels"]["min_count"])
        if self.places is not None:         # describe -> query -> add: the scan is searched for before it is stored
            self.places.describe(source)
            self.places.query(out=self._loop[n], **self.loop)
            if self.keyframes is not None:  # prepare -> verify -> emit -> add: an edge's j is the store's count before add
                self.keyframes.prepare(source)
                if self._verifier is not None:
                    self._verifier.verify(self._loop[n], out=self._checks[n])
                    self._edges.emit(self._checks[n], self.keyframes)
                self.keyframes.add()
            self.places.add()
        elif self.keyframes is not None:
            self.keyframes.prepare(source)
            self.keyframes.add()
        self._n += 1
        self.stats["scans"] += 1
        return self._rel[n], self._traj[n]

    def _capture(self):
        """Warm up (the kernels' first launches, the allocator's blocks) with the head alone -- the pose chain must not
        advance -- then capture head + pose chain over the static pair map."""
        self._head()
        torch.cuda.current_stream(self.device).synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._head_and_chain()
        self._graph = g
        self.stats["captures"] += 1
