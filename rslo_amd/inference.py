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
    * Back end: everything behind the head replay -- de-skewing, the refined chain and both registration stages, free-space
      carving, the voxel map and the surfel map with their pruning, place recognition, the keyframe store and loop
      verification -- and everything on what has been streamed -- the pose graph, the map rebuild, adopting a loop
      closure -- is rslo_amd.backend.BackEnd, built from the keyword arguments voxel_map, refine, local_map, places,
      loop, pose_graph, keyframes, verify, surfels, surfel_refine, deskew and carve: its class docstring describes every
      one of them.  run() calls backend.step(the tensor passed to submit(), its times) on the caller's stream behind
      the head and pose chain of that scan; refined_trajectory(), refine_info(), surfel_refine_info(), deskew_info(),
      deskewed(), loop_candidates(), loop_checks(), loop_edges(), close_loops(), close_verified_loops(),
      rebuild_map(), adopt_loop_closure(), optimized_trajectory() and pose_graph_info(), and the attributes of the
      keyword arguments' names, are the back end's.  The options are checked (backend.check) before anything is
      built: a refused option leaves nothing behind.  The encoder job's cloud is NOT what the back end reads: with
      normals="estimate" it is an arena buffer the helper thread may overwrite as soon as the event recorded by
      EncoderGraphRunner.run has passed, and the ENCODER's input is deliberately not de-skewed: its job is planned one
      scan ahead on the helper thread, before any motion for that scan exists.  The caller keeps the submitted tensor
      unmodified until run() of its handle has been consumed on the device.  trajectory() and relative() are the
      open-loop chain, bit for bit, whatever the back end does; reset() also resets the back end.  With every one of
      those arguments None (the default) run() issues nothing behind the pose chain.
    `rel` and `pose` are rows of the runner's device buffers [capacity, 7]; they stay valid until reset()."""

    def __init__(self, net, max_voxels=None, device="cuda", capacity=8192, arenas=4, point_capacity=160000,
                 normals="input", normal_radius=0.6, normal_max_nn=30, voxel_map=None, refine=None, local_map=None,
                 places=None, loop=None, pose_graph=None, keyframes=None, verify=None, surfels=None, surfel_refine=None,
                 deskew=None, carve=None):
        from rslo_amd import backend, synthetic
        back_end = dict(voxel_map=voxel_map, refine=refine, local_map=local_map, places=places, loop=loop,
                        pose_graph=pose_graph, keyframes=keyframes, verify=verify, surfels=surfels,
                        surfel_refine=surfel_refine, deskew=deskew, carve=carve)
        try:                    # before anything is built: a refused option leaves nothing behind
            backend.check(capacity, device, **back_end)
        except ValueError as e:
            raise capi.RsloHipError("OdometryRunner: %s" % e)
        if normals not in ("input", "estimate"):
            raise capi.RsloHipError("OdometryRunner: normals must be \"input\" or \"estimate\", got %r" % (normals,))
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
        self.chain = backend.PoseChain(self.capacity, dev)      # the open-loop chain: pushed inside the head graph
        self._pair = None          # [1, 2C, H, W] static input of the head graph
        self._graph = None
        self.backend = backend.BackEnd(self.chain, capacity=self.capacity, point_capacity=point_capacity, device=dev,
                                       **back_end)
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
        try:
            self.backend.check_scan(cloud, times)
        except ValueError as e:
            raise capi.RsloHipError("OdometryRunner.submit: %s" % e)
        h = self.encoder.submit(cloud)
        h.source = cloud if self.backend.reads_scans else None
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
        """A new sequence: the next scan is paired with itself and seeds a new trajectory; the back end starts anew."""
        self.chain.reset()
        self.backend.reset()

    def trajectory(self):
        return self.chain.rows(self.backend.n)[1]

    def relative(self):
        return self.chain.rows(self.backend.n)[0]

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
        self.chain.push(t[0], r[0])

    def run(self, handle, graph=True):
        """Encoder pass of the submitted scan, pair map, head + pose chain (a replay of the head graph, or with
        graph=False the same kernels issued eagerly).  Returns (rel [7] fp32, pose [7] fp64) device rows."""
        n = self.backend.n                  # scans of the current sequence
        if n >= self.capacity:
            raise capi.RsloHipError("OdometryRunner: more than %d scans in one sequence (capacity); reset() or a larger "
                                    "capacity" % self.capacity)
        bev, _, _ = self.encoder.run(handle, graph=graph)
        self.stats["encoder_runs"] += 1
        C = bev.shape[1]
        if self._pair is None or self._pair.shape[1] != 2 * C or self._pair.shape[2:] != bev.shape[2:]:
            self._pair = torch.empty((1, 2 * C) + tuple(bev.shape[2:]), dtype=torch.float32, device=self.device)
            self._graph = None
        prev, cur = self._pair[:, :C], self._pair[:, C:]
        if n == 0:
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
        self.backend.step(handle.source, handle.times)      # behind the head and the pose chain, which wrote rel[n]
        self.stats["scans"] += 1
        return self.chain.rel[n], self.chain.traj[n]

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


def _of_back_end(name):
    return property(lambda self: getattr(self.backend, name), lambda self, value: setattr(self.backend, name, value))


# what the back end owns under the runner's public names: its methods, and the attributes of its keyword arguments
for _name in ("refined_trajectory", "refine_info", "surfel_refine_info", "deskew_info", "deskewed", "loop_candidates",
              "loop_checks", "loop_edges", "close_loops", "close_verified_loops", "rebuild_map", "adopt_loop_closure",
              "optimized_trajectory", "pose_graph_info", "voxel_map", "surfels", "refine", "surfel_refine", "local_map", "carve",
              "deskew", "places", "loop", "keyframes", "verify", "pose_graph"):
    setattr(OdometryRunner, _name, _of_back_end(_name))
