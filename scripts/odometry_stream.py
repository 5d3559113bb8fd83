"""Streaming odometry in eval mode: the eager reference loop against rslo_amd.inference.OdometryRunner.

    python scripts/odometry_stream.py --scans 200 --warmup 20 --seed 0 [--out profiles/odometry_stream_eager_vs_runner.json]
    python scripts/odometry_stream.py --save-scans /tmp/drive.npz --scans 60 --warmup 5
    python scripts/odometry_stream.py --runner-only --load-scans /tmp/drive.npz --scans 20 --warmup 5   # under rocprofv3
    python scripts/odometry_stream.py --launches A_kernel_stats.csv B_kernel_stats.csv --scans-a 20 --scans-b 60
    python scripts/odometry_stream.py --raw --scans 200 --warmup 20 [--out profiles/odometry_stream_raw.json]
    python scripts/odometry_stream.py --map --scans 200 --warmup 20 [--map-out map.ply] [--out profiles/odometry_stream_map.json]
    python scripts/odometry_stream.py --refine --scans 200 --warmup 20 [--refine-iters 3] [--out profiles/odometry_stream_refine.json]
    python scripts/odometry_stream.py --refine --refine-levels 0.8 0.4 0.2 --refine-iters-per-level 4 [--refine-robust 0.5] [--out profiles/odometry_stream_pyramid.json]
    python scripts/odometry_stream.py --map --local-map-radius 100 --local-map-every 10 --scans 200 --warmup 20 [--out profiles/odometry_stream_local_map.json]
    python scripts/odometry_stream.py --places --scans 200 --warmup 20 [--out profiles/odometry_stream_places.json]
    python scripts/odometry_stream.py --pose-graph --scans 200 --warmup 20 [--out profiles/odometry_stream_posegraph.json]
    python scripts/odometry_stream.py --verify --scans 200 --warmup 20 [--out profiles/odometry_stream_verify.json]
    python scripts/odometry_stream.py --rebuild-map --scans 200 --warmup 20 [--out profiles/odometry_stream_rebuild.json]
    python scripts/odometry_stream.py --surfels --scans 200 --warmup 20 [--surfel-voxel 0.4] [--surfel-iters 4] [--out profiles/odometry_stream_surfels.json]
    python scripts/odometry_stream.py --surfels --surfel-cost distribution --scans 200 --warmup 20 [--surfel-reg-abs 0.02]
    python scripts/odometry_stream.py --surfels --local-map-radius 50 --surfel-min-count 2 --surfel-inner-radius 25 --scans 180 --warmup 20
    python scripts/odometry_stream.py --deskew --scans 100 --warmup 10 [--out profiles/odometry_stream_deskew.json]

A synthetic drive (rslo_amd.synthetic.sequence_scan: C2-shaped 64-beam scans, consecutive scans overlapping) is fed
scan by scan to
  (a) the eager loop of evaluate.py:363-408: the example of scan i is built from frames (max(i-1, 0), i) the way the
      dataset builds it (kitti_dataset_hdf5.py:184-185, workload.make_example) and `net(example)` runs under no_grad;
  (b) the runner: OdometryRunner.feed (submit one scan ahead, run), no host read.
Both are timed with device events over --scans scans after --warmup scans; one JSON line is printed.
--raw: a third loop feeds the same scans stripped to [P, 4] (what a LiDAR produces) to a runner built with
normals="estimate" (csrc/normals.hip on the plan stream) and reports its ms per scan, the distance of its trajectory
from the [P, 7] run and the median angle between the estimated and the drive's analytic normals (a report, not a
test: the analytic normals are exact only away from edges).
--map: one more runner loop with a world voxel map attached (rslo_amd.mapping.VoxelMap, csrc/map.hip: every run() inserts
its scan under its absolute pose): ms per scan with the map beside the plain runner's, the inserts alone (the same scans
under the same trajectory rows into a second map, device events over the timed scans), the map's counters, the mean
overlap of each scan with the map before its insertion, and --map-out FILE.ply.  The same figures under the drive's own
poses (synthetic.sequence_pose; --seed must be the drive's): with random weights the runner's trajectory is not a drive.
--refine (implies --map): one more runner loop with refine=dict(iters=--refine-iters) (csrc/mapreg.hip: every scan is
registered against the map before it is inserted), timed beside the --map loop of the same run, and a "registration
alone" pass on the drive: the prediction of scan i is refined[i-1] o (true relative motion o a fixed seeded error of
about 5 cm and 0.1 degrees); pose error against synthetic.sequence_pose before and after VoxelMap.register, pairs per
scan and ms per register call from device events (--seed must be the drive's).
--refine-levels V0 V1 .. (coarse to fine; implies --refine) [--refine-iters-per-level N] [--refine-robust F]: one more
runner loop with voxel_map=MapPyramid(levels) and its default schedule (N iterations per level, scale = F * voxel below
the coarsest level; F omitted: the library's default), ms per scan beside the --refine loop of the same process; the
inserts alone into the pyramid beside those into the one map; and the registration-alone pass once per setting -- the
parent's (VoxelMap.register, --refine-iters), the same with robust weights, and the schedule with factors 0, 0.5 and 1
-- with the same seeded disturbance: ms per call and pose error before / after for each.
--local-map-radius R [--local-map-every K] (implies --map): the --map loop, the --refine loop when given, and the
inserts alone under the drive's own poses once more with the rolling local map (VoxelMap.prune about the scan's pose
every K scans; rslo_map_prune in csrc/map.hip), each beside the same loop without pruning in this process: ms per scan,
prune_stats, the largest n_cells seen, dropped_full, ms per prune call from device events (and of a call that evicts
nothing), and the insert time over the last 200 scans.
--places: one more runner loop with a place database attached (rslo_amd.places.PlaceDB, csrc/places.hip: every run()
describes its scan, searches the scans before it and adds it), ms per scan beside the plain runner loop of this process;
describe, query (10 ring-key candidates, and exhaustive) and add alone under device events against the database of the
whole drive; and a revisit pass: the drive's scans go into the database, then queries are made with synthetic.scan at
earlier drive positions moved 0.7 m / 0.8 m with the heading reversed -- top-1 within 5 m, the distances of the true
matches, and the smallest distance to any entry more than 10 m away (--seed must be the drive's).
--pose-graph: the runner is built with a pose graph (rslo_amd.posegraph.PoseGraph, csrc/posegraph.hip); after its loop,
loop measurements between scan 0 and eight later scans are made from the SYNTHETIC GROUND TRUTH (synthetic.sequence_pose
-- the library cannot verify a loop candidate yet, so nothing here comes from place recognition), close_loops optimises
and the translation RMSE against the ground truth is reported before and after -- for the runner's own trajectory, and
for the drive's true relative motions disturbed by a seeded 2 cm / 0.1 degree error per scan and chained (the network
of this script is untrained: its own trajectory is noise, and Gauss-Newton has no step control).  Then a size sweep on
PoseGraphRef.synthetic_graph, N in {256, 1024, 4096, 8192} x L in {1, 16, 256}: per case the device-event time of
optimize (6 Gauss-Newton iterations), of one iteration, of the edge launch with the sums (PoseGraph.cost; what is left
of an iteration is the one-workgroup solve plus the update launch), and the CG iterations per Gauss-Newton iteration.
--rebuild-map (implies --verify): a runner with keyframes, verification, a voxel map and a pose graph streams every scan
and closes its verified loops; then the map is rebuilt from the keyframe store under the optimised trajectory (a) in one
call (VoxelMap.insert_frames, rslo_map_insert_frames in csrc/map.hip) and (b) as one VoxelMap.insert per frame on views
of the store's rows, the counts read back once outside the timed window -- the per-scan kernels, the baseline.  Each into
a reset map, device events, one warm-up of both and then the two alternated five times: median, min and max.  The same at
a second size: a store of 4096 entries (the streamed frames re-added) under two laps of a circle, a metre per frame.  Per
size: frames, points, cells, dropped_full, the times, and whether the two maps are bit-equal.
--surfels --local-map-radius R [--local-map-every K --surfel-min-count M --surfel-inner-radius r]: also the surfel map
filled under the drive's own poses unpruned and pruned (SurfelMap.prune about the scan's pose every K scans;
rslo_surfel_prune in csrc/surfel.hip): n_cells, n_planar, dropped_full and the prune counters side by side, and the
device-event time of the prune call at capacity 2^20 beside VoxelMap.prune's (surfel_local_map_report).
--deskew: scan de-skewing (rslo_amd.deskew, csrc/deskew.hip).  The drive's scans are rigid snapshots; their SKEWED twin
is what a sensor that moves during the sweep records: deskew.skew_ref under the drive's true motion
between(sequence_pose(i-1), sequence_pose(i)), the time of a return being the sweep fraction of the azimuth at which it
is recorded, stamp 0.5.  The twin is de-skewed on the device (Deskewer, the motion given as that pose pair), and the
registration-alone pass against a surfel map runs on three lists -- the original scans, the skewed ones, the de-skewed
ones: pose error before / after for each (the network of this script is untrained, so accuracy is measured as the other
reports measure it), with the distance of the skewed and of the de-skewed points from the original ones.  The kernel
alone under device events, and the runner with and without deskew= in this one process, plain and with the surfel stage
(--seed must be the drive's).
--carve [--carve-scans 40]: free-space carving (rslo_amd.carve, csrc/carve.hip), a report of its own that needs no network
and returns before the loops above: a drive of --carve-scans scans of the synthetic world in which a vehicle-sized box
(synthetic.scan(extra_boxes=...)) drives 12..20 m ahead of the sensor for the first half and is then gone.  The map is
filled under the drive's true poses without and with VoxelMap.carve in front of every insert (the defaults of
carve.CARVE_DEFAULTS): the cells inside the swept volume of the box at the end, with and without, and the share of all
OTHER cells that carving removed.  Then, on the uncarved table at --map-capacity: the device-event time of RangeImage, of
VoxelMap.carve and of VoxelMap.prune (60 m about the last pose), carve and prune alternated on a table restored from a
snapshot before every call, median / min / max of 11; and the same two as calls that evict nothing.
--launches: launches per scan of the runner from the kernel statistics of two rocprofv3 runs of different lengths
(their difference: warm-up, capture and set-up cancel), and the kernels per scan that are not hand-written ones."""
import argparse
import csv
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _scan(args):
    from rslo_amd import synthetic
    i, seed = args
    return synthetic.sequence_scan(i, seed=seed)


def make_scans(n, seed, workers):
    """The scans of the drive, ray-cast on `workers` processes (about a second of numpy per scan)."""
    if workers <= 1:
        return [_scan((i, seed)) for i in range(n)]
    import multiprocessing as mp
    with mp.get_context("spawn").Pool(workers) as pool:
        return pool.map(_scan, [(i, seed) for i in range(n)])


CARVE_BOX = (4.2, 1.8, 1.5)      # a vehicle: length, width, height in metres


def _carve_box(i, n, seed):
    """(cx, cy, sx, sy, sz) of the vehicle in front of scan i of the --carve drive, or None once it is gone: 12 m ahead of
    the sensor at scan 0, 20 m at the last scan of the first half (axis-aligned: the drive's heading stays within degrees)"""
    import math
    from rslo_amd import synthetic
    half = n // 2
    if i >= half:
        return None
    p = synthetic.sequence_pose(i, seed)
    yaw = 2.0 * math.atan2(p[6], p[3])
    d = 12.0 + 8.0 * i / max(1, half - 1)
    return (p[0] + d * math.cos(yaw), p[1] + d * math.sin(yaw)) + CARVE_BOX


def _carve_scan(a):
    import math
    from rslo_amd import synthetic
    i, n, seed = a
    p = synthetic.sequence_pose(i, seed)
    box = _carve_box(i, n, seed)
    return synthetic.scan(pose_xy=(p[0], p[1]), yaw=2.0 * math.atan2(p[6], p[3]), scan_seed=7 * seed + 3 * i + 1,
                          extra_boxes=None if box is None else [box])


def carve_report(args):
    """--carve (module docstring)"""
    import numpy as np
    import torch
    import rslo_amd  # noqa: F401
    from rslo_amd import carve, mapping, synthetic
    n, seed = args.carve_scans, args.seed
    t0 = time.time()
    jobs = [(i, n, seed) for i in range(n)]
    if args.workers <= 1:
        clouds = [_carve_scan(j) for j in jobs]
    else:
        import multiprocessing as mp
        with mp.get_context("spawn").Pool(args.workers) as pool:
            clouds = pool.map(_carve_scan, jobs)
    out = {"metric": "odometry_stream_carve", "scans": n, "seed": seed, "scan_generation_s": round(time.time() - t0, 1),
           "points_per_scan": int(sum(len(c) for c in clouds) / n), "box": list(CARVE_BOX), "map_voxel": args.map_voxel,
           "map_capacity": args.map_capacity,
           "carve": {k: (round(v, 6) if isinstance(v, float) else v) for k, v in carve.CARVE_DEFAULTS.items()}}
    dev = torch.device("cuda", 0)
    scans = [torch.from_numpy(c).to(dev) for c in clouds]
    true = [torch.from_numpy(synthetic.sequence_pose(i, seed)).to(dev) for i in range(n)]
    boxes = [b for b in (_carve_box(i, n, seed) for i in range(n)) if b is not None]
    opts = {k: carve.CARVE_DEFAULTS[k] for k in ("win_rows", "win_cols", "margin_abs", "margin_rel", "max_range", "grace")}
    ri = carve.RangeImage(device=dev)

    def fill(carving):
        vmap = mapping.VoxelMap(args.map_voxel, args.map_capacity, dev, min_range=2.5, max_range=80.0)
        vmap.reserve(max(s.shape[0] for s in scans))
        vmap.reserve_prune()
        for s, p in zip(scans, true):
            if carving:
                vmap.carve(ri(s), p, **opts)
            vmap.insert(s, p)
        return vmap

    def in_swept_volume(rows):
        """the cells a box ever covered, above the road surface (the ground under the box is static)"""
        inside = np.zeros((len(rows),), bool)
        for cx, cy, sx, sy, sz in boxes:
            inside |= ((np.abs(rows[:, 0] - cx) <= sx / 2 + 0.1) & (np.abs(rows[:, 1] - cy) <= sy / 2 + 0.1)
                       & (rows[:, 2] > -synthetic.SENSOR_H + 0.25) & (rows[:, 2] <= -synthetic.SENSOR_H + sz + 0.1))
        return inside

    plain, carved = fill(False), fill(True)
    rows_p, rows_c = plain.points()[0].cpu().numpy(), carved.points()[0].cpu().numpy()
    tp, tc = in_swept_volume(rows_p), in_swept_volume(rows_c)
    out["cells_plain"], out["cells_carved"] = len(rows_p), len(rows_c)
    out["swept_cells_plain"], out["swept_cells_carved"] = int(tp.sum()), int(tc.sum())
    out["other_cells_plain"], out["other_cells_carved"] = int((~tp).sum()), int((~tc).sum())
    out["other_cells_removed_share"] = round(1.0 - float((~tc).sum()) / float((~tp).sum()), 5)
    out["carve_stats"], out["carved_map_stats"], out["plain_map_stats"] = carved.carve_stats(), carved.stats(), plain.stats()
    out["carved_map_n_lost"] = carved.prune_stats()["n_lost"]

    # the calls alone, on the uncarved table: restored from a snapshot in front of every timed call
    snapshot = plain._buf.clone()
    last, reps = n - 1, 11

    def timed(fn, restore=True):
        if restore:
            plain._buf.copy_(snapshot)
        return device_ms(lambda _: fn(), 1)

    def spread(ms):
        ms = sorted(ms)
        return {"median": round(ms[len(ms) // 2], 4), "min": round(ms[0], 4), "max": round(ms[-1], 4)}

    do_image = lambda: ri(scans[last])
    do_carve = lambda: plain.carve(ri, true[last], **dict(opts, grace=0))      # grace 0: the whole table is eligible
    do_prune = lambda: plain.prune(true[last], 60.0)
    for fn in (do_image, do_carve, do_prune):      # first launches
        timed(fn)
    image_ms, carve_ms, prune_ms = [], [], []
    for _ in range(reps):
        image_ms.append(timed(do_image, restore=False))
        carve_ms.append(timed(do_carve))
        prune_ms.append(timed(do_prune))
    plain._buf.copy_(snapshot)
    before = plain.stats()["n_cells"]
    do_carve()
    out["timed_carve_evicts"] = before - plain.stats()["n_cells"]
    plain._buf.copy_(snapshot)
    do_prune()
    out["timed_prune_evicts"] = before - plain.stats()["n_cells"]
    out["timed_table_cells"], out["timed_table_load"] = before, round(before / float(args.map_capacity), 4)
    out["range_image_ms"], out["carve_ms"], out["prune_ms"] = spread(image_ms), spread(carve_ms), spread(prune_ms)
    out["carve_over_prune"] = round(out["carve_ms"]["median"] / out["prune_ms"]["median"], 3)
    # calls that evict nothing, on the table the carve above left (a second carve from the same pose finds nothing new)
    plain._buf.copy_(snapshot)
    do_carve()
    noop_carve, noop_prune = [], []
    for _ in range(reps):
        noop_carve.append(timed(do_carve, restore=False))
        noop_prune.append(timed(lambda: plain.prune(true[last], float("inf")), restore=False))
    out["carve_no_evict_ms"], out["prune_no_evict_ms"] = spread(noop_carve), spread(noop_prune)
    # the contended image: every point in one pixel, beside a scan's spread of the same size
    P = scans[last].shape[0]
    one = torch.zeros((P, 3), dtype=torch.float32, device=dev)
    one[:, 0] = torch.linspace(30.0, 5.0, P, device=dev)
    ri(one)
    out["range_image_one_pixel_ms"] = spread([device_ms(lambda _: ri(one), 1) for _ in range(reps)])
    return out


def _kernel_counts(path):
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            out[row["Name"]] = out.get(row["Name"], 0) + int(row["Calls"])
    return out


def _hand_written_names():
    """The text of rslo_amd/csrc: a kernel is hand-written when its name is defined there."""
    import glob
    return "\n".join(open(f).read() for f in glob.glob(os.path.join(ROOT, "rslo_amd", "csrc", "*.hip")))


def _is_hand_written(name, src):
    base = re.split(r"[<(]", name[5:] if name.startswith("void ") else name, 1)[0].strip()
    return bool(re.match(r"^\w+$", base)) and re.search(r"\b%s\b" % base, src) is not None


def launches(a_csv, b_csv, n_a, n_b):
    a, b = _kernel_counts(a_csv), _kernel_counts(b_csv)
    per = {k: (b.get(k, 0) - a.get(k, 0)) / float(n_b - n_a) for k in set(a) | set(b)}
    per = {k: v for k, v in per.items() if abs(v) > 1e-9}
    names = _hand_written_names()
    foreign = {k: v for k, v in per.items() if not _is_hand_written(k, names)}
    return {"launches_per_scan": round(sum(per.values()), 2),
            "hand_written_per_scan": round(sum(v for k, v in per.items() if _is_hand_written(k, names)), 2),
            "hand_written_kernels_per_scan": {k[:120]: round(v, 2) for k, v in sorted(per.items(), key=lambda kv: -kv[1])
                                              if _is_hand_written(k, names)},
            "other_per_scan": {k[:160]: round(v, 2) for k, v in sorted(foreign.items(), key=lambda kv: -kv[1])},
            "miopen_kernels": sorted(k[:160] for k in per if "miopen" in k.lower() or "MIOpen" in k),
            "scans_a": n_a, "scans_b": n_b}


def device_ms(fn, n):
    """ms per call of fn(0) .. fn(n - 1): two device events around the n calls, behind a synchronise"""
    import torch
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def timed_feed(runner, scans, W, N):
    """(device ms, host ms) per scan of runner.feed over scans W .. W + N - 1, behind the W scans in front of them"""
    import torch
    runner.feed(scans[:W])
    torch.cuda.synchronize()
    h0 = time.perf_counter()
    ms = device_ms(lambda _: runner.feed(scans[W:W + N]), 1)
    return ms / N, (time.perf_counter() - h0) * 1e3 / N


class EagerLoop:
    """(a) of the module docstring behind the face timed_feed drives: feed(scans) runs net(example) scan by scan"""

    def __init__(self, net):
        self.net, self.prev = net, None

    def feed(self, scans):
        import torch
        from rslo_amd import workload
        with torch.no_grad():
            for s in scans:
                out = self.net(workload.make_example(self.net, [[s if self.prev is None else self.prev, s]]))
                out["translation_preds"], out["rotation_preds"]
                self.prev = s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--workers", type=int, default=14)
    ap.add_argument("--runner-only", action="store_true")
    ap.add_argument("--raw", action="store_true", help="also run the runner with normals=\"estimate\" on [P, 4] scans")
    ap.add_argument("--map", action="store_true", help="also run the runner with a world voxel map attached")
    ap.add_argument("--map-voxel", type=float, default=0.2)
    ap.add_argument("--map-capacity", type=int, default=1 << 22, help="slots of the map's table (a power of two)")
    ap.add_argument("--map-out", default=None, help="write the map as a binary PLY")
    ap.add_argument("--refine", action="store_true", help="also run the runner with scan-to-map refinement (implies --map)")
    ap.add_argument("--refine-iters", type=int, default=3, help="Gauss-Newton iterations per scan")
    ap.add_argument("--refine-levels", type=float, nargs="+", default=None,
                    help="voxel sizes of a map pyramid, coarse to fine: also run the coarse-to-fine loops (implies --refine)")
    ap.add_argument("--refine-iters-per-level", type=int, default=4)
    ap.add_argument("--refine-robust", type=float, default=None, help="robust factor of the default schedule")
    ap.add_argument("--local-map-radius", type=float, default=None,
                    help="also run the map loops with a rolling local map of this radius in metres (implies --map)")
    ap.add_argument("--local-map-every", type=int, default=10, help="prune every K scans")
    ap.add_argument("--places", action="store_true", help="also run the runner with a place-recognition database attached")
    ap.add_argument("--places-queries", type=int, default=20, help="revisit queries of the --places report")
    ap.add_argument("--verify", action="store_true",
                    help="also run the runner with a keyframe store and loop verification (implies --places)")
    ap.add_argument("--verify-k", type=int, default=2048, help="points per keyframe of the --verify store")
    ap.add_argument("--pose-graph", action="store_true", help="close loops over the runner's trajectory and time the optimiser")
    ap.add_argument("--rebuild-map", action="store_true",
                    help="rebuild the map from the keyframe store after loop closure: one call against one insert per frame "
                         "(implies --verify)")
    ap.add_argument("--surfels", action="store_true",
                    help="also run the runner with a surfel map and its registration stage, and the registration-alone rows")
    ap.add_argument("--surfel-voxel", type=float, default=0.4)
    ap.add_argument("--surfel-iters", type=int, default=4, help="Gauss-Newton iterations of the surfel stage")
    ap.add_argument("--surfel-cost", choices=("plane", "distribution"), default="plane",
                    help="with --surfels: distribution runs the registration-alone rows of BOTH costs in one process and "
                         "nothing else, and writes profiles/odometry_stream_surfels_dist.json unless --out is given")
    ap.add_argument("--surfel-reg-abs", type=float, default=0.02,
                    help="with --surfel-cost distribution: the absolute regularisation of a cell's covariance in metres")
    ap.add_argument("--surfel-min-count", type=int, default=1,
                    help="with --surfels --local-map-radius: evict surfel cells with fewer points beyond the inner radius")
    ap.add_argument("--surfel-inner-radius", type=float, default=None,
                    help="with --surfels --local-map-radius: cells nearer than this are exempt from --surfel-min-count "
                         "(default: the radius)")
    ap.add_argument("--deskew", action="store_true",
                    help="also de-skew a skewed twin of the drive and run the runner with deskew=")
    ap.add_argument("--carve", action="store_true",
                    help="the free-space carving report alone: a box drives ahead of the sensor and is then gone")
    ap.add_argument("--carve-scans", type=int, default=40, help="scans of the --carve drive")
    ap.add_argument("--out", default=None)
    ap.add_argument("--launches", nargs=2, default=None)
    ap.add_argument("--scans-a", type=int, default=20)
    ap.add_argument("--scans-b", type=int, default=60)
    ap.add_argument("--save-scans", default=None, help="write the drive's scans to this .npz and stop")
    ap.add_argument("--load-scans", default=None, help="read the scans from a --save-scans file (profiled runs)")
    args = ap.parse_args()
    args.refine = args.refine or args.refine_levels is not None
    args.map = args.map or args.refine or args.local_map_radius is not None
    args.verify = args.verify or args.rebuild_map
    args.places = args.places or args.verify
    if args.launches:
        res = launches(args.launches[0], args.launches[1], args.scans_a, args.scans_b)
        line = json.dumps(res)
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return
    if args.carve:
        line = json.dumps(carve_report(args))
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return

    t0 = time.time()
    n_scans = args.warmup + args.scans
    if args.load_scans:
        import numpy as np
        with np.load(args.load_scans) as z:
            clouds = [z["s%d" % i] for i in range(n_scans)]
    else:
        clouds = make_scans(n_scans, args.seed, args.workers)
    if args.save_scans:
        import numpy as np
        np.savez(args.save_scans, **{"s%d" % i: c for i, c in enumerate(clouds)})
        return
    t_scans = time.time() - t0
    import torch
    import rslo_amd  # noqa: F401
    if args.surfels and args.surfel_cost == "distribution":
        scans = [torch.from_numpy(c).to(torch.device("cuda", 0)) for c in clouds]
        res = {"metric": "surfel_alone_ms_per_iteration", "scans": args.scans, "warmup": args.warmup, "seed": args.seed,
               "points_per_scan": int(sum(c.shape[0] for c in clouds) / len(clouds)), "scan_generation_s": round(t_scans, 1)}
        res.update(surfel_dist_report(args, scans))
        line = json.dumps(res)
        print(line)
        with open(args.out or os.path.join(ROOT, "profiles", "odometry_stream_surfels_dist.json"), "w") as f:
            f.write(line + "\n")
        return
    from rslo_amd import inference, workload
    torch.manual_seed(args.seed)
    net, _ = workload.build_network()
    net.eval()
    dev = torch.device("cuda", 0)
    scans = [torch.from_numpy(c).to(dev) for c in clouds]
    if not args.runner_only:       # (a profiled run keeps the eager pass -- and its library kernels -- out of the trace)
        workload.calibrate_head_bn(net, (scans[0], scans[1]))      # eval statistics: poses of a sane magnitude
    W, N = args.warmup, args.scans
    res = {"metric": "odometry_stream_ms_per_scan", "scans": N, "warmup": W, "seed": args.seed,
           "points_per_scan": int(sum(c.shape[0] for c in clouds) / len(clouds)), "scan_generation_s": round(t_scans, 1)}

    if not args.runner_only:
        res["eager_ms_per_scan"], res["eager_host_ms_per_scan"] = [round(v, 3) for v in timed_feed(EagerLoop(net), scans, W, N)]

    graph = None
    if args.pose_graph:
        from rslo_amd import posegraph
        graph = posegraph.PoseGraph(capacity=8192, max_loops=256, device=dev)
    runner = inference.OdometryRunner(net, pose_graph=graph)
    res["runner_ms_per_scan"], res["runner_host_ms_per_scan"] = [round(v, 3) for v in timed_feed(runner, scans, W, N)]
    # the pair map: the two device copies per scan, measured on their own
    C = runner._pair.shape[1] // 2
    bev = torch.empty_like(runner._pair[:, C:])

    def copies(_):
        runner._pair[:, :C].copy_(runner._pair[:, C:])
        runner._pair[:, C:].copy_(bev)
    res["pair_map_copies_ms_per_scan"] = round(device_ms(copies, 100), 4)
    res["pair_map_bytes_per_scan"] = int(2 * 2 * bev.numel() * 4)
    res["runner_stats"] = dict(runner.stats)
    res["encoder_runs_per_scan"] = round(runner.encoder.stats["runs"] / max(1, runner.stats["scans"]), 3)
    if "eager_ms_per_scan" in res:
        res["speedup"] = round(res["eager_ms_per_scan"] / res["runner_ms_per_scan"], 2)
    # the two paths on the same drive: the last scan's relative pose
    if not args.runner_only:
        i = W + N - 1
        with torch.no_grad():
            out = net(workload.make_example(net, [[scans[i - 1], scans[i]]]))
        ref = torch.cat([out["translation_preds"][0], out["rotation_preds"][0]])
        res["last_rel_max_rel_diff"] = float((runner.relative()[-1] - ref).abs().max() / ref.abs().max())
    traj_input, rel_input = runner.trajectory().clone(), runner.relative().clone()
    if args.pose_graph:
        res.update(pose_graph_report(args, runner))
    runner.close()
    if args.raw:
        res.update(raw_report(args, net, scans, res, traj_input, rel_input))
    if args.map:
        res.update(map_report(args, net, scans, res, traj_input))
    if args.refine:
        res.update(refine_report(args, net, scans, res))
    if args.refine_levels is not None:
        res.update(pyramid_report(args, net, scans, res))
    if args.local_map_radius is not None:
        res.update(local_map_report(args, net, scans, res))
    if args.places:
        res.update(places_report(args, net, scans, res))
    if args.verify:
        res.update(verify_report(args, net, scans, res))
    if args.rebuild_map:
        res.update(rebuild_report(args, net, scans, res))
    if args.surfels:
        res.update(surfel_report(args, net, scans, res))
        if args.local_map_radius is not None:
            res.update(surfel_local_map_report(args, scans))
    if args.deskew:
        res.update(deskew_report(args, net, scans, res))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


def raw_report(args, net, scans, res, traj_input, rel_input):
    """--raw: the runner fed [P, 4] scans beside the plain runner's figures, and the normals of one scan on their own"""
    import torch
    from rslo_amd import capi, inference
    W, N = args.warmup, args.scans
    out = {}
    raw_scans = [s[:, :4].contiguous() for s in scans]
    raw = inference.OdometryRunner(net, normals="estimate")
    out["raw_ms_per_scan"], out["raw_host_ms_per_scan"] = [round(v, 3) for v in timed_feed(raw, raw_scans, W, N)]
    out["raw_minus_input_ms_per_scan"] = round(out["raw_ms_per_scan"] - res["runner_ms_per_scan"], 3)
    d = (raw.trajectory() - traj_input)[:, :3].norm(dim=1)
    path = (traj_input[1:, :3] - traj_input[:-1, :3]).norm(dim=1).sum()
    out["raw_traj_max_dist_m"], out["raw_traj_end_dist_m"] = float(d.max()), float(d[-1])
    out["input_traj_path_m"] = float(path)
    dr = (raw.relative() - rel_input).abs().max(dim=1).values / rel_input.abs().max(dim=1).values
    out["raw_rel_diff_median"], out["raw_rel_diff_max"] = float(dr.median()), float(dr.max())
    raw.close()
    # normals of one scan on their own: time of the six launches, agreement with the analytic normals
    s0 = scans[W]
    est, cnt = capi.estimate_normals(raw_scans[W], zero_vertical=True)
    out["normals_alone_ms_per_scan"] = round(device_ms(lambda _: capi.estimate_normals(raw_scans[W], zero_vertical=True), 20), 4)
    both = (s0[:, 4:7].norm(dim=1) > 0) & (est.norm(dim=1) > 0)
    cosang = (s0[:, 4:7] * est)[both].sum(1).abs().clamp(max=1.0)
    out["normals_median_angle_deg"] = float(torch.rad2deg(torch.acos(cosang)).median())
    out["normals_compared_points"] = int(both.sum())
    out["normals_points_with_fewer_than_3_neighbours"] = int((cnt < 3).sum())
    return out


def map_report(args, net, scans, res, traj_input):
    """--map: the runner with a world voxel map beside the plain runner's figures, and the inserts alone"""
    import torch
    from rslo_amd import inference, mapping, synthetic
    dev = scans[0].device
    W, N = args.warmup, args.scans
    out = {}
    vmap = mapping.VoxelMap(args.map_voxel, args.map_capacity, dev)
    mapped = inference.OdometryRunner(net, voxel_map=vmap)
    out["map_ms_per_scan"], out["map_host_ms_per_scan"] = [round(v, 3) for v in timed_feed(mapped, scans, W, N)]
    out["map_minus_runner_ms_per_scan"] = round(out["map_ms_per_scan"] - res["runner_ms_per_scan"], 3)
    traj = mapped.trajectory().clone()
    out["map_traj_equals_runner"] = bool(torch.equal(traj.view(torch.int64), traj_input.view(torch.int64)))      # bits: a NaN equals itself
    out["map_stats"] = vmap.stats()
    out["map_voxel"], out["map_capacity"] = args.map_voxel, args.map_capacity
    out["map_load"] = round(out["map_stats"]["n_cells"] / float(args.map_capacity), 4)
    mapped.close()
    # the inserts alone: the same scans into a second map, under the runner's trajectory rows and under the drive's own
    # poses (synthetic.sequence_pose: the registered cloud a trained network would approach)
    alone = mapping.VoxelMap(args.map_voxel, args.map_capacity, dev)
    alone.reserve(max(s.shape[0] for s in scans))

    def insert_pass(poses):
        """(ms per timed insert, counters, mean overlap of a scan with the map before its insertion)"""
        alone.reset()
        for i in range(W):
            alone.insert(scans[i], poses[i])
        ms = device_ms(lambda i: alone.insert(scans[W + i], poses[W + i]), N)
        stats = alone.stats()
        alone.reset()
        ov = torch.zeros((), dtype=torch.float32, device=dev)      # one host read at the end
        for i in range(W + N):
            if i > 0:
                ov += alone.overlap(scans[i], poses[i])
            alone.insert(scans[i], poses[i])
        return round(ms, 4), stats, round(float(ov) / (W + N - 1), 4)

    out["map_insert_alone_ms_per_scan"], stats, out["map_mean_overlap_before_insert"] = insert_pass(traj)
    out["map_insert_alone_stats_equal"] = stats == out["map_stats"]
    # (--load-scans: the file must hold the drive of --seed)
    true = [torch.from_numpy(synthetic.sequence_pose(i, args.seed)).to(dev) for i in range(W + N)]
    (out["map_true_pose_insert_ms_per_scan"], out["map_true_pose_stats"],
     out["map_true_pose_mean_overlap_before_insert"]) = insert_pass(true)
    out["map_true_pose_load"] = round(out["map_true_pose_stats"]["n_cells"] / float(args.map_capacity), 4)
    if args.map_out:
        vmap.save_ply(args.map_out)
        out["map_ply_bytes"] = os.path.getsize(args.map_out)
    return out


def pose_graph_report(args, runner):
    """--pose-graph: loops closed over the runner's trajectory, then the size sweep"""
    return {**posegraph_close(args, runner), **posegraph_sweep(runner.pose_graph)}


def posegraph_close(args, runner):
    """--pose-graph, first part: loops from the synthetic ground truth onto the runner's trajectory"""
    import numpy as np
    import torch
    from rslo_amd import posegraph, synthetic
    n = runner.trajectory().shape[0]
    truth = np.stack([synthetic.sequence_pose(i, args.seed) for i in range(n)])
    j = np.unique(np.linspace(n // 8, n - 1, 8).astype(np.int64))
    j = j[j > 0]
    ij = np.stack([np.zeros_like(j), j], 1).astype(np.int32)
    Z = posegraph.between(truth[ij[:, 0]], truth[ij[:, 1]])
    dev = runner.trajectory().device
    w = torch.full((len(j), 2), 10.0, dtype=torch.float64, device=dev)
    w[:, 1] = 100.0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    poses, info = runner.close_loops(torch.from_numpy(ij).to(dev), torch.from_numpy(Z).to(dev), w, chain_w=(1.0, 10.0),
                                     gn_iters=6, cg_iters=64, cg_tol=1e-8)
    e1.record()
    e1.synchronize()
    rmse = lambda P: float(np.sqrt(((P[:, :3] - truth[:, :3]) ** 2).sum(1).mean()))
    info = info.cpu().numpy()
    # the same loops on a trajectory with the drift of a working odometry: the drive's true relative motions disturbed by
    # a seeded error of 2 cm and 0.1 degrees per scan (the network here is untrained, its own trajectory is noise)
    rng = np.random.default_rng(args.seed)
    st, sr = 0.02, np.deg2rad(0.1)
    noise = np.concatenate([st * rng.standard_normal((n - 1, 3)), sr * rng.standard_normal((n - 1, 3))], 1)
    rel = posegraph.retract(posegraph.between(truth[:-1], truth[1:]), noise)
    drift = np.empty((n, 7))
    drift[0] = truth[0]
    for k in range(n - 1):
        drift[k + 1] = posegraph.compose(drift[k], rel[k])
        drift[k + 1, 3:] /= np.linalg.norm(drift[k + 1, 3:])
    wd = torch.tensor([[10.0, 10.0 * st / sr]] * len(j), dtype=torch.float64, device=dev)
    pd, infod = runner.pose_graph.optimize(torch.from_numpy(drift).to(dev), torch.from_numpy(ij).to(dev),
                                           torch.from_numpy(Z).to(dev), wd, chain_w=(1.0, st / sr), gn_iters=6, cg_iters=128,
                                           cg_tol=1e-8)
    infod = infod.cpu().numpy()
    extra = {"posegraph_drift_sigma": [st, 0.1], "posegraph_drift_translation_rmse_before_m": round(rmse(drift), 4),
             "posegraph_drift_translation_rmse_after_m": round(rmse(pd.cpu().numpy()), 4),
             "posegraph_drift_status": infod[:, 0].tolist(), "posegraph_drift_cg_iters": infod[:, 3].tolist(),
             "posegraph_drift_cost": [float("%.6g" % v) for v in infod[:, 2]]}
    return {**extra, "posegraph_loops_from": "synthetic ground truth (synthetic.sequence_pose); no candidate is verified by the library",
            "posegraph_loops_ij": ij.tolist(), "posegraph_nodes": int(n),
            "posegraph_translation_rmse_before_m": round(rmse(runner.trajectory().cpu().numpy()), 4),
            "posegraph_translation_rmse_after_m": round(rmse(poses.cpu().numpy()), 4),
            "posegraph_close_loops_ms": round(e0.elapsed_time(e1), 3),
            "posegraph_status": info[:, 0].tolist(), "posegraph_cg_iters": info[:, 3].tolist(),
            "posegraph_cost": [float("%.6g" % v) for v in info[:, 2]]}


def posegraph_sweep(graph):
    """--pose-graph, second part: optimize on synthetic graphs of growing size, under device events"""
    import torch
    from rslo_amd import posegraph
    dev = graph.device
    rows = []

    def events(fn, n):      # one call to warm up, then n timed
        fn()
        return device_ms(lambda _: fn(), n)

    for N in (256, 1024, 4096, 8192):
        for L in (1, 16, 256):
            g = posegraph.synthetic_graph(N, loops=L, seed=1)
            t = {k: torch.from_numpy(g[k]).to(dev) for k in ("traj0", "loops_ij", "loops_Z", "loops_w")}
            cw = tuple(g["chain_w"])
            poses, info = t["traj0"].clone(), torch.zeros((6, 8), dtype=torch.float64, device=dev)
            opt = dict(chain_w=cw, cg_iters=128, cg_tol=1e-8)

            def six():
                poses.copy_(t["traj0"])
                graph.optimize(t["traj0"], t["loops_ij"], t["loops_Z"], t["loops_w"], poses=poses, gn_iters=6, info=info, **opt)

            def one():
                poses.copy_(t["traj0"])
                graph.optimize(t["traj0"], t["loops_ij"], t["loops_Z"], t["loops_w"], poses=poses, gn_iters=1, info=info[:1], **opt)
            out4 = torch.zeros((4,), dtype=torch.float64, device=dev)
            ms6 = events(six, 3)
            inf = info.cpu().numpy().copy()
            ms1 = events(one, 3)
            ms_edges = events(lambda: graph.cost(t["traj0"], poses, t["loops_ij"], t["loops_Z"], t["loops_w"], chain_w=cw, out=out4), 10)
            rows.append({"N": N, "L": L, "optimize_6_iterations_ms": round(ms6, 3), "first_iteration_ms": round(ms1, 3),
                         "edges_and_sums_ms": round(ms_edges, 4), "solve_and_update_ms": round(ms1 - ms_edges, 3),
                         "cg_iters": inf[:, 3].tolist(), "status": inf[:, 0].tolist(),
                         "cost_first_last": [float("%.6g" % inf[0, 2]), float("%.6g" % inf[-1, 2])]})
    return {"posegraph_sweep": rows}


def _revisit_scan(a):
    from rslo_amd import synthetic
    x, y, yaw, seed = a
    return synthetic.scan(pose_xy=(x, y), yaw=yaw, scan_seed=seed)


def places_report(args, net, scans, res):
    """--places: the runner with a place database, the three calls alone, and the revisit pass"""
    import numpy as np
    import torch
    from rslo_amd import inference, places, synthetic
    W, N = args.warmup, args.scans
    dev = scans[0].device
    out = {}
    loop = dict(exclude_recent=50, num_candidates=10, top_k=1)
    db = places.PlaceDB(capacity=max(1024, W + N), device=dev)
    runner = inference.OdometryRunner(net, places=db, loop=loop)
    out["places_ms_per_scan"], out["places_host_ms_per_scan"] = [round(v, 3) for v in timed_feed(runner, scans, W, N)]
    out["places_minus_runner_ms_per_scan"] = round(out["places_ms_per_scan"] - res["runner_ms_per_scan"], 3)
    out["places_loop"] = loop
    out["places_stats"] = db.stats()
    cand = runner.loop_candidates().cpu().numpy()
    found = cand[:, 0, 0] >= 0
    out["places_runner_scans_with_a_candidate"] = int(found.sum())
    out["places_runner_smallest_distance"] = float(cand[found, 0, 1].min()) if found.any() else None      # a drive without a loop
    runner.close()

    # the three calls alone: the database holds the whole drive while it is queried
    descs = [tuple(t.clone() for t in db.describe(s)) for s in scans]
    db.reset()
    for d in descs:
        db.add(*d)
    row = torch.zeros((16, 4), dtype=torch.float64, device=dev)
    out["places_entries_when_queried"] = W + N
    out["places_describe_ms"] = round(device_ms(lambda i: db.describe(scans[W + i]), N), 4)
    for C in (10, 0):
        out["places_query_c%d_ms" % C] = round(device_ms(
            lambda i: db.query(*descs[W + i], exclude_recent=0, num_candidates=C, top_k=1, out=row[:1]), N), 4)
    side = places.PlaceDB(capacity=max(1024, W + N), device=dev)
    out["places_add_ms"] = round(device_ms(lambda i: side.add(*descs[W + i]), N), 4)

    # revisit: earlier drive positions, 0.7 m / 0.8 m off, heading reversed
    n_q = max(1, min(args.places_queries, W + N))
    idx = [int(v) for v in np.linspace(0, W + N - 1, n_q + 2)[1:-1]]
    poses = [synthetic._sequence_xy_yaw(i, args.seed) for i in range(W + N)]
    jobs = [(poses[i][0] + 0.7, poses[i][1] + 0.8, poses[i][2] + np.pi, 100000 + i) for i in idx]
    if args.workers <= 1:
        qscans = [_revisit_scan(j) for j in jobs]
    else:
        import multiprocessing as mp
        with mp.get_context("spawn").Pool(args.workers) as pool:
            qscans = pool.map(_revisit_scan, jobs)
    ref = db.reference()
    eD, enorm, ekey = db.entries()
    for k in range(len(eD)):
        ref.add(eD[k], ekey[k], enorm[k])
    xy = np.array([p[:2] for p in poses])
    hits = {10: 0, 0: 0}
    true_d, false_d, shifts, ranks = [], [], [], []
    for i, j, q in zip(idx, jobs, qscans):
        D, key, norm = db.describe(torch.from_numpy(q).to(dev))
        far = np.linalg.norm(xy - np.array(j[:2]), axis=1)
        for C in (10, 0):
            top = db.query(D, key, norm, exclude_recent=0, num_candidates=C, top_k=1).cpu().numpy()[0]
            hits[C] += bool(top[0] >= 0 and far[int(top[0])] <= 5.0)
            if C == 0:
                shifts.append(int(top[2]))
        d, _ = ref.distances(D.cpu().numpy(), norm.cpu().numpy(), np.arange(len(eD)))
        true_d.append(float(d[far <= 5.0].min()))
        false_d.append(float(d[far > 10.0].min()))
        ranks.append(int((d < true_d[-1]).sum()))
    out["places_revisit_queries"] = len(idx)
    out["places_revisit_query_x_m"] = [round(j[0], 1) for j in jobs]      # (the street's walls and boxes end at x = 80 m)
    out["places_revisit_top1_within_5m_c10"], out["places_revisit_top1_within_5m_c0"] = hits[10], hits[0]
    out["places_revisit_true_match_distance_min_max"] = [round(min(true_d), 4), round(max(true_d), 4)]
    out["places_revisit_true_match_distances"] = [round(v, 4) for v in true_d]
    out["places_revisit_smallest_distance_beyond_10m"] = round(min(false_d), 4)
    out["places_revisit_distances_beyond_10m"] = [round(v, 4) for v in false_d]
    out["places_revisit_shifts"] = shifts
    out["places_revisit_entries_closer_than_the_true_match"] = ranks
    args._revisit = (db, idx, jobs, qscans, poses)      # --verify runs the same queries again
    return out


def verify_report(args, net, scans, res):
    """--verify: the runner with store and verifier beside the --places loop (already in `res`), the four calls alone,
    and the revisit pass of places_report with verification"""
    import numpy as np
    import torch
    from rslo_amd import inference, loops, places, se3
    W, N = args.warmup, args.scans
    dev = scans[0].device
    out = {}
    # exclude_recent = 1: on a drive without a revisit every scan still has a candidate (its neighbour but one), so every
    # scan pays for a whole fit and the per-scan figure is the cost of verifying, not of finding nothing to verify
    loop = dict(exclude_recent=1, num_candidates=10, top_k=1)
    cap = max(1024, W + N)
    db = places.PlaceDB(capacity=cap, device=dev)
    store = loops.KeyframeStore(capacity=cap, K=args.verify_k, device=dev)
    runner = inference.OdometryRunner(net, capacity=cap, places=db, loop=loop, keyframes=store, verify=dict())
    out["verify_ms_per_scan"], out["verify_host_ms_per_scan"] = [round(v, 3) for v in timed_feed(runner, scans, W, N)]
    out["verify_minus_places_ms_per_scan"] = round(out["verify_ms_per_scan"] - res["places_ms_per_scan"], 3)
    out["verify_minus_runner_ms_per_scan"] = round(out["verify_ms_per_scan"] - res["runner_ms_per_scan"], 3)
    out["verify_options"] = {k: (v if k != "stages" else [list(st) for st in v]) for k, v in runner.verify.items()}
    out["verify_loop"] = loop
    out["verify_K"], out["verify_store_stats"] = store.K, store.stats()
    checks = runner.loop_checks().cpu().numpy()
    out["verify_runner_statuses"] = {loops.STATUS[k]: int((checks[:, :, 0] == k).sum()) for k in sorted(loops.STATUS)}
    out["verify_runner_edges"] = runner.loop_edges()[3].tolist()
    cands = runner.loop_candidates().clone()
    runner.close()

    # the four calls alone: the store holds the whole drive while it is verified against
    ver, edges = loops.LoopVerifier(store), loops.EdgeList(256, device=dev)
    row = torch.zeros((1, loops.OUT_COLS), dtype=torch.float64, device=dev)
    out["verify_entries_when_verified"] = W + N
    out["verify_prepare_ms"] = round(device_ms(lambda i: store.prepare(scans[W + i]), N), 4)
    out["verify_verify_top1_ms"] = round(device_ms(lambda i: ver.verify(cands[W + i], out=row), N), 4)
    out["verify_emit_ms"] = round(device_ms(lambda i: edges.emit(row, store), N), 4)
    side = loops.KeyframeStore(capacity=cap, K=args.verify_k, device=dev)
    side.prepare(scans[W])
    out["verify_add_ms"] = round(device_ms(lambda i: side.add(), N), 4)

    # revisit, as in places_report: three candidates of the exhaustive search per query, verified
    pdb, idx, jobs, qscans, poses = args._revisit
    pose7 = lambda x, y, yaw: np.array([x, y, 0.0, np.cos(0.5 * yaw), 0.0, 0.0, np.sin(0.5 * yaw)])
    xy = np.array([p[:2] for p in poses])
    rows3 = torch.zeros((3, loops.OUT_COLS), dtype=torch.float64, device=dev)
    queries, accepted_true, accepted_false, rejected_true, t_err, r_err = [], 0, 0, 0, [], []
    ms = []
    for i, j, q in zip(idx, jobs, qscans):
        qs = torch.from_numpy(q).to(dev)
        D, key, norm = pdb.describe(qs)
        top = pdb.query(D, key, norm, exclude_recent=0, num_candidates=0, top_k=3)
        store.prepare(qs)
        ms.append(device_ms(lambda _: ver.verify(top, out=rows3), 1))
        got = rows3.cpu().numpy()
        far = np.linalg.norm(xy - np.array(j[:2]), axis=1)
        rec = []
        for o in got:
            e = int(o[1])
            near = bool(e >= 0 and far[e] <= 5.0)
            item = {"entry": e, "status": loops.STATUS[int(o[0])], "overlap": round(float(o[3]), 3), "within_5m": near}
            if o[0] == 0:
                truth = se3.between(pose7(*poses[e]), pose7(j[0], j[1], j[2]))
                et = float(np.linalg.norm(o[6:9] - truth[:3]))
                er = float(np.rad2deg(2.0 * np.arccos(min(abs(float(np.dot(o[9:13], truth[3:]))), 1.0))))
                item["t_err_m"], item["r_err_deg"] = round(et, 4), round(er, 4)
                if near:
                    t_err.append(et)
                    r_err.append(er)
            accepted_true += bool(o[0] == 0 and near)
            accepted_false += bool(o[0] == 0 and not near)
            rejected_true += bool(o[0] != 0 and near)
            rec.append(item)
        queries.append(rec)
    out["verify_revisit_queries"] = len(idx)
    out["verify_revisit_top3_ms"] = round(float(np.mean(ms)), 4)
    out["verify_revisit_accepted_within_5m"], out["verify_revisit_accepted_beyond_5m"] = accepted_true, accepted_false
    out["verify_revisit_rejected_within_5m"] = rejected_true
    out["verify_revisit_t_err_m_max"] = round(max(t_err), 4) if t_err else None
    out["verify_revisit_r_err_deg_max"] = round(max(r_err), 4) if r_err else None
    out["verify_revisit_rows"] = queries
    return out


def rebuild_report(args, net, scans, res):
    """--rebuild-map: the map rebuilt from the keyframe store in one call beside the same rebuild as one insert per frame"""
    import numpy as np
    import torch
    from rslo_amd import inference, loops, mapping, places, posegraph
    dev = scans[0].device
    n, K = len(scans), args.verify_k
    cap = max(1024, n)
    out = {}
    store = loops.KeyframeStore(capacity=cap, K=K, device=dev)
    runner = inference.OdometryRunner(net, capacity=cap, voxel_map=mapping.VoxelMap(args.map_voxel, args.map_capacity, device=dev),
                                      places=places.PlaceDB(capacity=cap, device=dev),
                                      loop=dict(exclude_recent=1, num_candidates=10, top_k=1), keyframes=store, verify=dict(),
                                      pose_graph=posegraph.PoseGraph(capacity=max(8192, cap), max_loops=256, device=dev))
    runner.feed(scans)
    poses, _ = runner.close_verified_loops()
    torch.cuda.synchronize()
    out["rebuild_loop_edges"] = runner.loop_edges()[3].tolist()
    runner.rebuild_map()                                       # the public path once, before the tables are taken apart
    out["rebuild_runner_map_stats"] = runner.voxel_map.stats()
    runner.close()

    # the second size: 4096 entries, the streamed frames re-added under two laps of a circle, one metre per frame
    F = 4096
    rows, counts = store.frames()
    infos = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    infos[:, 0] = counts[:n]
    big = loops.KeyframeStore(capacity=F, K=K, device=dev)
    for e in range(F):
        big.add(rows[e % n], infos[e % n])
    a = 2.0 * (2.0 * np.pi) * np.arange(F) / F
    R = F / (2.0 * 2.0 * np.pi)
    lap = np.stack([R * np.sin(a), R * (1.0 - np.cos(a)), np.zeros(F), np.cos(a / 2), np.zeros(F), np.zeros(F), np.sin(a / 2)], 1)
    reps = 5
    for name, st, P in (("streamed", store, poses), ("4096", big, torch.from_numpy(lap).to(dev))):
        m = int(P.shape[0])
        slots = args.map_capacity
        while slots < 2 * m * K:                               # room for every point in a cell of its own at half load
            slots *= 2
        one, per = (mapping.VoxelMap(args.map_voxel, slots, device=dev) for _ in range(2))
        per.reserve(K)
        frows, fcounts = st.frames()
        chost = fcounts[:m].tolist()                           # the per-frame loop needs the counts on the host: read once, untimed

        def one_call():
            one.insert_frames(st, P)

        def per_frame():
            for e in range(m):
                per.insert(frows[e][:chost[e]], P[e])
        ms = {"one_call": [], "per_frame": []}
        for rep in range(reps + 1):                            # rep 0 warms both up; then the two alternate
            for key, vm, fn in (("one_call", one, one_call), ("per_frame", per, per_frame)):
                vm.reset()
                t = device_ms(lambda _: fn(), 1)
                if rep:
                    ms[key].append(t)
        got = [[t.cpu().numpy().tobytes() for t in vm.points()] for vm in (one, per)]
        st_one = one.stats()
        rec = {"frames": m, "K": K, "map_slots": slots, "points": st_one["n_points"], "cells": st_one["n_cells"],
               "dropped_full": st_one["dropped_full"], "dropped_range": st_one["dropped_range"], "reps": reps,
               "bit_equal": bool(got[0] == got[1] and st_one == per.stats())}
        for key, v in ms.items():
            rec[key + "_ms"] = {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        out["rebuild_" + name] = rec
        del one, per, got
    return out


def local_map_report(args, net, scans, res):
    """The map loops with a rolling local map beside the figures of the same loops without one (already in `res`, or
    measured here in the same way)."""
    import torch
    from rslo_amd import inference, mapping, synthetic
    dev = scans[0].device
    W, N = args.warmup, args.scans
    lm = dict(radius=args.local_map_radius, every=args.local_map_every)
    out = {"local_map": lm}

    def runner_loop(name, base, **kw):
        vmap = mapping.VoxelMap(args.map_voxel, args.map_capacity, dev)
        runner = inference.OdometryRunner(net, voxel_map=vmap, local_map=lm, **kw)
        out[name + "_ms_per_scan"], out[name + "_host_ms_per_scan"] = [round(v, 3) for v in timed_feed(runner, scans, W, N)]
        out[name + "_minus_%s_ms_per_scan" % base] = round(out[name + "_ms_per_scan"] - res[base + "_ms_per_scan"], 3)
        out[name + "_stats"], out[name + "_prune_stats"] = vmap.stats(), vmap.prune_stats()
        # once more, untimed, for the largest n_cells: behind a run() that pruned, the cells in front of that prune are
        # the cells now plus what the prune evicted or lost (two host reads per prune, hence not in the timed loop)
        runner.reset()
        peak, gone = 0, 0
        for i in range(W + N):
            runner.feed(scans[i:i + 1])
            if (i + 1) % lm["every"] == 0 or i == W + N - 1:
                ps = vmap.prune_stats()
                peak = max(peak, vmap.stats()["n_cells"] + ps["n_evicted"] + ps["n_lost"] - gone)
                gone = ps["n_evicted"] + ps["n_lost"]
        out[name + "_largest_n_cells"] = peak
        out[name + "_largest_load"] = round(peak / float(args.map_capacity), 4)
        out[name + "_dropped_full"] = vmap.stats()["dropped_full"]
        runner.close()

    runner_loop("local_map", "map")
    if args.refine:
        runner_loop("local_refine", "refine", refine=dict(iters=args.refine_iters))
    # the inserts alone under the drive's own poses, without and with pruning
    true = [torch.from_numpy(synthetic.sequence_pose(i, args.seed)).to(dev) for i in range(W + N)]
    alone = mapping.VoxelMap(args.map_voxel, args.map_capacity, dev)
    alone.reserve(max(s.shape[0] for s in scans))
    alone.reserve_prune()
    K, R = lm["every"], lm["radius"]
    tail = min(200, N)

    def drive(prune):
        """Three passes over the drive: timed as a whole (no event inside the loop, so nothing but the calls themselves
        is charged); every prune call between two events of its own; n_cells read where it peaks."""
        alone.reset()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        for i in range(W + N):
            if i == W:
                torch.cuda.synchronize()
                ev[0].record()
            if i == W + N - tail:
                ev[1].record()
            alone.insert(scans[i], true[i])
            if prune and (i + 1) % K == 0:
                alone.prune(true[i], R)
        ev[2].record()
        ev[2].synchronize()
        r = {"ms_per_scan": round(ev[0].elapsed_time(ev[2]) / N, 4),
             "last_%d_ms_per_scan" % tail: round(ev[1].elapsed_time(ev[2]) / tail, 4),
             "stats": alone.stats(), "prune_stats": alone.prune_stats()}
        # once more: n_cells in front of every prune (without pruning it only grows), each prune call timed on its own
        alone.reset()
        peak, calls = 0, []
        for i in range(W + N):
            alone.insert(scans[i], true[i])
            if (i + 1) % K == 0 or i == W + N - 1:
                n_cells = alone.stats()["n_cells"]
                peak = max(peak, n_cells)
                if prune and (i + 1) % K == 0:
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    alone.prune(true[i], R)
                    b.record()
                    calls.append((i, n_cells, a, b))
        torch.cuda.synchronize()
        r["largest_n_cells"] = peak
        r["largest_load"] = round(peak / float(args.map_capacity), 4)
        if calls:
            ms = [a.elapsed_time(b) for i, n, a, b in calls if i >= W]
            evicting = [i for i, n, a, b in calls if i >= W]
            r["prune_calls_timed"] = len(ms)
            if ms:
                r["prune_ms_per_call_mean"] = round(sum(ms) / len(ms), 4)
                r["prune_ms_per_call_min"], r["prune_ms_per_call_max"] = round(min(ms), 4), round(max(ms), 4)
                r["prune_ms_per_scan"] = round(sum(ms) / N, 4)
                loads = [n / float(args.map_capacity) for i, n, a, b in calls if i >= W]
                r["prune_load_min"], r["prune_load_max"] = round(min(loads), 4), round(max(loads), 4)
                r["prune_last_calls"] = [[evicting[k], round(loads[k], 4), round(ms[k], 4)] for k in range(max(0, len(ms) - 5), len(ms))]
        return r

    out["true_pose_plain"] = drive(False)
    out["true_pose_local_map"] = drive(True)
    # a call that evicts nothing, on the map the pruned pass left
    out["prune_load_at_no_evict_calls"] = round(alone.stats()["n_cells"] / float(args.map_capacity), 4)
    alone.prune(true[-1], float("inf"))
    out["prune_no_evict_ms_per_call"] = round(device_ms(lambda _: alone.prune(true[-1], float("inf")), 20), 4)
    return out


def _pose_error(a, b):
    """(metres, degrees) between two poses"""
    import numpy as np
    from rslo_amd import se3
    d = se3.compose(se3.inverse(b), a)
    return float(np.linalg.norm(a[:3] - b[:3])), float(np.rad2deg(2.0 * np.arcsin(min(1.0, np.linalg.norm(d[4:])))))


def refine_report(args, net, scans, res):
    """--refine: the runner with scan-to-map refinement beside the --map loop, and the registration-alone pass"""
    from rslo_amd import inference, mapping
    dev = scans[0].device
    W, N, K = args.warmup, args.scans, args.refine_iters
    out = {"refine_iters": K}
    rmap = mapping.VoxelMap(args.map_voxel, args.map_capacity, dev)
    runner = inference.OdometryRunner(net, voxel_map=rmap, refine=dict(iters=K))
    out["refine_ms_per_scan"], out["refine_host_ms_per_scan"] = [round(v, 3) for v in timed_feed(runner, scans, W, N)]
    out["refine_minus_map_ms_per_scan"] = round(out["refine_ms_per_scan"] - res["map_ms_per_scan"], 3)
    info = runner.refine_info().cpu().numpy()
    out["refine_runner_status_counts"] = [int((info[:, :, 0] == k).sum()) for k in range(4)]
    out["refine_runner_mean_pairs"] = round(float(info[1:, 0, 1].mean()), 1)
    out["refine_map_stats"] = rmap.stats()
    runner.close()
    # registration alone: the drive's own motion, disturbed by a fixed seeded error, corrected against the map so far
    rmap.reserve(max(s.shape[0] for s in scans))
    out.update(register_alone(args, scans, rmap, lambda s, pose: rmap.register(s, pose, iters=K)[1], "register_alone"))
    out["register_alone_ms_per_iteration"] = round(out["register_alone_ms_per_call"] / K, 4)
    return out


def register_alone(args, scans, target, call, name, pairs_row=0):
    """The registration-alone pass: the prediction of scan i is refined[i-1] o (true relative motion o a seeded error of
    about 5 cm and 0.1 degrees; the same draws for every caller); call(scan, pose) corrects pose in place against
    `target` (a VoxelMap or a MapPyramid, reset here) and returns its info rows; the scan is inserted under the result."""
    import numpy as np
    import torch
    from rslo_amd import se3, synthetic
    dev = scans[0].device
    W, N = args.warmup, args.scans
    out = {}
    true = [synthetic.sequence_pose(i, args.seed) for i in range(W + N)]
    rng = np.random.default_rng(777)
    target.reset()
    pose = torch.zeros((7,), dtype=torch.float64, device=dev)
    refined = true[0].copy()
    target.insert(scans[0], refined)
    before, after, pairs, status, ms, left = [], [], [], [], [], []
    for i in range(1, W + N):
        axis = rng.normal(size=3)
        ang = np.deg2rad(0.1) * rng.uniform(0.5, 1.5)
        err = np.concatenate([0.05 * rng.normal(size=3) * [1.0, 1.0, 0.3], [np.cos(ang / 2)],
                              np.sin(ang / 2) * axis / np.linalg.norm(axis)])
        pred = se3.compose(refined, se3.compose(se3.compose(se3.inverse(true[i - 1]), true[i]), err))
        pose.copy_(torch.from_numpy(pred))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        info = call(scans[i], pose)
        e1.record()
        refined = pose.cpu().numpy()                # (a host read per scan: this pass times register alone)
        target.insert(scans[i], pose)
        before.append(_pose_error(pred, true[i]))
        after.append(_pose_error(refined, true[i]))
        left.append(refined[:3] - true[i][:3])      # world frame: x runs along the synthetic street, y across it, z up
        info = info.cpu().numpy()
        pairs.append(float(info[pairs_row, 1]))
        status.append(info[:, 0].tolist())
        if i >= W:
            ms.append(e0.elapsed_time(e1))
    before, after = np.array(before), np.array(after)
    out[name + "_ms_per_call"] = round(float(np.mean(ms)), 4)
    out[name + "_pairs_per_scan"] = round(float(np.mean(pairs)), 1)
    out[name + "_status_counts"] = [int((np.array(status) == k).sum()) for k in range(4)]
    for which, e in (("before", before), ("after", after)):
        out["%s_%s_trans_m_mean" % (name, which)] = round(float(e[:, 0].mean()), 5)
        out["%s_%s_trans_m_max" % (name, which)] = round(float(e[:, 0].max()), 5)
        out["%s_%s_rot_deg_mean" % (name, which)] = round(float(e[:, 1].mean()), 5)
        out["%s_%s_rot_deg_max" % (name, which)] = round(float(e[:, 1].max()), 5)
    left = np.array(left)
    out[name + "_after_err_xyz_mean_abs_m"] = [round(float(v), 5) for v in np.abs(left).mean(axis=0)]
    out[name + "_after_err_xyz_last_m"] = [round(float(v), 5) for v in left[-1]]
    out[name + "_map_stats"] = target.stats()
    return out


class _Targets:
    """several registration targets that receive the same scans (register_alone's `target`)"""

    def __init__(self, *targets):
        self.targets = targets

    def reset(self):
        for t in self.targets:
            t.reset()

    def insert(self, points, pose):
        for t in self.targets:
            t.insert(points, pose)

    def stats(self):
        return [t.stats() for t in self.targets]


def surfel_report(args, net, scans, res):
    """--surfels: the runner with a surfel map and its registration stage; surfel inserts beside voxel-map inserts under
    the drive's own poses; and the registration-alone pass with the parent's best row (pyramid, factor 0.5), the
    surfels alone, and the pyramid followed by the surfel stage, in this one process."""
    import torch
    from rslo_amd import inference, mapping, surfels, synthetic
    dev = scans[0].device
    W, N, K = args.warmup, args.scans, args.surfel_iters
    opts = dict(surfels.SURFEL_REFINE_DEFAULTS, iters=K)
    out = {"surfel_voxel": args.surfel_voxel, "surfel_refine": opts}
    smap = surfels.SurfelMap(args.surfel_voxel, 1 << 20, dev)
    plain = inference.OdometryRunner(net)
    out["surfel_plain_ms_per_scan"], _ = [round(v, 3) for v in timed_feed(plain, scans, W, N)]
    plain.close()
    runner = inference.OdometryRunner(net, surfels=smap, surfel_refine=opts)
    out["surfel_ms_per_scan"], out["surfel_host_ms_per_scan"] = [round(v, 3) for v in timed_feed(runner, scans, W, N)]
    info = runner.surfel_refine_info().cpu().numpy()
    out["surfel_runner_status_counts"] = [int((info[:, :, 0] == k).sum()) for k in range(4)]
    out["surfel_runner_map_stats"] = smap.stats()
    runner.close()
    # the inserts alone under the drive's own poses, each beside the voxel map's insert at the same cell edge
    true = [torch.from_numpy(synthetic.sequence_pose(i, args.seed)).to(dev) for i in range(W + N)]
    for voxel in sorted({args.surfel_voxel, 0.8}):
        targets = (("surfel_insert_alone_v%g_ms_per_scan" % voxel, surfels.SurfelMap(voxel, 1 << 20, dev)),
                   ("map_insert_alone_v%g_ms_per_scan" % voxel, mapping.VoxelMap(voxel, 1 << 20, dev)))
        for name, target in targets:
            target.reserve(max(s.shape[0] for s in scans))
            for i in range(W):
                target.insert(scans[i], true[i])
            out[name] = round(device_ms(lambda i: target.insert(scans[W + i], true[W + i]), N), 4)
            out[name.replace("_ms_per_scan", "_stats")] = target.stats()
    # the registration-alone pass: the same seeded disturbance for every row
    smap.reserve(max(s.shape[0] for s in scans))
    pyr = mapping.MapPyramid((0.8, 0.4, 0.2), args.map_capacity, dev)
    pyr.reserve(max(s.shape[0] for s in scans))
    sch = pyr.default_schedule(4, 0.5)
    kw = {k: v for k, v in opts.items() if k != "iters"}
    out.update(register_alone(args, scans, pyr, lambda s, p: pyr.register(s, p, sch)[1], "pyramid_alone_f0.5", pairs_row=-1))
    out.update(register_alone(args, scans, smap, lambda s, p: smap.register(s, p, iters=K, **kw)[1], "surfel_alone"))
    out["surfel_alone_ms_per_iteration"] = round(out["surfel_alone_ms_per_call"] / K, 4)
    out.update(register_alone(args, scans, _Targets(pyr, smap),
                              lambda s, p: torch.cat([pyr.register(s, p, sch)[1], smap.register(s, p, iters=K, **kw)[1]]),
                              "pyramid_then_surfel", pairs_row=-1))
    return out


def surfel_dist_report(args, scans):
    """--surfels --surfel-cost distribution: the registration-alone pass (register_alone: the same seeded disturbance
    for every row) against a surfel map, once with the plane cost and the runner's defaults and once with the
    point-to-distribution cost over every fitted cell and its defaults, in this one process: ms per call and per
    iteration, pairs, and the error against the synthetic truth behind the last iteration."""
    from rslo_amd import surfels
    K = args.surfel_iters
    out = {"surfel_voxel": args.surfel_voxel}
    smap = surfels.SurfelMap(args.surfel_voxel, 1 << 20, scans[0].device)
    smap.reserve(max(s.shape[0] for s in scans))
    rows = (("surfel_alone", {}), ("surfel_dist_alone", dict(cost="distribution", reg_abs=args.surfel_reg_abs)))
    for name, options in rows:
        kw = surfels.check_surfel_refine(dict(options, iters=K), smap)
        out[name + "_options"] = kw
        out.update(register_alone(args, scans, smap, lambda s, p: smap.register(s, p, **kw)[1], name))
        out[name + "_ms_per_iteration"] = round(out[name + "_ms_per_call"] / K, 4)
        print("%-18s %.4f ms per call, %.4f ms per iteration, %.1f pairs, error %.5f -> %.5f m, %.5f -> %.5f deg" % (
            name, out[name + "_ms_per_call"], out[name + "_ms_per_iteration"], out[name + "_pairs_per_scan"],
            out[name + "_before_trans_m_mean"], out[name + "_after_trans_m_mean"], out[name + "_before_rot_deg_mean"],
            out[name + "_after_rot_deg_mean"]), flush=True)
    out["surfel_dist_over_plane_ms_per_iteration"] = round(
        out["surfel_dist_alone_ms_per_iteration"] / out["surfel_alone_ms_per_iteration"], 3)
    return out


def deskew_report(args, net, scans, res):
    """--deskew: the skewed twin of the drive de-skewed on the device; the registration-alone pass on the original, the
    skewed and the de-skewed scans against a surfel map; the kernel alone; the runner with and without deskew=."""
    import numpy as np
    import torch
    from rslo_amd import deskew, inference, se3, surfels, synthetic
    dev = scans[0].device
    W, N, K = args.warmup, args.scans, args.surfel_iters
    opts = dict(deskew.DESKEW_DEFAULTS)
    out = {"deskew": opts, "deskew_surfel_voxel": args.surfel_voxel}
    true = [synthetic.sequence_pose(i, args.seed) for i in range(W + N)]
    pairs = [(true[max(i - 1, 0)], true[max(i, 1)]) for i in range(W + N)]      # scan 0: the motion of the sweep after it
    stage = deskew.Deskewer(max(s.shape[0] for s in scans), scans[0].shape[1], dev)
    skewed, flat, d_skew, d_flat, angles, steps = [], [], [], [], [], []
    for s, (A, B) in zip(scans, pairs):
        block = deskew.motion_ref(pose_a=A, pose_b=B, stamp=opts["stamp"])
        host = s.cpu().numpy()
        twin = torch.from_numpy(deskew.skew_ref(host, None, block, stamp=opts["stamp"], normal_col=4).astype(np.float32)).to(dev)
        skewed.append(twin)
        flat.append(stage(twin, pose_a=torch.from_numpy(A).to(dev), pose_b=torch.from_numpy(B).to(dev)).clone())
        d_skew.append((twin[:, :3] - s[:, :3]).norm(dim=1))
        d_flat.append((flat[-1][:, :3] - s[:, :3]).norm(dim=1))
        angles.append(block[3])
        steps.append(float(np.linalg.norm(se3.between(A, B)[:3])))
    out["deskew_motion_mean_m"] = round(float(np.mean(steps)), 4)
    out["deskew_motion_mean_deg"] = round(float(np.rad2deg(np.mean(angles))), 4)
    for name, d in (("skewed", torch.cat(d_skew)), ("deskewed", torch.cat(d_flat))):
        p99 = (d if d.numel() < (1 << 24) else d[::8]).quantile(0.99)       # (quantile takes 2^24 elements at the most)
        out["deskew_%s_point_offset_m" % name] = {"mean": float(d.mean()), "p99": float(p99), "max": float(d.max())}
    # the registration-alone pass: the same seeded disturbance and the same map parameters for the three lists
    smap = surfels.SurfelMap(args.surfel_voxel, 1 << 20, dev)
    smap.reserve(max(s.shape[0] for s in scans))
    kw = {k: v for k, v in surfels.SURFEL_REFINE_DEFAULTS.items() if k != "iters"}
    for name, rows in (("original", scans), ("skewed", skewed), ("deskewed", flat)):
        out.update(register_alone(args, rows, smap, lambda s, p: smap.register(s, p, iters=K, **kw)[1], "deskew_%s_alone" % name))
    # the kernel alone: one launch per scan, the pose pair already on the device
    dpairs = [(torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev)) for A, B in pairs]
    stage(skewed[0], pose_a=dpairs[0][0], pose_b=dpairs[0][1])
    out["deskew_kernel_ms_per_call"] = round(device_ms(lambda i: stage(skewed[W + i], pose_a=dpairs[W + i][0],
                                                                       pose_b=dpairs[W + i][1]), N), 5)
    out["deskew_kernel_bytes_per_call"] = int(2 * 4 * sum(s.numel() for s in skewed[W:W + N]) / N)
    # the runner with and without the stage, alternated in this one process
    for name, kwargs in (("plain", {}), ("surfels", dict(surfel_refine=dict(surfels.SURFEL_REFINE_DEFAULTS, iters=K)))):
        for rep in range(2):
            for which, extra in (("without", {}), ("with", dict(deskew={}))):
                if "surfel_refine" in kwargs:
                    smap.reset()
                    kwargs["surfels"] = smap
                runner = inference.OdometryRunner(net, **kwargs, **extra)
                ms, host_ms = timed_feed(runner, skewed, W, N)
                key = "deskew_runner_%s_%s_ms_per_scan" % (name, which)
                out[key] = min(out.get(key, float("inf")), round(ms, 3))
                if extra:
                    info = runner.deskew_info().cpu().numpy()
                    out["deskew_runner_%s_status_counts" % name] = [int((info[:, 7] == k).sum()) for k in range(4)]
                runner.close()
    return out


def surfel_local_map_report(args, scans, reps=11, pruned_drive=True):
    """--surfels with --local-map-radius R: the surfel map (capacity 2^20) filled under the drive's own poses without
    pruning, and once more pruned about the scan's pose every K scans (SurfelMap.prune, rslo_surfel_prune in
    csrc/surfel.hip): counters, prune counters and the largest n_cells seen, side by side.  Then the prune call itself on
    the table the unpruned drive left, about the last pose: the table is put back from a copy in front of every timed
    call (outside the events), one warm-up, the median, min and max of `reps` calls and the survivors' count; beside it
    VoxelMap.prune at the same capacity, cell edge, centre and radius, timed the same way in the same process; and a call
    of each that evicts nothing.  Needs only the scans (--seed must be the drive's)."""
    import statistics
    import torch
    from rslo_amd import mapping, surfels, synthetic
    dev = scans[0].device
    R, K, M, ri = args.local_map_radius, args.local_map_every, args.surfel_min_count, args.surfel_inner_radius
    voxel, cap, n = args.surfel_voxel, 1 << 20, len(scans)
    true = [torch.from_numpy(synthetic.sequence_pose(i, args.seed)).to(dev) for i in range(n)]
    out = {"surfel_local_map": dict(radius=R, every=K, min_count=M, inner_radius=R if ri is None else ri),
           "surfel_local_map_scans": n, "surfel_local_map_capacity": cap}

    def drive(target, prune):
        target.reserve(max(s.shape[0] for s in scans))
        peak = 0
        for i in range(n):
            target.insert(scans[i], true[i])
            if prune and (i + 1) % K == 0:
                peak = max(peak, target.stats()["n_cells"])
                prune(target, true[i])
        return max(peak, target.stats()["n_cells"])

    def timed(target, prune):
        """ms of prune(target, last pose) on the table as it is now: (median, min, max, n_cells afterwards)"""
        table, ms = target._buf.clone(), []
        for rep in range(reps + 1):
            target._buf.copy_(table)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            prune(target, true[-1])
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms = ms[1:]
        return [round(statistics.median(ms), 4), round(min(ms), 4), round(max(ms), 4), target.stats()["n_cells"]]

    def surfel_prune(t, c):
        t.prune(c, R, ri, M)

    def map_prune(t, c):
        t.prune(c, R)
    smap = surfels.SurfelMap(voxel, cap, dev)
    smap.reserve_prune()
    out["surfel_unpruned_peak_cells"] = drive(smap, None)
    out["surfel_unpruned_stats"] = smap.stats()
    if pruned_drive:
        local = surfels.SurfelMap(voxel, cap, dev)
        local.reserve_prune()
        out["surfel_local_map_peak_cells"] = drive(local, surfel_prune)
        out["surfel_local_map_stats"], out["surfel_local_map_prune_stats"] = local.stats(), local.prune_stats()
        del local
    vmap = mapping.VoxelMap(voxel, cap, dev)
    vmap.reserve_prune()
    drive(vmap, None)
    out["map_unpruned_stats"] = vmap.stats()
    for name, target, prune in (("surfel_prune", smap, surfel_prune), ("map_prune", vmap, map_prune)):
        out[name + "_cells_before"] = target.stats()["n_cells"]
        out[name + "_no_evict_ms_median_min_max_survivors"] = timed(target, lambda t, c: t.prune(c, float("inf")))
        out[name + "_ms_median_min_max_survivors"] = timed(target, prune)
    out["surfel_prune_staged_bytes_per_survivor"] = 2 * 152
    return out


def pyramid_report(args, net, scans, res):
    """Coarse-to-fine robust registration beside the figures of the --refine loop of this process (already in `res`)."""
    import torch
    from rslo_amd import inference, mapping, synthetic
    dev = scans[0].device
    W, N, K, per = args.warmup, args.scans, args.refine_iters, args.refine_iters_per_level
    levels = tuple(args.refine_levels)
    pyr = mapping.MapPyramid(levels, args.map_capacity, dev)
    sched = pyr.default_schedule(per, args.refine_robust)
    out = {"pyramid_levels": list(levels), "pyramid_schedule": [list(st) for st in sched]}
    runner = inference.OdometryRunner(net, voxel_map=pyr, refine=dict(schedule=sched))
    out["pyramid_refine_ms_per_scan"], out["pyramid_refine_host_ms_per_scan"] = [
        round(v, 3) for v in timed_feed(runner, scans, W, N)]
    out["pyramid_refine_minus_refine_ms_per_scan"] = round(out["pyramid_refine_ms_per_scan"] - res["refine_ms_per_scan"], 3)
    info = runner.refine_info().cpu().numpy()
    out["pyramid_refine_runner_status_counts"] = [int((info[:, :, 0] == k).sum()) for k in range(4)]
    out["pyramid_refine_map_stats"] = pyr.stats()
    runner.close()
    # the inserts alone under the drive's own poses: every level of the pyramid beside its finest level alone
    true = [torch.from_numpy(synthetic.sequence_pose(i, args.seed)).to(dev) for i in range(W + N)]
    pyr.reserve(max(s.shape[0] for s in scans))
    for name, target in (("pyramid_finest_insert_alone_ms_per_scan", pyr.levels[-1]), ("pyramid_insert_alone_ms_per_scan", pyr)):
        pyr.reset()
        for i in range(W):
            target.insert(scans[i], true[i])
        out[name] = round(device_ms(lambda i: target.insert(scans[W + i], true[W + i]), N), 4)
    out["pyramid_true_pose_stats"] = pyr.stats()
    # the registration-alone pass, the same seeded disturbance for every setting
    single = mapping.VoxelMap(args.map_voxel, args.map_capacity, dev)
    single.reserve(max(s.shape[0] for s in scans))
    scale = (mapping.DEFAULT_ROBUST_FACTOR if args.refine_robust is None else args.refine_robust) * args.map_voxel
    out["weighted_scale"] = scale
    out.update(register_alone(args, scans, single, lambda s, p: single.register(s, p, iters=K)[1], "parent_alone"))
    out.update(register_alone(args, scans, single, lambda s, p: single.register(s, p, iters=K, robust_scale=scale)[1],
                              "weighted_alone"))
    for f in (0.0, 0.5, 1.0):
        sch = pyr.default_schedule(per, f)
        out.update(register_alone(args, scans, pyr, lambda s, p: pyr.register(s, p, sch)[1], "pyramid_alone_f%g" % f,
                                  pairs_row=-1))
    return out


if __name__ == "__main__":
    main()
