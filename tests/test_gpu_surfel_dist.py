"""The point-to-distribution cost of the surfel map on the GPU (csrc/surfel.hip: rslo_surfel_nearest_d / _normal_eq_d /
_register_d; rslo_amd/surfels.py SurfelMap with cost="distribution") against the float64 restatement SurfelMapRef run
on the same fp32 inputs, and the distribution stage of an OdometryRunner.

The bars are those of tests/test_gpu_surfels.py and follow from the formats, not from what the kernels return:
  * nearest_d: BIT equality of keys, d2, rows and the information rows {M, det, lam}: the match is the plane call's, and
    an information row is a fixed sequence of double +, -, *, / on the slot's integers.
  * normal equations: the pair count is exact; each of the 28 sums is held to K * 2^-50 * sum|addend| over the K addends
    of SurfelMapRef._pair_terms: the addends are the same expressions in the same order, only the summation order differs.
  * one Gauss-Newton step from the same pose: 1e4 * cond2(H) * 2^-52 * (1 + |t|).
"""
import numpy as np
import pytest
import torch
from stream_support import cond_of, dev, odom_fixture, same_bits, seed_poses, stream
from test_gpu_loops import quiet_collector
from test_gpu_mapreg import IDENT, POSE_FULL
from test_gpu_surfels import SENTINEL, SURF_ARGS, drive, same_device_maps      # noqa: F401 (drive is a fixture)
from test_surfel_dist_host import POLE_START, pole_scene
from test_surfels_host import DRIVE_ARGS, drive_start, lattice

pytestmark = pytest.mark.gpu

DIST = (1, 0.01, 0.02)                                     # min_flag, reg_rel, reg_abs: the defaults
D = dict(cost="distribution")


def _same_nearest_d(smap, ref, q, pose, label="", dev_q=None, **kw):
    got = smap.nearest(dev(q) if dev_q is None else dev_q, dev(pose), return_rows=True, return_info=True, **D, **kw)
    want = ref.nearest(q, pose, return_rows=True, return_info=True, **D, **kw)
    got = [t.cpu().numpy() for t in got]
    print("%s: %d queries, %d matched (reference %d)" % (label, len(q), int((got[0] >= 0).sum()), int((want[0] >= 0).sum())))
    assert [g.dtype for g in got] == [np.int64, np.float64, np.float64, np.float64]
    assert got[2].shape == got[3].shape == (len(q), 8)
    assert (got[0] == want[0]).all()
    for g, w in zip(got[1:], want[1:]):
        assert (g.view(np.int64) == w.view(np.int64)).all()
    return want


# ---------------------------------------------------------------------------------------------------------------------
# nearest_d
# ---------------------------------------------------------------------------------------------------------------------
def test_nearest_d_on_the_drive(drive):
    ref, smap = drive["ref"], drive["smap"]
    before = smap._buf.clone()
    for min_flag in (1, 2):
        wk, _, wrows, winfo = _same_nearest_d(smap, ref, drive["raw"], drive["start"], "drive, min_flag %d" % min_flag,
                                              min_flag=min_flag)
        assert (wk >= 0).sum() > 3000 and (wk < 0).sum() > 1000
        assert (winfo[wk >= 0, 6] > 0).all() and not winfo[wk < 0].any()
        assert ((wrows[wk >= 0, 7] == 1.0).sum() > 500) == (min_flag == 1)
    _same_nearest_d(smap, ref, drive["raw"], drive["start"], "drive, max_dist 0.25, other regularisation", max_dist=0.25,
                    reg_rel=0.05, reg_abs=0.0)
    _same_nearest_d(smap, ref, drive["raw"], POSE_FULL, "drive, tilted")
    q7 = dev(drive["scans"][2])
    for view in (q7, q7[:, :3], q7[:, :3].contiguous()):   # stride 7 (two widths) and stride 3
        _same_nearest_d(smap, ref, drive["scans"][2], drive["start"], "stride %d" % view.stride(0), dev_q=view)
    # with min_flag = 2 the match is the plane call's
    k2, d2 = smap.nearest(drive["dev2"], dev(drive["start"]), min_flag=2, **D)
    kp, dp = smap.nearest(drive["dev2"], dev(drive["start"]))
    assert torch.equal(k2, kp) and same_bits(d2, dp)
    assert torch.equal(before, smap._buf)                   # read-only: every bit of the table and its header


@pytest.mark.parametrize("min_flag", [1, 2])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 513])
def test_nearest_d_sizes(drive, N, min_flag):
    from rslo_amd import capi
    ref, smap = drive["ref"], drive["smap"]
    q = drive["mixed"][:N]
    wk, wd, wr, wi = _same_nearest_d(smap, ref, q, drive["start"], "N %d min_flag %d" % (N, min_flag), min_flag=min_flag)
    assert (wk >= 0).sum() >= (N + 1) // 2 and ((wk >= 0).sum() == (N + 1) // 2 or min_flag == 1)
    sent_k = torch.full((N + 3,), -7, dtype=torch.int64, device="cuda")
    sent_d = torch.full((N + 3,), -7.0, dtype=torch.float64, device="cuda")
    sent_r = torch.full((N + 3, 8), -7.0, dtype=torch.float64, device="cuda")
    sent_i = torch.full((N + 3, 8), -7.0, dtype=torch.float64, device="cuda")
    capi.surfel_nearest_d(smap._buf, dev(q), dev(drive["start"]), 0.4, None, min_flag, 0.01, 0.02, keys=sent_k[:N],
                          d2=sent_d[:N], rows=sent_r[:N], info=sent_i[:N])
    for t in (sent_k, sent_d, sent_r, sent_i):              # nothing behind row N - 1
        assert (t[N:] == -7).all()
    assert (sent_k[:N].cpu().numpy() == wk).all()
    assert (sent_i[:N].cpu().numpy().view(np.int64) == wi.view(np.int64)).all()
    # info alone, rows alone
    only_i = capi.surfel_nearest_d(smap._buf, dev(q), dev(drive["start"]), 0.4, None, min_flag, info=True)
    only_r = capi.surfel_nearest_d(smap._buf, dev(q), dev(drive["start"]), 0.4, None, min_flag, rows=True)
    assert len(only_i) == len(only_r) == 3
    assert (only_i[2].cpu().numpy().view(np.int64) == wi.view(np.int64)).all()
    assert (only_r[2].cpu().numpy().view(np.int64) == wr.view(np.int64)).all()


# ---------------------------------------------------------------------------------------------------------------------
# normal equations and register
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [0.0, 3.0])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 513, 7374])
def test_normal_equations_d(drive, N, scale):
    ref, smap = drive["ref"], drive["smap"]
    pts = (drive["raw"] if N > 1000 else drive["mixed"])[:N]
    assert len(pts) == N
    terms = ref._weighted_terms(pts, drive["start"], robust_scale=scale, dist=DIST)
    K = len(terms)
    want = ref.normal_equations(pts, drive["start"], robust_scale=scale, **D)
    dpts, dpose = dev(pts), dev(drive["start"])
    got = smap.normal_equations(dpts, dpose, robust_scale=scale, **D).cpu().numpy()
    again = smap.normal_equations(dpts, dpose, robust_scale=scale, **D).cpu().numpy()
    bound = K * 2.0 ** -50 * np.abs(terms).sum(axis=0)
    err = np.abs(got[:28] - want[:28])
    with np.errstate(all="ignore"):
        print("N %d scale %.1f: %d pairs; worst |dev - ref| / bound %.3g" % (
            N, scale, K, np.nanmax(np.where(bound > 0, err / bound, 0.0))))
    assert got.shape == (29,) and got[28] == K == want[28]
    assert K > 4500 if N >= 7000 else K >= (N + 1) // 2
    assert K > ref.normal_equations(pts, drive["start"])[28] or N < 255       # more pairs than the plane cost
    assert (err <= bound).all()
    assert got.tobytes() == again.tobytes()
    if scale and K:
        assert got[27] < ref.normal_equations(pts, drive["start"], **D)[27]  # the weights are below one


@pytest.mark.parametrize("scale", [0.0, 3.0])
def test_one_step_teacher_forced_d(drive, scale):
    """Six successive iterations; both implementations start every one of them from the DEVICE's current pose."""
    ref, smap, pts = drive["ref"], drive["smap"], drive["raw"]
    pose = dev(drive["start"])
    for it in range(6):
        cur = pose.cpu().numpy().copy()
        want, winfo = ref.register(pts, cur, iters=1, robust_scale=scale, damping=1e-6, **D)
        out, info = smap.register(drive["dev2"], pose, iters=1, robust_scale=scale, damping=1e-6, **D)
        assert out is pose                           # in place
        got, info = pose.cpu().numpy(), info.cpu().numpy()
        assert info.shape == (1, 8) and info[0, 0] == winfo[0, 0] == 0.0 and info[0, 1] == winfo[0, 1] > 4500
        assert not info[0, 5:].any()
        bound = 1e4 * cond_of(ref.normal_equations(pts, cur, robust_scale=scale, **D)) * 2.0 ** -52 * (
            1.0 + np.linalg.norm(cur[:3]))
        err = np.abs(got - want).max()
        print("scale %.1f iteration %d: step %.3e m, |dev - ref| %.3e, bound %.3e, pairs %d" % (
            scale, it, np.linalg.norm(got[:3] - cur[:3]), err, bound, info[0, 1]))
        assert err <= bound
        assert abs(info[0, 2] - winfo[0, 2]) <= 1e-9 * winfo[0, 2]
        assert abs(info[0, 3] - winfo[0, 3]) <= bound and abs(info[0, 4] - winfo[0, 4]) <= bound


def test_whole_call_and_statuses_d(drive):
    from rslo_amd.surfels import SurfelMap, SurfelMapRef
    smap, pts, true = drive["smap"], drive["dev2"], drive["poses"][2]
    kw = dict(robust_scale=3.0, **D)
    pose8 = dev(drive["start"])
    _, info8 = smap.register(pts, pose8, iters=8, **kw)
    pose1 = dev(drive["start"])
    rows = [smap.register(pts, pose1, iters=1, **kw)[1] for _ in range(8)]
    assert same_bits(pose8, pose1) and same_bits(info8, torch.cat(rows))      # and two runs give the same bits
    plane = dev(drive["start"])
    _, pinfo = smap.register(pts, plane, iters=8)
    e0 = np.linalg.norm(drive["start"][:3] - true[:3])
    e1 = np.linalg.norm(pose8.cpu().numpy()[:3] - true[:3])
    print("distribution: translation error %.4f -> %.4f m (ratio %.3f), pairs %d (plane: %d)" % (
        e0, e1, e1 / e0, info8[-1, 1], pinfo[-1, 1]))
    assert (info8[:, 0] == 0).all() and (info8[:, 1] > pinfo[:, 1]).all() and e1 <= 0.25 * e0
    # status 3: tolerances that the first step meets
    after_one = dev(drive["start"])
    smap.register(pts, after_one, iters=1, **kw)
    pose = dev(drive["start"])
    _, info = smap.register(pts, pose, iters=4, tol_t=10.0, tol_r=10.0, **kw)
    assert info[:, 0].tolist() == [0.0, 3.0, 3.0, 3.0] and not info[1:, 1:].any() and same_bits(pose, after_one)
    pose = dev(drive["start"])
    _, info = smap.register(pts, pose, iters=8, tol_t=1e-30, tol_r=1e-30, **kw)      # never met: nothing skipped
    assert same_bits(pose, pose8) and (info[:, 0] == 0).all()
    # status 1: an empty map, N == 0, min_pairs out of reach; the pose is left alone
    start = dev(drive["start"])
    bits = start.view(torch.int64).clone()
    empty = SurfelMap(0.4, 1024, **DRIVE_ARGS)
    pose, info = empty.register(pts, start, iters=2, **kw)
    assert info[:, 0].tolist() == [1.0, 1.0] and info[:, 1].tolist() == [0.0, 0.0] and torch.equal(pose.view(torch.int64), bits)
    pose, info = smap.register(pts[:0], start, iters=2, **kw)
    assert info[:, 0].tolist() == [1.0, 1.0] and torch.equal(pose.view(torch.int64), bits)
    pose, info = smap.register(pts, start, iters=2, min_pairs=10 ** 6, **kw)
    assert info[:, 0].tolist() == [1.0, 1.0] and info[0, 1] > 4500 and torch.equal(pose.view(torch.int64), bits)
    # status 2: one fitted cell matched by ONE point, which the pose carries to w = (0, 0, 0) exactly: the rotation
    # columns of J are zeros, H is [[M, 0], [0, 0]] and its fourth pivot is 0.0 without damping
    one = SurfelMap(1.0, 1024)
    one.insert(dev(lattice()), IDENT)
    one_ref = SurfelMapRef(1.0)
    one_ref.insert(lattice(), IDENT)
    pt = np.array([[0.5, 0.25, 0.125]], np.float32)
    at = np.array([-0.5, -0.25, -0.125, 1.0, 0.0, 0.0, 0.0])
    _, winfo = one_ref.register(pt, at, iters=2, min_pairs=1, **D)
    pose, info = one.register(dev(pt), dev(at), iters=2, min_pairs=1, **D)
    assert winfo[:, 0].tolist() == [2.0, 2.0] and info[:, 0].tolist() == [2.0, 2.0] and info[:, 1].tolist() == [1.0, 1.0]
    assert pose.cpu().numpy().tobytes() == at.tobytes() and info[0, 2] == winfo[0, 2] > 0
    _, info = one.register(dev(pt), dev(at), iters=1, min_pairs=1, damping=1e-6, **D)      # damped: a step
    assert info[0, 0] == 0.0
    host = drive["start"].copy()                            # a host pose is copied, not written
    pose, _ = smap.register(pts, host, iters=1, **kw)
    assert pose.is_cuda and host.tobytes() == drive["start"].tobytes() and not torch.equal(pose.view(torch.int64), bits)


def test_scene_without_planes():
    """24 poles and 24 blobs (tests/test_surfel_dist_host.py): the plane cost finds fewer than min_pairs pairs and does not
    refine; the distribution cost does, and every step is the reference's within the teacher-forced bound."""
    from rslo_amd.surfels import SurfelMap
    ref, pts, scan = pole_scene()
    smap = SurfelMap(0.4, 1 << 14)
    smap.insert(dev(pts), IDENT)
    st = smap.stats()
    assert st == ref.stats() and st["n_planar"] < 10 and st["n_cells"] > 150
    dscan = dev(scan)
    start = dev(POLE_START)
    _, pinfo = smap.register(dscan, start, iters=8, damping=1e-6)
    assert (pinfo[:, 0] == 1).all() and (pinfo[:, 1] <= 49).all() and same_bits(start, dev(POLE_START))
    pose, info = smap.register(dscan, dev(POLE_START), iters=8, damping=1e-6, robust_scale=3.0, **D)
    _, winfo = ref.register(scan, POLE_START, iters=8, damping=1e-6, robust_scale=3.0, **D)
    e0, e1 = np.linalg.norm(POLE_START[:3]), np.linalg.norm(pose.cpu().numpy()[:3])
    print("poles: %.4f -> %.4f m (ratio %.3f), pairs %d of %d" % (e0, e1, e1 / e0, info[-1, 1], len(scan)))
    assert info[:, 0].tolist() == winfo[:, 0].tolist() == [0.0] * 8 and info[-1, 1] > 1000 and e1 <= 0.25 * e0
    pose = dev(POLE_START)
    for it in range(8):
        cur = pose.cpu().numpy().copy()
        want, winfo = ref.register(scan, cur, iters=1, damping=1e-6, robust_scale=3.0, **D)
        _, info = smap.register(dscan, pose, iters=1, damping=1e-6, robust_scale=3.0, **D)
        bound = 1e4 * cond_of(ref.normal_equations(scan, cur, robust_scale=3.0, **D)) * 2.0 ** -52 * (
            1.0 + np.linalg.norm(cur[:3]))
        err = np.abs(pose.cpu().numpy() - want).max()
        print("iteration %d: |dev - ref| %.3e, bound %.3e, pairs %d" % (it, err, bound, info[0, 1]))
        assert info[0, 0] == winfo[0, 0] == 0.0 and info[0, 1] == winfo[0, 1] and err <= bound


def test_capture_and_replay_d(drive):
    """One graph holding register(cost="distribution") over static buffers.  Replayed after the pose and after the points
    were changed it gives the eager bits: the launch count does not depend on the data and nothing reads the host."""
    smap, pts = drive["smap"], drive["dev2"]
    kw = dict(iters=3, robust_scale=3.0, tol_t=1e-4, tol_r=1e-5, **D)
    other = drive["start"].copy()
    other[:3] += (-0.03, 0.05, 0.02)
    far = torch.zeros_like(pts)
    far[:, 0] = 500.0                                       # no cell there: no pairs
    smap.reserve(len(pts))
    smap.register(pts, dev(drive["start"]), **kw)           # the kernels have run once before the capture
    static_pts = torch.zeros_like(pts)
    static_pose = torch.zeros(7, dtype=torch.float64, device="cuda")
    static_info = torch.zeros((3, 8), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with quiet_collector(), torch.cuda.graph(g):
        smap.register(static_pts, static_pose, info=static_info, **kw)
    assert not static_pose.any() and not static_info.any()  # captured, not run
    for cloud, first in ((pts, drive["start"]), (pts, other), (far, drive["start"])):
        want_pose = dev(first)
        _, want_info = smap.register(cloud, want_pose, **kw)
        static_pts.copy_(cloud)
        static_pose.copy_(dev(first))
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(static_pose, want_pose) and same_bits(static_info, want_info)
        if cloud is far:
            assert want_info[:, 0].tolist() == [1.0] * 3 and same_bits(static_pose, dev(first))
        else:
            assert want_info[0, 0] == 0 and want_info[0, 1] > 4500 and not same_bits(static_pose, dev(first))


# ---------------------------------------------------------------------------------------------------------------------
# the runner
# ---------------------------------------------------------------------------------------------------------------------
N_SCANS = 3
SURF_REFINE_D = dict(cost="distribution", iters=3)
odom = odom_fixture(21, 3, N_SCANS)


def _by_hand(scans, rel, seeds):
    """The refined chain of a surfel_refine runner issued call by call into a fresh map that holds a copy of every scan at
    its seed: pose_chain on scratch buffers, register, the state copy, insert.  -> (map, trajectory [n, 7], info)"""
    from rslo_amd import capi
    from rslo_amd.surfels import SurfelMap, check_surfel_refine
    smap = SurfelMap(**SURF_ARGS)
    kw = check_surfel_refine(SURF_REFINE_D, smap)
    assert kw["cost"] == "distribution" and kw["robust_scale"] == 3.0 and kw["iters"] == 3
    n = len(scans)
    for j in range(n):
        smap.insert(scans[j], seeds[j])
    state = torch.zeros(7, dtype=torch.float64, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    rel2 = torch.zeros((n, 7), dtype=torch.float32, device="cuda")
    traj = torch.zeros((n, 7), dtype=torch.float64, device="cuda")
    infos = []
    for i, s in enumerate(scans):
        capi.pose_chain(rel[i, :3], rel[i, 3:], state, count, rel2, traj)
        infos.append(smap.register(s, traj[i], **kw)[1])
        state.copy_(traj[i])
        smap.insert(s, traj[i])
    return smap, traj, torch.stack(infos)


def test_runner_refines_with_the_distribution_cost(odom):
    """tests/test_gpu_surfels.py::test_runner_refines_against_the_surfels with cost="distribution".  Copies of ALL the
    scans, scan 0 included, are seeded a few centimetres from where the chain will predict them before the stream
    starts, so that every scan finds a map: every row of the info is status 0."""
    from rslo_amd import capi, inference
    from rslo_amd.surfels import SurfelMap
    net, scans = odom
    for bad in (dict(cost="ndt"), dict(cost="distribution", min_flag=3), dict(reg_abs=0.01), dict(cost="distribution", lam=1)):
        with pytest.raises(capi.RsloHipError):
            inference.OdometryRunner(net, surfels=SurfelMap(**SURF_ARGS), surfel_refine=bad)
    smap = SurfelMap(**SURF_ARGS)
    runner = inference.OdometryRunner(net, surfels=smap, surfel_refine=SURF_REFINE_D)
    try:
        stream(runner, scans)
        rel = runner.relative().clone()
        info = runner.surfel_refine_info()
        assert info.shape == (N_SCANS, 3, 8) and info[0, :, 0].tolist() == [1.0] * 3      # scan 0 meets an empty table
        runner.reset()
        assert len(runner.refined_trajectory()) == 0 and set(smap.stats().values()) == {0}
        seeds = seed_poses(rel)
        for j in range(N_SCANS):
            smap.insert(scans[j], seeds[j])
        stream(runner, scans)
        assert same_bits(runner.relative(), rel)
        refined, info = runner.refined_trajectory(), runner.surfel_refine_info()
        print("seeded map: status\n%s\npairs\n%s\n|dt|\n%s" % tuple(info[:, :, k].cpu().numpy() for k in (0, 1, 3)))
        assert (info[:, :, 0] == 0).all() and (info[:, :, 1] > 10000).all()
        # scan 0 starts 6.7 cm from its copy; the later scans start where the REFINED chain predicts them, next to theirs
        assert info[0, 0, 3] > 1e-2 and (info[:, 0, 3] > 0).all()
        assert not torch.equal(refined, runner.trajectory())
        hand_map, hand_traj, hand_info = _by_hand(scans, rel, seeds)
        assert same_bits(refined, hand_traj) and same_bits(info, hand_info)
        assert same_device_maps(smap, hand_map) and smap.stats()["n_scans"] == 2 * N_SCANS
    finally:
        runner.close()


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_never_reset_allocation_and_argument_errors_d(drive):
    from rslo_amd import capi
    lib = capi.lib()
    smap = drive["smap"]
    N = 500
    pts, pose = dev(drive["raw"][:N]), dev(drive["start"])
    raw = torch.full((capi.surfel_bytes(1024) // 8,), SENTINEL, dtype=torch.int64, device="cuda")
    keys, d2, rows, info = capi.surfel_nearest_d(raw, pts, pose, 0.4, rows=True, info=True)      # never reset: "none"
    sums = capi.surfel_normal_eq_d(raw, pts, pose, 0.4, robust_scale=3.0)
    rinfo = capi.surfel_register_d(raw, pts, pose, 0.4, iters=2, robust_scale=3.0)
    torch.cuda.synchronize()
    assert bool((raw == SENTINEL).all()) and bool((keys == -1).all()) and bool((d2 == -1.0).all())
    assert not rows.any() and not info.any() and not sums.any()
    assert rinfo[:, 0].tolist() == [1.0, 1.0] and not rinfo[:, 1:].any() and same_bits(pose, dev(drive["start"]))
    before = smap._buf.clone()
    p, nbytes = smap._buf.data_ptr(), smap._buf.numel() * 8
    S = -7.0
    out = torch.full((29,), S, dtype=torch.float64, device="cuda")
    info = torch.full((33, 8), S, dtype=torch.float64, device="cuda")
    keys = torch.full((N,), -7, dtype=torch.int64, device="cuda")
    d2 = torch.full((N,), S, dtype=torch.float64, device="cuda")
    rows = torch.full((N, 8), S, dtype=torch.float64, device="cuda")
    inf8 = torch.full((N, 8), S, dtype=torch.float64, device="cuda")
    rws = torch.full((lib.rslo_surfel_register_ws_bytes(N) // 8,), -7, dtype=torch.int64, device="cuda")
    nan = float("nan")

    def nearest(md=0.4, mf=1, rr=0.01, ra=0.02, voxel=0.4, stride=4):
        return lib.rslo_surfel_nearest_d(p, nbytes, voxel, pts.data_ptr(), stride, N, pose.data_ptr(), md, mf, rr, ra,
                                         keys.data_ptr(), d2.data_ptr(), rows.data_ptr(), inf8.data_ptr(), None)

    def normal_eq(md=0.4, mf=1, rr=0.01, ra=0.02, scale=3.0, wsb=rws.numel() * 8, voxel=0.4):
        return lib.rslo_surfel_normal_eq_d(p, nbytes, voxel, pts.data_ptr(), 4, N, pose.data_ptr(), md, mf, rr, ra, scale,
                                           out.data_ptr(), rws.data_ptr(), wsb, None)

    def register(md=0.4, mf=1, rr=0.01, ra=0.02, iters=3, scale=3.0, tol=0.0, wsb=rws.numel() * 8):
        return lib.rslo_surfel_register_d(p, nbytes, 0.4, pts.data_ptr(), 4, N, pose.data_ptr(), iters, md, 0.0, 50, tol, tol,
                                          scale, mf, rr, ra, info.data_ptr(), rws.data_ptr(), wsb, None)
    inf = float("inf")
    rcs = [f(**kw) for f in (nearest, normal_eq, register)
           for kw in (dict(mf=0), dict(mf=3), dict(mf=-1), dict(rr=0.0, ra=0.0), dict(rr=-0.01), dict(ra=-0.02), dict(rr=nan),
                      dict(ra=nan), dict(rr=inf), dict(ra=inf), dict(md=0.41), dict(md=0.0), dict(md=-0.1), dict(md=nan))]
    rcs += [register(iters=0), register(iters=33), register(tol=nan), register(tol=-1.0)]
    rcs += [normal_eq(scale=-1.0), normal_eq(scale=nan), register(scale=1e200)]
    rcs += [normal_eq(wsb=256), register(wsb=16), nearest(voxel=nan), normal_eq(voxel=0.0), nearest(stride=2)]
    print("return codes:", rcs, lib.rslo_last_error().decode())
    assert all(rc != 0 for rc in rcs)
    torch.cuda.synchronize()
    assert (keys == -7).all() and (d2 == S).all() and (rows == S).all() and (inf8 == S).all()
    assert (out == S).all() and (info == S).all() and (rws == -7).all()
    assert torch.equal(before, smap._buf) and same_bits(pose, dev(drive["start"]))
    assert nearest() == 0 and normal_eq() == 0 and normal_eq(rr=0.0) == 0 and normal_eq(ra=0.0) == 0      # and the good calls run
    torch.cuda.synchronize()
    assert (keys != -7).all() and (out != S).all() and torch.equal(before, smap._buf)
    q = pts.contiguous()
    for kw in (dict(min_flag=0), dict(min_flag=3), dict(reg_rel=0.0, reg_abs=0.0), dict(reg_rel=-1.0), dict(reg_abs=nan)):
        for call in (smap.nearest, smap.normal_equations, smap.register):
            with pytest.raises(ValueError):
                call(q, pose, **D, **kw)
    for kw in (dict(min_flag=1), dict(reg_rel=0.01), dict(reg_abs=0.02)):      # the new options with cost="plane"
        for call in (smap.nearest, smap.normal_equations, smap.register):
            with pytest.raises(ValueError):
                call(q, pose, **kw)
    with pytest.raises(ValueError):
        smap.nearest(q, pose, return_info=True)
    assert same_bits(pose, dev(drive["start"]))
