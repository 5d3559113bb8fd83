"""Scan de-skewing on the GPU (csrc/deskew.hip, rslo_amd/deskew.py Deskewer) against the float64 restatement deskew_ref /
motion_ref run on the same fp32 inputs, and the de-skewing stage of an OdometryRunner.

The bars follow from the formats, not from what the kernel returns:
  * the rows: BIT equality.  Every operation of the per-point rule is an IEEE double +, -, *, / or floor on exactly
    converted fp32 inputs in one fixed order without contraction, sin, cos and atan are fixed polynomials, and the result
    is rounded to float once; numpy does the same operations in the same order.
  * the motion block: its one libm call is theta = 2 atan2(su, q0).  OpenCL bounds double atan2 at 6 ulp and glibc's is
    within 1, so the two angles may differ by 8 ulp at the most; motion_ref(theta=the device's bits) is then held to BIT
    equality in axis, t' and status, as everything behind the angle is again fixed-order double arithmetic.
"""
import numpy as np
import pytest
import torch
from stream_support import dev, odom_fixture, same_bits, stream
from test_deskew_host import AXIS, pose, rigid_cloud
from test_gpu_loops import quiet_collector

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1000, 65537]      # one thread per row, 256 per workgroup, the grid is not capped
REL = pose((1.1, -0.3, 0.08), AXIS, 0.21).astype(np.float32)
REL_NEG = (-2.5 * pose((0.9, 0.2, -0.05), (0.5, 0.1, 0.85), 0.4)).astype(np.float32)      # w < 0, |q| = 2.5; t = -2.5 (...)
PAIR = (pose((5, 2, -1), (0.1, 0.9, 0.2), 0.7), pose((5.9, 2.4, -1.1), (0.12, 0.88, 0.18), 0.78))
_CLOUD = {}


def cloud(n_cols):
    """65537 rows of n_cols columns with the rows the rule treats apart, and their times; made once, never modified"""
    if n_cols not in _CLOUD:
        pts = rigid_cloud(SIZES[-1], 11 + n_cols, cols=n_cols)
        times = np.random.default_rng(n_cols).uniform(-0.2, 1.2, len(pts)).astype(np.float32)
        if n_cols > 3:
            pts[40, 3] = np.nan                                   # a column that is copied keeps its bits
        for base in (0, 300):                                     # below 63 rows, and again in the second workgroup
            pts[base + 3, 0], pts[base + 4, 1], pts[base + 5, 2] = np.nan, np.inf, -np.inf
            times[base + 6], times[base + 7] = np.nan, np.inf
            pts[base + 8, :2] = 0.0
            pts[base + 9, 0], pts[base + 10, 1] = 0.0, 0.0        # on the axes
            pts[base + 11, :2], pts[base + 12, :2] = (-3.0, 0.0), (-3.0, -1e-30)      # either side of the default seam
        _CLOUD[n_cols] = (pts, times)
    return _CLOUD[n_cols]


def motion_args(source):
    """-> (keyword arguments for capi.deskew, the same for motion_ref)"""
    if source == "pair":
        return dict(pose_a=dev(PAIR[0]), pose_b=dev(PAIR[1])), dict(pose_a=PAIR[0], pose_b=PAIR[1])
    rel = {"rel7": REL, "neg": REL_NEG, None: None}[source]
    return (dict(rel7=dev(rel)), dict(rel7=rel)) if rel is not None else ({}, {})


def run_kernel(pts, times, source, n_cols, normal_col, in_pad=2, out_pad=5, inplace=False, **opts):
    """-> (out [N, n_cols] fp32, the whole output allocation, the motion block) on the host"""
    from rslo_amd import capi
    N = len(pts)
    big = torch.full((N, n_cols + in_pad), 3.5, dtype=torch.float32, device="cuda")
    big[:, :n_cols] = dev(pts)
    obig = big if inplace else torch.full((N, n_cols + out_pad), SENTINEL, dtype=torch.float32, device="cuda")
    motion = torch.full((8,), SENTINEL, dtype=torch.float64, device="cuda")
    capi.deskew(big[:, :n_cols], obig[:, :n_cols], None if times is None else dev(times), normal_col=normal_col,
                motion_out=motion, **motion_args(source)[0], **opts)
    torch.cuda.synchronize()
    whole = obig.cpu().numpy()
    return whole[:, :n_cols], whole, motion.cpu().numpy()


def reference(pts, times, source, normal_col, block, **opts):
    from rslo_amd import deskew
    mopts = {k: opts[k] for k in ("stamp", "max_angle") if k in opts}
    popts = {k: opts[k] for k in ("stamp", "az_start_turn", "az_clockwise") if k in opts}
    want_block = deskew.motion_ref(theta=block[3] if block[7] == 0.0 else None, **motion_args(source)[1], **mopts)
    return deskew.deskew_ref(pts, times, want_block, normal_col=normal_col, **popts), want_block


@pytest.mark.parametrize("n_cols,normal_col", [(3, -1), (4, -1), (7, -1), (7, 4)])
def test_rows_are_bit_equal_to_the_reference(n_cols, normal_col):
    pts, times = cloud(n_cols)
    cases = [(N, True, "rel7", {}) for N in SIZES] + [(N, False, "pair", {}) for N in SIZES]
    cases += [(257, True, "pair", dict(stamp=1.0)), (257, False, "neg", dict(stamp=0.0, az_start_turn=0.125, az_clockwise=True)),
              (1000, False, "rel7", dict(stamp=0.3, az_start_turn=0.0)), (1000, True, "neg", dict(max_angle=0.5))]
    moved = 0
    for N, timed, source, opts in cases:
        t = times[:N] if timed else None
        out, whole, block = run_kernel(pts[:N], t, source, n_cols, normal_col, **opts)
        want, want_block = reference(pts[:N], t, source, normal_col, block, **opts)
        label = "N %d, %s, %s, %r" % (N, "times" if timed else "azimuth", source, opts)
        assert block[7] == 0.0 and block.tobytes() == want_block.tobytes(), label
        assert out.tobytes() == want.tobytes(), label
        assert (whole[:, n_cols:] == SENTINEL).all(), label               # the padding of out is not written
        moved += int((out[:, :3] != pts[:N, :3]).any(1).sum())
    assert moved > 100000
    N = 1000                                                              # in place: out is points itself
    out, whole, block = run_kernel(pts[:N], times[:N], "rel7", n_cols, normal_col, inplace=True)
    want, _ = reference(pts[:N], times[:N], "rel7", normal_col, block)
    assert out.tobytes() == want.tobytes() and (whole[:, n_cols:] == 3.5).all()
    out, _, block = run_kernel(pts[:N], None, "pair", n_cols, normal_col, in_pad=0, out_pad=0)      # no padding at all
    assert out.tobytes() == reference(pts[:N], None, "pair", normal_col, block)[0].tobytes()


@pytest.mark.parametrize("source", ["rel7", "neg", "pair"])
def test_motion_block(source):
    from rslo_amd import deskew
    pts, _ = cloud(3)
    for stamp in (0.5, 0.0, 1.0):
        _, _, block = run_kernel(pts[:0], None, source, 3, -1, stamp=stamp)      # N == 0 still writes the block
        host = deskew.motion_ref(stamp=stamp, **motion_args(source)[1])
        ulps = abs(block[3] - host[3]) / np.spacing(host[3])
        print("%s, stamp %.1f: theta %.17g, %g ulp from the host's" % (source, stamp, block[3], ulps))
        assert block[7] == 0.0 and host[7] == 0.0 and ulps <= 8
        assert block.tobytes() == deskew.motion_ref(stamp=stamp, theta=block[3], **motion_args(source)[1]).tobytes()
        assert abs(np.linalg.norm(block[:3]) - 1.0) < 1e-15
    if source == "neg":                                 # negated and normalised: the motion of the unit quaternion with w > 0
        q = REL_NEG[3:].astype(np.float64)
        q = -q / np.linalg.norm(q)
        assert q[0] > 0 and abs(block[3] - 2 * np.arctan2(np.linalg.norm(q[1:]), q[0])) < 1e-14
        assert np.abs(block[:3] - q[1:] / np.linalg.norm(q[1:])).max() < 1e-14


def test_other_statuses_copy_every_row():
    pts, times = cloud(7)
    N = 1000
    zero_q = np.array([1, 0, 0, 0, 0, 0, 0], np.float32)
    nan_t = np.array([1, np.nan, 0, 1, 0, 0, 0], np.float32)
    inf_q = np.array([1, 0, 0, np.inf, 0, 0, 0], np.float32)
    from rslo_amd import capi

    def call(**kw):
        out = torch.full((N, 9), SENTINEL, dtype=torch.float32, device="cuda")
        motion = torch.full((8,), SENTINEL, dtype=torch.float64, device="cuda")
        capi.deskew(dev(pts[:N]), out[:, :7], normal_col=4, motion_out=motion, **kw)
        torch.cuda.synchronize()
        return out.cpu().numpy(), motion.cpu().numpy()
    for status, kw in ((1, {}), (2, dict(rel7=dev(zero_q))), (2, dict(rel7=dev(nan_t))), (2, dict(rel7=dev(inf_q))),
                       (3, dict(rel7=dev(REL), max_angle=0.2)),
                       (3, dict(pose_a=dev(PAIR[0]), pose_b=dev(PAIR[1]), max_angle=0.05))):
        for t in (dev(times[:N]), None):
            out, motion = call(times=t, **kw)
            assert motion.tolist() == [0.0] * 7 + [float(status)], (status, motion)
            assert out[:, :7].tobytes() == pts[:N].tobytes() and (out[:, 7:] == SENTINEL).all(), status


def test_argument_errors_write_nothing():
    from rslo_amd import capi
    lib = capi.lib()
    N = 100
    pts = dev(cloud(7)[0][:N])
    out = torch.full((N, 7), SENTINEL, dtype=torch.float32, device="cuda")
    motion = torch.full((8,), SENTINEL, dtype=torch.float64, device="cuda")
    rel, A, B = dev(REL), dev(PAIR[0]), dev(PAIR[1])
    good = dict(points=pts.data_ptr(), stride=7, N=N, n_cols=7, normal_col=4, times=None, rel7=rel.data_ptr(), pose_a=None,
                pose_b=None, stamp=0.5, start=-0.5, cw=0, max_angle=np.pi / 2, out=out.data_ptr(), out_stride=7)
    bad = [dict(points=None), dict(out=None), dict(N=-1), dict(n_cols=2), dict(n_cols=8), dict(n_cols=7, out_stride=6),
           dict(stride=6), dict(normal_col=2), dict(normal_col=5), dict(normal_col=-2), dict(normal_col=0),
           dict(stamp=-0.01), dict(stamp=1.01), dict(stamp=float("nan")), dict(max_angle=0.0), dict(max_angle=-1.0),
           dict(max_angle=1.5707963267948968), dict(max_angle=float("nan")), dict(max_angle=float("inf")),
           dict(start=float("inf")), dict(start=float("nan")), dict(pose_a=A.data_ptr(), pose_b=B.data_ptr()),
           dict(rel7=None, pose_a=A.data_ptr()), dict(rel7=None, pose_b=B.data_ptr()), dict(pose_b=B.data_ptr())]
    for change in bad:
        a = dict(good, **change)
        rc = lib.rslo_deskew(a["points"], a["stride"], a["N"], a["n_cols"], a["normal_col"], a["times"], a["rel7"], a["pose_a"],
                             a["pose_b"], a["stamp"], a["start"], a["cw"], a["max_angle"], a["out"], a["out_stride"],
                             motion.data_ptr(), None)
        assert rc == -1 and lib.rslo_last_error(), change         # RSLO_EINVAL
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (motion == SENTINEL).all()
    a = good                                                      # the same call with nothing changed is accepted
    assert lib.rslo_deskew(a["points"], a["stride"], a["N"], a["n_cols"], a["normal_col"], a["times"], a["rel7"], a["pose_a"],
                           a["pose_b"], a["stamp"], a["start"], a["cw"], a["max_angle"], a["out"], a["out_stride"],
                           motion.data_ptr(), None) == 0
    assert lib.rslo_deskew(None, 7, 0, 7, 4, None, None, None, None, 0.5, -0.5, 0, 1.0, None, 7, None, None) == 0
    torch.cuda.synchronize()
    assert motion[7] == 0 and not (out == SENTINEL).any()
    with pytest.raises(capi.RsloHipError):
        capi.deskew(pts, out[:50])
    with pytest.raises(capi.RsloHipError):
        capi.deskew(pts, out, times=torch.zeros(N + 1, device="cuda"))
    with pytest.raises(capi.RsloHipError):
        capi.deskew(pts.cpu(), out)


def test_two_calls_give_the_same_bits():
    from rslo_amd.deskew import Deskewer
    pts, times = cloud(7)
    stage, other = Deskewer(len(pts), 7), Deskewer(len(pts), 7)
    assert stage.normal_col == 4 and Deskewer(8, 4).normal_col == -1
    a = stage(dev(pts), rel7=dev(REL))
    b = other(dev(pts), rel7=dev(REL))
    assert a.shape == pts.shape and a.data_ptr() == stage.out.data_ptr()
    assert same_bits(a, b) and same_bits(stage.motion, other.motion) and stage.motion[7] == 0
    first = a.clone()
    assert same_bits(stage(dev(pts), rel7=dev(REL)), first)
    timed = Deskewer(len(pts), 7, times="input", stamp=1.0)
    from rslo_amd import capi
    with pytest.raises(capi.RsloHipError):
        timed(dev(pts))                                           # times="input" without times
    with pytest.raises(capi.RsloHipError):
        stage(dev(pts), dev(times))                               # times under "azimuth"
    with pytest.raises(capi.RsloHipError):
        stage(dev(pts[:, :4]))
    with pytest.raises(ValueError, match="stamp"):
        Deskewer(8, 7, stamp=2.0)
    out = timed(dev(pts[:1000]), dev(times[:1000]), pose_a=dev(PAIR[0]), pose_b=dev(PAIR[1]))
    want, _ = reference(pts[:1000], times[:1000], "pair", 4, timed.motion.cpu().numpy(), stamp=1.0)
    assert out.cpu().numpy().tobytes() == want.tobytes()


def test_capture_and_replay():
    """The motion is read when the kernel runs: one captured call, replayed under two motions, follows both."""
    from rslo_amd import deskew
    pts, _ = cloud(7)
    N = 1000
    stage = deskew.Deskewer(N, 7)
    static_pts, static_rel = dev(pts[:N]), dev(REL)
    stage(static_pts, rel7=static_rel)                            # the kernel's first launch, outside the capture
    stage.out.zero_()
    stage.motion.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with quiet_collector(), torch.cuda.graph(g):
        stage(static_pts, rel7=static_rel)
    assert not stage.out.any()                                    # captured, not run
    for rel in (REL, REL_NEG):
        static_rel.copy_(dev(rel))
        g.replay()
        torch.cuda.synchronize()
        block = stage.motion.cpu().numpy()
        want_block = deskew.motion_ref(rel7=rel, theta=block[3])
        assert block[7] == 0 and block.tobytes() == want_block.tobytes()
        assert stage.out.cpu().numpy().tobytes() == deskew.deskew_ref(pts[:N], None, want_block, normal_col=4).tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# the runner
# ---------------------------------------------------------------------------------------------------------------------
N_SCANS = 5
SURF_ARGS = dict(voxel_size=0.4, capacity=1 << 18, min_range=2.5, max_range=80.0)
odom = odom_fixture(21, 3, N_SCANS)


def cells(smap):
    return tuple(t.cpu().numpy() for t in smap.cells(0))


def test_runner_with_times_at_the_stamp_changes_nothing(odom):
    """times == stamp: every point keeps its position, so the maps the back end builds are those of a plain runner."""
    from rslo_amd import capi, inference
    from rslo_amd.surfels import SurfelMap
    net, scans = odom
    plain_map, smap = SurfelMap(**SURF_ARGS), SurfelMap(**SURF_ARGS)
    plain = inference.OdometryRunner(net, surfels=plain_map)
    try:
        rel0, traj0 = stream(plain, scans)
        with pytest.raises(capi.RsloHipError):
            plain.deskew_info()
        with pytest.raises(capi.RsloHipError):
            plain.deskewed()
        with pytest.raises(capi.RsloHipError):
            plain.submit(scans[0], torch.zeros(len(scans[0]), device="cuda"))      # times without deskew
    finally:
        plain.close()
    runner = inference.OdometryRunner(net, surfels=smap, deskew=dict(times="input", stamp=0.25))
    try:
        with pytest.raises(capi.RsloHipError):
            runner.deskewed()
        with pytest.raises(capi.RsloHipError):
            runner.submit(scans[0])                                                # times missing under "input"
        with pytest.raises(capi.RsloHipError):
            runner.feed(scans, [None] * (N_SCANS - 1))
        before = [s.clone() for s in scans]
        runner.feed(scans, [torch.full((len(s),), 0.25, device="cuda") for s in scans])
        torch.cuda.synchronize()
        assert runner.relative().cpu().numpy().tobytes() == rel0.tobytes()
        assert runner.trajectory().cpu().numpy().tobytes() == traj0.tobytes()
        assert all(same_bits(a, b) for a, b in zip(scans, before))                 # the caller's tensors are not written
        got, want = cells(smap), cells(plain_map)
        assert len(want[0]) > 1000 and got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        assert smap.stats() == plain_map.stats()
        info = runner.deskew_info().cpu().numpy()
        print("statuses %s" % info[:, 7])
        assert info.shape == (N_SCANS, 8) and info[0].tolist() == [0.0] * 7 + [1.0]
        assert same_bits(runner.deskewed()[:, :4], scans[-1][:, :4])
        runner.reset()
        assert len(runner.deskew_info()) == 0
    finally:
        runner.close()


def test_runner_deskews_with_the_network_motion(odom):
    from rslo_amd import capi, deskew, inference
    net, scans = odom
    for bad in (dict(motion="refined"), dict(stamps=0.5), dict(max_angle=2.0), dict(times="column")):
        with pytest.raises(capi.RsloHipError):
            inference.OdometryRunner(net, deskew=bad)
    plain = inference.OdometryRunner(net)
    try:
        rel0, traj0 = stream(plain, scans)
    finally:
        plain.close()
    runner = inference.OdometryRunner(net, deskew={})
    try:
        with pytest.raises(capi.RsloHipError):
            runner.submit(scans[0], torch.zeros(len(scans[0]), device="cuda"))     # a times tensor under "azimuth"
        rel, traj = stream(runner, scans)
        assert rel.tobytes() == rel0.tobytes() and traj.tobytes() == traj0.tobytes()
        info = runner.deskew_info().cpu().numpy()
        print("statuses %s, angles %s" % (info[:, 7], info[:, 3]))
        assert info[0].tolist() == [0.0] * 7 + [1.0]
        for n in range(1, N_SCANS):
            want = deskew.motion_ref(rel7=rel[n], theta=info[n, 3] if info[n, 7] == 0 else None)
            assert info[n].tobytes() == want.tobytes(), n
        last = scans[-1].cpu().numpy()
        got = runner.deskewed().cpu().numpy()
        assert got.tobytes() == deskew.deskew_ref(last, None, info[-1], normal_col=4).tobytes()
        assert (got.tobytes() != last.tobytes()) == bool(info[-1, 7] == 0)
    finally:
        runner.close()


def test_runner_deskews_with_the_refined_motion(odom):
    from rslo_amd import deskew, inference
    from rslo_amd.surfels import SurfelMap
    net, scans = odom
    runner = inference.OdometryRunner(net, surfels=SurfelMap(**SURF_ARGS), surfel_refine=dict(iters=2),
                                      deskew=dict(motion="refined", stamp=1.0))
    try:
        stream(runner, scans)
        info = runner.deskew_info().cpu().numpy()
        refined = runner.refined_trajectory().cpu().numpy()
        print("statuses %s, angles %s" % (info[:, 7], info[:, 3]))
        assert info[0].tolist() == [0.0] * 7 + [1.0] and info[1].tolist() == [0.0] * 7 + [1.0]
        for n in range(2, N_SCANS):
            want = deskew.motion_ref(pose_a=refined[n - 2], pose_b=refined[n - 1], stamp=1.0,
                                     theta=info[n, 3] if info[n, 7] == 0 else None)
            assert info[n].tobytes() == want.tobytes(), n
        got = runner.deskewed().cpu().numpy()
        assert got.tobytes() == deskew.deskew_ref(scans[-1].cpu().numpy(), None, info[-1], stamp=1.0, normal_col=4).tobytes()
    finally:
        runner.close()
