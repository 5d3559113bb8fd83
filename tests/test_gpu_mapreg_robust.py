"""Coarse-to-fine robust scan-to-map registration on the GPU (csrc/mapreg.hip: rslo_map_normal_eq_w / _register_w /
_register_sched; VoxelMap robust_scale=, MapPyramid) against the float64 restatement (VoxelMapRef, MapPyramidRef) run on
the same fp32 inputs, and the runner's refined chain over a pyramid.

The bars are those of tests/test_gpu_mapreg.py and follow from the formats:
  * weighted normal equations: the pair count is exact; the weight of a point is a handful of IEEE operations on its
    own cost addend, so device and restatement hold the same weighted addends up to a last bit and differ in the order
    of the sum: each of the 28 sums is held to K * 2^-50 * sum|weighted addend| over the K addends of the restatement;
    two runs are bit-equal; scale 0 is the unweighted entry point to the bit;
  * one weighted Gauss-Newton step from the same pose: 1e4 * cond2(H_weighted) * 2^-52 * (1 + |t|);
  * a schedule is the same launches as its stages issued as separate register calls: BIT equality.
"""
import numpy as np
import pytest
import torch
from stream_support import bits, cond_of, dev, disturbed, odom_fixture, same_bits, seed_poses, stream, turned

pytestmark = pytest.mark.gpu

DRIVE_MAP = dict(voxel_size=0.4, min_range=2.5, max_range=80.0)
GATE = dict(min_range=2.5, max_range=80.0)
PYRAMID = (1.6, 0.8, 0.4)


@pytest.fixture(scope="module")
def drive():
    """The 16-beam drive of tests/test_gpu_mapreg.py, rebuilt here: scans 0 and 1 under their true poses in a map of
    voxel 0.4 (1 << 16 slots) and in a pyramid (1.6, 0.8, 0.4), device and restatement; scan 2 is registered.  Made
    once and never modified."""
    from rslo_amd import synthetic
    from rslo_amd.mapping import MapPyramid, MapPyramidRef, VoxelMap, VoxelMapRef
    scans = [synthetic.sequence_scan(i, seed=3, n_el=16, n_az=520) for i in range(3)]
    poses = [synthetic.sequence_pose(i, seed=3) for i in range(3)]
    ref = VoxelMapRef(**DRIVE_MAP)
    vmap = VoxelMap(capacity=1 << 16, **DRIVE_MAP)
    pref = MapPyramidRef(PYRAMID, **GATE)
    pyr = MapPyramid(PYRAMID, capacity=1 << 16, **GATE)
    for s, p in zip(scans[:2], poses[:2]):
        for m in (ref, pref):
            m.insert(s, p)
        for m in (vmap, pyr):
            m.insert(dev(s), p)
    axis = np.array([0.3, -0.4, 0.866])
    start = np.concatenate([poses[2][:3] + 0.1 * np.array([0.6, -0.5, 0.2]),
                            turned(poses[2][3:], np.deg2rad(0.15) * axis / np.linalg.norm(axis))])
    tiled = np.concatenate([scans[2] + np.array([0.01 * k, -0.01 * k, 0, 0, 0, 0, 0], np.float32) for k in range(9)])
    assert len(scans[2]) == 7374
    assert vmap.stats()["dropped_full"] == 0 and vmap.stats() == ref.stats()
    assert pyr.stats() == pref.stats() and all(st["dropped_full"] == 0 for st in pyr.stats())
    return dict(scans=scans, poses=poses, ref=ref, vmap=vmap, pref=pref, pyr=pyr, start=start, tiled=tiled,
                dev2=dev(scans[2]))


# ---------------------------------------------------------------------------------------------------------------------
# weighted normal equations
# ---------------------------------------------------------------------------------------------------------------------
def _check_sums(ref, vmap, pts, pose, metric, scale, label):
    terms = ref._weighted_terms(pts, pose, metric, robust_scale=scale)
    K = len(terms)
    want = ref.normal_equations(pts, pose, metric, robust_scale=scale)
    dpts, dpose = dev(pts), dev(pose)
    got = vmap.normal_equations(dpts, dpose, metric, robust_scale=scale).cpu().numpy()
    again = vmap.normal_equations(dpts, dpose, metric, robust_scale=scale).cpu().numpy()
    bound = K * 2.0 ** -50 * np.abs(terms).sum(axis=0)
    err = np.abs(got[:28] - want[:28])
    with np.errstate(all="ignore"):
        print("%s: %d pairs; worst |dev - ref| / bound %.3g" % (label, K, np.nanmax(np.where(bound > 0, err / bound, 0.0))))
    assert got.shape == (29,) and got[28] == K == want[28]
    assert np.isfinite(got).all()
    assert (err <= bound).all()
    assert got.tobytes() == again.tobytes()
    return got, K


@pytest.mark.parametrize("scale", [0.2, 0.05])
@pytest.mark.parametrize("metric", ["point", "plane"])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 1025, 7374, 66366])
def test_weighted_normal_equations(drive, N, metric, scale):
    src = drive["tiled"] if N > len(drive["scans"][2]) else drive["scans"][2]
    assert N <= len(src) and (N < 60000 or N > 256 * 256)      # the largest: more block partials than one 256-wide pass
    got, K = _check_sums(drive["ref"], drive["vmap"], src[:N], drive["start"], metric, scale,
                         "N %d %s scale %g" % (N, metric, scale))
    if N >= 1025:
        assert K > N // 2
        plain = drive["vmap"].normal_equations(dev(src[:N]), dev(drive["start"]), metric).cpu().numpy()
        assert got[27] < plain[27] and got[28] == plain[28]      # the weights lower the cost, not the count


@pytest.mark.parametrize("metric", ["point", "plane"])
@pytest.mark.parametrize("N", [257, 7374])
def test_scale_zero_is_the_unweighted_entry_point(drive, N, metric):
    from rslo_amd import capi
    vmap = drive["vmap"]
    pts, pose = dev(drive["scans"][2][:N]), dev(drive["start"])
    plain = capi.map_normal_eq(vmap._buf, pts, pose, 0.4, metric)                        # rslo_map_normal_eq
    zero = capi.map_normal_eq(vmap._buf, pts, pose, 0.4, metric, robust_scale=0.0)       # rslo_map_normal_eq_w, scale 0
    assert same_bits(plain, zero) and plain[28] > N // 2
    assert same_bits(vmap.normal_equations(pts, pose, metric, robust_scale=0.0), plain)
    a, b = pose.clone(), pose.clone()
    ia = capi.map_register(vmap._buf, pts, a, 0.4, 3, metric)                            # rslo_map_register
    ib = capi.map_register(vmap._buf, pts, b, 0.4, 3, metric, robust_scale=0.0)          # rslo_map_register_w, scale 0
    assert same_bits(a, b) and same_bits(ia, ib) and not same_bits(a, pose)


def test_nan_normal_and_vanishing_weight(drive):
    """A NaN normal makes its point a point term, as without weights.  A point whose e is so large against the scale
    that rho underflows to 0 adds zeros, not NaNs, beside points that keep their weight: a scan registered at the very
    pose it was inserted under meets its own rows, so the owner of a cell has e == 0 exactly (rho == 1) and every other
    point of the cell e > 0, which at scale 1e-150 gives u of about 1e-298 and rho == 0."""
    from rslo_amd.mapping import VoxelMap, VoxelMapRef
    ref, vmap = drive["ref"], drive["vmap"]
    pts = drive["scans"][2][:1025].copy()
    matched = np.nonzero(ref.nearest(pts, drive["start"])[0] >= 0)[0]
    pts[matched[3], 4] = np.nan
    pts[matched[5], 4:7] = np.nan
    got, K = _check_sums(ref, vmap, pts, drive["start"], "plane", 0.2, "NaN normals")
    assert K == len(matched)
    ident = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
    own_ref, own = VoxelMapRef(**DRIVE_MAP), VoxelMap(capacity=1 << 14, **DRIVE_MAP)
    own_ref.insert(pts, ident)
    own.insert(dev(pts), ident)
    n_cells = own.stats()["n_cells"]
    got, K = _check_sums(own_ref, own, pts, ident, "point", 1e-150, "own rows, scale 1e-150")
    assert n_cells < K and got[0] == float(n_cells)      # H(0, 0) of a point term is 1: only the owners count
    assert got[27] == 0.0 and not got[21:27].any()       # ... and their residual is zero
    got, K = _check_sums(own_ref, own, pts, ident, "plane", 1e-150, "own rows, plane, scale 1e-150")
    assert got[27] == 0.0 and got[:21].any()
    # every weight vanishes: sums of zeros, and still the count of pairs
    got, K = _check_sums(ref, vmap, pts, drive["start"], "plane", 1e-150, "scale 1e-150")
    assert K == len(matched) and not got[:28].any()


@pytest.mark.parametrize("metric,scale", [("plane", 0.2), ("point", 0.2), ("plane", 0.05)])
def test_weighted_step_teacher_forced(drive, metric, scale):
    """Six successive weighted iterations; both implementations start every one of them from the DEVICE's current pose."""
    ref, vmap, pts = drive["ref"], drive["vmap"], drive["scans"][2]
    pose = dev(drive["start"])
    worst = 0.0
    for it in range(6):
        cur = pose.cpu().numpy().copy()
        want, winfo = ref.register(pts, cur, iters=1, metric=metric, robust_scale=scale)
        out, info = vmap.register(drive["dev2"], pose, iters=1, metric=metric, robust_scale=scale)
        assert out is pose                           # in place
        got, info = pose.cpu().numpy(), info.cpu().numpy()
        assert info.shape == (1, 8) and info[0, 0] == winfo[0, 0] == 0.0 and info[0, 1] == winfo[0, 1]
        sums = ref.normal_equations(pts, cur, metric, robust_scale=scale)
        bound = 1e4 * cond_of(sums) * 2.0 ** -52 * (1.0 + np.linalg.norm(cur[:3]))
        err = np.abs(got - want).max()
        worst = max(worst, err / bound)
        print("%s scale %g iteration %d: step %.3e m, |dev - ref| %.3e, bound %.3e, pairs %d, cost %.4f" % (
            metric, scale, it, np.linalg.norm(got[:3] - cur[:3]), err, bound, info[0, 1], info[0, 2]))
        assert err <= bound
        assert abs(info[0, 3] - winfo[0, 3]) <= bound and abs(info[0, 4] - winfo[0, 4]) <= bound
        assert abs(info[0, 2] - sums[27]) <= info[0, 1] * 2.0 ** -50 * sums[27]      # the weighted cost (all addends >= 0)
    print("%s scale %g: largest |dev - ref| / bound over six steps %.3g" % (metric, scale, worst))


# ---------------------------------------------------------------------------------------------------------------------
# the schedule
# ---------------------------------------------------------------------------------------------------------------------
SCHED = [(0, 3, None, 0.0), (1, 2, 0.7, 0.4), (2, 3, None, 0.2)]


def test_schedule_equals_its_stages(drive):
    pyr, pts = drive["pyr"], drive["dev2"]
    start = disturbed(drive["poses"][2], 0.3, 0.5)
    before = [m._buf.clone() for m in pyr.levels]
    pose = dev(start)
    out, info = pyr.register(pts, pose, SCHED, metric="plane")
    assert out is pose and info.shape == (8, 8) and info.dtype == torch.float64
    hand = dev(start)
    rows = []
    for level, iters, md, scale in SCHED:
        rows.append(pyr.levels[level].register(pts, hand, iters=iters, metric="plane", max_dist=md, robust_scale=scale)[1])
    rows = torch.cat(rows)
    assert same_bits(pose, hand) and same_bits(info[:, :5], rows[:, :5])
    assert (info[:, 0] == 0).all() and (info[:, 1] > 1000).all()
    assert info[:, 5].tolist() == [0.0] * 3 + [1.0] * 2 + [2.0] * 3
    assert info[:, 6].tolist() == [0.0] * 3 + [1.0] * 2 + [2.0] * 3 and not info[:, 7].any()
    # the levels may come in any order and more than once
    sched = [(2, 1, None, 0.2), (0, 2, None, 0.0), (2, 2, 0.3, 0.1)]
    pose, hand = dev(start), dev(start)
    _, info = pyr.register(pts, pose, sched, metric="point")
    for level, iters, md, scale in sched:
        pyr.levels[level].register(pts, hand, iters=iters, metric="point", max_dist=md, robust_scale=scale)
    assert same_bits(pose, hand) and info[:, 6].tolist() == [2.0, 0.0, 0.0, 2.0, 2.0] and info[:, 5].tolist() == [0.0, 1.0, 1.0, 2.0, 2.0]
    # against the restatement: the device pyramid follows MapPyramidRef within what six teacher-free steps allow
    want, winfo = drive["pref"].register(drive["scans"][2], start, SCHED, metric="plane")
    pose = dev(start)
    _, info = pyr.register(pts, pose, SCHED, metric="plane")
    assert (info[:, 1].cpu().numpy() == winfo[:, 1]).all() and (info[:, 5:].cpu().numpy() == winfo[:, 5:]).all()
    assert np.abs(pose.cpu().numpy() - want).max() < 1e-6
    assert all(torch.equal(a, m._buf) for a, m in zip(before, pyr.levels))      # read-only on every level


def test_tolerance_skips_only_its_own_stage(drive):
    pyr, pts = drive["pyr"], drive["dev2"]
    start = disturbed(drive["poses"][2], 0.3, 0.5)
    sched = [(0, 3, None, 0.0), (1, 2, None, 0.4), (2, 2, None, 0.2)]
    pose = dev(start)
    _, info = pyr.register(pts, pose, sched, metric="plane", tol_t=10.0, tol_r=10.0)      # met by every first step
    assert info[:, 0].tolist() == [0.0, 3.0, 3.0, 0.0, 3.0, 0.0, 3.0]
    skipped = info[:, 0] == 3.0
    assert not info[skipped][:, 1:5].any()
    assert info[:, 5].tolist() == [0.0, 0.0, 0.0, 1.0, 1.0, 2.0, 2.0] and info[:, 6].tolist() == info[:, 5].tolist()
    hand = dev(start)
    for level, _, _, scale in sched:                 # one iteration per stage is what ran
        pyr.levels[level].register(pts, hand, iters=1, metric="plane", robust_scale=scale)
    assert same_bits(pose, hand)
    # a tolerance that is never met skips nothing, whatever the flag held before
    a, b = dev(start), dev(start)
    _, ia = pyr.register(pts, a, sched, metric="plane", tol_t=1e-30, tol_r=1e-30)
    _, ib = pyr.register(pts, b, sched, metric="plane")
    assert (ia[:, 0] == 0).all() and same_bits(a, b) and same_bits(ia, ib)


def _err(pose, true):
    return float(np.linalg.norm(pose.cpu().numpy()[:3] - true[:3]))


def test_basin_pyramid_without_weights(drive):
    pyr, pts, true = drive["pyr"], drive["dev2"], drive["poses"][2]
    start = disturbed(true, 1.00, 2.0)
    pose, info = pyr.register(pts, dev(start), [(0, 4, None, 0), (1, 4, None, 0), (2, 4, None, 0)], metric="plane")
    fine, _ = pyr.levels[2].register(pts, dev(start), iters=12, metric="plane")
    print("start 1.00 m, 2.0 deg: pyramid %.4f m, fine map alone %.4f m" % (_err(pose, true), _err(fine, true)))
    assert (info[:, 0] == 0).all()
    assert _err(pose, true) <= 0.05
    assert _err(fine, true) > 0.5


def test_basin_robust_schedule(drive):
    pyr, pts, true = drive["pyr"], drive["dev2"], drive["poses"][2]
    start = disturbed(true, 0.60, 1.0)
    pose, info = pyr.register(pts, dev(start), [(k, 4, None, 0.5 * v) for k, v in enumerate(PYRAMID)], metric="plane")
    fine, _ = pyr.levels[2].register(pts, dev(start), iters=12, metric="plane")
    print("start 0.60 m, 1.0 deg: robust pyramid %.4f m, fine map alone %.4f m" % (_err(pose, true), _err(fine, true)))
    assert (info[:, 0] == 0).all()
    assert _err(pose, true) <= 0.02
    assert _err(fine, true) > 0.05


def test_schedule_leaves_the_pose_alone(drive):
    from rslo_amd.mapping import MapPyramid
    pyr, pts = drive["pyr"], drive["dev2"]
    start = dev(drive["start"])
    bits = start.view(torch.int64).clone()
    sched = [(0, 2, None, 0.0), (2, 1, None, 0.2)]
    empty = MapPyramid(PYRAMID, capacity=1024, **GATE)
    pose, info = empty.register(pts, start, sched)
    assert info[:, 0].tolist() == [1.0] * 3 and info[:, 1].tolist() == [0.0] * 3 and torch.equal(pose.view(torch.int64), bits)
    assert info[:, 5].tolist() == [0.0, 0.0, 1.0] and info[:, 6].tolist() == [0.0, 0.0, 2.0]
    pose, info = pyr.register(pts[:0], start, sched)                                      # N = 0
    assert info[:, 0].tolist() == [1.0] * 3 and torch.equal(pose.view(torch.int64), bits)
    pose, info = pyr.register(pts, start, sched, min_pairs=10 ** 6)
    assert info[:, 0].tolist() == [1.0] * 3 and (info[:, 1] > 1000).all() and torch.equal(pose.view(torch.int64), bits)
    pose, info = pyr.register(pts, start, sched, damping=-1e30)                           # no stage is positive definite
    assert info[:, 0].tolist() == [2.0] * 3 and torch.equal(pose.view(torch.int64), bits)
    pose, info = drive["vmap"].register(pts, start, iters=2, robust_scale=0.2, damping=-1e30)
    assert info[:, 0].tolist() == [2.0, 2.0] and torch.equal(pose.view(torch.int64), bits)
    # a host pose is copied, not written
    host = drive["start"].copy()
    pose, _ = pyr.register(pts, host, sched)
    assert pose.is_cuda and host.tobytes() == drive["start"].tobytes() and not torch.equal(pose.view(torch.int64), bits)


def test_argument_errors_write_nothing(drive):
    import ctypes as C
    from rslo_amd import capi
    lib = capi.lib()
    vmap, pyr, pts = drive["vmap"], drive["pyr"], drive["dev2"]
    N = 500
    p, nbytes = vmap._buf.data_ptr(), vmap._buf.numel() * 8
    before = [m._buf.clone() for m in pyr.levels] + [vmap._buf.clone()]
    pose = dev(drive["start"])
    S = -7.0
    out = torch.full((29,), S, dtype=torch.float64, device="cuda")
    info = torch.full((65, 8), S, dtype=torch.float64, device="cuda")
    ws = torch.full((lib.rslo_map_register_ws_bytes(N) // 8,), -7, dtype=torch.int64, device="cuda")
    wsb = ws.numel() * 8
    nan, inf = float("nan"), float("inf")

    def normal_eq_w(scale, md=0.4, metric=1, wsb=wsb):
        return lib.rslo_map_normal_eq_w(p, nbytes, 0.4, pts.data_ptr(), 7, 7, N, pose.data_ptr(), metric, md, 1, scale,
                                        out.data_ptr(), ws.data_ptr(), wsb, None)

    def register_w(scale, md=0.4, iters=3, wsb=wsb):
        return lib.rslo_map_register_w(p, nbytes, 0.4, pts.data_ptr(), 7, 7, N, pose.data_ptr(), iters, 1, md, 1, 0.0, 50,
                                       0.0, 0.0, scale, info.data_ptr(), ws.data_ptr(), wsb, None)

    def sched(stages, n_levels=3, null_map=None, wsb=wsb, tol=0.0, metric=1):
        L = max(min(n_levels, 8), 1)
        bufs = [pyr.levels[min(k, 2)]._buf for k in range(L)]
        maps = (C.c_void_p * L)(*[None if k == null_map else b.data_ptr() for k, b in enumerate(bufs)])
        nb = (C.c_size_t * L)(*[b.numel() * 8 for b in bufs])
        vox = (C.c_double * L)(*[PYRAMID[min(k, 2)] for k in range(L)])
        flat = (C.c_double * (4 * len(stages)))(*[float(v) for st in stages for v in st])
        return lib.rslo_map_register_sched(maps, nb, vox, n_levels, flat, len(stages), pts.data_ptr(), 7, 7, N,
                                           pose.data_ptr(), metric, 1, 0.0, 50, tol, tol, info.data_ptr(), ws.data_ptr(), wsb,
                                           None)
    rcs = [f(scale) for f in (normal_eq_w, register_w) for scale in (-0.1, nan, inf, -inf, 1e-200, 1e200)]
    rcs += [f(0.2, md=md) for f in (normal_eq_w, register_w) for md in (0.41, 0.0, nan)]
    rcs += [register_w(0.2, iters=0), register_w(0.2, iters=33), normal_eq_w(0.2, metric=2)]
    ok = (0, 2, 1.6, 0.0)
    rcs += [sched([ok, (3, 2, 0.4, 0.0)]), sched([ok, (-1, 2, 0.4, 0.0)]), sched([ok, (0.5, 2, 0.4, 0.0)]),      # level
            sched([ok, (nan, 2, 0.4, 0.0)]),
            sched([ok, (1, 0, 0.8, 0.0)]), sched([ok, (1, -1, 0.8, 0.0)]), sched([ok, (1, 1.5, 0.8, 0.0)]),      # iters
            sched([(0, 33, 1.6, 0.0), (1, 32, 0.8, 0.0)]), sched([]),                                            # 65, none
            sched([ok, (2, 2, 0.41, 0.0)]), sched([ok, (2, 2, 0.0, 0.0)]), sched([ok, (2, 2, nan, 0.0)]),        # max_dist
            sched([ok, (2, 2, 0.4, -0.1)]), sched([ok, (2, 2, 0.4, nan)]), sched([ok, (2, 2, 0.4, inf)]),        # scale
            sched([ok], n_levels=0), sched([ok], n_levels=9), sched([ok], null_map=1),
            sched([ok], tol=nan), sched([ok], tol=-1.0), sched([ok], metric=2)]
    short = [normal_eq_w(0.2, wsb=wsb - 256), register_w(0.2, wsb=16), sched([ok], wsb=wsb - 256)]
    print("return codes:", rcs, short, lib.rslo_last_error().decode())
    assert all(rc == -1 for rc in rcs) and all(rc == -4 for rc in short)      # RSLO_EINVAL, RSLO_EWS
    torch.cuda.synchronize()
    assert (out == S).all() and (info == S).all() and (ws == -7).all()
    assert torch.equal(pose.cpu(), torch.from_numpy(drive["start"]))
    assert all(torch.equal(a, b._buf) for a, b in zip(before, pyr.levels + [vmap]))
    # the same calls with good arguments succeed (the errors above were the arguments')
    assert normal_eq_w(0.2) == 0 and register_w(0.2) == 0 and sched([ok, (2, 2, 0.4, 0.2)]) == 0
    torch.cuda.synchronize()
    assert (info[:4] != S).all() and (info[4:] == S).all()
    # the Python face refuses before anything is enqueued
    pose = dev(drive["start"])
    for bad in ([(3, 1, None, 0.0)], [(0, 0, None, 0.0)], [(2, 1, 0.41, 0.0)], [(0, 1, None, -1.0)], [(0, 1, None, nan)], []):
        with pytest.raises(ValueError):
            pyr.register(pts, pose, bad)
    for bad in (-0.1, nan, inf):
        with pytest.raises(ValueError):
            vmap.register(pts, pose, robust_scale=bad)
        with pytest.raises(ValueError):
            vmap.normal_equations(pts, pose, robust_scale=bad)
    with pytest.raises(TypeError):
        pyr.register(pts, pose, iters=3)
    assert torch.equal(pose.cpu(), torch.from_numpy(drive["start"]))


def test_capture_and_replay(drive):
    """One graph holding a three-stage MapPyramid.register over a static cloud, pose and info buffer; replayed for two
    scans it equals the eager calls: the stage state lives on the device and the schedule is baked into the launches."""
    pyr = drive["pyr"]
    n = min(len(drive["scans"][1]), len(drive["scans"][2]))
    clouds = [dev(drive["scans"][2][:n]), dev(drive["scans"][1][:n])]
    starts = [dev(disturbed(drive["poses"][2], 0.3, 0.5)), dev(disturbed(drive["poses"][1], 0.2, 0.3))]
    sched = [(0, 2, None, 0.0), (1, 3, None, 0.4), (2, 3, None, 0.2)]
    kw = dict(metric="plane", tol_t=0.004, tol_r=0.004)
    eager = []
    for c, s in zip(clouds, starts):
        pose = s.clone()
        _, info = pyr.register(c, pose, sched, **kw)      # (also the kernels' first launches)
        eager.append((pose, info))
    pyr.reserve(n)
    static_pts, static_pose = torch.zeros_like(clouds[0]), torch.zeros(7, dtype=torch.float64, device="cuda")
    static_info = torch.zeros((8, 8), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pyr.register(static_pts, static_pose, sched, info=static_info, **kw)
    assert not static_pose.any()                    # captured, not run
    for c, s, (pose, info) in zip(clouds, starts, eager):
        static_pts.copy_(c)
        static_pose.copy_(s)
        g.replay()
        assert same_bits(static_pose, pose) and same_bits(static_info, info)
        assert (static_info[:, 1][static_info[:, 0] == 0] > 1000).all() and static_info[0, 0] == 0.0
        assert not same_bits(static_pose, s)
    print("statuses of the replays' last scan:", static_info[:, 0].tolist())


# ---------------------------------------------------------------------------------------------------------------------
# the runner's refined chain over a pyramid
# ---------------------------------------------------------------------------------------------------------------------
N_SCANS = 3
IDENT = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
PYR_ARGS = dict(voxel_sizes=(0.8, 0.4, 0.2), capacity=1 << 21, min_range=2.5, max_range=80.0)
RUN_SCHED = [(0, 2, None, 0.0), (2, 2, None, 0.1)]


odom = odom_fixture(21, 3, N_SCANS)


def _replay_by_hand(scans, rel, seeds):
    """The refined chain issued call by call into a fresh pyramid: pose_chain on scratch buffers, register, the state
    copy, insert; the map is seeded behind scan 0.  -> (pyramid, trajectory [n, 7], info [n, rows, 8])"""
    from rslo_amd import capi
    from rslo_amd.mapping import MapPyramid
    pyr = MapPyramid(**PYR_ARGS)
    n = len(scans)
    state = torch.zeros(7, dtype=torch.float64, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    rel2 = torch.zeros((n, 7), dtype=torch.float32, device="cuda")
    traj = torch.zeros((n, 7), dtype=torch.float64, device="cuda")
    infos = []
    for i, s in enumerate(scans):
        capi.pose_chain(rel[i, :3], rel[i, 3:], state, count, rel2, traj)
        infos.append(pyr.register(s, traj[i], RUN_SCHED)[1])
        state.copy_(traj[i])
        pyr.insert(s, traj[i])
        if i == 0:
            for k in range(1, n):
                pyr.insert(scans[k], seeds[k])
    return pyr, traj, torch.stack(infos)


def _same_pyramid(a, b):
    return all(all(torch.equal(x, y) for x, y in zip(m.points(), w.points())) and m.stats() == w.stats()
               for m, w in zip(a.levels, b.levels))


def test_runner_refines_against_a_pyramid(odom):
    from rslo_amd import capi, inference
    from rslo_amd.mapping import MapPyramid, VoxelMap
    net, scans = odom
    plain = inference.OdometryRunner(net)
    try:
        rel0, traj0 = stream(plain, scans)
    finally:
        plain.close()
    single = VoxelMap(0.2, 1 << 21, min_range=2.5, max_range=80.0)
    with pytest.raises(capi.RsloHipError):
        inference.OdometryRunner(net, voxel_map=single, refine=dict(schedule=RUN_SCHED))      # a schedule needs a pyramid
    pyr = MapPyramid(**PYR_ARGS)
    with pytest.raises(capi.RsloHipError):
        inference.OdometryRunner(net, voxel_map=pyr, refine=dict(iters=3, schedule=RUN_SCHED))
    with pytest.raises(capi.RsloHipError):
        inference.OdometryRunner(net, voxel_map=pyr, refine=dict(schedule=[(5, 1, None, 0.0)]))
    runner = inference.OdometryRunner(net, voxel_map=pyr, refine=dict(schedule=RUN_SCHED))
    try:
        rel, traj = stream(runner, scans)
        assert rel.tobytes() == rel0.tobytes() and traj.tobytes() == traj0.tobytes()      # the open-loop chain is untouched
        refined, info = runner.refined_trajectory(), runner.refine_info()
        assert refined.shape == (N_SCANS, 7) and info.shape == (N_SCANS, 4, 8) and info.is_cuda
        assert refined[0].tolist() == IDENT.tolist() and info[0, :, 0].tolist() == [1.0] * 4      # scan 0 meets empty maps
        assert info[0, :, 5].tolist() == [0.0, 0.0, 1.0, 1.0] and info[0, :, 6].tolist() == [0.0, 0.0, 2.0, 2.0]
        assert all(st["n_scans"] == N_SCANS and st["dropped_full"] == 0 for st in pyr.stats())
        cells = [st["n_cells"] for st in pyr.stats()]
        assert cells[0] < cells[1] < cells[2]
        rel_dev = runner.relative().clone()
        runner.reset()                                  # a new sequence: both chains and every level restart
        assert len(runner.refined_trajectory()) == 0 and len(runner.refine_info()) == 0
        assert all(set(st.values()) == {0} for st in pyr.stats())
        # a seeded map, where the registration has pairs to work on, against the replay by hand
        seeds = seed_poses(rel_dev)
        runner.run(runner.submit(scans[0]))
        for k in range(1, N_SCANS):
            pyr.insert(scans[k], seeds[k])
        stream(runner, scans[1:])
        assert same_bits(runner.relative(), rel_dev)
        refined, info = runner.refined_trajectory(), runner.refine_info()
        print("seeded pyramid: status\n%s\npairs\n%s\n|dt|\n%s" % tuple(info[:, :, k].cpu().numpy() for k in (0, 1, 3)))
        assert (info[1:, :, 0] == 0).all() and (info[1:, :, 1] > 10000).all() and (info[1:, 0, 3] > 1e-3).all()
        hand_pyr, hand_traj, hand_info = _replay_by_hand(scans, rel_dev, seeds)
        assert same_bits(refined, hand_traj) and same_bits(info, hand_info)
        assert _same_pyramid(pyr, hand_pyr) and all(st["n_scans"] == 2 * N_SCANS - 1 for st in pyr.stats())
    finally:
        runner.close()
