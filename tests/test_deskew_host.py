"""The float64 restatement of scan de-skewing (rslo_amd/deskew.py) on its own: the accuracy of its fixed polynomials
against numpy, its convention against the pose algebra of rslo_amd/se3.py, the round trip through skew_ref, and the rows
it must leave alone.  No GPU: tests/test_gpu_deskew.py holds the kernel to these functions bit for bit.

Bounds.  sin_poly / cos_poly: 2^-52 on [-pi/4, pi/4] (measured 2^-53, one rounding of a result below 1).  atan_poly: the
published 2e-8 rad of Abramowitz & Stegun 4.4.49 (measured 1.36e-8).  Round trip: the skewed cloud is rounded to fp32
(half an ulp per coordinate, sqrt(3)/2 ulp as a vector), the map back preserves norms, and the store rounds once more
(half an ulp): (sqrt(3)/2 + 1/2) ulp < 2 ulp of the largest input coordinate (measured 1.02)."""
import numpy as np
import pytest

from rslo_amd import deskew, se3

AXIS = np.array([0.2, -0.3, 0.933])


def quat(axis, theta):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return np.concatenate([[np.cos(theta / 2)], np.sin(theta / 2) * a])


def pose(t, axis, theta):
    return np.concatenate([np.asarray(t, np.float64), quat(axis, theta)])


def rigid_cloud(n, seed, cols=3):
    r = np.random.default_rng(seed)
    pts = np.zeros((n, cols), np.float32)
    pts[:, :3] = r.uniform(-1, 1, (n, 3)) * (80.0, 80.0, 5.0)
    if cols > 3:
        pts[:, 3] = r.random(n)
    if cols >= 7:
        nrm = r.normal(size=(n, 3))
        pts[:, 4:7] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    if cols > 7:
        pts[:, 7:] = r.normal(size=(n, cols - 7))
    return pts


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_sin_and_cos_polynomials_against_numpy():
    x = np.linspace(-np.pi / 4, np.pi / 4, 2000001)
    es, ec = np.abs(deskew.sin_poly(x) - np.sin(x)).max(), np.abs(deskew.cos_poly(x) - np.cos(x)).max()
    print("sin_poly %.3g  cos_poly %.3g  (2^-53 = %.3g)" % (es, ec, 2.0 ** -53))
    assert es <= 2.0 ** -52 and ec <= 2.0 ** -52
    assert deskew.sin_poly(0.0) == 0.0 and deskew.cos_poly(0.0) == 1.0


def test_atan_polynomial_against_numpy():
    r = np.linspace(0.0, 1.0, 2000001)
    e = np.abs(deskew.atan_poly(r) - np.arctan(r)).max()
    print("atan_poly %.3g rad" % e)
    assert e <= 2e-8


def test_sweep_fraction_against_arctan2():
    r = np.random.default_rng(0)
    xy = (r.normal(size=(1000000, 2)) * 40.0).astype(np.float32)
    xy[:5] = [(3, 0), (0, 3), (-3, 0), (0, -3), (2, 2)]
    for start, cw in ((-0.5, False), (0.125, False), (-0.5, True), (0.3, True)):
        got = deskew.sweep_fraction_ref(xy, start, cw)
        assert got.shape == (len(xy),) and (got >= 0).all() and (got <= 1).all()
        f = np.arctan2(xy[:, 1].astype(np.float64), xy[:, 0].astype(np.float64)) / (2 * np.pi) - start
        d = np.abs(got - (-f if cw else f))
        d = np.abs(d - np.round(d))                 # circular distance in turns
        print("start %r clockwise %r: %.3g of a turn" % (start, cw, d.max()))
        assert d.max() <= 2e-8 / (2 * np.pi)


def test_axis_directions_give_exact_quarters():
    xy = np.array([(1, 0), (0, 1), (0, -1), (-1, 0)], np.float32)
    assert deskew.sweep_fraction_ref(xy, -0.5, False).tolist() == [0.5, 0.75, 0.25, 0.0]
    assert deskew.sweep_fraction_ref(xy, -0.5, True).tolist() == [0.5, 0.25, 0.75, 0.0]
    assert deskew.sweep_fraction_ref(7.5 * xy, -0.5, False).tolist() == [0.5, 0.75, 0.25, 0.0]
    assert np.isnan(deskew.sweep_fraction_ref(np.zeros((1, 2), np.float32))).all()


@pytest.mark.parametrize("source", ["rel7", "pair"])
def test_convention_against_the_pose_algebra(source):
    """stamp = 1, s = 0: the point is moved by inverse(M); stamp = 0, s = 1: by M."""
    pts = rigid_cloud(1000, 1)
    p64 = pts.astype(np.float64)
    if source == "rel7":
        rel = pose((1.1, -0.2, 0.05), AXIS, 0.2).astype(np.float32)
        kw = dict(rel7=rel)
        M = rel.astype(np.float64)
        M[3:] /= np.linalg.norm(M[3:])
    else:
        A, B = pose((5, 2, -1), (0.1, 0.9, 0.2), 0.7), pose((5.9, 2.4, -1.1), (0.3, 0.8, -0.1), 0.9)
        kw = dict(pose_a=A, pose_b=B)
        M = se3.between(A, B)
        blk = deskew.motion_ref(stamp=0.0, **kw)
        assert blk[7] == 0.0 and np.abs(blk[4:7] - M[:3]).max() == 0.0          # stamp 0: t' = rotate(identity, t) = t
        th = 2.0 * np.arctan2(np.linalg.norm(M[4:]), M[3])
        assert abs(blk[3] - th) < 1e-14 and np.abs(blk[:3] * np.sin(th / 2) - M[4:]).max() < 1e-14
    Mi = se3.inverse(M)
    zeros, ones = np.zeros(len(pts), np.float32), np.ones(len(pts), np.float32)
    back = deskew.deskew_ref(pts, zeros, deskew.motion_ref(stamp=1.0, **kw), stamp=1.0, store=False)
    want = Mi[:3] + se3.rotate(Mi[3:], p64)
    assert np.abs(back - want).max() < 1e-12
    fwd = deskew.deskew_ref(pts, ones, deskew.motion_ref(stamp=0.0, **kw), stamp=0.0, store=False)
    want = M[:3] + se3.rotate(M[3:], p64)
    assert np.abs(fwd - want).max() < 1e-12
    # the middle of the sweep: the start moves by the inverse of half the motion, the end by half the motion
    qh = quat(M[4:], np.arctan2(np.linalg.norm(M[4:]), M[3]))      # half the rotation
    for s, q in ((ones, qh), (zeros, se3.qconj(qh))):
        mid = deskew.deskew_ref(pts, s, deskew.motion_ref(stamp=0.5, **kw), stamp=0.5, store=False)
        sign = 0.5 if s is ones else -0.5
        assert np.abs(mid - (sign * se3.rotate(se3.qconj(qh), M[:3]) + se3.rotate(q, p64))).max() < 1e-12


def test_motion_block_normalises_and_negates():
    rel = pose((1.0, 0.1, 0.0), AXIS, 0.25)
    want = deskew.motion_ref(rel7=rel.astype(np.float32), stamp=0.5)
    assert want[7] == 0.0 and abs(want[3] - 0.25) < 1e-7 and abs(np.linalg.norm(want[:3]) - 1.0) < 1e-15
    neg = rel.copy()
    neg[3:] = -neg[3:]
    assert deskew.motion_ref(rel7=neg.astype(np.float32), stamp=0.5).tobytes() == want.tobytes()
    big = rel.copy()
    big[3:] *= 4.0                                      # a power of two: the normalised quaternion has the same bits
    assert deskew.motion_ref(rel7=big.astype(np.float32), stamp=0.5).tobytes() == want.tobytes()
    ident = deskew.motion_ref(rel7=np.array([0.5, 0, 0, 1, 0, 0, 0], np.float32), stamp=0.5)
    assert ident.tolist() == [0, 0, 0, 0, 0.5, 0, 0, 0]
    assert deskew.motion_ref(rel7=rel.astype(np.float32), theta=0.125)[3] == 0.125
    with pytest.raises(ValueError):
        deskew.motion_ref(rel7=rel, pose_a=rel, pose_b=rel)
    with pytest.raises(ValueError):
        deskew.motion_ref(pose_a=rel)


def test_round_trip_through_skew_ref():
    n = 200000
    pts = rigid_cloud(n, 2)
    times = np.random.default_rng(3).random(n).astype(np.float32)
    rel = pose((3.0, 0.2, -0.1), AXIS, 0.3).astype(np.float32)
    for stamp in (0.5, 1.0):
        blk = deskew.motion_ref(rel7=rel, stamp=stamp)
        skewed = deskew.skew_ref(pts, times, blk, stamp=stamp).astype(np.float32)
        assert np.abs(skewed - pts).max() > 1.0         # metres of skew
        back = deskew.deskew_ref(skewed, times, blk, stamp=stamp)
        ulp = np.spacing(np.float32(np.abs(pts).max()))
        err = np.abs(back.astype(np.float64) - pts.astype(np.float64)).max() / ulp
        print("stamp %.1f: round trip %.3f ulp of the largest coordinate" % (stamp, err))
        assert err <= 2.0


def test_round_trip_with_azimuth_times():
    """skew_ref(times=None) dates a return by the azimuth at which it is recorded, so de-skewing by azimuth undoes it."""
    pts = rigid_cloud(20000, 4)
    pts = pts[np.hypot(pts[:, 0], pts[:, 1]) > 3.0]
    blk = deskew.motion_ref(rel7=pose((1.0, 0.05, 0.0), (0, 0, 1), 0.007).astype(np.float32))
    skewed = deskew.skew_ref(pts, None, blk, iters=6).astype(np.float32)
    back = deskew.deskew_ref(skewed, None, blk)
    far = np.abs(np.abs(deskew.sweep_fraction_ref(pts[:, :2]) - 0.5) - 0.5) > 0.01       # not astride the sweep's seam
    assert far.sum() > 0.9 * len(pts) and np.abs(skewed - pts)[far].max() > 0.3
    assert np.abs(back - pts)[far].max() < 1e-4


def test_statuses_copy_every_row():
    pts = rigid_cloud(5000, 5, cols=9)
    pts[7, 8] = np.nan
    pts[9, 1] = -0.0
    times = np.random.default_rng(6).random(len(pts)).astype(np.float32)
    rel = pose((1.0, 0.0, 0.0), AXIS, 0.5).astype(np.float32)
    blocks = {1: deskew.motion_ref(), 3: deskew.motion_ref(rel7=rel, max_angle=0.4),
              2: deskew.motion_ref(rel7=np.array([1, 0, 0, 0, 0, 0, 0], np.float32))}
    blocks["nan t"] = deskew.motion_ref(rel7=np.array([1, np.nan, 0, 1, 0, 0, 0], np.float32))
    blocks["inf q"] = deskew.motion_ref(pose_a=pose((0, 0, 0), AXIS, 0.1), pose_b=np.array([0, 0, 0, np.inf, 0, 0, 0]))
    for name, blk in blocks.items():
        assert blk[7] == (name if isinstance(name, int) else 2) and not blk[:7].any(), name
        for t in (times, None):
            out = deskew.deskew_ref(pts, t, blk, normal_col=4)
            assert out.dtype == np.float32 and out.tobytes() == pts.tobytes(), name
    assert deskew.deskew_ref(pts, times, None, normal_col=4).tobytes() == pts.tobytes()
    assert deskew.motion_ref(rel7=rel, max_angle=0.5000001)[7] == 0.0


def test_times_at_the_stamp_keep_the_positions():
    pts = rigid_cloud(5000, 7, cols=7)
    blk = deskew.motion_ref(rel7=pose((2.0, -1.0, 0.3), AXIS, 0.9).astype(np.float32), stamp=0.25)
    out = deskew.deskew_ref(pts, np.full(len(pts), 0.25, np.float32), blk, stamp=0.25, normal_col=4)
    assert (bits(out[:, :3]) == bits(pts[:, :3])).all() and (bits(out[:, 3]) == bits(pts[:, 3])).all()


def test_rows_that_are_left_alone_and_columns_that_are_kept():
    pts = rigid_cloud(4000, 8, cols=9)
    times = np.random.default_rng(9).uniform(-0.5, 1.5, len(pts)).astype(np.float32)
    pts[3, 0], pts[4, 1], pts[5, 2] = np.nan, np.inf, -np.inf
    times[6], times[7] = np.nan, np.inf
    pts[8, :2] = 0.0
    blk = deskew.motion_ref(rel7=pose((1.5, 0.3, -0.2), AXIS, 0.4).astype(np.float32))
    out = deskew.deskew_ref(pts, times, blk, normal_col=4)
    for i in range(3, 8):
        assert out[i].tobytes() == pts[i].tobytes(), i
    moved = np.ones(len(pts), bool)
    moved[3:8] = False
    assert (np.abs(out[moved, :3] - pts[moved, :3]).max(1) > 0).mean() > 0.99 and (out[8, :3] != pts[8, :3]).any()
    assert (bits(out[:, 3]) == bits(pts[:, 3])).all() and (bits(out[:, 7:]) == bits(pts[:, 7:])).all()
    assert np.abs(np.linalg.norm(out[moved, 4:7].astype(np.float64), axis=1) - 1.0).max() <= 4 * 2.0 ** -24
    assert (out[moved, 4:7] != pts[moved, 4:7]).any()
    plain = deskew.deskew_ref(pts, times, blk)                      # no normal column: columns 4..6 are data
    assert (bits(plain[:, 3:]) == bits(pts[:, 3:])).all() and (bits(plain[:, :3]) == bits(out[:, :3])).all()
    clamped = deskew.deskew_ref(pts, np.clip(times, 0.0, 1.0), blk, normal_col=4)      # times outside [0, 1] clamp
    assert clamped[moved].tobytes() == out[moved].tobytes() and (times[moved] < 0).any() and (times[moved] > 1).any()
    az = deskew.deskew_ref(pts, None, blk, normal_col=4)            # azimuth mode: x == y == 0 has no azimuth
    assert az[8].tobytes() == pts[8].tobytes() and az[3].tobytes() == pts[3].tobytes()
    assert out.shape == pts.shape and deskew.deskew_ref(pts[:0], None, blk).shape == (0, 9)


def test_check_deskew_names_the_key():
    d = deskew.check_deskew({})
    assert d == dict(motion="network", times="azimuth", stamp=0.5, az_start_turn=-0.5, az_clockwise=False,
                     max_angle=np.pi / 2)
    assert deskew.check_deskew(dict(motion="refined", times="input", stamp=1, az_clockwise=True))["stamp"] == 1.0
    bad = [("motion", "imu"), ("motion", None), ("times", "column"), ("stamp", -0.1), ("stamp", 1.5), ("stamp", float("nan")),
           ("stamp", "mid"), ("az_start_turn", float("inf")), ("az_start_turn", float("nan")), ("az_clockwise", 1),
           ("az_clockwise", "yes"), ("max_angle", 0.0), ("max_angle", 1.6), ("max_angle", float("nan")), ("max_angle", -1.0)]
    for key, value in bad:
        with pytest.raises(ValueError, match=key):
            deskew.check_deskew({key: value})
    with pytest.raises(ValueError, match="stamps"):
        deskew.check_deskew(dict(stamps=0.5))
