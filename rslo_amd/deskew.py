"""Scan de-skewing: motion-compensate a LiDAR sweep before it is registered, mapped or described.

    dk = Deskewer(point_capacity=160000, n_cols=7)              # owns the output buffer and an [8] motion block
    flat = dk(scan, rel7=rel)                                   # fp32 CUDA [P, 7] -> a [P, 7] view of the buffer
    flat = dk(scan, pose_a=refined[n - 2], pose_b=refined[n - 1])
    runner = inference.OdometryRunner(net, surfels=smap, deskew=dict(motion="network"))

A spinning LiDAR does not take a rigid snapshot: while the sweep lasts the sensor moves by M = (t, q).  Under the
constant-velocity model of LOAM / LIO-SAM the sensor pose at sweep fraction s in [0, 1] is (s t, R^s); de-skewing moves
every point from the sensor frame at its own time to the sensor frame at `stamp` (0.5, the middle of the sweep, as in
KISS-ICP).  With stamp = 1 a point seen at s = 0 is moved by M^-1; with stamp = 0 a point seen at s = 1 by M.

Deskewer is the device stage (csrc/deskew.hip, rules in include/rslo_hip.h "Scan de-skewing"): one launch per scan, no
host read, nothing allocated after construction.  The functions below restate the same rules in numpy float64, operation
by operation, and are the arbiter of the tests: given the device's angle (the one libm call, theta = 2 atan2(su, q0)),
the output is compared bit for bit.  The rules in one place:

  * motion block (motion_ref): M = rel7 widened, or se3.between(A, B); q is normalised and negated when w < 0; axis a,
    angle theta, and t' = rotate((cosP(h), sinP(h) a), t) with h = ((-stamp) theta) 0.5;
    block = {a, theta, t', status}; status 0 applied, 1 no motion, 2 invalid motion, 3 theta > max_angle: for a status
    other than 0 the first seven words are 0 and every row is copied;
  * per point (deskew_ref): s = its time, or the sweep fraction of its azimuth (sweep_fraction_ref), clamped to [0, 1];
    alpha = s - stamp; h = (alpha theta) 0.5; qp = (cosP(h), sinP(h) a); o = rotate(qp, p) + alpha t'; the normal, if
    any, becomes rotate(qp, n); every other column is copied.  A row whose x, y, z or s is not finite -- or, in azimuth
    mode, with x == y == 0 -- is copied;
  * sin_poly / cos_poly are the Taylor polynomials to x^15 / x^16 in Horner form (within 2^-53 of sin and cos on
    |x| <= pi/4, hence max_angle <= pi/2); atan_poly is Abramowitz & Stegun 4.4.49 (2e-8 rad on [0, 1]).  Fixed
    polynomials, not libm, make the per-point result the same bits on the device and here;
  * skew_ref is the inverse map p = R^-alpha (p' - alpha t'): it makes the skewed twin of a rigid cloud for tests and
    reports.
"""
import math

import numpy as np

from . import se3

HALF_PI, PI, TWO_PI = 1.5707963267948966, 3.141592653589793, 6.283185307179586
_SIN = [(-1.0) ** (k // 2) / math.factorial(k) for k in range(1, 16, 2)]        # S1 .. S15
_COS = [(-1.0) ** (k // 2) / math.factorial(k) for k in range(0, 17, 2)]        # C0 .. C16
_ATAN = [1.0, -0.3333314528, 0.1999355085, -0.1420889944, 0.1065626393, -0.0752896400, 0.0429096138, -0.0161657367,
         0.0028662257]

DESKEW_DEFAULTS = dict(motion="network", times="azimuth", stamp=0.5, az_start_turn=-0.5, az_clockwise=False, max_angle=HALF_PI)


def _horner(coef, z):
    p = np.full_like(z, coef[-1])
    for c in coef[-2::-1]:
        p = c + z * p
    return p


def sin_poly(x):
    x = np.asarray(x, np.float64)
    return x * _horner(_SIN, x * x)


def cos_poly(x):
    x = np.asarray(x, np.float64)
    return _horner(_COS, x * x)


def atan_poly(r):
    r = np.asarray(r, np.float64)
    return r * _horner(_ATAN, r * r)


def sweep_fraction_ref(xy, start_turn=-0.5, clockwise=False):
    """The sweep fraction of returns at xy [..., 2] from their azimuth: float64 [...] in [0, 1].  A row with x == y == 0
    gives NaN (the kernel copies such a row without computing a fraction)."""
    xy = np.asarray(xy).astype(np.float64)
    x, y = xy[..., 0], xy[..., 1]
    ax, ay = np.abs(x), np.abs(y)
    with np.errstate(invalid="ignore", divide="ignore"):
        phi = atan_poly(np.where(ax < ay, ax, ay) / np.where(ax < ay, ay, ax))
        phi = np.where(ay > ax, HALF_PI - phi, phi)
        phi = np.where(x < 0.0, PI - phi, phi)
        phi = np.where(y < 0.0, -phi, phi)
        f = phi / TWO_PI - float(start_turn)
        if clockwise:
            f = -f
        return f - np.floor(f)


def motion_ref(rel7=None, pose_a=None, pose_b=None, stamp=0.5, max_angle=HALF_PI, theta=None):
    """The 8-word motion block {a, theta, t', status} of rel7 (fp32 [7], widened) or of the pose pair (float64 [7] each:
    se3.between).  theta=: the device's angle in place of this host's 2 atan2(su, q0)."""
    out = np.zeros(8)
    if rel7 is not None and (pose_a is not None or pose_b is not None):
        raise ValueError("motion_ref: give rel7 or the pose pair, not both")
    if (pose_a is None) != (pose_b is None):
        raise ValueError("motion_ref: pose_a and pose_b go together")
    if rel7 is None and pose_a is None:
        out[7] = 1.0
        return out
    with np.errstate(all="ignore"):
        if rel7 is not None:
            M = np.asarray(rel7, np.float32).reshape(7).astype(np.float64)
        else:
            M = se3.between(np.asarray(pose_a, np.float64).reshape(7), np.asarray(pose_b, np.float64).reshape(7))
        t, q = M[:3], M[3:].copy()
        n2 = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]
        if not (n2 > 0.0 and n2 < np.inf) or not np.isfinite(t).all():
            out[7] = 2.0
            return out
        q = q / np.sqrt(n2)
        if q[0] < 0.0:
            q = -q
        su = np.sqrt((q[1] * q[1] + q[2] * q[2]) + q[3] * q[3])
        th = 2.0 * np.arctan2(su, q[0]) if theta is None else float(theta)
        a = q[1:] / su if su != 0.0 else np.zeros(3)
        if th > max_angle:
            out[7] = 3.0
            return out
        h = np.float64(((-float(stamp)) * th) * 0.5)
        qs = np.concatenate([[cos_poly(h)], sin_poly(h) * a])
        out[:3], out[3], out[4:7] = a, th, se3.rotate(qs, t)
    return out


def _times_of(xyz, times, az_start_turn, az_clockwise):
    """(s float64 [N] unclamped, rows that have a time at all)"""
    if times is not None:
        s = np.asarray(times).astype(np.float64).reshape(len(xyz))
        return s, np.ones(len(xyz), bool)
    return sweep_fraction_ref(xyz[:, :2], az_start_turn, az_clockwise), ~((xyz[:, 0] == 0.0) & (xyz[:, 1] == 0.0))


def _quats(alpha, motion):
    h = (alpha * motion[3]) * 0.5
    return np.concatenate([cos_poly(h)[:, None], sin_poly(h)[:, None] * motion[None, :3]], 1)


def deskew_ref(points, times=None, motion=None, stamp=0.5, az_start_turn=-0.5, az_clockwise=False, normal_col=-1,
               store=True):
    """The per-point rule on fp32 rows [N, F] under the 8-word block `motion` (motion_ref; None: no motion).  -> fp32
    [N, F]; store=False: the float64 [N, 3] positions before the store (rows that are copied: their input)."""
    points = np.ascontiguousarray(points, np.float32)
    out = points.copy()
    xyz = points[:, :3].astype(np.float64)
    if motion is None or motion[7] != 0.0 or len(points) == 0:
        return out if store else xyz
    motion = np.asarray(motion, np.float64)
    with np.errstate(all="ignore"):
        s, has = _times_of(xyz, times, az_start_turn, az_clockwise)
        move = has & np.isfinite(xyz).all(1) & np.isfinite(s)
        s = np.where(s < 0.0, 0.0, np.where(s > 1.0, 1.0, s))
        alpha = s - float(stamp)
        qp = _quats(alpha, motion)
        o = se3.rotate(qp, xyz) + alpha[:, None] * motion[None, 4:7]
        if not store:
            return np.where(move[:, None], o, xyz)
        out[move, :3] = o[move].astype(np.float32)
        if normal_col >= 0:
            n = se3.rotate(qp, points[:, normal_col:normal_col + 3].astype(np.float64))
            out[move, normal_col:normal_col + 3] = n[move].astype(np.float32)
    return out


def skew_ref(points, times=None, motion=None, stamp=0.5, az_start_turn=-0.5, az_clockwise=False, normal_col=-1, iters=4):
    """The inverse map: the rigid cloud `points` [N, F] (sensor frame at `stamp`) as the moving sensor would have recorded
    it, p = R^-alpha (p' - alpha t'), float64 [N, F] (the caller rounds).  times=None: the time of a return is the
    sweep fraction of the azimuth at which it is RECORDED, found by `iters` fixed-point rounds from the rigid azimuth."""
    out = np.array(points, dtype=np.float64)
    if motion is None or motion[7] != 0.0 or len(out) == 0:
        return out
    motion = np.asarray(motion, np.float64)
    rigid = out[:, :3].copy()
    ok = np.isfinite(rigid).all(1)
    with np.errstate(all="ignore"):
        p = rigid
        for _ in range(1 if times is not None else max(int(iters), 1)):
            s, has = _times_of(p, times, az_start_turn, az_clockwise)
            move = ok & has & np.isfinite(s)
            s = np.where(s < 0.0, 0.0, np.where(s > 1.0, 1.0, s))
            alpha = s - float(stamp)
            qi = _quats(-alpha, motion)
            p = np.where(move[:, None], se3.rotate(qi, rigid - alpha[:, None] * motion[None, 4:7]), rigid)
        out[:, :3] = p
        if normal_col >= 0:
            n = se3.rotate(qi, out[:, normal_col:normal_col + 3])
            out[move, normal_col:normal_col + 3] = n[move]
    return out


def check_deskew(options):
    """The deskew= options of an OdometryRunner / the keyword options of a Deskewer (ValueError naming the key): -> the
    options with the defaults filled in."""
    unknown = set(options) - set(DESKEW_DEFAULTS)
    if unknown:
        raise ValueError("deskew takes %s; got %s" % (", ".join(sorted(DESKEW_DEFAULTS)), sorted(unknown)))
    o = dict(DESKEW_DEFAULTS, **options)
    if o["motion"] not in ("network", "refined"):
        raise ValueError("deskew: motion must be \"network\" or \"refined\", got %r" % (o["motion"],))
    if o["times"] not in ("azimuth", "input"):
        raise ValueError("deskew: times must be \"azimuth\" or \"input\", got %r" % (o["times"],))
    for key in ("stamp", "az_start_turn", "max_angle"):
        try:
            o[key] = float(o[key])
        except (TypeError, ValueError):
            raise ValueError("deskew: %s must be a number, got %r" % (key, o[key]))
    if not 0.0 <= o["stamp"] <= 1.0:
        raise ValueError("deskew: stamp must lie in [0, 1] (NaN is refused), got %r" % (o["stamp"],))
    if not math.isfinite(o["az_start_turn"]):
        raise ValueError("deskew: az_start_turn must be finite, got %r" % (o["az_start_turn"],))
    if not isinstance(o["az_clockwise"], (bool, np.bool_)):
        raise ValueError("deskew: az_clockwise must be True or False, got %r" % (o["az_clockwise"],))
    o["az_clockwise"] = bool(o["az_clockwise"])
    if not 0.0 < o["max_angle"] <= HALF_PI:
        raise ValueError("deskew: max_angle must lie in (0, pi/2] (NaN is refused), got %r" % (o["max_angle"],))
    return o


class Deskewer:
    """The device stage: owns the output buffer [point_capacity, n_cols] and an [8] motion block; calling it enqueues
    ONE launch on the current stream and returns the [P, n_cols] view of the buffer that holds the de-skewed scan.  With
    n_cols >= 7 columns 4..6 are the normal and are rotated.  Nothing is allocated after construction and nothing is
    read on the host.  options: those of check_deskew (`motion` names the runner's source and is not used here)."""

    def __init__(self, point_capacity, n_cols, device="cuda", **options):
        import torch
        from rslo_amd import capi
        self.options = check_deskew(options)
        self.point_capacity, self.n_cols = int(point_capacity), int(n_cols)
        if self.point_capacity < 0 or self.n_cols < 3:
            raise capi.RsloHipError("Deskewer: point_capacity must be >= 0 and n_cols >= 3")
        self.normal_col = 4 if self.n_cols >= 7 else -1
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.out = torch.zeros((self.point_capacity, self.n_cols), dtype=torch.float32, device=self.device)
        self.motion = torch.zeros((8,), dtype=torch.float64, device=self.device)

    def __call__(self, points, times=None, rel7=None, pose_a=None, pose_b=None, motion_out=None):
        """points fp32 CUDA [P, n_cols]; times fp32 CUDA [P] exactly when the stage was built with times="input"; the
        motion is rel7 (fp32 CUDA [7]) or pose_a, pose_b (float64 CUDA [7]: A^-1 o B) or nothing (a copy).  motion_out:
        a float64 CUDA [8] row for the motion block (default: self.motion)."""
        from rslo_amd import capi
        o = self.options
        if points.dim() != 2 or points.shape[1] != self.n_cols or points.shape[0] > self.point_capacity:
            raise capi.RsloHipError("Deskewer: takes [P <= %d, %d] scans, got %s"
                                    % (self.point_capacity, self.n_cols, tuple(points.shape)))
        if (times is not None) != (o["times"] == "input"):
            raise capi.RsloHipError("Deskewer: times=\"input\" needs a times tensor per scan, times=\"azimuth\" takes none")
        view = self.out[:points.shape[0]]
        capi.deskew(points, view, times, rel7, pose_a, pose_b, o["stamp"], o["az_start_turn"], o["az_clockwise"],
                    o["max_angle"], self.normal_col, self.motion if motion_out is None else motion_out)
        return view
