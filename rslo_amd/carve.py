"""Free-space carving: evict the cells of a world voxel map that the current scan sees through.

    ri = RangeImage(rows=64, cols=1024)                          # owns the device image [H, W]
    vmap.carve(ri(scan), pose, max_range=60.0)                   # scan fp32 CUDA [P, F >= 3], pose float64 CUDA [7]
    runner = inference.OdometryRunner(net, voxel_map=vmap, carve=dict(every=1))

A map that only fills keeps every cell a moving object ever occupied: a car that drives ahead of the sensor leaves a trail
along its whole path, and min_hits does not help, because a slow vehicle collects more hits than a wall seen once.  The
visibility check of Removert-like methods removes the trail: bin the scan into a range image, move every stored cell into
the sensor frame, and evict the cell when the scan's return in its direction lies well BEHIND it -- the sensor looked
straight through the place where it stands.

RangeImage is the device stage (csrc/carve.hip rslo_range_image; rules: include/rslo_hip.h "Free-space carving"): two
launches per scan, no host read, nothing allocated after construction.  The functions below restate the pixel rules in
numpy float64, operation by operation, and are the arbiter of the tests, which compare the image bit for bit; the carve
rule itself is restated by mapping.VoxelMapRef.carve on top of pixel_ref.  The rules in one place:

  * pixel of a sensor-frame position (x, y, z) with rho2 = x*x + y*y != 0, image of H rows x W columns over the elevation
    tangents [tan_lo, tan_hi):  col = min(W-1, int(floor(f*W))) with f = deskew.sweep_fraction_ref((x, y)) (start -0.5,
    counter-clockwise; f can round to exactly 1);  e = z / sqrt(rho2);  u = ((e - tan_lo) / (tan_hi - tan_lo)) * H;  no
    pixel unless u >= 0 and u < H;  row = int(floor(u)).  Rows are binned in the tangent of the elevation, so no second
    arctangent is needed;
  * image: a point with a non-finite coordinate, with rho2 == 0 or without a pixel is skipped; r = sqrt(rho2 + z*z); a
    pixel holds the minimum, as uint32, of the bit patterns of float32(r) over its points (positive floats order as their
    bits), an empty pixel 0xFFFFFFFF.  A minimum does not depend on arrival order;
  * the carve rule: module docstring of rslo_amd/mapping.py.
"""
import math

import numpy as np

from .deskew import sweep_fraction_ref

EMPTY = np.uint32(0xFFFFFFFF)
MAX_ROWS, MAX_COLS, MAX_WIN_ROWS, MAX_WIN_COLS = 256, 4096, 4, 8

CARVE_DEFAULTS = dict(every=1, rows=64, cols=1024, tan_lo=math.tan(math.radians(-25.0)), tan_hi=math.tan(math.radians(3.0)),
                      win_rows=1, win_cols=1, margin_abs=0.3, margin_rel=0.0, max_range=60.0, grace=1)


def check_image(rows, cols, tan_lo, tan_hi, name="carve"):
    """The shape and the elevation span of a range image (ValueError naming the argument): -> (H, W, tan_lo, tan_hi)"""
    for key, v, lo, hi in (("rows", rows, 1, MAX_ROWS), ("cols", cols, 8, MAX_COLS)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError("%s: %s must be an integer in %d .. %d, got %r" % (name, key, lo, hi, v))
    for key, v in (("tan_lo", tan_lo), ("tan_hi", tan_hi)):
        try:
            ok = math.isfinite(float(v))
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError("%s: %s must be a finite number, got %r" % (name, key, v))
    if not float(tan_lo) < float(tan_hi):
        raise ValueError("%s: tan_lo must be below tan_hi, got %r and %r" % (name, tan_lo, tan_hi))
    return int(rows), int(cols), float(tan_lo), float(tan_hi)


def check_rule(win_rows, win_cols, margin_abs, margin_rel, max_range, grace, name="carve"):
    """The arguments of the carve rule (ValueError naming the argument), before anything is written: -> the six, typed"""
    for key, v, hi in (("win_rows", win_rows, MAX_WIN_ROWS), ("win_cols", win_cols, MAX_WIN_COLS), ("grace", grace, None)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < 0 or (hi is not None and v > hi):
            raise ValueError("%s: %s must be an integer %s, got %r" % (name, key, ">= 0" if hi is None else "in 0 .. %d" % hi, v))
    out = []
    for key, v in (("margin_abs", margin_abs), ("margin_rel", margin_rel), ("max_range", max_range)):
        try:
            f = float(v)
        except (TypeError, ValueError):
            raise ValueError("%s: %s must be a number, got %r" % (name, key, v))
        if key == "max_range" and not f > 0.0:
            raise ValueError("%s: max_range must be > 0 (NaN is refused; +inf is allowed), got %r" % (name, v))
        if key != "max_range" and not f >= 0.0:
            raise ValueError("%s: %s must be >= 0 (NaN is refused), got %r" % (name, key, v))
        out.append(f)
    return (int(win_rows), int(win_cols)) + tuple(out) + (int(grace),)


def check_carve(options):
    """The carve= options of an OdometryRunner (ValueError naming the key): -> the options with the defaults filled in."""
    unknown = set(options) - set(CARVE_DEFAULTS)
    if unknown:
        raise ValueError("carve takes %s; got %s" % (", ".join(sorted(CARVE_DEFAULTS)), sorted(unknown)))
    o = dict(CARVE_DEFAULTS, **options)
    every = o["every"]
    if isinstance(every, (bool, np.bool_)) or not isinstance(every, (int, np.integer)) or every < 1:
        raise ValueError("carve: every must be an integer >= 1, got %r" % (every,))
    o["every"] = int(every)
    o["rows"], o["cols"], o["tan_lo"], o["tan_hi"] = check_image(o["rows"], o["cols"], o["tan_lo"], o["tan_hi"])
    (o["win_rows"], o["win_cols"], o["margin_abs"], o["margin_rel"], o["max_range"], o["grace"]) = check_rule(
        o["win_rows"], o["win_cols"], o["margin_abs"], o["margin_rel"], o["max_range"], o["grace"])
    return o


def pixel_ref(xyz, rows, cols, tan_lo, tan_hi):
    """The pixel rule on float64 positions xyz [N, 3] in the sensor frame: -> (has [N] bool, row [N], col [N] int64; row
    and col are 0 where has is False).  has is False for rho2 == 0, for a position without a row in the image and for
    anything NaN; the caller applies its own test on rho2 (== 0 in the image, > 0 in the carve) on top."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    H, W, tan_lo, tan_hi = int(rows), int(cols), float(tan_lo), float(tan_hi)
    with np.errstate(all="ignore"):
        x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
        rho2 = x * x + y * y
        e = z / np.sqrt(rho2)
        u = ((e - tan_lo) / (tan_hi - tan_lo)) * float(H)
        f = sweep_fraction_ref(xyz[:, :2], -0.5, False)
        has = (u >= 0.0) & (u < float(H)) & (rho2 != 0.0) & np.isfinite(f)
        row = np.floor(np.where(has, u, 0.0)).astype(np.int64)
        col = np.minimum(W - 1, np.floor(np.where(has, f, 0.0) * float(W)).astype(np.int64))
    return has, row, col


def range_image_ref(points, rows=64, cols=1024, tan_lo=CARVE_DEFAULTS["tan_lo"], tan_hi=CARVE_DEFAULTS["tan_hi"]):
    """The range image of fp32 rows [N, >= 3] (module docstring): uint32 [rows, cols], empty pixels 0xFFFFFFFF."""
    H, W, tan_lo, tan_hi = check_image(rows, cols, tan_lo, tan_hi, "range_image_ref")
    pts = np.asarray(points)
    if pts.dtype != np.float32 or pts.ndim != 2 or pts.shape[1] < 3:
        raise ValueError("points must be float32 [P, >= 3]")
    img = np.full((H * W,), EMPTY, np.uint32)
    with np.errstate(all="ignore"):
        xyz = pts[:, :3].astype(np.float64)
        finite = np.isfinite(pts[:, :3]).all(axis=1)
        rho2 = xyz[:, 0] * xyz[:, 0] + xyz[:, 1] * xyz[:, 1]
        r = np.sqrt(rho2 + xyz[:, 2] * xyz[:, 2])
        has, row, col = pixel_ref(xyz, H, W, tan_lo, tan_hi)
        ok = finite & (rho2 != 0.0) & has
        bits = r[ok].astype(np.float32).view(np.uint32)
    np.minimum.at(img, row[ok] * W + col[ok], bits)
    return img.reshape(H, W)


def window_min_ref(img, row, col, win_rows, win_cols):
    """The minimum word of the window about (row [N], col [N]) in img (uint32 [H, W]): rows clipped to the image, columns
    wrapped modulo W.  An empty pixel is the largest word, so the minimum skips it by itself; uint32 [N]."""
    img = np.asarray(img)
    H, W = img.shape
    m = np.full(np.shape(row), EMPTY, np.uint32)
    for dr in range(-int(win_rows), int(win_rows) + 1):
        rr = row + dr
        inside = (rr >= 0) & (rr < H)
        rr = np.clip(rr, 0, H - 1)
        for dc in range(-int(win_cols), int(win_cols) + 1):
            m = np.minimum(m, np.where(inside, img[rr, (col + dc) % W], EMPTY))
    return m


class RangeImage:
    """The device stage: owns the image (int32 CUDA [rows, cols], holding the uint32 range words) of one scan; calling it
    enqueues TWO launches on the current stream and returns itself, ready for VoxelMap.carve.  Nothing is allocated after
    construction and nothing is read on the host; numpy() makes one host read."""

    def __init__(self, rows=64, cols=1024, tan_lo=CARVE_DEFAULTS["tan_lo"], tan_hi=CARVE_DEFAULTS["tan_hi"], device="cuda"):
        import torch
        self.rows, self.cols, self.tan_lo, self.tan_hi = check_image(rows, cols, tan_lo, tan_hi, "RangeImage")
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.img = torch.full((self.rows, self.cols), -1, dtype=torch.int32, device=self.device)

    def __call__(self, points):
        """points fp32 CUDA [P, F >= 3], read in place (a column view of a wider cloud will do)"""
        from rslo_amd import capi
        capi.range_image(points, self.img, self.tan_lo, self.tan_hi)
        return self

    def numpy(self):
        """the image as uint32 [rows, cols] on the host"""
        return self.img.cpu().numpy().view(np.uint32)
