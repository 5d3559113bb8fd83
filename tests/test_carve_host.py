"""Free-space carving on the float64 restatement alone (rslo_amd/carve.py range_image_ref / pixel_ref / window_min_ref,
rslo_amd/mapping.py VoxelMapRef.carve; rules: include/rslo_hip.h "Free-space carving"): the pixel rules on hand-made
points, the window on hand-made images, and the rule as a whole on a synthetic street with a block of ghost cells on
the free road.  No GPU needed."""
import math

import numpy as np
import pytest

IDENT = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
EMPTY = 0xFFFFFFFF


def _pts(*rows):
    return np.array(rows, np.float32).reshape(len(rows), -1)


def _bits(r):
    return int(np.float32(r).view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# pixel rules
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [8, 24, 1024])
def test_axes_land_in_exact_quarter_columns(W):
    """start -0.5, counter-clockwise: -x is column 0, -y a quarter turn on, +x half a turn, +y three quarters"""
    from rslo_amd import carve
    pts = _pts((-3, 0, 0), (0, -2, 0), (5, 0, 0), (0, 7, 0))
    has, row, col = carve.pixel_ref(pts.astype(np.float64), 4, W, -1.0, 1.0)
    assert has.all() and (row == 2).all()                      # e = 0 -> u = 0.5 * 4
    assert col.tolist() == [0, W // 4, W // 2, 3 * W // 4]
    img = carve.range_image_ref(pts, 4, W, -1.0, 1.0)
    assert img.dtype == np.uint32 and img.shape == (4, W) and (img != EMPTY).sum() == 4
    assert [int(img[2, c]) for c in col] == [_bits(3), _bits(2), _bits(5), _bits(7)]


def test_the_seam_and_the_clamp(monkeypatch):
    """just short of +pi is the last column, just past -pi the first; and a fraction of exactly 1 -- which the subtraction
    f - floor(f) can round to -- is held to W - 1"""
    from rslo_amd import carve
    has, row, col = carve.pixel_ref(np.array([[-1.0, 1e-9, 0.0], [-1.0, -1e-9, 0.0], [-1.0, -1e-300, 0.0]]), 1, 24, -1.0, 1.0)
    assert has.all() and col.tolist() == [23, 0, 0]
    monkeypatch.setattr(carve, "sweep_fraction_ref", lambda xy, *a: np.ones(len(xy)))
    has, row, col = carve.pixel_ref(np.array([[1.0, 2.0, 0.0]]), 1, 24, -1.0, 1.0)
    assert has.all() and col.tolist() == [23]


def test_skipped_points_and_row_edges():
    from rslo_amd import carve
    H = 8
    pts = _pts((0, 0, 4),                       # vertical: rho2 == 0
               (1, 0, -1),                      # e == tan_lo: u exactly 0 -> row 0
               (1, 0, 1),                       # e == tan_hi: u exactly H -> no pixel
               (2, 0, 1.75),                    # e = 0.875: u = 7.5 -> the last row
               (1, 0, -1.0000001),              # below the image
               (np.nan, 1, 0), (1, np.inf, 0), (1, 1, -np.inf))
    has, row, col = carve.pixel_ref(pts.astype(np.float64), H, 16, -1.0, 1.0)
    assert has[:5].tolist() == [False, True, False, True, False]
    assert row[1] == 0 and row[3] == H - 1
    # (a non-finite coordinate is the image's own test: an infinite y alone would still name a pixel)
    img = carve.range_image_ref(pts, H, 16, -1.0, 1.0)
    assert (img != EMPTY).sum() == 2
    assert int(img[0, 8]) == _bits(math.sqrt(2.0)) and int(img[7, 8]) == _bits(math.sqrt(4.0 + 1.75 * 1.75))


def test_a_pixel_keeps_its_nearest_return_whatever_the_order():
    from rslo_amd import carve
    rng = np.random.default_rng(3)
    pts = np.zeros((500, 4), np.float32)
    pts[:, 0] = rng.uniform(2.0, 30.0, 500)      # all on +x, e = 0: one pixel
    img = carve.range_image_ref(pts, 8, 16, -1.0, 1.0)
    assert (img != EMPTY).sum() == 1 and int(img[4, 8]) == _bits(pts[:, 0].min())
    assert (carve.range_image_ref(pts[::-1].copy(), 8, 16, -1.0, 1.0) == img).all()
    assert (carve.range_image_ref(np.zeros((0, 3), np.float32), 8, 16, -1.0, 1.0) == EMPTY).all()


def test_argument_errors_name_the_argument():
    from rslo_amd import carve
    for kw, word in ((dict(rows=0), "rows"), (dict(rows=257), "rows"), (dict(cols=7), "cols"), (dict(cols=4097), "cols"),
                     (dict(tan_lo=0.1, tan_hi=0.1), "tan_lo"), (dict(tan_hi=float("nan")), "tan_hi"),
                     (dict(tan_lo=float("-inf")), "tan_lo"), (dict(win_rows=5), "win_rows"), (dict(win_cols=9), "win_cols"),
                     (dict(win_cols=-1), "win_cols"), (dict(margin_abs=-0.1), "margin_abs"),
                     (dict(margin_rel=float("nan")), "margin_rel"), (dict(max_range=0.0), "max_range"),
                     (dict(max_range=float("nan")), "max_range"), (dict(grace=-1), "grace"), (dict(every=0), "every"),
                     (dict(evry=2), "evry")):
        with pytest.raises(ValueError, match=word):
            carve.check_carve(kw)
    o = carve.check_carve(dict(max_range=float("inf"), every=3))
    assert o["max_range"] == float("inf") and o["every"] == 3 and o["rows"] == 64 and o["cols"] == 1024
    assert o["tan_lo"] == math.tan(math.radians(-25.0)) and o["tan_hi"] == math.tan(math.radians(3.0))
    assert (o["win_rows"], o["win_cols"], o["margin_abs"], o["margin_rel"], o["grace"]) == (1, 1, 0.3, 0.0, 1)


# ---------------------------------------------------------------------------------------------------------------------
# the window, on an 8 x 16 image over tangents -1 .. 1 and one cell at 5 m in a chosen pixel
# ---------------------------------------------------------------------------------------------------------------------
H, W = 8, 16


def _cell_at(row, col, rho=5.0):
    """a map of ONE cell whose stored point lies in the middle of pixel (row, col), horizontal range rho"""
    from rslo_amd import carve
    from rslo_amd.mapping import VoxelMapRef
    phi = ((col + 0.5) / W - 0.5) * 2.0 * math.pi
    e = -1.0 + (row + 0.5) / H * 2.0
    p = _pts((rho * math.cos(phi), rho * math.sin(phi), rho * e, 0.5))
    ref = VoxelMapRef(0.2)
    ref.insert(p, IDENT)
    has, r, c = carve.pixel_ref(ref.rows[:, :3].astype(np.float64), H, W, -1.0, 1.0)
    assert has.all() and (int(r[0]), int(c[0])) == (row, col)
    return ref, float(np.sqrt((p[0, :3].astype(np.float64) ** 2).sum()))


def _evicted(ref, img, **kw):
    kw = dict(dict(tan_lo=-1.0, tan_hi=1.0, grace=0, margin_abs=0.3), **kw)
    return bool(ref.carve_mask(img, IDENT, **kw)[0])


@pytest.mark.parametrize("col, nbr", [(0, W - 1), (W - 1, 0)])
def test_columns_wrap(col, nbr):
    ref, r_m = _cell_at(3, col)
    img = np.full((H, W), EMPTY, np.uint32)
    img[3, col] = _bits(r_m + 10.0)                          # the scan looks through the cell ...
    assert _evicted(ref, img, win_rows=0, win_cols=0) and _evicted(ref, img, win_rows=1, win_cols=1)
    img[3, nbr] = _bits(r_m - 1.0)                           # ... but the pixel across the seam holds a nearer return
    assert _evicted(ref, img, win_rows=0, win_cols=0) and not _evicted(ref, img, win_rows=0, win_cols=1)
    img[3, nbr] = EMPTY
    img[3, (col + 8) % W] = _bits(r_m - 1.0)                 # half a turn away: reached by no window narrower than 8
    assert _evicted(ref, img, win_cols=7) and not _evicted(ref, img, win_cols=8)


@pytest.mark.parametrize("row, other", [(0, H - 1), (H - 1, 0)])
def test_rows_are_clipped_not_wrapped(row, other):
    ref, r_m = _cell_at(row, 5)
    img = np.full((H, W), EMPTY, np.uint32)
    img[row, 5] = _bits(r_m + 10.0)
    img[other, 5] = _bits(r_m - 1.0)                         # the far edge of the image does not protect
    assert _evicted(ref, img, win_rows=1, win_cols=1) and _evicted(ref, img, win_rows=4, win_cols=0)      # 4 < H - 1
    inner = row + 1 if row == 0 else row - 1
    img[inner, 6] = _bits(r_m - 1.0)                         # the row next to it does
    assert not _evicted(ref, img, win_rows=1, win_cols=1) and _evicted(ref, img, win_rows=0, win_cols=1)


def test_empty_centre_keeps_and_empty_neighbours_are_ignored():
    ref, r_m = _cell_at(4, 9)
    img = np.full((H, W), EMPTY, np.uint32)
    assert not _evicted(ref, img)                            # nothing observed at all
    for r in (3, 4, 5):
        for c in (8, 9, 10):
            img[r, c] = _bits(r_m + 10.0)
    img[4, 9] = EMPTY
    assert not _evicted(ref, img)                            # its own pixel is empty: not observed, whatever the neighbours say
    img[:] = EMPTY
    img[4, 9] = _bits(r_m + 10.0)
    assert _evicted(ref, img)                                # all eight neighbours empty: the centre decides
    img[4, 9] = _bits(r_m + 0.25)
    assert not _evicted(ref, img)                            # within margin_abs
    assert _evicted(ref, img, margin_abs=0.2) and not _evicted(ref, img, margin_abs=0.0, margin_rel=0.1)
    img[4, 9] = _bits(r_m + 10.0)
    assert not _evicted(ref, img, max_range=r_m) and _evicted(ref, img, max_range=float("inf"))
    assert not _evicted(ref, img, grace=1)                   # S = 1: the cell is of the last scan


# ---------------------------------------------------------------------------------------------------------------------
# the scene
# ---------------------------------------------------------------------------------------------------------------------
_SCENE = {}


def _scene():
    """synthetic.scan(1024, 64) at the origin in a 0.2 m map, a 4 x 2 x 1.4 m block of ghost cells standing on the free
    road 11 .. 15 m ahead (what a vehicle that has driven on leaves behind), one more, empty scan so that every cell is
    one scan old (the default grace), and the image of the scan taken 1 m further on"""
    if not _SCENE:
        from rslo_amd import carve, synthetic
        from rslo_amd.mapping import VoxelMapRef
        ref = VoxelMapRef(0.2)
        ref.insert(synthetic.scan(1024, 64), IDENT)
        static_keys = ref.keys.copy()
        g = np.mgrid[11.1:15:0.2, -0.9:1:0.2, 0.1:1.4:0.2].reshape(3, -1).T
        ghost = np.zeros((len(g), 4), np.float32)
        ghost[:, :3] = g - np.array([0.0, 0.0, synthetic.SENSOR_H])
        ref.insert(ghost, IDENT)
        ref.insert(np.zeros((0, 4), np.float32), IDENT)
        _SCENE.update(ref=ref, ghost_keys=ref.keys[~np.isin(ref.keys, static_keys)].copy(),
                      image=carve.range_image_ref(synthetic.scan(1024, 64, (1.0, 0.0))),
                      pose=np.array([1.0, 0, 0, 1, 0, 0, 0], np.float64))
    return _SCENE


def _copy(ref):
    from rslo_amd.mapping import VoxelMapRef
    out = VoxelMapRef(ref.voxel_size)
    out.keys, out.tags, out.hits, out.rows = ref.keys.copy(), ref.tags.copy(), ref.hits.copy(), ref.rows.copy()
    out.counters, out.prune_counters = dict(ref.counters), dict(ref.prune_counters)
    return out


def test_the_scene():
    """The restatement's own figures on this scene (also in profiles/NOTES.md "Free-space carving"): 1 of 13756 static
    cells evicted (0.007 %), 896 of 1346 ghost cells (66.6 %); the ghost cells that stay lie within the margin of the
    ground or behind the block's own far side as the scan sees the road.  Required: static loss <= 0.5 %, ghost removal
    >= 50 %."""
    sc = _scene()
    ref = _copy(sc["ref"])
    is_ghost = np.isin(ref.keys, sc["ghost_keys"])
    n_ghost, n_static = int(is_ghost.sum()), int((~is_ghost).sum())
    assert 1100 <= n_ghost <= 1400 and n_static > 10000
    before = ref.points()
    evict = ref.carve_mask(sc["image"], sc["pose"])
    lost_static, gone_ghost = int((evict & ~is_ghost).sum()), int((evict & is_ghost).sum())
    print("static cells evicted: %d of %d (%.3f %%); ghost cells evicted: %d of %d (%.1f %%)" % (
        lost_static, n_static, 100.0 * lost_static / n_static, gone_ghost, n_ghost, 100.0 * gone_ghost / n_ghost))
    assert lost_static <= 0.005 * n_static
    assert gone_ghost >= 0.5 * n_ghost
    survivors = set(ref.tags[~evict].tolist())
    ref.carve(sc["image"], sc["pose"])
    rows, tags, hits = ref.points()
    assert set(tags.tolist()) == survivors and ref.stats()["n_cells"] == len(tags) == n_ghost + n_static - int(evict.sum())
    assert ref.carve_stats() == {"n_carves": 1, "n_carved": int(evict.sum())}
    assert ref.prune_stats() == {"n_prunes": 0, "n_evicted": 0, "n_lost": 0}
    keep = np.isin(before[1], tags)                           # kept cells keep tag, row and hits to the bit
    assert before[0][keep].tobytes() == rows.tobytes() and (before[2][keep] == hits).all()
    st0, st = sc["ref"].stats(), ref.stats()
    assert {k: v for k, v in st.items() if k != "n_cells"} == {k: v for k, v in st0.items() if k != "n_cells"}


@pytest.mark.parametrize("case", ["nan pose", "empty image", "grace beyond the drive"])
def test_calls_that_evict_nothing(case):
    from rslo_amd import carve
    sc = _scene()
    ref = _copy(sc["ref"])
    before = ref.points()
    image, pose, kw = sc["image"], sc["pose"], {}
    if case == "nan pose":
        pose = pose.copy()
        pose[1] = np.nan
    elif case == "empty image":
        image = carve.range_image_ref(np.zeros((0, 3), np.float32))
    else:
        kw = dict(grace=3)                                     # three scans so far: no cell is three scans old
    ref.carve(image, pose, **kw)
    after = ref.points()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
    assert ref.carve_stats() == {"n_carves": 1, "n_carved": 0} and ref.stats() == sc["ref"].stats()
    if case == "nan pose":                                   # ... in whichever word the NaN sits
        for k in range(7):
            bad = sc["pose"].copy()
            bad[k] = np.nan
            assert not ref.carve_mask(sc["image"], bad).any()


def test_refused_arguments_write_nothing():
    sc = _scene()
    ref = _copy(sc["ref"])
    for kw in (dict(win_rows=5), dict(win_cols=9), dict(margin_abs=-1.0), dict(margin_rel=float("nan")), dict(max_range=0.0),
               dict(grace=-1), dict(tan_lo=1.0, tan_hi=1.0)):
        with pytest.raises(ValueError):
            ref.carve(sc["image"], sc["pose"], **kw)
    with pytest.raises(ValueError):
        ref.carve(np.zeros((4, 4), np.uint32), sc["pose"])   # fewer than 8 columns
    assert ref.carve_stats() == {"n_carves": 0, "n_carved": 0} and ref.stats() == sc["ref"].stats()


def test_pyramid_applies_one_image_to_every_level():
    from rslo_amd import synthetic
    from rslo_amd.mapping import MapPyramidRef, VoxelMapRef
    sc = _scene()
    cloud = synthetic.scan(256, 32)
    pyr, singles = MapPyramidRef((0.8, 0.4)), [VoxelMapRef(0.8), VoxelMapRef(0.4)]
    for m in [pyr] + singles:
        m.insert(cloud, IDENT)
        m.insert(cloud[:0], IDENT)
    pyr.carve(sc["image"], sc["pose"], max_range=30.0)
    for lvl, single in zip(pyr.levels, singles):
        single.carve(sc["image"], sc["pose"], max_range=30.0)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(lvl.points(), single.points()))
    assert pyr.carve_stats() == [s.carve_stats() for s in singles] and all(s["n_carves"] == 1 for s in pyr.carve_stats())
    with pytest.raises(ValueError):
        pyr.carve(sc["image"], sc["pose"], win_rows=9)
    assert all(s["n_carves"] == 1 for s in pyr.carve_stats())


def test_extra_boxes_leave_the_plain_scan_alone():
    """synthetic.scan(extra_boxes=...): a box on the free road is hit, the scan without it is today's"""
    from rslo_amd import synthetic
    plain = synthetic.scan(256, 16)
    assert synthetic.scan(256, 16, extra_boxes=None).tobytes() == plain.tobytes()
    assert synthetic.scan(256, 16, extra_boxes=[]).tobytes() == plain.tobytes()
    boxed = synthetic.scan(256, 16, extra_boxes=[(14.0, 0.0, 4.0, 2.0, 1.4)])
    on_box = lambda s: int(((np.abs(s[:, 0] - 14.0) < 2.1) & (np.abs(s[:, 1]) < 1.1) & (s[:, 2] > -synthetic.SENSOR_H + 0.1)).sum())
    assert on_box(plain) == 0 and on_box(boxed) > 20
