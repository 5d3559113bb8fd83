"""Point normals without a GPU: the float64 restatement rslo_amd/normals.py of the rules the kernel implements
(include/rslo_hip.h), an independent neighbour search, the C-ABI / Python bindings of the new entry points, and the fp32
twin estimate_normals_f32 of the kernel against that restatement (with the clouds tests/test_gpu_normals_exact.py shares)."""
import ctypes

import numpy as np
import pytest

from rslo_amd import normals


def _plane(shift):
    rng = np.random.default_rng(4)
    gx, gy = np.meshgrid(np.arange(40) * 0.1 - 1.95, np.arange(40) * 0.1 - 1.95, indexing="ij")
    x, y = gx.ravel() + shift[0], gy.ravel() + shift[1]
    z = 0.3 * x - 0.2 * y - 1.5 + rng.normal(0, 1e-4, x.shape)
    return np.stack([x, y, z], 1), (gx.ravel(), gy.ravel())


@pytest.mark.parametrize("shift", [(0.0, 0.0), (60.0, 0.0)])
def test_known_plane(shift):
    xyz, (gx, gy) = _plane(shift)
    n, cnt, gap, amb = normals.estimate_normals_ref(xyz, 0.6, 30, (0.0, 0.0, 0.0), False)
    want = np.array([-0.3, 0.2, 1.0]) / np.linalg.norm([-0.3, 0.2, 1.0])
    # oriented towards the origin: the sign of want . (0 - p)
    sign = np.where((-xyz * want).sum(1) < 0, -1.0, 1.0)
    ang = np.arccos(np.clip((n * want).sum(1) * sign, -1, 1))
    assert ang.max() < 1e-3, ang.max()
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-12)
    interior = (np.abs(gx) < 1.3) & (np.abs(gy) < 1.3)
    assert interior.sum() > 500 and (cnt[interior] == 30).all()
    assert (gap[interior] > 0.3).all()          # a plane: l0 << l1 ~ l2


def test_rules_isolated_points_and_nan():
    pts = np.array([[5.0, 0.0, 1.0], [0.0, 7.0, -1.0], [-9.0, -3.0, -2.0]], np.float32)
    n, cnt, gap, amb = normals.estimate_normals_ref(pts, 0.6, 30, (0, 0, 0), False)
    assert cnt.tolist() == [1, 1, 1] and not amb.any() and (gap == 0).all()
    assert n.tolist() == [[0, 0, -1], [0, 0, 1], [0, 0, 1]]          # the point with z > 0 looks down at the origin
    n, cnt, _, _ = normals.estimate_normals_ref(pts, 0.6, 30, (0, 0, 0), True)
    assert (n == 0).all() and cnt.tolist() == [1, 1, 1]
    # a NaN point: count 0, zero normal, and its neighbours do not see it
    rng = np.random.default_rng(0)
    cloud = rng.random((40, 3)) * 0.5
    base = normals.estimate_normals_ref(cloud)
    bad = np.concatenate([cloud[:10], [[np.nan, 0.2, 0.2]], cloud[10:], [[0.1, np.inf, 0.1]]])
    n, cnt, _, _ = normals.estimate_normals_ref(bad)
    keep = np.r_[0:10, 11:41]
    assert cnt[10] == 0 and cnt[41] == 0 and (n[10] == 0).all() and (n[41] == 0).all()
    assert (cnt[keep] == base[1]).all() and np.array_equal(n[keep], base[0])


@pytest.mark.parametrize("max_nn", [3, 8, 30])
def test_selection_equals_brute_force(max_nn):
    rng = np.random.default_rng(7)
    pts = (rng.random((200, 3)) * 0.2 + np.array([3.0, -2.0, 0.5])).astype(np.float32)
    pts[150:160] = pts[20:30]                    # exact duplicates: ties go to the lower index
    n, cnt, gap, amb = normals.estimate_normals_ref(pts, 0.6, max_nn)
    assert (cnt == max_nn).all()
    p = pts.astype(np.float64)
    for i in range(0, 200, 7):
        d2 = ((p - p[i]) ** 2).sum(1)
        sel = sorted(range(200), key=lambda j: (d2[j], j))[:max_nn]
        o = p[sel] - p[i]
        cov = np.cov(o.T, bias=True)
        w, v = np.linalg.eigh(cov)
        if (w[1] - w[0]) / w[2] < 1e-3:
            continue
        assert abs(abs(np.dot(v[:, 0], n[i])) - 1.0) < 1e-9, i


def test_counts_against_independent_kdtree():
    spatial = pytest.importorskip("scipy.spatial")
    from rslo_amd import synthetic
    xyz = synthetic.small_cloud(4000, seed=0)[:, :3]
    _, cnt, _, amb = normals.estimate_normals_ref(xyz, 0.6, 30)
    d, _ = spatial.cKDTree(xyz.astype(np.float64)).query(xyz.astype(np.float64), k=31, distance_upper_bound=0.6)
    want = np.minimum(np.isfinite(d).sum(1), 30)
    assert amb.sum() <= 40
    assert np.array_equal(cnt[~amb], want[~amb])


def test_bindings():
    import torch
    from rslo_amd import build, capi
    lib = ctypes.CDLL(build.build(verbose=False))
    assert hasattr(lib, "rslo_normals_ws_bytes") and hasattr(lib, "rslo_estimate_normals")
    assert "rslo_normals_ws_bytes" in capi.SIGNATURES and "rslo_estimate_normals" in capi.SIGNATURES
    l = capi.lib()
    sizes = [l.rslo_normals_ws_bytes(n) for n in (0, 1, 64, 65, 4000, 130000, 1 << 20)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0] > 0
    with pytest.raises(capi.RsloHipError):
        capi.estimate_normals(torch.zeros(8, 4))
    with pytest.raises(capi.RsloHipError):
        capi.append_normals(torch.zeros(8, 4))
    # argument checks happen before anything is launched
    f = ctypes.c_float
    assert l.rslo_estimate_normals(None, 4, -1, f(0.6), 30, None, 0, None, None, None, 0, None) == -1
    assert l.rslo_estimate_normals(None, 4, 10, f(0.6), 2, None, 0, None, None, None, 0, None) == -1
    assert l.rslo_estimate_normals(None, 4, 10, f(0.6), 33, None, 0, None, None, None, 0, None) == -1
    assert l.rslo_estimate_normals(None, 4, 10, f(0.0), 30, None, 0, None, None, None, 0, None) == -1
    assert l.rslo_estimate_normals(None, 4, 0, f(0.6), 30, None, 0, None, None, None, 0, None) == 0
    buf = (ctypes.c_float * 64)()
    assert l.rslo_estimate_normals(buf, 4, 10, f(0.6), 30, None, 0, buf, None, buf, 16, None) == -4


# ---------------------------------------------------------------------------------------------------------------------
# the fp32 twin estimate_normals_f32 of k_nm_normals: clouds, caches and constructed cases shared with
# tests/test_gpu_normals_exact.py, which holds the kernel to the twin bit for bit
# ---------------------------------------------------------------------------------------------------------------------
ANGLE_BAR = np.deg2rad(0.1)        # the bar of tests/test_gpu_normals.py, on the reference's own checked set
GAP_MIN = 0.05
HOST_PAIRS = [(0.6, 30), (0.6, 3), (0.6, 32), (0.25, 30), (2.5, 16)]
GRID = np.float32(1.0 / 64)        # the constructed clouds live on this grid: offsets and their squares are exact in fp32
TIE_RADIUS = 0.5                   # f32(0.5)^2 = 1024 grid units^2 exactly, so a candidate can sit ON the radius
TIE_QUERY, EDGE_QUERY = 0, 41      # indices in tie_cloud()
_CLOUDS, _TWIN, _REF64 = {}, {}, {}


def cloud(name):
    """the three clouds of tests/test_gpu_normals.py, made once and never modified"""
    from rslo_amd import synthetic
    if name not in _CLOUDS:
        if name == "small":
            xyz = synthetic.small_cloud(4000, seed=0)[:, :3].copy()
        elif name == "scan":
            xyz = synthetic.scan(n_az=520, n_el=16)[:, :3].copy()
        elif name == "patch":
            rng = np.random.default_rng(11)
            u = rng.random((3000, 2)) * 0.5 - 0.25
            z = 0.4 * u[:, 0] - 0.25 * u[:, 1] + rng.normal(0, 1e-3, 3000)
            xyz = (np.stack([u[:, 0], u[:, 1], z], 1) + np.array([60.0, -30.0, 1.0])).astype(np.float32)
            xyz = np.concatenate([xyz, xyz[:64]], 0)
        else:
            raise KeyError(name)
        xyz.setflags(write=False)
        _CLOUDS[name] = xyz
    return _CLOUDS[name]


def twin(name, radius, max_nn):
    """(normals, counts, selected) of the fp32 twin on a named cloud, computed once per session"""
    key = (name, radius, max_nn)
    if key not in _TWIN:
        _TWIN[key] = normals.estimate_normals_f32(cloud(name), radius, max_nn)
    return _TWIN[key]


def ref64(name, radius, max_nn):
    key = (name, radius, max_nn)
    if key not in _REF64:
        _REF64[key] = normals.estimate_normals_ref(cloud(name), radius, max_nn, selected=True)
    return _REF64[key]


def tie_cloud():
    """Query 0 at (3, -2, 0.5) and 40 points at grid offsets from it.  25 points (the query among them) lie strictly
    inside 25 grid steps, within one step of the plane z = 0.5.  Then 16 candidates tie at exactly 25 steps
    (a^2 + b^2 + c^2 = 625, bit-equal in fp32): indices 25..32 in the plane, and their mirror images 33..40 rotated out
    of it by 15 to 24 steps.  With max_nn = 30 the tie decides slots 25..29, with max_nn = 27 slots 25..26; "lower
    index wins" keeps the neighbourhood in the plane, "higher index wins" lifts it out.
    A second query (EDGE_QUERY) at (10, 5, 0.5) has three neighbours strictly inside the radius 0.5 = 32 steps and three
    candidates at exactly 32 steps, whose fp32 d2 equals r2 bit for bit: its count is 4 under d2 < r2, 7 under <=."""
    rng = np.random.default_rng(23)
    near, seen = [(0, 0, 0)], {(0, 0)}
    while len(near) < 25:
        a, b = (int(v) for v in rng.integers(-12, 13, 2))
        if (a, b) not in seen:
            seen.add((a, b))
            near.append((a, b, int(rng.integers(-1, 2))))
    in_plane = [(25, 0, 0), (0, 25, 0), (-25, 0, 0), (0, -25, 0), (15, 20, 0), (20, -15, 0), (-7, 24, 0), (24, 7, 0)]
    lifted = [(15, 0, 20), (0, 15, 20), (7, 0, 24), (0, 7, 24), (20, 0, 15), (0, 20, 15), (-7, 0, 24), (0, -7, 24)]
    a = np.array(near + in_plane + lifted, np.float32) * GRID + np.array([3.0, -2.0, 0.5], np.float32)
    edge = [(0, 0, 0), (3, 0, 0), (0, 4, 0), (-2, -2, 1), (32, 0, 0), (0, -32, 0), (0, 0, 32)]
    b = np.array(edge, np.float32) * GRID + np.array([10.0, 5.0, 0.5], np.float32)
    xyz = np.concatenate([a, b], 0)
    assert xyz.dtype == np.float32 and len(a) == EDGE_QUERY
    return xyz


def corner_cloud():
    """eight clusters of 80 points (more than one tile of 64) beyond the sort range, at the (+-150, +-150, +-30) corners of
    the cell grid, dense enough to reach the cap; cluster k holds points [80 k, 80 k + 80), (-,-,-) first, (+,+,+) last"""
    rng = np.random.default_rng(31)
    parts = []
    for sz in (-1.0, 1.0):
        for sy in (-1.0, 1.0):
            for sx in (-1.0, 1.0):
                parts.append(np.array([150.0 * sx, 150.0 * sy, 30.0 * sz]) + rng.normal(0, 0.12, (80, 3)))
    return np.concatenate(parts, 0).astype(np.float32)


def row_cloud():
    """600 points of one grid row: x over [0.2, 5.2), y and z inside one cell of the radius-0.6 grid"""
    rng = np.random.default_rng(37)
    x = rng.uniform(0.2, 5.2, 600)
    y = rng.uniform(0.0, 0.25, 600)
    z = 0.1 * x + rng.uniform(0.0, 0.3, 600)
    return np.stack([x, y, z], 1).astype(np.float32)


def kernel_cells(xyz, radius):
    """(cx, cy, cz) of every point by the kernel's own fp32 formula: floorf((v + org) * inv), clamped (nm_cell1)"""
    f = np.float32
    r = f(radius)
    inv_xy = f(1) / np.maximum(f(0.625), r * f(1.0625))
    inv_z = f(1) / np.maximum(f(2.5), r * f(1.0625))
    cx = np.clip(np.floor((xyz[:, 0] + f(80)) * inv_xy), 0, 255)
    cy = np.clip(np.floor((xyz[:, 1] + f(80)) * inv_xy), 0, 255)
    cz = np.clip(np.floor((xyz[:, 2] + f(10)) * inv_z), 0, 7)
    assert cx.dtype == np.float32 and cz.dtype == np.float32
    return cx.astype(np.int64), cy.astype(np.int64), cz.astype(np.int64)


def _normal64(p, q, sel):
    o = p[sel] - q
    w, v = np.linalg.eigh(np.cov(o.T, bias=True))
    return v[:, 0]


@pytest.mark.parametrize("radius,max_nn", HOST_PAIRS)
@pytest.mark.parametrize("name", ["small", "scan", "patch"])
def test_twin_against_float64(name, radius, max_nn):
    xyz = cloud(name)
    n, c, s = twin(name, radius, max_nn)
    rn, rc, gap, amb, rs = ref64(name, radius, max_nn)
    assert n.dtype == np.float32 and c.dtype == np.int32 and s.dtype == np.int64 and s.shape == (len(xyz), max_nn)
    clear = ~amb
    print("%s r=%g k=%d: %d ambiguous, %d counts differ on them, %d at the cap, %d under 3"
          % (name, radius, max_nn, amb.sum(), (c != rc)[amb].sum(), (c == max_nn).sum(), (c < 3).sum()))
    assert np.array_equal(c[clear], rc[clear])
    assert np.array_equal((s >= 0).sum(1), c)
    # the neighbour SET (inside it two fp32 distances a rounding apart may swap places against float64)
    assert np.array_equal(np.sort(s[clear], 1), np.sort(rs[clear], 1))
    # in key order the query itself comes first: d2 = 0 and, among duplicates, the lowest index
    d0 = (xyz[np.maximum(s[:, 0], 0)] == xyz).all(1)
    assert d0.all() and (s[:, 0] <= np.arange(len(xyz))).all()
    chk = clear & (rc >= 3) & (gap >= GAP_MIN)
    dot = (n[chk].astype(np.float64) * rn[chk]).sum(1)
    ang = np.arccos(np.clip(np.abs(dot), 0.0, 1.0))
    print("angle on %d points: max %.4f deg" % (chk.sum(), np.rad2deg(ang.max())))
    assert chk.sum() >= 500 and ang.max() <= ANGLE_BAR          # never vacuous: at least 500 points are checked
    firm = np.abs((rn[chk] * -xyz[chk].astype(np.float64)).sum(1)) / np.linalg.norm(xyz[chk], axis=1) > 1e-3
    assert (dot[firm] > 0).all()


def test_twin_cases_reach_the_cap_and_the_fallback():
    """what tests/test_gpu_normals_exact.py relies on: the eviction path and the fallback are populated"""
    assert (twin("scan", 0.6, 30)[1] == 30).sum() > 1000
    assert (twin("small", 0.6, 30)[1] < 3).sum() > 100
    assert (twin("small", 0.6, 30)[1] == 30).sum() == 0          # why `small` alone never tested the eviction


def test_twin_rules():
    pts = np.array([[5.0, 0.0, 1.0], [0.0, 7.0, -1.0], [-9.0, -3.0, -2.0], [np.nan, 0.0, 0.0], [1.0, np.inf, 0.0]], np.float32)
    n, c, s = normals.estimate_normals_f32(pts, 0.6, 30)
    assert c.tolist() == [1, 1, 1, 0, 0] and s[:, 0].tolist() == [0, 1, 2, -1, -1] and (s[:, 1:] == -1).all()
    assert n.tolist() == [[0, 0, -1], [0, 0, 1], [0, 0, 1], [0, 0, 0], [0, 0, 0]]
    n, _, _ = normals.estimate_normals_f32(pts, 0.6, 30, zero_vertical=True)
    assert (n == 0).all() and not np.signbit(n).any()
    n, c, s = normals.estimate_normals_f32(np.zeros((0, 3), np.float32))
    assert n.shape == (0, 3) and c.shape == (0,) and s.shape == (0, 30)
    with pytest.raises(ValueError):
        normals.estimate_normals_f32(pts, 0.6, 33)


@pytest.mark.parametrize("max_nn,slots", [(30, 5), (27, 2)])
def test_tie_cloud_preconditions(max_nn, slots):
    xyz = tie_cloud()
    p = xyz.astype(np.float64)
    q = p[TIE_QUERY]
    # mirrored squared distances are bit-equal in fp32, computed as the kernel does
    d = xyz[:EDGE_QUERY] - xyz[TIE_QUERY]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert d2.dtype == np.float32
    r2 = np.float32(TIE_RADIUS) * np.float32(TIE_RADIUS)
    tied = np.float32(625.0 / 4096.0)
    assert (d2[:25] < tied).all() and (d2[25:] == tied).all() and tied < r2
    assert 25 < max_nn and 25 + slots == max_nn and slots < 8
    assert (np.abs(p[25:33, 2] - q[2]) == 0).all() and (np.abs(p[33:41, 2] - q[2]) >= 15.0 / 64).all()
    d264 = ((p[:EDGE_QUERY] - q) ** 2).sum(1)
    low = sorted(range(EDGE_QUERY), key=lambda j: (d264[j], j))[:max_nn]
    high = sorted(range(EDGE_QUERY), key=lambda j: (d264[j], -j))[:max_nn]
    assert sorted(low) == list(range(25 + slots)) and sorted(high) == list(range(25)) + list(range(41 - slots, 41))
    ang = np.rad2deg(np.arccos(min(1.0, abs(float(_normal64(p, q, low) @ _normal64(p, q, high))))))
    print("max_nn %d: the two tie rules differ by %.1f deg" % (max_nn, ang))
    assert ang >= 10.0
    n, c, s = normals.estimate_normals_f32(xyz, TIE_RADIUS, max_nn)
    assert c[TIE_QUERY] == max_nn and s[TIE_QUERY].tolist() == low            # the twin: lower index wins
    got = np.rad2deg(np.arccos(min(1.0, abs(float(n[TIE_QUERY].astype(np.float64) @ _normal64(p, q, low))))))
    assert got < 0.1, got
    # a candidate whose fp32 d2 equals r2 bit for bit is outside (strict <)
    e = xyz[EDGE_QUERY:] - xyz[EDGE_QUERY]
    e2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    assert (e2[:4] < r2).all() and (e2[4:].view(np.int32) == r2.view(np.int32)).all()
    assert c[EDGE_QUERY] == 4 and sorted(s[EDGE_QUERY, :4].tolist()) == [41, 42, 43, 44]


def test_corner_and_row_cloud_preconditions():
    xyz = corner_cloud()
    cx, cy, cz = kernel_cells(xyz, 0.6)
    key = (cz * 256 + cy) * 256 + cx
    assert (key[:80] == 0).all() and (key[-80:] == 256 * 256 * 8 - 1).all() and len(np.unique(key)) == 8
    assert (np.abs(xyz[:, 0]) > 140).all() and (np.abs(xyz[:, 2]) > 25).all()
    _, c, _ = normals.estimate_normals_f32(xyz, 0.6, 30)
    assert all((c[k * 80:(k + 1) * 80] == 30).any() for k in range(8))
    xyz = row_cloud()
    cx, cy, cz = kernel_cells(xyz, 0.6)
    assert len(np.unique(cy)) == 1 and len(np.unique(cz)) == 1
    cells = np.unique(cx)
    assert len(cells) >= 6 and np.array_equal(cells, np.arange(cells[0], cells[0] + len(cells)))
    _, c, s = normals.estimate_normals_f32(xyz, 0.6, 30)
    ncx = np.where(s >= 0, cx[np.maximum(s, 0)], cx[:, None])
    left, right = (ncx < cx[:, None]).any(1).sum(), (ncx > cx[:, None]).any(1).sum()
    print("row cloud: %d queries select from the cell to the left, %d to the right, %d at the cap" % (left, right, (c == 30).sum()))
    assert left >= 50 and right >= 50 and (np.abs(ncx - cx[:, None]) <= 1).all()
