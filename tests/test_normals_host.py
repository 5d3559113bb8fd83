"""Point normals without a GPU: the float64 restatement rslo_amd/normals.py of the rules the kernel implements
(include/rslo_hip.h), an independent neighbour search, and the C-ABI / Python bindings of the new entry points."""
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
