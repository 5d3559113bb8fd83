"""Point normals on the GPU (csrc/normals.hip) against their fp32 twin rslo_amd.normals.estimate_normals_f32.

The bar is BIT equality on every point, with no ambiguity mask and no excluded point: counts equal, normals equal viewed
as int32.  It follows from how the kernel is written, not from what it returns: fp contract(off), no fast-math, every
operation one correctly rounded fp32 + - * / or sqrtf, a total selection key (d2 bits << 32 | index) and sums formed in
key order, all of which the twin restates operation by operation in numpy float32.  The twin itself is held to the
float64 reference on the CPU (tests/test_normals_host.py), where the constructed clouds' preconditions are asserted too.
The float64 tests of tests/test_gpu_normals.py stay as they are.
"""
import numpy as np
import pytest
import torch

from rslo_amd import normals
from test_normals_host import (EDGE_QUERY, TIE_QUERY, TIE_RADIUS, cloud, corner_cloud, kernel_cells, row_cloud, tie_cloud,
                               twin)

pytestmark = pytest.mark.gpu

# (0.25, 30): the 0.625 m minimum cell edge; 0.58 / 0.59: either side of the xy cell-edge switch at 0.588; (2.5, 16):
# above the z cell-edge switch at 2.353; max_nn 3 and 32: the bounds of the truncation of the 32-entry list
PAIRS = [(0.6, 30), (0.6, 3), (0.6, 32), (0.25, 30), (0.58, 30), (0.59, 30), (2.5, 16)]


def _run(xyz, radius, max_nn, **kw):
    from rslo_amd import capi
    pts = torch.from_numpy(np.array(xyz, np.float32, order="C")).cuda()          # a copy: the shared clouds are read-only
    n, c = capi.estimate_normals(pts, radius, max_nn, **kw)
    torch.cuda.synchronize()
    return n.cpu().numpy(), c.cpu().numpy()


def _assert_bits(got, want, label=""):
    n, c = got
    wn, wc = want[0], want[1]
    assert n.dtype == np.float32 and wn.dtype == np.float32 and n.shape == wn.shape
    bad_c = np.nonzero(c != wc)[0]
    bad_n = np.nonzero((n.view(np.int32) != wn.view(np.int32)).any(1))[0]
    if bad_n.size:
        dot = np.abs((n[bad_n].astype(np.float64) * wn[bad_n]).sum(1))
        worst = np.rad2deg(np.arccos(np.clip(dot, 0.0, 1.0)).max())
    else:
        worst = 0.0
    print("%s: %d points, %d at the cap, %d under 3; counts differ on %d, normals on %d (largest angle %.5f deg)"
          % (label, len(wc), (wc == want[2].shape[1]).sum(), (wc < 3).sum(), bad_c.size, bad_n.size, worst))
    assert bad_c.size == 0, (bad_c[:10], c[bad_c[:10]], wc[bad_c[:10]])
    assert bad_n.size == 0, (bad_n[:10], n[bad_n[:10]], wn[bad_n[:10]])


@pytest.mark.parametrize("radius,max_nn", PAIRS)
@pytest.mark.parametrize("name", ["small", "scan", "patch"])
def test_cloud_equals_twin(name, radius, max_nn):
    want = twin(name, radius, max_nn)
    if (name, radius, max_nn) == ("scan", 0.6, 30):
        assert (want[1] == 30).sum() > 1000              # the eviction path of the 32-entry list
    if (name, radius, max_nn) == ("small", 0.6, 30):
        assert (want[1] < 3).sum() > 100                 # the fallback
    if max_nn == 3 or radius == 2.5:
        assert (want[1] == max_nn).sum() > 1000
    _assert_bits(_run(cloud(name), radius, max_nn), want, "%s r=%g k=%d" % (name, radius, max_nn))


@pytest.mark.parametrize("N", [1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1025])
def test_sizes(N):
    """the padded tail in every wave of a 256-query workgroup, and the whole-wave exit qt * 64 >= Npad"""
    scale = 0.01 if N <= 3 else (0.05 if N <= 257 else 0.25)       # shrunk so that the first N points are neighbours
    xyz = (cloud("small")[:N] * np.float32(scale)).astype(np.float32)
    want = normals.estimate_normals_f32(xyz, 0.6, 30)
    if N == 3:
        assert want[1].tolist() == [3, 3, 3]
    if N >= 63:
        assert (want[1] == 30).any() and (want[1] >= 3).all()
    _assert_bits(_run(xyz, 0.6, 30), want, "N=%d" % N)


@pytest.mark.parametrize("max_nn", [30, 27])
def test_tie_at_the_cap(max_nn):
    """equal squared distance goes to the lower original index (preconditions: test_tie_cloud_preconditions); the other
    rule moves the query's normal by 60 / 80 deg.  The same cloud holds candidates whose d2 equals r2 bit for bit."""
    xyz = tie_cloud()
    want = normals.estimate_normals_f32(xyz, TIE_RADIUS, max_nn)
    assert want[1][TIE_QUERY] == max_nn and want[2][TIE_QUERY].max() == max_nn - 1      # indices 0 .. max_nn-1: in the plane
    assert want[1][EDGE_QUERY] == 4
    got = _run(xyz, TIE_RADIUS, max_nn)
    _assert_bits(got, want, "tie k=%d" % max_nn)
    assert got[1][EDGE_QUERY] == 4


def test_grid_corners():
    """clusters clamped into all eight corner cells: the (+,+,+) one is the grid's last row, where the end of the candidate
    range is N and not an offset (k1 == NM_BINS); the (-,-,-) one is key 0"""
    xyz = corner_cloud()
    cx, cy, cz = kernel_cells(xyz, 0.6)
    assert (cx[-80:] == 255).all() and (cy[-80:] == 255).all() and (cz[-80:] == 7).all()
    assert (cx[:80] == 0).all() and (cy[:80] == 0).all() and (cz[:80] == 0).all()
    want = normals.estimate_normals_f32(xyz, 0.6, 30)
    assert all((want[1][k * 80:(k + 1) * 80] == 30).any() for k in range(8))
    _assert_bits(_run(xyz, 0.6, 30), want, "corners")


def test_one_grid_row_along_x():
    """neighbour sets that cross cell boundaries along x on both sides: the NM_WIN grouping and its lo / hi window"""
    xyz = row_cloud()
    cx, cy, cz = kernel_cells(xyz, 0.6)
    assert len(np.unique(cy)) == 1 and len(np.unique(cz)) == 1 and len(np.unique(cx)) >= 6
    want = normals.estimate_normals_f32(xyz, 0.6, 30)
    ncx = np.where(want[2] >= 0, cx[np.maximum(want[2], 0)], cx[:, None])
    assert (ncx < cx[:, None]).any(1).sum() >= 50 and (ncx > cx[:, None]).any(1).sum() >= 50
    _assert_bits(_run(xyz, 0.6, 30), want, "row")


def test_viewpoint_and_zero_vertical():
    xyz = cloud("small")
    view = (1.5, -2.25, 3.0)
    want = normals.estimate_normals_f32(xyz, 0.6, 30, viewpoint=view, zero_vertical=True)
    plain = twin("small", 0.6, 30)
    assert (want[0] != plain[0]).any(1).sum() > 100                  # the viewpoint flips some, the rule zeroes others
    assert ((want[0] == 0).all(1) & (want[1] < 3)).sum() > 100
    _assert_bits(_run(xyz, 0.6, 30, viewpoint=view, zero_vertical=True), want, "viewpoint")
