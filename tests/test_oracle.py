"""Pins the CPU oracle (oracle/rslo_oracle.c) -- no GPU needed.

  * chamfer NN   : bit-exact vs oracle/_ref (the reference's chamfer_distance.cpp compiled from
                   /root/reference) when that build is present, vs committed golden vectors, and
                   vs torch.cdist.
  * sparse conv  : no reference source exists (spconv_plus is not in the tree).  Arbiter = dense
                   F.conv3d / conv_transpose3d on the densified tensor sampled at the active sites
                   ("known-answer material" (i)).
  * voxelizer    : hand-made known-answer clouds (first-come ids, T truncation, max_voxels break).
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle as O

GOLD = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, GOLD)
import make_golden_chamfer_build  # noqa: E402  (the recorded cases and how the reference build is called)


def rand_sites(rng, batch, dims, n):
    vol = batch * dims[0] * dims[1] * dims[2]
    lin = rng.choice(vol, size=min(n, vol), replace=False)
    rng.shuffle(lin)
    x = lin % dims[2]; r = lin // dims[2]
    y = r % dims[1]; r //= dims[1]
    z = r % dims[0]; b = r // dims[0]
    return np.stack([b, z, y, x], 1).astype(np.int32)


def densify(feat, coords, batch, dims):
    return torch.from_numpy(O.dense(feat, coords, batch, dims))


# ------------------------------------------------------------------------------- voxelizer
def test_voxelize_known_answer():
    rng_ = [0, 0, 0, 4, 4, 2]
    vs = [1.0, 1.0, 1.0]
    pts = np.array([
        [0.5, 0.5, 0.5, 1],   # voxel A (0,0,0)  -> id 0
        [3.5, 0.5, 0.5, 2],   # voxel B (x=3)    -> id 1
        [0.6, 0.4, 0.5, 3],   # A again
        [9.0, 0.5, 0.5, 4],   # out of range
        [0.5, 2.5, 1.5, 5],   # voxel C (z=1,y=2,x=0) -> id 2
        [0.1, 0.9, 0.9, 6],   # A third point (dropped, T=2)
        [3.9, 0.1, 0.1, 7],   # B again
        [-0.01, 0.5, 0.5, 8],  # just below range
    ], np.float32)
    v, c, n = O.voxelize(pts, rng_, vs, max_points=2, max_voxels=10)
    assert c.tolist() == [[0, 0, 0], [0, 0, 3], [1, 2, 0]]
    assert n.tolist() == [2, 2, 1]
    assert v[0, :, 3].tolist() == [1, 3] and v[1, :, 3].tolist() == [2, 7] and v[2, :, 3].tolist() == [5, 0]


def test_voxelize_max_voxels_breaks():
    pts = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [2.5, 0.5, 0.5], [0.6, 0.5, 0.5]], np.float32)
    v, c, n = O.voxelize(pts, [0, 0, 0, 4, 4, 2], [1, 1, 1], max_points=5, max_voxels=2)
    # the third point would open voxel #2 -> the loop stops; the 4th point (voxel 0) is never seen
    assert len(c) == 2 and n.tolist() == [1, 1]


def test_voxelize_empty_and_grid_size():
    v, c, n = O.voxelize(np.zeros((0, 7), np.float32), [0, 0, 0, 4, 4, 2], [1, 1, 1], 5, 8)
    assert v.shape == (0, 5, 7) and c.shape == (0, 3)
    assert O.grid_size([-70.4, -38.4, -3, 70.4, 38.4, 5], [0.1, 0.1, 0.2]).tolist() == [1408, 768, 40]


# ------------------------------------------------------------------------------- rulebooks
def test_subm_rulebook_known_answer():
    coords = np.array([[0, 1, 1, 1], [0, 1, 1, 2], [0, 0, 0, 0], [1, 1, 1, 1]], np.int32)
    nbr = O.rulebook_subm(coords, 2, [3, 3, 3])
    assert nbr[0, 13] == 0 and nbr[1, 13] == 1 and nbr[3, 13] == 3
    assert nbr[0, 14] == 1            # +x neighbour of row 0 is row 1
    assert nbr[1, 12] == 0            # -x neighbour of row 1 is row 0
    assert nbr[0, 0] == 2             # (-1,-1,-1) of (1,1,1) is (0,0,0)
    assert nbr[2, 26] == 0
    assert (nbr[3] >= 0).sum() == 1   # other batch: only itself
    # symmetry used by the SubM dgrad: pair (i -> o via k) <=> (o -> i via K-1-k)
    for o in range(4):
        for k in range(27):
            i = nbr[o, k]
            if i >= 0:
                assert nbr[i, 26 - k] == o


def test_conv_rulebook_order_and_tables():
    rng = np.random.default_rng(0)
    dims = [9, 12, 10]
    coords = rand_sites(rng, 2, dims, 150)
    oc, od, nbr, nbrT = O.rulebook_conv(coords, 2, dims, [3, 3, 3], [2, 2, 2], [1, 1, 1])
    assert od == [5, 6, 5]
    lin = ((oc[:, 0] * od[0] + oc[:, 1]) * od[1] + oc[:, 2]) * od[2] + oc[:, 3]
    assert (np.diff(lin) > 0).all(), "outputs must be in ascending linear order"
    # nbr / nbrT are transposes of each other
    pairs_a = {(int(nbr[o, k]), o, k) for o in range(len(oc)) for k in range(27) if nbr[o, k] >= 0}
    pairs_b = {(i, int(nbrT[i, k]), k) for i in range(len(coords)) for k in range(27) if nbrT[i, k] >= 0}
    assert pairs_a == pairs_b and len(pairs_a) > 0
    # geometry of every pair: in = out*stride - pad + k
    for (i, o, k) in list(pairs_a)[:200]:
        kz, ky, kx = k // 9, (k // 3) % 3, k % 3
        assert coords[i, 0] == oc[o, 0]
        assert (coords[i, 1:] == oc[o, 1:] * 2 - 1 + np.array([kz, ky, kx])).all()
    # spconv-style export
    pairs, num = O.pairs_from_nbrT(nbrT)
    assert num.sum() == len(pairs_a)
    for k in range(27):
        assert (np.diff(pairs[k, 0, :num[k]]) > 0).all()


# ----------------------------------------------------------------- sparse conv vs dense conv
@pytest.mark.parametrize("cin,cout", [(7, 16), (16, 7), (32, 64)])
def test_subm_conv_equals_dense_conv3d(cin, cout):
    rng = np.random.default_rng(1)
    dims, B = [6, 9, 8], 2
    coords = rand_sites(rng, B, dims, 120)
    x = rng.normal(size=(len(coords), cin)).astype(np.float32)
    W = (rng.normal(size=(27, cin, cout)) * 0.2).astype(np.float32)
    b = rng.normal(size=(cout,)).astype(np.float32)
    nbr = O.rulebook_subm(coords, B, dims)
    y = O.spconv_fwd(x, W, b, nbr)
    xd = densify(x, coords, B, dims)
    wt = torch.from_numpy(W).reshape(3, 3, 3, cin, cout).permute(4, 3, 0, 1, 2).contiguous()
    yd = F.conv3d(xd.double(), wt.double(), torch.from_numpy(b).double(), padding=1)
    ys = yd[coords[:, 0], :, coords[:, 1], coords[:, 2], coords[:, 3]].float().numpy()
    np.testing.assert_allclose(y, ys, rtol=1e-5, atol=1e-5)


def test_strided_and_inverse_conv_equal_dense():
    rng = np.random.default_rng(2)
    dims, B, cin, cout = [9, 10, 12], 2, 16, 32
    ks, st, pd = [3, 3, 3], [2, 2, 2], [0, 1, 1]
    coords = rand_sites(rng, B, dims, 200)
    x = rng.normal(size=(len(coords), cin)).astype(np.float32)
    W = (rng.normal(size=(27, cin, cout)) * 0.2).astype(np.float32)
    oc, od, nbr, nbrT = O.rulebook_conv(coords, B, dims, ks, st, pd)
    y = O.spconv_fwd(x, W, None, nbr)
    xd = densify(x, coords, B, dims).double()
    wt = torch.from_numpy(W).reshape(3, 3, 3, cin, cout).permute(4, 3, 0, 1, 2).contiguous().double()
    yd = F.conv3d(xd, wt, None, stride=st, padding=pd)
    assert list(yd.shape[2:]) == od
    # active outputs = where the occupancy conv is positive
    occ = F.conv3d((xd.abs().sum(1, keepdim=True) > 0).double(), torch.ones(1, 1, 3, 3, 3).double(),
                   stride=st, padding=pd)
    assert int((occ > 0).sum()) == len(oc)
    ys = yd[oc[:, 0], :, oc[:, 1], oc[:, 2], oc[:, 3]].float().numpy()
    np.testing.assert_allclose(y, ys, rtol=1e-5, atol=1e-5)
    # inverse conv (SparseInverseConv3d): conv_transpose3d sampled at the saved input sites
    Wi = (rng.normal(size=(27, cout, 8)) * 0.2).astype(np.float32)
    z = O.spconv_fwd(y, Wi, None, nbrT)
    ydn = densify(y, oc, B, od).double()
    wti = torch.from_numpy(Wi).reshape(3, 3, 3, cout, 8).permute(3, 4, 0, 1, 2).contiguous().double()
    out_pad = [dims[i] - ((od[i] - 1) * st[i] - 2 * pd[i] + 3) for i in range(3)]
    zd = F.conv_transpose3d(ydn, wti, None, stride=st, padding=pd, output_padding=out_pad)
    zs = zd[coords[:, 0], :, coords[:, 1], coords[:, 2], coords[:, 3]].float().numpy()
    np.testing.assert_allclose(z, zs, rtol=1e-5, atol=1e-5)


def test_backward_matches_autograd_of_dense_conv():
    rng = np.random.default_rng(3)
    dims, B, cin, cout = [5, 7, 6], 1, 16, 16
    coords = rand_sites(rng, B, dims, 70)
    x = rng.normal(size=(len(coords), cin)).astype(np.float32)
    W = (rng.normal(size=(27, cin, cout)) * 0.2).astype(np.float32)
    gy = rng.normal(size=(len(coords), cout)).astype(np.float32)
    nbr = O.rulebook_subm(coords, B, dims)
    xd = densify(x, coords, B, dims).double().requires_grad_(True)
    wt = torch.from_numpy(W).reshape(3, 3, 3, cin, cout).permute(4, 3, 0, 1, 2).contiguous().double().requires_grad_(True)
    yd = F.conv3d(xd, wt, None, padding=1)
    ys = yd[coords[:, 0], :, coords[:, 1], coords[:, 2], coords[:, 3]]
    (ys * torch.from_numpy(gy).double()).sum().backward()
    gx_ref = xd.grad[coords[:, 0], :, coords[:, 1], coords[:, 2], coords[:, 3]].float().numpy()
    gw_ref = wt.grad.permute(2, 3, 4, 1, 0).reshape(27, cin, cout).float().numpy()
    # SubM: nbrT[i][k] = nbr[i][K-1-k]
    nbrT = nbr[:, ::-1].copy()
    gx = O.spconv_dgrad(gy, W, nbrT)
    gw, gb = O.spconv_wgrad(x, gy, nbr, cin, cout)
    np.testing.assert_allclose(gx, gx_ref, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(gw, gw_ref, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(gb, gy.sum(0), rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------- chamfer
def _ref_module():
    from oracle import build_ref
    return build_ref.load()


def test_chamfer_matches_reference_build_bitexact():
    """The oracle against the reference's chamfer CPU path on random inputs with exact hits / ties: against its outputs
    recorded in tests/golden/chamfer_build_ref.npz (make_golden_chamfer_build.py) always, against the live build in
    oracle/_ref where it is present."""
    g = np.load(os.path.join(GOLD, "chamfer_build_ref.npz"))
    ref = _ref_module()
    for k in range(3):
        a, c, gd = g["a%d" % k], g["c%d" % k], g["gd%d" % k]
        outs = [tuple(g["%s%d" % (f, k)] for f in ("dist1_", "idx1_", "gradxyz1_", "gradxyz2_"))]
        if ref is not None:
            outs.append(make_golden_chamfer_build.run(ref, a, c, gd))
        d, i = O.chamfer_nn(a, c)
        # backward (direction 1 only): zero grad for direction 2
        o1, o2 = O.chamfer_grad(a, c, gd, i)
        for d1, i1, g1, g2 in outs:
            assert (i == i1).all() and (d == d1).all()
            np.testing.assert_allclose(o1, g1, rtol=0, atol=0)
            np.testing.assert_allclose(o2, g2, rtol=1e-6, atol=1e-6)


def test_chamfer_golden_vectors():
    f = os.path.join(GOLD, "chamfer_ref.npz")
    g = np.load(f)
    d, i = O.chamfer_nn(g["xyz1"], g["xyz2"])
    assert (i == g["idx1"]).all() and (d == g["dist1"]).all()


def test_chamfer_golden_vectors_both_directions():
    """cd.forward / cd.backward (both directions, chamfer_distance.cpp:116-235) restated as two one-direction calls."""
    g = np.load(os.path.join(GOLD, "chamfer_ref.npz"))
    d2, i2 = O.chamfer_nn(g["xyz2"], g["xyz1"])
    assert (i2 == g["idx2"]).all() and (d2 == g["dist2"]).all()
    a1, a2 = O.chamfer_grad(g["xyz1"], g["xyz2"], g["graddist1"], g["idx1"])
    b2, b1 = O.chamfer_grad(g["xyz2"], g["xyz1"], g["graddist2"], g["idx2"])
    np.testing.assert_allclose(a1 + b1, g["gradxyz1_both"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(a2 + b2, g["gradxyz2_both"], rtol=1e-6, atol=1e-6)


def test_host_chamfer_entry_points_match_golden_vectors_and_reference_build():
    """cd.forward / cd.backward on HOST tensors (librslo_host.so: rslo_host_chamfer_forward / _backward, what the mirror's
    `cd` serves for CPU tensors like the reference's chamfer_distance.cpp:147-234): dist / idx of both directions bit-exact
    against the reference-generated vectors, both-direction gradients to rounding, and -- where oracle/_ref is built --
    against the reference's own functions on fresh inputs incl. ties; the two-direction autograd module on CPU tensors."""
    import rslo_amd  # noqa: F401
    from thirdparty.chamfer_distance.chamfer_distance import ChamferDistance, cd
    g = np.load(os.path.join(GOLD, "chamfer_ref.npz"))
    a, c = torch.from_numpy(g["xyz1"]), torch.from_numpy(g["xyz2"])
    b, n, m = a.shape[0], a.shape[1], c.shape[1]
    d1, d2 = torch.zeros(b, n), torch.zeros(b, m)
    i1, i2 = torch.zeros(b, n, dtype=torch.int32), torch.zeros(b, m, dtype=torch.int32)
    cd.forward(a, c, d1, d2, i1, i2)
    assert (i1.numpy() == g["idx1"]).all() and (d1.numpy() == g["dist1"]).all()
    assert (i2.numpy() == g["idx2"]).all() and (d2.numpy() == g["dist2"]).all()
    g1, g2 = torch.full((b, n, 3), 7.0), torch.full((b, m, 3), 7.0)      # overwritten, not accumulated into
    cd.backward(a, c, g1, g2, torch.from_numpy(g["graddist1"]), torch.from_numpy(g["graddist2"]), i1, i2)
    np.testing.assert_allclose(g1.numpy(), g["gradxyz1_both"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(g2.numpy(), g["gradxyz2_both"], rtol=1e-6, atol=1e-6)
    ref = _ref_module()
    if ref is not None:
        rng = np.random.default_rng(15)
        for (bb, nn, mm) in [(2, 333, 1025), (1, 1, 1), (1, 64, 3)]:
            x = torch.from_numpy(rng.normal(size=(bb, nn, 3)).astype(np.float32) * 10)
            y = torch.from_numpy(rng.normal(size=(bb, mm, 3)).astype(np.float32) * 10)
            y[:, : min(mm, 5)] = x[:, : min(mm, 5)][:, : min(mm, nn)] if nn >= min(mm, 5) else y[:, : min(mm, 5)]
            outs = []
            for fwd, bwd in ((ref.forward, ref.backward), (cd.forward, cd.backward)):
                e1, e2 = torch.zeros(bb, nn), torch.zeros(bb, mm)
                j1, j2 = torch.zeros(bb, nn, dtype=torch.int32), torch.zeros(bb, mm, dtype=torch.int32)
                fwd(x, y, e1, e2, j1, j2)
                gd1 = torch.from_numpy(np.random.default_rng(3).normal(size=(bb, nn)).astype(np.float32))
                gd2 = torch.from_numpy(np.random.default_rng(4).normal(size=(bb, mm)).astype(np.float32))
                h1, h2 = torch.zeros(bb, nn, 3), torch.zeros(bb, mm, 3)
                bwd(x, y, h1, h2, gd1, gd2, j1, j2)
                outs.append((e1, e2, j1, j2, h1, h2))
            for r_, o_ in zip(outs[0], outs[1]):
                assert torch.equal(r_, o_)          # the same loops in the same order: identical bits
    # the module on CPU tensors (chamfer_distance.py:34,61): autograd through the host entry points
    x = a[:, :200].clone().requires_grad_(True)
    y = c[:, :150].clone().requires_grad_(True)
    e1, e2 = ChamferDistance()(x, y)
    (e1.sum() + 2 * e2.sum()).backward()
    xd, yd = x.detach().double(), y.detach().double()
    dd = ((xd[:, :, None] - yd[:, None]) ** 2).sum(-1)
    np.testing.assert_allclose(e1.detach().numpy(), dd.min(2).values.numpy(), rtol=1e-5, atol=1e-6)
    assert x.grad is not None and y.grad is not None and float(x.grad.abs().sum()) > 0


def test_chamfer_vs_cdist_and_tie_break():
    rng = np.random.default_rng(6)
    a = rng.normal(size=(1, 400, 3)).astype(np.float32)
    c = rng.normal(size=(1, 300, 3)).astype(np.float32)
    d, i = O.chamfer_nn(a, c)
    ref = torch.cdist(torch.from_numpy(a).double(), torch.from_numpy(c).double()).argmin(-1).numpy()
    assert (i == ref).mean() > 0.999
    c2 = np.repeat(c[:, :10], 3, axis=1)  # duplicated targets: lowest index must win
    d2, i2 = O.chamfer_nn(a, c2)
    assert (i2 % 3 == 0).all()


@pytest.mark.parametrize("stride,H,W", [(1, 7, 9), (2, 7, 9), (2, 8, 10)])
def test_dense_conv2d_wgrad_restatement_matches_autograd(stride, H, W):
    """The numpy restatement of the BEV head's Conv2d weight gradient vs torch's own autograd (float64)."""
    import torch
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 5, H, W))
    w = torch.zeros((4, 5, 3, 3), dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv2d(torch.from_numpy(x), w, None, stride, 1)
    g = rng.standard_normal(tuple(y.shape))
    y.backward(torch.from_numpy(g))
    np.testing.assert_allclose(O.conv2d_wgrad(x, g, stride), w.grad.numpy(), rtol=1e-12, atol=1e-12)


def test_dense_conv2d_fwd_dgrad_restatement_matches_torch():
    import torch
    rng = np.random.default_rng(4)
    x = torch.from_numpy(rng.standard_normal((2, 5, 7, 9))).requires_grad_(True)
    w = torch.from_numpy(rng.standard_normal((4, 5, 3, 3)))
    bias = torch.from_numpy(rng.standard_normal(4))
    y = torch.nn.functional.conv2d(x, w, bias, 1, 1)
    g = rng.standard_normal(tuple(y.shape))
    y.backward(torch.from_numpy(g))
    np.testing.assert_allclose(O.conv2d_fwd(x.detach().numpy(), w.numpy(), bias.numpy()), y.detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(O.conv2d_dgrad(g, w.numpy()), x.grad.numpy(), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("k", [1, 3])
def test_stride2_conv_restatement_matches_torch_float64(k):
    """oracle.conv2d_s2_fwd / conv2d_s2_dgrad (the checkers of the stride-2 HIP kernels) against torch's own float64
    convolution and its autograd, even and odd map sizes."""
    import torch
    rng = np.random.default_rng(k)
    for H, W in ((12, 22), (13, 21)):
        x = rng.standard_normal((2, 5, H, W))
        w = rng.standard_normal((4, 5, k, k))
        tx = torch.from_numpy(x).requires_grad_(True)
        ty = torch.nn.functional.conv2d(tx, torch.from_numpy(w), None, 2, (k - 1) // 2)
        g = rng.standard_normal(tuple(ty.shape))
        ty.backward(torch.from_numpy(g))
        assert np.abs(O.conv2d_s2_fwd(x, w) - ty.detach().numpy()).max() < 1e-12
        assert np.abs(O.conv2d_s2_dgrad(g, w, H, W) - tx.grad.numpy()).max() < 1e-12
