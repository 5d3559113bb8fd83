"""Streaming odometry on the GPU: the eval-BatchNorm epilogues of the dense convolutions, the pose-chain kernel and
rslo_amd.inference.OdometryRunner against the eager eval forward of the same network."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from stream_support import odom_fixture

pytestmark = pytest.mark.gpu

ERR_BAR = 2e-5          # max|err| / max|ref| of the dense convolution kernels against float64 (the existing conv bar)


def _ref_conv_bn(x, w, bias, g, b, m, v, eps, stride, res, slope):
    k = w.shape[2]
    y = F.conv2d(x.double().cpu(), w.double().cpu(), None if bias is None else bias.double().cpu(), stride, k // 2)
    y = F.batch_norm(y, m.double().cpu(), v.double().cpu(), g.double().cpu(), b.double().cpu(), False, 0.0, eps)
    if res is not None:
        y = y + res.double().cpu()
    if slope is not None:
        y = F.leaky_relu(y, slope) if slope != 0.0 else F.relu(y)
    return y


def _bn_params(C, gen):
    g = torch.rand(C, generator=gen) + 0.5
    b = torch.randn(C, generator=gen) * 0.3
    m = torch.randn(C, generator=gen) * 0.2
    v = torch.rand(C, generator=gen) + 0.2
    return [t.cuda() for t in (g, b, m, v)]


# (cin, cout, H, W) of the head's stride-1 layers and the epilogue options each is checked with: every shape with a
# different (residual, activation) pair, and all six pairs on two shapes
S1_CASES = [(c, o, H, W, res, slope)
            for (c, o, H, W) in [(64, 64, 96, 176), (128, 128, 48, 88), (256, 64, 48, 88), (128, 128, 24, 44),
                                 (512, 128, 24, 44), (256, 256, 12, 22), (64, 32, 96, 176)]
            for res in (False, True) for slope in (None, 0.0, 1e-3)
            if (c, o, H) in [(128, 128, 24), (256, 256, 12)] or (res, slope) in [(False, 0.0), (True, 0.0), (False, None)]]


@pytest.mark.parametrize("cin,cout,H,W,res,slope", S1_CASES)
def test_conv2d_fwd_bn_epilogue(cin, cout, H, W, res, slope):
    from rslo_amd import capi
    from rslo.layers import hip_conv2d
    gen = torch.Generator().manual_seed(cin * 7 + cout + H)
    x = torch.randn(1, cin, H, W, generator=gen).cuda()
    w = (torch.randn(cout, cin, 3, 3, generator=gen) / (3.0 * cin ** 0.5)).cuda()
    bias = (torch.randn(cout, generator=gen) * 0.1).cuda()
    g, b, m, v = _bn_params(cout, gen)
    r = torch.randn(1, cout, H, W, generator=gen).cuda() if res else None
    sc, sh = hip_conv2d.fold_bn_host(g, b, m, v, 1e-3)
    out = capi.conv2d_fwd_bn(x, capi.conv2d_wsplit(w, False), bias, sc.contiguous(), sh.contiguous(), cout, r, slope)
    ref = _ref_conv_bn(x, w, bias, g, b, m, v, 1e-3, 1, r, slope)
    err = (out.double().cpu() - ref).abs().max().item() / ref.abs().max().item()
    assert err < ERR_BAR, err


S2_CASES = [(256, 128, 96, 176, 3, False, 0.0), (256, 128, 96, 176, 1, False, None), (128, 128, 48, 88, 3, True, 1e-3),
            (128, 128, 48, 88, 1, True, None), (128, 256, 24, 44, 3, False, 0.0), (128, 256, 24, 44, 1, False, None),
            (64, 64, 13, 21, 3, True, 0.0), (64, 128, 21, 37, 1, True, 1e-3)]


@pytest.mark.parametrize("cin,cout,H,W,k,res,slope", S2_CASES)
def test_conv2d_fwd_s2_bn_epilogue(cin, cout, H, W, k, res, slope):
    from rslo_amd import capi
    from rslo.layers import hip_conv2d
    gen = torch.Generator().manual_seed(cin + cout * 3 + H + k)
    x = torch.randn(2, cin, H, W, generator=gen).cuda()
    w = (torch.randn(cout, cin, k, k, generator=gen) / (k * cin ** 0.5)).cuda()
    bias = (torch.randn(cout, generator=gen) * 0.1).cuda() if res else None
    g, b, m, v = _bn_params(cout, gen)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    r = torch.randn(2, cout, Ho, Wo, generator=gen).cuda() if res else None
    sc, sh = hip_conv2d.fold_bn_host(g, b, m, v, 1e-3)
    out = capi.conv2d_fwd_s2_bn(x, capi.conv2d_wsplit_k(w, False), bias, sc.contiguous(), sh.contiguous(), cout, k, r, slope)
    ref = _ref_conv_bn(x, w, bias, g, b, m, v, 1e-3, 2, r, slope)
    assert out.shape == ref.shape
    err = (out.double().cpu() - ref).abs().max().item() / ref.abs().max().item()
    assert err < ERR_BAR, err


def test_bn_fold_many_reads_live_storage():
    from rslo_amd import capi
    from rslo.layers import hip_conv2d
    from rslo.layers.SparseConv import SPC_SyncBN2d
    bns = [SPC_SyncBN2d(c, eps=1e-3).cuda().eval() for c in (32, 64, 256)]
    gen = torch.Generator().manual_seed(5)
    for bn in bns:
        for t, (lo, sc) in zip((bn.weight.data, bn.bias.data, bn.running_mean, bn.running_var),
                               ((0.5, 1.0), (0.0, 0.3), (0.0, 0.2), (0.2, 1.0))):
            t.copy_(torch.rand(t.shape, generator=gen) * sc + lo)
    plan, views = capi.bn_fold_many(bns)
    capi.bn_fold_run(plan)
    bns[1].running_var.mul_(1.5)          # an in-place change: the next launch sees it
    capi.bn_fold_run(plan)
    for bn, (sc, sh) in zip(bns, views):
        rs, rh = hip_conv2d.fold_bn_host(bn.weight.data, bn.bias.data, bn.running_mean, bn.running_var, bn.eps)
        assert torch.allclose(sc, rs, rtol=1e-6, atol=0) and torch.allclose(sh, rh, rtol=1e-6, atol=1e-7)


def test_pose_chain_kernel_1000_steps():
    from rslo_amd import capi, inference
    from rslo.utils import geometric
    rng = np.random.default_rng(17)
    n = 1000
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    rows = np.concatenate([rng.normal(size=(n, 3)), q], 1).astype(np.float32)
    dev = torch.device("cuda")
    state = torch.zeros(7, dtype=torch.float64, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    rel = torch.zeros((n, 7), dtype=torch.float32, device=dev)
    traj = torch.zeros((n, 7), dtype=torch.float64, device=dev)
    rows_d = torch.from_numpy(rows).to(dev)
    for i in range(n):
        capi.pose_chain(rows_d[i, :3], rows_d[i, 3:], state, count, rel, traj)
    assert int(count.item()) == n
    assert torch.equal(rel.cpu(), torch.from_numpy(rows))
    ref = geometric.odom_to_abs_pose(rows.astype(np.float64))
    got = traj.cpu().numpy()
    assert np.abs(got - ref).max() < 1e-6, np.abs(got - ref).max()
    assert np.abs(got - inference.pose_chain_host(rows)).max() < 1e-9


# ---------------------------------------------------------------------------------------------------------------------
# the runner on the shipped eval configuration
# ---------------------------------------------------------------------------------------------------------------------
N_SCANS = 12


odom = odom_fixture(21, 3, N_SCANS)


def _eager_rel(net, a, b):
    from rslo_amd import workload
    with torch.no_grad():
        out = net(workload.make_example(net, [[a, b]]))
    return torch.cat([out["translation_preds"][0], out["rotation_preds"][0]]).double().cpu()


def _run_sequence(runner, scans, graph=True, keep_pairs=()):
    rels, pairs = [], {}
    hs = [runner.submit(scans[0])]
    for i in range(len(scans)):
        if i + 1 < len(scans):
            hs.append(runner.submit(scans[i + 1]))      # one scan ahead: its structure work beside this scan's pass
        rel, _ = runner.run(hs[i], graph=graph)
        rels.append(rel)
        if i in keep_pairs:
            pairs[i] = runner._pair.clone()
    return torch.stack(rels).double().cpu(), pairs


def test_runner_matches_eager_eval(odom):
    from rslo_amd import inference
    from rslo.utils import geometric
    net, scans = odom
    head = net.odom_predictor
    runner = inference.OdometryRunner(net)
    try:
        rel, pairs = _run_sequence(runner, scans, keep_pairs=(0, 5, 11))
        traj = runner.trajectory().cpu().numpy()
        st = dict(runner.stats)
        enc_runs, plans = runner.encoder.stats["runs"], runner.encoder.stats["plans"]
    finally:
        runner.close()
    # the encoder ran once per scan
    assert st["scans"] == N_SCANS and st["encoder_runs"] == N_SCANS and enc_runs == N_SCANS and plans == N_SCANS
    assert st["head_replays"] == N_SCANS and st["captures"] == 1
    # trajectory = odom_to_abs_pose of the returned rows
    ref_traj = geometric.odom_to_abs_pose(rel.numpy())
    assert np.abs(traj - ref_traj).max() < 1e-9
    # the eager eval forward of the pairs the dataset builds: (max(i-1, 0), i)
    eager = torch.stack([_eager_rel(net, scans[max(i - 1, 0)], scans[i]) for i in range(N_SCANS)])
    scale = eager.abs().max().item()
    d_eager = (rel - eager).abs().max().item() / scale
    # against a float64 CPU forward of the same head modules on the same pair maps: no further away than the eager GPU path
    h64 = copy.deepcopy(head).double().cpu()
    C = pairs[0].shape[1] // 2
    e_run, e_eager = [], []
    for i, p in pairs.items():
        with torch.no_grad():
            o64 = h64([p[:, :C].double().cpu(), p[:, C:].double().cpu()])
            og = head([p[:, :C], p[:, C:]])
        r64 = torch.cat([o64["translation_preds"][0][0], o64["rotation_preds"][0][0]])
        rg = torch.cat([og["translation_preds"][0][0], og["rotation_preds"][0][0]]).double().cpu()
        s = r64.abs().max().item()
        e_run.append((rel[i] - r64).abs().max().item() / s)
        e_eager.append((rg - r64).abs().max().item() / s)
    # floor: fp32 rounding of a ~50-layer forward through the softmax-weighted vote; measured on MI355X, relative to
    # max|pose|: runner 5.9e-6 / 5.5e-6 / 4.4e-5, eager GPU 3.6e-6 / 3.2e-6 / 4.2e-5 on the three pairs
    floor = 1e-4
    print("odometry runner vs eager eval: max rel diff %.3g; vs float64 CPU head: runner %s, eager GPU %s"
          % (d_eager, ["%.3g" % e for e in e_run], ["%.3g" % e for e in e_eager]))
    for er, ee in zip(e_run, e_eager):
        assert er <= max(ee, floor), (er, ee)
    assert d_eager < 1e-3, d_eager


def test_replay_equals_eager_fused_path_and_reset(odom):
    from rslo_amd import inference
    net, scans = odom
    runner = inference.OdometryRunner(net)
    try:
        sub = scans[:5]
        rel_g, _ = _run_sequence(runner, sub, graph=True)
        runner.reset()
        rel_e, _ = _run_sequence(runner, sub, graph=False)
        assert torch.equal(rel_g, rel_e)          # replay == the same kernels issued eagerly, bit for bit
        # after reset() the first scan pairs with itself and the trajectory restarts at the identity
        runner.reset()
        h = runner.submit(scans[7])
        rel, pose = runner.run(h)
        C = runner._pair.shape[1] // 2
        assert torch.equal(runner._pair[:, :C], runner._pair[:, C:])
        assert pose.cpu().tolist() == [0, 0, 0, 1, 0, 0, 0] and runner.trajectory().shape[0] == 1
        self_pair = _eager_rel(net, scans[7], scans[7])
        assert (rel.double().cpu() - self_pair).abs().max().item() / self_pair.abs().max().item() < 1e-3
    finally:
        runner.close()


def test_inplace_running_var_change_reaches_the_next_pose(odom):
    from rslo_amd import inference
    net, scans = odom
    bn = net.odom_predictor.tq_map_conv[1]
    saved = bn.running_var.clone()
    runner = inference.OdometryRunner(net)
    try:
        rel0, _ = _run_sequence(runner, scans[:2])
        bn.running_var.mul_(1.7)                     # in place: version counter bumped, storage unchanged
        runner.reset()
        rel1, _ = _run_sequence(runner, scans[:2])
        assert runner.stats["captures"] == 1 and runner.stats["weight_refreshes"] == 2
        assert (rel1[1] - rel0[1]).abs().max().item() > 1e-4
        eager = _eager_rel(net, scans[0], scans[1])
        assert (rel1[1] - eager).abs().max().item() / eager.abs().max().item() < 1e-3
    finally:
        runner.close()
        with torch.no_grad():
            bn.running_var.copy_(saved)


def test_pyramid_block_fused_eval_matches_eager(odom):
    from rslo.layers import hip_conv2d
    net, _ = odom
    head = net.odom_predictor
    ops = hip_conv2d.EvalOperands(head)
    ops.refresh()
    gen = torch.Generator().manual_seed(2)
    for blk, (c, H, W) in zip(head.pyramid_motion_blocks, [(128, 24, 44), (64, 48, 88)]):
        x = torch.relu(torch.randn(1, c, H, W, generator=gen)).cuda()
        with torch.no_grad():
            ref = blk(x)
            got = blk.forward_eval_fused(x)
        assert (got - ref).abs().max().item() / ref.abs().max().item() < 1e-4


def test_unsupported_configuration_raises(odom):
    from rslo_amd import capi, inference
    net, _ = odom
    head = net.odom_predictor
    head.use_svd = True
    try:
        with pytest.raises(capi.RsloHipError, match="use_svd"):
            inference.OdometryRunner(net)
    finally:
        head.use_svd = False
