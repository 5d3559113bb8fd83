"""Streaming odometry (rslo_amd.inference.OdometryRunner) on the host: the pose-chain recurrence of rslo_pose_chain, the
BatchNorm folding of rslo_bn_fold_many, the runner's configuration checks and the call order of OdometryRunner.feed, the
one submit-ahead loop, on a stand-in that only records submit() and run() (no GPU needed)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rslo_amd  # noqa: F401
from rslo_amd import capi, inference


def _random_rows(n, seed):
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    t = rng.normal(size=(n, 3)) * 0.8
    return np.concatenate([t, q], 1)


@pytest.mark.parametrize("n", [1, 2, 7, 300])
def test_pose_chain_recurrence_equals_odom_to_abs_pose(n):
    from rslo.utils import geometric
    rows = _random_rows(n, 11 + n)
    ref = geometric.odom_to_abs_pose(rows)
    got = inference.pose_chain_host(rows)
    assert got.shape == ref.shape == (n, 7)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12)
    # the quirk: scan 0 is the identity, and its own odometry seeds the chain (pose 1 = odom 0 o odom 1)
    assert (got[0] == [0, 0, 0, 1, 0, 0, 0]).all()
    if n > 1:
        rows2 = rows.copy()
        rows2[0, :3] += 1.0
        assert not np.allclose(inference.pose_chain_host(rows2)[1], got[1])


def test_bn_fold_matches_batch_norm_eval():
    from rslo.layers import hip_conv2d
    torch.manual_seed(3)
    C = 96
    x = torch.randn(2, C, 5, 7, dtype=torch.float64)
    g, b = torch.randn(C, dtype=torch.float64), torch.randn(C, dtype=torch.float64)
    m, v = torch.randn(C, dtype=torch.float64), torch.rand(C, dtype=torch.float64) + 0.05
    for eps, (gg, bb) in [(1e-3, (g, b)), (1e-5, (None, None))]:
        ref = F.batch_norm(x, m, v, gg, bb, False, 0.0, eps)
        sc, sh = hip_conv2d.fold_bn_host(gg, bb, m, v, eps)
        got = x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)
        assert torch.allclose(got, ref, rtol=0, atol=1e-12)


def _head(**over):
    from rslo.models import odom_pred
    kw = dict(num_input_features=32, layer_nums=[1, 1, 1], layer_strides=[2, 2, 2], num_filters=[32, 32, 64],
              upsample_strides=[2, 2, 2], num_upsample_filters=[32, 32, 32], cycle_constraint=True, bn_type="SyncBN",
              pred_pyramid_motion=True, use_deep_supervision=True, conv_type="mask_conv", odom_format="rx+t",
              dense_predict=True, dropout=1e-22, conf_type="softmax", use_svd=False,
              point_cloud_range=[-70.4, -38.4, -3, 70.4, 38.4, 1])
    kw.update(over)
    return odom_pred.UNRResNetOdomPredEncDecSVDTempMask(**kw).eval()


def test_eval_path_covers_the_shipped_head_configuration():
    assert _head().eval_fused_unsupported() is None


@pytest.mark.parametrize("case", ["svd", "masksyncbn", "no_running_stats", "float64", "training"])
def test_eval_path_refuses_what_it_does_not_cover(case):
    if case == "svd":
        h = _head(use_svd=True)
    elif case == "masksyncbn":
        h = _head(bn_type="MaskSyncBN")
    elif case == "no_running_stats":
        h = _head()
        bn = [m for m in h.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)][3]
        bn.track_running_stats = False
        bn.running_mean = bn.running_var = None
    elif case == "float64":
        h = _head().double()
    else:
        h = _head().train()
    assert isinstance(h.eval_fused_unsupported(), str)


def test_runner_refuses_a_cpu_or_training_network():
    class _Net:
        training = False
        odom_predictor = _head()
    with pytest.raises(capi.RsloHipError):
        inference.OdometryRunner(_Net())
    _Net.odom_predictor = _head(use_svd=True)
    with pytest.raises(capi.RsloHipError, match="use_svd"):
        inference.OdometryRunner(_Net())
    _Net.training = True
    with pytest.raises(capi.RsloHipError, match="eval"):
        inference.OdometryRunner(_Net())


def test_plain_eval_forward_does_not_take_the_fused_path():
    h = _head()
    assert not h.__dict__.get("_eval_fused", False)
    x = torch.randn(1, 32, 32, 48)
    with torch.no_grad():
        out = h([x[:, :16], x[:, 16:]])
    assert len(out["translation_preds"]) == 1 and "pyramid_motion" in out


class _Recorder:
    def __init__(self):
        self.calls, self.outstanding, self.most = [], set(), 0

    def submit(self, cloud):
        self.calls.append(("s", cloud))
        self.outstanding.add(cloud)
        self.most = max(self.most, len(self.outstanding))
        return ("handle", cloud)

    def run(self, handle):
        tag, cloud = handle
        assert tag == "handle" and cloud in self.outstanding      # run() gets what submit() returned, once
        self.outstanding.remove(cloud)
        self.calls.append(("r", cloud))


@pytest.mark.parametrize("n", [0, 1, 2, 5])
def test_feed_submits_one_scan_ahead(n):
    rec = _Recorder()
    assert inference.OdometryRunner.feed(rec, list(range(n))) is None
    want = []                                     # s0, s1, r0, s2, r1, ..., r(n-1)
    for i in range(n):
        if i == 0:
            want.append(("s", 0))
        if i + 1 < n:
            want.append(("s", i + 1))
        want.append(("r", i))
    assert rec.calls == want
    assert [c for k, c in rec.calls if k == "r"] == list(range(n))      # every handle run exactly once, in order
    assert not rec.outstanding and rec.most <= 2
    if n >= 2:
        assert rec.most == 2                      # it does submit ahead


def test_feed_of_nothing_does_nothing():
    rec = _Recorder()
    inference.OdometryRunner.feed(rec, [])
    assert rec.calls == []
