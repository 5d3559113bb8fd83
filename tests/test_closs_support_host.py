"""CPU checks of tests/closs_support.py: the float32 order emulator is a sum, its two rules can be told apart, and the
float64 restatement really runs in float64."""
import numpy as np
import pytest
import torch

import closs_support as CS

RUNS = (1, 32, 33, 64, 65, 200)


def _values(K, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((K, 10)) * np.exp(rng.uniform(-3, 3, (K, 10)))).astype(np.float32)


@pytest.mark.parametrize("K", RUNS)
def test_emulator_is_a_sum(K):
    """Any order of K float32 additions is within (K - 1) * 2^-24 * sum|c| (1 + O(2^-24)) of the exact sum; K is asserted."""
    c = _values(K, K)
    got = CS.sum_run_f32(c).astype(np.float64)
    exact = c.astype(np.float64).sum(0)
    bound = K * 2.0 ** -24 * np.abs(c.astype(np.float64)).sum(0)
    assert (np.abs(got - exact) <= bound).all(), (np.abs(got - exact) / bound).max()
    # through ordered_gather_f32: one partner, sources scattered, one gated-out source in between
    perm = np.random.default_rng(100 + K).permutation(K + 1)
    contrib = np.zeros((1, K + 1, 10), np.float32)
    roi = np.ones((1, K + 1), bool)
    roi[0, perm[K]] = False
    contrib[0, perm[K]] = 1e6                                # must not be added
    srcs = np.sort(perm[:K])
    contrib[0, srcs] = c                                     # ascending source order = the order of c
    out = CS.ordered_gather_f32(contrib, np.full((1, K + 1), 2), roi, 4)
    assert out.dtype == np.float32 and out.shape == (1, 4, 10)
    assert np.array_equal(out[0, 2].view(np.int32), CS.sum_run_f32(c).view(np.int32))
    assert not out[0, [0, 1, 3]].view(np.int32).any()        # untouched rows are +0


def test_threshold_between_the_rules():
    assert CS.RB_SHORT == 32
    c = _values(33, 5)
    assert np.array_equal(CS.sum_run_f32(c[:32]).view(np.int32), CS.sum_short_f32(c[:32]).view(np.int32))
    assert np.array_equal(CS.sum_run_f32(c).view(np.int32), CS.sum_long_f32(c).view(np.int32))


def test_short_and_long_rule_give_different_bits():
    diff = 0
    for seed in range(8):
        c = _values(33, 1000 + seed)
        diff += int((CS.sum_short_f32(c).view(np.int32) != CS.sum_long_f32(c).view(np.int32)).sum())
    assert diff > 0


def test_long_rule_is_the_stated_tree():
    """Exactly representable values: lane l holds 2^l-ish weights so a dropped or doubled lane shows in the integer sum."""
    c = np.zeros((130, 1), np.float32)
    c[:, 0] = np.arange(1, 131)
    assert CS.sum_long_f32(c)[0] == 130 * 131 / 2
    # order inside a lane: lane 0 adds rows 0, 64, 128 in that order
    c = np.zeros((129, 1), np.float32)
    c[0, 0], c[64, 0], c[128, 0] = 2.0 ** 24, 1.0, 1.0       # (2^24 + 1) + 1 = 2^24 in float32; 2^24 + (1 + 1) would not be
    assert CS.sum_long_f32(c)[0] == 2.0 ** 24
    # level order: lanes 0 and 32 meet first, lane 16 (+ 48) joins after
    c = np.zeros((64, 1), np.float32)
    c[0, 0], c[32, 0], c[16, 0], c[48, 0] = 2.0 ** 24, 1.0, 1.0, 1.0
    assert CS.sum_long_f32(c)[0] == 2.0 ** 24 + 2.0          # (2^24 + 1 -> 2^24) + (1 + 1)


def test_gather_keeps_batch_members_apart():
    c = _values(3 * 5, 9).reshape(3, 5, 10)
    out = CS.ordered_gather_f32(c, np.zeros((3, 5), np.int64), np.ones((3, 5), bool), 1)
    for b in range(3):
        assert np.array_equal(out[b, 0].view(np.int32), CS.sum_short_f32(c[b]).view(np.int32))


def test_restatement_runs_in_float64_and_float32_is_close():
    rng = np.random.default_rng(3)
    B, N, M = 3, 257, 40
    idx = rng.integers(0, M, (B, N))
    roi = rng.random((B, N)) < 0.9
    case = CS.make_case(B, N, M, idx, roi, 3)
    assert all(case[k].dtype == torch.float32 for k in ("p1", "tgt", "cov1", "cov2", "Rd", "dist", "thr", "gloss"))
    assert float(case["cov1"][..., :3].min()) >= 0.5 and float(case["cov1"][..., 3:].norm(dim=-1).min()) >= 0.5 - 1e-6
    assert bool((case["gloss"] != 0).all())
    r64 = CS.residual_ref64(case)
    r32 = CS.residual_ref64(case, torch.float32)
    assert r64["loss"].dtype == torch.float64 and r32["loss"].dtype == torch.float32
    assert torch.equal(r64["cnt"], torch.from_numpy(roi.sum(-1).astype(np.float64)))
    for k in ("loss", "gp1", "gtgt", "gcov1", "gcov2"):
        e = float((r32[k].double() - r64[k]).abs().max())
        assert e <= 1e-5 * float(r64[k].abs().max()), (k, e)      # float32 formulation: far inside the project's bars
        assert e > 0
    # the unrolled case is the same loss
    u64 = CS.residual_ref64(CS.unrolled_case(case))
    assert float((u64["loss"] - r64["loss"]).abs().max()) <= 1e-12 * float(r64["loss"].abs().max())


def test_icp_restatement_composes():
    rng = np.random.default_rng(4)
    B, N = 2, 300
    case = CS.icp_case(B, N, N + 11, rng.integers(0, N + 11, (B, N)), rng.random((B, N)) < 0.8, 4)
    w = CS.icp_weights(case, torch.float64)
    assert w.dtype == torch.float64 and float(w.max()) <= 1.0
    R0, t0 = CS.icp_ref64(case, w)
    R1, t1 = CS.icp_ref64(case, w, case["res_r"], case["res_t"])
    assert torch.allclose(R1, R0 @ case["res_r"].double(), atol=1e-14)
    assert torch.allclose(t1, (R0 @ case["res_t"].double()[..., None]).squeeze(-1) + t0, atol=1e-13)
    assert float((R0 @ R0.transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-13
    assert bool((torch.det(R0) > 0).all())
