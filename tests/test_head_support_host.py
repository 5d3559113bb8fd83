"""CPU checks of tests/head_support.py: the float64 restatements are the project's own unfused formulations, the chosen
inputs would catch the mistakes a kernel can make, and the bars keep under the project's existing ones."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_support as HS

import rslo_amd  # noqa: F401  (makes `rslo` resolve to the mirror)

F64 = torch.float64


def _agree(a, b, what):
    """|a - b| <= 1e-12 max(1, |b|) per element."""
    assert a.dtype == F64 and b.dtype == F64 and a.shape == b.shape, what
    assert bool(((a - b).abs() <= 1e-12 * b.abs().clamp_min(1.0)).all()), (what, float((a - b).abs().max()))


# =====================================================================================================================
# the restatements are the project's formulations
# =====================================================================================================================
@pytest.mark.parametrize("B,H,W", [(3, 5, 13), (1, 1, 1), (3, 19, 27), (1, 257, 1)])
def test_vote_restatement_is_the_projects_formulation(B, H, W):
    from rslo.data.dataset import _grid_geometry
    from rslo.models.odom_pred import UNOdomPredEncDecSVDTempMaskBase as Head
    case = HS.vote_case(B, H, W)
    ref = HS.vote_ref(case, F64)
    pc = HS.pc_range_for(H, W)
    _, vs, origin = _grid_geometry([1, H, W], pc)          # the derived range gives back the chosen float32 geometry
    assert tuple(float(np.float32(v)) for v in origin) == HS.GEOM[0]
    assert tuple(float(np.float32(v)) for v in vs) == HS.GEOM[1]
    tq, tc, rc = (case[k].double().requires_grad_(True) for k in ("tq", "tc", "rc"))
    stub = types.SimpleNamespace(point_cloud_range=pc, fused_vote=False)
    tq_g, odom = Head.vote(stub, tq, tc, rc)               # CPU tensors: from_pointwise_local_transformation_tch + means
    _agree(tq_g.detach(), ref["tq_g"], "tq_g")
    _agree(odom.detach(), ref["odom"], "odom")
    (odom * case["g"].double()).sum().backward()
    for got, name in ((tq.grad, "d_tq"), (tc.grad, "d_tc"), (rc.grad, "d_rc")):
        top = float(ref[name].abs().max())
        assert bool(torch.isfinite(got).all()), name
        assert float((got - ref[name]).abs().max()) <= 1e-12 * max(top, 1.0), name


@pytest.mark.parametrize("B,cells", [(2, 65), (2, 1024), (1, 63), (1, 64)])
def test_softmax_restatement_is_masked_spatial_softmax(B, cells):
    from rslo.layers.confidence import masked_spatial_softmax
    case = HS.sm_case(B, cells)
    o = case["outside"]
    for logit in (case["t_logit"].double(), case["r_logit"].double()):
        for T in (1, 20):
            _agree(HS._masked_softmax(logit, o, float(T)), masked_spatial_softmax(logit, None, T, o), "T=%d" % T)
            mask = (~o).double()                             # and from the mask, as ConfidenceModule is called
            _agree(HS._masked_softmax(logit, o, float(T)), masked_spatial_softmax(logit, mask, T), "mask T=%d" % T)


@pytest.mark.parametrize("key", [(3, 8, 8, 4, "half"), (1, 16, 24, 3, "half"), (3, 6, 10, 2, "half"), (1, 8, 8, 4, "negative")])
def test_masks_restatement_is_the_heads_pooling(key):
    """The head's unfused tail (models/odom_pred.py): MaxPool2d(3, 2, 1) for the occupancy, AvgPool2d(3, 2, padding=1) for
    the weights, coarse levels weighted by the pooled finer ones."""
    from rslo.models import odom_pred
    maxpool, avgpool = torch.nn.MaxPool2d(3, 2, 1), torch.nn.AvgPool2d(3, 2, padding=1)
    assert odom_pred._maxpool_321(maxpool) and odom_pred._avgpool_321(avgpool)
    case = HS.hm_case(*key)
    ref = HS.masks_ref(case, F64)
    mask, conf, tq = case["mask"].double(), case["conf"].double(), case["tq"].double()
    py_masks = [mask]
    for _ in case["preds"]:
        py_masks.append(maxpool(py_masks[-1]))
    motion = [[p.double() * (m > 0).to(F64), m] for p, m in zip(case["preds"][::-1], py_masks[:0:-1])]
    motion += [[tq * mask, mask * conf]]
    for p in range(2, len(motion) + 1):
        motion[-p][1] = motion[-p][1] * avgpool(motion[-(p - 1)][1])
    for k, (mp, w) in enumerate(motion[::-1]):             # finest first
        _agree(w, ref["w"][k], "w%d" % k)
        assert torch.equal(py_masks[k], ref["occ"][k])
        assert torch.equal(mp, ref["mtq"] if k == 0 else ref["mpreds"][k - 1])
    assert torch.equal(case["tq_g"].double() * mask, ref["mtq_g"])


@pytest.mark.parametrize("name,B", [("L4", 3), ("src3x24", 1), ("L1_same", 3), ("L1_1x257", 1)])
def test_pyramid_restatement_is_adaptive_l2_on_a_resampled_map(name, B):
    from rslo.core import losses
    from rslo.data.dataset import generate_pointwise_local_transformation_tch as gen
    case = HS.pyramid_case(name, B)
    ref = HS.pyramid_ref(case, F64)
    H0, W0 = case["H0"], case["W0"]
    tq = case["tq"].double()
    maps = torch.stack([gen(t, [W0, H0], HS.GEOM[0], HS.GEOM[1]).reshape(7, H0, W0) for t in tq])
    mod = losses.AdaptiveWeightedL2Loss(init_alpha=0.0).double()
    for l, (p, m) in enumerate(zip(case["preds"], case["masks"])):
        p, m = p.double().requires_grad_(True), m.double()
        # the network resamples a float32 map; on a float64 map F.interpolate would work out the source index in double,
        # which is another rule at (12, 74) and (9, 111).  So the 2-D F.interpolate resamples the float32 NUMBER of every
        # source cell (exact up to 2^24) and the float64 map is read at those cells.
        h, w = p.shape[2:]
        number = torch.arange(H0 * W0, dtype=torch.float32).view(1, 1, H0, W0)
        cell = number if (h, w) == (H0, W0) else F.interpolate(number, size=(h, w), mode="nearest")
        tgt = maps.flatten(2)[:, :, cell.flatten().long()].view(B, 7, h, w)
        total = 0.0
        for b in range(B):
            for c, (sl, mm) in enumerate(((slice(0, 3), m[:, :1]), (slice(3, 7), m[:, -1:]))):
                one = mod(p[b:b + 1, sl], tgt[b:b + 1, sl], mask=mm[b:b + 1])
                # one sample, focal_gamma 0, alpha 0: loss_b / (1 + 1e-12)
                want = losses._adaptive_reduce(ref["loss_b"][l, b, c].reshape(1), mod.alpha.detach(), 0)
                assert abs(float(one.detach()) - float(want)) <= 1e-12 * max(1.0, abs(float(want))), (l, b, c)
                total = total + one * (1 + 1e-12) * float(case["gl"][l, b, c])
        total.backward()
        top = float(ref["dpred"][l].abs().max())
        assert float((p.grad - ref["dpred"][l]).abs().max()) <= 1e-12 * max(top, 1.0), l
    den, _ = HS.pyramid_den(case)
    _agree(den, ref["den"], "den")


@pytest.mark.parametrize("B,cells", [(3, 257), (1, 1)])
def test_tq_normalize_restatement_is_the_heads_line(B, cells):
    case = HS.tqn_case(B, cells)
    tq = case["tq"].double()
    t_part, q_part = tq.split([3, 4], dim=1)                 # models/odom_pred.py, the unfused branch
    want = torch.cat([t_part, q_part / torch.norm(q_part, dim=1, keepdim=True)], dim=1)
    assert torch.equal(HS.tqn_ref(case, F64)["out"], want)


def test_float32_twins_run_in_float32():
    for fam, key in (("vote", (3, 5, 13)), ("pyramid", ("L4", 1)), ("tqn", (1, 257)), ("softmax", (2, 65)),
                     ("masks", (3, 8, 8, 4, "half"))):
        _, r64, r32, _ = HS.bundle(fam, key)
        for name, ts in HS._flat(r32).items():
            assert all(t.dtype == torch.float32 for t in ts), (fam, name)
            assert all(t.dtype == F64 for t in HS._flat(r64)[name]), (fam, name)


# =====================================================================================================================
# the index cases bite
# =====================================================================================================================
def test_nearest_index_is_torchs_float32_rule_and_not_the_rational_floor():
    for n_src, n_dst in ((12, 74), (24, 74), (9, 111), (3, 123)):
        a, b = HS.nearest_index(n_src, n_dst), HS.nearest_index(n_src, n_dst, exact=True)
        assert int((a != b).sum()) > 0, (n_src, n_dst)
        assert int((a - b).abs().max()) == 1 and int(a.max()) == n_src - 1
    # min(floor(dst * (float32) src / dst_size), src - 1) in float32, the rule csrc/pyramid.hip states
    for n_src in range(1, 17):
        for n_dst in range(1, 200):
            sc = np.float32(n_src) / np.float32(n_dst)
            own = np.minimum(np.floor(np.arange(n_dst, dtype=np.float32) * sc).astype(np.int64), n_src - 1)
            assert np.array_equal(own, HS.nearest_index(n_src, n_dst).numpy()), (n_src, n_dst)


# =====================================================================================================================
# sensitivity: one mistake moves the float64 restatement by more than 10 bars
# =====================================================================================================================
def _moved(family, key, variant, names):
    """largest |variant - true| / bar over the elements of the named outputs of one case."""
    case, r64, _, S = HS.bundle(family, key)
    K = HS.measured_K(family)
    wrong = HS.FAMILIES[family][2](case, F64, variant)
    worst = 0.0
    for name in names:
        for a, b, s in zip(HS._flat(wrong)[name], HS._flat(r64)[name], HS._flat(S)[name]):
            bar = K[name] * HS.U * s
            diff = (a - b).abs()
            pos = bar > 0
            if bool(pos.any()):
                worst = max(worst, float((diff[pos] / bar[pos]).max()))
    return worst


def _vote_odom_moved(key, variant):
    """the voted pose against the derived bar, with the float32 twin's global map standing in for the device's."""
    case, r64, r32, _ = HS.bundle("vote", key)
    red = HS.vote_reduction(r32["tq_g"], case["tc"], case["rc"])
    wrong = HS.vote_ref(case, F64, variant)
    pos = red["bar_odom"] > 0
    return float(((wrong["odom"] - r64["odom"]).abs()[pos] / red["bar_odom"][pos]).max())


GEOMETRY = ("swap_v", "swap_o", "flip_y", "q_other_way", "q_norm_first")


@pytest.mark.parametrize("variant", GEOMETRY)
def test_vote_inputs_catch_geometry_and_rotation_mistakes(variant):
    for key in HS.VOTE_CASES:
        assert _moved("vote", key, variant, ("tq_g",)) > 10, (variant, key)
        assert _vote_odom_moved(key, variant) > 10, (variant, key)


@pytest.mark.parametrize("variant", ["drop_block", "drop_wave"])
def test_vote_inputs_catch_a_lost_tail(variant):
    for key in HS.VOTE_CASES:
        cells = key[1] * key[2]
        lost = cells % 256 if variant == "drop_block" else cells - ((cells - 1) // 64) * 64
        if lost:
            assert _vote_odom_moved(key, variant) > 10, (variant, key)


@pytest.mark.parametrize("variant", GEOMETRY + ("drop_block", "drop_wave"))
def test_pyramid_inputs_catch_geometry_rotation_and_tail_mistakes(variant):
    for key in HS.PYR_CASES:
        names = ("loss_b",) if variant.startswith("drop") else ("loss_b", "dpred")
        assert _moved("pyramid", key, variant, names) > 10, (variant, key)


def test_pyramid_inputs_catch_the_wrong_mask_channel_and_index():
    for B in (1, 3):
        for name in ("L4", "L1_1x257", "src3x24"):           # the cases with a three-channel mask
            assert _moved("pyramid", (name, B), "rot_ch1", ("loss_b", "dpred")) > 10, name
        for name in ("L4", "src3x24"):                       # the cases with the size pairs of the index test
            assert _moved("pyramid", (name, B), "exact_index", ("loss_b", "dpred")) > 10, name
    # and the denominators of the rotation column move off their derived bar
    case = HS.pyramid_case("L1_1x257", 1)
    den, bar = HS.pyramid_den(case)
    wrong = HS.pyramid_ref(case, F64, "rot_ch1")["den"]
    assert float(((wrong - den).abs() / bar)[..., 1].max()) > 10


def test_masks_inputs_catch_the_pooling_mistakes():
    for key in HS.HM_CASES:
        if key[3] >= 2 and key[4] == "half":
            assert _moved("masks", key, "avg_valid", ("w",)) > 10, key
    # a max that counts the padding as 0 shows only on negative inputs: with 0/1 occupancies it is the same function,
    # which is why the 'negative' case exists
    neg = HS.hm_case(1, 8, 8, 4, "negative")
    a, b = HS.masks_ref(neg, F64)["occ"], HS.masks_ref(neg, F64, "maxpool_pad0")["occ"]
    assert all(not torch.equal(x, y) for x, y in zip(a[1:], b[1:]))
    half = HS.hm_case(3, 8, 8, 4, "half")
    a, b = HS.masks_ref(half, F64)["occ"], HS.masks_ref(half, F64, "maxpool_pad0")["occ"]
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# =====================================================================================================================
# the conditions on the bars hold on the reference alone
# =====================================================================================================================
@pytest.mark.parametrize("family", list(HS.FAMILIES))
def test_bars_keep_under_the_projects_ceilings(family):
    K = HS.measured_K(family)
    assert all(np.isfinite(v) for v in K.values()), K
    print("head K %-8s %s" % (family, {k: round(v, 2) for k, v in K.items()}))
    top = {}
    for key in HS.FAMILIES[family][0]:
        case, r64, r32, S = HS.bundle(family, key)
        for name, scales in HS._flat(S).items():
            for a, b, s in zip(HS._flat(r32)[name], HS._flat(r64)[name], scales):
                bar = K[name] * HS.U * s
                ok, frac, noise_only = HS.check_ceiling(bar, b, name in HS.GRADIENTS)
                assert ok, (family, key, name, frac)
                if not noise_only:
                    top[name] = max(top.get(name, 0.0), frac)
                # the twin sits within a quarter of the bar (and the floor, where one applies)
                floor = HS.softmax_floor(b, key[1]) if family == "softmax" else torch.zeros_like(b)
                assert bool(((a.double() - b).abs() <= bar / 4 * (1 + 1e-9) + floor).all()), (family, key, name)
    print("head ceilings %-8s max bar / max|ref| %s" % (family, {k: "%.2e" % v for k, v in top.items()}))


def test_derived_bars_keep_under_the_ceilings():
    for key in HS.VOTE_CASES:
        case, r64, r32, _ = HS.bundle("vote", key)
        red = HS.vote_reduction(r32["tq_g"], case["tc"], case["rc"])
        for b in range(key[0]):                              # per sample: a zero-confidence sample has bar 0
            for sl in (slice(0, 3), slice(3, 7)):
                top = float(red["odom"][b, sl].abs().max())
                assert float(red["bar_odom"][b, sl].max()) <= 1e-5 * top or top == 0.0, key
        assert bool((red["bar_sums"] <= 1e-5 * red["sums"]).all())
        zero_t = case["tc"].reshape(key[0], -1).sum(1) == 0
        assert bool((red["odom"][zero_t, :3] == 0).all()) and bool((red["bar_odom"][zero_t, :3] == 0).all())
        assert bool((red["sums"][zero_t, 0] == HS.EPS32).all())
    for key in HS.PYR_CASES:
        den, bar = HS.pyramid_den(HS.pyramid_case(*key))
        assert bool((bar <= 1e-5 * den).all())


def test_softmax_floor_covers_what_float32_cannot_hold():
    """T = 1 with a spread of +-80 underflows (the floor applies there), T = 20 does not, except for the -2000 logit."""
    case, r64, r32, _ = HS.bundle("softmax", (2, 1025))
    inside = ~case["outside"][0, 0, 0]
    t1, tT = r64["t_conf"][0, 0, 0][inside], r64["confT"][0, 0, 0][inside]
    assert int((t1 < 2.0 ** -126).sum()) > 10
    assert int((tT < 2.0 ** -126).sum()) == 1 and float(case["t_logit"][0, 0, 0][inside][tT < 2.0 ** -126]) == -2000.0
    assert float(HS.softmax_floor(t1, 1025).max()) == 1025 * 2.0 ** -126
