"""The BEV head's element-wise tail, the ego-motion vote and the pyramid loss (csrc/headtail.hip, csrc/vote.hip,
csrc/pyramid.hip) on their own, through capi, against the float64 restatements of head_support.py at the launch edges:
one cell, the wave of 64, the block of 256 and its neighbours, several blocks, the softmax's 1024 x 32 limit, levels of very
different sizes in one pyramid launch, and the counters the last block of a sample puts back to zero.

Every element of every output is compared.  The bars are per element and come from head_support.py (its docstring has the
derivations): K * 2^-24 * S_i for the elementwise outputs, S_i the magnitude sum behind element i and K four times what
the float32 restatement is off from the float64 one on the CPU; bars derived from the formats for what the kernels sum in
double (odom, sums, den), with the reference sum fed by the device's own elementwise outputs; torch.equal for the exact
outputs.  Nothing is measured on a kernel.  Geometry everywhere: origin (3.3, 5.7, 0.4), cell size (0.4, 0.7, 1.3).

A. vote_fwd / vote_bwd: cells 1 .. 1025 in B = 1 and 3 (and 65); |q| in 0.7 .. 1.3, one q = 0, zero-confidence samples
   (odom exactly 0, sums exactly float32(1e-12)); the counter over block counts 1 -> 5 -> 1 -> 3 and B past 64 and back.
B. pyramid_l2_fwd / _bwd: source (12, 9) with levels (74, 111), (16, 16), (3, 5), (1, 1) in one launch (33 / 1 / 1 / 1
   blocks; the index pairs (12, 74), (9, 111) where torch's float32 nearest rule is not the rational floor), single levels,
   source (3, 24) with (123, 74), one to three mask channels, an all-zero-mask sample, the counter across L * B = 12, 1, 4,
   3, 68, 1; five levels and an empty level are refused before anything is written.
C. tq_normalize_fwd / _bwd: cells 1 .. 1025, |q| from 1e-3 to 1e3.
D. conf_softmax_fwd / _bwd: cells 1 .. 32768, T = 1 and 20 from one call, logits of +-80, a -2000 inside logit, one inside
   cell, no inside cell (exactly 1 / cells); the backward on the device's own confidences; 32769 cells are refused.
E. head_masks_fwd / _bwd: 1 to 4 levels down to 1 x 1, an empty sample, an all-negative mask (the max must not see the
   padding), absent incoming gradients; a size that does not halve is refused.

Measured K (4 x the float32 restatement's worst error in units of 2^-24 S, CPU):
  vote     tq_g 14.4, d_tq 28.5, d_tc 12.9, d_rc 23.4        pyramid  loss_b 1.95, dpred 16.1
  tqn      out 10.3, d_tq 22.2                               masks    w 12.6
  softmax  t_conf 19.4, r_conf 44.3, confT 10.9, d_t 12.5, d_r 9.0
Largest bar relative to its tensor's maximum: 5.8e-06 for a value (confT), 5.7e-05 for a gradient (softmax d_t).

Observed on the MI355X (worst error / bar over all cases of the section); the 52 tests of the file take 2.9 s:
  A: measured bars 0.21 (d_tq of B = 3, 33 x 31: error 69.6 under a bar of 3422 next to the 1e12 of the q = 0 cell); tq_g 0.20,
     d_tc 0.20, d_rc 0.18.  Derived bars 0.53 (odom of B = 65, 1 x 63: error 1.48e-06, bar 4.13e-06), sums 0.46.
  B: loss_b 0.16, dpred 0.22 (both at L4, B = 17).  den 0.94: its error is the one rounding of the double sum to float32,
     which is the derived bar's leading term, so that bar is as tight as a bar can be.
  C: out 0.25, d_tq 0.22 (B = 3, 1025 cells).
  D: confT 0.15 (B = 2, 2049 cells), t_conf 0.15, d_t 0.14, d_r 0.11, r_conf 0.06.
  E: w 0.25 (level 2 of B = 3, 8 x 16); level 0 and every exact output equal their float32 restatement.
No kernel defect was found: all three files pass as they are.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import head_support as HS

pytestmark = pytest.mark.gpu

SENTINEL = -7.0


def _bits(t):
    return t.contiguous().view(torch.int32)


def _cpu(d):
    return {k: ([t.cpu() for t in v] if isinstance(v, (list, tuple)) else v.cpu()) for k, v in d.items()}


def _sentinel(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.float32, device="cuda")


def _untouched(*tensors):
    torch.cuda.synchronize()
    return all(bool((t == SENTINEL).all()) for t in tensors)


# =====================================================================================================================
# A. vote
# =====================================================================================================================
def _vote_dev(hip, case):
    tq, tc, rc, g = (case[k].cuda() for k in ("tq", "tc", "rc", "g"))
    tq_g, odom, sums = hip.vote_fwd(tq, tc, rc, *HS.GEOM)
    d_tq, d_tc, d_rc = hip.vote_bwd(tq, tc, rc, *HS.GEOM, odom, sums, g)
    torch.cuda.synchronize()
    return _cpu(dict(tq_g=tq_g, odom=odom, sums=sums, d_tq=d_tq, d_tc=d_tc, d_rc=d_rc))


def _check_vote(hip, key):
    case, r64, _, S = HS.bundle("vote", key)
    K = HS.measured_K("vote")
    B = key[0]
    tag = "vote B%d_%dx%d" % key
    got = _vote_dev(hip, case)
    fails = []
    for name in ("tq_g", "d_tq", "d_tc", "d_rc"):
        HS.compare(tag, name, got[name], r64[name], K[name] * HS.U * S[name], fails)
    # the reduction alone: the float64 sum of the device's own global map
    red = HS.vote_reduction(got["tq_g"], case["tc"], case["rc"])
    HS.compare(tag, "odom", got["odom"], red["odom"], red["bar_odom"], fails)
    HS.compare(tag, "sums", got["sums"], red["sums"], red["bar_sums"], fails)
    eps = torch.tensor(1e-12, dtype=torch.float32)
    for col, conf, sl in ((0, "tc", slice(0, 3)), (1, "rc", slice(3, 7))):
        zero = case[conf].reshape(B, -1).sum(1) == 0
        if B >= 3:
            assert int(zero.sum()) == 1
        assert torch.equal(got["odom"][zero][:, sl], torch.zeros(int(zero.sum()), sl.stop - sl.start))
        assert torch.equal(got["sums"][zero, col], eps.expand(int(zero.sum())))
    # the cell with q = 0: its normalised quaternion is exactly 0 (the clamp, no 0 / 0)
    qzero = (case["tq"][:, 3:] == 0).all(1, keepdim=True).expand(-1, 4, -1, -1)
    assert not bool(got["tq_g"][:, 3:][qzero].any())
    again = _vote_dev(hip, case)
    assert torch.equal(_bits(got["odom"]), _bits(again["odom"])) and torch.equal(_bits(got["sums"]), _bits(again["sums"]))
    assert not fails, fails


@pytest.mark.parametrize("H,W", HS.VOTE_SHAPES, ids=["%dx%d" % s for s in HS.VOTE_SHAPES])
def test_vote_matches_float64(hip, H, W):
    for B in (1, 3):
        _check_vote(hip, (B, H, W))


def test_vote_counter_and_workspace_across_calls(hip):
    """Blocks per sample 1 -> 5 -> 1 -> 3 in one process, then more samples than the cached counter first held (a new
    counter) and fewer again: a counter that the last block did not put back to zero would end a later call early or never."""
    order = [(3, 8, 8), (3, 25, 41), (1, 16, 16), (3, 19, 27), (65, 1, 63), (1, 33, 31), (3, 5, 13)]
    assert [-(-h * w // 256) for _, h, w in order[:4]] == [1, 5, 1, 3]
    for key in order:
        _check_vote(hip, key)
    done = hip._vote_done[torch.device("cuda", torch.cuda.current_device())]
    assert done.numel() >= 65 and not bool(done.any())


# =====================================================================================================================
# B. pyramid loss
# =====================================================================================================================
def _pyr_dev(hip, case):
    preds, masks = [p.cuda() for p in case["preds"]], [m.cuda() for m in case["masks"]]
    tq, gl = case["tq"].cuda(), case["gl"].cuda()
    loss_b, den = hip.pyramid_l2_fwd(preds, masks, tq, case["H0"], case["W0"], *HS.GEOM)
    dpred = hip.pyramid_l2_bwd(preds, masks, tq, case["H0"], case["W0"], *HS.GEOM, gl, den)
    torch.cuda.synchronize()
    return _cpu(dict(loss_b=loss_b, den=den, dpred=dpred))


def _check_pyramid(hip, key):
    case, r64, _, S = HS.bundle("pyramid", key)
    K = HS.measured_K("pyramid")
    tag = "pyramid %s_B%d" % key
    got = _pyr_dev(hip, case)
    fails = []
    HS.compare(tag, "loss_b", got["loss_b"], r64["loss_b"], K["loss_b"] * HS.U * S["loss_b"], fails)
    for l, (g, r, s) in enumerate(zip(got["dpred"], r64["dpred"], S["dpred"])):
        HS.compare(tag, "dpred%d" % l, g, r, K["dpred"] * HS.U * s, fails)
    den, bar = HS.pyramid_den(case)
    HS.compare(tag, "den", got["den"], den, bar, fails)
    if case["B"] >= 3:                                       # sample 1: every mask zero
        assert not bool(got["loss_b"][:, 1].any()) and not bool(got["den"][:, 1].any())
        assert all(not bool(d[1].any()) for d in got["dpred"])
    again = _pyr_dev(hip, case)
    assert torch.equal(_bits(got["loss_b"]), _bits(again["loss_b"]))
    assert not fails, fails


@pytest.mark.parametrize("name", list(HS.PYR_SPECS))
def test_pyramid_matches_float64(hip, name):
    for B in (1, 3):
        _check_pyramid(hip, (name, B))


def test_pyramid_counter_across_calls(hip):
    """Rows (L * B) 12 -> 1 -> 4 -> 3 -> 68 -> 1 with 33, 1, 33, 36, 33 and 1 blocks in the grid: the 68 rows are more than
    the cached counter first held."""
    for key in [("L4", 3), ("L1_15x17", 1), ("L4", 1), ("src3x24", 3), ("L4", 17), ("L1_same", 1)]:
        _check_pyramid(hip, key)
    done = hip._py_done[torch.device("cuda", torch.cuda.current_device())]
    assert done.numel() >= 68 and not bool(done.any())


def _pyr_raw(hip, preds, masks, tq, H0, W0, loss_b, den, dpreds, gl):
    """The two C entries on outputs the caller owns; returns the two return codes' exceptions (or None)."""
    lib = hip.lib()
    L = len(preds)
    arr, B = hip._pyramid_levels(preds, masks, dpreds)
    done = torch.zeros(64, dtype=torch.int32, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    o3, v3 = hip._F3(*HS.GEOM[0]), hip._F3(*HS.GEOM[1])
    errs = []
    for name, call in (
            ("rslo_pyramid_l2_fwd", lambda: lib.rslo_pyramid_l2_fwd(arr, L, B, tq.data_ptr(), H0, W0, o3, v3, ws.data_ptr(),
                                                                    ws.numel(), done.data_ptr(), loss_b.data_ptr(),
                                                                    den.data_ptr(), hip._stream())),
            ("rslo_pyramid_l2_bwd", lambda: lib.rslo_pyramid_l2_bwd(arr, L, B, tq.data_ptr(), H0, W0, o3, v3, gl.data_ptr(),
                                                                    den.data_ptr(), hip._stream()))):
        try:
            hip._chk(call(), name)
            errs.append(None)
        except hip.RsloHipError as e:
            errs.append(e)
    torch.cuda.synchronize()
    return errs, done


@pytest.mark.parametrize("what", ["five_levels", "empty_level"])
def test_pyramid_refuses_and_writes_nothing(hip, what):
    B = 2
    sizes = [(4, 4)] * 5 if what == "five_levels" else [(4, 4), (0, 5)]
    preds = [torch.randn(B, 7, h, w, device="cuda") for h, w in sizes]
    masks = [torch.ones(B, 1, h, w, device="cuda") for h, w in sizes]
    dpreds = [_sentinel(B, 7, max(h, 1), w) for h, w in sizes]
    tq = torch.randn(B, 7, device="cuda")
    L = len(sizes)
    loss_b, den, gl = _sentinel(L, B, 2), _sentinel(L, B, 2), torch.ones(L, B, 2, device="cuda")
    errs, done = _pyr_raw(hip, preds, masks, tq, 12, 9, loss_b, den, dpreds, gl)
    assert all(isinstance(e, hip.RsloHipError) for e in errs), errs
    assert _untouched(loss_b, den, *dpreds) and not bool(done.any())
    with pytest.raises(hip.RsloHipError):                   # and through the binding
        hip.pyramid_l2_fwd(preds, masks, tq, 12, 9, *HS.GEOM)


# =====================================================================================================================
# C. quaternion normalisation
# =====================================================================================================================
@pytest.mark.parametrize("B,cells", HS.TQN_CASES, ids=["B%d_%d" % c for c in HS.TQN_CASES])
def test_tq_normalize_matches_float64(hip, B, cells):
    case, r64, _, S = HS.bundle("tqn", (B, cells))
    K = HS.measured_K("tqn")
    tq, g = case["tq"].cuda(), case["g"].cuda()
    out, d_tq = hip.tq_normalize_fwd(tq), hip.tq_normalize_bwd(tq, g)
    torch.cuda.synchronize()
    fails = []
    tag = "tqn B%d_%d" % (B, cells)
    HS.compare(tag, "out", out, r64["out"], K["out"] * HS.U * S["out"], fails)
    HS.compare(tag, "d_tq", d_tq, r64["d_tq"], K["d_tq"] * HS.U * S["d_tq"], fails)
    assert torch.equal(out[:, :3].cpu(), case["tq"][:, :3]) and torch.equal(d_tq[:, :3].cpu(), case["g"][:, :3])      # copies
    assert not fails, fails


# =====================================================================================================================
# D. masked spatial softmax
# =====================================================================================================================
def _softmax_dev(hip, case):
    tl, rl, o = case["t_logit"].cuda(), case["r_logit"].cuda(), case["outside"].cuda()
    t_conf, r_conf, confT = hip.conf_softmax_fwd(tl, rl, o, case["temp"])
    d_t, d_r = hip.conf_softmax_bwd(t_conf, r_conf, case["g_t"].cuda(), case["g_r"].cuda(), o)      # its own confidences
    torch.cuda.synchronize()
    return _cpu(dict(t_conf=t_conf, r_conf=r_conf, confT=confT, d_t=d_t, d_r=d_r))


@pytest.mark.parametrize("cells", HS.SM_CELLS)
def test_conf_softmax_matches_float64(hip, cells):
    K = HS.measured_K("softmax")
    for B in (1, 2):
        case, r64, _, S = HS.bundle("softmax", (B, cells))
        got = _softmax_dev(hip, case)
        fails = []
        tag = "softmax B%d_%d" % (B, cells)
        for name in ("t_conf", "r_conf", "confT", "d_t", "d_r"):
            HS.compare(tag, name, got[name], r64[name], K[name] * HS.U * S[name], fails, floor=HS.softmax_floor(r64[name], cells))
        o = case["outside"]
        assert not bool(got["d_t"][o].any()) and not bool(got["d_r"][o].any())      # outside cells: exactly 0
        one = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(cells), dtype=torch.float32)
        for b, kind in enumerate(HS.sm_kinds(B, cells)):
            if kind == "all_outside":
                for t in (got["t_conf"][b], got["r_conf"][b], got["confT"][b]):
                    assert torch.equal(t, one.expand_as(t)), (tag, b)
            if kind == "one_inside" and cells > 1:          # everything on the one inside cell at T = 1
                assert float(got["t_conf"][b].max()) == 1.0 and int((got["t_conf"][b] > 0).sum()) == 1
        assert not fails, fails


def test_conf_softmax_refuses_more_cells_than_it_holds(hip):
    B, cells = 1, 32769
    tl, rl = torch.randn(B, 1, 1, cells, device="cuda"), torch.randn(B, 1, 1, cells, device="cuda")
    o = torch.zeros(B, 1, 1, cells, dtype=torch.bool, device="cuda")
    t_conf, r_conf, confT, d_t, d_r = (_sentinel(B, 1, 1, cells), _sentinel(B, 1, 1, cells), _sentinel(B, 2, 1, cells),
                                       _sentinel(B, 1, 1, cells), _sentinel(B, 1, 1, cells))
    lib = hip.lib()
    with pytest.raises(hip.RsloHipError):
        hip._chk(lib.rslo_conf_softmax_fwd(tl.data_ptr(), rl.data_ptr(), o.data_ptr(), B, cells, 20.0, t_conf.data_ptr(),
                                           r_conf.data_ptr(), confT.data_ptr(), hip._stream()), "rslo_conf_softmax_fwd")
    with pytest.raises(hip.RsloHipError):
        hip._chk(lib.rslo_conf_softmax_bwd(tl.data_ptr(), rl.data_ptr(), tl.data_ptr(), rl.data_ptr(), o.data_ptr(), B, cells,
                                           d_t.data_ptr(), d_r.data_ptr(), hip._stream()), "rslo_conf_softmax_bwd")
    assert _untouched(t_conf, r_conf, confT, d_t, d_r)
    with pytest.raises(hip.RsloHipError):
        hip.conf_softmax_fwd(tl, rl, o, 20.0)


# =====================================================================================================================
# E. mask / weight pyramid
# =====================================================================================================================
def _masks_fwd_owned(hip, mask, conf, tq, tq_g, preds, levels):
    """rslo_head_masks_fwd on sentinel-filled outputs of the caller; returns (outputs, error or None)."""
    B, _, H, W = mask.shape
    a = hip.HeadMasks()
    a.mask, a.conf, a.tq, a.tq_g = mask.data_ptr(), conf.data_ptr(), tq.data_ptr(), tq_g.data_ptr()
    outs = [_sentinel(B, 7, H, W), _sentinel(B, 7, H, W)]
    a.mtq, a.mtq_g = outs[0].data_ptr(), outs[1].data_ptr()
    for k in range(levels):
        w = _sentinel(B, 2, max(H >> k, 1), max(W >> k, 1))
        outs.append(w)
        a.w[k] = w.data_ptr()
        if k:
            occ, mp = _sentinel(B, 1, max(H >> k, 1), max(W >> k, 1)), _sentinel(*preds[k - 1].shape)
            outs += [occ, mp]
            a.occ[k], a.pred[k - 1], a.mpred[k - 1] = occ.data_ptr(), preds[k - 1].data_ptr(), mp.data_ptr()
    a.B, a.H, a.W, a.levels = B, H, W, levels
    try:
        hip._chk(hip.lib().rslo_head_masks_fwd(C.byref(a), hip._stream()), "rslo_head_masks_fwd")
        err = None
    except hip.RsloHipError as e:
        err = e
    return outs, err


@pytest.mark.parametrize("key", HS.HM_CASES, ids=["B%d_%dx%d_L%d_%s" % k for k in HS.HM_CASES])
def test_head_masks_match_float64_and_exact_outputs(hip, key):
    case, r64, r32, S = HS.bundle("masks", key)
    K = HS.measured_K("masks")
    L = case["levels"]
    mask, conf, tq, tq_g = (case[k].cuda() for k in ("mask", "conf", "tq", "tq_g"))
    preds = [p.cuda() for p in case["preds"]]
    w, occ, mp, mtq, mtq_g = hip.head_masks_fwd(mask, conf, tq, tq_g, preds)
    torch.cuda.synchronize()
    assert len(w) == L and len(occ) == L and len(mp) == L - 1
    fails = []
    tag = "masks B%d_%dx%d_L%d_%s" % key
    for k in range(L):
        HS.compare(tag, "w%d" % k, w[k], r64["w"][k], K["w"] * HS.U * S["w"][k], fails)
    assert torch.equal(w[0].cpu(), r32["w"][0])              # level 0 is one float32 product
    for k in range(1, L):
        assert torch.equal(occ[k].cpu(), r32["occ"][k]), k
        assert torch.equal(mp[k - 1].cpu(), r32["mpreds"][k - 1]), k
    assert torch.equal(mtq.cpu(), r32["mtq"]) and torch.equal(mtq_g.cpu(), r32["mtq_g"])
    if key[0] >= 3:                                          # the empty sample
        assert all(not bool(t[1].any()) for t in w) and all(not bool(t[1].any()) for t in occ)
    # backward: every incoming gradient present, then one level's and g_mtq absent (zero-filled)
    shapes = [tuple(p.shape) for p in preds]
    g_mp, g_mtq = [g.cuda() for g in case["g_mpreds"]], case["g_mtq"].cuda()
    runs = [(None, False)] + [(k, True) for k in range(1, L)] + ([(None, True)] if L == 1 else [])
    for absent, no_mtq in runs:
        want = HS.masks_ref(case, torch.float32, absent_level=absent, absent_mtq=no_mtq)
        d_preds, d_tq = hip.head_masks_bwd(mask, occ, [None if k == absent else g for k, g in enumerate(g_mp, 1)],
                                           None if no_mtq else g_mtq, shapes)
        torch.cuda.synchronize()
        assert torch.equal(d_tq.cpu(), want["d_tq"]), (absent, no_mtq)
        for k, (d, r) in enumerate(zip(d_preds, want["d_preds"]), 1):
            assert torch.equal(d.cpu(), r), (absent, k)
        if no_mtq:
            assert not bool(d_tq.any())
        if absent is not None:
            assert not bool(d_preds[absent - 1].any())
    assert not fails, fails


def test_head_masks_refuse_a_size_that_does_not_halve(hip):
    B, H, W, L = 2, 6, 8, 3
    mask, conf = torch.ones(B, 1, H, W, device="cuda"), torch.rand(B, 2, H, W, device="cuda")
    tq, tq_g = torch.randn(B, 7, H, W, device="cuda"), torch.randn(B, 7, H, W, device="cuda")
    preds = [torch.randn(B, 7, H >> k, W >> k, device="cuda") for k in range(1, L)]
    outs, err = _masks_fwd_owned(hip, mask, conf, tq, tq_g, preds, L)
    assert isinstance(err, hip.RsloHipError) and _untouched(*outs)
    # the same call on a size that halves writes every output
    outs, err = _masks_fwd_owned(hip, mask[:, :, :4].contiguous(), conf[:, :, :4].contiguous(), tq[:, :, :4].contiguous(),
                                 tq_g[:, :, :4].contiguous(), [p[:, :, :(4 >> k)].contiguous() for k, p in enumerate(preds, 1)], L)
    torch.cuda.synchronize()
    assert err is None and all(not bool((t == SENTINEL).any()) for t in outs)
