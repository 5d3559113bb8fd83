"""The consistency loss's fused kernels (csrc/loss.hip) on their own, with the correspondence index and the ROI GIVEN.

A. rslo_cov_residual_bwd's ordered gather -- no tolerance, bit patterns only.  Every source's ten partner values are read
   off an "unrolled" call (each source gets a partner row of its own); the real call's partner rows must equal
   closs_support.ordered_gather_f32 of those values: one thread in ascending source order up to 32 sources, one wave
   (lane-strided partials, fixed shuffle tree) above.
B. rslo_cov_residual_fwd / _bwd against the float64 restatement (closs_support.residual_ref64).  Bar per output tensor:
   8 * e32, e32 = max|float32 restatement - float64 restatement| on the CPU -- measured on the reference, never on the
   kernel; 8 because the kernel associates the same expressions differently, multiplies by 1/det where torch divides and
   symmetrises sigma^-1 in the log-det term.  Ceiling (asserted): 8 * e32 <= 1e-5 * max|loss| and <= 1e-4 * max|gradient|,
   the project's existing bars.  cnt is exact.
C. rslo_icp_step / _first against losses.masked_kabsch in float64 + the composition in float64.  The kernel sums in
   double; what differs is the float32 weight and the float32 rounding of the outputs.  Bar per pair:
   4 * d_w + 2^-22 * scale, d_w = |restatement with float32 weights - restatement with float64 weights| (measured on the
   reference), 4 because the kernel's weight expression rounds in another order than cosine_similarity, scale = 1 for R and
   1 + max|coordinate| for t.  Ceiling (asserted): bar < 1e-5 for R, < 1e-4 for t (test_icp_step_recovers_known_motion).
   Where the rotation is not determined (N = 1, N = 2) only a proper rotation (|R R^T - I| <= 1e-6, det > 0) and the
   centroid map are asserted; the centroid bar is 2^-22 * (1 + 3 max|coordinate|): nine R entries and t rounded to float32
   (2^-24 relative each, three products per row) with a factor 4 / 3 of room for the float64 arithmetic behind them.
D. rslo_transform_points / _rows / _rows_bwd against float64, bars derived from the formats alone.
   backward: a product of two floats is exact in double, M additions in double and one rounding to float32:
   |got - ref| <= 2^-24 |ref| + M 2^-52 sum|g||x| (dt: sum|g|).
   forward: three products and three additions in float32, contracted or not:
   |got - ref| <= 4 * 2^-24 (sum_c |R_ac||x_c| + |t_a|).

Observed on the MI355X (worst error / bar over all cases of the section, and the measured reference error behind it):
  B: 0.80 -- the loss of (B, N, M) = (1, 1, 1): e32 = 1.008e-09, bar 8.07e-09, error 6.44e-09 (one source, so e32 is one
     draw of a rounding error and not a maximum over many).  Next: 0.48, the loss of (1, 16385, 16422), e32 = 2.62e-09.
     Worst gradient: 0.24, gcov2 of (3, 256, 293), e32 = 3.91e-10, error 7.61e-10.  The bars sat 5.5 to 150 times under
     their ceilings.
  C: 0.12 -- R of member 2 at N = M = 16385, first step: d_w = 1.28e-10, bar 2.39e-07, error 2.95e-08 (the float32
     rounding of R; d_w was at most 5.2e-09 for R and 7.1e-09 for t anywhere).  Worst t: 0.022.
  The N = 2 case found k_icp_solve returning a non-orthogonal matrix (|R R^T - I| = 0.49) for a rank-one H: the second
  column of U was set to the unit vector e_1 whatever the first column was.  It is now made orthogonal to the first.
"""
import functools

import numpy as np
import pytest
import torch

import closs_support as CS

pytestmark = pytest.mark.gpu


def _eq(a, b):
    return a.shape == b.shape and torch.equal(CS.bits(a), CS.bits(b))


def _is_plus_zero(t):
    return not bool(CS.bits(t).any())


# =====================================================================================================================
# A. the gather equals its promised order, bit for bit
# =====================================================================================================================
RUN_LENGTHS = (0, 1, 2, 31, 32, 33, 34, 63, 64, 65, 96, 127, 128, 129, 200, 1000, 0)


def _case_run_lengths():
    """B = 1, M = 17: partner j collects RUN_LENGTHS[j] ROI sources and about 10 % more gated-out ones (at least one, so
    partners 0 and 16 are named by sources that must not reach them); a fixed permutation scatters every run over 0..N-1."""
    part, inroi = [], []
    for j, L in enumerate(RUN_LENGTHS):
        extra = max(1, int(round(0.1 * L)))
        part += [j] * (L + extra)
        inroi += [True] * L + [False] * extra
    perm = np.random.default_rng(11).permutation(len(part))
    idx, roi = np.array(part)[perm][None], np.array(inroi)[perm][None]
    assert tuple(np.bincount(idx[roi], minlength=17)) == RUN_LENGTHS
    return CS.make_case(1, idx.shape[1], 17, idx, roi, 11)


def _case_one_partner():
    """B = 3, N = 70, M = 1: one long run per member (70, 65 and 33 sources), the same j = 0 in each."""
    roi = np.ones((3, 70), bool)
    roi[1, [3, 17, 40, 41, 69]] = False
    roi[2, np.random.default_rng(12).permutation(70)[:37]] = False
    assert tuple(roi.sum(1)) == (70, 65, 33)
    return CS.make_case(3, 70, 1, np.zeros((3, 70), int), roi, 12)


def _case_more_partners_than_sources():
    """B = 2, N = 5, M = 300: the zero-fill has to cover the partner rows past N."""
    idx = np.array([[0, 2, 2, 4, 1], [3, 3, 299, 0, 3]])
    roi = np.array([[1, 1, 1, 0, 1], [1, 1, 1, 1, 1]], bool)
    return CS.make_case(2, 5, 300, idx, roi, 13)


def _case_power_of_two_rows():
    """B = 4, M = 256, N = 300 (B M = 2^10): partner 255 of member 3 has a run of exactly 40, so the largest real key sits
    next to the all-ones key of the gated-out sources."""
    rng = np.random.default_rng(14)
    idx = rng.integers(0, 256, (4, 300))
    roi = rng.random((4, 300)) < 0.85
    idx[3][idx[3] == 255] = 254
    top = rng.permutation(300)[:44]
    idx[3, top] = 255
    roi[3, top[:40]] = True
    roi[3, top[40:]] = False
    assert int((roi[3] & (idx[3] == 255)).sum()) == 40 and int((~roi[3]).sum()) >= 4
    return CS.make_case(4, 300, 256, idx, roi, 14)


def _case_513_long_runs():
    """B = 1, M = 513, N = 513 * 33: every partner has a run of exactly 33 -- 513 long runs for 512 workgroups."""
    idx = np.random.default_rng(15).permutation(np.repeat(np.arange(513), 33))[None]
    return CS.make_case(1, 513 * 33, 513, idx, np.ones_like(idx, bool), 15)


GATHER_CASES = {"run_lengths": _case_run_lengths, "B3_N70_M1": _case_one_partner, "B2_N5_M300": _case_more_partners_than_sources,
                "B4_M256_N300": _case_power_of_two_rows, "M513_runs_of_33": _case_513_long_runs}


@pytest.mark.parametrize("name", list(GATHER_CASES))
def test_gather_equals_promised_order(hip, name):
    case = GATHER_CASES[name]()
    B, N, M = case["B"], case["N"], case["M"]
    d, u = CS.to_dev(case), CS.to_dev(CS.unrolled_case(case))
    _, cnt = CS.residual_fwd_dev(hip, d)
    assert torch.equal(cnt.cpu(), case["roi"].sum(-1).float())
    gp1, gtgt, gcov1, gcov2 = CS.residual_bwd_owned(hip, d, cnt)
    up1, utgt, ucov1, ucov2 = CS.residual_bwd_owned(hip, u, cnt)              # same cnt, same gloss
    for t in (gp1, gtgt, gcov1, gcov2, up1, utgt, ucov1, ucov2):
        assert bool(torch.isfinite(t).all()), "a row no kernel wrote, or a non-finite gradient"
    roi = d["roi"]
    # 1. the unrolled call does the same per-source arithmetic
    assert _eq(gp1, up1) and _eq(gcov1, ucov1)
    assert _is_plus_zero(gp1[~roi]) and _is_plus_zero(gcov1[~roi])
    # 2. a partner with one source holds +0 + (-gp1); one without holds +0
    zero = torch.zeros_like(up1)
    assert _eq(utgt, torch.where(roi[..., None], zero + (-up1), zero))
    assert _is_plus_zero(ucov2[~roi])
    # 3. the real call's partner rows are the emulated ordered sums of those values
    contrib = torch.cat([utgt, ucov2], -1).cpu().numpy()
    want = CS.ordered_gather_f32(contrib, case["idx"].numpy(), case["roi"].numpy(), M)
    got = torch.cat([gtgt, gcov2], -1).cpu().numpy()
    bad = np.argwhere((got.view(np.int32) != want.view(np.int32)).any(-1))
    runs = [(int(b), int(j), int((case["roi"][b] & (case["idx"][b] == j)).sum())) for b, j in bad[:8]]
    assert len(bad) == 0, "partner rows (b, j, run length) off their promised order: %s" % runs
    # 4. and the same bits again
    again = CS.residual_bwd_owned(hip, d, cnt)
    assert all(_eq(a, b) for a, b in zip(again, (gp1, gtgt, gcov1, gcov2)))


# =====================================================================================================================
# B. the per-source mathematics against float64
# =====================================================================================================================
# N at and around the wave, the block and 64 blocks of the second-stage reductions; M rotates over 1, N, N + 37
RESID_CASES = [(1, 1), (63, 3), (64, 1), (65, 3), (255, 1), (256, 3), (257, 1), (16384, 3), (16385, 1), (16384, 1), (257, 3),
               (16385, 3)]
RESID_CASES = [(B, N, (1, N, N + 37)[k % 3]) for k, (N, B) in enumerate(RESID_CASES)]
GRADS = ("gp1", "gtgt", "gcov1", "gcov2")


@functools.lru_cache(maxsize=None)
def _resid_case(B, N, M, empty_member=-1):
    rng = np.random.default_rng(1000 + 7 * N + B)
    idx = rng.integers(0, M, (B, N))                       # random, many-to-one
    roi = rng.random((B, N)) < 0.9                         # differs per member
    roi[:, 0] = roi[:, -1] = True                          # (no member empty by chance; the last block counts)
    if empty_member >= 0:
        roi[empty_member] = False
    case = CS.make_case(B, N, M, idx, roi, 1000 + N)
    return case, CS.residual_ref64(case), CS.residual_ref64(case, torch.float32)


def _resid_dev(hip, case):
    d = CS.to_dev(case)
    loss, cnt = CS.residual_fwd_dev(hip, d)
    out = dict(zip(GRADS, CS.residual_bwd_owned(hip, d, cnt)))
    out.update(loss=loss, cnt=cnt)
    return {k: v.cpu() for k, v in out.items()}


def _check_against_ref64(tag, got, ref, r32, members=None):
    """max|gpu - f64| <= 8 e32 per tensor, with the ceiling on 8 e32; prints every figure and returns the failures."""
    fails = []
    sel = (lambda t: t) if members is None else (lambda t: t[members])
    for k in ("loss",) + GRADS:
        r = sel(ref[k])
        e32 = float((sel(r32[k]).double() - r).abs().max())
        err = float((sel(got[k]).double() - r).abs().max())
        bar, ceiling = 8 * e32, (1e-5 if k == "loss" else 1e-4) * float(r.abs().max())
        print("closs B %-22s %-6s e32 %.3e  bar %.3e  ceiling %.3e  err %.3e  err/bar %.3f" %
              (tag, k, e32, bar, ceiling, err, err / bar if bar else float("inf")))
        if not bar <= ceiling:
            fails.append("%s: bar %.3e above the ceiling %.3e" % (k, bar, ceiling))
        if not err <= bar:
            fails.append("%s: error %.3e above 8 e32 = %.3e" % (k, err, bar))
    return fails


@pytest.mark.parametrize("B,N,M", RESID_CASES, ids=["B%d_N%d_M%d" % c for c in RESID_CASES])
def test_residual_matches_float64(hip, B, N, M):
    case, ref, r32 = _resid_case(B, N, M)
    got = _resid_dev(hip, case)
    assert torch.equal(got["cnt"].double(), ref["cnt"])
    for k in GRADS:
        assert bool(torch.isfinite(got[k]).all()), k
    fails = _check_against_ref64("B%d_N%d_M%d" % (B, N, M), got, ref, r32)
    assert not fails, fails


def test_residual_gated_out_member(hip):
    """B = 3 with member 1's ROI empty: cnt 0, the loss the restatement's forward gives (0 / 0), exactly +0 gradients;
    members 0 and 2 are what they are without member 1 between them, bit for bit, and within the bars of the reference."""
    case, ref, r32 = _resid_case(3, 257, 40, empty_member=1)
    got = _resid_dev(hip, case)
    assert torch.equal(got["cnt"].double(), ref["cnt"]) and float(got["cnt"][1]) == 0.0
    assert bool(torch.isnan(ref["loss"][1])) and bool(torch.isnan(got["loss"][1]))
    for k in GRADS:
        assert _is_plus_zero(got[k][1]), k
        assert not bool(ref[k][1].any())
    keep = [0, 2]
    two = {k: (v[keep].contiguous() if torch.is_tensor(v) else v) for k, v in case.items()}
    two["B"] = 2
    alone = _resid_dev(hip, two)
    for k in ("loss", "cnt") + GRADS:
        assert _eq(got[k][keep], alone[k]), k
    fails = _check_against_ref64("gated_member", got, ref, r32, members=keep)
    assert not fails, fails


# =====================================================================================================================
# C. rslo_icp_step against float64 masked_kabsch
# =====================================================================================================================
def _icp_rand_case(N, M, seed, B=3):
    rng = np.random.default_rng(seed)
    idx = np.tile(np.arange(N), (B, 1)) if M == N else rng.integers(0, M, (B, N))
    roi = rng.random((B, N)) < np.array([0.9, 0.6, 0.3])[:B, None]      # a different ROI fraction per member
    roi[:, 0] = roi[:, -1] = True
    return CS.icp_case(B, N, M, idx, roi, seed)


def _check_icp(hip, tag, case, composed=True):
    """One step from the case's running motion (and once from the identity through `first`) against the restatement."""
    B = case["B"]
    d = CS.to_dev(case)
    w64, w32 = CS.icp_weights(case, torch.float64), CS.icp_weights(case, torch.float32)
    assert w32.dtype == torch.float32
    coord = max(float(case["p1"].abs().max()), float(case["tgt"].abs().max()))
    fails = []
    starts = [("first", None, None)] + ([("composed", case["res_r"], case["res_t"])] if composed else [])
    out = {}
    for name, r0, t0 in starts:
        Rr, tr = CS.icp_ref64(case, w64, r0, t0)
        Rw, tw = CS.icp_ref64(case, w32, r0, t0)
        if r0 is None:
            res_r = torch.eye(3, device="cuda").repeat(B, 1, 1).contiguous()
            res_t = torch.zeros(B, 3, device="cuda")
        else:
            res_r, res_t = r0.cuda().clone(), t0.cuda().clone()
        CS.icp_step_dev(hip, d, res_r, res_t)
        out[name] = (res_r, res_t)
        for b in range(B):
            for what, g, r, w, scale, ceil in (("R", res_r, Rr, Rw, 1.0, 1e-5), ("t", res_t, tr, tw, 1.0 + coord, 1e-4)):
                d_w = float((w[b] - r[b]).abs().max())
                err = float((g[b].cpu().double() - r[b]).abs().max())
                bar = 4 * d_w + 2.0 ** -22 * scale
                print("closs C %-18s %-8s b%d %s d_w %.3e  bar %.3e  err %.3e  err/bar %.3f" %
                      (tag, name, b, what, d_w, bar, err, err / bar))
                if not bar < ceil:
                    fails.append("%s b%d %s: bar %.3e above the ceiling %.0e" % (name, b, what, bar, ceil))
                if not err <= bar:
                    fails.append("%s b%d %s: error %.3e above the bar %.3e" % (name, b, what, err, bar))
    # first=True on NaN-filled buffers: the bits of the eye / zeros start
    fr = torch.full((B, 3, 3), float("nan"), device="cuda")
    ft = torch.full((B, 3), float("nan"), device="cuda")
    CS.icp_step_dev(hip, d, fr, ft, first=True)
    assert _eq(fr, out["first"][0]) and _eq(ft, out["first"][1])
    assert not fails, fails
    return out


ICP_SIZES = [(255, 255), (256, 267), (257, 257), (16384, 16395), (16385, 16385), (16385, 16396)]


@pytest.mark.parametrize("N,M", ICP_SIZES, ids=["N%d_M%d" % c for c in ICP_SIZES])
def test_icp_step_matches_float64(hip, N, M):
    _check_icp(hip, "N%d_M%d" % (N, M), _icp_rand_case(N, M, 2000 + N + M))


def _icp_geometry(kind):
    """N = M = 300, idx = arange, B = 2."""
    B, N = 2, 300
    rng = np.random.default_rng(31)
    roi = rng.random((B, N)) < 0.9
    roi[:, :8] = True
    c = CS.icp_case(B, N, N, np.tile(np.arange(N), (B, 1)), roi, 31)
    if kind == "planar":                                   # z = 0 on both sides: the third singular value is exactly 0
        c["p1"][..., 2] = 0.0
        c["tgt"][..., 2] = 0.0
        a = torch.tensor([0.03, -0.05], dtype=torch.float64)
        Rz = torch.stack([torch.stack([a.cos(), -a.sin()], -1), torch.stack([a.sin(), a.cos()], -1)], -2)
        xy = c["p1"][..., :2].double() @ Rz.transpose(1, 2) + torch.tensor([[0.4, -0.2], [-0.3, 0.1]], dtype=torch.float64)[:, None]
        c["tgt"][..., :2] = (xy + 0.05 * torch.from_numpy(rng.standard_normal((B, N, 2)))).float()
    elif kind == "mirrored":                               # det(V U^T) < 0: the reflection fix
        c["tgt"] = (c["p1"] * torch.tensor([1.0, 1.0, -1.0])).contiguous()
    elif kind == "zero_weights":                           # every normal exactly perpendicular to tgt[idx] - p1
        tgt, n1 = c["p1"].clone(), torch.zeros(B, N, 3)
        e = torch.from_numpy(rng.uniform(0.1, 0.6, (B, N, 3))).float()
        tgt[:, 0::2, :2] += e[:, 0::2, :2]                 # even rows: offset in x, y (z copied: the difference is exactly 0)
        n1[:, 0::2, 2] = 1.0
        tgt[:, 1::2, 2] += e[:, 1::2, 2]                   # odd rows: offset in z, normal in the x-y plane
        n1[:, 1::2, :2] = torch.nn.functional.normalize(e[:, 1::2, :2], dim=-1)
        n1[:, 5] = 0.0                                     # a zero normal
        tgt[:, 6] = c["p1"][:, 6]                          # a target on its source
        c["tgt"], c["n1"] = tgt.contiguous(), n1.contiguous()      # (rows 0..7 are in the ROI)
    else:
        raise KeyError(kind)
    return c


@pytest.mark.parametrize("kind", ["planar", "mirrored", "zero_weights"])
def test_icp_step_degenerate_geometry(hip, kind):
    case = _icp_geometry(kind)
    if kind == "zero_weights":
        assert not bool(CS.icp_weights(case, torch.float32).any()) and not bool(CS.icp_weights(case, torch.float64).any())
    out = _check_icp(hip, kind, case)
    R, t = out["first"][0].cpu().double(), out["first"][1].cpu().double()
    assert bool((torch.det(R) > 0).all())
    assert float((R @ R.transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max()) <= 1e-6
    if kind == "zero_weights":                             # H = 0: R = I, t = the centroid difference (target -> source)
        assert _eq(out["first"][0], torch.eye(3, device="cuda").repeat(2, 1, 1))
        m = case["roi"].double()[..., None]
        diff = ((case["p1"].double() - case["tgt"].double()) * m).sum(1) / m.sum(1)
        coord = max(float(case["p1"].abs().max()), float(case["tgt"].abs().max()))
        assert float((t - diff).abs().max()) <= 2.0 ** -22 * (1 + coord)


def test_icp_step_empty_roi(hip):
    case = _icp_rand_case(300, 311, 41)
    case["roi"][:] = False
    case["dist"][:] = 5.0
    d = CS.to_dev(case)
    fr = torch.full((3, 3, 3), float("nan"), device="cuda")
    ft = torch.full((3, 3), float("nan"), device="cuda")
    CS.icp_step_dev(hip, d, fr, ft, first=True)
    assert _eq(fr, torch.eye(3, device="cuda").repeat(3, 1, 1)) and _is_plus_zero(ft)
    res_r, res_t = d["res_r"].clone(), d["res_t"].clone()
    CS.icp_step_dev(hip, d, res_r, res_t)
    assert _eq(res_r, d["res_r"]) and _eq(res_t, d["res_t"])


@pytest.mark.parametrize("N", [1, 2])
def test_icp_step_rotation_not_determined(hip, N):
    """One or two correspondences leave the rotation open: any proper rotation that maps the ROI's target centroid onto its
    source centroid is right.  Member 2 of the N = 2 case has only one of its two rows in the ROI."""
    B = 3
    roi = np.ones((B, N), bool)
    if N == 2:
        roi[2, 0] = False
    case = CS.icp_case(B, N, N, np.tile(np.arange(N), (B, 1)), roi, 50 + N)
    fr = torch.full((B, 3, 3), float("nan"), device="cuda")
    ft = torch.full((B, 3), float("nan"), device="cuda")
    CS.icp_step_dev(hip, CS.to_dev(case), fr, ft, first=True)
    R, t = fr.cpu().double(), ft.cpu().double()
    assert bool(torch.isfinite(R).all()) and bool(torch.isfinite(t).all())
    ortho = float((R @ R.transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max())
    print("closs C undetermined N=%d  |R R^T - I| %.3e  det %s" % (N, ortho, torch.det(R).tolist()))
    assert ortho <= 1e-6 and bool((torch.det(R) > 0).all())
    m = case["roi"].double()[..., None]
    cs = (case["p1"].double() * m).sum(1) / m.sum(1)
    ct = (case["tgt"].double() * m).sum(1) / m.sum(1)
    coord = max(float(case["p1"].abs().max()), float(case["tgt"].abs().max()))
    err = float(((R @ ct[..., None]).squeeze(-1) + t - cs).abs().max())
    print("closs C undetermined N=%d  centroid error %.3e  bar %.3e" % (N, err, 2.0 ** -22 * (1 + 3 * coord)))
    assert err <= 2.0 ** -22 * (1 + 3 * coord)


# =====================================================================================================================
# D. rigid transforms and their pose gradient
# =====================================================================================================================
# one block per pair up to M = 1024, several from 1025, the cap of 32 blocks with a per-thread loop from 32769
TR_SIZES = (1, 255, 256, 257, 1024, 1025, 32768, 32769, 40000)


@functools.lru_cache(maxsize=None)
def _tr_case(B, M):
    rng = np.random.default_rng(3000 + M + B)
    wide = torch.full((B, M, 7), float("nan"))             # the columns that are not the rows' must not be read
    wide[..., :3] = torch.from_numpy((rng.random((B, M, 3)) - 0.5) * np.array([20.0, 10.0, 2.0])).float()
    R = torch.from_numpy(CS._small_rotations(B, rng)).float().contiguous()
    t = torch.from_numpy(rng.uniform(-1, 1, (B, 3))).float().contiguous()
    g = torch.from_numpy(rng.standard_normal((B, M, 3))).float().contiguous()
    x64, g64, R64 = wide[..., :3].double(), g.double(), R.double()
    fwd = x64 @ R64.transpose(1, 2)
    mag = x64.abs() @ R64.abs().transpose(1, 2)
    ref = dict(fwd=fwd, mag=mag, dR=g64.transpose(1, 2) @ x64, dt=g64.sum(1),
               sR=g64.abs().transpose(1, 2) @ x64.abs(), st=g64.abs().sum(1))
    return wide, R, t, g, ref


@pytest.mark.parametrize("layout", ["contiguous", "stride7"])
@pytest.mark.parametrize("M", TR_SIZES)
def test_transform_rows_and_pose_gradient(hip, M, layout):
    for B in (1, 3):
        wide, R, t, g, ref = _tr_case(B, M)
        Rd, td, gd = R.cuda(), t.cuda(), g.cuda()
        x = wide.cuda()[:, :, :3] if layout == "stride7" else wide[..., :3].contiguous().cuda()
        assert M == 1 or x.stride(1) == (7 if layout == "stride7" else 3)
        u = 2.0 ** -24
        # forward, with and without t
        for tt in (td, None):
            out = hip.transform_rows(x, Rd, tt)
            want = ref["fwd"] + (t.double()[:, None] if tt is not None else 0.0)
            bound = 4 * u * (ref["mag"] + (t.double().abs()[:, None] if tt is not None else 0.0))
            assert bool(((out.cpu().double() - want).abs() <= bound).all()), (B, M, tt is None)
            assert _eq(out, hip.transform_rows(x, Rd, tt))
        if layout == "contiguous":
            out = hip.transform_points(x, Rd, td)
            bound = 4 * u * (ref["mag"] + t.double().abs()[:, None])
            assert bool(((out.cpu().double() - (ref["fwd"] + t.double()[:, None])).abs() <= bound).all()), (B, M)
            assert _eq(out, hip.transform_points(x, Rd, td))
        # backward with respect to the pose
        dR, dt = hip.transform_rows_bwd(x, gd)
        assert bool(((dR.cpu().double() - ref["dR"]).abs() <= u * ref["dR"].abs() + M * 2.0 ** -52 * ref["sR"]).all()), (B, M)
        assert bool(((dt.cpu().double() - ref["dt"]).abs() <= u * ref["dt"].abs() + M * 2.0 ** -52 * ref["st"]).all()), (B, M)
        dR2, dt2 = hip.transform_rows_bwd(x, gd)
        assert _eq(dR, dR2) and _eq(dt, dt2)
