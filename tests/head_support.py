"""Helpers of the head-tail, vote and pyramid-loss kernel tests (test_gpu_head_kernels.py, test_head_support_host.py).

Restatements.  vote_ref, pyramid_ref, tqn_ref, softmax_ref and masks_ref restate what csrc/vote.hip, csrc/pyramid.hip and
csrc/headtail.hip compute as plain torch on the CPU, in the dtype they are asked for: float64 is the reference, float32 the
twin the bars are measured with.  The geometry is given as three float32 values each for origin and cell size (GEOM), widened
for float64; gradients are torch.autograd's.  A `variant` argument applies ONE deliberate mistake (swapped cell sizes, the
inverse rotation, ...) for the sensitivity checks of the host test.

Bars.  Every bar is per element.

  measured   |got_i - ref64_i| <= K * 2^-24 * S_i.  S_i is the sum of the magnitudes of the terms that are added to form
             element i (the *_scales functions, float64): for a rotated vector v + 2 qs (qv x v) + 2 qv x (qv x v) it is the
             same expression with every product replaced by the product of the magnitudes and every difference by a sum, and
             v = t - x counts as |t| + |x|.  K = 4 * max |ref32_i - ref64_i| / (2^-24 S_i) over all elements of all cases
             of that output (measured_K), i.e. it is measured between the two CPU restatements and never on a kernel; the 4
             allows the kernel to associate the same expressions differently and to contract them into FMAs.  Where S_i is 0
             the two restatements must agree exactly and so must the kernel.
  derived    the sums the kernels add in double (vote_reduction, pyramid_den), from the formats alone:
             n terms that are exact in double (a float32, or the float32 product the kernel forms), added in double in any
             order: |sum^ - sum| <= n 2^-53 sum|term| =: delta, for the kernel and for the float64 reference alike, so they
             differ by at most 2 delta.  u = 2^-24.
               sums = fl32(fl32(D^) + eps32), D^ >= 0:        |sums - (D + eps32)| <= (2u + u^2)(D + eps32) + 2 delta_D (1 + 2u)
               odom = fl32(fl32(A^) / sums):  relative roundings of A^ (u), of sums (2u, above) and of the divide (u):
                 |odom - A / (D + eps32)| <= 4u |A| / S + 2 delta_A / S + 2 |A| delta_D / S^2,   S = D + eps32,
               both times (1 + 2^-20) for the second-order terms.  den = fl32(sum 3 m): u den + 2 delta, again (1 + 2^-20).
             A zero confidence map gives A = D = 0: bar 0, odom exactly 0 and sums exactly float32(1e-12).
  ceilings   max_i bar_i <= 1e-5 max|ref| for values and <= 1e-4 max|ref| for gradients (check_ceiling), the project's
             existing bars.
  floor      a softmax output whose float64 value is below 2^-126 may be off by cells * 2^-126 (flushed or denormal).
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
EPS32 = float(np.float32(1e-12))
SECOND_ORDER = 1.0 + 2.0 ** -20
# asymmetric on purpose: vx != vy != vz, ox != oy, oz != 0, none of the origins an integer
GEOM = (tuple(float(np.float32(v)) for v in (3.3, 5.7, 0.4)), tuple(float(np.float32(v)) for v in (0.4, 0.7, 1.3)))
F64, F32 = torch.float64, torch.float32


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


# --------------------------------------------------------------------------------------------------------------------
# geometry and rotation
# --------------------------------------------------------------------------------------------------------------------
def centres(H, W, dtype, variant=None, geom=GEOM):
    """[3,H,W]: x = (j - ox) vx, y = (oy - i) vy, z = (0 - oz) vz."""
    (ox, oy, oz), (vx, vy, vz) = geom
    if variant == "swap_v":
        vx, vy = vy, vx
    if variant == "swap_o":
        ox, oy = oy, ox
    i = torch.arange(H, dtype=dtype).view(H, 1).expand(H, W)
    j = torch.arange(W, dtype=dtype).view(1, W).expand(H, W)
    x = (j - ox) * vx
    y = ((i - oy) if variant == "flip_y" else (oy - i)) * vy
    z = (torch.zeros(H, W, dtype=dtype) - oz) * vz
    return torch.stack([x, y, z], 0)


def pc_range_for(H, W, geom=GEOM):
    """A point-cloud range whose grid geometry for an H x W map (rslo.data.dataset._grid_geometry) is `geom`."""
    (ox, oy, oz), (vx, vy, vz) = geom
    x0, y1, z0 = -ox * vx, oy * vy, -oz * vz
    return [x0, y1 - vy * H, z0, x0 + vx * W, y1, z0 + vz]


def rotate(v, q):
    """v + 2 qs (qv x v) + 2 qv x (qv x v), q = (w, x, y, z) as given, channels in dim 1."""
    v, qv = torch.broadcast_tensors(v, q[:, 1:])
    qs = q[:, :1]
    b = torch.cross(qv, v, dim=1)
    return v + 2 * b * qs + 2 * torch.cross(qv, b, dim=1)


def qconj(q):
    return torch.cat([q[:, :1], -q[:, 1:]], 1)


def _rot_q(q, variant, inverse):
    if variant == "q_norm_first":
        q = q / q.norm(dim=1, keepdim=True).clamp_min(1e-12)
    if (variant == "q_other_way") != inverse:
        q = qconj(q)
    return q


def abscross(a, b):
    a, b = torch.broadcast_tensors(a, b)
    a0, a1, a2 = a.unbind(1)
    b0, b1, b2 = b.unbind(1)
    return torch.stack([a1 * b2 + a2 * b1, a2 * b0 + a0 * b2, a0 * b1 + a1 * b0], 1)


def rot_scale(V, q):
    """Magnitude sum of rotate(v, q) for |v| <= V, and the one of qv x v."""
    Bm = abscross(q[:, 1:].abs(), V)
    return V + 2 * q[:, :1].abs() * Bm + 2 * abscross(q[:, 1:].abs(), Bm), Bm


def _keep(cells, variant, dtype):
    """1 for the cells a reduction keeps; the two variants lose the cells a wrong tail would lose."""
    k = torch.ones(cells, dtype=dtype)
    if variant == "drop_block":
        k[(cells // 256) * 256:] = 0
    if variant == "drop_wave":
        k[((cells - 1) // 64) * 64:] = 0
    return k


# --------------------------------------------------------------------------------------------------------------------
# vote
# --------------------------------------------------------------------------------------------------------------------
VOTE_SHAPES = ((1, 1), (1, 63), (8, 8), (5, 13), (15, 17), (16, 16), (1, 257), (257, 1), (19, 27), (33, 31))
VOTE_EXTRA = ((3, 25, 41), (65, 1, 63))          # five blocks per sample; more samples than the cached counter's first size
VOTE_CASES = tuple((B, H, W) for H, W in VOTE_SHAPES for B in (1, 3)) + VOTE_EXTRA


@functools.lru_cache(maxsize=None)
def vote_case(B, H, W):
    """|q| in 0.7 .. 1.3, q = 0 exactly in the middle cell of sample 0 (not when that is the only cell there is),
    confidences over five decades; with B >= 3 sample 1 has an all-zero t_conf and sample 2 an all-zero r_conf."""
    rng = np.random.default_rng(7000 + 1009 * H + 13 * W + B)
    cells = H * W
    tl = 2.0 * rng.standard_normal((B, 3, H, W))
    d = rng.standard_normal((B, 4, H, W))
    q = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.7, 1.3, (B, 1, H, W))
    if B * cells > 1:                                         # (a map of one cell that rotated nothing would test nothing)
        q[0, :, (cells // 2) // W, (cells // 2) % W] = 0.0
    tc = np.exp(rng.uniform(-12.0, 0.0, (B, 1, H, W)))
    rc = np.exp(rng.uniform(-12.0, 0.0, (B, 1, H, W)))
    if B >= 3:
        tc[1] = 0.0
        rc[2] = 0.0
    return dict(B=B, H=H, W=W, tq=_t(np.concatenate([tl, q], 1)), tc=_t(tc), rc=_t(rc), g=_t(rng.standard_normal((B, 7))))


def vote_ref(case, dtype=F64, variant=None):
    B, H, W = case["B"], case["H"], case["W"]
    tq, tc, rc = (case[k].to(dtype).clone().requires_grad_(True) for k in ("tq", "tc", "rc"))
    x = centres(H, W, dtype, variant)[None]
    q = tq[:, 3:]
    tg = rotate(tq[:, :3] - x, _rot_q(q, variant, False)) + x
    qg = q / q.norm(dim=1, keepdim=True).clamp_min(1e-12)
    keep = _keep(H * W, variant, dtype).view(1, 1, H, W)
    st = (tc * keep).sum(dim=(2, 3)) + 1e-12
    sr = (rc * keep).sum(dim=(2, 3)) + 1e-12
    odom = torch.cat([(tg * tc * keep).sum(dim=(2, 3)) / st, (qg * rc * keep).sum(dim=(2, 3)) / sr], 1)
    (odom * case["g"].to(dtype)).sum().backward()
    out = dict(tq_g=torch.cat([tg, qg], 1).detach(), odom=odom.detach(), sums=torch.cat([st, sr], 1).detach(),
               d_tq=tq.grad, d_tc=tc.grad, d_rc=rc.grad)
    assert all(v.dtype == dtype for v in out.values())
    return out


def vote_scales(case, ref):
    B, H, W = case["B"], case["H"], case["W"]
    tq, tc, rc, g = (case[k].to(F64) for k in ("tq", "tc", "rc", "g"))
    x = centres(H, W, F64)[None].abs()
    q = tq[:, 3:]
    V = tq[:, :3].abs() + x
    R, Bm = rot_scale(V, q)
    S_tg = R + x
    qg = ref["tq_g"][:, 3:].abs()
    n = q.norm(dim=1, keepdim=True).clamp_min(1e-12)
    st, sr = ref["sums"][:, 0].view(B, 1, 1, 1), ref["sums"][:, 1].view(B, 1, 1, 1)
    od = ref["odom"].abs().view(B, 7, 1, 1)
    gt, gq = g[:, :3].abs().view(B, 3, 1, 1), g[:, 3:].abs().view(B, 4, 1, 1)
    S_dtc = (gt * (S_tg + od[:, :3])).sum(1, keepdim=True) / st
    S_drc = (gq * (qg + od[:, 3:])).sum(1, keepdim=True) / sr
    G = gt * tc / st
    S_dtl, _ = rot_scale(G, q)
    S_dqs = 2 * (Bm * G).sum(1, keepdim=True)
    S_dqv = 2 * q[:, :1].abs() * abscross(V, G) + 2 * abscross(Bm, G) + 2 * abscross(V, abscross(G, q[:, 1:].abs()))
    Gq = gq * rc / sr
    S_nrm = (Gq + qg * (qg * Gq).sum(1, keepdim=True)) / n
    return dict(tq_g=torch.cat([S_tg, qg], 1), d_tq=torch.cat([S_dtl, torch.cat([S_dqs, S_dqv], 1) + S_nrm], 1),
                d_tc=S_dtc, d_rc=S_drc)


def vote_reduction(tq_g, tc, rc):
    """odom and sums in float64 from float32 elementwise outputs (the device's own), with the derived bars (docstring)."""
    n = tq_g.shape[2] * tq_g.shape[3]
    p = torch.cat([tq_g[:, :3] * tc, tq_g[:, 3:] * rc], 1)
    assert p.dtype == F32                                     # the float32 products the kernel forms
    A, Aabs = p.double().sum(dim=(2, 3)), p.double().abs().sum(dim=(2, 3))
    D = torch.cat([tc.double().sum(dim=(2, 3)), rc.double().sum(dim=(2, 3))], 1)
    S = D + EPS32
    S7 = torch.cat([S[:, :1].expand(-1, 3), S[:, 1:].expand(-1, 4)], 1)
    D7 = torch.cat([D[:, :1].expand(-1, 3), D[:, 1:].expand(-1, 4)], 1)
    d = n * 2.0 ** -53
    bar_odom = SECOND_ORDER * (4 * U * A.abs() / S7 + 2 * d * Aabs / S7 + 2 * A.abs() * d * D7 / S7 ** 2)
    bar_sums = SECOND_ORDER * ((2 * U + U * U) * S + 2 * d * D)
    return dict(odom=A / S7, sums=S, bar_odom=bar_odom, bar_sums=bar_sums)


# --------------------------------------------------------------------------------------------------------------------
# pyramid loss
# --------------------------------------------------------------------------------------------------------------------
PYR_SPECS = {
    # name: (H0, W0, level sizes, mask channels per level)
    "L4": (12, 9, ((74, 111), (16, 16), (3, 5), (1, 1)), (2, 3, 1, 2)),
    "L1_15x17": (12, 9, ((15, 17),), (1,)),
    "L1_1x257": (12, 9, ((1, 257),), (3,)),
    "L1_same": (12, 9, ((12, 9),), (2,)),
    "src3x24": (3, 24, ((123, 74),), (3,)),
}
PYR_CASES = tuple((name, B) for name in PYR_SPECS for B in (1, 3)) + (("L4", 17),)      # 68 rows: past the counter's first size


def nearest_index(n_src, n_dst, exact=False):
    """Source index of every destination index under torch's 'nearest' rule: F.interpolate of a float32 index grid."""
    if exact:
        return (torch.arange(n_dst) * n_src) // n_dst
    grid = torch.arange(n_src, dtype=F32).view(1, 1, n_src)
    return F.interpolate(grid, size=n_dst, mode="nearest").view(-1).long()


def pyramid_target_map(tq, H0, W0, dtype, variant=None):
    """[B,7,H0,W0]: t_l = R(q)^-1 (t_g - x) + x, q copied."""
    B = tq.shape[0]
    x = centres(H0, W0, dtype, variant)[None]
    q = tq[:, 3:].view(B, 4, 1, 1)
    t = rotate(tq[:, :3].view(B, 3, 1, 1) - x, _rot_q(q, variant, True)) + x
    return torch.cat([t, q.expand(B, 4, H0, W0)], 1)


def _resample(full, h, w, variant=None):
    H0, W0 = full.shape[2:]
    ex = variant == "exact_index"
    return full[:, :, nearest_index(H0, h, ex)][:, :, :, nearest_index(W0, w, ex)]


@functools.lru_cache(maxsize=None)
def pyramid_case(name, B):
    """Predictions 1.5 sigma around their targets; every mask channel its own values over one 60 % support; |q| in
    0.8 .. 1.2 and far from the identity; with B >= 3 every mask of sample 1 is zero."""
    H0, W0, sizes, cms = PYR_SPECS[name]
    rng = np.random.default_rng(9000 + 31 * H0 + W0 + 7 * B + len(sizes))
    t = 3.0 * rng.standard_normal((B, 3))
    d = rng.standard_normal((B, 4))
    q = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.8, 1.2, (B, 1))
    tq = _t(np.concatenate([t, q], 1))
    full = pyramid_target_map(tq.double(), H0, W0, F64)
    preds, masks = [], []
    for (h, w), cm in zip(sizes, cms):
        preds.append(_t(_resample(full, h, w).numpy() + 1.5 * rng.standard_normal((B, 7, h, w))))
        m = rng.uniform(0.1, 1.0, (B, cm, h, w)) * (rng.random((B, 1, h, w)) > 0.4)
        if B >= 3:
            m[1] = 0.0
        masks.append(_t(m))
    return dict(B=B, H0=H0, W0=W0, sizes=sizes, tq=tq, preds=preds, masks=masks, gl=_t(rng.standard_normal((len(sizes), B, 2))))


def pyramid_ref(case, dtype=F64, variant=None):
    full = pyramid_target_map(case["tq"].to(dtype), case["H0"], case["W0"], dtype, variant)
    preds = [p.to(dtype).clone().requires_grad_(True) for p in case["preds"]]
    loss, den, diffs = [], [], []
    for p, m in zip(preds, case["masks"]):
        m = m.to(dtype)
        h, w = p.shape[2:]
        d = p - _resample(full, h, w, variant)
        keep = _keep(h * w, variant, dtype).view(1, 1, h, w)
        rot_ch = min(1, m.shape[1] - 1) if variant == "rot_ch1" else m.shape[1] - 1
        row_l, row_d = [], []
        for dd, mm in ((d[:, :3], m[:, :1] * keep), (d[:, 3:], m[:, rot_ch:rot_ch + 1] * keep)):
            dn = dd.shape[1] * mm.sum(dim=(1, 2, 3))
            row_l.append((dd * dd * mm).sum(dim=(1, 2, 3)) / (dn + 1e-12))
            row_d.append(dn)
        loss.append(torch.stack(row_l, -1))
        den.append(torch.stack(row_d, -1))
        diffs.append(d.detach())
    loss_b, den = torch.stack(loss), torch.stack(den)
    (loss_b * case["gl"].to(dtype)).sum().backward()
    out = dict(loss_b=loss_b.detach(), den=den, dpred=[p.grad for p in preds], diff=diffs)
    assert loss_b.dtype == dtype and all(g.dtype == dtype for g in out["dpred"])
    return out


def pyramid_scales(case, ref):
    B, H0, W0 = case["B"], case["H0"], case["W0"]
    tq, gl = case["tq"].to(F64), case["gl"].to(F64)
    x = centres(H0, W0, F64)[None].abs()
    q = tq[:, 3:].view(B, 4, 1, 1)
    R, _ = rot_scale(tq[:, :3].abs().view(B, 3, 1, 1) + x, q)
    S_full = torch.cat([R + x, q.abs().expand(B, 4, H0, W0)], 1)
    S_loss, S_dp = [], []
    for l, (p, m) in enumerate(zip(case["preds"], case["masks"])):
        p, m = p.to(F64), m.to(F64)
        h, w = p.shape[2:]
        mag = p.abs() + _resample(S_full, h, w)
        d = ref["diff"][l].abs()
        m7 = torch.cat([m[:, :1].expand(B, 3, h, w), m[:, -1:].expand(B, 4, h, w)], 1)
        dn7 = torch.cat([ref["den"][l][:, :1].expand(B, 3), ref["den"][l][:, 1:].expand(B, 4)], 1).view(B, 7, 1, 1) + 1e-12
        g7 = torch.cat([gl[l][:, :1].expand(B, 3), gl[l][:, 1:].expand(B, 4)], 1).view(B, 7, 1, 1).abs()
        S_dp.append(mag * 2 * g7 * m7 / dn7)
        e = (2 * d * mag + 3 * d * d) * m7 / dn7
        S_loss.append(torch.stack([e[:, :3].sum(dim=(1, 2, 3)), e[:, 3:].sum(dim=(1, 2, 3))], -1))
    return dict(loss_b=torch.stack(S_loss), dpred=S_dp)


def pyramid_den(case):
    """den = n_ch sum m in float64 and its derived bar."""
    den, bar = [], []
    for m in case["masks"]:
        m = m.double()
        n = m.shape[2] * m.shape[3]
        dn = torch.stack([3 * m[:, 0].sum(dim=(1, 2)), 4 * m[:, -1].sum(dim=(1, 2))], -1)
        den.append(dn)
        bar.append(SECOND_ORDER * (U * dn + 2 * n * 2.0 ** -53 * dn))
    return torch.stack(den), torch.stack(bar)


# --------------------------------------------------------------------------------------------------------------------
# quaternion normalisation
# --------------------------------------------------------------------------------------------------------------------
TQN_CASES = tuple((B, cells) for cells in (1, 255, 256, 257, 1025) for B in (1, 3))


@functools.lru_cache(maxsize=None)
def tqn_case(B, cells):
    rng = np.random.default_rng(11000 + 3 * cells + B)
    d = rng.standard_normal((B, 4, 1, cells))
    mag = 10.0 ** rng.uniform(-3.0, 3.0, (B, 1, 1, cells))
    mag[0, 0, 0, 0], mag[-1, 0, 0, -1] = 1e-3, 1e3
    q = d / np.linalg.norm(d, axis=1, keepdims=True) * mag
    return dict(B=B, cells=cells, tq=_t(np.concatenate([rng.standard_normal((B, 3, 1, cells)), q], 1)),
                g=_t(rng.standard_normal((B, 7, 1, cells))))


def tqn_ref(case, dtype=F64):
    tq = case["tq"].to(dtype).clone().requires_grad_(True)
    out = torch.cat([tq[:, :3], tq[:, 3:] / tq[:, 3:].norm(dim=1, keepdim=True)], 1)      # no epsilon
    (out * case["g"].to(dtype)).sum().backward()
    return dict(out=out.detach(), d_tq=tq.grad)


def tqn_scales(case, ref):
    tq, g = case["tq"].to(F64), case["g"].to(F64)
    q, gq = tq[:, 3:].abs(), g[:, 3:].abs()
    n = tq[:, 3:].norm(dim=1, keepdim=True)
    S_q = gq / n + q * (q * gq).sum(1, keepdim=True) / n ** 3
    return dict(out=ref["out"].abs(), d_tq=torch.cat([g[:, :3].abs(), S_q], 1))


# --------------------------------------------------------------------------------------------------------------------
# masked spatial softmax
# --------------------------------------------------------------------------------------------------------------------
SM_CELLS = (1, 63, 64, 65, 1023, 1024, 1025, 2049, 32767, 32768)
SM_TEMP = 20.0
SM_CASES = tuple((B, cells) for cells in SM_CELLS for B in (1, 2))
SM_KINDS = ("spread", "one_inside", "all_outside")


def sm_kinds(B, cells):
    """The kind of every sample: B = 1 rotates over the three kinds with the size, B = 2 is (spread, one of the others)."""
    k = SM_CELLS.index(cells)
    return (SM_KINDS[k % 3],) if B == 1 else ("spread", SM_KINDS[1 + k % 2])


@functools.lru_cache(maxsize=None)
def sm_case(B, cells):
    """t_logit: 'spread' = uniform +-80 with 30 % outside and one inside logit of -2000 (the first and the last cell are
    inside); 'one_inside' = one inside cell; 'all_outside'.  r_logit: 3 sigma normal over the same outside mask."""
    rng = np.random.default_rng(13000 + 5 * cells + B)
    tl = rng.uniform(-80.0, 80.0, (B, 1, 1, cells))
    rl = 3.0 * rng.standard_normal((B, 1, 1, cells))
    outside = rng.random((B, 1, 1, cells)) < 0.3
    for b, kind in enumerate(sm_kinds(B, cells)):
        if kind == "spread":
            outside[b, 0, 0, 0] = outside[b, 0, 0, -1] = False
            tl[b, 0, 0, 0], tl[b, 0, 0, -1] = 79.5, 80.0       # two cells share the top: the gradient is no cancellation
            if cells > 2:
                outside[b, 0, 0, cells // 2] = False
                tl[b, 0, 0, cells // 2] = -2000.0
        elif kind == "one_inside":
            outside[b] = True
            outside[b, 0, 0, (2 * cells) // 3] = False
        else:
            outside[b] = True
    return dict(B=B, cells=cells, t_logit=_t(tl), r_logit=_t(rl), outside=torch.from_numpy(outside), temp=SM_TEMP,
                g_t=_t(rng.standard_normal((B, 1, 1, cells))), g_r=_t(rng.standard_normal((B, 1, 1, cells))))


def _masked_softmax(logit, outside, T):
    z = torch.where(outside, torch.full_like(logit, -1000.0), logit) / T
    return F.softmax(z.reshape(z.shape[0], -1), dim=-1).reshape(logit.shape)


def softmax_ref(case, dtype=F64):
    tl, rl = (case[k].to(dtype).clone().requires_grad_(True) for k in ("t_logit", "r_logit"))
    o = case["outside"]
    t_conf, r_conf = _masked_softmax(tl, o, 1.0), _masked_softmax(rl, o, 1.0)
    confT = torch.cat([_masked_softmax(tl, o, case["temp"]), _masked_softmax(rl, o, case["temp"])], 1).detach()
    ((t_conf * case["g_t"].to(dtype)).sum() + (r_conf * case["g_r"].to(dtype)).sum()).backward()
    out = dict(t_conf=t_conf.detach(), r_conf=r_conf.detach(), confT=confT, d_t=tl.grad, d_r=rl.grad)
    if dtype == F64:        # an all-outside sample is an exact output: the float32 quotient 1 / cells, not the float64 one
        rows = o.reshape(o.shape[0], -1).all(dim=1)
        for k in ("t_conf", "r_conf", "confT"):
            out[k][rows] = float(np.float32(1.0) / np.float32(case["cells"]))
    return out


def softmax_scales(case, ref):
    """p_i (1 + e_i): e_i is the magnitude of what is rounded on the way to the exponent, |z_i - m| at T = 1 and
    (|z_i| + |m| + |z_i - m|) / T otherwise.  Gradient c_i (g_i - sum c g): c_i [(|g_i| + A)(1 + e_i) + sum c |g| e]."""
    o, T = case["outside"], case["temp"]
    out = {}
    for head, logit, conf, g, d in (("t", "t_logit", "t_conf", "g_t", "d_t"), ("r", "r_logit", "r_conf", "g_r", "d_r")):
        z = torch.where(o, torch.full_like(case[logit], -1000.0), case[logit]).double()
        m = z.amax(dim=3, keepdim=True)
        e1 = (z - m).abs()
        eT = (z.abs() + m.abs() + (z - m).abs()) / T
        c, ga = ref[conf], case[g].double().abs()
        A, Ae = (c * ga).sum(3, keepdim=True), (c * ga * e1).sum(3, keepdim=True)
        out[conf] = c * (1 + e1)
        out[d] = c * ((ga + A) * (1 + e1) + Ae)
        out["T" + head] = eT
    out["confT"] = ref["confT"] * (1 + torch.cat([out.pop("Tt"), out.pop("Tr")], 1))
    rows = o.reshape(o.shape[0], -1).all(dim=1)
    for k in ("t_conf", "r_conf", "confT"):
        out[k][rows] = 0.0                                    # exact outputs (softmax_ref): bar 0
    return out


def softmax_floor(ref64, cells):
    """cells * 2^-126 where the float64 value is below the smallest normal float32 in magnitude, else 0."""
    return (ref64.abs() < 2.0 ** -126).double() * (cells * 2.0 ** -126)


# --------------------------------------------------------------------------------------------------------------------
# mask / weight pyramid
# --------------------------------------------------------------------------------------------------------------------
HM_SHAPES = ((8, 8, 4), (8, 16, 4), (16, 24, 3), (6, 10, 2), (5, 7, 1))
HM_CASES = tuple((B, H, W, L, "half") for H, W, L in HM_SHAPES for B in (1, 3)) + ((1, 8, 8, 4, "negative"),)


@functools.lru_cache(maxsize=None)
def hm_case(B, H, W, levels, kind="half"):
    """0/1 masks of about 50 % occupancy (B >= 3: sample 1 empty); kind 'negative': every mask value below zero, the
    input on which a max that counted the padding as 0 would show."""
    rng = np.random.default_rng(15000 + 101 * H + 7 * W + 3 * levels + B)
    mask = (rng.random((B, 1, H, W)) < 0.5).astype(np.float64)
    if B >= 3:
        mask[1] = 0.0
    if kind == "negative":
        mask = -rng.uniform(0.5, 1.5, (B, 1, H, W))
    conf = np.exp(rng.uniform(-8.0, 0.0, (B, 2, H, W)))
    shapes = [(B, 7, H >> k, W >> k) for k in range(levels)]
    return dict(B=B, H=H, W=W, levels=levels, mask=_t(mask), conf=_t(conf), tq=_t(rng.standard_normal(shapes[0])),
                tq_g=_t(rng.standard_normal(shapes[0])), preds=[_t(rng.standard_normal(s)) for s in shapes[1:]],
                g_mtq=_t(rng.standard_normal(shapes[0])), g_mpreds=[_t(rng.standard_normal(s)) for s in shapes[1:]])


def masks_ref(case, dtype=F64, variant=None, absent_level=None, absent_mtq=False):
    """absent_level = k: no gradient arrives for the masked prediction of level k (1-based); absent_mtq: none for mtq."""
    mask, conf, tq_g = (case[k].to(dtype) for k in ("mask", "conf", "tq_g"))
    tq = case["tq"].to(dtype).clone().requires_grad_(True)
    preds = [p.to(dtype).clone().requires_grad_(True) for p in case["preds"]]
    occ, w = [mask], [mask * conf]
    for _ in preds:
        if variant == "maxpool_pad0":
            occ.append(F.max_pool2d(F.pad(occ[-1], (1, 1, 1, 1), value=0.0), 3, 2, 0))
        else:
            occ.append(F.max_pool2d(occ[-1], 3, 2, 1))
        w.append(occ[-1] * F.avg_pool2d(w[-1], 3, 2, 1, count_include_pad=variant != "avg_valid"))
    mpreds = [p * (o > 0).to(dtype) for p, o in zip(preds, occ[1:])]
    mtq, mtq_g = tq * mask, tq_g * mask
    total = 0.0 if absent_mtq else (mtq * case["g_mtq"].to(dtype)).sum()
    for k, (mp, g) in enumerate(zip(mpreds, case["g_mpreds"]), 1):
        if k != absent_level:
            total = total + (mp * g.to(dtype)).sum()
    if torch.is_tensor(total):
        total.backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad      # noqa: E731
    return dict(w=[t.detach() for t in w], occ=[t.detach() for t in occ], mpreds=[t.detach() for t in mpreds],
                mtq=mtq.detach(), mtq_g=mtq_g.detach(), d_preds=[zero(p) for p in preds], d_tq=zero(tq))


def masks_scales(case, ref):
    S = [ref["w"][0].abs()]
    for o in ref["occ"][1:]:
        S.append(o.abs() * F.avg_pool2d(S[-1], 3, 2, 1))
    return dict(w=S)


# --------------------------------------------------------------------------------------------------------------------
# measured K, bars, ceilings
# --------------------------------------------------------------------------------------------------------------------
def ratio(r32, r64, S, floor=None):
    """max |r32 - r64| / (2^-24 S), after the floor's allowance where one applies; inf if they differ where S is 0."""
    err = (r32.double() - r64).abs()
    if floor is not None:
        err = (err - floor).clamp_min(0.0)
    pos = S > 0
    if bool((err[~pos] > 0).any()) or not bool(torch.isfinite(err).all()):
        return float("inf")
    return float((err[pos] / (U * S[pos])).max()) if bool(pos.any()) else 0.0


def _flat(d):
    """name -> list of tensors: list-valued entries (one tensor per level) are kept as lists, tensors become [tensor]."""
    return {k: (list(v) if isinstance(v, (list, tuple)) else [v]) for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def bundle(family, key):
    """(case, float64 restatement, float32 twin, scales) of one case."""
    case_fn, ref_fn, scale_fn = FAMILIES[family][1:]
    case = case_fn(*key)
    r64 = ref_fn(case, F64)
    return case, r64, ref_fn(case, F32), scale_fn(case, r64)


FAMILIES = {
    "vote": (VOTE_CASES, vote_case, vote_ref, vote_scales),
    "pyramid": (PYR_CASES, pyramid_case, pyramid_ref, pyramid_scales),
    "tqn": (TQN_CASES, tqn_case, tqn_ref, tqn_scales),
    "softmax": (SM_CASES, sm_case, softmax_ref, softmax_scales),
    "masks": (HM_CASES, hm_case, masks_ref, masks_scales),
}


@functools.lru_cache(maxsize=None)
def measured_K(family):
    """output name -> K = 4 * the largest |ref32 - ref64| / (2^-24 S) over every element of every case of the family."""
    worst = {}
    for key in FAMILIES[family][0]:
        _, r64, r32, S = bundle(family, key)
        for name, scales in _flat(S).items():
            for a, b, s in zip(_flat(r32)[name], _flat(r64)[name], scales):
                floor = softmax_floor(b, key[1]) if family == "softmax" else None
                worst[name] = max(worst.get(name, 0.0), ratio(a, b, s, floor))
    return {k: 4.0 * v for k, v in worst.items()}


def check_ceiling(bar, ref, gradient):
    """max bar <= 1e-5 (values) / 1e-4 (gradients) of max|ref|; returns (ok, max bar / max|ref|, noise_only).
    noise_only: max|ref| <= max bar, i.e. the whole tensor is a cancellation to zero within its own bars (the confidence
    gradients of a one-cell map, the logit gradients of a sample with one inside cell or none).  No bar relative to the
    tensor's maximum means anything there -- the float32 twin itself is 100 % off on that measure -- so the ceiling is
    not asked of such a tensor; the per-element bar is."""
    top, bmax = float(ref.abs().max()), float(bar.max())
    if top <= bmax:
        return True, float("inf") if bmax > 0 else 0.0, True
    frac = bmax / top
    return frac <= (1e-4 if gradient else 1e-5), frac, False


GRADIENTS = {"d_tq", "d_tc", "d_rc", "dpred", "d_t", "d_r"}


def compare(tag, name, got, ref64, bar, fails, floor=None):
    """Every element of `got` (float32, CPU) against ref64 within bar (+ floor); NaN on either side fails.  Prints the
    worst error / bar and appends to `fails`; returns that ratio."""
    got = got.detach().cpu()
    if tuple(got.shape) != tuple(ref64.shape):
        fails.append("%s %s: shape %s, expected %s" % (tag, name, tuple(got.shape), tuple(ref64.shape)))
        return float("inf")
    err = (got.double() - ref64).abs()
    lim = bar if floor is None else torch.maximum(bar, floor)
    finite = bool(torch.isfinite(got).all()) and bool(torch.isfinite(ref64).all())
    pos = lim > 0
    worst = float((err[pos] / lim[pos]).max()) if bool(pos.any()) else 0.0
    if bool((err[~pos] > 0).any()):
        worst = float("inf")
    print("head %-28s %-8s max err %.3e  max bar %.3e  worst err/bar %.3f" %
          (tag, name, float(err.max()) if err.numel() else 0.0, float(lim.max()) if lim.numel() else 0.0, worst))
    if not finite:
        fails.append("%s %s: not finite" % (tag, name))
    elif not bool((err <= lim).all()):
        i = int(torch.argmax(torch.where(pos, err / lim.clamp_min(1e-300), err * float("inf")).flatten().nan_to_num(posinf=3e38)))
        fails.append("%s %s: %d of %d elements over their bar, worst err/bar %.3f at flat index %d" %
                     (tag, name, int((err > lim).sum()), err.numel(), worst, i))
    return worst
