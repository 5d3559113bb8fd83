"""Helpers of the consistency-loss kernel tests (test_gpu_closs_kernels.py, test_closs_support_host.py).

  make_case            float32 CPU inputs of rslo_cov_residual_fwd / _bwd with a GIVEN correspondence index and ROI
  residual_ref64       the same loss restated with rslo/core/losses.py's own functions in float64 (or float32, for the bars)
  ordered_gather_f32   numpy float32 emulation of the summation order rslo_cov_residual_bwd promises for the partner rows
  residual_fwd_dev / residual_bwd_owned
                       the C entries through capi.lib(), the backward into NaN-filled outputs the caller owns
  icp_case / icp_ref64 inputs and the float64 restatement (losses.masked_kabsch + composition) of rslo_icp_step

Nothing here runs device code to decide what is expected: the emulator is written from the rule stated in
csrc/loss.hip (k_resid_gather: one thread, ascending source order; k_resid_gather_long: lane-strided partials and a fixed
shuffle tree).
"""
import numpy as np
import torch

import rslo_amd  # noqa: F401  (makes `rslo` resolve to the mirror)

REG = 0.005            # the project's reg_weight (rslo_amd/workload.py)
RB_SHORT = 32          # csrc/loss.hip: runs up to this length are added by one thread, longer ones by one wave
WAVE = 64


# --------------------------------------------------------------------------------------------------------------------
# residual: inputs
# --------------------------------------------------------------------------------------------------------------------
def _small_rotations(B, rng):
    """A different small rotation per batch member, orthonormal in float64 and then rounded to float32."""
    q = np.concatenate([0.05 * rng.standard_normal((B, 3)), np.ones((B, 1))], 1)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    x, y, z, w = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                  2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(B, 3, 3)
    return R


def _cov_params(shape, rng):
    lam = rng.uniform(0.5, 2.0, shape + (3,))
    q = rng.standard_normal(shape + (4,))
    n = np.linalg.norm(q, axis=-1, keepdims=True)
    q = q * np.maximum(1.0, 0.5 / n)                       # |q| >= 0.5
    return np.concatenate([lam, q], -1)


def make_case(B, N, M, idx, roi, seed):
    """float32 CPU tensors for one residual call.  idx [B,N] (partner row of every source), roi [B,N] bool."""
    rng = np.random.default_rng(seed)
    idx = np.asarray(idx).reshape(B, N).astype(np.int64)
    roi = np.asarray(roi).reshape(B, N).astype(bool)
    assert idx.min() >= 0 and idx.max() < M
    tgt = ((rng.random((B, M, 3)) - 0.5) * np.array([20.0, 10.0, 2.0])).astype(np.float32)
    p1 = (np.take_along_axis(tgt, idx[..., None], 1) + 0.3 * rng.standard_normal((B, N, 3))).astype(np.float32)
    gloss = rng.uniform(0.5, 1.5, B) * np.where(rng.random(B) < 0.5, -1.0, 1.0)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return dict(B=B, N=N, M=M, p1=f(p1), tgt=f(tgt), cov1=f(_cov_params((B, N), rng)), cov2=f(_cov_params((B, M), rng)),
                Rd=f(_small_rotations(B, rng)), idx=torch.from_numpy(idx.astype(np.int32)),
                roi=torch.from_numpy(roi), dist=f(np.where(roi, 0.5, 5.0)), thr=torch.ones(B), gloss=f(gloss), reg=REG)


def unrolled_case(case):
    """The same sources with a partner row of their own each: M' = N, tgt' = tgt[idx], cov2' = cov2[idx], idx' = arange."""
    from rslo.core import losses
    B, N = case["B"], case["N"]
    il = case["idx"].long()
    out = dict(case)
    out.update(M=N, tgt=losses.gather_rows(case["tgt"], il).contiguous(), cov2=losses.gather_rows(case["cov2"], il).contiguous(),
               idx=torch.arange(N, dtype=torch.int32).repeat(B, 1).contiguous())
    return out


# --------------------------------------------------------------------------------------------------------------------
# residual: float64 restatement
# --------------------------------------------------------------------------------------------------------------------
def residual_ref64(case, dtype=torch.float64):
    """loss [B], cnt [B], gp1, gtgt, gcov1, gcov2 of pair_losses_torch's residual with the index and ROI GIVEN, evaluated
    in `dtype` on the float32 inputs (float64: the reference; float32: the same formulation, for the measured bars)."""
    from rslo.core import losses
    leaves = [case[k].to(dtype).clone().requires_grad_(True) for k in ("p1", "tgt", "cov1", "cov2")]
    p1, tgt, cov1, cov2 = leaves
    il, roi = case["idx"].long(), case["roi"]
    sig1, _ = losses.span_cov2(cov1)
    sig2, _ = losses.span_cov2(cov2)
    d = p1 - losses.gather_rows(tgt, il)
    Rd = case["Rd"].to(dtype)[:, None]
    sigma = sig1 + Rd @ losses.gather_rows(sig2, il) @ Rd.transpose(-1, -2)
    sinv, det = losses.sym3_inverse_det(sigma)
    sq = (d.unsqueeze(-2) @ sinv @ d.unsqueeze(-1)).reshape(d.shape[:2])
    cnt = roi.to(dtype).sum(-1)
    zero = torch.zeros_like(sq)
    loss = torch.where(roi, sq, zero).sum(-1) / cnt + case["reg"] * torch.where(roi, 0.5 * torch.log(det), zero).sum(-1) / cnt
    ok = cnt > 0                                            # a gated-out member: loss 0/0 = NaN, no gradient
    (loss[ok] * case["gloss"].to(dtype)[ok]).sum().backward()
    assert loss.dtype == dtype and all(t.grad.dtype == dtype for t in leaves)
    return dict(loss=loss.detach(), cnt=cnt, gp1=p1.grad, gtgt=tgt.grad, gcov1=cov1.grad, gcov2=cov2.grad)


# --------------------------------------------------------------------------------------------------------------------
# the promised summation order, in numpy float32
# --------------------------------------------------------------------------------------------------------------------
def sum_short_f32(c):
    """One thread: acc = +0.0f; acc += c[t] for t ascending.  c [K, V] float32."""
    acc = np.zeros(c.shape[1], np.float32)
    for row in c:
        acc = acc + row
    return acc


def sum_long_f32(c):
    """One wave: lane l adds rows l, l + 64, ... in order from +0.0f; then acc[l] = acc[l] + acc[l + o] for
    o = 32, 16, 8, 4, 2, 1 on the lanes with l + o < 64 (old values of the level); lane 0 is the result."""
    acc = np.zeros((WAVE, c.shape[1]), np.float32)
    for r in range(0, len(c), WAVE):
        chunk = c[r:r + WAVE]
        acc[:len(chunk)] = acc[:len(chunk)] + chunk
    for o in (32, 16, 8, 4, 2, 1):
        nxt = acc.copy()
        nxt[:WAVE - o] = acc[:WAVE - o] + acc[o:]
        acc = nxt
    return acc[0]


def sum_run_f32(c):
    c = np.ascontiguousarray(c, dtype=np.float32)
    return sum_short_f32(c) if len(c) <= RB_SHORT else sum_long_f32(c)


def ordered_gather_f32(contrib, idx, roi, M):
    """contrib [B,N,V] float32, idx [B,N], roi [B,N] -> [B,M,V] float32: partner row (b, j) is the sum of its ROI sources
    (idx == j) in ascending source order, by the short rule up to 32 sources and the wave rule above; no source: +0."""
    contrib = np.ascontiguousarray(contrib, dtype=np.float32)
    idx, roi = np.asarray(idx), np.asarray(roi).astype(bool)
    B, N, V = contrib.shape
    out = np.zeros((B, M, V), np.float32)
    for b in range(B):
        src = np.nonzero(roi[b])[0]
        order = src[np.argsort(idx[b, src], kind="stable")]          # by partner, ascending source inside a partner
        js = idx[b, order]
        cuts = np.nonzero(np.diff(js))[0] + 1
        for run in np.split(order, cuts):
            if len(run):
                out[b, idx[b, run[0]]] = sum_run_f32(contrib[b, run])
    return out


# --------------------------------------------------------------------------------------------------------------------
# device calls
# --------------------------------------------------------------------------------------------------------------------
_DEV_KEYS = ("p1", "tgt", "cov1", "cov2", "idx", "dist", "thr", "Rd", "gloss")


def to_dev(case):
    return {k: (v.cuda().contiguous() if torch.is_tensor(v) else v) for k, v in case.items()}


def residual_fwd_dev(capi, d):
    return capi.cov_residual_fwd(d["p1"], d["tgt"], d["cov1"], d["cov2"], d["idx"], d["dist"], d["thr"], d["Rd"], d["reg"])


def residual_bwd_owned(capi, d, cnt):
    """rslo_cov_residual_bwd through the C entry into NaN-filled outputs of the caller (a row no kernel writes stays NaN);
    the workspace has exactly the size rslo_cov_residual_bwd_ws_bytes asks for."""
    lib = capi.lib()
    B, N, M = d["B"], d["N"], d["M"]
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device="cuda")
    gp1, gtgt, gcov1, gcov2 = nan(B, N, 3), nan(B, M, 3), nan(B, N, 7), nan(B, M, 7)
    wsb = int(lib.rslo_cov_residual_bwd_ws_bytes(B, N, M))
    ws = torch.empty((wsb,), dtype=torch.uint8, device="cuda")
    f32, i32 = torch.float32, torch.int32
    for k in _DEV_KEYS:
        assert d[k].is_cuda and d[k].is_contiguous() and d[k].dtype == (i32 if k == "idx" else f32), k
    assert cnt.is_cuda and cnt.dtype == f32 and tuple(cnt.shape) == (B,)
    assert tuple(d["p1"].shape) == (B, N, 3) and tuple(d["tgt"].shape) == (B, M, 3) and tuple(d["idx"].shape) == (B, N)
    assert tuple(d["cov1"].shape) == (B, N, 7) and tuple(d["cov2"].shape) == (B, M, 7)
    capi._chk(lib.rslo_cov_residual_bwd(d["p1"].data_ptr(), d["tgt"].data_ptr(), d["cov1"].data_ptr(), d["cov2"].data_ptr(),
                                        d["idx"].data_ptr(), d["dist"].data_ptr(), d["thr"].data_ptr(), d["Rd"].data_ptr(),
                                        d["gloss"].data_ptr(), cnt.data_ptr(), B, N, M, float(d["reg"]), gp1.data_ptr(),
                                        gtgt.data_ptr(), gcov1.data_ptr(), gcov2.data_ptr(), ws.data_ptr(), wsb,
                                        capi._stream()), "rslo_cov_residual_bwd")
    torch.cuda.synchronize()
    return gp1, gtgt, gcov1, gcov2


def bits(t):
    """int32 view of a float32 tensor: equality of bit patterns (+0 != -0, NaN == the same NaN)."""
    return t.contiguous().view(torch.int32)


# --------------------------------------------------------------------------------------------------------------------
# ICP step
# --------------------------------------------------------------------------------------------------------------------
def icp_case(B, N, M, idx, roi, seed):
    """float32 CPU inputs of rslo_icp_step: the residual case's clouds moved by a small rigid motion, unit normals, and a
    non-identity running motion (res_r, res_t) to compose with."""
    c = make_case(B, N, M, idx, roi, seed)
    rng = np.random.default_rng(seed + 7919)
    R = torch.from_numpy(_small_rotations(B, rng))
    t = torch.from_numpy(rng.uniform(-0.5, 0.5, (B, 3)))
    tgt = (c["tgt"].double() @ R.transpose(1, 2) + t[:, None]).float().contiguous()
    n1 = torch.from_numpy(rng.standard_normal((B, N, 3)))
    n1 = (n1 / n1.norm(dim=-1, keepdim=True)).float().contiguous()
    res_r = torch.from_numpy(_small_rotations(B, rng)).float().contiguous()
    res_t = torch.from_numpy(rng.uniform(-1.0, 1.0, (B, 3))).float().contiguous()
    return dict(B=B, N=N, M=M, p1=c["p1"], n1=n1, tgt=tgt, idx=c["idx"], roi=c["roi"], dist=c["dist"], thr=c["thr"],
                res_r=res_r, res_t=res_t)


def icp_weights(case, dtype):
    """cos^2 of the angle between the normal and (tgt[idx] - p1), as _associate / pair_losses_torch form it, in `dtype`."""
    from rslo.core import losses
    assoc = losses.gather_rows(case["tgt"].to(dtype), case["idx"].long())
    w = torch.nn.functional.cosine_similarity(case["n1"].to(dtype), assoc - case["p1"].to(dtype), dim=-1).abs()
    return w * w


def icp_ref64(case, w, res_r=None, res_t=None):
    """losses.masked_kabsch in float64 on the upcast inputs with the weights `w` given, then res_r <- R res_r,
    res_t <- R res_t + t in float64.  res_r / res_t default to the identity / zeros (the `first` start)."""
    from rslo.core import losses
    B = case["B"]
    src, tgt = case["p1"].double(), case["tgt"].double()
    assoc = losses.gather_rows(tgt, case["idx"].long())
    R, t = losses.masked_kabsch(src, assoc, w.double(), case["roi"])
    rr = torch.eye(3, dtype=torch.float64).expand(B, 3, 3) if res_r is None else res_r.double()
    rt = torch.zeros(B, 3, dtype=torch.float64) if res_t is None else res_t.double()
    return R @ rr, (R @ rt[..., None]).squeeze(-1) + t


def icp_step_dev(capi, d, res_r, res_t, first=False):
    capi.icp_step(d["p1"], d["n1"], d["tgt"], d["idx"], d["dist"], d["thr"], res_r, res_t, first=first)
    torch.cuda.synchronize()
    return res_r, res_t
