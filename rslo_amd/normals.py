"""Float64 restatement of the point-normal rules of csrc/normals.hip, and the fp32 twin of its kernel (numpy only).

The reference computes normals offline with Open3D (script/create_hdf5.py:130-147):
    pcd.estimate_normals(KDTreeSearchParamHybrid(radius=0.6, max_nn=30)); pcd.orient_normals_towards_camera_location((0,0,0))
Open3D is not part of the reference tree and is not a dependency here: the rules are recalled from its EstimateNormals /
OrientNormalsTowardsCameraLocation / KDTreeFlann::SearchHybrid and are stated in include/rslo_hip.h.  This module is the
arbiter of the kernel's tests and a utility for scripts.  It is NOT a fallback: capi.estimate_normals never calls it.

estimate_normals_ref states the RULES in float64 (which neighbours, which eigenvector); estimate_normals_f32 restates the
KERNEL operation by operation in float32, so that the kernel can be compared with it bit for bit, selected set included.
"""
import numpy as np

RADIUS_MARGIN = 1e-4      # m: a candidate this close to the radius may fall on either side in fp32
KTH_MARGIN = 1e-5         # m: the max_nn-th and the next distance this close may swap in fp32
_CHUNK = 4_000_000        # distance-matrix entries per batch


def estimate_normals_ref(xyz, radius=0.6, max_nn=30, viewpoint=(0.0, 0.0, 0.0), zero_vertical=False, selected=False):
    """xyz [P, >=3] (read as given, computed in float64).  Returns (normals [P,3] float64, counts [P] int32, gap [P],
    ambiguous [P] bool): gap = (l1 - l0) / l2 of the neighbourhood covariance (the conditioning of the normal, 0 where
    the fallback applies); ambiguous marks a query whose neighbour SET fp32 arithmetic may legitimately decide otherwise
    (a candidate within RADIUS_MARGIN of the radius while fewer than max_nn lie safely inside it, or the max_nn-th and
    (max_nn+1)-th distances within KTH_MARGIN).  selected=True appends the neighbour set itself: [P, max_nn] int64
    original indices in ascending (float64 distance, index), -1 where empty."""
    xyz = np.asarray(xyz)[:, :3].astype(np.float64)
    P, K = len(xyz), int(max_nn)
    radius = float(radius)
    normals = np.zeros((P, 3))
    counts = np.zeros(P, np.int32)
    gap = np.zeros(P)
    ambiguous = np.zeros(P, bool)
    chosen = np.full((P, K), -1, np.int64)
    ids = np.nonzero(np.isfinite(xyz).all(1))[0]          # a non-finite point is nobody's neighbour: count 0, normal 0
    if ids.size == 0:
        return (normals, counts, gap, ambiguous, chosen) if selected else (normals, counts, gap, ambiguous)
    pts = xyz[ids]
    # cell grid of edge 2 * radius: the neighbours of a point lie in the 27 cells around its own
    cells = np.floor(np.clip(pts / (2.0 * radius), -1e15, 1e15)).astype(np.int64)
    ucells, inv = np.unique(cells, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    order = np.argsort(inv, kind="stable")                # members of a cell in ascending original index
    start = np.searchsorted(inv[order], np.arange(len(ucells) + 1))
    lookup = {tuple(c): k for k, c in enumerate(ucells.tolist())}
    nbr = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)]
    view = np.asarray(viewpoint, np.float64)
    r2 = radius * radius
    for k, c in enumerate(ucells.tolist()):
        near = [lookup.get((c[0] + a, c[1] + b, c[2] + d)) for a, b, d in nbr]
        cand = np.sort(np.concatenate([order[start[j]:start[j + 1]] for j in near if j is not None]))
        members = order[start[k]:start[k + 1]]
        step = max(1, _CHUNK // len(cand))
        for s in range(0, len(members), step):
            q = members[s:s + step]
            n, cnt, g, amb, idx = _batch(pts[q], pts[cand], cand, pts, r2, radius, K)
            normals[ids[q]], counts[ids[q]], gap[ids[q]], ambiguous[ids[q]] = n, cnt, g, amb
            chosen[ids[q]] = np.where(idx >= 0, ids[np.maximum(idx, 0)], -1)
    # orientation towards the viewpoint, then the reader's rule
    fin = np.zeros(P, bool)
    fin[ids] = True
    v = view[None, :] - np.where(fin[:, None], xyz, 0.0)
    flip = fin & ((normals * v).sum(1) < 0)
    normals[flip] = -normals[flip]
    if zero_vertical:
        normals = np.where(np.abs(normals) == np.array([0.0, 0.0, 1.0]), 0.0, normals)
    normals[~fin] = 0.0
    return (normals, counts, gap, ambiguous, chosen) if selected else (normals, counts, gap, ambiguous)


def _batch(Q, C, cand, pts, r2, radius, K):
    """Q [q,3] queries against candidates C [c,3] (ascending original index, so a stable sort breaks ties by index)."""
    d = Q[:, None, :] - C[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    inside = d2 < r2
    total = inside.sum(1)
    d2m = np.where(inside, d2, np.inf)
    if d2m.shape[1] < K + 1:
        d2m = np.concatenate([d2m, np.full((len(Q), K + 1 - d2m.shape[1]), np.inf)], 1)
    sel = np.argsort(d2m, axis=1, kind="stable")[:, :K + 1]
    dsel = np.take_along_axis(d2m, sel, 1)
    cnt = np.minimum(total, K)
    dist = np.sqrt(d2)
    # a candidate at the radius matters only while fewer than max_nn candidates are safely inside it
    amb = (np.abs(dist - radius) < RADIUS_MARGIN).any(1) & ((dist <= radius - RADIUS_MARGIN).sum(1) < K)
    over = total > K
    amb |= over & (np.sqrt(np.where(over, dsel[:, K], 0.0)) - np.sqrt(np.where(over, dsel[:, K - 1], 0.0)) < KTH_MARGIN)
    use = np.arange(K)[None, :] < cnt[:, None]
    idx = cand[np.minimum(sel[:, :K], len(cand) - 1)]
    off = (pts[idx] - Q[:, None, :]) * use[..., None]          # offsets about the query, never raw coordinates
    safe = np.maximum(cnt, 1)[:, None]
    mean = off.sum(1) / safe
    dev = (off - mean[:, None, :]) * use[..., None]
    cov = np.einsum("qki,qkj->qij", dev, dev) / safe[..., None]
    w, v = np.linalg.eigh(cov)
    n = v[:, :, 0].copy()
    norm = np.linalg.norm(n, axis=1)
    ok = (cnt >= 3) & np.isfinite(norm) & (norm > 0)
    n[ok] /= norm[ok, None]
    n[~ok] = (0.0, 0.0, 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(ok & (w[:, 2] > 0), (w[:, 1] - w[:, 0]) / w[:, 2], 0.0)
    return n, cnt.astype(np.int32), g, amb, np.where(use, idx, -1)


# ---------------------------------------------------------------------------------------------------------------------
# the fp32 twin of k_nm_normals
# ---------------------------------------------------------------------------------------------------------------------
_F = np.float32
_KEY_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
_TWIN_BATCH = 2_000_000      # distance-matrix entries per batch


def _f32(*arrays):
    """every intermediate of the twin is float32: a silent promotion to float64 would round differently"""
    for a in arrays:
        assert a.dtype == np.float32, a.dtype
    return arrays[0] if len(arrays) == 1 else arrays


def _rot_f32(app, aqq, apq, arp, arq, v0p, v0q, v1p, v1q, v2p, v2q):
    """nm_rot (csrc/normals.hip:139-154) on arrays: lanes with apq == 0 keep every value (the early exit)."""
    live = apq != _F(0)
    theta = _f32((aqq - app) / (_F(2) * apq))
    t = _f32(np.copysign(_F(1), theta) / (np.abs(theta) + np.sqrt(theta * theta + _F(1))))
    c = _f32(_F(1) / np.sqrt(t * t + _F(1)))
    s = _f32(t * c)
    new = [app - t * apq, aqq + t * apq, np.zeros_like(apq), c * arp - s * arq, s * arp + c * arq,
           c * v0p - s * v0q, s * v0p + c * v0q, c * v1p - s * v1q, s * v1p + c * v1q, c * v2p - s * v2q,
           s * v2p + c * v2q]
    old = [app, aqq, apq, arp, arq, v0p, v0q, v1p, v1q, v2p, v2q]
    return [_f32(np.where(live, n, o)) for n, o in zip(new, old)]


def estimate_normals_f32(xyz, radius=0.6, max_nn=30, viewpoint=(0.0, 0.0, 0.0), zero_vertical=False):
    """The host twin of k_nm_normals (csrc/normals.hip:156-270), as gauss_newton.py is of gauss_newton.h: the kernel
    restated operation by operation on float32 arrays, so that the kernel can be held to it bit for bit.  That is
    possible because the kernel is compiled with fp contract(off) and without fast-math, every operation is one
    correctly rounded fp32 + - * / or sqrtf, the selection key is total, and the sums run in key order.
    xyz [P, >=3] (cast to float32 as capi does not: pass float32).  Returns (normals [P,3] float32, counts [P] int32,
    selected [P, max_nn] int64: original indices in ascending key order, -1 where empty).

    What is restated, with the kernel's lines:
      :310     r2 = f32(radius) * f32(radius) (the launch's argument)
      :168     a point is finite when its three coordinates are; a non-finite point selects nothing
      :202-205 d = p_j - q, d2 = (dx*dx + dy*dy) + dz*dz, candidate when d2 < r2, key = d2 bits << 32 | j
      :128-136, :220 the max_nn smallest keys (the 32-entry list holds the 32 smallest, the sums read its first max_nn)
      :216-228 s0..s2 and m00..m22 in ascending key order from o = p_j - q, every product rounded before it is added
      :231-235 ic = 1 / cnt, mean = s * ic, a = m * ic - mean * mean, tr = (a00 + a11) + a22
      :236-238 gate tr > 0 && tr < inf, scale by 1 / tr
      :240-244 six sweeps of nm_rot in the order (0,1,2), (0,2,1), (1,2,0)
      :245-251 smallest diagonal entry, ties to the lower index; n = e / sqrtf((ex*ex + ey*ey) + ez*ez); else (0, 0, 1)
      :254-256 flip when (nx*(vx-qx) + ny*(vy-qy)) + nz*(vz-qz) < 0
      :257-261 zero_vertical, -0 -> +0 included
      :262-265 a non-finite point: zero normal, count 0
    The cell grid is not restated: the key order makes the selected set independent of the order of arrival, so brute
    force over all pairs selects what the kernel must.  A test arbiter and a script utility; capi never calls it."""
    pts = np.ascontiguousarray(np.asarray(xyz)[:, :3], dtype=np.float32)
    P, K = len(pts), int(max_nn)
    if not 3 <= K <= 32:
        raise ValueError("max_nn must be in 3..32, got %d" % K)
    r2 = _f32(_F(radius) * _F(radius))
    view = np.asarray(viewpoint, np.float32)
    normals = np.zeros((P, 3), np.float32)
    counts = np.zeros(P, np.int32)
    selected = np.full((P, K), -1, np.int64)
    if P == 0:
        return normals, counts, selected
    fin = np.isfinite(pts).all(1)
    index = np.arange(P, dtype=np.uint64)
    step = max(1, _TWIN_BATCH // P)
    with np.errstate(all="ignore"):
        for b in range(0, P, step):
            q = pts[b:b + step]
            n, c, s = _twin_batch(q, fin[b:b + step], pts, fin, index, r2, K, view, bool(zero_vertical))
            normals[b:b + step], counts[b:b + step], selected[b:b + step] = n, c, s
    return normals, counts, selected


def _twin_batch(q, qfin, pts, fin, index, r2, K, view, zero_vertical):
    B = len(q)
    qx, qy, qz = q[:, 0], q[:, 1], q[:, 2]
    # selection
    dx, dy, dz = _f32(pts[None, :, 0] - qx[:, None], pts[None, :, 1] - qy[:, None], pts[None, :, 2] - qz[:, None])
    d2 = _f32((dx * dx + dy * dy) + dz * dz)
    ok = (d2 < r2) & fin[None, :] & qfin[:, None]                 # NaN / inf distances never qualify
    keys = np.where(ok, (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | index[None, :], _KEY_NONE)
    if keys.shape[1] < K:
        keys = np.concatenate([keys, np.full((B, K - keys.shape[1]), _KEY_NONE)], 1)
    best = np.partition(keys, K - 1, axis=1)[:, :K]
    best.sort(axis=1)
    assert best.dtype == np.uint64
    used = best != _KEY_NONE
    sel = np.where(used, (best & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    cnt = used.sum(1).astype(np.int32)
    # sums in key order, about the query
    zero = np.zeros(B, np.float32)
    s0, s1, s2, m00, m01, m02, m11, m12, m22 = (zero.copy() for _ in range(9))
    for j in range(K):
        u = used[:, j]
        p = pts[np.maximum(sel[:, j], 0)]
        ox, oy, oz = _f32(p[:, 0] - qx, p[:, 1] - qy, p[:, 2] - qz)
        s0, s1, s2 = np.where(u, s0 + ox, s0), np.where(u, s1 + oy, s1), np.where(u, s2 + oz, s2)
        m00, m01, m02 = np.where(u, m00 + ox * ox, m00), np.where(u, m01 + ox * oy, m01), np.where(u, m02 + ox * oz, m02)
        m11, m12, m22 = np.where(u, m11 + oy * oy, m11), np.where(u, m12 + oy * oz, m12), np.where(u, m22 + oz * oz, m22)
    _f32(s0, s1, s2, m00, m01, m02, m11, m12, m22)
    # covariance, trace-scaled
    ic = _f32(_F(1) / cnt.astype(np.float32))
    mx, my, mz = _f32(s0 * ic, s1 * ic, s2 * ic)
    a00, a01, a02 = _f32(m00 * ic - mx * mx, m01 * ic - mx * my, m02 * ic - mx * mz)
    a11, a12, a22 = _f32(m11 * ic - my * my, m12 * ic - my * mz, m22 * ic - mz * mz)
    tr = _f32((a00 + a11) + a22)
    gate = (cnt >= 3) & (tr > _F(0)) & (tr < _F(np.inf))
    sc = _f32(_F(1) / tr)
    a00, a01, a02, a11, a12, a22 = _f32(a00 * sc, a01 * sc, a02 * sc, a11 * sc, a12 * sc, a22 * sc)
    one = np.ones(B, np.float32)
    v00, v01, v02, v10, v11, v12, v20, v21, v22 = one, zero, zero, zero, one, zero, zero, zero, one
    for _ in range(6):
        a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21 = _rot_f32(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21)
        a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22 = _rot_f32(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22)
        a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22 = _rot_f32(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22)
    c1 = a11 < a00                                       # smallest eigenvalue, ties to the lower index
    c2 = a22 < np.where(c1, a11, a00)
    ex = np.where(c2, v02, np.where(c1, v01, v00))
    ey = np.where(c2, v12, np.where(c1, v11, v10))
    ez = np.where(c2, v22, np.where(c1, v21, v20))
    nn = _f32(np.sqrt((ex * ex + ey * ey) + ez * ez))
    good = gate & (nn > _F(0)) & (nn < _F(np.inf))
    nx, ny, nz = _f32(np.where(good, ex / nn, zero), np.where(good, ey / nn, zero), np.where(good, ez / nn, one))
    # orientation, the reader's rule, non-finite points
    flip = _f32((nx * (view[0] - qx) + ny * (view[1] - qy)) + nz * (view[2] - qz)) < _F(0)
    nx, ny, nz = np.where(flip, -nx, nx), np.where(flip, -ny, ny), np.where(flip, -nz, nz)
    if zero_vertical:
        nx = np.where(nx == _F(0), zero, nx)             # -0 -> +0
        ny = np.where(ny == _F(0), zero, ny)
        nz = np.where(np.abs(nz) == _F(1), zero, nz)
    out = np.stack(_f32(nx, ny, nz), 1)
    out[~qfin] = 0.0
    cnt[~qfin] = 0
    return _f32(out), cnt, sel
