"""Float64 restatement of the point-normal rules of csrc/normals.hip (numpy only).

The reference computes normals offline with Open3D (script/create_hdf5.py:130-147):
    pcd.estimate_normals(KDTreeSearchParamHybrid(radius=0.6, max_nn=30)); pcd.orient_normals_towards_camera_location((0,0,0))
Open3D is not part of the reference tree and is not a dependency here: the rules are recalled from its EstimateNormals /
OrientNormalsTowardsCameraLocation / KDTreeFlann::SearchHybrid and are stated in include/rslo_hip.h.  This module is the
arbiter of the kernel's tests and a utility for scripts.  It is NOT a fallback: capi.estimate_normals never calls it.
"""
import numpy as np

RADIUS_MARGIN = 1e-4      # m: a candidate this close to the radius may fall on either side in fp32
KTH_MARGIN = 1e-5         # m: the max_nn-th and the next distance this close may swap in fp32
_CHUNK = 4_000_000        # distance-matrix entries per batch


def estimate_normals_ref(xyz, radius=0.6, max_nn=30, viewpoint=(0.0, 0.0, 0.0), zero_vertical=False):
    """xyz [P, >=3] (read as given, computed in float64).  Returns (normals [P,3] float64, counts [P] int32, gap [P],
    ambiguous [P] bool): gap = (l1 - l0) / l2 of the neighbourhood covariance (the conditioning of the normal, 0 where
    the fallback applies); ambiguous marks a query whose neighbour SET fp32 arithmetic may legitimately decide otherwise
    (a candidate within RADIUS_MARGIN of the radius while fewer than max_nn lie safely inside it, or the max_nn-th and
    (max_nn+1)-th distances within KTH_MARGIN)."""
    xyz = np.asarray(xyz)[:, :3].astype(np.float64)
    P, K = len(xyz), int(max_nn)
    radius = float(radius)
    normals = np.zeros((P, 3))
    counts = np.zeros(P, np.int32)
    gap = np.zeros(P)
    ambiguous = np.zeros(P, bool)
    ids = np.nonzero(np.isfinite(xyz).all(1))[0]          # a non-finite point is nobody's neighbour: count 0, normal 0
    if ids.size == 0:
        return normals, counts, gap, ambiguous
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
            n, cnt, g, amb = _batch(pts[q], pts[cand], cand, pts, r2, radius, K)
            normals[ids[q]], counts[ids[q]], gap[ids[q]], ambiguous[ids[q]] = n, cnt, g, amb
    # orientation towards the viewpoint, then the reader's rule
    fin = np.zeros(P, bool)
    fin[ids] = True
    v = view[None, :] - np.where(fin[:, None], xyz, 0.0)
    flip = fin & ((normals * v).sum(1) < 0)
    normals[flip] = -normals[flip]
    if zero_vertical:
        normals = np.where(np.abs(normals) == np.array([0.0, 0.0, 1.0]), 0.0, normals)
    normals[~fin] = 0.0
    return normals, counts, gap, ambiguous


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
    return n, cnt.astype(np.int32), g, amb
