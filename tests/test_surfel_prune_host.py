"""Rolling local surfel map, the float64 restatement (rslo_amd/surfels.py SurfelMapRef.prune; rules: include/rslo_hip.h
"Rolling local surfel map").  No GPU: the restatement is the arbiter of tests/test_gpu_surfel_prune.py, so it is held
here against inputs whose outcome is known in advance -- survivor counts that follow from an identity that is exact in
binary, hand-placed point counts on both sides of the inner radius, and maps built without the evicted points."""
import numpy as np
import pytest
from test_mapreg_host import IDENT, POSE_YAW, _cloud

CENTER = np.array([3.0, -2.0, 0.1])
KS = [0, 1, 63, 64, 65, 257, 1000]


def row_of_cells(n=1000, voxel=0.5):
    """[5 n, 4]: n cells in a row along x, each holding its centre and four points of the plane z = v / 2 around it (a
    planar cell, flag 2); points 0 .. n-1 are the centres.  The centre of cell i is ((i + 0.5) v, v / 2, v / 2), and
    ((i + 0.5)^2 + 0.5) v^2 < (K v)^2 holds exactly for i < K: every term is exact in binary at v = 0.5"""
    pts = np.zeros((5, n, 4), np.float32)
    pts[:, :, 0] = (np.arange(n) + 0.5) * voxel
    pts[:, :, 1:3] = 0.5 * voxel
    for k, (dx, dy) in enumerate(((-1, -1), (-1, 1), (1, -1), (1, 1))):
        pts[k + 1, :, 0] += 0.25 * voxel * dx
        pts[k + 1, :, 1] += 0.25 * voxel * dy
    return pts.reshape(-1, 4)


def key_of(cx, cy, cz):
    return ((cx + (1 << 20)) << 42) | ((cy + (1 << 20)) << 21) | (cz + (1 << 20))


def counted_cells():
    """Twelve 1 m cells (i, 0, 0), i = 0 .. 11, holding (i % 6) + 1 points each: with the centre at the origin and
    inner_radius 6, (i + 0.5)^2 + 0.5 < 36 holds for i <= 5, so counts 1 .. 6 lie inside and counts 1 .. 6 outside"""
    rng = np.random.default_rng(17)
    pts = [np.concatenate([rng.uniform(0.1, 0.9, (i % 6 + 1, 3)) + (i, 0, 0), np.zeros((i % 6 + 1, 1))], axis=1)
           for i in range(12)]
    return np.concatenate(pts).astype(np.float32)


def snapshot(ref):
    return ref.keys.copy(), ref.moments.copy(), ref.rows.copy(), ref.stats(), ref.prune_stats()


def two_scans(voxel=2.0, **kw):
    from rslo_amd.surfels import SurfelMapRef
    ref = SurfelMapRef(voxel, **kw)
    ref.insert(_cloud(0), IDENT)
    ref.insert(_cloud(5), POSE_YAW)
    return ref


@pytest.mark.parametrize("K", KS)
def test_survivor_counts(K):
    from rslo_amd.surfels import SurfelMapRef
    ref = SurfelMapRef(0.5)
    ref.insert(row_of_cells(), IDENT)
    assert ref.stats()["n_cells"] == 1000 == ref.stats()["n_planar"]
    assert ref.prune_stats() == {"n_prunes": 0, "n_evicted": 0, "n_lost": 0}
    ref.prune(np.zeros(3), K * 0.5)
    assert ref.stats()["n_cells"] == K == len(ref.keys) == ref.stats()["n_planar"]
    assert ref.prune_stats() == {"n_prunes": 1, "n_evicted": 1000 - K, "n_lost": 0}
    assert (ref.keys == key_of(np.arange(K), 0, 0)).all()                 # the K cells nearest the origin, no others
    assert ref.stats()["n_points"] == 5000 and ref.stats()["n_scans"] == 1      # cumulative counters stay


@pytest.mark.parametrize("min_count", [1, 2, 4, 6, 7])
def test_sparse_rule(min_count):
    from rslo_amd.surfels import SurfelMapRef
    ref = SurfelMapRef(1.0)
    ref.insert(counted_cells(), IDENT)
    assert ref.moments[:, 0].tolist() == [1, 2, 3, 4, 5, 6] * 2
    ref.prune(np.zeros(3), 100.0, inner_radius=6.0, min_count=min_count)
    want = [i for i in range(12) if i < 6 or i % 6 + 1 >= min_count]    # beyond the inner radius the sparse cells go
    assert ref.keys.tolist() == [key_of(i, 0, 0) for i in want]
    assert ref.prune_stats()["n_evicted"] == 12 - len(want)
    everywhere = SurfelMapRef(1.0)
    everywhere.insert(counted_cells(), IDENT)
    everywhere.prune(min_count=min_count)                                # no centre: no exemption
    assert everywhere.keys.tolist() == [key_of(i, 0, 0) for i in range(12) if i % 6 + 1 >= min_count]
    same = SurfelMapRef(1.0)                                             # inner_radius=None means radius
    same.insert(counted_cells(), IDENT)
    same.prune(np.zeros(3), 6.0, min_count=min_count)
    assert same.keys.tolist() == [key_of(i, 0, 0) for i in range(6)]
    inner0 = SurfelMapRef(1.0)                                           # inner_radius 0: no cell is exempt
    inner0.insert(counted_cells(), IDENT)
    inner0.prune(np.zeros(3), 100.0, inner_radius=0.0, min_count=min_count)
    assert inner0.keys.tolist() == everywhere.keys.tolist()


def test_kept_cells_keep_their_bits_and_n_planar_is_recounted():
    ref = two_scans(2.0)
    keys0, mom0, rows0, st0, _ = snapshot(ref)
    ref.prune(CENTER, 9.0, inner_radius=5.0, min_count=8)
    assert 20 < len(ref.keys) < len(keys0) - 20
    at = np.searchsorted(keys0, ref.keys)
    assert (keys0[at] == ref.keys).all()
    assert ref.moments.tobytes() == mom0[at].tobytes() and ref.rows.tobytes() == rows0[at].tobytes()
    st = ref.stats()
    assert st["n_planar"] == int((ref.rows[:, 7] == 2.0).sum()) and 0 < st["n_planar"] < st0["n_planar"]
    assert st == dict(st0, n_cells=len(ref.keys), n_planar=st["n_planar"])
    # the survivors are exactly the cells the rule names, judged by the cell's centre and not by the row's mean
    cell = np.stack([(keys0 >> 42) & 0x1fffff, (keys0 >> 21) & 0x1fffff, keys0 & 0x1fffff], axis=1) - (1 << 20)
    d2 = (((cell + 0.5) * 2.0 - CENTER) ** 2).sum(axis=1)
    want = (d2 < 81.0) & ((mom0[:, 0] >= 8) | (d2 < 25.0))
    assert abs(d2 - 81.0).min() > 1e-6 and abs(d2 - 25.0).min() > 1e-6      # no cell on a boundary: the sums' order is moot here
    assert (keys0[want] == ref.keys).all()
    flag0 = rows0[:, 7] == 0.0
    assert (want & flag0).sum() > 0 and (~want & flag0).sum() > 0          # rows of zeros on both sides


def test_insert_into_an_evicted_cell_starts_from_zero():
    from rslo_amd.surfels import SurfelMapRef
    A, B = _cloud(0), _cloud(5)
    ref = SurfelMapRef(2.0)
    ref.insert(A, IDENT)
    keysA = ref.keys.copy()
    ref.prune(CENTER, 6.0)
    kept = ref.keys.copy()
    gone = np.setdiff1d(keysA, kept)
    ref.insert(B, POSE_YAW)
    alone, both = SurfelMapRef(2.0), SurfelMapRef(2.0)
    alone.insert(B, POSE_YAW)
    both.insert(A, IDENT)
    both.insert(B, POSE_YAW)
    again = np.intersect1d(gone, alone.keys)                              # evicted, then hit by B
    stayed = np.intersect1d(kept, alone.keys)
    assert len(again) > 20 and len(stayed) > 20 and len(kept) > 20
    i, j = np.searchsorted(ref.keys, again), np.searchsorted(alone.keys, again)
    assert ref.moments[i].tobytes() == alone.moments[j].tobytes() and ref.rows[i].tobytes() == alone.rows[j].tobytes()
    i, j = np.searchsorted(ref.keys, stayed), np.searchsorted(both.keys, stayed)
    assert ref.moments[i].tobytes() == both.moments[j].tobytes() and ref.rows[i].tobytes() == both.rows[j].tobytes()
    assert (np.sort(np.concatenate([kept, np.setdiff1d(alone.keys, kept)])) == ref.keys).all()
    assert ref.stats()["n_cells"] == len(ref.keys) and ref.stats()["n_planar"] == int((ref.rows[:, 7] == 2.0).sum())


def test_a_call_that_evicts_nothing_changes_only_n_prunes():
    ref = two_scans(2.0)
    before = snapshot(ref)
    calls = (dict(), dict(center=CENTER, radius=float("inf")), dict(center=POSE_YAW, radius=1.0e4),
             dict(center=CENTER, radius=1.0e4, inner_radius=1.0e4, min_count=10 ** 6))
    for n, kw in enumerate(calls):
        ref.prune(**kw)
        now = snapshot(ref)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before[:3], now[:3])) and now[3] == before[3]
        assert now[4] == {"n_prunes": n + 1, "n_evicted": 0, "n_lost": 0}


def test_radius_zero_and_a_nan_centre_evict_everything():
    for kw in (dict(center=CENTER, radius=0.0), dict(center=np.array([np.nan, 0.0, 0.0]), radius=float("inf")),
               dict(center=np.array([0.0, 0.0, np.nan]), radius=10.0, min_count=3)):
        ref = two_scans(2.0)
        n, st0 = len(ref.keys), ref.stats()
        ref.prune(**kw)
        assert len(ref.keys) == 0 and ref.moments.shape == (0, 10) and ref.rows.shape == (0, 8)
        assert ref.stats() == dict(st0, n_cells=0, n_planar=0)
        assert ref.prune_stats() == {"n_prunes": 1, "n_evicted": n, "n_lost": 0}
        ref.insert(_cloud(5), POSE_YAW)                                   # and the map lives on
        assert ref.stats()["n_cells"] > 50
    ref.reset()
    assert ref.prune_stats() == {"n_prunes": 0, "n_evicted": 0, "n_lost": 0}


def test_argument_errors():
    from rslo_amd.surfels import check_surfel_prune
    ref = two_scans(2.0)
    before = snapshot(ref)
    nan = float("nan")
    for kw in (dict(center=CENTER), dict(center=CENTER, radius=-1.0), dict(center=CENTER, radius=nan),
               dict(center=CENTER, radius=5.0, inner_radius=5.5), dict(center=CENTER, radius=5.0, inner_radius=-0.1),
               dict(center=CENTER, radius=5.0, inner_radius=nan), dict(min_count=0), dict(min_count=2.5),
               dict(center=CENTER, radius=5.0, min_count=-3), dict(radius=-2.0)):
        with pytest.raises(ValueError):
            ref.prune(**kw)
    now = snapshot(ref)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before[:3], now[:3])) and now[3:] == before[3:]
    assert check_surfel_prune(CENTER, 5, None, 2) == (5.0, 5.0, 2)
    assert check_surfel_prune(None, None, None, 1) == (0.0, 0.0, 1)
    assert check_surfel_prune(None, 30.0, 15.0, 2, has_center=True) == (30.0, 15.0, 2)
    assert check_surfel_prune(CENTER, float("inf"), float("inf"), 1) == (float("inf"), float("inf"), 1)
    with pytest.raises(ValueError):
        check_surfel_prune(None, None, None, 1, has_center=True)
