"""The float64 restatement of place recognition (rslo_amd/places.py ScanContextRef / PlaceDBRef; rules: include/rslo_hip.h
"Place recognition"): the edge rules of the descriptor, the corner cases of the database and the query, and a revisit on
the synthetic street.  No GPU.  tests/test_gpu_places.py holds the kernels to these classes bit for bit."""
import numpy as np
import pytest

from rslo_amd import places, synthetic

R, S, RANGE, ZOFF = 20, 60, 80.0, 2.0


def edge_clouds():
    """name -> [P, 3] float32; shared with the GPU test.  Every radius below is exact in float32."""
    out = {}
    # the four axes at radius 10 (ring 2) and the diagonals at 10 sqrt 2 (ring 3): exactly on a sector boundary for S = 60 (90 deg = 15 sectors)
    # and in the middle of one (45 deg = 7.5 sectors)
    a = np.float32(10.0)
    out["axes_diagonals"] = np.array([[a, 0, 0], [0, a, 0], [-a, 0, 0], [0, -a, 0], [a, a, 0], [-a, a, 0], [-a, -a, 0],
                                      [a, -a, 0]], np.float32)
    # exactly at r = k * max_range / R = 4 k, on the x axis and on a 3-4-5 direction (r = 20 = 5 * 4: (12, 16))
    ring = [[4.0 * k, 0, 0.5] for k in range(0, R + 2)] + [[12.0, 16.0, 0.5], [-16.0, 12.0, 0.25], [48.0, -64.0, 1.0],
                                                           [np.nextafter(np.float32(8.0), np.float32(0)), 0, 0.5]]
    out["ring_edges"] = np.array(ring, np.float32)
    out["origin"] = np.array([[0, 0, 0], [0, 0, 5.0], [-0.0, 0.0, 1.0], [1e-30, 0, 1.0]], np.float32)
    out["far"] = np.array([[80.0, 0, 0], [0, -80.0, 0], [100.0, 100.0, 0], [79.99999, 0, 0], [48.0, 64.0, 0], [3e38, 0, 0],
                           [3e38, 3e38, 0]], np.float32)
    out["low"] = np.array([[5, 5, -2.0], [5, 5, -2.5], [5, 5, np.nextafter(np.float32(-2.0), np.float32(0))], [5, 5, -1e30],
                           [-7, 3, -1.9999]], np.float32)
    out["non_finite"] = np.array([[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [1, 1, np.nan], [np.inf, np.inf, np.inf],
                                  [3, 4, 1]], np.float32)
    out["duplicates"] = np.array([[10, 1, 0.5], [10, 1, 1.5], [10, 1, -0.5], [10.01, 1.01, 1.5], [10, 1, 0.25]], np.float32)
    return out


def street_db():
    """the 61 descriptors of the street, x = -60, -58, ..., 60, made once per process and never modified"""
    if "db" not in _STREET:
        sc = places.ScanContextRef(R, S, RANGE, ZOFF)
        _STREET["db"] = [sc.describe(synthetic.scan(720, 16, (-60.0 + 2.0 * k, 0.0), 0.0, scan_seed=k))[:3] for k in range(61)]
    return _STREET["db"]


def street_queries():
    if "q" not in _STREET:
        sc = places.ScanContextRef(R, S, RANGE, ZOFF)
        qs = []
        for k in range(2, 59, 4):
            scan = synthetic.scan(720, 16, (-60.0 + 2.0 * k + 0.7, 0.8), np.pi + 0.1, scan_seed=1000 + k)
            qs.append((k, scan, sc.describe(scan)[:3], sc.no_sector))
        _STREET["q"] = qs
    return _STREET["q"]


_STREET = {}


def _sc():
    return places.ScanContextRef(R, S, RANGE, ZOFF)


def test_tables():
    t = places.tables(R, S, RANGE)
    assert t.shape == (2 * (S + 1) + R + 1,) and t.dtype == np.float64
    dirs, edge2 = t[:2 * (S + 1)].reshape(S + 1, 2), t[2 * (S + 1):]
    assert dirs[0].tolist() == [1.0, 0.0] and dirs[S].tolist() == dirs[0].tolist()
    assert edge2[0] == 0.0 and edge2[R] == 6400.0 and edge2[5] == 400.0
    for bad in ((0, 60, 80.0), (65, 60, 80.0), (20, 2, 80.0), (20, 129, 80.0), (20, 60, 0.0), (20, 60, float("inf"))):
        with pytest.raises(ValueError):
            places.tables(*bad)


def test_sector_boundaries():
    """A point exactly on a boundary direction belongs to the sector that STARTS there (c_k >= 0): +x is sector 0.  The
    other axes depend on the rounding of cos / sin of the table (cos(pi/2) is 6e-17, not 0); what must hold is that each
    lands in one of the two sectors that meet there, and that the decision is the rule's, sign for sign."""
    sc = _sc()
    ring, sector, v, why = sc.bins(edge_clouds()["axes_diagonals"])
    assert (why == 0).all() and ring.tolist() == [2] * 4 + [3] * 4 and sc.no_sector == 0
    assert sector[0] == 0
    for i, k in ((1, 15), (2, 30), (3, 45)):
        assert sector[i] in (k - 1, k)
    assert sector[4:].tolist() == [7, 22, 37, 52]
    pts = edge_clouds()["axes_diagonals"].astype(np.float64)
    for p, s in zip(pts, sector):
        c = sc.dirs[:, 0] * p[1] - sc.dirs[:, 1] * p[0]
        assert c[s] >= 0 and c[s + 1] < 0
        assert not any(c[k] >= 0 and c[k + 1] < 0 for k in range(s))


def test_ring_edges():
    sc = _sc()
    ring, sector, v, why = sc.bins(edge_clouds()["ring_edges"])
    # x = 4k on the axis: k = 0 is the origin (dropped), k = 1..R-1 open ring k, k = R and R + 1 are out of range
    assert why[0] == 2 and (why[1:R] == 0).all() and (why[R:R + 2] == 2).all()
    assert ring[1:R].tolist() == list(range(1, R))
    assert ring[R + 2:].tolist() == [5, 5, 19, 1] and why[R + 2:].tolist() == [0, 0, 2, 0]      # (48, -64) is r = 80: out


def test_origin_far_low_invalid():
    sc = _sc()
    D, key, norm, cnt = sc.describe(edge_clouds()["origin"])
    assert cnt == {"n_points": 1, "dropped_invalid": 0, "dropped_range": 3, "dropped_low": 0} and D[0, 0] == 3.0
    D, key, norm, cnt = sc.describe(edge_clouds()["far"])
    assert cnt == {"n_points": 1, "dropped_invalid": 0, "dropped_range": 6, "dropped_low": 0}      # 3e38^2 is finite in double
    assert D[19, 0] == 2.0 and key.sum() == 1
    D, key, norm, cnt = sc.describe(edge_clouds()["low"])
    assert cnt == {"n_points": 2, "dropped_invalid": 0, "dropped_range": 0, "dropped_low": 3}
    assert D.max() == np.float32(-1.9999) + np.float32(2.0) and (D > 0).sum() == 2
    D, key, norm, cnt = sc.describe(edge_clouds()["non_finite"])
    assert cnt == {"n_points": 1, "dropped_invalid": 5, "dropped_range": 0, "dropped_low": 0}
    assert D[1].max() == 3.0 and norm.max() == 3.0


def test_duplicates_keep_the_maximum():
    sc = _sc()
    D, key, norm, cnt = sc.describe(edge_clouds()["duplicates"])
    assert cnt["n_points"] == 5 and (D > 0).sum() == 1 and D.max() == 3.5
    assert key.tolist() == [0, 0, 1] + [0] * 17
    assert norm[norm > 0].tolist() == [3.5]
    D0, key0, norm0, cnt0 = sc.describe(np.zeros((0, 3), np.float32))
    assert not D0.any() and not key0.any() and not norm0.any() and set(cnt0.values()) == {0}


def _tiny_db(n=6, capacity=16):
    rng = np.random.default_rng(5)
    db = places.PlaceDBRef(capacity, 4, 8, 40.0, 2.0)
    descs = []
    for i in range(n):
        D = (rng.random((4, 8)) * (rng.random((4, 8)) > 0.3)).astype(np.float32)
        key, norm = places.key_and_norm(D)
        descs.append((D, key, norm))
        db.add(D, key, norm)
    return db, descs


def test_ties_and_ordering():
    db, descs = _tiny_db()
    db.add(*descs[2])                                    # entry 6 duplicates entry 2
    out = db.query(*descs[2], exclude_recent=0, num_candidates=0, top_k=3)
    assert out[0, 0] == 2 and out[1, 0] == 6             # equal distances: the lower index first
    assert out[0, 1] == out[1, 1] and abs(out[0, 1]) < 1e-15 and out[0, 2] == 0 and out[0, 3] == 0.0
    assert out[2, 1] > out[1, 1]
    one = db.query(*descs[2], exclude_recent=0, num_candidates=1, top_k=3)      # kd = 0 twice: candidate 2 alone
    assert one[0, 0] == 2 and one[1].tolist() == list(places.UNUSED_ROW)
    # a rotated copy: the descriptor shifted by 3 columns is found at distance ~0 with shift 3 or S - 3
    D = np.roll(descs[4][0], 3, axis=1)
    key, norm = places.key_and_norm(D)
    out = db.query(D, key, norm, 0, 0, 1)
    assert out[0, 0] == 4 and abs(out[0, 1]) < 1e-15 and out[0, 2] in (3.0, 5.0)
    assert out[0, 3] == (out[0, 2] * places.TWO_PI) / 8.0


def test_exclude_candidates_full_and_zero():
    db, descs = _tiny_db(n=6, capacity=6)
    unused = [list(places.UNUSED_ROW)] * 2
    assert db.query(*descs[0], exclude_recent=6, num_candidates=10, top_k=2).tolist() == unused
    assert db.query(*descs[0], exclude_recent=100, num_candidates=0, top_k=2).tolist() == unused
    a = db.query(*descs[0], exclude_recent=2, num_candidates=200, top_k=16)      # C beyond the 4 eligible entries
    b = db.query(*descs[0], exclude_recent=2, num_candidates=0, top_k=16)
    assert a.tobytes() == b.tobytes() and (a[:4, 0] >= 0).all() and (a[:4, 0] < 4).all() and (a[4:, 0] == -1).all()
    assert (np.diff(a[:4, 1]) >= 0).all()
    db.add(*descs[1])                                    # full: not stored, counted
    assert db.stats()["n_entries"] == 6 and db.stats()["dropped_full"] == 1
    assert db.query(*descs[0], 2, 0, 16).tobytes() == b.tobytes()
    # an all-zero descriptor has no valid column: as a query nothing is returned, as an entry it is never returned
    Z = np.zeros((4, 8), np.float32)
    zk, zn = places.key_and_norm(Z)
    assert db.query(Z, zk, zn, 0, 0, 2).tolist() == unused
    db2, descs2 = _tiny_db(n=2)
    db2.add(Z, zk, zn)
    out = db2.query(*descs2[0], 0, 0, 16)
    assert sorted(out[:2, 0].tolist()) == [0, 1] and (out[2:, 0] == -1).all()
    for bad in (dict(exclude_recent=-1), dict(num_candidates=257), dict(top_k=0), dict(top_k=17), dict(num_candidates=1.5)):
        with pytest.raises(ValueError):
            db.query(*descs[0], **bad)
    db.reset()
    assert db.stats()["n_entries"] == 0 and db.stats()["dropped_full"] == 0


def test_partly_empty_columns():
    """columns that are empty on one side only are left out of the mean, on both sides of the comparison"""
    db = places.PlaceDBRef(4, 2, 4, 10.0, 2.0)
    De = np.array([[1, 0, 2, 0], [0, 0, 1, 0]], np.float32)
    db.add(De, *places.key_and_norm(De))
    Dq = np.array([[1, 0, 0, 2], [0, 0, 0, 1]], np.float32)
    out = db.query(Dq, *places.key_and_norm(Dq), exclude_recent=0, num_candidates=0, top_k=1)
    # s = 0: only column 0 is valid on both sides, cos = 1 -> d = 0; the lowest s of the minimum
    assert out[0].tolist() == [0.0, 0.0, 0.0, 0.0]


def test_revisit_on_the_synthetic_street():
    """61 places 2 m apart; 15 revisits 0.7 m / 0.8 m off with the heading reversed (pi + 0.1: shift 31 of 60).  At least 14 of
    15 top-1 results within one entry of the truth, exhaustively and through 10 ring-key candidates, and at least 14 of 15
    shifts equal to 31."""
    db = places.PlaceDBRef(64, R, S, RANGE, ZOFF)
    for d in street_db():
        db.add(*d)
    hit0 = hit10 = shift31 = 0
    true_d, false_d, no_sector = [], [], 0
    for k, scan, (D, key, norm), ns in street_queries():
        no_sector += ns
        cand = db.candidates(key, 0, 0)
        d, shift = db.distances(D, norm, cand)
        top = db.query(D, key, norm, 0, 0, 1)[0]
        top10 = db.query(D, key, norm, 0, 10, 1)[0]
        assert top[0] == np.lexsort((cand, d))[0] and top[1] == d.min()
        hit0 += abs(top[0] - k) <= 1
        hit10 += abs(top10[0] - k) <= 1
        shift31 += top[2] == 31
        true_d.append(d[k - 1:k + 2].min())
        false_d.append(d[np.abs(cand - k) > 3].min())
    print("revisit: top-1 within +-1: C=0 %d/15, C=10 %d/15; shift 31: %d/15; true-match distance %.3f .. %.3f; best entry "
          "with |i - k| > 3 no closer than %.3f; points without a sector %d"
          % (hit0, hit10, shift31, min(true_d), max(true_d), min(false_d), no_sector))
    assert hit0 >= 14 and hit10 >= 14 and shift31 >= 14
    assert no_sector == 0
