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

# ---------------------------------------------------------------------------------------------------------------------
# a database larger than any stride of the query kernels (k_place_keys: 256 per workgroup, k_place_select: 1024 threads,
# k_place_topk: 256 threads), shared with tests/test_gpu_places_large.py
# ---------------------------------------------------------------------------------------------------------------------
LARGE_N = 2100
LARGE_SHAPES = ((7, 13), (20, 60))
LARGE_COPIES = (0, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 2099)      # column-rolled copies of Q
LARGE_SCALED = ((300, 0.5), (700, 0.25), (1836, 0.5))      # copies of Q with the stored norm scaled: distances -1, -3, -1
LARGE_NEGATED = 1500                                       # -Q with the true norm: d(0) = 2, distance in (1, 2]
LARGE_KEEP = (0.2, 0.5, 0.8)                               # P(bin filled) of a filler; one level per entry
LARGE_SEED = {(7, 13): 2, (20, 60): 9}                     # chosen for test_large_db_has_the_cases_it_is_for


def large_db(R, S):
    """{D [n, R, S] f32, key [n, R] i32, norm [n, S] f64, Q: (D, key, norm), roll: {index: columns rolled}} of LARGE_N
    entries, made once per process and never modified.  Q's level is the first of LARGE_KEEP, so a third of the fillers
    have ring keys near Q's and the candidate cut falls among them."""
    if (R, S) not in _LARGE:
        rng = np.random.default_rng(LARGE_SEED[(R, S)])
        level = rng.integers(0, 3, LARGE_N)
        keep = rng.random((LARGE_N, R, S)) < np.array(LARGE_KEEP)[level][:, None, None]
        D = ((0.25 + 3.0 * rng.random((LARGE_N, R, S))) * keep).astype(np.float32)
        Q = ((0.25 + 3.0 * rng.random((R, S))) * (rng.random((R, S)) < LARGE_KEEP[0])).astype(np.float32)
        roll = {}
        for n, i in enumerate(LARGE_COPIES):                 # shifts 1, 4, 7, ...; the last repeats the second
            roll[i] = (3 * n + 1) % S if n < len(LARGE_COPIES) - 1 else 4
        for n, (i, _) in enumerate(LARGE_SCALED):
            roll[i] = (5, 0, 2)[n]
        for i, k in roll.items():
            D[i] = np.roll(Q, k, axis=1)
        D[LARGE_NEGATED] = -Q
        kn = [places.key_and_norm(d) for d in D]
        key, norm = np.stack([k for k, _ in kn]), np.stack([n for _, n in kn])
        for i, f in LARGE_SCALED:
            norm[i] = norm[i] * f                            # the API takes the norm from the caller
        key[LARGE_NEGATED] = places.key_and_norm(Q)[0]       # ... and the key: -Q counts as Q in stage 1
        _LARGE[(R, S)] = dict(D=D, key=key, norm=norm, Q=(Q,) + places.key_and_norm(Q), roll=roll)
    return _LARGE[(R, S)]


def large_ref(R, S, max_range=40.0, z_offset=2.0, tables_=None):
    """a PlaceDBRef (capacity 2112) holding large_db(R, S); made once per process, only queried"""
    if ("ref", R, S) not in _LARGE:
        L = large_db(R, S)
        ref = places.PlaceDBRef(2112, R, S, max_range, z_offset, tables_)
        for i in range(LARGE_N):
            ref.add(L["D"][i], L["key"][i], L["norm"][i])
        _LARGE[("ref", R, S)] = ref
    return _LARGE[("ref", R, S)]


def large_queries(R, S):
    """Q, a roll of Q, a filler entry (it finds itself) and an all-zero descriptor, as (D, key, norm)"""
    L = large_db(R, S)
    Qr = np.roll(L["Q"][0], 2, axis=1)
    Z = np.zeros((R, S), np.float32)
    return [L["Q"], (Qr,) + places.key_and_norm(Qr), (L["D"][1234], L["key"][1234], L["norm"][1234]),
            (Z,) + places.key_and_norm(Z)]


_LARGE = {}


def saturation_db():
    """(entry keys, query keys) for R = 4: ring keys no honest descriptor has, where a 64-bit sum of squares wraps (four
    terms of (2^31)^2 are 2^64), where one term is just below / exactly at 2^16 (65535^2 < 2^32 - 1 <= 65536^2), where the
    sum alone passes the bound, and INT32_MIN against INT32_MAX"""
    lo, hi, b = -2 ** 31, 2 ** 31 - 1, 2 ** 30
    entries = [[-b] * 4, [b + 1] * 4, [b] * 4, [65535, 0, 0, 0], [65536, 0, 0, 0], [65535, 363, 0, 0], [65535, 362, 0, 0],
               [lo] * 4, [hi] * 4, [0] * 4, [-65536, 0, 0, 0], [0, 0, 0, -65535], [0, 1, 0, 65535], [hi, lo, hi, lo]]
    queries = [[b] * 4, [0] * 4, [hi] * 4, [lo] * 4, [-1, 0, 0, 0]]
    return entries, queries


def saturation_order(entries, q, n=None):
    """the stage-1 order of the first n entries by the header's rule, in Python integers"""
    kd = [min(sum((int(a) - int(b)) ** 2 for a, b in zip(q, e)), 2 ** 32 - 1) for e in entries[:n]]
    return sorted(range(len(kd)), key=lambda i: (kd[i], i)), kd


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


def test_stage1_distance_is_total():
    """kd = min(sum of squares, 2^32 - 1) for any int32 keys, against Python integers: the full candidate order for every
    C, with and without excluded entries"""
    entries, queries = saturation_db()
    n = len(entries)
    db = places.PlaceDBRef(16, 4, 8, 40.0, 2.0)
    for e in entries:
        db.add(np.zeros((4, 8), np.float32), np.array(e, np.int32), np.zeros(8))
    top = 2 ** 32 - 1
    for q in queries:
        for exclude in (0, 3):
            order, kd = saturation_order(entries, q, n - exclude)
            print("query key %s, exclude %d: kd %s order %s" % (q, exclude, kd, order))
            assert db.candidates(np.array(q, np.int32), exclude, 0).tolist() == list(range(n - exclude))
            for C in range(1, n + 1):
                assert db.candidates(np.array(q, np.int32), exclude, C).tolist() == order[:C], (q, exclude, C)
    # what the cases are there for, in the integers of the rule
    order, kd = saturation_order(entries, queries[0])
    assert kd[:3] == [top, 4, 0] and order[:3] == [2, 1, 0]              # 4 * (2^31)^2 = 2^64 must not read as 0
    assert order[3:] == list(range(3, n)) and set(kd[3:]) == {top}       # saturated entries tie: index order
    order, kd = saturation_order(entries, queries[1])
    assert kd[3] == 65535 ** 2 < top and kd[4] == top and 65536 ** 2 > top and kd[10] == top
    assert kd[6] == 65535 ** 2 + 362 ** 2 < top and kd[5] == top and 65535 ** 2 + 363 ** 2 > top      # the sum passes it
    assert order[:5] == [9, 3, 11, 12, 6]
    for qi in (2, 3):
        order, kd = saturation_order(entries, queries[qi])
        assert kd[10 - qi] == 0 and kd[5 + qi] == top and sum(int(a) - int(b) for a, b in zip(
            queries[qi], entries[5 + qi])) in (4 * (2 ** 32 - 1), -4 * (2 ** 32 - 1))      # INT32_MIN against INT32_MAX


@pytest.mark.parametrize("shape", LARGE_SHAPES)
def test_large_db_has_the_cases_it_is_for(shape):
    """Properties of large_db on the restatement alone; the GPU test means nothing without them: negative distances
    (with a tie), a run of bit-equal distances on entries of every stride, a candidate cut inside a run of equal kd."""
    L, ref = large_db(*shape), large_ref(*shape)
    D, key, norm = L["Q"]
    assert ref.stats()["n_entries"] == LARGE_N and L["key"].dtype == np.int32 and L["norm"].dtype == np.float64
    top = ref.query(D, key, norm, exclude_recent=0, num_candidates=0, top_k=16)
    idx, d, shift = top[:, 0].astype(int).tolist(), top[:, 1], top[:, 2].astype(int).tolist()
    print("top 16 of Q: entries %s\ndistances %s\nshifts %s" % (idx, d.tolist(), shift))
    assert idx[:3] == [700, 300, 1836] and d[0] < d[1] < 0 and d[1:3].view(np.int64).tolist() == [d[1].view(np.int64)] * 2
    assert abs(d[0] + 3) < 1e-14 and abs(d[1] + 1) < 1e-14
    nc = len(LARGE_COPIES)
    assert idx[3:3 + nc] == list(LARGE_COPIES) and len(set(d[3:3 + nc].view(np.int64).tolist())) == 1 and nc >= 8
    assert abs(d[3]) < 1e-15 and d[3 + nc] > d[3] and (np.diff(d) >= 0).all()
    assert {i // 1024 for i in LARGE_COPIES} == {0, 1, 2} and len({i // 256 for i in LARGE_COPIES}) >= 5
    for stride in (256, 1024):                                 # equal distances on one thread of a kernel and on several
        assert 1 < len({i % stride for i in LARGE_COPIES}) < nc
    assert shift[:3 + nc] == [L["roll"][i] for i in idx[:3 + nc]]
    rolls = [L["roll"][i] for i in LARGE_COPIES]
    assert len(set(rolls)) == nc - 1                           # two copies share a shift
    dn, _ = ref.distances(D, norm, [LARGE_NEGATED])
    assert 1.0 < dn[0] <= 2.0 + 1e-14      # every cosine is negative: 2 at shift 0, the smallest d(s) still above any honest one
    order, kd = saturation_order(L["key"].tolist(), key.tolist())
    s = [kd[i] for i in order]
    for C in (255, 256):
        cand = ref.candidates(key, 0, C).tolist()
        print("C = %d: kd at the cut %s, shared by %d entries" % (C, s[C - 2:C + 2], s.count(s[C])))
        assert cand == order[:C]
        assert s[C - 2] == s[C - 1] == s[C] == s[C + 1]        # >= 2 entries of the cut's kd on each side of it
        for lo, hi in ((0, 256), (256, 1024), (1024, 2048), (2048, LARGE_N)):
            assert any(lo <= c < hi for c in cand)
    for D, key, norm in large_queries(*shape)[1:3]:            # the other queries see ties in kd as well
        kd = saturation_order(L["key"].tolist(), key.tolist())[1]
        assert len(set(kd)) < LARGE_N - 100
    self_top = ref.query(*large_queries(*shape)[2], exclude_recent=0, num_candidates=10, top_k=1)
    assert self_top[0, 0] == 1234 and abs(self_top[0, 1]) < 1e-15
