"""Place recognition on the GPU (csrc/places.hip, rslo_amd/places.py PlaceDB) against the float64 restatement
ScanContextRef / PlaceDBRef run on the same fp32 inputs and the same tables, and the candidates an OdometryRunner records
while it streams.

The bar is BIT equality, with no tolerance: a bin is decided by signs and comparisons of IEEE double products of
exactly-converted fp32 inputs (no transcendental function, no contraction), a cell is a maximum (order-free), keys and
counters are integers; a distance is a fixed-order sequence of double +, *, / and sqrt, each correctly rounded on both
sides, and ranking compares those bits, then indices.  It follows from the formats, not from what the kernels return.
"""
import numpy as np
import pytest
import torch

from test_places_host import R, S, RANGE, ZOFF, edge_clouds, street_db, street_queries
from stream_support import dev, odom_fixture, stream

pytestmark = pytest.mark.gpu

_CACHE = {}


def _cloud(seed=0):
    from rslo_amd import synthetic
    if ("cloud", seed) not in _CACHE:
        _CACHE[("cloud", seed)] = synthetic.small_cloud(4000, seed=seed)
    return _CACHE[("cloud", seed)]


def _db(capacity=8, **kw):
    from rslo_amd.places import PlaceDB
    args = dict(R=R, S=S, max_range=RANGE, z_offset=ZOFF)
    args.update(kw)
    return PlaceDB(capacity, **args)


def _assert_descriptor(db, pts_dev, pts_host, label):
    """describe on the device == ScanContextRef on the host, to the bit; returns the reference's (D, key, norm)"""
    ref = db.reference().sc
    D, key, norm = db.describe(pts_dev)
    D, key, norm = D.cpu().numpy(), key.cpu().numpy(), norm.cpu().numpy()
    rD, rkey, rnorm, rcnt = ref.describe(pts_host)
    st = db.stats()
    print("%s: %d points, %d bins filled, counters %s, no sector %d" % (label, len(pts_host), int((rD > 0).sum()), rcnt,
                                                                         ref.no_sector))
    assert {k: st[k] for k in rcnt} == rcnt
    assert D.dtype == np.float32 and D.view(np.int32).tolist() == rD.view(np.int32).tolist()
    assert key.dtype == np.int32 and key.tolist() == rkey.tolist()
    assert norm.dtype == np.float64 and norm.view(np.int64).tolist() == rnorm.view(np.int64).tolist()
    return rD, rkey, rnorm


def test_small_cloud_both_layouts():
    db = _db()
    c = _cloud()
    assert len(c) > 2048                                    # more than one workgroup
    rD, _, _ = _assert_descriptor(db, dev(c), c, "[P, 7]")
    assert (rD > 0).sum() > 100
    _assert_descriptor(db, dev(c[:, :4]), c[:, :4], "[P, 4] copy")
    _assert_descriptor(db, dev(c)[:, :3], c[:, :3], "[P, 3] view of [P, 7]")


def test_synthetic_scan():
    from rslo_amd import synthetic
    scan = synthetic.scan(720, 16, (-20.0, 0.5), 0.3, scan_seed=4)
    assert scan.shape[0] > 8000
    rD, rkey, _ = _assert_descriptor(_db(), dev(scan), scan, "16 x 720 scan")
    assert (rD > 0).sum() > 200 and rkey.max() <= S


@pytest.mark.parametrize("name", sorted(edge_clouds()))
def test_edge_clouds(name):
    c = edge_clouds()[name]
    _assert_descriptor(_db(), dev(c), c, name)


def test_all_edge_clouds_in_one_scan():
    c = np.concatenate([edge_clouds()[k] for k in sorted(edge_clouds())] + [_cloud()[:300, :3]])
    _assert_descriptor(_db(), dev(c), c, "edge clouds together")


@pytest.mark.parametrize("P", [0, 1, 63, 64, 65, 257])
def test_sizes(P):
    c = _cloud()[:P, :4]
    db = _db()
    if P:
        db.describe(dev(_cloud(1)))                        # the buffers hold another scan's descriptor first
    rD, rkey, rnorm = _assert_descriptor(db, dev(c), c, "P = %d" % P)
    if P == 0:
        assert not rD.any() and not rkey.any() and not rnorm.any()


@pytest.mark.parametrize("shape", [(1, 3), (7, 13), (20, 60), (64, 128), (3, 16), (5, 17), (2, 32), (4, 33)])
def test_shapes(shape):
    """every (R, S) corner: the descriptor, and a small query (S = 13: one short pass of the distance kernel, S = 128:
    eight passes and the largest LDS image; S = 16, 17, 32, 33: exactly one and two passes of 16 columns, and one column
    more)"""
    r, s = shape
    db = _db(capacity=5, R=r, S=s, max_range=25.0, z_offset=1.0)
    ref = db.reference()
    descs = []
    for seed in range(4):
        c = _cloud(seed)
        descs.append(_assert_descriptor(db, dev(c), c, "R = %d, S = %d, cloud %d" % (r, s, seed)))
        if seed < 3:
            db.add()
            ref.add(*descs[-1])
    for C in (0, 2):
        got = db.query(num_candidates=C, top_k=4).cpu().numpy()
        want = ref.query(*descs[3], exclude_recent=0, num_candidates=C, top_k=4)
        print("C = %d:\n%s" % (C, want))
        assert got.view(np.int64).tolist() == want.view(np.int64).tolist()


# ---------------------------------------------------------------------------------------------------------------------
# query: the 61 places of the street, an all-zero entry and a duplicated entry
# ---------------------------------------------------------------------------------------------------------------------
def _street():
    """(device database, reference, queries): 63 entries -- street 0..29, zeros, street 30..60, street 12 again"""
    if "street" not in _CACHE:
        db = _db(capacity=64)
        ref = db.reference()
        zero = (np.zeros((R, S), np.float32), np.zeros(R, np.int32), np.zeros(S, np.float64))
        entries = street_db()[:30] + [zero] + street_db()[30:] + [street_db()[12]]
        for D, key, norm in entries:
            ref.add(D, key, norm)
            db.add(dev(D), dev(key), dev(norm))
        queries = [q[2] for q in street_queries()[::5]] + [street_db()[12], zero]      # 3 revisits, a stored scan, zeros
        _CACHE["street"] = (db, ref, queries)
    return _CACHE["street"]


def test_database_holds_what_was_added():
    db, ref, _ = _street()
    D, norm, key = db.entries()
    assert db.stats()["n_entries"] == 63 and db.stats()["dropped_full"] == 0
    assert D.tobytes() == np.stack(ref.D).tobytes() and norm.tobytes() == np.stack(ref.norm).tobytes()
    assert key.tobytes() == np.stack(ref.key).tobytes()


def _ref_query(qi, exclude, C, top_k):
    db, ref, queries = _street()
    k = ("rq", qi, exclude, C, top_k)
    if k not in _CACHE:
        _CACHE[k] = ref.query(*queries[qi], exclude_recent=exclude, num_candidates=C, top_k=top_k)
    return _CACHE[k]


@pytest.mark.parametrize("exclude", [0, 3, 100])
@pytest.mark.parametrize("top_k", [1, 5, 16])
@pytest.mark.parametrize("C", [0, 1, 10, 256])
def test_query(C, top_k, exclude):
    db, ref, queries = _street()
    for qi, (D, key, norm) in enumerate(queries):
        got = db.query(dev(D), dev(key), dev(norm), exclude_recent=exclude, num_candidates=C, top_k=top_k).cpu().numpy()
        want = _ref_query(qi, exclude, C, top_k)
        if top_k == 5:
            print("query %d, C = %d, exclude %d: entries %s distances %s shifts %s" % (
                qi, C, exclude, want[:, 0].astype(int).tolist(), np.round(want[:, 1], 4).tolist(),
                want[:, 2].astype(int).tolist()))
        assert got.shape == (top_k, 4) and got.dtype == np.float64
        assert got.view(np.int64).tolist() == want.view(np.int64).tolist(), (qi, got, want)
        if exclude == 100 or qi == 4:
            assert (want[:, 0] == -1).all()
    if exclude == 0 and top_k >= 5 and C in (0, 256):      # the stored scan finds itself and its copy at the same distance
        want = _ref_query(3, 0, C, top_k)
        assert want[0, 0] == 12 and want[1, 0] == 62 and want[0, 1] == want[1, 1] and 30 not in want[:, 0]


def test_overflowing_database():
    db = _db(capacity=4)
    ref = db.reference()
    for D, key, norm in street_db()[:12:2]:
        ref.add(D, key, norm)
        db.add(dev(D), dev(key), dev(norm))
    st = db.stats()
    assert st["n_entries"] == 4 and st["dropped_full"] == 2 and ref.stats()["dropped_full"] == 2
    assert db.entries()[0].tobytes() == np.stack(ref.D).tobytes()
    D, key, norm = street_queries()[0][2]
    for C in (0, 2, 256):
        got = db.query(dev(D), dev(key), dev(norm), exclude_recent=1, num_candidates=C, top_k=5).cpu().numpy()
        want = ref.query(D, key, norm, exclude_recent=1, num_candidates=C, top_k=5)
        assert got.view(np.int64).tolist() == want.view(np.int64).tolist()
        n = min(C, 3) if C else 3                          # three eligible entries
        assert (want[:n, 0] >= 0).all() and (want[n:, 0] == -1).all()
    db.reset()
    assert db.stats()["n_entries"] == 0 and db.stats()["dropped_full"] == 0
    assert (db.query(dev(D), dev(key), dev(norm), top_k=2).cpu().numpy()[:, 0] == -1).all()


def test_argument_errors_write_nothing():
    from rslo_amd import capi, places
    lib = capi.lib()
    nbytes = capi.place_bytes(8, R, S)
    assert nbytes == 256 + 8 * R * S * 4 + 8 * S * 8 + (8 * R * 4 + 255) // 256 * 256
    assert capi.place_bytes(0, R, S) == 0 and capi.place_bytes(8, 65, S) == 0 and capi.place_bytes(8, R, 2) == 0
    assert capi.place_bytes(8, 0, S) == 0 and capi.place_bytes(8, R, 129) == 0 and capi.place_bytes((1 << 24) + 1, R, S) == 0
    sentinel = 0x5A5A5A5A5A5A5A5A
    buf = torch.full((nbytes // 8,), sentinel, dtype=torch.int64, device="cuda")
    outs = torch.full((1024,), sentinel, dtype=torch.int64, device="cuda")
    p, o = buf.data_ptr(), outs.data_ptr()
    pts = dev(_cloud()[:64, :4])
    tab = dev(places.tables(R, S, RANGE))
    ws = capi.place_query_ws(8, "cuda")
    wsb = ws.numel() * 8
    D, key, norm = o, o + 5120, o + 5632
    rcs = [lib.rslo_place_reset(p, nbytes, 0, R, S, None), lib.rslo_place_reset(p, nbytes, 8, 0, S, None),
           lib.rslo_place_reset(p, nbytes, 8, R, 2, None), lib.rslo_place_reset(p, nbytes - 8, 8, R, S, None),
           lib.rslo_place_reset(p, nbytes, 9, R, S, None), lib.rslo_place_reset(None, nbytes, 8, R, S, None),
           lib.rslo_place_describe(pts.data_ptr(), 2, 64, R, S, tab.data_ptr(), 2.0, D, key, norm, o + 7168, None),
           lib.rslo_place_describe(pts.data_ptr(), 4, -1, R, S, tab.data_ptr(), 2.0, D, key, norm, o + 7168, None),
           lib.rslo_place_describe(pts.data_ptr(), 4, 64, 65, S, tab.data_ptr(), 2.0, D, key, norm, o + 7168, None),
           lib.rslo_place_describe(pts.data_ptr(), 4, 64, R, S, None, 2.0, D, key, norm, o + 7168, None),
           lib.rslo_place_describe(pts.data_ptr(), 4, 64, R, S, tab.data_ptr(), float("nan"), D, key, norm, o + 7168, None),
           lib.rslo_place_describe(None, 4, 64, R, S, tab.data_ptr(), 2.0, D, key, norm, o + 7168, None),
           lib.rslo_place_add(p, nbytes - 8, 8, R, S, D, key, norm, None),
           lib.rslo_place_add(p, nbytes, 8, R, S, None, key, norm, None),
           lib.rslo_place_query(p, nbytes, 8, R, S, D, key, norm, -1, 10, 1, o, ws.data_ptr(), wsb, None),
           lib.rslo_place_query(p, nbytes, 8, R, S, D, key, norm, 0, 257, 1, o, ws.data_ptr(), wsb, None),
           lib.rslo_place_query(p, nbytes, 8, R, S, D, key, norm, 0, -1, 1, o, ws.data_ptr(), wsb, None),
           lib.rslo_place_query(p, nbytes, 8, R, S, D, key, norm, 0, 10, 0, o, ws.data_ptr(), wsb, None),
           lib.rslo_place_query(p, nbytes, 8, R, S, D, key, norm, 0, 10, 17, o, ws.data_ptr(), wsb, None),
           lib.rslo_place_query(p, nbytes, 8, R, S, D, key, norm, 0, 10, 1, o, ws.data_ptr(), 64, None),
           lib.rslo_place_query(p, nbytes, 8, R, S, D, key, norm, 0, 10, 1, o, None, wsb, None)]
    print("return codes:", rcs, lib.rslo_last_error().decode())
    assert all(rc != 0 for rc in rcs)
    # a buffer that was never reset holds no database: the kernels of valid calls leave it, and the result rows, alone
    assert lib.rslo_place_add(p, nbytes, 8, R, S, D, key, norm, None) == 0
    assert lib.rslo_place_query(p, nbytes, 8, R, S, D, key, norm, 0, 10, 1, o, ws.data_ptr(), wsb, None) == 0
    assert lib.rslo_place_query(p, nbytes, 8, R, S, D, key, norm, 0, 0, 1, o, ws.data_ptr(), wsb, None) == 0
    torch.cuda.synchronize()
    assert bool((buf == sentinel).all()) and bool((outs == sentinel).all())
    # ... and so does a database that was reset with another shape
    assert lib.rslo_place_reset(p, nbytes, 8, R, S, None) == 0
    assert lib.rslo_place_add(p, nbytes, 4, R, S, D, key, norm, None) == 0
    torch.cuda.synchronize()
    assert buf[4:6].tolist() == [0, 0] and bool((buf[32:] == sentinel).all())
    for bad in (dict(capacity=0), dict(R=0), dict(S=200), dict(max_range=-1.0), dict(z_offset=float("nan"))):
        with pytest.raises((capi.RsloHipError, ValueError)):
            _db(**bad)
    with pytest.raises(capi.RsloHipError):
        _db().describe(dev(_cloud()).cpu())
    with pytest.raises(capi.RsloHipError):
        _db().query(top_k=17)


def _three_scans(db, clouds, loop):
    """describe -> query -> add per scan, eagerly; (results [n, top_k, 4], entries, stats)"""
    out = torch.zeros((len(clouds), loop["top_k"], 4), dtype=torch.float64, device="cuda")
    for i, c in enumerate(clouds):
        db.describe(c)
        db.query(out=out[i], **loop)
        db.add()
    return out.cpu().numpy(), db.entries(), db.stats()


def test_capture_and_replay():
    """describe + query + add captured once on one stream over a static scan buffer; replayed per scan it equals the eager
    bits, which equal the restatement; two eager runs agree."""
    loop = dict(exclude_recent=1, num_candidates=2, top_k=3)
    hosts = [_cloud(seed)[:, :4] for seed in (0, 1, 2, 0)]
    clouds = [dev(h) for h in hosts]
    res_a, ent_a, st_a = _three_scans(_db(), clouds, loop)
    res_b, ent_b, st_b = _three_scans(_db(), clouds, loop)
    assert res_a.tobytes() == res_b.tobytes() and st_a == st_b and all(a.tobytes() == b.tobytes() for a, b in zip(ent_a, ent_b))
    ref = _db().reference()
    want = []
    for h in hosts:
        d = ref.describe(h)
        want.append(ref.query(*d, **loop))
        ref.add(*d)
    want = np.stack(want)
    print("eager rows:\n%s" % res_a[:, 0])
    assert res_a.view(np.int64).tolist() == want.view(np.int64).tolist()
    assert want[3, 0, 0] == 0 and want[0, 0, 0] == -1          # the fourth scan is the first again; the first finds nothing
    db = _db()
    static = torch.zeros_like(clouds[0])
    row = torch.zeros((loop["top_k"], 4), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        db.describe(static)
        db.query(out=row, **loop)
        db.add()
    assert db.stats()["n_entries"] == 0                       # captured, not run
    res = []
    for c in clouds:
        static.copy_(c)
        g.replay()
        res.append(row.clone())
    res = torch.stack(res).cpu().numpy()
    assert res.tobytes() == res_a.tobytes()
    assert db.stats() == st_a and all(a.tobytes() == b.tobytes() for a, b in zip(db.entries(), ent_a))


# ---------------------------------------------------------------------------------------------------------------------
# the runner's database
# ---------------------------------------------------------------------------------------------------------------------
N_SCANS = 3
LOOP = dict(exclude_recent=1, num_candidates=2, top_k=2)


odom = odom_fixture(21, 3, N_SCANS)


def test_runner_records_loop_candidates(odom):
    from rslo_amd import capi, inference
    net, scans = odom
    for bad in (dict(loop=dict(top_k=1)), dict(places=_db(), loop=dict(threshold=0.3)),
                dict(places=_db(), loop=dict(top_k=17)), dict(places=_db(), loop=dict(exclude_recent=-1))):
        with pytest.raises(capi.RsloHipError):                  # refused before anything is built
            inference.OdometryRunner(net, **bad)
    plain = inference.OdometryRunner(net)
    try:
        rel0, traj0 = stream(plain, scans)
        keys0 = set(plain.stats)
        with pytest.raises(capi.RsloHipError):
            plain.loop_candidates()
    finally:
        plain.close()
    db = _db(capacity=16)
    runner = inference.OdometryRunner(net, places=db, loop=LOOP)
    try:
        rel, traj = stream(runner, scans)
        assert set(runner.stats) == keys0
        assert rel.tobytes() == rel0.tobytes() and traj.tobytes() == traj0.tobytes()      # the database disturbs nothing
        got = runner.loop_candidates().cpu().numpy()
        ref = db.reference()
        want = []
        for s in scans:
            d = ref.describe(s.cpu().numpy())
            want.append(ref.query(*d, **LOOP))
            ref.add(*d)
        want = np.stack(want)
        print("runner candidates:\n%s" % want)
        assert got.shape == (N_SCANS, LOOP["top_k"], 4) and got.view(np.int64).tolist() == want.view(np.int64).tolist()
        assert (want[:2, :, 0] == -1).all() and want[2, 0, 0] == 0 and want[2, 1, 0] == -1      # exclude_recent = 1
        assert db.stats()["n_entries"] == N_SCANS and db.stats()["n_points"] == ref.stats()["n_points"] > 50000
        assert db.entries()[0].tobytes() == np.stack(ref.D).tobytes()
        runner.reset()                                      # a new sequence has a new database
        assert db.stats()["n_entries"] == 0 and len(runner.loop_candidates()) == 0
        stream(runner, scans[:1])
        assert db.stats()["n_entries"] == 1 and (runner.loop_candidates().cpu().numpy()[0, :, 0] == -1).all()
    finally:
        runner.close()
