"""The place-search kernels (csrc/places.hip) past one stride of every loop they are written around, against the float64
restatement PlaceDBRef / ScanContextRef, bit for bit as in tests/test_gpu_places.py (the reasons are given there):

  * a database of 2100 entries (tests/test_places_host.py large_db, whose properties are asserted there on the
    restatement alone) in a capacity of 2112: k_place_keys runs 9 workgroups, k_place_select's 1024 threads and
    k_place_topk's 256 threads loop up to 3 and 9 times, equal and negative distances meet on one thread and on
    threads several strides apart, and the candidate cut falls inside a run of equal ring-key distances;
  * the eligible count swept over every stride boundary with exclude_recent;
  * clouds beyond the capped grid of k_place_describe (256 workgroups x 2048 points);
  * ring keys no honest descriptor has, where the stage-1 sum must saturate and not wrap.
"""
import numpy as np
import pytest
import torch

from test_places_host import LARGE_N, LARGE_SHAPES, large_db, large_queries, large_ref, saturation_db, saturation_order
from test_gpu_places import _assert_descriptor
from stream_support import dev

pytestmark = pytest.mark.gpu

CAPACITY = 2112                     # neither a power of two nor a multiple of 256
MAX_RANGE, Z_OFFSET = 40.0, 2.0
E_ALL = (1, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 2100)
E_OF = {(7, 13): E_ALL, (20, 60): (257, 1025, 2100)}      # the restatement of (20, 60) takes 0.5 s per 1000 entries
_CACHE = {}


def _large(shape):
    """(device database, restatement, device queries, host queries) of large_db(*shape); filled once, then only queried"""
    if shape not in _CACHE:
        from rslo_amd.places import PlaceDB
        L = large_db(*shape)
        db = PlaceDB(CAPACITY, *shape, max_range=MAX_RANGE, z_offset=Z_OFFSET)
        stacked = dev(L["D"]), dev(L["key"]), dev(L["norm"])      # one upload; add() reads row views
        for i in range(LARGE_N):
            db.add(stacked[0][i], stacked[1][i], stacked[2][i])
        torch.cuda.synchronize()
        host = large_queries(*shape)
        _CACHE[shape] = (db, large_ref(*shape, MAX_RANGE, Z_OFFSET), [tuple(dev(a) for a in q) for q in host], host)
    return _CACHE[shape]


def _want(shape, qi, E, C, top_k):
    k = (shape, qi, E, C, top_k)
    if k not in _CACHE:
        _, ref, _, host = _large(shape)
        _CACHE[k] = ref.query(*host[qi], exclude_recent=LARGE_N - E, num_candidates=C, top_k=top_k)
    return _CACHE[k]


@pytest.mark.parametrize("shape", LARGE_SHAPES)
def test_large_database_holds_what_was_added(shape):
    db, ref, _, _ = _large(shape)
    st = db.stats()
    assert st["n_entries"] == LARGE_N and st["dropped_full"] == 0
    D, norm, key = db.entries()
    assert D.tobytes() == np.stack(ref.D).tobytes() and norm.tobytes() == np.stack(ref.norm).tobytes()
    assert key.tobytes() == np.stack(ref.key).tobytes()


def _check_queries(shape, E, C, top_k):
    db, _, queries, _ = _large(shape)
    for qi, q in enumerate(queries):
        got = db.query(*q, exclude_recent=LARGE_N - E, num_candidates=C, top_k=top_k).cpu().numpy()
        want = _want(shape, qi, E, C, top_k)
        assert got.shape == (top_k, 4) and got.dtype == np.float64
        assert got.view(np.int64).tolist() == want.view(np.int64).tolist(), (shape, E, C, qi, got, want)
        if qi == 3:
            assert (want[:, 0] == -1).all()                     # the all-zero query finds nothing
    return _want(shape, 0, E, C, top_k)


@pytest.mark.parametrize("C", [0, 1, 255, 256])
@pytest.mark.parametrize("shape,E", [(s, e) for s in LARGE_SHAPES for e in E_OF[s]])
def test_eligible_count_sweep(shape, E, C):
    want = _check_queries(shape, E, C, 16)
    print("R, S = %s, E = %d, C = %d, query Q: entries %s distances %s" % (
        shape, E, C, want[:, 0].astype(int).tolist(), want[:, 1].tolist()))
    if E == LARGE_N and C != 1:                                 # what large_db is for reaches the device's result
        assert want[0, 1] < want[1, 1] == want[2, 1] < 0 and want[1, 0] < want[2, 0]
        assert len(set(want[3:14, 1].view(np.int64).tolist())) == 1 and want[3, 0] == 0 and want[13, 0] == 2099


@pytest.mark.parametrize("top_k", [1, 5])
@pytest.mark.parametrize("C", [0, 256])
@pytest.mark.parametrize("shape", LARGE_SHAPES)
def test_fewer_rows_than_equal_distances(shape, C, top_k):
    _check_queries(shape, 1025, C, top_k)


def test_capture_and_replay_at_size():
    """one query captured on the 2100-entry database over static query buffers; each replay equals the eager bits"""
    shape = LARGE_SHAPES[0]
    db, ref, queries, host = _large(shape)
    args = dict(exclude_recent=76, num_candidates=256, top_k=16)
    eager = [db.query(*queries[qi], **args).cpu().numpy() for qi in (0, 2)]
    for qi, e in zip((0, 2), eager):
        assert e.view(np.int64).tolist() == ref.query(*host[qi], **args).view(np.int64).tolist()
    static = tuple(torch.zeros_like(a) for a in queries[0])
    row = torch.zeros((16, 4), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        db.query(*static, out=row, **args)
    for qi, e in zip((0, 2), eager):
        for s, a in zip(static, queries[qi]):
            s.copy_(a)
        row.zero_()
        g.replay()
        assert row.cpu().numpy().tobytes() == e.tobytes()
    assert db.stats()["n_entries"] == LARGE_N


# ---------------------------------------------------------------------------------------------------------------------
# describe beyond the capped grid: 256 workgroups x 2048 points = 524 288
# ---------------------------------------------------------------------------------------------------------------------
N_MAX = 526337


def _big_cloud():
    if "cloud" not in _CACHE:
        rng = np.random.default_rng(11)
        c = (rng.standard_normal((N_MAX, 3)) * (12.0, 12.0, 1.5)).astype(np.float32)
        c[[7, 100000, 524286, 526000], [0, 1, 2, 0]] = np.nan
        c[[11, 300000, 524287, 525000], 0] = (1000.0, -1000.0, np.inf, 41.0)
        c[[524285, 526335]] = (3.0, -4.0, -10.0)                # low
        c[524288] = (3.0, 4.0, 30.0)                            # the first point of the second trip, and the last point:
        c[N_MAX - 1] = (-5.0, 2.0, 31.0)                        # each the maximum of its bin
        _CACHE["cloud"] = (c, dev(c))
    return _CACHE["cloud"]


@pytest.mark.parametrize("N", [524288, 524289, N_MAX])
@pytest.mark.parametrize("shape", LARGE_SHAPES)
def test_describe_beyond_the_grid_cap(shape, N):
    from rslo_amd.places import PlaceDB
    host, device = _big_cloud()
    db = PlaceDB(1, *shape, max_range=MAX_RANGE, z_offset=Z_OFFSET)
    rD, _, _ = _assert_descriptor(db, device[:N], host[:N], "R, S = %s, N = %d" % (shape, N))
    st = db.stats()
    assert min(st[k] for k in ("n_points", "dropped_invalid", "dropped_range", "dropped_low")) > 0
    assert (rD == np.float32(32.0)).any() == (N > 524288) and (rD == np.float32(33.0)).any() == (N == N_MAX)


# ---------------------------------------------------------------------------------------------------------------------
# ring keys where the stage-1 sum of squares must saturate
# ---------------------------------------------------------------------------------------------------------------------
def test_stage1_saturates():
    """kd = min(sum, 2^32 - 1) on the device: bit equality with the restatement for every C, and the candidate set
    against Python integers.  A sum that wraps makes entry 0 (four terms of (2^31)^2) the best candidate of query 0."""
    from rslo_amd.places import PlaceDB, key_and_norm
    entries, queries = saturation_db()
    n = len(entries)
    rng = np.random.default_rng(5)
    db = PlaceDB(16, 4, 8, max_range=MAX_RANGE, z_offset=Z_OFFSET)
    ref = db.reference()
    descs = []
    for e in entries:
        D = (rng.random((4, 8)) * (rng.random((4, 8)) > 0.3)).astype(np.float32)
        descs.append((D, np.array(e, np.int32), key_and_norm(D)[1]))
        ref.add(*descs[-1])
        db.add(*(dev(a) for a in descs[-1]))
    assert db.entries()[2].tobytes() == np.array(entries, np.int32).tobytes()
    D, _, norm = descs[2]
    assert np.isfinite(ref.distances(D, norm, np.arange(n))[0]).all()      # every candidate is returned
    for qi, q in enumerate(queries):
        key = np.array(q, np.int32)
        for exclude in (0, 3):
            order, kd = saturation_order(entries, q, n - exclude)
            for C in range(0, n + 1):
                got = db.query(dev(D), dev(key), dev(norm), exclude_recent=exclude, num_candidates=C, top_k=16).cpu().numpy()
                want = ref.query(D, key, norm, exclude_recent=exclude, num_candidates=C, top_k=16)
                assert got.view(np.int64).tolist() == want.view(np.int64).tolist(), (q, exclude, C, got, want)
                chosen = sorted(int(i) for i in got[:, 0] if i >= 0)
                assert chosen == sorted(order[:C] if C else order), (q, exclude, C, kd)
                if qi == 0 and C == 1:
                    assert got[0, 0] == 2 and got[0, 1] == want[0, 1] and abs(got[0, 1]) < 1e-15
