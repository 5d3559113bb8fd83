"""Loop verification, host side: the float64 restatements KeyframeStoreRef / LoopVerifierRef / EdgeListRef of
rslo_amd/loops.py on small clouds and on the synthetic street of tests/test_places_host.py.  No GPU.
tests/test_gpu_loops.py holds the kernels to these classes."""
import numpy as np
import pytest

from rslo_amd import loops, places, se3, synthetic
from rslo_amd.downsample import voxel_down_sample_ref

_STREET = {}
# (lateral / longitudinal offset, yaw, k): the revisit queries; entry index = k / 4
REVISITS = (((0.7, 0.8), np.pi + 0.1, 20), ((-1.0, -0.6), 0.3, 40), ((1.5, 1.0), np.pi - 0.2, 8), ((0.3, -1.2), -1.0, 32))


def street():
    """16 entries 8 m apart and the four revisit queries, verified ONCE per process with the defaults; never modified"""
    if not _STREET:
        db, st = places.PlaceDBRef(64), loops.KeyframeStoreRef(64)
        for k in range(0, 61, 4):
            s = synthetic.scan(720, 16, (-60.0 + 2.0 * k, 0.0), 0.0, scan_seed=k)
            db.add(*db.describe(s))
            st.prepare(s)
            st.add()
        ver = loops.LoopVerifierRef(st)
        res = []
        for off, yaw, k in REVISITS:
            s = synthetic.scan(720, 16, (-60.0 + 2.0 * k + off[0], off[1]), yaw, scan_seed=1000 + k)
            rows = db.query(*db.describe(s), exclude_recent=0, num_candidates=0, top_k=3)
            frame, info = (a.copy() for a in st.prepare(s))
            truth = np.array([off[0], off[1], 0.0, np.cos(yaw / 2), 0.0, 0.0, np.sin(yaw / 2)])
            res.append(dict(k=k, scan=s, rows=rows, frame=frame, info=info, truth=truth, out=ver.verify(rows, frame, info)[0]))
        _STREET.update(db=db, store=st, ver=ver, queries=res)
    return _STREET


def pose_error(Z, truth):
    """(metres, degrees) between two poses"""
    dq = abs(float(np.dot(Z[3:] / np.linalg.norm(Z[3:]), truth[3:])))
    return float(np.linalg.norm(Z[:3] - truth[:3])), float(np.rad2deg(2.0 * np.arccos(min(dq, 1.0))))


def cloud(n, seed, extent=(6.0, 5.0, 1.5)):
    r = np.random.default_rng(seed)
    return ((r.random((n, 3)) * 2 - 1) * np.asarray(extent)).astype(np.float32)


def cloud_of_cells(Q, voxel=0.5):
    """Q points, one per down-sample cell, on a 40-cell-wide sheet around the origin (on cell centres, so that no
    rounding moves a point into a neighbour)"""
    p = np.zeros((Q, 3), np.float32)
    p[:, 0] = ((np.arange(Q) % 40 - 20) * voxel).astype(np.float32)
    p[:, 1] = ((np.arange(Q) // 40 - 16) * voxel).astype(np.float32)
    return p


# ---------------------------------------------------------------------------------------------------------------------
# store
# ---------------------------------------------------------------------------------------------------------------------
def test_gate_counts():
    st = loops.KeyframeStoreRef(4, 64, voxel_size=0.5, min_z=-1.0, max_range=10.0)
    p = np.array([[1, 1, 0], [1, 1, -1.0], [1, 1, -0.999], [np.nan, 0, 0], [0, np.inf, 0], [10, 0, 0], [6, 8, 0.1],
                  [6, 7.9, 0], [0, 0, 11], [3, 3, 3]], np.float32)
    keep = st.gate(p)
    assert keep.tolist() == [True, False, True, False, False, False, False, True, False, True]
    frame, info = st.prepare(p)
    assert info.tolist() == [4, 4, 0, 6]
    rows = voxel_down_sample_ref(p[keep], None, 0.5)[0]
    assert frame.dtype == np.float32 and frame.shape == (64, 4)
    assert np.array_equal(frame[:4, :3], rows) and not frame[4:].any() and not frame[:, 3].any()


@pytest.mark.parametrize("K", [64, 256])
@pytest.mark.parametrize("dQ", ["below", 0, 1, "far"])
def test_selection(K, dQ):
    Q = {"below": K - 7, 0: K, 1: K + 1, "far": 5 * K + 3}[dQ]
    st = loops.KeyframeStoreRef(2, K, min_z=-5.0)
    p = cloud_of_cells(Q)
    frame, info = st.prepare(p)
    rows = voxel_down_sample_ref(p, None, 0.5)[0]
    assert len(rows) == Q and info.tolist() == [min(Q, K), Q, 0, 0]
    count = min(Q, K)
    want = [(k * Q) // K if Q > K else k for k in range(count)]
    assert want[0] == 0 and (Q <= K or want[-1] == ((K - 1) * Q) // K < Q)
    assert np.array_equal(frame[:count, :3], rows[want]) and not frame[count:].any()
    if Q > K:
        assert len(set(want)) == K      # Q > K: K distinct rows, spread over the whole cloud


def test_all_gated_empty_and_overflow():
    st = loops.KeyframeStoreRef(2, 64)
    low = cloud(100, 1)
    low[:, 2] = -2.0
    frame, info = st.prepare(low)
    assert info.tolist() == [0, 0, 0, 100] and not frame.any()
    frame, info = st.prepare(np.zeros((0, 4), np.float32))
    assert info.tolist() == [0, 0, 0, 0] and not frame.any()
    wide = loops.KeyframeStoreRef(2, 64, voxel_size=1e-6, max_range=float("inf"))
    frame, info = wide.prepare(np.array([[0, 0, 0], [3, 0, 0]], np.float32))      # 3e6 cells along x
    assert info.tolist() == [0, 0, 1, 0] and not frame.any()


def test_full_store_drops_and_counts():
    st = loops.KeyframeStoreRef(2, 64, min_z=-5.0)
    for s in range(4):
        st.prepare(cloud(300, s))
        st.add()
    rows, counts = st.entries()
    assert st.stats()["n_entries"] == 2 and st.stats()["dropped_full"] == 2 and rows.shape == (2, 64, 4)
    assert np.array_equal(rows[1], loops.KeyframeStoreRef(2, 64, min_z=-5.0).prepare(cloud(300, 1))[0]) and counts.tolist() == [64, 64]
    st.reset()
    assert st.stats()["n_entries"] == 0 and st.stats()["dropped_full"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# verification
# ---------------------------------------------------------------------------------------------------------------------
def test_street_true_matches_accepted_false_rejected():
    worst_t = worst_r = 0.0
    ov_true, ov_false = [], []
    for q in street()["queries"]:
        own = q["k"] // 4
        assert (q["rows"][:, 0] == own).sum() == 1
        for row, out in zip(q["rows"], q["out"]):
            assert out[1] == row[0] and out[13] == row[1] and out[14] == row[3] and out[5] == q["info"][0]
            if row[0] == own:
                et, er = pose_error(out[6:13], q["truth"])
                print("k=%d entry %d accepted: overlap %.3f rms %.3f, %.3f m %.4f deg" % (q["k"], own, out[3], out[4], et, er))
                assert out[0] == 0.0 and et <= 0.1 and er <= 0.2
                worst_t, worst_r = max(worst_t, et), max(worst_r, er)
                ov_true.append(out[3])
            else:
                assert out[0] == 5.0
                ov_false.append(out[3])
    print("true overlaps %.2f..%.2f, false overlaps <= %.2f, worst %.3f m %.4f deg" % (min(ov_true), max(ov_true), max(ov_false),
                                                                                     worst_t, worst_r))
    assert len(ov_true) == 4 and len(ov_false) == 8


def test_street_rank_recovery():
    q = street()["queries"][3]
    assert q["rows"][0, 0] != q["k"] // 4 and q["out"][0, 0] == 5.0      # the place search ranks a wrong entry first
    accepted = np.nonzero(q["out"][:, 0] == 0.0)[0]
    assert len(accepted) == 1 and accepted[0] != 0
    e = loops.EdgeListRef(4)
    e.emit(q["out"], 16)
    assert e.counters.tolist() == [1, 0] and e.ij[0].tolist() == [q["k"] // 4, 16]
    assert np.array_equal(e.Z[0], q["out"][accepted[0], 6:13])


def test_heading_start_is_near_the_truth():
    """the sign of the start: every revisit's heading is within half a sector (3 degrees) of the true yaw"""
    for q in street()["queries"]:
        row = q["rows"][q["rows"][:, 0] == q["k"] // 4][0]
        assert pose_error(loops.heading_pose(row[3]), np.concatenate([[0, 0, 0], q["truth"][3:]]))[1] <= 3.0 + 1e-9


def test_status_paths():
    s = street()
    st, q = s["store"], s["queries"][0]
    own = float(q["k"] // 4)
    rows = np.array([[-1, np.inf, -1, 0], [16, 0.1, 0, 0], [np.nan, 0.1, 0, 0], [own, 0.3, 0, 0.1]])
    out, info, m = loops.LoopVerifierRef(st, max_distance=0.3).verify(rows, q["frame"], q["info"])
    assert out[:, 0].tolist() == [1, 1, 1, 2] and (m == -1).all()
    for o, r in zip(out, rows):
        assert (o[1] == r[0] or np.isnan(r[0])) and o[6:13].tolist() == list(loops.IDENTITY)
        assert not o[2:6].any() and not o[13:].any()
    assert (info[:, :, 0] == out[:, :1]).all() and not info[:, :, 1:].any()
    # too few points: in the query, then in the entry
    few = q["info"].copy()
    few[0] = 49
    assert loops.LoopVerifierRef(st).verify(rows[3:], q["frame"], few)[0][0, 0] == 3
    assert loops.LoopVerifierRef(st, min_pairs=max(st.counts) + 1).verify(rows[3:], q["frame"], q["info"])[0][0, 0] == 3
    # status 4: no pair within the gate; a matrix that is not positive definite
    far = np.array([own, 0.1, 0, 0.0])
    start = np.array([[500.0, 0, 0, 1, 0, 0, 0]])
    out, info, m = loops.LoopVerifierRef(st).verify(far[None], q["frame"], q["info"], start=start)
    assert out[0, 0] == 4 and out[0, 2] == 0 and out[0, 6:13].tolist() == start[0].tolist() and (m == -1).all()
    assert (info[0, :, 0] == 4).all() and info[0, :, 5].tolist() == [0] * 5 + [1] * 5 + [2] * 10 and not out[0, 3:5].any()
    true_row = q["rows"][q["rows"][:, 0] == own]
    out, info, _ = loops.LoopVerifierRef(st, damping=-1e30).verify(true_row, q["frame"], q["info"])
    assert out[0, 0] == 4 and out[0, 2] >= 50 and info[0, 0, 1] == out[0, 2] and info[0, 0, 2] > 0
    assert np.array_equal(out[0, 6:13], loops.heading_pose(true_row[0, 3]))
    # rejected by rms alone
    out = loops.LoopVerifierRef(st, max_rms=0.01).verify(true_row, q["frame"], q["info"])[0]
    assert out[0, 0] == 5 and out[0, 3] > 0.9


def test_nearest_exact_ties_and_outlier():
    t = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [-1, 0, 0], [1e6, 0, 0]], np.float32)
    w = np.array([[0.5, 0, 0], [0.9, 0, 0], [-0.5, 0, 0], [9e5, 0, 0], [np.nan, 0, 0]])
    idx, d2 = loops.nearest_exact(w, t)
    assert idx.tolist() == [0, 1, 0, 4, -1] and d2[:3].tolist() == [0.25, (0.9 - 1.0) * (0.9 - 1.0), 0.25]
    assert loops.nearest_exact(w, t[:0])[0].tolist() == [-1] * 5


def test_emit_rules():
    e = loops.EdgeListRef(2, edge_w=(2.0, 3.0))
    assert (e.ij == -1).all() and e.Z[:, 3].tolist() == [1.0, 1.0] and not e.w.any()
    out = np.zeros((3, 16))
    out[:, 0], out[:, 1], out[:, 3], out[:, 9] = (0, 0, 5), (7, 8, 9), (0.8, 0.8, 0.99), 1.0
    e.emit(out, 11)                              # a tie: the lowest row; the rejected row's overlap does not count
    assert e.ij[0].tolist() == [7, 11] and e.w[0].tolist() == [2.0, 3.0] and e.counters.tolist() == [1, 0]
    out[:, 0] = (5, 4, 1)
    e.emit(out, 12)                              # none accepted: nothing
    assert e.counters.tolist() == [1, 0] and e.ij[1].tolist() == [-1, -1]
    out[:, 0], out[:, 3] = (0, 0, 0), (0.6, 0.7, 0.65)
    e.emit(out, 13)
    assert e.ij[1].tolist() == [8, 13] and e.counters.tolist() == [2, 0]
    e.emit(out, 14)                              # a full list drops and counts
    assert e.counters.tolist() == [2, 1] and e.ij.tolist() == [[7, 11], [8, 13]]
    e.reset()
    assert e.counters.tolist() == [0, 0] and (e.ij == -1).all()


@pytest.mark.parametrize("kw", [dict(K=100), dict(K=0), dict(K=4160), dict(capacity=0), dict(capacity=(1 << 16) + 1),
                                dict(voxel_size=0.0), dict(voxel_size=float("inf")), dict(min_z=float("nan")),
                                dict(max_range=0.0)])
def test_store_option_errors(kw):
    with pytest.raises(ValueError):
        loops.KeyframeStoreRef(**kw)


@pytest.mark.parametrize("kw", [dict(threshold=1.0), dict(stages=[]), dict(stages=[(1.0, 1)] * 9), dict(stages=[(1.0, 65)]),
                                dict(stages=[(1.0, 40), (0.5, 25)]), dict(stages=[(0.0, 1)]), dict(stages=[(float("nan"), 1)]),
                                dict(stages=[(1.0, 0)]), dict(stages=[(1.0, 1.5)]), dict(stages=5), dict(inlier_dist=0.0),
                                dict(min_overlap=1.5), dict(min_overlap=float("nan")), dict(max_rms=-1.0), dict(min_pairs=0),
                                dict(min_pairs=2.5), dict(damping=float("nan")), dict(max_distance=float("nan"))])
def test_verify_option_errors(kw):
    with pytest.raises(ValueError):
        loops.check_verify(kw)


def test_option_defaults_and_edges():
    o = loops.check_verify(None)
    assert o["stages"] == ((3.0, 5), (1.5, 5), (0.75, 10)) and o["min_pairs"] == 50 and o["inlier_dist"] == 0.5
    assert o["min_overlap"] == 0.5 and o["damping"] == 0.0 and o["max_distance"] == o["max_rms"] == float("inf")
    assert loops.check_verify(dict(stages=[(1.0, 64)]))["stages"] == ((1.0, 64),)
    for bad in (dict(max_edges=0), dict(max_edges=4097), dict(edge_w=(1.0,)), dict(edge_w=(-1.0, 1.0)),
                dict(edge_w=(1.0, float("inf")))):
        with pytest.raises(ValueError):
            loops.EdgeListRef(**bad)
    with pytest.raises(ValueError):
        loops.LoopVerifierRef(street()["store"]).verify(np.zeros((17, 4)))


def test_edge_is_a_pose_graph_loop():
    """Z is the pose of the query in the frame of the entry: between(entry pose, query pose) of the synthetic truth"""
    q = street()["queries"][1]
    k = q["k"]
    entry = np.array([-60.0 + 2.0 * k, 0, 0, 1, 0, 0, 0], np.float64)
    yaw = REVISITS[1][1]
    query = np.array([-60.0 + 2.0 * k + REVISITS[1][0][0], REVISITS[1][0][1], 0, np.cos(yaw / 2), 0, 0, np.sin(yaw / 2)])
    assert np.allclose(se3.between(entry, query), q["truth"], atol=1e-12)
