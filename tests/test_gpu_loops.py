"""Loop verification on the GPU (csrc/loopverify.hip) against the float64 restatements of rslo_amd/loops.py: the keyframe
store bit for bit, the nearest-neighbour matching exactly, one Gauss-Newton iteration within the rounding bounds of
tests/test_gpu_mapreg.py, the whole call against its own single iterations, capture, and the runner."""
import contextlib
import gc

import numpy as np
import pytest
import torch

from test_loops_host import REVISITS, cloud, cloud_of_cells, pose_error, street
from stream_support import cond_of, dev, odom_fixture, same_bits, stream

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A5A5A5A5A
IDENT = (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)


@contextlib.contextmanager
def quiet_collector():
    """Around code that captures a graph: dead cycles left by earlier tests (runners, their captured graphs, device memory)
    are collected HERE, and the collector stays off inside, so that no collection destroys them in the middle of a capture
    (torch.cuda.graph does not collect on entry)."""
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


def _store(**kw):
    from rslo_amd import loops
    kw.setdefault("capacity", 16)
    kw.setdefault("K", 64)
    return loops.KeyframeStore(**kw)


def _same_store(store, ref):
    rows, counts = store.entries()
    want_rows, want_counts = ref.entries()
    assert rows.tobytes() == want_rows.tobytes() and counts.tolist() == want_counts.tolist()
    assert store.stats() == ref.stats()


def _prepared(store, ref, host, view=None):
    """prepare on both sides; the device reads `view` (a tensor over the same points) when given"""
    frame, info = store.prepare(dev(host) if view is None else view)
    want_frame, want_info = ref.prepare(host)
    assert frame.cpu().numpy().tobytes() == want_frame.tobytes(), (info.tolist(), want_info.tolist())
    assert info.tolist() == want_info.tolist()
    return want_info


# ---------------------------------------------------------------------------------------------------------------------
# store
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [64, 256])
def test_store_selection_shapes(K):
    store = _store(K=K, min_z=-5.0)
    ref = store.reference()
    for Q in (K - 7, K, K + 1, 5 * K + 3):
        info = _prepared(store, ref, cloud_of_cells(Q))
        assert info.tolist() == [min(Q, K), Q, 0, 0]
        store.add()
        ref.add()
    _same_store(store, ref)


@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_store_sizes_and_gate(N):
    """N straddles the gate kernel's block and the selection's strides; a fifth of the points is gated for each reason"""
    store = _store(K=128, min_z=-1.0, max_range=7.0)
    ref = store.reference()
    p = cloud(N, N + 3)
    r = np.random.default_rng(N)
    why = r.integers(0, 10, N)
    p[why == 0, r.integers(0, 3)] = np.nan
    p[why == 1, 1] = np.inf
    p[why == 2, 2] = -1.0                       # z > min_z is false on the boundary
    info = _prepared(store, ref, p)
    assert info[3] == int((~ref.gate(p)).sum()) and (N < 20 or 0 < info[3] < N)
    store.add()
    ref.add()
    _same_store(store, ref)


def test_store_all_gated_overflow_views_and_full():
    store = _store(capacity=3, K=64)
    ref = store.reference()
    low = cloud(300, 1)
    low[:, 2] = -2.0
    assert _prepared(store, ref, low).tolist() == [0, 0, 0, 300]
    store.add()
    ref.add()
    wide_s, wide_r = _store(voxel_size=1e-6, max_range=float("inf")), None
    wide_r = wide_s.reference()
    assert _prepared(wide_s, wide_r, np.array([[0, 0, 0], [3, 0, 0]], np.float32)).tolist() == [0, 0, 1, 0]
    # strided views: the first columns of a [P, 7] cloud and a [P, 4] scan, read in place
    from rslo_amd import synthetic
    c7 = synthetic.small_cloud(700, seed=4)
    t7 = dev(c7)
    _prepared(store, ref, c7, t7)
    store.add()
    ref.add()
    _prepared(store, ref, c7[:, :4], t7[:, :4])
    store.add()
    ref.add()
    _prepared(store, ref, c7[::2, :3], t7[::2, :3])
    store.add()                                 # the fourth and fifth entries do not fit
    ref.add()
    store.add()
    ref.add()
    _same_store(store, ref)
    assert store.stats()["n_entries"] == 3 and store.stats()["dropped_full"] == 2
    store.reset()
    assert store.stats()["n_entries"] == 0 and store.stats()["dropped_full"] == 0 and len(store.entries()[0]) == 0


def test_argument_errors_write_nothing():
    from rslo_amd import capi, loops
    lib = capi.lib()
    K, cap = 64, 4
    nbytes = capi.keyframe_bytes(cap, K)
    assert nbytes == 256 + 256 + cap * K * 16
    for bad in ((0, K), ((1 << 16) + 1, K), (cap, 0), (cap, 100), (cap, 4160)):
        assert capi.keyframe_bytes(*bad) == 0
    buf = torch.full((nbytes // 8,), SENTINEL, dtype=torch.int64, device="cuda")
    outs = torch.full((4096,), SENTINEL, dtype=torch.int64, device="cuda")
    p, o = buf.data_ptr(), outs.data_ptr()
    pts = dev(cloud(64, 0))
    ws = capi.keyframe_prepare_ws(64, "cuda")
    wsb = ws.numel() * 8
    frame, info, cands, out, ij, Z, w, cnt = o, o + 1024, o + 2048, o + 4096, o + 8192, o + 9216, o + 12288, o + 16384
    stages = (capi.C.c_double * 2)(1.0, 1.0)
    bad_stage = (capi.C.c_double * 2)(1.0, 65.0)
    nan, inf = float("nan"), float("inf")
    verify = lambda **kw: lib.rslo_loop_verify(*[{**dict(
        store=p, bytes=nbytes, cap=cap, K=K, frame=frame, info=info, cands=cands, top_k=1, start=None, stages=stages, n=1,
        max_distance=inf, inlier=0.5, overlap=0.5, rms=inf, pairs=50, damping=0.0, out=out, rows=None, matches=None,
        stream=None), **kw}[k] for k in ("store", "bytes", "cap", "K", "frame", "info", "cands", "top_k", "start", "stages",
                                         "n", "max_distance", "inlier", "overlap", "rms", "pairs", "damping", "out",
                                         "rows", "matches", "stream")])
    rcs = [lib.rslo_keyframe_reset(p, nbytes, 0, K, None), lib.rslo_keyframe_reset(p, nbytes, cap, 100, None),
           lib.rslo_keyframe_reset(p, nbytes - 8, cap, K, None), lib.rslo_keyframe_reset(None, nbytes, cap, K, None),
           lib.rslo_keyframe_reset(p + 8, nbytes, cap, K, None),
           lib.rslo_keyframe_prepare(pts.data_ptr(), 2, 64, K, 0.5, -1.4, 80.0, frame, info, ws.data_ptr(), wsb, None),
           lib.rslo_keyframe_prepare(pts.data_ptr(), 3, -1, K, 0.5, -1.4, 80.0, frame, info, ws.data_ptr(), wsb, None),
           lib.rslo_keyframe_prepare(pts.data_ptr(), 3, 64, 96, 0.5, -1.4, 80.0, frame, info, ws.data_ptr(), wsb, None),
           lib.rslo_keyframe_prepare(pts.data_ptr(), 3, 64, K, 0.0, -1.4, 80.0, frame, info, ws.data_ptr(), wsb, None),
           lib.rslo_keyframe_prepare(pts.data_ptr(), 3, 64, K, 0.5, nan, 80.0, frame, info, ws.data_ptr(), wsb, None),
           lib.rslo_keyframe_prepare(pts.data_ptr(), 3, 64, K, 0.5, -1.4, 0.0, frame, info, ws.data_ptr(), wsb, None),
           lib.rslo_keyframe_prepare(None, 3, 64, K, 0.5, -1.4, 80.0, frame, info, ws.data_ptr(), wsb, None),
           lib.rslo_keyframe_prepare(pts.data_ptr(), 3, 64, K, 0.5, -1.4, 80.0, None, info, ws.data_ptr(), wsb, None),
           lib.rslo_keyframe_prepare(pts.data_ptr(), 3, 64, K, 0.5, -1.4, 80.0, frame, info, None, wsb, None),
           lib.rslo_keyframe_prepare(pts.data_ptr(), 3, 64, K, 0.5, -1.4, 80.0, frame, info, ws.data_ptr(), 64, None),
           lib.rslo_keyframe_add(p, nbytes - 8, cap, K, frame, info, None), lib.rslo_keyframe_add(p, nbytes, cap, K, None, info, None),
           verify(bytes=nbytes - 8), verify(frame=None), verify(cands=None), verify(out=None), verify(top_k=0), verify(top_k=17),
           verify(n=0), verify(n=9), verify(stages=bad_stage), verify(inlier=0.0), verify(inlier=nan), verify(overlap=1.5),
           verify(rms=-1.0), verify(pairs=0), verify(damping=nan), verify(max_distance=nan),
           lib.rslo_loop_edges_reset(ij, Z, w, cnt, 0, None), lib.rslo_loop_edges_reset(ij, Z, w, cnt, 4097, None),
           lib.rslo_loop_edges_reset(None, Z, w, cnt, 4, None),
           lib.rslo_loop_emit(out, 0, p, nbytes, cap, K, ij, Z, w, cnt, 4, 1.0, 1.0, None),
           lib.rslo_loop_emit(out, 1, p, nbytes - 8, cap, K, ij, Z, w, cnt, 4, 1.0, 1.0, None),
           lib.rslo_loop_emit(out, 1, p, nbytes, cap, K, ij, Z, w, cnt, 0, 1.0, 1.0, None),
           lib.rslo_loop_emit(out, 1, p, nbytes, cap, K, ij, Z, w, cnt, 4, -1.0, 1.0, None),
           lib.rslo_loop_emit(None, 1, p, nbytes, cap, K, ij, Z, w, cnt, 4, 1.0, 1.0, None)]
    print("return codes:", rcs, lib.rslo_last_error().decode())
    assert all(rc != 0 for rc in rcs)
    # a buffer that was never reset holds no store: add and emit leave it, and the edge list, alone
    assert lib.rslo_keyframe_add(p, nbytes, cap, K, frame, info, None) == 0
    assert lib.rslo_loop_emit(out, 1, p, nbytes, cap, K, ij, Z, w, cnt, 4, 1.0, 1.0, None) == 0
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all()) and bool((outs == SENTINEL).all())
    # ... and so does a store that was reset with another shape
    assert lib.rslo_keyframe_reset(p, nbytes, cap, K, None) == 0
    assert lib.rslo_keyframe_add(p, nbytes, 2, K, frame, info, None) == 0
    torch.cuda.synchronize()
    assert buf[4:6].tolist() == [0, 0] and bool((buf[32:] == SENTINEL).all())
    for bad in (dict(capacity=0), dict(K=100), dict(voxel_size=0.0), dict(min_z=nan), dict(max_range=-1.0)):
        with pytest.raises(capi.RsloHipError):
            _store(**bad)
    for bad in (dict(threshold=1.0), dict(stages=[(1.0, 65)]), dict(min_pairs=0)):
        with pytest.raises(capi.RsloHipError):
            loops.LoopVerifier(_store(), **bad)
    with pytest.raises(capi.RsloHipError):
        loops.EdgeList(max_edges=0)
    with pytest.raises(capi.RsloHipError):
        _store().prepare(dev(cloud(64, 0)).cpu())
    with pytest.raises(capi.RsloHipError):
        loops.LoopVerifier(_store()).verify(torch.zeros((17, 4), dtype=torch.float64, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------------
# exact matching
# ---------------------------------------------------------------------------------------------------------------------
COUNTS = (50, 63, 64, 65, 255, 256, 257, 1023, 1024, 2048)
K_MATCH = 2048


def _lattice(n, seed):
    """n points on a quarter-metre lattice in [-6, 6)^3 (negative coordinates, many exact ties), every fifth one a
    duplicate of an earlier point, the last one an outlier at 10^6 m"""
    r = np.random.default_rng(seed)
    p = (r.integers(-24, 24, (n, 3)) * 0.25).astype(np.float32)
    dup = np.arange(5, n, 5)
    p[dup] = p[r.integers(0, dup, len(dup))]
    p[n - 1] = (1.0e6, 0.0, 0.0)
    return p


def _frame_of(points, K):
    f = np.zeros((K, 4), np.float32)
    f[:len(points), :3] = points
    return f, np.array([len(points), len(points), 0, 0], np.int32)


@pytest.fixture(scope="module")
def lattice_store():
    """ten entries with COUNTS points on both sides, never modified"""
    store = _store(capacity=16, K=K_MATCH)
    ref = store.reference()
    for n in COUNTS:
        f, i = _frame_of(_lattice(n, n), K_MATCH)
        store.add(dev(f), dev(i))
        ref.add(f, i)
    _same_store(store, ref)
    return store, ref


@pytest.mark.parametrize("nq", COUNTS)
def test_exact_matching(lattice_store, nq):
    """every query count against every entry count in one launch; the device's matches at the pose it ended on equal the
    brute force of the restatement at that pose, index for index"""
    from rslo_amd import loops
    store, ref = lattice_store
    r = np.random.default_rng(1000 + nq)
    q = _lattice(nq, nq)[:, :3] + np.float32(0.125) * r.integers(-1, 2, (nq, 3)).astype(np.float32)      # on and between lattice planes
    q[nq - 1] = 0.0                                                       # (the outlier is a target only)
    frame, info = _frame_of(q, K_MATCH)
    cands = np.array([[e, 0.1, 0, 0] for e in range(len(COUNTS))], np.float64)
    start = np.tile(np.array([0.25, -0.5, 0.0, 1, 0, 0, 0], np.float64), (len(COUNTS), 1))
    opts = dict(stages=[(2.0, 1)], inlier_dist=0.75, min_pairs=1)
    out, rows, matches = loops.LoopVerifier(store, **opts).verify(dev(cands), dev(frame), dev(info), start=dev(start), info=True,
                                                                  matches=True)
    out, rows, matches = out.cpu().numpy(), rows.cpu().numpy(), matches.cpu().numpy()
    vref = loops.LoopVerifierRef(ref, **opts)
    for e, nt in enumerate(COUNTS):
        assert out[e, 0] in (0.0, 5.0) and out[e, 5] == nq and out[e, 1] == e
        _, idx0, _ = vref.match(frame, info, e, start[e], 2.0)           # the iteration's pairs, at the given start
        assert rows[e, 0, 1] == float((idx0 >= 0).sum()) == out[e, 2]
        _, idx, d2 = vref.match(frame, info, e, out[e, 6:13], 0.75)      # the fitness, at the device's final pose
        assert matches[e, :nq].tolist() == idx.tolist() and (matches[e, nq:] == -1).all()
        assert out[e, 3] == (idx >= 0).sum() / float(nq)
        assert (idx != nt - 1).all()                                     # the outlier is nobody's match


def test_exact_ties_at_an_exact_pose():
    """A zero step keeps Z at the identity, where the lattice ties are exact: duplicates and equidistant targets go to
    the lowest index, and a target at 10^6 m changes nothing."""
    from rslo_amd import loops
    r = np.random.default_rng(5)
    body = np.unique((r.integers(-16, 16, (300, 3)) * 0.5).astype(np.float32), axis=0)[:200]
    target = np.concatenate([body, body[:40],                            # duplicates at higher indices
                             np.array([[20, 0, 0], [21, 0, 0], [19, 0, 0], [1.0e6, 0, 0]], np.float32)])
    query = np.concatenate([body[::-1], np.array([[20.5, 0, 0], [19.5, 0, 0]], np.float32)])      # two midpoints: residuals cancel
    store = _store(capacity=2, K=256)
    ref = store.reference()
    f, i = _frame_of(target, 256)
    store.add(dev(f), dev(i))
    ref.add(f, i)
    frame, info = _frame_of(query, 256)
    opts = dict(stages=[(1.0, 2)], inlier_dist=0.75, min_pairs=50)
    cands = np.array([[0, 0.1, 0, 0.0]])
    out, rows, matches = loops.LoopVerifier(store, **opts).verify(dev(cands), dev(frame), dev(info), info=True, matches=True)
    out, rows, matches = out.cpu().numpy()[0], rows.cpu().numpy()[0], matches.cpu().numpy()[0]
    assert out[0] == 0.0 and np.abs(out[6:13]).tolist() == list(IDENT) and (rows[:, 3:5] == 0).all()
    assert rows[:, 1].tolist() == [202.0, 202.0] and rows[:, 2].tolist() == [0.5, 0.5]
    want = loops.LoopVerifierRef(ref, **opts).match(frame, info, 0, np.array(IDENT), 0.75)[1]
    assert matches[:202].tolist() == want.tolist() and want[200:].tolist() == [240, 240] and want[:200].max() < 200


# ---------------------------------------------------------------------------------------------------------------------
# the street: one iteration, the whole call
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev_street():
    """the street of the host tests in a device store, filled through prepare / add"""
    from rslo_amd import synthetic
    s = street()
    store = _store(capacity=64, K=2048)
    for k in range(0, 61, 4):
        store.prepare(dev(synthetic.scan(720, 16, (-60.0 + 2.0 * k, 0.0), 0.0, scan_seed=k)))
        store.add()
    _same_store_entries(store, s["store"])
    return store


def _same_store_entries(store, ref):
    rows, counts = store.entries()
    want_rows, want_counts = ref.entries()
    assert rows.tobytes() == want_rows.tobytes() and counts.tolist() == want_counts.tolist()


def test_one_iteration_teacher_forced(dev_street):
    """Six successive iterations; both implementations start every one of them from the DEVICE's current Z."""
    from rslo_amd import loops
    from rslo_amd.gauss_newton import gauss_newton_step
    s = street()
    q = s["queries"][0]
    row = q["rows"][q["rows"][:, 0] == q["k"] // 4]
    frame, info = dev(q["frame"]), dev(q["info"])
    vref = loops.LoopVerifierRef(s["store"], stages=[(3.0, 1)])
    ver = loops.LoopVerifier(dev_street, stages=[(3.0, 1)])
    Z = dev(loops.heading_pose(row[0, 3])[None])
    worst = 0.0
    for it in range(6):
        cur = Z.cpu().numpy()[0].copy()
        out, rows, _ = ver.verify(dev(row), frame, info, start=Z, info=True)
        out, rows = out.cpu().numpy()[0], rows.cpu().numpy()[0]
        terms = vref.terms(q["frame"], q["info"], int(row[0, 0]), cur, 3.0)
        sums = terms.sum(axis=0)
        pairs = len(terms)
        assert rows[0, 0] == 0.0 and rows[0, 1] == pairs == out[2]
        cost_bound = pairs * 2.0 ** -50 * np.abs(terms[:, 27]).sum()
        assert abs(rows[0, 2] - sums[27]) <= cost_bound
        want, nt, th = gauss_newton_step(sums, cur, 0.0)
        bound = 1e4 * cond_of(sums) * 2.0 ** -52 * (1.0 + np.linalg.norm(cur[:3]))
        err = np.abs(out[6:13] - want).max()
        worst = max(worst, err / bound)
        print("iteration %d: step %.3e m, |dev - ref| %.3e, bound %.3e, pairs %d, cost %.6f (|dev - ref| %.1e, bound %.1e)" % (
            it, nt, err, bound, pairs, sums[27], abs(rows[0, 2] - sums[27]), cost_bound))
        assert err <= bound and abs(rows[0, 3] - nt) <= bound and abs(rows[0, 4] - th) <= bound
        Z = dev(out[None, 6:13])
    print("largest |dev - ref| / bound over six steps %.3g" % worst)


def test_whole_call(dev_street):
    from rslo_amd import loops
    s = street()
    ver = loops.LoopVerifier(dev_street)
    for q in s["queries"]:
        frame, info, cands = dev(q["frame"]), dev(q["info"]), dev(q["rows"])
        out, rows, matches = ver.verify(cands, frame, info, info=True, matches=True)
        out2, rows2, matches2 = ver.verify(cands, frame, info, info=True, matches=True)
        assert same_bits(out, out2) and same_bits(rows, rows2) and torch.equal(matches, matches2)      # two runs, the same bits
        # the same iterations as successive single-iteration calls chained through `start`
        Z = None                                            # the first one starts from the heading, as the whole call does
        singles = []
        for max_dist, iters in loops.DEFAULT_STAGES:
            one = loops.LoopVerifier(dev_street, stages=[(max_dist, 1)])
            for _ in range(iters):
                o1, r1, m1 = one.verify(cands, frame, info, start=Z, info=True, matches=True)
                singles.append(r1)
                Z = o1[:, 6:13].contiguous()
        assert same_bits(out, o1) and torch.equal(matches, m1)
        assert same_bits(rows[:, :, :5].contiguous(), torch.cat(singles, 1)[:, :, :5].contiguous())
        assert rows[0, :, 5].tolist() == [0.0] * 5 + [1.0] * 5 + [2.0] * 10
        got = out.cpu().numpy()
        print("k=%d statuses %s (restatement %s), overlaps %s" % (q["k"], got[:, 0], q["out"][:, 0], got[:, 3].round(3)))
        assert got[:, 0].tolist() == q["out"][:, 0].tolist() and got[:, 1].tolist() == q["rows"][:, 0].tolist()
        assert got[:, 5].tolist() == [float(q["info"][0])] * 3 and got[:, 13:15].tolist() == q["rows"][:, [1, 3]].tolist()
        for o in got[got[:, 0] == 0.0]:
            et, er = pose_error(o[6:13], q["truth"])
            print("  accepted entry %d: %.3f m, %.4f deg from the truth" % (o[1], et, er))
            assert et <= 0.25 and er <= 0.5
        assert (got[:, 0] == 0.0).sum() == 1


def test_status_paths(dev_street):
    from rslo_amd import loops
    s = street()
    q = s["queries"][0]
    own = float(q["k"] // 4)
    frame, info = dev(q["frame"]), dev(q["info"])
    rows = np.array([[-1, np.inf, -1, 0], [16, 0.1, 0, 0], [np.nan, 0.1, 0, 0], [own, 0.3, 0, 0.1]])
    for opts, cands, start, finfo in ((dict(max_distance=0.3), rows, None, q["info"]),
                                      (dict(), rows[3:], None, np.array([49, 49, 0, 0], np.int32)),
                                      (dict(min_pairs=1300), rows[3:], None, q["info"]),
                                      (dict(), rows[3:], np.array([[500.0, 0, 0, 1, 0, 0, 0]]), q["info"]),
                                      (dict(damping=-1e30), q["rows"][q["rows"][:, 0] == own], None, q["info"])):
        want = loops.LoopVerifierRef(s["store"], **opts).verify(cands, q["frame"], finfo, start=start)
        got = loops.LoopVerifier(dev_street, **opts).verify(dev(cands), frame, dev(finfo), start=None if start is None else dev(start),
                                                           info=True, matches=True)
        got = [g.cpu().numpy() for g in got]
        print(opts, "statuses", got[0][:, 0])
        assert got[0][:, 0].tolist() == want[0][:, 0].tolist() and set(got[0][:, 0]) <= {1.0, 2.0, 3.0, 4.0}
        assert np.array_equal(got[0], want[0], equal_nan=True) or (got[0][:, 0] == 4).all()
        assert np.array_equal(got[0][:, [0, 2, 3, 4, 5, 13, 14, 15]], want[0][:, [0, 2, 3, 4, 5, 13, 14, 15]])
        assert np.array_equal(got[1][:, :, [0, 1, 3, 4, 5, 6, 7]], want[1][:, :, [0, 1, 3, 4, 5, 6, 7]])
        assert np.array_equal(got[2], want[2]) and (got[2] == -1).all()
        if start is None and (got[0][:, 0] == 4).all():      # the failed step leaves the start (cos and sin differ in the last bit at most)
            assert np.abs(got[0][:, 6:13] - want[0][:, 6:13]).max() <= 2.0 ** -52


def test_emit_rules():
    from rslo_amd import loops
    store = _store(capacity=4, K=64)
    f, i = _frame_of(cloud(60, 0), 64)
    e, ref = loops.EdgeList(2, edge_w=(2.0, 3.0)), loops.EdgeListRef(2, edge_w=(2.0, 3.0))

    def same():
        got = [t.cpu().numpy() for t in e.tensors()]
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, (ref.ij, ref.Z, ref.w, ref.counters)))
    same()
    out = np.zeros((3, 16))
    out[:, 1], out[:, 3], out[:, 6:13] = (7, 8, 9), (0.8, 0.8, 0.99), np.array(IDENT) * 0.5
    for n, (status, overlap) in enumerate((((0, 0, 5), (0.8, 0.8, 0.99)), ((5, 4, 1), (0.8, 0.8, 0.99)), ((0, 0, 0), (0.6, 0.7, 0.65)),
                                            ((0, 0, 0), (0.6, 0.7, 0.65)))):
        out[:, 0], out[:, 3] = status, overlap
        e.emit(dev(out), store)                  # tie -> the lowest row; none accepted; the best; a full list
        ref.emit(out, n)
        store.add(dev(f), dev(i))                # j is the store's count at that moment
        same()
    assert ref.counters.tolist() == [2, 1] and ref.ij.tolist() == [[7, 0], [8, 2]]
    e.reset()
    ref.reset()
    same()


# ---------------------------------------------------------------------------------------------------------------------
# capture
# ---------------------------------------------------------------------------------------------------------------------
def test_capture_and_replay():
    """prepare -> verify -> emit -> add captured once on one stream over a static scan buffer and a static candidate row;
    replayed per scan it equals the eager bits; two eager runs agree."""
    from rslo_amd import loops, synthetic
    hosts = [synthetic.scan(720, 16, (2.0 * i, 0.1 * i), 0.02 * i, scan_seed=40 + i)[:, :4] for i in range(4)]
    n = max(len(h) for h in hosts)
    hosts = [np.concatenate([h, np.full((n - len(h), 4), np.nan, np.float32)]) for h in hosts]      # one static shape
    clouds = [dev(h) for h in hosts]
    cands = [dev(np.array([[i - 1, 0.2, 0, 0.0], [i - 2, 0.3, 0, 0.0]], np.float64)) for i in range(4)]

    def eager():
        store, edges = _store(capacity=8, K=256), loops.EdgeList(8)
        ver = loops.LoopVerifier(store)
        outs = torch.zeros((4, 2, 16), dtype=torch.float64, device="cuda")
        for i in range(4):
            store.prepare(clouds[i])
            ver.verify(cands[i], out=outs[i])
            edges.emit(outs[i], store)
            store.add()
        return outs, store, edges
    outs_a, store_a, edges_a = eager()
    outs_b, store_b, edges_b = eager()
    assert same_bits(outs_a, outs_b) and all(same_bits(a, b) for a, b in zip(edges_a.tensors(), edges_b.tensors()))
    print("eager statuses:\n%s\nedges %s" % (outs_a[:, :, 0].cpu().numpy(), edges_a.ij[:4].tolist()))
    assert outs_a[0, :, 0].tolist() == [1.0, 1.0] and outs_a[1, 1, 0] == 1.0 and (outs_a[1:, 0, 0] != 1.0).all()
    assert edges_a.counters.tolist()[0] >= 1
    store, edges = _store(capacity=8, K=256), loops.EdgeList(8)
    ver = loops.LoopVerifier(store)
    store.reserve(n)
    static, row = torch.zeros_like(clouds[0]), torch.zeros((2, 4), dtype=torch.float64, device="cuda")
    out = torch.zeros((2, 16), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with quiet_collector(), torch.cuda.graph(g):
        store.prepare(static)
        ver.verify(row, out=out)
        edges.emit(out, store)
        store.add()
    assert store.stats()["n_entries"] == 0                    # captured, not run
    res = []
    for c, r in zip(clouds, cands):
        static.copy_(c)
        row.copy_(r)
        g.replay()
        res.append(out.clone())
    assert same_bits(torch.stack(res), outs_a)
    assert all(same_bits(a, b) for a, b in zip(edges.tensors(), edges_a.tensors()))
    assert store.stats() == store_a.stats() and all(a.tobytes() == b.tobytes() for a, b in zip(store.entries(), store_a.entries()))


# ---------------------------------------------------------------------------------------------------------------------
# the runner
# ---------------------------------------------------------------------------------------------------------------------
LOOP = dict(exclude_recent=1, num_candidates=2, top_k=2)
odom = odom_fixture(21, 3, 3)


def test_runner_verifies_and_closes_loops(odom):
    """Three scans of the drive and one revisit of its start, K = 1024 so that the selection is exercised.  Scan 2 already
    has a candidate (entry 0: exclude_recent = 1 leaves it eligible), which is a true match one step back and is accepted;
    the revisit has two and emits exactly one edge with j = 3."""
    from rslo_amd import capi, inference, loops, places, posegraph, synthetic
    net, scans = odom
    scans = list(scans) + [dev(synthetic.scan(2083, 64, (0.5, 0.4), 0.2, scan_seed=999))]
    db = lambda cap=16: places.PlaceDB(capacity=cap)
    kf = lambda cap=16: loops.KeyframeStore(capacity=cap, K=1024)
    for bad in (dict(verify=dict()), dict(places=db(), loop=LOOP, verify=dict()), dict(keyframes=kf(), verify=dict()),
                dict(places=db(), keyframes=kf(), verify=dict(threshold=0.5)),
                dict(places=db(), keyframes=kf(), verify=dict(stages=[(1.0, 65)])),
                dict(places=db(), keyframes=kf(), verify=dict(max_edges=0)),
                dict(places=db(), keyframes=kf(), verify=dict(edge_w=(1.0, -1.0))),
                dict(places=db(8), keyframes=kf(), verify=dict(), capacity=16),
                dict(places=db(), keyframes=kf(8), verify=dict(), capacity=16),
                dict(places=db(), keyframes=kf(), verify=dict(max_edges=8), capacity=16,
                     pose_graph=posegraph.PoseGraph(capacity=16, max_loops=4))):
        with pytest.raises(capi.RsloHipError):                  # refused before anything is built
            inference.OdometryRunner(net, **bad)
    plain = inference.OdometryRunner(net)
    try:
        with quiet_collector():
            rel0, traj0 = stream(plain, scans)
        keys0 = set(plain.stats)
        for method in (plain.loop_checks, plain.loop_edges, plain.close_verified_loops):
            with pytest.raises(capi.RsloHipError):
                method()
    finally:
        plain.close()
    places_db, store = db(), kf()
    pg = posegraph.PoseGraph(capacity=16, max_loops=8)
    runner = inference.OdometryRunner(net, capacity=16, places=places_db, loop=LOOP, keyframes=store, verify=dict(max_edges=8),
                                      pose_graph=pg)
    try:
        with quiet_collector():
            rel, traj = stream(runner, scans)
        assert set(runner.stats) == keys0
        assert rel.tobytes() == rel0.tobytes() and traj.tobytes() == traj0.tobytes()      # verification disturbs nothing
        # the restatement of the same stream
        pref, sref = places_db.reference(), store.reference()
        vref, eref = loops.LoopVerifierRef(sref), loops.EdgeListRef(8)
        want = []
        for s in scans:
            h = s.cpu().numpy()
            d = pref.describe(h)
            rows = pref.query(*d, **LOOP)
            sref.prepare(h)
            want.append(vref.verify(rows)[0])
            eref.emit(want[-1], len(sref.rows))
            sref.add()
            pref.add(*d)
        want = np.stack(want)
        got = runner.loop_checks().cpu().numpy()
        eref.reset()
        for n in range(4):                                  # the emit rule on the device's own rows
            eref.emit(got[n], n)
        print("statuses:\n%s\nrestatement:\n%s\noverlaps:\n%s\nQ of the last scan %d" % (got[:, :, 0], want[:, :, 0], got[:, :, 3],
                                                                                     sref.info[1]))
        assert got.shape == (4, 2, 16) and got[:, :, 0].tolist() == want[:, :, 0].tolist()
        assert np.array_equal(got[:, :, [1, 5, 13, 14]], want[:, :, [1, 5, 13, 14]])
        assert (got[:2, :, 0] == 1).all() and got[2, 1, 0] == 1      # no candidate before scan 2 (exclude_recent = 1)
        assert sref.info[1] > 1024                                   # the selection is exercised
        # both candidates of the revisit are true matches and accepted.  (The restatement's overlaps here are 0.89 and 0.85:
        # K = 1024 keeps every second of the scan's Q = 1977 rows; at K = 2048, without selection, they are 0.91 and 0.94.)
        assert (want[3, :, 0] == 0).all() and (want[3, :, 3] >= 0.5).all() and np.abs(got[3, :, 3] - want[3, :, 3]).max() < 0.01
        _same_store(store, sref)
        ij, Z, w, counters = (t.cpu().numpy() for t in runner.loop_edges())
        assert counters.tolist() == eref.counters.tolist() and ij.tolist() == eref.ij.tolist()
        n_edges = int(counters[0])
        assert (ij[:n_edges, 1] == 3).sum() == 1 and ij[n_edges - 1].tolist() == [int(got[3, np.argmax(got[3, :, 3]), 1]), 3]
        assert (ij[n_edges:] == -1).all() and w[:n_edges].tolist() == [[1.0, 1.0]] * n_edges
        best = got[3, np.argmax(got[3, :, 3])]
        assert Z[n_edges - 1].tobytes() == best[6:13].tobytes()
        # close_verified_loops() is pose_graph.optimize on the same tensors
        poses, info = runner.close_verified_loops(gn_iters=3)
        poses2, info2 = pg.optimize(runner.trajectory(), *runner.loop_edges()[:3], gn_iters=3)
        assert same_bits(poses, poses2) and same_bits(info, info2)
        assert runner.optimized_trajectory() is poses and info.cpu().numpy()[0, 1] == n_edges
        runner.reset()                                      # a new sequence: an empty store and an empty list
        assert store.stats()["n_entries"] == 0 and len(runner.loop_checks()) == 0
        ij, _, _, counters = runner.loop_edges()
        assert counters.tolist() == [0, 0] and bool((ij == -1).all())
        stream(runner, scans[:1])
        assert store.stats()["n_entries"] == 1 and (runner.loop_checks().cpu().numpy()[0, :, 0] == 1).all()
    finally:
        runner.close()
    only = inference.OdometryRunner(net, capacity=16, keyframes=kf())      # keyframes= without verify= only stores frames
    try:
        with quiet_collector():
            rel, traj = stream(only, scans[:2])
        assert rel.tobytes() == rel0[:2].tobytes() and only.keyframes.stats()["n_entries"] == 2
        with pytest.raises(capi.RsloHipError):
            only.loop_checks()
    finally:
        only.close()
