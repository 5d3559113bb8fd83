"""Pose-graph optimisation on the GPU (csrc/posegraph.hip, rslo_amd/posegraph.py PoseGraph) against the float64
restatement PoseGraphRef.  Device and host sum in different orders, so the bars are rounding bounds, not bit equality;
bit equality is asked only between two device runs.

Where the bars come from (none from what the kernels return):
  * edge records: |dev - ref| <= 2^-46 * scale of the field.  Every value is a short expression (< 100 roundings of
    2^-53) of inputs bounded by (1 + |t|) and the weights: residuals and blocks scale as w (1 + |t|), B^-1 as (1 + |t|) /
    w, gradient parts as a block times a residual, e as a residual squared, rho is a ratio in [0, 1].
  * sums (gradient per node, cost, H x): |dev - ref| <= K * 2^-50 * sum|addend| over the K addends, four times the
    any-order bound, as in test_gpu_mapreg.py.  H x is compared on the DEVICE's own records (from_records),
    so that only order and rounding of the product differ, with addends |J|^T (|J| |x|).
  * chain solve: the host bar 64 cond2(J_c) 2^-52 |z| against the sequential recurrence on the device's records; cond2 is
    dense up to N = 66 and beyond that a LOWER bound from a few power iterations (a lower bound only tightens the bar).
  * a Gauss-Newton step: |x - x*|_H <= 2 sqrt(kappa) cg_tol |x*|_H against numpy.linalg.solve on the dense system
    linearised at the device's current poses (test_posegraph_host.py derives it).  The device's step is read back from
    the poses before and after (local_step), which round it to 2^-52 (1 + |t|) per component, sqrt(lambda_max(H))
    times that in the energy norm (about 3e-11).  Where the bound is above that rounding it is asserted as it stands; the
    later of the six steps are of rounding size themselves (|x*|_H ~ 1e-10 from the fifth on, the bound 1e-15), and
    there the error is held to the storage rounding alone.
"""
import numpy as np
import pytest
import torch

from rslo_amd import posegraph as pg
from test_posegraph_host import REF, from_records, local_step, piece_graph, records, synthetic
from stream_support import dev as _dev, network_and_scans      # (`dev` names the device's results below)

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2049, 8191]      # N - 1
LOOPS = [0, 1, 5]
_CACHE = {}


def _graph():
    if "pg" not in _CACHE:
        _CACHE["pg"] = pg.PoseGraph(capacity=8192, max_loops=32)
    return _CACHE["pg"]


def _loops(g):
    if len(g["loops_ij"]) == 0:
        return None, None, None
    return _dev(g["loops_ij"]), _dev(g["loops_Z"]), _dev(g["loops_w"])


def _linearized(E, L):
    """(graph, reference linearisation, device result as numpy, the device's records as a Linearization); the
    workspace of _graph() holds this linearisation afterwards"""
    g = piece_graph(E + 1, L)
    dev = _graph().linearize(_dev(g["traj0"]), _dev(g["poses"]), *_loops(g), chain_w=tuple(g["chain_w"]),
                             robust_scale=g["scale"])
    dev = {k: v.cpu().numpy() for k, v in dev.items()}
    if ("lin", E, L) not in _CACHE:
        _CACHE[("lin", E, L)] = REF.linearize(g["traj0"], g["poses"], g["chain_w"], g["loops_ij"], g["loops_Z"],
                                              g["loops_w"], g["scale"])
    return g, _CACHE[("lin", E, L)], dev, from_records(dev["edges"], E + 1, g["loops_ij"])


def _field_scales(g, lin):
    tmax = 1.0 + np.abs(np.concatenate([g["traj0"][:, :3], g["poses"][:, :3], g["loops_Z"][:, :3]])).max()
    w = np.concatenate([g["chain_w"][None, :], g["loops_w"]])
    wmax, wmin = w.max(), g["chain_w"].min()
    rmax = 1.0 + np.abs(lin.r).max()
    blk = wmax * tmax
    return {"r": blk, "rho": 1.0, "Att": blk, "Atr": blk, "Arr": blk, "Btt": blk, "Brr": blk, "gi": blk * rmax,
            "gj": blk * rmax, "e": rmax * rmax, "Binv_tt": tmax / wmin, "Binv_rr": tmax / wmin}


@pytest.mark.parametrize("L", LOOPS)
@pytest.mark.parametrize("E", SIZES)
def test_linearize(E, L):
    g, lin, dev, _ = _linearized(E, L)
    N = E + 1
    want = records(lin)
    got = dev["edges"]
    assert got.shape == want.shape == (E + L, pg.REC_DOUBLES)
    assert (got[:, pg.REC["flag"]] == want[:, pg.REC["flag"]]).all()           # used / skipped, no singular edge
    worst = 0.0
    offs = sorted(pg.REC.items(), key=lambda kv: kv[1])
    for (name, o), nxt in zip(offs, [v for _, v in offs[1:]] + [pg.REC_DOUBLES]):
        if name == "flag":
            continue
        tol = 2.0 ** -46 * _field_scales(g, lin)[name]
        err = np.abs(got[:, o:nxt] - want[:, o:nxt]).max() if len(got) else 0.0
        worst = max(worst, err / tol)
        assert err <= tol, (name, err, tol)
    # sums into a node and the cost: K * 2^-50 * sum|addend|
    terms = np.zeros((N, 6))
    np.add.at(terms, lin.i, np.abs(lin.gi))
    np.add.at(terms, lin.j, np.abs(lin.gj))
    K = np.zeros(N)
    np.add.at(K, lin.i[lin.valid], 1)
    np.add.at(K, lin.j[lin.valid], 1)
    tol_g = (K[:, None] * 2.0 ** -50) * terms + 2.0 ** -46 * _field_scales(g, lin)["gi"] * K[:, None]
    err_g = np.abs(dev["g"] - lin.g)
    assert (dev["g"][0] == 0).all() and (err_g[1:] <= tol_g[1:]).all()
    addends = lin.rho * lin.e
    tol_c = (E + L) * 2.0 ** -50 * addends.sum() + 2.0 ** -46 * _field_scales(g, lin)["e"] * (E + L)
    assert abs(dev["sums"][0] - lin.cost) <= tol_c and abs(dev["sums"][1] - lin.chain_cost) <= tol_c
    assert dev["sums"][2] == lin.loops_used and dev["sums"][3] == lin.loops_skipped
    print("N-1 %d L %d: %d loops used, %d skipped; worst record error / bar %.3g, gradient %.3g"
          % (E, L, lin.loops_used, lin.loops_skipped, worst, (err_g[1:] / np.maximum(tol_g[1:], 1e-300)).max()))
    again = _graph().linearize(_dev(g["traj0"]), _dev(g["poses"]), *_loops(g), chain_w=tuple(g["chain_w"]),
                               robust_scale=g["scale"])
    for k in dev:
        assert np.array_equal(again[k].cpu().numpy().view(np.int64), dev[k].view(np.int64)), k


@pytest.mark.parametrize("L", LOOPS)
@pytest.mark.parametrize("E", SIZES)
def test_matvec(E, L):
    g, lin, dev, dlin = _linearized(E, L)
    N = E + 1
    rng = np.random.default_rng(E + L)
    x = rng.standard_normal((N, 6))
    damping = 0.25
    got = _graph().matvec(_dev(x), damping).cpu().numpy()
    want = REF.matvec(dlin, x, damping)
    alin = from_records(np.abs(dev["edges"]), N, g["loops_ij"])               # |J|^T (|J| |x|): the addends' size
    alin.valid = dlin.valid
    terms = REF.matvec(alin, np.abs(x), damping)
    K = np.full(N, 1.0)
    np.add.at(K, dlin.i[dlin.valid], 72)                                        # 6 x 12 products per edge and component
    np.add.at(K, dlin.j[dlin.valid], 72)
    bar = K[:, None] * 2.0 ** -50 * terms
    err = np.abs(got - want)
    print("N-1 %d L %d: worst |dev - ref| / bar %.3g" % (E, L, (err[1:] / np.maximum(bar[1:], 1e-300)).max()))
    assert (got[0] == 0).all() and (err[1:] <= bar[1:]).all()
    x[0] = 7.0                                                                  # row 0 is read as zero
    again = _graph().matvec(_dev(x), damping).cpu().numpy()
    assert np.array_equal(again.view(np.int64), got.view(np.int64))


def _cond_lower_bound(E):
    """cond2(J_c) of the piece graph with E chain edges: dense up to 65 edges, else sigma_max and 1 / sigma_min from five
    power iterations each on H_chain and its inverse (both converge from below)"""
    if ("cond", E) in _CACHE:
        return _CACHE[("cond", E)]
    g = piece_graph(E + 1, 0)
    lin = REF.linearize(g["traj0"], g["poses"], g["chain_w"])
    if E <= 65:
        c = np.linalg.cond(REF.dense(lin)[3])
    else:
        rng = np.random.default_rng(0)
        v = rng.standard_normal((E + 1, 6))
        u = v.copy()
        for _ in range(5):
            v[0] = u[0] = 0.0
            v = REF.matvec(lin, v / np.linalg.norm(v))
            u = REF.chain_solve(lin, u / np.linalg.norm(u))
        c = np.sqrt(np.linalg.norm(v) * np.linalg.norm(u))
    _CACHE[("cond", E)] = c
    return c


@pytest.mark.parametrize("L", LOOPS)
@pytest.mark.parametrize("E", SIZES)
def test_chain_solve(E, L):
    g, lin, dev, dlin = _linearized(E, L)
    N = E + 1
    rng = np.random.default_rng(3 * E + L)
    r = rng.standard_normal((N, 6))
    r[0] = 0.0
    got = _graph().chain_solve(_dev(r)).cpu().numpy()
    want = REF.chain_solve(dlin, r)
    cond = _cond_lower_bound(E)
    bar = 64.0 * cond * 2.0 ** -52 * np.linalg.norm(want)
    err = np.linalg.norm(got - want)
    print("N-1 %d L %d: cond2(J_c) >= %.3g, |dev - ref| / bar %.3g, relative %.3g" % (E, L, cond, err / bar, err / np.linalg.norm(want)))
    assert (got[0] == 0).all() and err <= bar
    again = _graph().chain_solve(_dev(r)).cpu().numpy()
    assert np.array_equal(again.view(np.int64), got.view(np.int64))


OPT = dict(cg_iters=64, cg_tol=1e-8)


def _args(g):
    return (_dev(g["traj0"]),) + _loops(g)


def test_teacher_forced_gauss_newton_steps():
    g = synthetic(256, 4)
    graph = _graph()
    poses = _dev(g["traj0"]).clone()
    for step in range(6):
        before = poses.cpu().numpy()
        _, info = graph.optimize(*_args(g), poses=poses, chain_w=tuple(g["chain_w"]), gn_iters=1, **OPT)
        info = info.cpu().numpy()[0]
        x = local_step(before, poses.cpu().numpy())
        lin = REF.linearize(g["traj0"], before, g["chain_w"], g["loops_ij"], g["loops_Z"], g["loops_w"])
        H, gv, _, Jc = REF.dense(lin)
        want = np.linalg.solve(H, -gv)
        Ji = np.linalg.inv(Jc)
        ev = np.linalg.eigvalsh(Ji.T @ H @ Ji)
        kappa = ev[-1] / ev[0]
        d = x[1:].reshape(-1) - want
        err, nrm = np.sqrt(d @ H @ d), np.sqrt(want @ H @ want)
        _, rstatus, riters, _ = REF.pcg(lin, **OPT)
        # the issue's bound, unpadded, wherever it is above what the stored poses can resolve; below that only the
        # storage rounding itself: x is read back from poses that round it to 2^-52 (1 + |t|) per component
        eh = np.linalg.eigvalsh(H)
        tmax = 1.0 + np.abs(before[:, :3]).max()
        storage = np.sqrt(eh[-1]) * 2.0 ** -52 * tmax * np.sqrt(6 * 255)
        bar = 2.0 * np.sqrt(kappa) * 1e-8 * nrm
        print("step %d: kappa %.3g, CG %d (reference %d), |x - x*|_H %.3g, |x*|_H %.3g, bar %.3g, storage rounding %.3g, cost %.6g"
              % (step, kappa, info[3], riters, err, nrm, bar, storage, info[2]))
        assert err <= (bar if bar > storage else storage)
        assert info[0] == rstatus == 0 and info[1] == lin.loops_used == 4 and info[7] == 0
        assert abs(info[3] - riters) <= 2 and info[3] < 64
        assert abs(info[2] - lin.cost) <= 1e-12 * lin.cost + 1e-20


def _six(g, **kw):
    key = ("six", id(g), tuple(sorted(kw.items())))
    if key not in _CACHE:
        P, info = _graph().optimize(*_args(g), chain_w=tuple(g["chain_w"]), gn_iters=6, **OPT, **kw)
        _CACHE[key] = (P.cpu().numpy(), info.cpu().numpy())
    return _CACHE[key]


def test_six_iterations_equal_six_calls_and_reach_the_stationary_cost():
    g = synthetic(256, 4)
    P6, info6 = _six(g)
    poses = _dev(g["traj0"]).clone()
    rows = []
    for _ in range(6):
        _, info = _graph().optimize(*_args(g), poses=poses, chain_w=tuple(g["chain_w"]), gn_iters=1, **OPT)
        rows.append(info.cpu().numpy()[0])
    assert np.array_equal(poses.cpu().numpy().view(np.int64), P6.view(np.int64))
    assert np.array_equal(np.array(rows).view(np.int64), info6.view(np.int64))
    if "stationary" not in _CACHE:
        Pr, _ = REF.optimize(g["traj0"], g["loops_ij"], g["loops_Z"], g["loops_w"], chain_w=g["chain_w"], gn_iters=8,
                             exact=True)
        _CACHE["stationary"] = REF.cost(g["traj0"], Pr, g["chain_w"], g["loops_ij"], g["loops_Z"], g["loops_w"])[0]
    cost = _graph().cost(_dev(g["traj0"]), _dev(P6), *_loops(g), chain_w=tuple(g["chain_w"])).cpu().numpy()
    print("cost after six iterations %.12g, stationary %.12g; CG per iteration %s" % (cost[0], _CACHE["stationary"], info6[:, 3].tolist()))
    assert abs(cost[0] - _CACHE["stationary"]) <= 1e-6 * _CACHE["stationary"] and cost[2] == 4 and cost[3] == 0


def test_met_tolerances_skip_the_rest():
    g = synthetic(256, 4)
    P, info = _graph().optimize(*_args(g), chain_w=tuple(g["chain_w"]), gn_iters=4, tol_t=1e9, tol_r=1e9, **OPT)
    info = info.cpu().numpy()
    assert info[:, 0].tolist() == [0, 3, 3, 3] and (info[1:, 1:] == 0).all()
    P1, info1 = _graph().optimize(*_args(g), chain_w=tuple(g["chain_w"]), gn_iters=1, **OPT)
    assert torch.equal(P, P1) and np.array_equal(info1.cpu().numpy()[0], info[0])


def test_capture_and_two_replays_give_the_eager_bits():
    g = synthetic(256, 4)
    P6, info6 = _six(g)
    graph = _graph()
    traj0, ij, Z, w = _args(g)
    poses, info = traj0.clone(), torch.zeros((6, 8), dtype=torch.float64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph.optimize(traj0, ij, Z, w, poses=poses, chain_w=tuple(g["chain_w"]), gn_iters=6, info=info, **OPT)   # warm-up
        side.synchronize()
        cg = torch.cuda.CUDAGraph()
        poses.copy_(traj0)
        with torch.cuda.graph(cg, stream=side):
            graph.optimize(traj0, ij, Z, w, poses=poses, chain_w=tuple(g["chain_w"]), gn_iters=6, info=info, **OPT)
        for _ in range(2):
            poses.copy_(traj0)
            info.zero_()
            cg.replay()
            side.synchronize()
            assert np.array_equal(poses.cpu().numpy().view(np.int64), P6.view(np.int64))
            assert np.array_equal(info.cpu().numpy().view(np.int64), info6.view(np.int64))
    torch.cuda.current_stream().wait_stream(side)


def test_8192_nodes_16_loops_converge():
    g = synthetic(8192, 16)
    graph = _graph()
    P, info = graph.optimize(*_args(g), chain_w=tuple(g["chain_w"]), gn_iters=6, cg_iters=128, cg_tol=1e-8)
    info = info.cpu().numpy()
    c0 = REF.cost(g["traj0"], g["traj0"], g["chain_w"], g["loops_ij"], g["loops_Z"], g["loops_w"])[0]
    c6 = REF.cost(g["traj0"], P.cpu().numpy(), g["chain_w"], g["loops_ij"], g["loops_Z"], g["loops_w"])[0]
    print("N 8192 L 16: cost %.6g -> %.6g, CG %s, steps %s" % (c0, c6, info[:, 3].tolist(), info[:, 5].tolist()))
    assert (info[:, 0] == 0).all() and (info[:, 1] == 16).all()
    assert c6 < 1e-2 * c0                                 # the loops are true: closing them removes the drift's cost
    assert info[-1, 5] < 1e-3 * info[0, 5] and info[-1, 6] < 1e-3 * info[0, 6]      # Gauss-Newton has converged
    lin = REF.linearize(g["traj0"], P.cpu().numpy(), g["chain_w"], g["loops_ij"], g["loops_Z"], g["loops_w"])
    lin0 = REF.linearize(g["traj0"], g["traj0"], g["chain_w"], g["loops_ij"], g["loops_Z"], g["loops_w"])
    assert np.abs(lin.g).max() < 1e-6 * np.abs(lin0.g).max()


def _bits(*tensors):
    return [t.clone() for t in tensors]


def test_argument_errors_write_nothing():
    from rslo_amd import capi
    g = synthetic(64, 1)
    graph = pg.PoseGraph(capacity=64, max_loops=4)
    traj0, ij, Z, w = _args(g)
    poses = traj0.clone()
    info = torch.full((2, 8), -7.0, dtype=torch.float64, device="cuda")
    graph._ws.fill_(0x5a5a5a5a)
    keep = _bits(poses, info, graph._ws)
    ok = dict(gn_iters=2, cg_iters=8, cg_tol=1e-8, robust_scale=0.0, damping=0.0, tol_t=0.0, tol_r=0.0)
    bad = [dict(gn_iters=0), dict(gn_iters=33), dict(cg_iters=0), dict(cg_iters=257), dict(cg_tol=-1.0),
           dict(cg_tol=float("nan")), dict(robust_scale=-1.0), dict(robust_scale=float("inf")), dict(robust_scale=1e-200),
           dict(damping=-1.0), dict(damping=float("nan")), dict(tol_t=-1.0), dict(tol_r=float("nan"))]
    for kw in bad:
        args = dict(ok)
        args.update(kw)
        gn = args.pop("gn_iters")
        with pytest.raises(capi.RsloHipError, match=r"\(-1\)"):
            capi.posegraph_optimize(traj0, poses, (1.0, 1.0), ij, Z, w, gn, args["cg_iters"], args["cg_tol"],
                                    args["robust_scale"], args["damping"], args["tol_t"], args["tol_r"],
                                    info[:gn] if 1 <= gn <= 2 else info, graph._ws)
    for cw in ((0.0, 1.0), (1.0, -1.0), (float("nan"), 1.0), (1.0, float("inf"))):
        with pytest.raises(capi.RsloHipError, match=r"\(-1\)"):
            capi.posegraph_optimize(traj0, poses, cw, ij, Z, w, 2, 8, 1e-8, 0.0, 0.0, 0.0, 0.0, info, graph._ws)
    with pytest.raises(capi.RsloHipError, match=r"\(-4\)"):                    # a short workspace
        capi.posegraph_optimize(traj0, poses, (1.0, 1.0), ij, Z, w, 2, 8, 1e-8, 0.0, 0.0, 0.0, 0.0, info, graph._ws[:64])
    with pytest.raises(capi.RsloHipError, match=r"\(-1\)"):                    # N = 1
        capi.posegraph_optimize(traj0[:1], poses[:1], (1.0, 1.0), None, None, None, 2, 8, 1e-8, 0.0, 0.0, 0.0, 0.0, info,
                                graph._ws)
    lib = capi.lib()
    assert lib.rslo_posegraph_ws_bytes(1, 0) == 0 and lib.rslo_posegraph_ws_bytes(65537, 0) == 0
    assert lib.rslo_posegraph_ws_bytes(64, 4097) == 0 and lib.rslo_posegraph_ws_bytes(64, -1) == 0
    x = torch.zeros((64, 6), dtype=torch.float64, device="cuda")
    with pytest.raises(capi.RsloHipError, match=r"\(-1\)"):
        capi.posegraph_matvec(x, x, 64, 1, 0.0, graph._ws)
    with pytest.raises(capi.RsloHipError, match=r"\(-1\)"):
        capi.posegraph_matvec(x, x.clone(), 64, 1, -1.0, graph._ws)
    with pytest.raises(capi.RsloHipError, match=r"\(-4\)"):
        capi.posegraph_chain_solve(x, x.clone(), 64, 1, graph._ws[:64])
    with pytest.raises(capi.RsloHipError):
        graph.optimize(_dev(synthetic(256, 4)["traj0"]))                       # above the capacity
    with pytest.raises(capi.RsloHipError):
        graph.matvec(x)                                                         # no linearisation held
    torch.cuda.synchronize()
    for was, now in zip(keep, (poses, info, graph._ws)):
        assert torch.equal(was, now)
    # the pieces refuse a workspace that holds no linearisation of this graph: nothing is written
    y = torch.full((64, 6), 3.0, dtype=torch.float64, device="cuda")
    capi.posegraph_matvec(x, y, 64, 1, 0.0, graph._ws)
    capi.posegraph_chain_solve(x, y, 64, 1, graph._ws)
    assert (y == 3.0).all()


def test_falsified_loop_matches_the_reference_weights():
    g = synthetic(256, 4, falsify=True)
    for scale in (0.0, 3.0):
        P, info = _graph().optimize(*_args(g), chain_w=tuple(g["chain_w"]), gn_iters=6, robust_scale=scale, **OPT)
        Pr, info_r = REF.optimize(g["traj0"], g["loops_ij"], g["loops_Z"], g["loops_w"], chain_w=g["chain_w"], gn_iters=6,
                                  robust_scale=scale, **OPT)
        lin = _graph().linearize(_dev(g["traj0"]), P, *_loops(g), chain_w=tuple(g["chain_w"]), robust_scale=scale)
        rho = lin["edges"][255:, pg.REC["rho"]].cpu().numpy()
        rho_r = REF.linearize(g["traj0"], Pr, g["chain_w"], g["loops_ij"], g["loops_Z"], g["loops_w"], scale).rho[255:]
        print("robust_scale %g: rho %s, reference %s" % (scale, rho, rho_r))
        assert np.abs(rho - rho_r).max() <= 1e-6 and (info.cpu().numpy()[:, 0] == 0).all()
        if scale:
            assert rho[g["falsified"]] < 1e-3 and (np.delete(rho, g["falsified"]) > 0.99).all()
        else:
            assert (rho == 1.0).all()


def test_skipped_rows_and_device_chain_weights():
    g = piece_graph(65, 5)
    cw = np.tile(g["chain_w"], (64, 1))
    a = _graph().cost(_dev(g["traj0"]), _dev(g["poses"]), *_loops(g), chain_w=tuple(g["chain_w"]), robust_scale=2.0)
    b = _graph().cost(_dev(g["traj0"]), _dev(g["poses"]), *_loops(g), chain_w=_dev(cw), robust_scale=2.0)
    want = REF.cost(g["traj0"], g["poses"], g["chain_w"], g["loops_ij"], g["loops_Z"], g["loops_w"], 2.0)
    assert torch.equal(a, b) and a[2].item() == want[2] == 4 and a[3].item() == want[3] == 1
    cw[10, 1] = 0.0                            # a singular B_k: status 2, poses untouched
    poses = _dev(g["poses"])
    P, info = _graph().optimize(_dev(g["traj0"]), *_loops(g), poses=poses.clone(), chain_w=_dev(cw), gn_iters=2, **OPT)
    assert info.cpu().numpy()[:, 0].tolist() == [2, 2] and torch.equal(P, poses)
    A, B = _dev(g["poses"][:10]), _dev(g["poses"][20:30])
    assert np.abs(_graph().between(A, B).cpu().numpy() - REF.between(g["poses"][:10], g["poses"][20:30])).max() < 1e-13


def test_singular_chain_edge_is_status_2():
    """q_E.w == 0 exactly on a chain edge: identity odometry, node 1 turned by pi about z"""
    T = np.tile(np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]), (3, 1))
    poses = T.copy()
    poses[1, 3:] = (0.0, 0.0, 0.0, 1.0)
    graph = _graph()
    lin = graph.linearize(_dev(T), _dev(poses))
    assert lin["edges"][0, pg.REC["flag"]].item() == 2.0 and REF.linearize(T, poses).singular
    dposes = _dev(poses)
    P, info = graph.optimize(_dev(T), poses=dposes.clone(), gn_iters=2, **OPT)
    info = info.cpu().numpy()
    assert info[:, 0].tolist() == [2, 2] and (info[:, 3] == 0).all() and (info[:, 5:7] == 0).all()
    assert torch.equal(P, dposes)


def test_pieces_write_nothing_without_the_scan_matrices():
    """cost() and a linearisation with a singular chain edge make no scan matrices: the mark is cleared, matvec and
    chain_solve with the same N, L and workspace leave their output alone"""
    from rslo_amd import capi
    g = piece_graph(65, 1)
    graph = pg.PoseGraph(capacity=65, max_loops=4)
    args = (_dev(g["traj0"]), _dev(g["poses"])) + _loops(g)
    r = _dev(np.random.default_rng(0).standard_normal((65, 6)))
    graph.linearize(*args, chain_w=tuple(g["chain_w"]))
    z_ok = graph.chain_solve(r)
    assert torch.isfinite(z_ok).all() and (z_ok[1:] != 3.0).any()
    graph.cost(*args, chain_w=tuple(g["chain_w"]))
    for call in (lambda out: capi.posegraph_chain_solve(r, out, 65, 1, graph._ws),
                 lambda out: capi.posegraph_matvec(r, out, 65, 1, 0.0, graph._ws)):
        out = torch.full((65, 6), 3.0, dtype=torch.float64, device="cuda")
        call(out)
        assert (out == 3.0).all()
    graph.linearize(*args, chain_w=tuple(g["chain_w"]))                      # the mark comes back with a linearize
    assert torch.equal(graph.chain_solve(r), z_ok)
    cw = np.tile(g["chain_w"], (64, 1))
    cw[5, 0] = 0.0                                                           # a singular B_5
    graph.linearize(*args, chain_w=_dev(cw))
    out = torch.full((65, 6), 3.0, dtype=torch.float64, device="cuda")
    capi.posegraph_chain_solve(r, out, 65, 1, graph._ws)
    assert (out == 3.0).all()


def test_loops_onto_the_fixed_node_cost_no_round():
    """eight loops (0, j): node 0 receives no sum, so the ranks there are not counted; the result is the reference's"""
    g = synthetic(256, 4)
    j = np.array([30, 60, 90, 120, 150, 180, 210, 255])
    ij = np.stack([np.zeros_like(j), j], 1).astype(np.int32)
    Z = pg.between(g["truth"][ij[:, 0]], g["truth"][ij[:, 1]])
    w = np.tile(10.0 * g["chain_w"][None, :], (8, 1))
    graph = _graph()
    lin = graph.linearize(_dev(g["traj0"]), _dev(g["traj0"]), _dev(ij), _dev(Z), _dev(w), chain_w=tuple(g["chain_w"]))
    ref = REF.linearize(g["traj0"], g["traj0"], g["chain_w"], ij, Z, w)
    x = np.random.default_rng(2).standard_normal((256, 6))
    got = graph.matvec(_dev(x)).cpu().numpy()
    want = REF.matvec(from_records(lin["edges"].cpu().numpy(), 256, ij), x)
    scale = np.abs(want).max()
    assert np.abs(got - want).max() <= 2.0 ** -40 * scale                    # (the rounding bars are test_matvec's business)
    assert np.abs(lin["g"].cpu().numpy() - ref.g).max() <= 2.0 ** -40 * np.abs(ref.g).max()
    hdr = graph._ws[:32].cpu().numpy().view(np.int32)
    assert hdr[4] == 0                                                       # the largest rank: one round


def test_runner_closes_loops():
    from rslo_amd import capi, inference
    net, scans = network_and_scans(21, 3, 6)
    graph = pg.PoseGraph(capacity=16, max_loops=4)
    runner = inference.OdometryRunner(net, capacity=16, pose_graph=graph)
    try:
        for scan in scans:
            runner.run(runner.submit(scan))
        with pytest.raises(capi.RsloHipError):
            runner.optimized_trajectory()
        traj = runner.trajectory().clone()
        rel = runner.relative().clone()
        ij = torch.tensor([[0, 5]], dtype=torch.int32, device="cuda")
        Z = graph.between(traj[0:1], traj[5:6]).clone()
        Z[0, 0] += 0.05                        # the loop disagrees with the odometry by 5 cm
        runner.close_loops(ij, Z, gn_iters=3, cg_iters=16)
        assert torch.equal(runner.trajectory(), traj) and torch.equal(runner.relative(), rel)
        want, info = graph.optimize(traj, ij, Z, gn_iters=3, cg_iters=16)
        assert torch.equal(runner.optimized_trajectory(), want) and torch.equal(runner.pose_graph_info(), info)
        assert not torch.equal(want, traj) and (info[:, 0] == 0).all()
        runner.pose_graph = None               # a runner without a pose graph raises
        with pytest.raises(capi.RsloHipError):
            runner.close_loops(ij, Z)
    finally:
        runner.close()
