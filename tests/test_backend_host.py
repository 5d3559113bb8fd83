"""The streaming back end (rslo_amd.backend) on the host: every refusal of backend.check and the defaults it fills in,
on stand-ins that carry only what the check reads; and the call order of BackEnd.step / reset on a BackEnd(device="cpu")
whose collaborators -- the maps, the database, the store, the stages it builds itself and both pose chains -- only
record what they are called with (no GPU needed).  The tables of expected calls are written out from the sequence
OdometryRunner.run() issued before the back end became a class."""
import math
import types

import pytest
import torch

import rslo_amd  # noqa: F401
from rslo_amd import backend, capi

CPU, ELSEWHERE = torch.device("cpu"), torch.device("cuda", 0)


def _standin(device=CPU, **attrs):
    return types.SimpleNamespace(device=device, **attrs)


MAP, SURF = _standin(), _standin(voxel_size=0.4)
DB, STORE, GRAPH = _standin(capacity=16), _standin(capacity=16), _standin(max_loops=4)
LOOPS = dict(places=DB, keyframes=STORE)

REFUSALS = {
    "carve without voxel_map": (dict(carve=dict()), "carve needs a voxel_map"),
    "carve key": (dict(voxel_map=MAP, carve=dict(evry=2)), "carve takes"),
    "carve every=0": (dict(voxel_map=MAP, carve=dict(every=0)), "every"),
    "refine without voxel_map": (dict(refine=dict()), "refine needs a voxel_map"),
    "refine without voxel_map, with surfels": (dict(refine=dict(iters=1), surfels=SURF), "refine needs a voxel_map"),
    "schedule on a plain map": (dict(voxel_map=MAP, refine=dict(schedule=[(0, 1, None, 0.0)])), "MapPyramid"),
    "refine key": (dict(voxel_map=MAP, refine=dict(metric="plane")), "refine takes"),
    "surfel_refine without surfels": (dict(surfel_refine=dict()), "surfel_refine needs surfels"),
    "surfel_refine key": (dict(surfels=SURF, surfel_refine=dict(iter=2)), "surfel_refine takes"),
    "deskew refined without a refining stage": (dict(deskew=dict(motion="refined")), "needs refine= or surfel_refine="),
    "deskew refined beside a plain map": (dict(voxel_map=MAP, deskew=dict(motion="refined")), "needs refine="),
    "deskew key": (dict(deskew=dict(stmp=0.5)), "deskew takes"),
    "loop without places": (dict(loop=dict()), "loop needs places"),
    "loop key": (dict(places=DB, loop=dict(topk=2)), "loop takes"),
    "loop value": (dict(places=DB, loop=dict(top_k=17)), "top_k"),
    "verify without places": (dict(keyframes=STORE, verify=dict()), "verify needs places"),
    "verify without keyframes": (dict(places=DB, verify=dict()), "verify needs places"),
    "verify key": (dict(verify=dict(stage=()), **LOOPS), "verify takes"),
    "max_edges above max_loops": (dict(verify=dict(max_edges=5), pose_graph=GRAPH, **LOOPS), "exceeds pose_graph.max_loops"),
    "store below capacity": (dict(keyframes=_standin(capacity=15)), "keyframes capacity 15"),
    "database below capacity": (dict(places=_standin(capacity=15), keyframes=STORE, verify=dict()), "places capacity 15"),
    "local_map without radius": (dict(voxel_map=MAP, local_map=dict(every=2)), "needs a radius"),
    "local_map every=0": (dict(voxel_map=MAP, local_map=dict(radius=30.0, every=0)), "every"),
    "local_map key": (dict(voxel_map=MAP, local_map=dict(radius=30.0, evry=2)), "local_map takes"),
    "local_map radius": (dict(voxel_map=MAP, local_map=dict(radius=-1.0)), "radius"),
    "local_map min_hits": (dict(voxel_map=MAP, local_map=dict(radius=30.0, min_hits=0)), "min_hits"),
    "surfels key without surfels=": (dict(voxel_map=MAP, local_map=dict(radius=30.0, surfels=True)), "needs surfels="),
    "no key and no voxel_map": (dict(surfels=SURF, local_map=dict(radius=30.0)), "needs a voxel_map"),
    "surfels key's keys": (dict(surfels=SURF, local_map=dict(radius=30.0, surfels=dict(min_cnt=2))), "local_map surfels takes"),
    "inner_radius above the radius": (dict(surfels=SURF, local_map=dict(radius=30.0, surfels=dict(inner_radius=31.0))),
                                      "inner_radius"),
    "min_count=0": (dict(surfels=SURF, local_map=dict(radius=30.0, surfels=dict(min_count=0))), "min_count"),
    "voxel map elsewhere": (dict(voxel_map=_standin(ELSEWHERE)), "the voxel map lives on cuda:0, the runner on cpu"),
    "surfel map elsewhere": (dict(surfels=_standin(ELSEWHERE)), "the surfel map lives on"),
    "database elsewhere": (dict(places=_standin(ELSEWHERE, capacity=16)), "the place database lives on"),
    "store elsewhere": (dict(keyframes=_standin(ELSEWHERE, capacity=16)), "the keyframe store lives on"),
    "pose graph elsewhere": (dict(pose_graph=_standin(ELSEWHERE, max_loops=4)), "the pose graph lives on"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_check_refuses(case):
    options, message = REFUSALS[case]
    with pytest.raises(ValueError, match=message):
        backend.check(16, "cpu", **options)
    with pytest.raises(ValueError, match=message):      # and a BackEnd of these options builds nothing either
        backend.BackEnd(None, capacity=16, device="cpu", **options)


def test_check_fills_in_the_defaults():
    """the values the class docstring of BackEnd promises"""
    off = backend.check(16, "cpu")
    assert off == dict(refine=None, info_rows=0, surfel_refine=None, local_map=None, loop=None, verify=None, edges=None,
                       deskew=None, carve=None)
    on = backend.check(16, "cpu", voxel_map=MAP, refine=dict(), surfels=SURF, surfel_refine=dict(), places=DB, keyframes=STORE,
                       pose_graph=GRAPH, verify=dict(max_edges=4), local_map=dict(radius=30), deskew=dict(), carve=dict())
    assert on["refine"] == dict(iters=5) and on["info_rows"] == 5
    assert on["surfel_refine"] == dict(iters=4, max_dist=None, robust_scale=0.2, damping=1e-6, min_pairs=50, tol_t=0.0, tol_r=0.0)
    assert on["loop"] == dict(exclude_recent=50, num_candidates=10, top_k=1)
    assert on["verify"] == dict(stages=((3.0, 5), (1.5, 5), (0.75, 10)), max_distance=math.inf, inlier_dist=0.5,
                                min_overlap=0.5, max_rms=math.inf, min_pairs=50, damping=0.0)
    assert on["edges"] == (4, (1.0, 1.0))
    assert on["local_map"] == dict(radius=30.0, every=1, min_hits=1, grace=0)
    assert on["deskew"] == dict(motion="network", times="azimuth", stamp=0.5, az_start_turn=-0.5, az_clockwise=False,
                                max_angle=math.pi / 2)
    assert on["carve"] == dict(every=1, rows=64, cols=1024, tan_lo=math.tan(math.radians(-25.0)),
                               tan_hi=math.tan(math.radians(3.0)), win_rows=1, win_cols=1, margin_abs=0.3, margin_rel=0.0,
                               max_range=60.0, grace=1)
    more = backend.check(16, "cpu", surfels=SURF, surfel_refine=dict(cost="distribution"), places=DB, keyframes=STORE,
                         verify=dict(), loop=dict(top_k=3), local_map=dict(radius=30.0, every=2, surfels=True))
    assert more["surfel_refine"] == dict(iters=4, max_dist=None, robust_scale=3.0, damping=1e-6, min_pairs=50, tol_t=0.0,
                                         tol_r=0.0, cost="distribution", min_flag=1, reg_rel=0.01, reg_abs=0.02)
    assert more["edges"] == (256, (1.0, 1.0)) and more["loop"]["top_k"] == 3
    assert more["local_map"] == dict(radius=30.0, every=2, min_hits=1, grace=0, surfels=dict(min_count=1, inner_radius=30.0))


def test_a_back_end_of_nothing_constructs_on_the_cpu():
    back = backend.BackEnd(backend.PoseChain(4, "cpu"), capacity=4, device="cpu")
    assert back.device == CPU and back.n == 0 and not back.reads_scans and back.chain.traj.shape == (4, 7)
    back.step(None)
    assert back.n == 1
    for name in ("refined_trajectory", "refine_info", "surfel_refine_info", "deskew_info", "deskewed", "loop_candidates",
                 "loop_checks", "loop_edges", "optimized_trajectory", "pose_graph_info", "close_verified_loops", "rebuild_map",
                 "adopt_loop_closure"):
        with pytest.raises(capi.RsloHipError):
            getattr(back, name)()
    with pytest.raises(capi.RsloHipError):
        back.close_loops(None, None)


# ---------------------------------------------------------------------------------------------------------------------
# the order of step() and reset()
# ---------------------------------------------------------------------------------------------------------------------
CAPACITY = 8


class _World:
    """the log, and the names of the tensors and objects that the recorded calls are given"""

    def __init__(self):
        self.log, self.names = [], {}

    def name(self, what, name):
        self.names[what.data_ptr() if torch.is_tensor(what) else id(what)] = name
        return what

    def describe(self, args, kwargs):
        key = lambda a: a.data_ptr() if torch.is_tensor(a) else id(a)
        known = [self.names[key(a)] for a in args if key(a) in self.names]
        known += ["%s=%s" % (k, self.names[key(a)]) for k, a in kwargs.items() if key(a) in self.names]
        return ", ".join(known)

    def take(self):
        out, self.log[:] = list(self.log), []
        return out


class _Fake:
    """records every call as "name.method(the arguments the world knows by name)"; calling the object itself records
    "name(...)" and returns `result`"""

    def __init__(self, world, name, result=None, **attrs):
        self.__dict__.update(attrs, _world=world, _name=name, _result=result)
        world.name(self, name)

    def __getattr__(self, method):
        if method.startswith("__"):
            raise AttributeError(method)
        return lambda *args, **kwargs: self._world.log.append("%s.%s(%s)" % (self._name, method, self._world.describe(args, kwargs)))

    def __call__(self, *args, **kwargs):
        self._world.log.append("%s(%s)" % (self._name, self._world.describe(args, kwargs)))
        return self if self._result is None else self._result


def _chain(world, name):
    """a stand-in for PoseChain: the tensors on the host, every row known by name, push / set_state / reset recorded"""
    rel, traj = torch.zeros((CAPACITY, 7)), torch.zeros((CAPACITY, 7), dtype=torch.float64)
    for i in range(CAPACITY):
        world.name(rel[i], "%s.rel[%d]" % (name, i))
        world.name(traj[i], "%s.traj[%d]" % (name, i))
    return _Fake(world, name, rel=rel, traj=traj)


def _back_end(monkeypatch, **options):
    """(world, BackEnd on the cpu over recording collaborators): options name the collaborators by True"""
    from rslo_amd import carve, deskew, loops
    world = _World()
    world.deskewed = world.name(torch.zeros((5, 7)), "deskewed")
    monkeypatch.setattr(backend, "PoseChain", lambda capacity, device: _chain(world, "refined"))
    monkeypatch.setattr(carve, "RangeImage", lambda *a: _Fake(world, "range_image"))
    monkeypatch.setattr(deskew, "Deskewer", lambda cap, F, device, **kw: _Fake(world, "deskew", result=world.deskewed, n_cols=F))
    monkeypatch.setattr(loops, "LoopVerifier", lambda store, **kw: _Fake(world, "verifier"))
    monkeypatch.setattr(loops, "EdgeList", lambda *a, **kw: _Fake(world, "edges"))
    made = dict(voxel_map=dict(), surfels=dict(voxel_size=0.4), places=dict(capacity=CAPACITY), keyframes=dict(capacity=CAPACITY),
                pose_graph=dict(max_loops=256))
    for key, attrs in made.items():
        if options.get(key) is True:
            options[key] = _Fake(world, key, device=CPU, **attrs)
    back = backend.BackEnd(_chain(world, "open"), capacity=CAPACITY, point_capacity=100, device="cpu", **options)
    return world, back


def _scan(world):
    return world.name(torch.zeros((5, 7)), "scan")


EVERYTHING = dict(voxel_map=True, refine=dict(iters=1), surfels=True, surfel_refine=dict(iters=1), places=True, keyframes=True,
                  verify=dict(), local_map=dict(radius=30.0, every=2, surfels=True), carve=dict(every=2))


def _expected(n, motion):
    """what run() issued for scan n of a runner with EVERYTHING and deskew=dict(motion=motion), in its order"""
    row, src = "refined.traj[%d]" % n, "deskewed"
    if motion == "network":
        calls = ["deskew(scan%s)" % (", rel7=open.rel[%d]" % n if n >= 1 else "")]
    else:
        calls = ["deskew(scan%s)" % (", pose_a=refined.traj[%d], pose_b=refined.traj[%d]" % (n - 2, n - 1) if n >= 2 else "")]
    calls += ["refined.push(open.rel[%d])" % n,
              "voxel_map.register(%s, %s)" % (src, row),
              "surfels.register(%s, %s)" % (src, row),
              "refined.set_state(%s)" % row]
    if n % 2 == 1:
        calls += ["range_image(%s)" % src, "voxel_map.carve(range_image, %s)" % row]
    calls += ["voxel_map.insert(%s, %s)" % (src, row), "surfels.insert(%s, %s)" % (src, row)]
    if n % 2 == 1:
        calls += ["voxel_map.prune(%s)" % row, "surfels.prune(%s)" % row]
    calls += ["places.describe(%s)" % src, "places.query()", "keyframes.prepare(%s)" % src, "verifier.verify()",
              "edges.emit(keyframes)", "keyframes.add()", "places.add()"]
    return calls


@pytest.mark.parametrize("motion", ["network", "refined"])
def test_step_order_with_everything_on(monkeypatch, motion):
    world, back = _back_end(monkeypatch, deskew=dict(motion=motion), **EVERYTHING)
    built = world.take()                                       # construction reserves, and nothing else
    assert sorted(built) == sorted(["voxel_map.reserve()", "surfels.reserve()", "places.reserve()", "keyframes.reserve()",
                                    "surfels.reserve_prune()", "voxel_map.reserve_prune()", "voxel_map.reserve_prune()"])
    assert back.reads_scans and back.range_image is not None
    for n in range(4):
        assert back.n == n
        back.step(_scan(world))
        assert world.take() == _expected(n, motion), "scan %d" % n
    assert back.n == 4 and back.deskewed() is world.deskewed
    assert back.refined_trajectory().shape == (4, 7) and back.refine_info().shape == (4, 1, 8)
    assert back.loop_candidates().shape == (4, 1, 4) and back.loop_checks().shape == (4, 1, 16)
    assert back.deskew_info().shape == (4, 8) and back.surfel_refine_info().shape == (4, 1, 8)


def test_step_order_with_a_store_and_no_database(monkeypatch):
    world, back = _back_end(monkeypatch, keyframes=True)
    world.take()
    for n in range(2):
        back.step(_scan(world))
        assert world.take() == ["keyframes.prepare(scan)", "keyframes.add()"]


def test_step_uses_the_open_loop_row_when_nothing_refines(monkeypatch):
    world, back = _back_end(monkeypatch, voxel_map=True, surfels=True, places=True,
                            local_map=dict(radius=30.0, every=2, surfels=True), carve=dict(every=2))
    world.take()
    assert back.refined is None
    for n in range(4):
        back.step(_scan(world))
        row = "open.traj[%d]" % n
        odd = n % 2 == 1
        assert world.take() == (
            ["range_image(scan)", "voxel_map.carve(range_image, %s)" % row] * odd
            + ["voxel_map.insert(scan, %s)" % row, "surfels.insert(scan, %s)" % row]
            + ["voxel_map.prune(%s)" % row, "surfels.prune(%s)" % row] * odd
            + ["places.describe(scan)", "places.query()", "places.add()"]), "scan %d" % n


def test_step_refuses_past_the_capacity_and_reset_reaches_everything(monkeypatch):
    world, back = _back_end(monkeypatch, deskew=dict(), pose_graph=True, **EVERYTHING)
    for n in range(CAPACITY):
        back.step(_scan(world))
    with pytest.raises(capi.RsloHipError, match="capacity"):
        back.step(_scan(world))
    world.take()
    back.reset()
    assert world.take() == ["voxel_map.reset()", "surfels.reset()", "refined.reset()", "places.reset()", "keyframes.reset()",
                            "edges.reset()"]                   # the open-loop chain is its owner's
    assert back.n == 0 and back.refined_trajectory().shape == (0, 7)
    with pytest.raises(capi.RsloHipError):
        back.deskewed()
    back.step(_scan(world))
    assert world.take() == _expected(0, "network")


def test_the_runner_names_reach_the_back_end():
    """the runner's attributes of the back end's names read AND write the back end's (callers switch a stage off by
    assigning None), and its methods of those names are the back end's"""
    from rslo_amd import inference
    runner = inference.OdometryRunner.__new__(inference.OdometryRunner)
    runner.backend = back = backend.BackEnd(backend.PoseChain(4, "cpu"), capacity=4, device="cpu", pose_graph=_standin())
    assert runner.pose_graph is back.pose_graph and runner.voxel_map is None and runner.loop is None
    runner.pose_graph = None
    assert back.pose_graph is None
    with pytest.raises(capi.RsloHipError, match="pose_graph"):
        runner.close_loops(None, None)
    assert runner.refine_info.__self__ is back and runner.rebuild_map.__func__ is backend.BackEnd.rebuild_map


def test_the_runner_checks_before_it_builds(monkeypatch):
    """OdometryRunner hands its back-end arguments to backend.check in front of everything else, and turns the refusal
    into its own error type: no network is looked at, so nothing can have been built"""
    from rslo_amd import inference
    with pytest.raises(capi.RsloHipError, match="OdometryRunner: refine needs a voxel_map"):
        inference.OdometryRunner(None, device="cpu", refine=dict())
    with pytest.raises(capi.RsloHipError, match="OdometryRunner: local_map takes"):
        inference.OdometryRunner(None, device="cpu", voxel_map=MAP, local_map=dict(radius=30.0, evry=2))
