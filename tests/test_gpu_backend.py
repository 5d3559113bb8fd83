"""The streaming back end as its own class (rslo_amd.backend) on the GPU: a BackEnd stepped by hand over a PoseChain that
is fed the runner's own odometry rows leaves every bit an OdometryRunner with the same options leaves; and a refused
back-end option leaves nothing of a runner behind.  Four scans reach every branch of step(): n = 0, 1, 2, 3 with
every=2 for the prunes and the carve, and the constant-velocity de-skewing that starts at n = 2."""
import threading

import pytest
import torch
from stream_support import network_and_scans, same_bits
from test_gpu_loops import LOOP
from test_gpu_map_frames import same_device_maps as same_voxel_maps
from test_gpu_surfel_prune import MAP_ARGS, SURF_ARGS
from test_gpu_surfels import same_device_maps as same_surfel_maps

pytestmark = pytest.mark.gpu

CAPACITY = 16


@pytest.fixture(scope="module")
def odom():
    return network_and_scans(21, 3, 4)


def _everything():
    """every back-end option on, over fresh collaborators"""
    from rslo_amd import loops, places
    from rslo_amd.mapping import VoxelMap
    from rslo_amd.surfels import SurfelMap
    return dict(voxel_map=VoxelMap(**MAP_ARGS), refine=dict(iters=1), surfels=SurfelMap(**SURF_ARGS),
                surfel_refine=dict(iters=1), local_map=dict(radius=30.0, every=2, surfels=True), carve=dict(every=2),
                deskew=dict(motion="refined"), places=places.PlaceDB(capacity=CAPACITY), loop=LOOP,
                keyframes=loops.KeyframeStore(capacity=CAPACITY, K=1024), verify=dict())


def _assert_same_results(runner, chain, back, n, label):
    torch.cuda.synchronize()
    assert back.n == n and same_bits(chain.rel[:n], runner.relative()) and same_bits(chain.traj[:n], runner.trajectory()), label
    for name in ("refined_trajectory", "refine_info", "surfel_refine_info", "deskew_info", "loop_candidates", "loop_checks"):
        got, want = getattr(back, name)(), getattr(runner, name)()
        assert got.shape[0] == n and same_bits(got, want), "%s: %s" % (label, name)
    for got, want in zip(back.loop_edges(), runner.loop_edges()):
        assert same_bits(got, want), "%s: loop_edges" % label
    assert same_bits(back.deskewed(), runner.deskewed()), label
    assert (back.range_image.numpy() == runner.backend.range_image.numpy()).all(), label
    vmap, smap = runner.voxel_map, runner.surfels
    print("%s: voxel map %s %s %s; surfel map %s %s; edges %s" % (label, vmap.stats(), vmap.prune_stats(), vmap.carve_stats(),
                                                                 smap.stats(), smap.prune_stats(), runner.loop_edges()[3].tolist()))
    assert same_voxel_maps(back.voxel_map, vmap), label                      # stats() and the sorted points()
    assert back.voxel_map.prune_stats() == vmap.prune_stats() and back.voxel_map.carve_stats() == vmap.carve_stats(), label
    assert same_surfel_maps(back.surfels, smap), label                      # stats() and the sorted cells()
    assert back.surfels.prune_stats() == smap.prune_stats(), label


def test_a_back_end_alone_equals_the_runner(odom):
    from rslo_amd import backend, inference
    net, scans = odom
    runner = inference.OdometryRunner(net, capacity=CAPACITY, **_everything())
    try:
        chain = backend.PoseChain(CAPACITY, "cuda")
        back = backend.BackEnd(chain, capacity=CAPACITY, device="cuda", **_everything())
        assert back.voxel_map is not runner.voxel_map and back.local_map == runner.local_map and back.verify == runner.verify
        for label, part in (("four scans", scans), ("two scans after reset()", scans[:2])):
            runner.feed(part)
            rel = runner.relative()
            for i, scan in enumerate(part):         # what the head graph does, then what run() does behind it
                chain.push(rel[i, :3], rel[i, 3:])
                back.step(scan)
            _assert_same_results(runner, chain, back, len(part), label)
            if len(part) == 4:                      # every branch was taken: both prunes and the carve twice, a motion twice
                assert runner.voxel_map.prune_stats()["n_prunes"] == 2 == runner.surfels.prune_stats()["n_prunes"]
                assert runner.voxel_map.carve_stats()["n_carves"] == 2
                status = runner.deskew_info()[:, 7].tolist()
                assert status[:2] == [1.0, 1.0] and 1.0 not in status[2:]        # no motion below n = 2, one from there on
            runner.reset()
            chain.reset()
            back.reset()
            assert back.n == 0 and back.voxel_map.stats()["n_scans"] == 0 == back.surfels.stats()["n_scans"]
    finally:
        runner.close()


@pytest.mark.parametrize("case", ["refine without voxel_map", "local_map without radius", "local_map key", "surfel min_count"])
def test_a_refused_option_leaves_nothing_behind(odom, case):
    """The encoder runner starts a helper thread and allocates its plan arenas; nobody can close() an object whose
    constructor raised, so every refusal has to come before it is built."""
    from rslo_amd import capi, inference
    from rslo_amd.surfels import SurfelMap
    net, _ = odom
    options = {"refine without voxel_map": lambda: dict(refine=dict()),
               "local_map without radius": lambda: dict(local_map=dict(every=2)),
               "local_map key": lambda: dict(local_map=dict(radius=30.0, evry=2)),
               "surfel min_count": lambda: dict(surfels=SurfelMap(0.4, 1024),
                                                local_map=dict(radius=30.0, surfels=dict(min_count=0)))}[case]()
    before = threading.active_count()
    with pytest.raises(capi.RsloHipError):
        inference.OdometryRunner(net, **options)
    assert threading.active_count() == before
