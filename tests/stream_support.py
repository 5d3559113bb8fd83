"""What the tests of the streaming back end share (a plain module, imported by name): array helpers, the seeded
disturbance of a pose, and the untrained network with a few scans of the synthetic drive that the runner tests stream."""
import numpy as np
import pytest
import torch


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def turned(q, rotvec):
    th = np.linalg.norm(rotvec)
    dq = np.concatenate([[np.cos(th / 2)], np.sin(th / 2) / th * rotvec])
    r = np.concatenate([[dq[0] * q[0] - dq[1:] @ q[1:]], dq[0] * q[1:] + q[0] * dq[1:] + np.cross(dq[1:], q[1:])])
    return r / np.linalg.norm(r)


def disturbed(true_pose, off, deg):
    """the true pose moved by `off` metres along (0.6, -0.5, 0.2) / norm and turned by `deg` degrees about
    (0.3, -0.4, 0.866) / norm"""
    d = np.array([0.6, -0.5, 0.2])
    axis = np.array([0.3, -0.4, 0.866])
    return np.concatenate([true_pose[:3] + off * d / np.linalg.norm(d),
                           turned(true_pose[3:], np.deg2rad(deg) * axis / np.linalg.norm(axis))])


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def cond_of(sums):
    """cond2 of the H whose upper triangle leads the 28 sums of the normal equations"""
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = sums[:21]
    return np.linalg.cond(H + np.triu(H, 1).T)


def network_and_scans(torch_seed, drive_seed, n_scans):
    """(the eval-mode network built under torch_seed, head BatchNorms calibrated on the first two scans; the first n_scans
    [P, 7] scans of the synthetic drive drive_seed on the device)"""
    from rslo_amd import synthetic, workload
    torch.manual_seed(torch_seed)
    net, _ = workload.build_network()
    net.eval()
    scans = [torch.from_numpy(synthetic.sequence_scan(i, seed=drive_seed)).cuda() for i in range(n_scans)]
    workload.calibrate_head_bn(net, (scans[0], scans[1]))
    return net, scans


def odom_fixture(torch_seed, drive_seed, n_scans):
    """the module-scoped fixture `odom` = network_and_scans(...): `odom = odom_fixture(21, 3, N_SCANS)` in the module"""
    @pytest.fixture(scope="module")
    def odom():
        return network_and_scans(torch_seed, drive_seed, n_scans)
    return odom


def stream(runner, scans):
    """feed the scans as a streaming caller does -> (relative [n, 7], trajectory [n, 7]) on the host"""
    runner.feed(scans)
    torch.cuda.synchronize()
    return runner.relative().cpu().numpy(), runner.trajectory().cpu().numpy()


def seed_poses(rel):
    """Where the refined chain will predict scans 1.. from an unrefined scan 0 (identity o rel[1] o ...), moved by a few
    centimetres: copies of the scans put there give the registration of an UNTRAINED network's poses something to find
    (its own scans do not overlap: the head's motion is metres per scan in changing directions)."""
    from rslo_amd import inference
    rows = rel.cpu().numpy().astype(np.float64)
    rows[0] = (0, 0, 0, 1, 0, 0, 0)
    seeds = inference.pose_chain_host(rows)
    seeds[:, :3] += np.array([0.05, -0.04, 0.02])
    return seeds
