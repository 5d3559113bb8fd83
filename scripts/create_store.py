"""A raw KITTI odometry directory -> the numpy store the training reader (rslo/data/kitti_dataset_hdf5.py) reads.

    python scripts/create_store.py --kitti ROOT --out DIR --seqs 00 01 ... [--hier 0.1 0.2 0.4 0.8]

ROOT holds sequences/<seq>/velodyne/*.bin, sequences/<seq>/calib.txt and (sequences 00-10) poses/<seq>.txt.  The
reference does this offline with Open3D and h5py (script/create_hdf5.py); here the normals and the voxel down-samples
run on the GPU (rslo_amd/rawstore.py).  One JSON line per sequence: the scan count and ms per scan split into read,
normals, down-sample and write.

--synthetic N first WRITES N synthetic scans (rslo_amd.synthetic.sequence_scan) with made-up poses and calibration
into ROOT for every sequence named, so the whole path can be tried and timed without the dataset.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_synthetic(kitti_root, seq, n):
    import numpy as np
    from rslo_amd import synthetic
    vel = os.path.join(kitti_root, "sequences", seq, "velodyne")
    os.makedirs(vel, exist_ok=True)
    os.makedirs(os.path.join(kitti_root, "poses"), exist_ok=True)
    for i in range(n):
        synthetic.sequence_scan(i, seed=int(seq))[:, :4].astype(np.float32).tofile(os.path.join(vel, "%06d.bin" % i))
    eye = np.eye(4)[:3]
    tr = np.array([[0.0, -1.0, 0.0, 0.0], [0.0, 0.0, -1.0, -0.08], [1.0, 0.0, 0.0, -0.27]])      # velodyne -> camera axes
    with open(os.path.join(kitti_root, "sequences", seq, "calib.txt"), "w") as f:
        for name, m in (("P0:", eye), ("P1:", eye), ("P2:", eye), ("P3:", eye), ("Tr:", tr)):
            f.write(name + " " + " ".join("%.9e" % v for v in m.reshape(-1)) + "\n")
    with open(os.path.join(kitti_root, "poses", seq + ".txt"), "w") as f:
        for i in range(n):
            pose = eye.copy()
            pose[2, 3] = float(i)          # one metre per scan along the camera's z
            f.write(" ".join("%.9e" % v for v in pose.reshape(-1)) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kitti", required=True, help="KITTI odometry root (sequences/, poses/)")
    ap.add_argument("--out", required=True, help="directory of the numpy store")
    ap.add_argument("--seqs", nargs="+", required=True, help="sequence names, e.g. 00 01")
    ap.add_argument("--hier", nargs="+", type=float, default=[0.1], help="voxel sizes of the down-samples (the reader reads 0.1)")
    ap.add_argument("--radius", type=float, default=0.6)
    ap.add_argument("--max-nn", type=int, default=30)
    ap.add_argument("--synthetic", type=int, default=0, metavar="N", help="write N synthetic scans per sequence into --kitti first")
    args = ap.parse_args()

    import rslo_amd  # noqa: F401
    from rslo_amd import rawstore
    for seq in args.seqs:
        if args.synthetic > 0:
            write_synthetic(args.kitti, seq, args.synthetic)
        paths, poses, calib = rawstore.read_kitti_sequence(args.kitti, seq)
        stats = rawstore.build_sequence(args.out, seq, paths, poses, calib, hier_sizes=args.hier, normal_radius=args.radius,
                                        normal_max_nn=args.max_nn)
        print(json.dumps({"seq": seq, "hier": args.hier, **{k: (round(v, 3) if isinstance(v, float) else v)
                                                            for k, v in stats.items()}}), flush=True)


if __name__ == "__main__":
    main()
