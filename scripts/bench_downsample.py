"""capi.voxel_downsample on one full synthetic scan (rslo_amd.synthetic.scan(), ~131 k points): ms per call at each
voxel size, next to capi.estimate_normals of the same scan -- the two offline steps of the reference's store builder.

    python scripts/bench_downsample.py [--sizes 0.1 0.8] [--calls 20] [--warmup 5]
    rocprofv3 --kernel-trace --stats ... -- python scripts/bench_downsample.py          # kernel table, a run of its own

Device events around every call, median of --calls calls after --warmup calls; buffers and workspace preallocated and
sync=False, so a call is the kernels alone.  One JSON line.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, calls, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", type=float, default=[0.1, 0.8])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()

    import torch
    import rslo_amd  # noqa: F401
    from rslo_amd import capi, synthetic
    assert torch.cuda.is_available(), "needs a GPU"
    cloud = torch.from_numpy(synthetic.scan()).cuda()
    P = cloud.shape[0]
    res = {"points": P, "calls": args.calls, "warmup": args.warmup}

    nrm = torch.empty((P, 3), device="cuda")
    cnt = torch.empty((P,), dtype=torch.int32, device="cuda")
    nws = torch.empty((capi.lib().rslo_normals_ws_bytes(P),), dtype=torch.uint8, device="cuda")
    res["estimate_normals"] = timed(lambda: capi.estimate_normals(cloud, 0.6, 30, out=nrm, counts=cnt, ws=nws), args.calls,
                                    args.warmup)

    out = torch.empty((P, 6), device="cuda")
    vop = torch.empty((P,), dtype=torch.int32, device="cuda")
    npts = torch.empty((P,), dtype=torch.int32, device="cuda")
    counts = torch.empty((2,), dtype=torch.int32, device="cuda")
    ws = torch.empty((capi.lib().rslo_voxel_downsample_ws_bytes(P),), dtype=torch.uint8, device="cuda")
    res["ws_bytes"] = ws.numel()
    for size in args.sizes:
        r = timed(lambda: capi.voxel_downsample(cloud, nrm, size, out=out, index=vop, npts=npts, counts=counts, ws=ws,
                                                sync=False), args.calls, args.warmup)
        Q = int(counts[0])
        r.update(rows=Q, longest_run=int(npts[:Q].max()), runs_over_64=int((npts[:Q] > 64).sum()))
        res["voxel_downsample_%g" % size] = r
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
