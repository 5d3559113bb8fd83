"""Generates tests/golden/chamfer_build_ref.npz: the reference's own chamfer CPU path (compiled by oracle/build_ref.py) on the
cases of tests/test_oracle.py::test_chamfer_matches_reference_build_bitexact, inputs and outputs, so that the test has its
yardstick where the reference build is absent.  Run where the reference tree is:  python tests/golden/make_golden_chamfer_build.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import build_ref  # noqa: E402

CASES = [(1, 700, 500), (2, 333, 1025), (1, 1, 1)]


def cases(rng):
    """The test's inputs, drawn in the test's order: (a, c, gd) per case."""
    for (b, n, m) in CASES:
        a = rng.normal(size=(b, n, 3)).astype(np.float32) * 10
        c = rng.normal(size=(b, m, 3)).astype(np.float32) * 10
        c[:, : min(m, 5)] = a[:, : min(m, 5)][:, :, :]  # exact hits / ties
        gd = rng.normal(size=(b, n)).astype(np.float32)
        yield a, c, gd


def run(ref, a, c, gd):
    """cd.forward, then cd.backward with direction 1 only (zero gradient for direction 2)."""
    b, n, m = a.shape[0], a.shape[1], c.shape[1]
    ta, tc = torch.from_numpy(a), torch.from_numpy(c)
    d1, d2 = torch.zeros(b, n), torch.zeros(b, m)
    i1, i2 = torch.zeros(b, n, dtype=torch.int32), torch.zeros(b, m, dtype=torch.int32)
    ref.forward(ta, tc, d1, d2, i1, i2)
    g1, g2 = torch.zeros(b, n, 3), torch.zeros(b, m, 3)
    ref.backward(ta, tc, g1, g2, torch.from_numpy(gd), torch.zeros(b, m), i1, i2)
    return d1.numpy(), i1.numpy(), g1.numpy(), g2.numpy()


if __name__ == "__main__":
    build_ref.build()
    ref = build_ref.load()
    arrs = {}
    for k, (a, c, gd) in enumerate(cases(np.random.default_rng(5))):
        d1, i1, g1, g2 = run(ref, a, c, gd)
        arrs.update({"a%d" % k: a, "c%d" % k: c, "gd%d" % k: gd, "dist1_%d" % k: d1, "idx1_%d" % k: i1,
                     "gradxyz1_%d" % k: g1, "gradxyz2_%d" % k: g2})
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "chamfer_build_ref.npz")
    np.savez_compressed(out, **arrs)
    print("wrote", out, os.path.getsize(out))
