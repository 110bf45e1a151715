#!/usr/bin/env python3
"""One SHA-256 per (family, dtype, n) over every output and info of the ten GP tile families whose kernels run the SPD sweep of
csrc/spd_sweep.hpp, by calling it (logml_grad, predict, multi_target) or as a line-for-line copy (loo, loo_grad, predict_cov,
multi_target_grad, trend, trend_grad, trend_loo).

    python tools/family_bits.py                      # the library in the tree
    MATINV_LIB=/path/to/libmatinv_hip.so python tools/family_bits.py   # another build, to compare with

Two builds that run the same arithmetic in the same order print the same lines; a change to the sweep or to an epilogue that alters one
bit of one output shows up as another hash. The hashes are tied to one compiler and one GPU: this is a tool to compare two builds side by
side, not a golden file.

Inputs (seeded, the same for every family): batch 64; n in {1, 16, 17, 48, 79, 96} (1 x 1, full and ragged edges, the ragged fp64 5 x 5
one-wave forms, full 6 x 6); K = min(3, n) basis vectors, D = 17 targets and Q = 17 queries (more than 16: the group loops run twice),
P = 2 derivative matrices, c given. Three matrices of the 64 are rejected: one has a negative diagonal entry in the last tile, one holds
a NaN, one has a first pivot of zero. Every optional output is requested through the *_batched_host entry points. trend_loo has no
n = 1 form (K <= n - 1) and prints no line there."""
import hashlib
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
api = importlib.import_module("cuda-matrix-inversion_amd.api")

BATCH, NS, D, Q, P = 64, (1, 16, 17, 48, 79, 96), 17, 17, 2
NEG, NAN, ZERO = 5, 20, 41  # the rejected matrices


def inputs(n, dtype):
    rng = np.random.default_rng(1000 + n)
    k = min(3, n)
    r = rng.standard_normal((BATCH, n, n))
    b = r @ r.transpose(0, 2, 1) / n + np.eye(n)  # symmetric: row- and column-major agree
    c = rng.random((BATCH, n))
    c[[NEG, NAN, ZERO]] = 0.0
    b[NEG, n - 1, n - 1] = -1.0
    b[NAN, n // 2, 0] = b[NAN, 0, n // 2] = np.nan
    b[ZERO, 0, 0] = 0.0
    sym = rng.standard_normal((BATCH, P, n, n))
    h = rng.standard_normal((BATCH, k, n))
    h[:, 0] = 1.0
    e = rng.standard_normal((BATCH, Q, Q))
    x = dict(B=b, C=c, d=rng.standard_normal((BATCH, n)), Y=rng.standard_normal((BATCH, D, n)), A=rng.standard_normal((BATCH, Q, n)),
             dM=sym + sym.transpose(0, 1, 3, 2), H=h, G=rng.standard_normal((BATCH, Q, k)), e=2.0 + rng.random((BATCH, Q)),
             E=e @ e.transpose(0, 2, 1))
    return {key: np.ascontiguousarray(v.reshape(-1), dtype=dtype) for key, v in x.items()}, k


def families(n, x, k):
    yield "loo", api.loo_batched_host(n, x["B"], x["C"], x["d"])
    yield "logml_grad", api.logml_grad_batched_host(n, x["B"], x["C"], x["d"], x["dM"])
    yield "loo_grad", api.loo_grad_batched_host(n, x["B"], x["C"], x["d"], x["dM"])
    yield "predict", api.predict_batched_host(n, x["B"], x["C"], x["d"], x["A"], x["e"])
    yield "predict_cov", api.predict_cov_batched_host(n, x["B"], x["C"], x["d"], x["A"], x["E"])
    yield "multi_target", api.multi_target_batched_host(n, x["B"], x["C"], x["Y"], x["A"], ntarget=D, nquery=Q)
    yield "multi_target_grad", api.multi_target_grad_batched_host(n, x["B"], x["C"], x["Y"], x["dM"], ntarget=D, nparam=P)
    yield "trend", api.trend_batched_host(n, x["B"], x["C"], x["H"], x["Y"], x["A"], x["G"], x["e"], nbasis=k, ntarget=D, nquery=Q)
    yield "trend_grad", api.trend_grad_batched_host(n, x["B"], x["C"], x["H"], x["Y"], x["dM"], nbasis=k, ntarget=D, nparam=P)
    if k <= n - 1:  # the leave-one-out trend model needs n - 1 points to carry the basis: no n = 1 form
        yield "trend_loo", api.trend_loo_batched_host(n, x["B"], x["C"], x["H"], x["Y"], nbasis=k, ntarget=D)


def main():
    for dtype in (np.float64, np.float32):
        for n in NS:
            x, k = inputs(n, dtype)
            for name, outs in families(n, x, k):
                assert all(o is not None for o in outs), (name, "an output was not computed")
                info = outs[-1]
                assert all(info[m] != 0 for m in (NEG, NAN, ZERO)), (name, n, "a defective matrix was accepted")
                sha = hashlib.sha256()
                for o in outs:
                    sha.update(np.ascontiguousarray(o).tobytes())
                print(f"{name:18s} {np.dtype(dtype).name} n={n:<3d} rejected={int((info != 0).sum()):<2d} {sha.hexdigest()}", flush=True)


if __name__ == "__main__":
    main()
