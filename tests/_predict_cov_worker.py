"""Reference, inputs, bounds and checks of the tests of the joint predictive covariance between a GP's query points
(tests/test_gpu_predict_cov.py and tests/test_predict_cov_cpu.py import them), and the worker of test_grid_stride_and_chunking: ONE process
under MATINV_TILE_GRID_MULT=1 and MATINV_BLOCKED_WS_MB=1 (the library reads each switch once per process), so that the tile kernels' stride
loop runs twice and the global launcher takes several chunks. Exits non-zero at the first failure and starts nothing after it; prints
`predict-cov-worker ok` at the end.

Reference: float64 numpy on the float64 image of exactly what the kernel reads, via _predict_worker.model (K = inv(M), alpha = K d). For
the Q queries of matrix k, with E the lower triangle of what the kernel is given, mirrored:
    mean[k, i] = a_ki^T alpha_k        cov[k, i, j] = E_k[i][j] - a_ki^T K_k a_kj

Inputs: B, c, d and a of the shared case of _predict_worker; per matrix E = a K a^T + R R^T / Q + diag U(0.1, 1) with R ~ N(0, 1) of size
Q x Q (Q = QMAX; smaller calls take the leading or a principal submatrix, which is again such a matrix), rounded to the working dtype
and its lower triangle mirrored. So the posterior covariance is a covariance (smallest eigenvalue >= 0.1 up to the rounding of E) and
the cancellation in E - a K a^T is real.

Bounds, first order and not fitted: the var bound of _predict_worker polarised. u = 2^-53 (fp64) or 2^-24 (fp32),
eps = (n + 4) * u * cond2(M)^2,
    |cov^[i][j] - cov[i][j]| <= eps * ||K||_2 * ||a_i||_2 ||a_j||_2 + 2 n * u * sum_pq |a_ip K_pq a_jq| + u * (|E_ij| + |cov_ij|)
(the backward error of the inverse, ||dK||_2 <= eps ||K||_2, then Cauchy-Schwarz with a_i and a_j; the rounding of the two n-term product
sums K a_j and a_i . (K a_j) in any order; the final subtraction). The mean bound is that of _predict_worker, unchanged.
tests/test_predict_cov_cpu.py confirms that a float32 numpy evaluation of the same formulas stays inside the fp32 bounds at every size, Q
and input the GPU tests use.
"""
import functools
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import _loo_worker as L  # noqa: E402
import _predict_worker as P  # noqa: E402
from conftest import as_mats  # noqa: E402

U = P.U
break_three = P.break_three
model = P.model
first_queries = P.first_queries
TILE_SIZES = P.TILE_SIZES
GLOBAL_SIZES = P.GLOBAL_SIZES
QS = P.QS
QMAX = P.QMAX
batch_of = P.batch_of


def prior(mdl, As, n, nquery, dt, seed):
    """Es: per matrix E = a K a^T + R R^T / Q + diag U(0.1, 1), rounded to dt, the lower triangle mirrored; packed column-major"""
    rng = np.random.default_rng(seed)
    a = np.asarray(As, dtype=np.float64).reshape(-1, nquery, n)
    batch = a.shape[0]
    R = rng.standard_normal((batch, nquery, nquery))
    E = (a @ mdl["K"]) @ a.transpose(0, 2, 1) + R @ R.transpose(0, 2, 1) / nquery
    idx = np.arange(nquery)
    E[:, idx, idx] += rng.uniform(0.1, 1.0, (batch, nquery))
    E = E.astype(dt)
    E = np.tril(E) + np.tril(E, -1).transpose(0, 2, 1)
    return np.ascontiguousarray(E.transpose(0, 2, 1)).reshape(-1)  # element (i, j) at j * Q + i


@functools.lru_cache(maxsize=None)
def case(n, dtname, with_c):
    """the shared case of _predict_worker of size n with the prior covariance of its QMAX queries in place of their prior variances:
    (B, c, d, model, As, Es). Computed once; nobody writes into it"""
    dt = np.dtype(dtname).type
    B, c, d, mdl, As, _ = P.case(n, dtname, with_c)
    Es = prior(mdl, As, n, QMAX, dt, seed=9700 + 7 * n + (1 if with_c else 0))
    Es.setflags(write=False)
    return B, c, d, mdl, As, Es


def pick(As, Es, n, sel, total=QMAX):
    """the queries `sel` (a slice or a list of indices) of the `total` queries of every matrix, packed, with E's principal submatrix"""
    a3 = As.reshape(-1, total, n)[:, sel]
    a = np.ascontiguousarray(a3).reshape(-1)
    if Es is None:
        return a, None
    e = Es.reshape(-1, total, total)[:, sel][:, :, sel]
    return a, np.ascontiguousarray(e).reshape(-1)


def leading(As, Es, n, nquery, total=QMAX):
    return pick(As, Es, n, slice(0, nquery), total)


def e_matrix(Es, batch, nquery):
    """float64 E[k, i, j] as the kernel reads it: the lower triangle of the packed column-major input, mirrored"""
    if Es is None:
        return np.zeros((batch, nquery, nquery))
    E = np.asarray(Es, dtype=np.float64).reshape(batch, nquery, nquery).transpose(0, 2, 1)
    return np.tril(E) + np.tril(E, -1).transpose(0, 2, 1)


def unpack(cov, nquery):
    """cov[k, i, j] of the packed column-major output"""
    return np.asarray(cov).reshape(-1, nquery, nquery).transpose(0, 2, 1)


def cov_reference(mdl, As, Es, n, nquery, idx=None):
    """mean, cov and the terms of the bounds for nquery queries per matrix of the model (float64)"""
    a = np.asarray(As, dtype=np.float64).reshape(-1, nquery, n)
    E = e_matrix(Es, a.shape[0], nquery)
    if idx is not None:
        a, E = a[idx], E[idx]
    K = mdl["K"]
    ref = dict(mdl, a=a, E=E, cov=E - (a @ K) @ a.transpose(0, 2, 1),
               covmag=(np.abs(a) @ np.abs(K)) @ np.abs(a).transpose(0, 2, 1))
    if mdl["alpha"] is not None:
        ref["mean"] = np.einsum("kqi,ki->kq", a, mdl["alpha"])
        ref["meanmag"] = np.einsum("kqi,ki->kq", np.abs(a), np.abs(mdl["alpha"]))
    return ref


def bounds(ref, n, u):
    """(b_mean[k, i] or None, b_cov[k, i, j]) of the module docstring"""
    eps = (n + 4) * u * ref["cond"] ** 2
    an = np.linalg.norm(ref["a"], axis=2)
    b_cov = (eps * ref["knorm"])[:, None, None] * an[:, :, None] * an[:, None, :] + 2 * n * u * ref["covmag"] \
        + u * (np.abs(ref["E"]) + np.abs(ref["cov"]))
    b_mean = None
    if "mean" in ref:
        b_mean = eps[:, None] * np.linalg.norm(ref["alpha"], axis=1)[:, None] * an + n * u * ref["meanmag"]
    return b_mean, b_cov


def ratios(mean, cov, ref, n, u, idx=None):
    """err / bound of every given output (None: not requested) of the matrices idx"""
    b_mean, b_cov = bounds(ref, n, u)
    nquery = ref["a"].shape[1]
    sel = slice(None) if idx is None else idx
    out = {}
    if mean is not None:
        out["mean"] = np.abs(np.asarray(mean, dtype=np.float64).reshape(-1, nquery)[sel] - ref["mean"]) / b_mean
    if cov is not None:
        out["cov"] = np.abs(unpack(cov, nquery).astype(np.float64)[sel] - ref["cov"]) / b_cov
    return out


def check(mean, cov, ref, n, u, idx=None, what="", factor=1.0):
    """every given output within factor * bound; prints err / bound first"""
    rs = ratios(mean, cov, ref, n, u, idx)
    print(f"  {what} n={n} Q={ref['a'].shape[1]} cond={ref['cond'].max():.2f} err/bound: " + " ".join(f"{k}={v.max():.3f}" for k, v in rs.items()))
    for k, v in rs.items():
        assert np.isfinite(v).all() and (v <= factor).all(), (what, n, k, float(np.nanmax(v)))


def assert_symmetric(cov, nquery, what=""):
    """bitwise: the upper triangle is a copy of the lower one (NaN equal to NaN)"""
    c = unpack(cov, nquery)
    assert np.array_equal(c, c.transpose(0, 2, 1), equal_nan=True), (what, "cov is not bitwise symmetric")


def float32_evaluation(B, c, d, As, Es, n, nquery):
    """the reference formulas evaluated in float32 numpy on the float32 inputs: what any fp32 implementation of them may expect"""
    f = np.float32
    m = as_mats(B, n).astype(f)
    M = np.tril(m) + np.tril(m, -1).transpose(0, 2, 1)
    if c is not None:
        idx = np.arange(n)
        M[:, idx, idx] = M[:, idx, idx] + np.asarray(c, dtype=f).reshape(-1, n)
    K = np.linalg.inv(M)
    assert K.dtype == f
    a = np.asarray(As, dtype=f).reshape(-1, nquery, n)
    alpha = np.einsum("kij,kj->ki", K, np.asarray(d, dtype=f).reshape(-1, n))
    mean = np.einsum("kqi,ki->kq", a, alpha)
    E = e_matrix(Es, a.shape[0], nquery).astype(f)  # exact: Es is float32
    cov = E - np.einsum("kip,kjp->kij", a, np.einsum("kpq,kjq->kjp", K, a))
    assert mean.dtype == f and cov.dtype == f
    return mean, np.ascontiguousarray(cov.transpose(0, 2, 1)).reshape(-1)


def check_with_rejects(mean, cov, info, B, c, d, As, Es, n, nquery, dt, want_info, what=""):
    """info as expected, all outputs NaN exactly at the not-SPD matrices, finite and within the bounds elsewhere; cov bitwise symmetric"""
    batch = info.size
    bad = sorted(want_info)
    ok = np.array([k for k in range(batch) if k not in want_info])
    expect = np.zeros(batch, dtype=np.int64)
    for k, v in want_info.items():
        expect[k] = v
    assert np.array_equal(info, expect), (what, n, info[bad], [want_info[k] for k in bad], np.flatnonzero(info != expect)[:10])
    for o in (mean.reshape(batch, nquery), cov.reshape(batch, nquery * nquery)):
        assert np.isnan(o[bad]).all(), (what, n)
        assert np.isfinite(o[ok]).all(), (what, n)
    assert_symmetric(cov, nquery, what)
    ref = cov_reference(model(B, c, d, n, idx=ok), As, Es, n, nquery, idx=ok)
    check(mean, cov, ref, n, U[np.dtype(dt)], idx=ok, what=what)


def run(api, torch, n, batch, nquery, dt, with_c, rejects_at=None):
    B, c, d = L.inputs(n, batch, dt, with_c)
    mdl = model(B, c, None, n)  # of the healthy matrices
    As, _ = P.queries(mdl, n, batch, nquery, dt, seed=9500 + n)
    Es = prior(mdl, As, n, nquery, dt, seed=9600 + n)
    want_info = break_three(B, c, n, rejects_at) if rejects_at else {}
    dev = lambda x: None if x is None else torch.from_numpy(x).cuda()  # noqa: E731
    info = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
    mean, cov = api.predict_cov_batched(n, dev(B), dev(c), dev(d), dev(As), dev(Es), info=info)
    torch.cuda.synchronize()
    what = f"{api.predict_cov_kernel_name(dt, n)} batch={batch}"
    check_with_rejects(mean.cpu().numpy(), cov.cpu().numpy(), info.cpu().numpy(), B, c, d, As, Es, n, nquery, dt, want_info, what)


def main():
    import torch
    api = importlib.import_module("cuda-matrix-inversion_amd.api")
    assert os.environ.get("MATINV_TILE_GRID_MULT") == "1" and os.environ.get("MATINV_BLOCKED_WS_MB") == "1"
    # 4000 matrices on a grid of 256 * 12 = 3072 workgroups (launch_predict_cov_tile takes predict_tile_grid, i.e. tile_grid(batch, 12)):
    # the stride loop runs twice; the rejects sit in the second round.
    run(api, torch, 33, 4000, 3, np.float64, True, rejects_at=(3073, 3500, 3999))
    run(api, torch, 33, 4000, 3, np.float32, False, rejects_at=(3100, 3600, 3998))
    # 20 working copies of 130 * (130 + 17) * 8 = 152 880 bytes under a cap of 1 MiB: six to a chunk, four chunks, three of them with a
    # non-zero `first`
    run(api, torch, 130, 20, 17, np.float64, True)
    run(api, torch, 130, 20, 17, np.float64, False, rejects_at=(7, 13, 19))
    print("predict-cov-worker ok")


if __name__ == "__main__":
    main()
