"""Reference, inputs, bounds and checks of the GP prediction tests (tests/test_gpu_predict.py and tests/test_predict_cpu.py import them),
and the worker of test_grid_stride_and_chunking: ONE process under MATINV_TILE_GRID_MULT=1 and MATINV_BLOCKED_WS_MB=1 (the library reads
each switch once per process), so that the tile kernels' stride loop runs twice and the global launcher takes several chunks. Exits
non-zero at the first failure and starts nothing after it; prints `predict-worker ok` at the end.

Reference: float64 numpy on the float64 image of exactly what the kernel reads (_logml_grad_worker.image: the lower triangle of B mirrored,
the diagonal B_ii + c_i rounded in the working precision). K = inv(M), alpha = K d, and for query j of matrix k
    mean[k, j] = a_kj^T alpha_k        var[k, j] = e_kj - a_kj^T K_k a_kj

Inputs: B, c, d of _loo_worker.inputs; a ~ N(0, 1); e = a^T K a + U(0.1, 1), rounded to the working dtype, so that var is of order 1 and
the cancellation in e - a^T K a is real.

Bounds, first order and not fitted: u = 2^-53 (fp64) or 2^-24 (fp32), eps = (n + 4) * u * cond2(M)^2 as in _logml_grad_worker,
    |mean^ - mean| <= eps * ||alpha||_2 * ||a||_2 + n * u * sum_i |a_i alpha_i|
    |var^ - var|   <= eps * ||K||_2 * ||a||_2^2 + 2 n * u * sum_ij |a_i K_ij a_j| + u * (|e| + |var|)
The first terms are the backward error of the inverse propagated as there (||d alpha|| <= eps ||alpha||, ||dK||_2 <= eps ||K||_2, then
Cauchy-Schwarz with a); the second terms are the rounding of an n-term product sum in any order (n u times the sum of the magnitudes),
done twice for the quadratic form (K a, then a . (K a)); the last term is the final subtraction. tests/test_predict_cpu.py confirms that
a float32 numpy evaluation of the same formulas stays inside the fp32 bounds at every size, Q and input the GPU tests use.
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
import _logml_grad_worker as G  # noqa: E402
import _loo_worker as L  # noqa: E402
from conftest import as_mats  # noqa: E402

U = L.U
break_three = L.break_three

TILE_SIZES = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 95, 96]
GLOBAL_SIZES = [97, 130, 200]
QS = (1, 16, 17, 33)  # a partial group, an exact group, a group plus one, two groups plus one
QMAX = max(QS)


def batch_of(n):
    return 13 if n <= 64 else (5 if n < 1024 else 2)


def model(B, c, d, n, idx=None):
    """what depends on the matrices alone, in float64: M as the kernel reads it, K, alpha, cond2(M), ||K||_2. idx: the matrices to
    compute (the others may be not SPD); d may be None (no alpha)"""
    M = G.image(B, c, n)
    dd = None if d is None else np.asarray(d, dtype=np.float64).reshape(-1, n)
    if idx is not None:
        M = M[idx]
        dd = None if dd is None else dd[idx]
    K = np.linalg.inv(M)
    sv = np.linalg.svd(M, compute_uv=False)  # descending: cond2 = s_max / s_min, ||K||_2 = 1 / s_min
    return {"M": M, "K": K, "alpha": None if dd is None else np.einsum("kij,kj->ki", K, dd), "cond": sv[:, 0] / sv[:, -1],
            "knorm": 1.0 / sv[:, -1]}


def predict_reference(mdl, As, Es, n, nquery, idx=None):
    """mean, var and the terms of the bounds for nquery queries per matrix of the model (float64)"""
    a = np.asarray(As, dtype=np.float64).reshape(-1, nquery, n)
    e = np.zeros(a.shape[:2]) if Es is None else np.asarray(Es, dtype=np.float64).reshape(-1, nquery)
    if idx is not None:
        a, e = a[idx], e[idx]
    Ka = np.einsum("kij,kqj->kqi", mdl["K"], a)
    ref = dict(mdl, a=a, e=e, var=e - np.einsum("kqi,kqi->kq", a, Ka),
               quadmag=np.einsum("kqi,kij,kqj->kq", np.abs(a), np.abs(mdl["K"]), np.abs(a)))
    if mdl["alpha"] is not None:
        ref["mean"] = np.einsum("kqi,ki->kq", a, mdl["alpha"])
        ref["meanmag"] = np.einsum("kqi,ki->kq", np.abs(a), np.abs(mdl["alpha"]))
    return ref


def queries(mdl, n, batch, nquery, dt, seed):
    """(As, Es): batch * nquery cross-covariance vectors a ~ N(0, 1) and prior variances e = a^T K a + U(0.1, 1), both in dt"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((batch, nquery, n)).astype(dt)
    a64 = a.astype(np.float64)
    quad = np.einsum("kqi,kij,kqj->kq", a64, mdl["K"], a64)
    e = (quad + rng.uniform(0.1, 1.0, (batch, nquery))).astype(dt)
    return a.reshape(-1), e.reshape(-1)


@functools.lru_cache(maxsize=None)
def case(n, dtname, with_c):
    """the shared case of size n: (B, c, d, model, As, Es) with QMAX queries per matrix. Computed once; nobody writes into it"""
    dt = np.dtype(dtname).type
    batch = batch_of(n)
    B, c, d = L.inputs(n, batch, dt, with_c)
    mdl = model(B, c, d, n)
    As, Es = queries(mdl, n, batch, QMAX, dt, seed=9000 + 7 * n + (1 if with_c else 0))
    for x in (B, c, d, As, Es):
        if x is not None:
            x.setflags(write=False)
    return B, c, d, mdl, As, Es


def first_queries(As, Es, n, nquery, total=QMAX):
    """the first nquery of the `total` queries of every matrix, packed"""
    a = np.ascontiguousarray(As.reshape(-1, total, n)[:, :nquery]).reshape(-1)
    e = None if Es is None else np.ascontiguousarray(Es.reshape(-1, total)[:, :nquery]).reshape(-1)
    return a, e


def bounds(ref, n, u):
    """(b_mean[k, j] or None, b_var[k, j]) of the module docstring"""
    eps = ((n + 4) * u * ref["cond"] ** 2)[:, None]
    an = np.linalg.norm(ref["a"], axis=2)
    b_var = eps * ref["knorm"][:, None] * an ** 2 + 2 * n * u * ref["quadmag"] + u * (np.abs(ref["e"]) + np.abs(ref["var"]))
    b_mean = None
    if "mean" in ref:
        b_mean = eps * np.linalg.norm(ref["alpha"], axis=1)[:, None] * an + n * u * ref["meanmag"]
    return b_mean, b_var


def ratios(mean, var, ref, n, u, idx=None):
    """err / bound of every given output (None: not requested) of the matrices idx"""
    b_mean, b_var = bounds(ref, n, u)
    nquery = ref["a"].shape[1]
    sel = slice(None) if idx is None else idx
    out = {}
    if mean is not None:
        out["mean"] = np.abs(np.asarray(mean, dtype=np.float64).reshape(-1, nquery)[sel] - ref["mean"]) / b_mean
    if var is not None:
        out["var"] = np.abs(np.asarray(var, dtype=np.float64).reshape(-1, nquery)[sel] - ref["var"]) / b_var
    return out


def check(mean, var, ref, n, u, idx=None, what="", factor=1.0):
    """every given output within factor * bound; prints err / bound first"""
    rs = ratios(mean, var, ref, n, u, idx)
    print(f"  {what} n={n} Q={ref['a'].shape[1]} cond={ref['cond'].max():.2f} err/bound: " + " ".join(f"{k}={v.max():.3f}" for k, v in rs.items()))
    for k, v in rs.items():
        assert np.isfinite(v).all() and (v <= factor).all(), (what, n, k, float(np.nanmax(v)))


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
    var = np.asarray(Es, dtype=f).reshape(-1, nquery) - np.einsum("kqi,kqi->kq", a, np.einsum("kij,kqj->kqi", K, a))
    assert mean.dtype == f and var.dtype == f
    return mean, var


def check_with_rejects(mean, var, info, B, c, d, As, Es, n, nquery, dt, want_info, what=""):
    """info as expected, both outputs NaN exactly at the not-SPD matrices, finite and within the bounds elsewhere"""
    batch = info.size
    bad = sorted(want_info)
    ok = np.array([k for k in range(batch) if k not in want_info])
    expect = np.zeros(batch, dtype=np.int64)
    for k, v in want_info.items():
        expect[k] = v
    assert np.array_equal(info, expect), (what, n, info[bad], [want_info[k] for k in bad], np.flatnonzero(info != expect)[:10])
    for o in (mean.reshape(batch, nquery), var.reshape(batch, nquery)):
        assert np.isnan(o[bad]).all(), (what, n)
        assert np.isfinite(o[ok]).all(), (what, n)
    ref = predict_reference(model(B, c, d, n, idx=ok), As, Es, n, nquery, idx=ok)
    check(mean, var, ref, n, U[np.dtype(dt)], idx=ok, what=what)


def run(api, torch, n, batch, nquery, dt, with_c, rejects_at=None):
    B, c, d = L.inputs(n, batch, dt, with_c)
    As, Es = queries(model(B, c, None, n), n, batch, nquery, dt, seed=9500 + n)  # of the healthy matrices: e - a^T K a is of order 1
    want_info = break_three(B, c, n, rejects_at) if rejects_at else {}
    dev = lambda x: None if x is None else torch.from_numpy(x).cuda()  # noqa: E731
    info = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
    mean, var = api.predict_batched(n, dev(B), dev(c), dev(d), dev(As), dev(Es), info=info)
    torch.cuda.synchronize()
    what = f"{api.predict_kernel_name(dt, n)} batch={batch}"
    check_with_rejects(mean.cpu().numpy(), var.cpu().numpy(), info.cpu().numpy(), B, c, d, As, Es, n, nquery, dt, want_info, what)


def main():
    import torch
    api = importlib.import_module("cuda-matrix-inversion_amd.api")
    assert os.environ.get("MATINV_TILE_GRID_MULT") == "1" and os.environ.get("MATINV_BLOCKED_WS_MB") == "1"
    # 4000 matrices on a grid of 256 * 12 = 3072 workgroups: the stride loop runs twice; the rejects sit in the second round.
    run(api, torch, 33, 4000, 3, np.float64, True, rejects_at=(3073, 3500, 3999))
    run(api, torch, 33, 4000, 3, np.float32, False, rejects_at=(3100, 3600, 3998))
    # 20 working copies of 135 200 bytes under a cap of 1 MiB: three chunks, two of them with a non-zero `first`
    run(api, torch, 130, 20, 17, np.float64, True)
    run(api, torch, 130, 20, 17, np.float64, False, rejects_at=(7, 13, 19))
    print("predict-worker ok")


if __name__ == "__main__":
    main()
