"""Reference, inputs, bounds and checks of the multi-output GP tests (tests/test_gpu_multi_target.py and tests/test_multi_target_cpu.py
import them), and the worker of test_grid_stride_and_chunking: ONE process under MATINV_TILE_GRID_MULT=1 and MATINV_BLOCKED_WS_MB=1 (the
library reads each switch once per process), so that the tile kernels' stride loop runs twice and the global launcher takes several chunks.
Exits non-zero at the first failure and starts nothing after it; prints `multi-target-worker ok` at the end.

Reference: float64 numpy on the float64 image of exactly what the kernel reads (_logml_grad_worker.image: the lower triangle of B mirrored,
the diagonal B_ii + c_i rounded in the working precision). K = inv(M), and for target t and query j of matrix k
    alpha[k, t] = K_k y_kt      quad[k, t] = y_kt^T alpha[k, t]      logdet[k] = log det M_k
    logml[k, t] = -(quad[k, t] + logdet[k] + n log 2 pi) / 2         mean[k, t, j] = a_kj^T alpha[k, t]
logdet is 2 sum log of the diagonal of a Cholesky factor taken in longdouble for n <= 96 (_whiten_worker.logdet_longdouble says why: at
n = 1 the float64 factor's own rounding is the whole bound), of the float64 factor beyond.

Inputs: B and c of _loo_worker.inputs; y ~ N(0, 1); a ~ N(0, 1) as in _predict_worker.queries.

Bounds, first order and not fitted: u = 2^-53 (fp64) or 2^-24 (fp32), eps = (n + 4) * u * cond2(M)^2 as in _logml_grad_worker.
    alpha   |alpha^_i - alpha_i| <= eps * ||alpha_t||_2                                    (_logml_grad_worker: the backward error of the
            inverse, u n cond, propagated through ||y|| <= ||M|| ||alpha||)
    quad    |quad^ - quad| <= eps * ||K||_2 * ||y||_2^2 + 2 n u sum_ij |y_i K_ij y_j| + u |quad|
            (_predict_worker's var bound with e = 0: var = -quad there. The first term is ||dK||_2 <= eps ||K||_2 with Cauchy-Schwarz,
            the second the rounding of the two n-term product sums K y and y . (K y) in any order, the third the last rounding)
    logdet  |logdet^ - logdet| <= n^2 u cond2(M) + n u max(1, |logdet|)                    (the bound() of tests/test_gpu_logdet.py on the
            same PivotProduct; the global form folds the roots L_ii and doubles the logarithm, 2 n u more, where n >= 97 and the first
            term is n cond / 2 times that: _whiten_worker bound (5))
    logml   |logml^ - logml| <= (b_quad + b_logdet) / 2 + u (|s| + 2 n log 2 pi + |s + n log 2 pi|) / 2,   s = quad + logdet
            (half of both, and the roundings of its own terms: fl(quad + logdet), the product with the rounded constant and the last
            addition; the factor -1/2 is exact. _whiten_worker's logpdf bound)
    mean    |mean^ - mean| <= eps * ||alpha_t||_2 * ||a_j||_2 + n u sum_i |a_ji alpha_ti|  (_predict_worker's mean bound with alpha_t)
The tile forms need no counted constant beyond these: alpha is the negated T = W y, n-term sums inside MFMAs on the W whose error eps
bounds; quad and mean are n-term sums of products with that T in registers, the terms the bounds name. Nothing here is fitted to what the
kernels return; tests/test_multi_target_cpu.py confirms that a float32 numpy evaluation of the same formulas stays inside the fp32 bounds
at every size and (D, Q) the GPU tests use.
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
import _predict_worker as P  # noqa: E402
import _whiten_worker as W  # noqa: E402
from conftest import as_mats  # noqa: E402

U = L.U
break_three = L.break_three
TILE_SIZES, GLOBAL_SIZES, batch_of = P.TILE_SIZES, P.GLOBAL_SIZES, P.batch_of
DQ = ((1, 1), (16, 17), (17, 16), (33, 33))  # a partial group, an exact group against a group plus one and back, two groups plus one
DQ_1024 = (17, 16)                           # n = 1024 runs once per dtype
DMAX = QMAX = 33
OUTPUTS = ("alpha", "quad", "logdet", "logml", "mean")
LOG2PI = W.LOG2PI


def model(B, c, n, idx=None):
    """what depends on the matrices alone: M as the kernel reads it, K, cond2(M), ||K||_2 (float64), logdet (longdouble). idx: the matrices
    to compute (the others may be not SPD)"""
    M = G.image(B, c, n)
    if idx is not None:
        M = M[idx]
    sv = np.linalg.svd(M, compute_uv=False)  # descending: cond2 = s_max / s_min, ||K||_2 = 1 / s_min
    return {"M": M, "K": np.linalg.inv(M), "cond": sv[:, 0] / sv[:, -1], "knorm": 1.0 / sv[:, -1],
            "logdet": W.logdet_longdouble(M, np.linalg.cholesky(M))}


def reference(mdl, Ys, As, n, D, Q, idx=None):
    """the five outputs and the terms of the bounds for D targets and Q queries per matrix of the model; Ys / As None: without them"""
    ref = dict(mdl)
    if Ys is None:
        return ref
    y = np.asarray(Ys, dtype=np.float64).reshape(-1, D, n)
    if idx is not None:
        y = y[idx]
    alpha = np.einsum("kij,ktj->kti", mdl["K"], y)
    quad = np.einsum("kti,kti->kt", y, alpha)
    ref.update(y=y, alpha=alpha, quad=quad, quadmag=np.einsum("kti,kij,ktj->kt", np.abs(y), np.abs(mdl["K"]), np.abs(y)),
               logml=-(quad + mdl["logdet"][:, None] + n * np.log(2 * np.longdouble(np.pi))) / 2)
    if As is not None and Q:
        a = np.asarray(As, dtype=np.float64).reshape(-1, Q, n)
        if idx is not None:
            a = a[idx]
        ref.update(a=a, mean=np.einsum("kqi,kti->ktq", a, alpha), meanmag=np.einsum("kqi,kti->ktq", np.abs(a), np.abs(alpha)))
    return ref


def targets(n, batch, D, dt, seed):
    return np.random.default_rng(seed).standard_normal((batch, D, n)).astype(dt).reshape(-1)


@functools.lru_cache(maxsize=None)
def case(n, dtname, with_c):
    """the shared case of size n: (B, c, Ys, As, reference) with DMAX targets and QMAX queries per matrix. Computed once; nobody writes
    into it; `take` slices the reference, `first` the vectors"""
    dt = np.dtype(dtname).type
    batch = batch_of(n)
    B, c, _ = L.inputs(n, batch, dt, with_c)
    mdl = model(B, c, n)
    Ys = targets(n, batch, DMAX, dt, seed=7000 + 11 * n + (1 if with_c else 0))
    As, _ = P.queries(mdl, n, batch, QMAX, dt, seed=9000 + 7 * n + (1 if with_c else 0))
    for x in (B, c, Ys, As):
        if x is not None:
            x.setflags(write=False)
    return B, c, Ys, As, reference(mdl, Ys, As, n, DMAX, QMAX)


def first(V, n, total, sel):
    """the vectors `sel` (a count, a slice or a list) of the `total` vectors of every matrix, packed"""
    sel = slice(0, sel) if isinstance(sel, int) else sel
    return np.ascontiguousarray(V.reshape(-1, total, n)[:, sel]).reshape(-1)


def take(ref, tsel, qsel):
    """the reference of the targets tsel and the queries qsel (counts, slices or lists) of every matrix"""
    tsel = slice(0, tsel) if isinstance(tsel, int) else tsel
    qsel = slice(0, qsel) if isinstance(qsel, int) else qsel
    out = dict(ref)
    for k in ("y", "alpha", "quad", "quadmag", "logml"):
        out[k] = ref[k][:, tsel]
    if "a" in ref:
        out["a"] = ref["a"][:, qsel]
        for k in ("mean", "meanmag"):
            out[k] = ref[k][:, tsel][:, :, qsel]
    return out


def bounds(ref, n, u):
    """dict of the bounds of the module docstring: alpha[k, t, 1], quad[k, t], logdet[k], logml[k, t], mean[k, t, j]"""
    eps = (n + 4) * u * ref["cond"] ** 2
    ld = ref["logdet"].astype(np.float64)
    out = {"logdet": n * n * u * ref["cond"] + n * u * np.maximum(1.0, np.abs(ld))}
    if "y" in ref:
        an = np.linalg.norm(ref["alpha"], axis=2)
        out["alpha"] = (eps[:, None] * an)[:, :, None]
        out["quad"] = (eps * ref["knorm"])[:, None] * np.linalg.norm(ref["y"], axis=2) ** 2 + 2 * n * u * ref["quadmag"] + \
            u * np.abs(ref["quad"])
        s = ref["quad"] + ld[:, None]
        out["logml"] = (out["quad"] + out["logdet"][:, None]) / 2 + u * (np.abs(s) + 2 * n * LOG2PI + np.abs(s + n * LOG2PI)) / 2
        if "a" in ref:
            out["mean"] = eps[:, None, None] * an[:, :, None] * np.linalg.norm(ref["a"], axis=2)[:, None, :] + n * u * ref["meanmag"]
    return out


def shapes(ref, n):
    D = ref["y"].shape[1] if "y" in ref else 0
    Q = ref["a"].shape[1] if "a" in ref else 0
    return dict(alpha=(-1, D, n), quad=(-1, D), logdet=(-1,), logml=(-1, D), mean=(-1, D, Q))


def ratios(out, ref, n, u, idx=None):
    """err / bound of every output in the dict `out` (packed, as the kernels pack them) for the matrices idx"""
    b = bounds(ref, n, u)
    shp = shapes(ref, n)
    pick = (lambda a: a) if idx is None else (lambda a: a[idx])
    rs = {}
    for name in OUTPUTS:
        if out.get(name) is None:
            continue
        got = pick(np.asarray(out[name]).reshape(shp[name]))
        err = np.abs(got.astype(np.longdouble) - ref[name]).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            rs[name] = np.where(err == 0, 0.0, err / b[name])
        assert np.isfinite(got).all(), name
    return rs


def check(out, ref, n, u, idx=None, what="", factor=1.0):
    """every given output within factor * bound; prints err / bound first. Returns {name: worst err / bound}"""
    rs = ratios(out, ref, n, u, idx)
    shp = shapes(ref, n)
    worst = {k: float(v.max()) for k, v in rs.items()}
    print(f"  {what} n={n} D={shp['quad'][1]} Q={shp['mean'][2]} cond={ref['cond'].max():.2f} err/bound: " +
          " ".join(f"{k}={v:.4f}" for k, v in worst.items()))
    for k, v in rs.items():
        assert np.isfinite(v).all() and (v <= factor).all(), (what, n, k, float(np.nanmax(v)))
    return worst


def float32_evaluation(B, c, Ys, As, n, D, Q):
    """the reference formulas evaluated in float32 numpy on the float32 inputs: what any fp32 implementation of them may expect"""
    f = np.float32
    m = as_mats(B, n).astype(f)
    M = np.tril(m) + np.tril(m, -1).transpose(0, 2, 1)
    if c is not None:
        idx = np.arange(n)
        M[:, idx, idx] = M[:, idx, idx] + np.asarray(c, dtype=f).reshape(-1, n)
    K = np.linalg.inv(M)
    y = np.asarray(Ys, dtype=f).reshape(-1, D, n)
    alpha = np.einsum("kij,ktj->kti", K, y)
    quad = np.einsum("kti,kti->kt", y, alpha)
    logdet = np.linalg.slogdet(M)[1]  # the pivots of an elimination, as the kernels fold them (_whiten_worker.float32_evaluation)
    logml = f(-0.5) * (quad + logdet[:, None] + f(n) * f(LOG2PI))
    out = dict(alpha=alpha.reshape(-1), quad=quad.reshape(-1), logdet=logdet, logml=logml.reshape(-1))
    if Q:
        out["mean"] = np.einsum("kqi,kti->ktq", np.asarray(As, dtype=f).reshape(-1, Q, n), alpha).reshape(-1)
    assert all(v.dtype == f for v in out.values())
    return out


# ---- GPU helpers (torch and the package are imported by the caller) ---------------------------------------------------------------------
def run(api, torch, n, B, c, Ys, As, want=OUTPUTS, D=None, Q=None):
    """api.multi_target_batched on packed numpy inputs: (dict of the numpy outputs in `want`, info). Asserts that no input changed a bit"""
    batch = B.size // (n * n)
    host = [None if x is None else np.ascontiguousarray(x) for x in (B, c, Ys, As)]
    dev = [None if x is None else torch.tensor(x).cuda() for x in host]
    info = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
    res = api.multi_target_batched(n, *dev, batchSize=batch, info=info, want=want, ntarget=D, nquery=Q)
    torch.cuda.synchronize()
    for h, d in zip(host, dev):
        assert h is None or np.array_equal(d.cpu().numpy(), h, equal_nan=True), "an input was modified"
    out = {k: (None if v is None else v.cpu().numpy()) for k, v in zip(OUTPUTS, res)}
    assert all((out[k] is not None) == (k in want) for k in OUTPUTS)
    return {k: v for k, v in out.items() if v is not None}, info.cpu().numpy()


def same_bits(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k].reshape(-1), b[k].reshape(-1), equal_nan=True), (what, k)


def check_with_rejects(out, info, B, c, Ys, As, n, D, Q, dt, want_info, what=""):
    """info as expected, every output NaN exactly at the not-SPD matrices, finite and within the bounds elsewhere"""
    batch = info.size
    bad = sorted(want_info)
    ok = np.array([k for k in range(batch) if k not in want_info])
    expect = np.zeros(batch, dtype=np.int64)
    for k, v in want_info.items():
        expect[k] = v
    assert np.array_equal(info, expect), (what, n, info[bad], [want_info[k] for k in bad], np.flatnonzero(info != expect)[:10])
    for k, v in out.items():
        o = v.reshape(batch, -1)
        assert np.isnan(o[bad]).all() and np.isfinite(o[ok]).all(), (what, n, k)
    ref = reference(model(B, c, n, idx=ok), Ys, As, n, D, Q, idx=ok)
    return check(out, ref, n, U[np.dtype(dt)], idx=ok, what=what)


def run_case(api, torch, n, batch, D, Q, dt, with_c, rejects_at=None):
    B, c, _ = L.inputs(n, batch, dt, with_c)
    Ys = targets(n, batch, D, dt, seed=7500 + n)
    As = targets(n, batch, Q, dt, seed=9500 + n)
    want_info = break_three(B, c, n, rejects_at) if rejects_at else {}
    out, info = run(api, torch, n, B, c, Ys, As)
    check_with_rejects(out, info, B, c, Ys, As, n, D, Q, dt, want_info, f"{api.multi_target_kernel_name(dt, n)} batch={batch}")


def main():
    import torch
    api = importlib.import_module("cuda-matrix-inversion_amd.api")
    assert os.environ.get("MATINV_TILE_GRID_MULT") == "1" and os.environ.get("MATINV_BLOCKED_WS_MB") == "1"
    # 4000 matrices on a grid of 256 * 12 = 3072 workgroups: the stride loop runs twice; the rejects sit in the second round.
    run_case(api, torch, 33, 4000, 3, 2, np.float64, True, rejects_at=(3073, 3500, 3999))
    run_case(api, torch, 33, 4000, 3, 2, np.float32, False, rejects_at=(3100, 3600, 3998))
    # 20 working copies of 130 * (130 + 17) * 8 = 152 880 bytes under a cap of 1 MiB: six to a chunk, four chunks, three of them with a
    # non-zero `first`
    run_case(api, torch, 130, 20, 17, 16, np.float64, True)
    run_case(api, torch, 130, 20, 17, 16, np.float64, False, rejects_at=(7, 13, 19))
    print("multi-target-worker ok")


if __name__ == "__main__":
    main()
