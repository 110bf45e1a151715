"""Reference, inputs, bounds and checks of the tests of GP prediction from coordinates (tests/test_gpu_ard_predict.py and
tests/test_ard_predict_cpu.py import them), and the worker of test_grid_stride_and_chunking: ONE process under MATINV_TILE_GRID_MULT=1 and
MATINV_BLOCKED_WS_MB=1 (the library reads each switch once per process), so that the tile kernels' stride loop runs several rounds and the
global launcher takes several chunks. The worker is given a file of the outputs of the same calls made under the default switches, which
the test has checked against the reference before: it asserts equal bits, exits non-zero at the first failure and starts nothing after it;
prints `ard-predict-worker ok` at the end.

Reference: float64 numpy on the float64 image of exactly the inputs the kernel reads (fp32: the float32 values widened). The formulas of
_ard_worker are evaluated on the AUGMENTED point set [X; Xq] (n + Q points): its n x n block is M (noise on the diagonal), its n x Q
block is A, column j the cross-covariance vector a_j = sf2 phi(s(x_i, xq_j)) -- an off-diagonal block, so without noise even where a query
coincides with a training point. Then K = inv(M), alpha = K y,
    mean[k, j] = a_j^T alpha        var[k, j] = sf2 - a_j^T K a_j          (the variance of the latent function; not clamped)

Inputs: X, y, theta of _ard_worker.inputs (so cond2(M) <= _ard_worker.COND_CAP, asserted on the CPU by tests/test_ard_predict_cpu.py);
the queries are uniform in the same box [0, n^(1/d)]^d.

Bounds, first order and derived, not fitted. u = 2^-53 (fp64) or 2^-24 (fp32), E = 4 u the error of the device exponential. Two parts.
(1) The bounds the project already uses for mean and var ON A GIVEN M, A and prior variance e = sf2 (_predict_worker.bounds):
      |d mean| <= eps ||alpha|| ||a|| + n u sum_i |a_i alpha_i|
      |d var|  <= eps ||K||_2 ||a||^2 + 2 n u sum_ij |a_i K_ij a_j| + u (|e| + |var|),      eps = (n + 4) u cond2(M)^2
(2) The propagated GENERATION error. |dM| and |dA| are the blocks of _ard_worker.generation_error on the augmented set (an element of A is
    generated as an off-diagonal element of M is: z, zq = x / l, the difference, d fused multiply-adds, the element function, times sf2).
    With dK = -K dM K to first order:
      mean = a^T K y:        d mean = da^T alpha - a^T K dM alpha
                             |d mean_j| <= |da_j|^T |alpha| + |a_j|^T |K| |dM| |alpha|
      var = sf2 - a^T K a:   d var = d sf2 - 2 da^T (K a) + (K a)^T dM (K a)
                             |d var_j| <= (E + u) sf2 + 2 |da_j|^T |K a_j| + |K a_j|^T |dM| |K a_j|
    (sf2 is one exponential of an exact input, E, and enters the final sum once more, u.)
Nothing here is fitted to what the kernels return; tests/test_ard_predict_cpu.py confirms that a float32 numpy evaluation of the formulas
stays inside the fp32 bounds at every (n, d, Q, kind) the GPU tests use, and that the bounds reject six kinds of wrong result.
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
import _ard_worker as A  # noqa: E402
import _predict_worker as P  # noqa: E402

U = A.U
SE, MATERN52, KINDS = A.SE, A.MATERN52, A.KINDS
DIMS = (1, 3, 16)
QS = (1, 16, 17, 33)  # a partial group, an exact group, a group plus one, two groups plus one
QMAX = max(QS)
OUTPUTS = ("mean", "var")
batch_of = A.batch_of
same_bits = A.same_bits
nan_points = A.nan_points


def queries(n, d, batch, nquery, dt, seed=None, shared=False):
    """Xq (batch or 1, nquery, d) in dtype dt, uniform in the box of _ard_worker.inputs"""
    rng = np.random.default_rng(21000 + 97 * n + 7 * d if seed is None else seed)
    return rng.uniform(0.0, n ** (1.0 / d), (1 if shared else batch, nquery, d)).astype(dt)


def augmented(X, Xq, n, d, nquery, batch):
    """[X; Xq] as (batch, n + nquery, d) in the dtype of X; either may be shared (leading axis 1)"""
    Xb = np.broadcast_to(np.asarray(X).reshape(-1, n, d), (batch, n, d))
    Qb = np.broadcast_to(np.asarray(Xq).reshape(-1, nquery, d), (batch, nquery, d))
    return np.concatenate([Xb, Qb], axis=1)


def reference(X, y, theta, Xq, n, d, nquery, kind, u, dt, idx=None):
    """mean, var and every term of the bounds (float64) for the matrices idx (the others may be not SPD); y may be None (no mean)"""
    th = np.asarray(theta, dtype=np.float64).reshape(-1, d + 2)
    batch = th.shape[0]
    aug = augmented(np.asarray(X, dtype=np.float64), np.asarray(Xq, dtype=np.float64), n, d, nquery, batch)
    yb = None if y is None else np.broadcast_to(np.asarray(y, dtype=np.float64).reshape(-1, n), (batch, n))
    if idx is not None:
        th, aug = th[idx], aug[idx]
        yb = None if yb is None else yb[idx]
    na = n + nquery
    r = A.formulas(aug, np.zeros((th.shape[0], na)), th, na, d, kind, np.float64)
    r["dM"] = A.derivative_matrices(r, na, d)  # generation_error reads it
    gen, _ = A.generation_error(r, na, d, kind, u, dt)
    M = r["M"][:, :n, :n]
    K = np.linalg.inv(M)
    sv = np.linalg.svd(M, compute_uv=False)
    mdl = {"M": M, "K": K, "alpha": None if yb is None else np.einsum("kij,kj->ki", K, yb), "cond": sv[:, 0] / sv[:, -1],
           "knorm": 1.0 / sv[:, -1]}
    a = np.ascontiguousarray(r["M"][:, :n, n:].transpose(0, 2, 1))  # (batch, Q, n)
    ref = P.predict_reference(mdl, a, np.repeat(r["sf2"][:, None], nquery, axis=1), n, nquery)
    ref.update(sf2=r["sf2"], dMerr=gen[:, :n, :n], dA=np.ascontiguousarray(gen[:, :n, n:].transpose(0, 2, 1)),
               Ka=np.einsum("kij,kqj->kqi", K, a))
    return ref


PER_QUERY = ("a", "e", "var", "quadmag", "mean", "meanmag", "dA", "Ka")


def first_queries(ref, nquery):
    """the reference of the first nquery queries of every matrix"""
    return {k: (v[:, :nquery] if k in PER_QUERY else v) for k, v in ref.items()}


def bounds(ref, n, u):
    """(b_mean[k, j] or None, b_var[k, j]) of the module docstring"""
    b_mean, b_var = P.bounds(ref, n, u)
    aK, dM, dA = np.abs(ref["K"]), ref["dMerr"], ref["dA"]
    aKa = np.abs(ref["Ka"])
    b_var = b_var + (A.E_EXP + 1) * u * ref["sf2"][:, None] + 2 * np.einsum("kqi,kqi->kq", dA, aKa) + \
        np.einsum("kqi,kij,kqj->kq", aKa, dM, aKa)
    if b_mean is not None:
        aa = np.abs(ref["alpha"])
        b_mean = b_mean + np.einsum("kqi,ki->kq", dA, aa) + np.einsum("kqi,kij,kj->kq", np.abs(ref["a"]), aK, np.einsum("kij,kj->ki", dM, aa))
    return b_mean, b_var


def ratios(out, ref, n, u, idx=None):
    """err / bound of every output in the dict `out` (packed, as the kernels pack them) for the matrices idx"""
    b = dict(zip(OUTPUTS, bounds(ref, n, u)))
    nquery = ref["a"].shape[1]
    rs = {}
    for name in OUTPUTS:
        if out.get(name) is None:
            continue
        got = np.asarray(out[name], dtype=np.float64).reshape(-1, nquery)
        got = got if idx is None else got[idx]
        assert np.isfinite(got).all(), name
        err = np.abs(got - ref[name])
        rs[name] = np.where(err == 0, 0.0, err / b[name])
    return rs


def check(out, ref, n, dt, idx=None, what="", factor=1.0):
    """every given output within factor * bound; prints err / bound first. Returns {name: worst err / bound}"""
    rs = ratios(out, ref, n, U[np.dtype(dt)], idx)
    worst = {k: float(v.max()) for k, v in rs.items()}
    print(f"  {what} n={n} Q={ref['a'].shape[1]} {np.dtype(dt).name} cond={ref['cond'].max():.2f} err/bound: " +
          " ".join(f"{k}={v:.4f}" for k, v in worst.items()))
    for k, v in rs.items():
        assert np.isfinite(v).all() and (v <= factor).all(), (what, n, k, float(np.nanmax(v)))
    return worst


@functools.lru_cache(maxsize=4)
def case(n, d, dtname, kind):
    """the shared case: (X, y, theta, Xq, reference) with per-matrix points and QMAX per-matrix queries. Nobody writes into it"""
    dt = np.dtype(dtname).type
    batch = batch_of(n)
    X, y, theta = A.inputs(n, d, batch, dt)
    Xq = queries(n, d, batch, QMAX, dt)
    for x in (X, y, theta, Xq):
        x.setflags(write=False)
    return X, y, theta, Xq, reference(X, y, theta, Xq, n, d, QMAX, kind, U[np.dtype(dt)], dt)


def gpu_cases():
    """every (n, d) the accuracy tests of tests/test_gpu_ard_predict.py run, for both dtypes, both kinds and every Q of QS"""
    return [(n, d) for n in A.TILE_SIZES + A.GLOBAL_SIZES for d in DIMS] + [(1024, A.DIM_1024)]


def evaluation(X, y, theta, Xq, n, d, nquery, kind, f, wrong=None):
    """the formulas evaluated in numpy dtype f on inputs rounded to f: dict(mean, var), packed. wrong: one of the mistakes of
    tests/test_ard_predict_cpu.py, made on purpose (None: none)"""
    th = np.asarray(theta, dtype=f).reshape(-1, d + 2)
    batch = th.shape[0]
    Xb = np.broadcast_to(np.asarray(X, dtype=f).reshape(-1, n, d), (batch, n, d))
    Qb = np.broadcast_to(np.asarray(Xq, dtype=f).reshape(-1, nquery, d), (batch, nquery, d))
    yb = np.broadcast_to(np.asarray(y, dtype=f).reshape(-1, n), (batch, n))
    sf2, ell, sn2 = np.exp(th[:, 0]), np.exp(th[:, 1:d + 1]), np.exp(th[:, d + 1])
    z = Xb / ell[:, None, :]
    if wrong == "two dimensions swapped":  # of the query's coordinates, not of the length scales
        Qb = Qb[:, :, [1, 0] + list(range(2, d))]
    zq = Qb if wrong == "query not divided by l" else Qb / ell[:, None, :]

    def sq(p, q):
        s = np.zeros((batch, p.shape[1], q.shape[1]), dtype=f)
        for k in range(d):
            dk = p[:, :, None, k] - q[:, None, :, k]
            s = s + dk * dk
        return s

    s_mm, s_mq = sq(z, z), sq(z, zq)
    M = sf2[:, None, None] * A.element(s_mm, kind, f)[0] + sn2[:, None, None] * np.eye(n, dtype=f)
    a = sf2[:, None, None] * A.element(s_mq, (1 - kind) if wrong == "phi of the other kind" else kind, f)[0]  # (batch, n, Q)
    if wrong == "noise at a coincident point":
        a = a + sn2[:, None, None] * (s_mq == 0)
    if wrong == "one training point dropped":
        a = a.copy()
        a[np.arange(batch), np.abs(a[:, :, 0]).argmax(axis=1), 0] = 0  # the largest element of query 0 of every matrix
    K = np.linalg.inv(M)
    alpha = np.einsum("kij,kj->ki", K, yb)
    prior = sf2 + sn2 if wrong == "prior variance with noise" else sf2
    mean = np.einsum("kiq,ki->kq", a, alpha)
    var = prior[:, None] - np.einsum("kiq,kiq->kq", a, np.einsum("kij,kjq->kiq", K, a))
    out = dict(mean=mean.reshape(-1), var=var.reshape(-1))
    assert all(v.dtype == f for v in out.values())
    return out


# ---- GPU helpers (torch and the package are imported by the caller) ---------------------------------------------------------------------
def run(api, torch, n, X, y, theta, Xq, kind, want=OUTPUTS, d=None):
    """api.ard_predict_batched on numpy inputs (y may be None without "mean"): (dict of the numpy outputs in `want`, info). Asserts that
    no input changed"""
    d = X.shape[-1] if d is None else d
    batch = theta.size // (d + 2)
    host = [None if x is None else np.ascontiguousarray(x) for x in (X, y, theta, Xq)]
    dev = [None if x is None else torch.tensor(x).cuda() for x in host]
    info = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
    res = api.ard_predict_batched(n, *dev, kind=kind, ndim=d, batchSize=batch, info=info, want=want)
    torch.cuda.synchronize()
    for h, dv in zip(host, dev):
        assert h is None or np.array_equal(dv.cpu().numpy(), h, equal_nan=True), "an input was modified"
    out = {k: (None if v is None else v.cpu().numpy()) for k, v in zip(OUTPUTS, res)}
    assert all((out[k] is not None) == (k in want) for k in OUTPUTS)
    return {k: v for k, v in out.items() if v is not None}, info.cpu().numpy()


def check_with_rejects(out, info, X, y, theta, Xq, n, d, nquery, kind, dt, want_info, what="", sample=None):
    """info as expected, every output NaN exactly at the rejected matrices, finite everywhere else and within the bounds there (sample:
    at that many of them, evenly spread and with both neighbours of every reject, where the reference of thousands would not fit)"""
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
    if sample is not None and ok.size > sample:
        near = [k + e for k in bad for e in (-1, 1) if 0 <= k + e < batch and k + e not in want_info]
        ok = np.unique(np.concatenate([ok[::max(1, ok.size // sample)], np.array(near, dtype=ok.dtype), ok[-1:]]))
    ref = reference(X, y, theta, Xq, n, d, nquery, kind, U[np.dtype(dt)], dt, idx=ok)
    return check(out, ref, n, dt, idx=ok, what=what)


# the calls of test_grid_stride_and_chunking: (n, d, Q, batch, dtype, kind, shared X / y / Xq, rejects {matrix: point}). 4000 matrices on
# a grid of 256 * 12 = 3072 workgroups run the stride loop twice; the rejects sit beyond the first round. 20 working copies of
# (100 * 100 + 100 * 2) * 8 = 81 600 bytes under a cap of 1 MiB: twelve to a chunk, two chunks, one with a non-zero `first`.
STRIDE_CASES = ((33, 2, 17, 4000, np.float64, SE, False, {3073: 0, 3500: 17, 3999: 32}),
                (33, 3, 3, 4000, np.float32, MATERN52, True, {}),
                (33, 2, 3, 4000, np.float32, SE, False, {3100: 16, 3600: 5, 3998: 0}),
                (100, 2, 17, 20, np.float64, MATERN52, False, {7: 0, 13: 64, 19: 99}))


def stride_inputs(n, d, nquery, batch, dt, kind, shared, rejects):
    X, y, theta = A.inputs(n, d, batch, dt, seed=16000 + n + d, shared=shared)
    Xq = queries(n, d, batch, nquery, dt, seed=17000 + n + d, shared=shared)
    want_info = {}
    if rejects:
        X, want_info = nan_points(X, n, rejects)
    return X, y, theta, Xq, want_info


def stride_key(i, k):
    return f"case{i}_{k}"


def main():
    import torch
    api = importlib.import_module("cuda-matrix-inversion_amd.api")
    assert os.environ.get("MATINV_TILE_GRID_MULT") == "1" and os.environ.get("MATINV_BLOCKED_WS_MB") == "1"
    saved = np.load(sys.argv[1])
    for i, (n, d, nquery, batch, dt, kind, shared, rejects) in enumerate(STRIDE_CASES):
        X, y, theta, Xq, _ = stride_inputs(n, d, nquery, batch, dt, kind, shared, rejects)
        s = (lambda x: x[0]) if shared else (lambda x: x)
        out, info = run(api, torch, n, s(X), s(y), theta, s(Xq), kind, d=d)
        assert np.array_equal(info, saved[stride_key(i, "info")]), (i, "info")
        same_bits(out, {k: saved[stride_key(i, k)] for k in out}, (i, "default call"))
        print(f"  {api.ard_predict_kernel_name(dt, kind, n)} batch={batch} d={d} Q={nquery}: the bits of the default call")
    print("ard-predict-worker ok")


if __name__ == "__main__":
    main()
