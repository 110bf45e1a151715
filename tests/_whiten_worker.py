"""Reference, bounds and checks of the tests of the batched whitening, Mahalanobis distances and Gaussian log-density
(tests/test_gpu_whiten.py and tests/test_whiten_cpu.py import them), and the worker of test_grid_stride_and_chunking: ONE process under
MATINV_TILE_GRID_MULT=1 and MATINV_BLOCKED_WS_MB=1 (the library reads each switch once per process), so that the tile kernels' stride loop
runs twice and the global launcher takes several chunks; it compares the bits with those of one-round, one-chunk calls of the same
matrices. Exits non-zero at the first failure and starts nothing after it; prints `whiten-worker ok` at the end.

Inputs: those of tests/_colour_worker.py (`case`: C = G G^T / q + I, cond2 of order 5; m ~ N(0, 1)); its samples Z are the points X.

Reference: float64 numpy on the float64 image of exactly what the kernel reads (the lower triangle of C, mirrored):
    Lh = numpy.linalg.cholesky(C);   in longdouble:  Wh = Lh^-1 (x - m) by forward substitution,  mh = sum_i Wh_i^2,
    ldh = 2 sum_i log L_ii with the factor itself taken in longdouble (logdet_longdouble says why),  ph = -(mh + ldh + q log 2 pi) / 2

Bounds. u = 2^-53 (fp64) or 2^-24 (fp32), gamma_k = k u / (1 - k u), kappa = cond2(C) from float64 numpy. (1) and (2) are the bounds of
tests/_colour_worker.py on the factor and on Y.

(3) W. The kernel solves with its own factor L = Lh + dL on the right-hand side fl(x - m) = (x - m) + e, |e_i| <= u (|x_i| + |m_i|), and the
    substitution is backward stable row by row (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Thm 8.5):
    (L + DL) W = (x - m) + e with |DL| <= gamma |L|. Subtracting Lh Wh = x - m:  Lh (W - Wh) = e - dL W - DL W, so to first order
        |W - Wh| <= |Lh^-1| r,     r_i = u (|x_i| + |m_i|) + dl ||Wh||_2 + gamma_{q+1+EXTRA_W} (|Lh| |Wh|)_i
    dl bounds ||dL||_F: the Thm 10.8 term of _colour_worker bound (2), 2^-1/2 kappa ||dC||_F ||Lh||_2 / ||C||_2 with dC from bound (1);
    |(dL W)_i| <= ||dL||_F ||W||_2 (Cauchy-Schwarz). gamma_{q+1} is the theorem's: one rounding per multiply-add of the row's q-term sum,
    in any order, and one division.
    q >= 97, the global form: the theorem's algorithm (columns ascending, a true division). EXTRA_W = 0.
    q <= 96, the tile forms: the rows of a block of four columns are solved at once as M y with the explicit inverse
    M = diag(1 / sqrt u) l^-1 of the 4 x 4 diagonal block of L (l: PanelSolve's unit-lower factor of the pivot block, u its squared
    Cholesky diagonal), one MFMA; the update of the rows below is the theorem's multiply-add, inside an MFMA. Roundings on the path of
    one term M_tk y_k beyond those the theorem counts, in units of u, to first order (whiten_tile_impl.hpp, columns()):
      *  1: rqc = fl(1 / sqrt u_t), where the theorem divides by the diagonal entry (the multiply-add with M_tk is the theorem's);
      *  1: the product e * rqc that forms M_tk;
      *  3: an entry of l^-1 is up to three multiply-adds (m30);
      *  9: a term of that entry is a product of up to three entries of l, each 3 roundings from the stored panel values (the count
            of _colour_worker bound (1): a product with a refined reciprocal);
      *  5: the theorem's T is the factor the bound names, here Lh + dL with dL the error of the STORED columns P l^-T diag(u)^-1/2; M
            is formed from l and u directly, and a stored entry differs from l_tk sqrt u_k by the three multiply-adds of x_k, the
            reciprocal and the product with it.
        EXTRA_W = 19
    As in _colour_worker bound (1) the count does not include the amplification of these roundings by the condition of the 4 x 4
    block; if the kernels needed it they would fail this bound. Nothing here is fitted to what the kernels return.

(4) maha. With b3 = bound (3): |W_i^2 - Wh_i^2| <= 2 |Wh_i| b3_i to first order, and the q-term sum of squares rounds once per
    multiply-add and once where the four partial sums meet, in any order gamma_{q+1}:
        |maha - mh| <= 2 sum_i |Wh_i| b3_i + gamma_{q+1} mh

(5) logdet. The bound() of tests/test_gpu_logdet.py on the same PivotProduct:  q^2 u kappa + q u max(1, |ldh|). The tile forms fold the
    pivots u_i = L_ii^2 as the log-determinant kernels do; the global form folds the roots L_ii and doubles the logarithm, which adds
    the roots' roundings, 2 q u, where q >= 97 and the first term is q kappa / 2 times that.

logpdf. Half of (4) + (5), and the roundings of its own terms: fl(maha + logdet), the product with the rounded constant log 2 pi and the
    last addition (the tile forms fuse the last two; the factor -1/2 is exact):
        |logpdf - ph| <= ((4) + (5)) / 2 + u (|mh + ldh| + 2 q log 2 pi + |mh + ldh + q log 2 pi|) / 2

tests/test_whiten_cpu.py confirms that a float32 numpy evaluation of the reference formulas stays inside the fp32 bounds at every size the
GPU tests use.
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
from _colour_worker import BATCH, QSIZES, SS, U, break_at, case, factor_bound, gamma, mats, reference, samples  # noqa: E402,F401

EXTRA_W_TILE = 19  # bound (3) of the module docstring, q <= 96
TILE_MAX = 96
LOG2PI = float(np.log(2 * np.pi))
OUTPUTS = ("W", "maha", "logdet", "logpdf")


def extra_w(q):
    return EXTRA_W_TILE if q <= TILE_MAX else 0


def forward_substitution(L, b):
    """L[k, i, j] lower triangular, b[k, s, i]: L^-1 b in the dtype of b, rows ascending"""
    w = np.zeros_like(b)
    Lb = L.astype(b.dtype)
    for i in range(L.shape[1]):
        acc = b[:, :, i] - np.einsum("kj,ksj->ks", Lb[:, i, :i], w[:, :, :i])
        w[:, :, i] = acc / Lb[:, i, i][:, None]
    return w


LOGDET_WIDE_MAX = 96  # the tile forms


def logdet_longdouble(c, L):
    """log det of the float64 matrices c[k]: 2 sum log of the diagonal of a Cholesky factor taken in longdouble (right-looking, the batch
    at once), so that the reference's own error stays out of what is held against bound (5): the float64 factor L carries up to u per
    diagonal entry, 2 q u in the sum, which at q = 1 is the whole bound. Beyond LOGDET_WIDE_MAX the float64 factor serves: 2 q u is then
    below 1 / (48 kappa) of the bound's first term q^2 u kappa, and the wide factorisation would take seconds to minutes"""
    ld = np.longdouble
    q = c.shape[1]
    if q > LOGDET_WIDE_MAX:
        return 2 * np.log(np.diagonal(L.astype(ld), axis1=1, axis2=2)).sum(axis=1)
    a = c.astype(ld)
    out = np.zeros(c.shape[0], dtype=ld)
    for j in range(q):
        d = a[:, j, j]
        assert (d > 0).all()
        out += np.log(d)  # the pivot is the square of the diagonal entry
        col = a[:, j + 1:, j]
        a[:, j + 1:, j + 1:] -= col[:, :, None] * (col / d[:, None])[:, None, :]
    return out


def whiten_reference(C, m, X, q, idx=None):
    """_colour_worker.reference (C, L, kappa, cnorm, lnorm, z = the points, m) plus, in longdouble, W[k, s, i], maha[k, s], logdet[k] and
    logpdf[k, s]; Linv[k, i, j] in float64"""
    ref = reference(C, m, X, q, idx=idx)
    ld = np.longdouble
    L = ref["L"].astype(ld)
    ref["W"] = forward_substitution(L, ref["z"].astype(ld) - ref["m"].astype(ld)[:, None, :])
    ref["maha"] = (ref["W"] ** 2).sum(axis=2)
    ref["logdet"] = logdet_longdouble(ref["C"], ref["L"])
    ref["logpdf"] = -(ref["maha"] + ref["logdet"][:, None] + q * np.log(2 * ld(np.pi))) / 2
    ref["Linv"] = np.linalg.inv(ref["L"])
    return ref


@functools.lru_cache(maxsize=None)
def case_reference(q, dtname, batch=BATCH, scale=1.0):
    """whiten_reference of `case` with all its SMAX points. Computed once, shared; `take` slices it"""
    C, m, X = case(q, dtname, batch, scale)
    return whiten_reference(C, m, X, q)


def take(ref, sel):
    """the reference of the points `sel` (a slice or a list) of every matrix: the point-wise fields sliced, the others shared"""
    out = dict(ref)
    for k in ("z", "W", "maha", "logpdf"):
        out[k] = ref[k][:, sel]
    return out


def logdet_reference(C, q, idx=None):
    """the part of whiten_reference that needs no points"""
    ref = reference(C, None, None, q, idx=idx)
    ref["logdet"] = logdet_longdouble(ref["C"], ref["L"])
    return ref


def w_bound(ref, q, u, extra_r=None):
    """bound (3): b[k, s, i]; extra_r[k, s, i]: a bound on one more perturbation of the right-hand side (the round trip)"""
    wh = np.abs(ref["W"]).astype(np.float64)
    dl = 2 ** -0.5 * ref["kappa"] * np.linalg.norm(factor_bound(ref, q, u), axis=(1, 2)) * ref["lnorm"] / ref["cnorm"]
    r = u * (np.abs(ref["z"]) + np.abs(ref["m"])[:, None, :]) + (dl[:, None] * np.linalg.norm(wh, axis=2))[:, :, None] + \
        gamma(q + 1 + extra_w(q), u) * np.einsum("kij,ksj->ksi", np.abs(ref["L"]), wh)
    if extra_r is not None:
        r = r + extra_r
    return np.einsum("kij,ksj->ksi", np.abs(ref["Linv"]), r)


def maha_bound(ref, q, u, b3):
    """bound (4): b[k, s]"""
    return 2 * (np.abs(ref["W"]).astype(np.float64) * b3).sum(axis=2) + gamma(q + 1, u) * ref["maha"].astype(np.float64)


def logdet_bound(ref, q, u):
    """bound (5): b[k]"""
    return q * q * u * ref["kappa"] + q * u * np.maximum(1.0, np.abs(ref["logdet"].astype(np.float64)))


def logpdf_bound(ref, q, u, b4, b5):
    s = (ref["maha"] + ref["logdet"][:, None]).astype(np.float64)
    return (b4 + b5[:, None]) / 2 + u * (np.abs(s) + 2 * q * LOG2PI + np.abs(s + q * LOG2PI)) / 2


def check(out, ref, q, u, idx=None, what="", extra_r=None):
    """out: dict of packed outputs (a subset of OUTPUTS) for the matrices idx; every one against its bound. Returns {name: worst err / bound}"""
    nb, S = (ref["z"].shape[0], ref["z"].shape[1]) if "z" in ref else (ref["L"].shape[0], 0)
    pick = (lambda a: a) if idx is None else (lambda a: a[idx])
    worst = {}
    b3 = b4 = None
    if set(out) - {"logdet"}:
        b3 = w_bound(ref, q, u, extra_r)
        b4 = maha_bound(ref, q, u, b3)
    b5 = logdet_bound(ref, q, u)
    bounds = dict(W=b3, maha=b4, logdet=b5, logpdf=None if b4 is None else logpdf_bound(ref, q, u, b4, b5))
    shapes = dict(W=(-1, S, q), maha=(-1, S), logdet=(-1,), logpdf=(-1, S))
    for name in OUTPUTS:
        if out.get(name) is None:
            continue
        got = pick(np.asarray(out[name], dtype=np.float64).reshape(shapes[name]))
        assert got.shape[0] == nb, (what, name, got.shape, nb)
        err = np.abs(got - ref[name]).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where(err == 0, 0.0, err / bounds[name])  # x = m: error and bound are both zero
        worst[name] = float(r.max())
        assert np.isfinite(got).all() and np.isfinite(r).all() and (r <= 1).all(), (what, q, name, float(np.nanmax(r)))
    print(f"  {what} q={q} S={S} kappa={ref['kappa'].max():.2f} err/bound: " + "  ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    return worst


def float32_evaluation(C, m, X, q):
    """the reference formulas in float32 numpy on the float32 inputs: dict of the four outputs packed as the kernels pack them"""
    f = np.float32
    c = mats(C, q).astype(f)  # exact: C is float32
    L = np.linalg.cholesky(c)
    x = np.asarray(X, dtype=f).reshape(c.shape[0], -1, q)
    w = forward_substitution(L, x - np.asarray(m, dtype=f).reshape(-1, 1, q))
    maha = (w * w).sum(axis=2, dtype=f)
    # the tile forms fold the pivots u_i = L_ii^2 of the elimination, not their roots, and bound (5) is the bound of such a product:
    # numpy's slogdet (the pivots of an elimination, too). 2 sum log fl(sqrt u_i) carries the roundings of the roots twice -- at q = 1
    # that alone is 2 u, the whole of bound (5). The global form does fold the roots: 2 q u more, against q^2 u kappa at q >= 97
    logdet = np.linalg.slogdet(c)[1]
    logpdf = f(-0.5) * (maha + logdet[:, None] + f(q) * f(LOG2PI))
    out = dict(W=w.reshape(-1), maha=maha.reshape(-1), logdet=logdet, logpdf=logpdf.reshape(-1))
    assert all(v.dtype == f for v in out.values())
    return out


# ---- GPU helpers (torch and the package are imported by the caller) ---------------------------------------------------------------------
def run(api, torch, q, C, m, X, want=OUTPUTS, sl=None, stride=None, batch=None):
    """api.whiten_batched on the matrices sl of the packed case: (dict of numpy outputs in `want`, info)"""
    nb = batch if batch is not None else C.size // (q * q)
    pick = (lambda a, per: a) if sl is None else (lambda a, per: np.ascontiguousarray(a.reshape(nb, per)[sl]).reshape(-1))
    t = lambda a: None if a is None else torch.tensor(np.ascontiguousarray(a)).cuda()  # noqa: E731
    c = t(C if stride is not None else pick(C, q * q))
    mm = t(None if m is None else pick(m, q))
    x = t(None if X is None else pick(X, X.size // nb))
    cnt = nb if sl is None else len(range(nb)[sl])
    info = torch.full((cnt,), -7, dtype=torch.int32, device="cuda")
    res = api.whiten_batched(q, c, mm, x, batchSize=cnt, info=info, want=want, strideC=stride)
    torch.cuda.synchronize()
    out = {k: (None if v is None else v.cpu().numpy()) for k, v in zip(OUTPUTS, res)}
    assert all((out[k] is not None) == (k in want) for k in OUTPUTS)
    return {k: v for k, v in out.items() if v is not None}, info.cpu().numpy()


def same_bits(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def break_many(C, q, rejects):
    """_colour_worker.break_at for every (matrix k -> column j) of `rejects` in one copy"""
    out = np.array(C)
    c = mats(C, q)
    for k, j in rejects.items():
        s = np.linalg.cholesky(c[k])[j - 1, j - 1] ** 2
        out.reshape(-1, q, q)[k, j - 1, j - 1] = c[k, j - 1, j - 1] - 1.5 * s
    return out


def run_rounds(api, torch, q, batch, dt, part, rejects):
    """a batch of `batch` matrices in one call against the same matrices in calls of `part` (one grid round, one chunk): the same bits,
    rejects (k -> column) included"""
    C, m, X = case(q, np.dtype(dt).name, batch)
    X = samples(X, q, slice(0, 3))
    C = break_many(C, q, rejects)
    out, info = run(api, torch, q, C, m, X)
    expect = np.zeros(batch, dtype=np.int64)
    for k, j in rejects.items():
        expect[k] = j
    assert np.array_equal(info, expect), (q, info[sorted(rejects)], rejects)
    bad = sorted(rejects)
    assert all(np.isnan(v.reshape(batch, -1)[bad]).all() for v in out.values())
    for lo in range(0, batch, part):
        sl = slice(lo, min(lo + part, batch))
        o1, i1 = run(api, torch, q, C, m, X, sl=sl)
        same_bits(o1, {k: v.reshape(batch, -1)[sl].reshape(-1) for k, v in out.items()}, (q, lo))
        assert np.array_equal(i1, info[sl]), (q, lo, "info")
    ok = np.array([k for k in range(batch) if k not in rejects])
    ref = whiten_reference(C, m, X, q, idx=ok)
    check(out, ref, q, U[np.dtype(dt)], idx=ok, what=f"{api.whiten_kernel_name(dt, q)} batch={batch}")


def main():
    import torch
    api = importlib.import_module("cuda-matrix-inversion_amd.api")
    assert os.environ.get("MATINV_TILE_GRID_MULT") == "1" and os.environ.get("MATINV_BLOCKED_WS_MB") == "1"
    # 4000 matrices on a grid of 256 * 12 = 3072 workgroups (launch_whiten_tile takes predict_tile_grid): the stride loop runs twice.
    # About 60 % of the matrices are rejects, in both rounds, at columns 1, 16, 17 and 33. Parts of 2000 stay inside one round.
    rng = np.random.default_rng(4500)
    for dt in (np.float64, np.float32):
        ks = rng.permutation(4000)[:2400]
        rejects = {int(k): int(rng.choice([1, 16, 17, 33])) for k in ks}
        assert any(k >= 3072 for k in rejects) and any(k < 3072 for k in rejects)
        run_rounds(api, torch, 33, 4000, dt, 2000, rejects)
    # 20 working copies of 130 * (130 + 3) * 8 = 138 320 bytes under a cap of 1 MiB: seven to a chunk, three chunks, two of them with a
    # non-zero `first`; 12 of the 20 are rejects. Parts of 5 stay inside one chunk.
    ks = rng.permutation(20)[:12]
    run_rounds(api, torch, 130, 20, np.float64, 5, {int(k): int(rng.choice([1, 16, 97, 130])) for k in ks})
    print("whiten-worker ok")


if __name__ == "__main__":
    main()
