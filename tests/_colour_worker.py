"""Reference, inputs, bounds and checks of the tests of the batched Cholesky factor, the coloured samples and the joint posterior samples
(tests/test_gpu_colour.py, tests/test_gpu_sample.py and tests/test_colour_cpu.py import them), and the worker of
test_grid_stride_and_chunking: ONE process under MATINV_TILE_GRID_MULT=1 and MATINV_BLOCKED_WS_MB=1 (the library reads each switch once
per process), so that the tile kernels' stride loop runs twice and the global launcher takes several chunks; it compares the bits with
those of one-round, one-chunk calls of the same matrices, and does the same for the k-range chunks of matinv_sample_batched when mean
and cov live in library scratch. Exits non-zero at the first failure and starts nothing after it; prints
`colour-worker ok` at the end.

Reference: float64 numpy on the float64 image of exactly what the kernel reads (the lower triangle of C, mirrored):
    Lh = numpy.linalg.cholesky(C),      Yh[:, s] = m + Lh z_s

Inputs: C = G G^T / q + I with G ~ N(0, 1) of size q x q, rounded to the working dtype and its lower triangle mirrored: cond2(C) is of
order 5, so forward bounds mean something. m, z ~ N(0, 1).

Bounds. u = 2^-53 (fp64) or 2^-24 (fp32), gamma_k = k u / (1 - k u), kappa = cond2(C) from float64 numpy.

(1) Backward error of the factor, componentwise (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Thm 10.3):
        |C - L L^T|_ij <= (gamma_{q+1} + EXTRA u) (|Lh| |Lh^T|)_ij
    gamma_{q+1} is the theorem's: one rounding (u) per multiply-add of the q-term sums, any order, one division and one square root.
    q >= 97, the global form: it runs the theorem's algorithm with a correctly rounded square root and a true division. EXTRA = 0.
    q <= 96, the tile forms: a blocked sweep that eliminates four columns at a time through the explicit inverse X of the 4 x 4 pivot
    block D, with the Cholesky columns of the step taken as P l^-T diag(u)^-1/2 from the panel P and the unit-lower factor l of D. The
    roundings on the path of one term beyond those the theorem counts, in units of u, to first order:
      *  2: a factor entry is x * fl(1 / sq) where the theorem divides once: one rounding more per entry, two per product l_ik l_jk
            (the diagonal entry is the correctly rounded square root itself: nothing more);
      * 19: a block step updates the trailing matrix with (P X) P^T instead of the product of the columns. One term p_is X_st p_jt
            sees the multiply-add the theorem counts (inside the MFMA) and, beyond it: 4 for the four-term sum P X; 4 for the back
            substitution behind X_st (three multiply-adds and a product with a reciprocal); 3 for the forward substitution; 2 for the
            refined reciprocal itself (1 ulp = 2 u); 3 for the unit-lower entry it multiplies (a product with another such
            reciprocal); 3 for the three multiply-adds of the pivot it inverts.
        EXTRA = 21
    A block step's terms are relative to its own share of |L| |L^T| and the shares add up, so the constant does not grow with q. The
    count does NOT include the amplification of these roundings by kappa(D) through the two triangular solves (kappa(D) <= kappa, D
    being a principal block of a Schur complement of C): if the kernels needed it they would fail this bound, and they do not. The
    worst observed error / bound is recorded in DESIGN.md; nothing here is fitted to it.

(2) Forward error of Y against Yh. With dC = |C - L L^T| bounded by (1) -- plus, for the posterior samples, the covariance route's own
    bound on cov (tests/_predict_cov_worker.bounds) -- the first-order perturbation bound of the Cholesky factor (Thm 10.8, Sun):
        ||L - Lh||_F <= 2^-1/2 kappa ||dC||_F / ||C||_2 * ||Lh||_2
    and row by row |((L - Lh) z)_i| <= ||L - Lh||_F ||z||_2 (Cauchy-Schwarz). The product's own rounding: m is the start of the
    q-term sum in the tile forms and its last addend in the global form, gamma_{q+1} (|Lh| |z| + |m|)_i either way. For the posterior
    samples the covariance route's bound on mean is added.
        |Y - Yh|_i <= 2^-1/2 kappa ||dC||_F ||Lh||_2 / ||C||_2 * ||z||_2 + gamma_{q+1} (|Lh| |z| + |m|)_i  (+ b_mean_i)
tests/test_colour_cpu.py confirms that a float32 numpy evaluation of the reference formulas stays inside the fp32 bounds at every size the
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
import _loo_worker as LW  # noqa: E402
import _predict_cov_worker as PC  # noqa: E402
import _predict_worker as P  # noqa: E402

U = {np.dtype(np.float64): 2.0 ** -53, np.dtype(np.float32): 2.0 ** -24}
QSIZES = [1, 15, 16, 17, 33, 96, 97, 130]
SS = (1, 16, 17, 33)
SMAX = max(SS)
BATCH = 200


def gamma(k, u):
    return k * u / (1 - k * u)


EXTRA_TILE = 21  # bound (1) of the module docstring, q <= 96
TILE_MAX = 96


def extra(q):
    return EXTRA_TILE if q <= TILE_MAX else 0


def mats(C, q):
    """float64 C[k, i, j] as the kernels read it: the lower triangle of the packed column-major input, mirrored"""
    c = np.asarray(C, dtype=np.float64).reshape(-1, q, q).transpose(0, 2, 1)
    return np.tril(c) + np.tril(c, -1).transpose(0, 2, 1)


def unpack(L, q):
    """L[k, i, j] of the packed column-major output"""
    return np.asarray(L).reshape(-1, q, q).transpose(0, 2, 1)


@functools.lru_cache(maxsize=None)
def case(q, dtname, batch=BATCH, scale=1.0):
    """(C, m, Z) packed, in the dtype: batch matrices C = (G G^T / q + I) * scale, m and SMAX samples each. Computed once, read-only"""
    dt = np.dtype(dtname).type
    rng = np.random.default_rng(4100 + q)
    G = rng.standard_normal((batch, q, q))
    C = ((G @ G.transpose(0, 2, 1)) / q + np.eye(q)) * scale
    C = C.astype(dt)
    C = np.tril(C) + np.tril(C, -1).transpose(0, 2, 1)
    m = rng.standard_normal((batch, q)).astype(dt)
    Z = rng.standard_normal((batch, SMAX, q)).astype(dt)
    out = (np.ascontiguousarray(C).reshape(-1), m.reshape(-1), Z.reshape(-1))
    for a in out:
        a.setflags(write=False)
    return out


def samples(Z, q, sel, total=SMAX):
    """the samples `sel` (a slice or a list) of the `total` samples of every matrix, packed"""
    return np.ascontiguousarray(Z.reshape(-1, total, q)[:, sel]).reshape(-1)


def reference(C, m, Z, q, idx=None):
    """float64: C, Lh, kappa, and with Z the samples z[k, s, :], m and Yh[k, s, :]"""
    c = mats(C, q)
    nb = c.shape[0]
    if idx is not None:
        c = c[idx]
    ref = dict(C=c, L=np.linalg.cholesky(c), kappa=np.linalg.cond(c), cnorm=np.linalg.norm(c, 2, axis=(1, 2)))
    ref["lnorm"] = np.linalg.norm(ref["L"], 2, axis=(1, 2))
    if Z is not None:
        z = np.asarray(Z, dtype=np.float64).reshape(nb, -1, q)
        mm = np.zeros((nb, q)) if m is None else np.asarray(m, dtype=np.float64).reshape(-1, q)
        if idx is not None:
            z, mm = z[idx], mm[idx]
        # Yh in extended precision: its own evaluation error stays out of what is held against bound (2)
        ld = np.longdouble
        ref.update(z=z, m=mm, Y=mm.astype(ld)[:, None, :] + np.einsum("kij,ksj->ksi", ref["L"].astype(ld), z.astype(ld)))
    return ref


def factor_bound(ref, q, u):
    """bound (1): tol[k, i, j]"""
    la = np.abs(ref["L"])
    return (gamma(q + 1, u) + extra(q) * u) * (la @ la.transpose(0, 2, 1))


def y_bound(ref, q, u, dcov=None, dmean=None):
    """bound (2): b[k, s, i]; dcov[k, i, j], dmean[k, i]: the bounds of the inputs' own errors (posterior samples)"""
    dC = factor_bound(ref, q, u)
    if dcov is not None:
        dC = dC + dcov
    dl = 2 ** -0.5 * ref["kappa"] * np.linalg.norm(dC, axis=(1, 2)) * ref["lnorm"] / ref["cnorm"]
    own = gamma(q + 1, u) * (np.einsum("kij,ksj->ksi", np.abs(ref["L"]), np.abs(ref["z"])) + np.abs(ref["m"])[:, None, :])
    b = (dl[:, None] * np.linalg.norm(ref["z"], axis=2))[:, :, None] + own
    if dmean is not None:
        b = b + dmean[:, None, :]
    return b


def check_factor(L, ref, q, u, idx=None, what=""):
    """structure and bound (1) of the packed output L for the matrices idx; returns the worst err / bound"""
    l = unpack(L, q)
    if idx is not None:
        l = l[idx]
    assert np.array_equal(np.triu(l, 1), np.zeros_like(l)), (what, "the strict upper triangle is not exactly zero")
    assert (np.diagonal(l, axis1=1, axis2=2) > 0).all(), (what, "diagonal not positive")
    # the residual of a float64 factor is of the order of float64's own rounding: it is evaluated in extended precision, so that what
    # is held against the bound is the kernel's error and not the evaluation's
    wide = np.longdouble if l.dtype == np.float64 else np.float64
    lw = l.astype(wide)
    r = np.abs(ref["C"].astype(wide) - np.einsum("kij,klj->kil", lw, lw)).astype(np.float64) / factor_bound(ref, q, u)
    print(f"  {what} q={q} kappa={ref['kappa'].max():.2f} factor err/bound: {r.max():.4f}")
    assert np.isfinite(r).all() and (r <= 1).all(), (what, q, float(np.nanmax(r)))
    return float(r.max())


def check_y(Y, ref, q, u, idx=None, what="", dcov=None, dmean=None):
    """bound (2) of the packed output Y for the matrices idx; returns the worst err / bound"""
    y = np.asarray(Y, dtype=np.float64).reshape(-1, ref["z"].shape[1], q)
    if idx is not None:
        y = y[idx]
    r = np.abs(y - ref["Y"]).astype(np.float64) / y_bound(ref, q, u, dcov, dmean)
    print(f"  {what} q={q} S={ref['z'].shape[1]} Y err/bound: {r.max():.4f}")
    assert np.isfinite(r).all() and (r <= 1).all(), (what, q, float(np.nanmax(r)))
    return float(r.max())


def float32_evaluation(C, m, Z, q):
    """the reference formulas in float32 numpy on the float32 inputs: (L, Y) packed as the kernels pack them"""
    f = np.float32
    c = mats(C, q).astype(f)  # exact: C is float32
    l = np.linalg.cholesky(c)
    z = np.asarray(Z, dtype=f).reshape(c.shape[0], -1, q)
    y = np.asarray(m, dtype=f).reshape(-1, 1, q) + np.einsum("kij,ksj->ksi", l, z)
    assert l.dtype == f and y.dtype == f
    return np.ascontiguousarray(l.transpose(0, 2, 1)).reshape(-1), y.reshape(-1)


def break_at(C, q, k, j):
    """a copy of packed C whose matrix k has diagonal element j (1-based) lowered so that the Schur complement of the first j - 1 columns
    goes from s to -s / 2 there: the first non-positive pivot is column j, whatever follows"""
    out = np.array(C)
    c = mats(C, q)[k]
    s = np.linalg.cholesky(c)[j - 1, j - 1] ** 2
    out.reshape(-1, q, q)[k, j - 1, j - 1] = c[j - 1, j - 1] - 1.5 * s
    return out


def first_bad_pivot(c):
    """1-based column of the first non-positive pivot of the float64 matrix c in natural order, 0 if none"""
    w = np.array(c, dtype=np.float64)
    for j in range(w.shape[0]):
        if not w[j, j] > 0:
            return j + 1
        w[j + 1:, j + 1:] -= np.outer(w[j + 1:, j], w[j + 1:, j]) / w[j, j]
    return 0


# ---- the joint posterior samples ----------------------------------------------------------------------------------------------------------
SAMPLE_BATCH = 6


@functools.lru_cache(maxsize=None)
def sample_case(n, nquery, dtname):
    """(B, c, d, As, Es, Z): SAMPLE_BATCH GP models of size n with nquery queries each (the construction of _predict_cov_worker.run) and
    SMAX samples per matrix. Computed once, read-only"""
    dt = np.dtype(dtname).type
    B, c, d = LW.inputs(n, SAMPLE_BATCH, dt, True)
    mdl = PC.model(B, c, None, n)
    As, _ = P.queries(mdl, n, SAMPLE_BATCH, nquery, dt, seed=9800 + n)
    Es = PC.prior(mdl, As, n, nquery, dt, seed=9900 + n + nquery)
    Z = np.random.default_rng(4300 + n + nquery).standard_normal((SAMPLE_BATCH, SMAX, nquery)).astype(dt).reshape(-1)
    out = (B, c, d, As, Es, Z)
    for a in out:
        a.setflags(write=False)
    return out


def sample_reference(B, c, d, As, Es, Z, n, nquery):
    """float64: the covariance route's reference (mean, cov and its bounds' terms), and the colour reference on that cov and mean"""
    cref = PC.cov_reference(PC.model(B, c, d, n), As, Es, n, nquery)
    cov = np.ascontiguousarray(cref["cov"].transpose(0, 2, 1)).reshape(-1)
    return cref, reference(cov, cref["mean"], Z, nquery)


# ---- the worker of test_grid_stride_and_chunking ----------------------------------------------------------------------------------------
def bits(api, torch, q, C, m, Z, sl=None):
    """(Y, L, info) as numpy of the matrices sl of the packed case"""
    pick = (lambda a, per: a) if sl is None else (lambda a, per: np.ascontiguousarray(a.reshape(-1, per)[sl]).reshape(-1))
    nz = Z.size // (C.size // (q * q))
    t = lambda a: torch.tensor(np.ascontiguousarray(a)).cuda()  # noqa: E731
    c, mm, z = t(pick(C, q * q)), t(pick(m, q)), t(pick(Z, nz))
    info = torch.full((c.numel() // (q * q),), -7, dtype=torch.int32, device="cuda")
    Y, L = api.colour_batched(q, c, mm, z, info=info)
    torch.cuda.synchronize()
    return Y.cpu().numpy(), L.cpu().numpy(), info.cpu().numpy()


def run_rounds(api, torch, q, batch, dt, part, rejects):
    """a batch of `batch` matrices in one call against the same matrices in calls of `part` (one grid round, one chunk): the same bits,
    rejects (k -> column) included"""
    C, m, Z = case(q, np.dtype(dt).name, batch)
    Z = samples(Z, q, slice(0, 3))
    for k, j in rejects.items():
        C = break_at(C, q, k, j)
    Y, L, info = bits(api, torch, q, C, m, Z)
    expect = np.zeros(batch, dtype=np.int64)
    for k, j in rejects.items():
        expect[k] = j
    assert np.array_equal(info, expect), (q, info[sorted(rejects)], rejects)
    bad = sorted(rejects)
    assert np.isnan(Y.reshape(batch, -1)[bad]).all() and np.isnan(L.reshape(batch, -1)[bad]).all()
    for lo in range(0, batch, part):
        sl = slice(lo, min(lo + part, batch))
        y1, l1, i1 = bits(api, torch, q, C, m, Z, sl)
        assert np.array_equal(y1, Y.reshape(batch, -1)[sl].reshape(-1), equal_nan=True), (q, lo, "Y")
        assert np.array_equal(l1, L.reshape(batch, -1)[sl].reshape(-1), equal_nan=True), (q, lo, "L")
        assert np.array_equal(i1, info[sl]), (q, lo, "info")
    ok = np.array([k for k in range(batch) if k not in rejects])
    ref = reference(C, m, Z, q, idx=ok)
    u = U[np.dtype(dt)]
    check_factor(L, ref, q, u, idx=ok, what=f"{api.colour_kernel_name(dt, q)} batch={batch}")
    check_y(Y, ref, q, u, idx=ok, what=f"{api.colour_kernel_name(dt, q)} batch={batch}")


def run_sample_chunks(api, torch, n, nquery, batch, dt, part):
    """matinv_sample_batched with nothing but Y requested, so that mean and cov live in library scratch and the batch goes in several
    k-range chunks: the bits and the info codes of calls of `part` matrices, each a single chunk. Matrix batch - 3 has E = 0 (info
    n + 1), matrix batch - 2 a first pivot of -1 in M (info 1): both lie in the last chunk, behind a non-zero offset"""
    B, c, d = LW.inputs(n, batch, dt, True)
    mdl = PC.model(B, c, None, n)
    As, _ = P.queries(mdl, n, batch, nquery, dt, seed=9800 + n)
    Es = PC.prior(mdl, As, n, nquery, dt, seed=9900 + n)
    Z = np.random.default_rng(4400 + n).standard_normal(batch * 3 * nquery).astype(dt)
    Es.reshape(batch, -1)[batch - 3] = 0
    c.reshape(batch, n)[batch - 2] = 0
    B.reshape(batch, n, n)[batch - 2, 0, 0] = -1.0
    expect = np.zeros(batch, dtype=np.int64)
    expect[batch - 3], expect[batch - 2] = n + 1, 1
    t = lambda a, per, sl: torch.tensor(np.ascontiguousarray(a.reshape(batch, per)[sl]).reshape(-1)).cuda()  # noqa: E731

    def call(sl):
        cnt = len(range(batch)[sl])
        info = torch.full((cnt,), -7, dtype=torch.int32, device="cuda")
        Y, mean, cov = api.sample_batched(n, t(B, n * n, sl), t(c, n, sl), t(d, n, sl), t(As, nquery * n, sl), t(Es, nquery * nquery, sl),
                                          t(Z, 3 * nquery, sl), info=info, want=("Y",))
        torch.cuda.synchronize()
        assert mean is None and cov is None
        return Y.cpu().numpy().reshape(cnt, -1), info.cpu().numpy()

    Y, info = call(slice(None))
    assert np.array_equal(info, expect), (n, nquery, info, expect)
    assert np.isnan(Y[[batch - 3, batch - 2]]).all() and np.isfinite(np.delete(Y, [batch - 3, batch - 2], axis=0)).all()
    for lo in range(0, batch, part):
        sl = slice(lo, min(lo + part, batch))
        y1, i1 = call(sl)
        assert np.array_equal(y1, Y[sl], equal_nan=True), (n, nquery, lo, "Y")
        assert np.array_equal(i1, info[sl]), (n, nquery, lo, "info")
    print(f"  sample n={n} Q={nquery} batch={batch}: the bits of calls of {part}")


def main():
    import torch
    api = importlib.import_module("cuda-matrix-inversion_amd.api")
    assert os.environ.get("MATINV_TILE_GRID_MULT") == "1" and os.environ.get("MATINV_BLOCKED_WS_MB") == "1"
    # 4000 matrices on a grid of 256 * 12 = 3072 workgroups (launch_colour_tile takes predict_tile_grid): the stride loop runs twice;
    # two of the rejects sit in the second round. Parts of 2000 stay inside one round.
    run_rounds(api, torch, 33, 4000, np.float64, 2000, {5: 17, 3073: 1, 3999: 33})
    run_rounds(api, torch, 33, 4000, np.float32, 2000, {7: 16, 3100: 17, 3998: 33})
    # 20 working copies of 130 * 130 * 8 = 135 200 bytes under a cap of 1 MiB: seven to a chunk, three chunks, two of them with a non-zero
    # `first`. Parts of 5 stay inside one chunk.
    run_rounds(api, torch, 130, 20, np.float64, 5, {7: 1, 13: 97, 19: 130})
    # matinv_sample_batched, Y only: per matrix 33 + 33^2 elements of its own scratch and, for the chunk size, the 97 * (97 + 33) of the
    # covariance route's global form: 13 732 * 8 = 109 856 bytes, nine to a chunk under 1 MiB, five chunks for 40 matrices. Parts of 8
    # are single chunks.
    run_sample_chunks(api, torch, 97, 33, 40, np.float64, 8)
    print("colour-worker ok")


if __name__ == "__main__":
    main()
