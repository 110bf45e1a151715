"""Reference, inputs, bounds and checks of the tests of the leave-one-out cross-validation of the trend GP (tests/test_gpu_trend_loo.py and
tests/test_trend_loo_cpu.py import them), and the worker of test_grid_stride_and_chunking: ONE process under MATINV_TILE_GRID_MULT=1 and
MATINV_BLOCKED_WS_MB=1 (the library reads each switch once per process) that repeats the calls of STRIDE_CASES and compares them bit for
bit with what a default-environment process saved. Exits non-zero at the first failure; prints `trend-loo-worker ok` at the end.

Reference: float64 numpy on the float64 image of exactly what the kernel reads (_trend_worker.model / basis_model / reference). With
Kinv = inv(M), KH = Kinv H, A = H^T KH, P = Kinv - KH A^-1 KH^T and alpha_t = P y_t of _trend_worker.reference:
    var_i = 1 / P_ii          mean_ti = y_ti - alpha_ti / P_ii          logpl_t = sum_i (1/2 log P_ii - 1/2 alpha_ti^2 / P_ii) - n/2 log 2 pi
tests/test_trend_loo_cpu.py confirms them against n brute-force fits on n - 1 points.

Inputs: those of _trend_worker (matrices, vectors, clip, break_three). Two conditions on the inputs are asserted for every case built:
cond2(A) <= COND_A_MAX = 100 (basis_model), and the leverage l_i = 1 - P_ii / Kinv_ii <= LEVERAGE_MAX = 0.8 of every point: P_ii is a
cancelling difference and its relative error grows as 1 / (1 - l_i). If a seed violates either, change the seed, not the cap.

Bounds, first order where a term is small against what it perturbs and exact where it is not, and not fitted. u, eps = (n + 4) u cond2(M)^2,
epsA = (K + 4) u cond2(A)^2, kn, hn, khn, dA = eps kn hn^2, ba (the bound of alpha) as in _trend_worker.
    P_ii    = Kinv_ii - s_i, s_i = r^T A^-1 r with r = row i of KH, w = A^-1 r. Kinv_ii carries eps kn. For s_i the argument of
            _trend_worker's var: ds = 2 w^T dr - w^T dA w and the K x K solve, with ||dr|| <= eps sqrt(K) khn (each of the K columns of
            KH is a product with the computed Kinv), and (K + 2) u s_i for the K-term sum of squares:
            bP := eps kn + 2 ||w|| eps sqrt(K) khn + ||w||^2 dA + (2 epsA + (K + 2) u) s_i + u (|Kinv_ii| + |P_ii|)
    1/P     |1 / (P + d) - 1 / P| <= |d| / (P (P - |d|)) for |d| < P (exact):   bI := bP / (P_ii (P_ii - bP)), infinite when bP >= P_ii
    var     bI + 2 u var_i                                 (the reciprocal and its rounding)
    mean    ba / P_ii + (|alpha_ti| + ba) bI + 3 u |alpha_ti / P_ii| + u |mean_ti|
    logpl   |log(P + d) - log P| <= |d| / (P - |d|) (exact), and for q = alpha^2 / P: dq <= (2 |alpha| ba + ba^2) (1 / P + bI) + alpha^2 bI:
            sum_i (1/2 bP / (P_ii - bP) + 1/2 dq_i) + (n + 4) u sum_i (1/2 |log P_ii| + 1/2 q_i) + u (n log 2 pi + |logpl_t|)
            (the n-term sum, the logarithm and the products round at most n + 4 times each term)
Nothing here is fitted to what the kernels return; tests/test_trend_loo_cpu.py confirms that a float32 numpy evaluation of the same formulas
stays inside the fp32 bounds at every size and (K, D) the GPU tests use, and that the bounds fail wrong results.
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
import _trend_worker as T  # noqa: E402
from conftest import as_mats  # noqa: E402

U = T.U
L = T.L
break_three, clip = T.break_three, T.clip
TILE_SIZES = (2, 15, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96)
GLOBAL_SIZES = (97, 130)
KD = ((1, 1), (3, 17), (16, 16), (4, 33))
KD_1024 = (4, 2)  # n = 1024 runs once per dtype, batch 2
DMAX = T.DMAX
OUTPUTS = ("mean", "var", "logpl")
LOG2PI = T.LOG2PI
LEVERAGE_MAX = 0.8


def batch_of(n):
    return 2 if n > 256 else T.batch_of(n)


def shapes_of(n):
    """the distinct (K, D) of size n after clipping (K < n: a held-out fit needs n - 1 >= K points)"""
    out = []
    for K, D in KD:
        s = (min(clip(K, n), n - 1), D)
        if s not in out:
            out.append(s)
    return out


def loo_terms(bm):
    """what depends on M and H alone: the diagonal of P, s_i, ||w_i|| and the leverage (checked)"""
    KH, Ainv = bm["KH"], bm["Ainv"]
    w = np.einsum("kbc,kic->kib", Ainv, KH)
    s = np.einsum("kib,kib->ki", KH, w)
    kd = np.diagonal(bm["Kinv"], axis1=1, axis2=2)
    pd = kd - s
    return dict(pd=pd, s=s, kd=kd, wn=np.linalg.norm(w, axis=2), leverage=1.0 - pd / kd)


def reference(tref, n, check_leverage=True):
    """the three outputs from a _trend_worker.reference (with or without targets)"""
    ref = {k: v for k, v in tref.items() if k not in ("a", "g", "e", "aKa", "w", "rar", "var", "akamag", "mean", "meanmag")}  # no queries
    ref.update(loo_terms(tref))
    if check_leverage:
        assert (ref["leverage"] <= LEVERAGE_MAX).all(), ("leverage too large: change the seed", n, tref["K"], float(ref["leverage"].max()))
    pd = ref["pd"]
    ref["var"] = 1.0 / pd
    if "y" in tref:
        al, y = tref["alpha"], tref["y"]
        ref["mean"] = y - al / pd[:, None, :]
        ref["logpl"] = (0.5 * np.log(pd)[:, None, :] - 0.5 * al ** 2 / pd[:, None, :]).sum(axis=2) - 0.5 * n * LOG2PI
    return ref


# The seeds of the basis vectors and targets are those of _trend_worker.case, but for the (n, K) whose draw breaks the leverage condition
# in one of the four (dtype, with_c) cases: those take the first later seed (steps of 100000) that keeps it in all four.
SEED_SHIFT = {(15, 3): 1, (33, 16): 17}  # unshifted: leverage 0.823 and 0.844; shifted: 0.733 and 0.783


@functools.lru_cache(maxsize=None)
def case(n, dtname, with_c, K, check_leverage=True):
    """the shared case of size n with K basis vectors: (B, c, Hs, Ys, reference) with DMAX targets per matrix, on the matrices of
    _trend_worker.matrices. Computed once; nobody writes into it; `take` slices the reference, _trend_worker.first the targets"""
    dt = np.dtype(dtname).type
    B, c, mdl = T.matrices(n, dtname, with_c)
    batch = B.size // (n * n)
    seed = 8000 + 13 * n + 101 * K + (1 if with_c else 0) + 100000 * SEED_SHIFT.get((n, K), 0)
    Hs, Ys, _, _, _ = T.vectors(n, batch, K, DMAX, 1, dt, seed)
    for x in (Hs, Ys):
        x.setflags(write=False)
    tref = T.reference(T.basis_model(mdl, Hs, n, K), Ys, None, None, None, n, K, DMAX, 0)
    return B, c, Hs, Ys, reference(tref, n, check_leverage)


def take(ref, tsel):
    """the reference of the targets tsel (a count, a slice or a list) of every matrix; 0: without targets"""
    out = dict(ref)
    if isinstance(tsel, int) and tsel == 0:
        for k in ("y", "Ky", "beta", "alpha", "quad", "quadmag", "logml", "mean", "logpl"):
            out.pop(k, None)
        return out
    tsel = slice(0, tsel) if isinstance(tsel, int) else tsel
    for k in ("y", "Ky", "beta", "alpha", "quad", "quadmag", "logml", "mean", "logpl"):
        if k in ref:
            out[k] = ref[k][:, tsel]
    return out


def p_bound(ref, n, u):
    """bP of the module docstring, per (matrix, point)"""
    K = ref["K"]
    eps = ((n + 4) * u * ref["cond"] ** 2)[:, None]
    epsA = ((K + 4) * u * ref["condA"] ** 2)[:, None]
    kn, hn, khn = ref["knorm"][:, None], ref["hnorm"][:, None], ref["khnorm"][:, None]
    dA = eps * kn * hn ** 2
    return eps * kn + 2 * ref["wn"] * eps * np.sqrt(K) * khn + ref["wn"] ** 2 * dA + (2 * epsA + (K + 2) * u) * ref["s"] + \
        u * (np.abs(ref["kd"]) + np.abs(ref["pd"]))


def bounds(ref, n, u):
    """dict of the bounds of the module docstring, each broadcastable against its output"""
    pd = ref["pd"]
    bP = p_bound(ref, n, u)
    with np.errstate(divide="ignore", invalid="ignore"):
        bI = np.where(bP < pd, bP / (pd * (pd - bP)), np.inf)
        bL = np.where(bP < pd, bP / (pd - bP), np.inf)
    out = {"var": bI + 2 * u * ref["var"], "P": bP}
    if "y" in ref:
        ba = T.bounds({k: v for k, v in ref.items() if k not in ("mean", "var")}, n, u)["alpha"]  # (k, t, 1)
        al = np.abs(ref["alpha"])
        P, I = pd[:, None, :], bI[:, None, :]
        out["mean"] = ba / P + (al + ba) * I + 3 * u * al / P + u * np.abs(ref["mean"])
        q = al ** 2 / P
        dq = (2 * al * ba + ba ** 2) * (1 / P + I) + al ** 2 * I
        out["logpl"] = (0.5 * bL[:, None, :] + 0.5 * dq).sum(axis=2) + (n + 4) * u * (0.5 * np.abs(np.log(P)) + 0.5 * q).sum(axis=2) + \
            u * (n * LOG2PI + np.abs(ref["logpl"]))
    return out


def shapes(ref, n):
    D = ref["y"].shape[1] if "y" in ref else 0
    return dict(mean=(-1, D, n), var=(-1, n), logpl=(-1, D))


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
        assert np.isfinite(got).all(), name
        err = np.abs(got.astype(np.longdouble) - ref[name]).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            rs[name] = np.where(err == 0, 0.0, err / b[name])
    return rs


def check(out, ref, n, u, idx=None, what="", factor=1.0):
    """every given output within factor * bound; prints err / bound first. Returns {name: worst err / bound}"""
    rs = ratios(out, ref, n, u, idx)
    worst = {k: float(v.max()) for k, v in rs.items()}
    print(f"  {what} n={n} K={ref['K']} D={shapes(ref, n)['logpl'][1]} cond={ref['cond'].max():.2f} condA={ref['condA'].max():.2f} "
          f"leverage={ref['leverage'].max():.3f} err/bound: " + " ".join(f"{k}={v:.4f}" for k, v in worst.items()))
    for k, v in rs.items():
        assert np.isfinite(v).all() and (v <= factor).all(), (what, n, k, float(np.nanmax(v)))
    return worst


def reference_of(B, c, Hs, Ys, n, K, D, idx=None, check_leverage=True):
    """the LOO reference of packed inputs of their own (not a shared case), for the matrices idx"""
    bm = T.basis_model(T.model(B, c, n, idx=idx), Hs, n, K, idx=idx)
    return reference(T.reference(bm, Ys if D else None, None, None, None, n, K, D, 0, idx=idx), n, check_leverage)


def float32_evaluation(B, c, Hs, Ys, n, K, D):
    """the reference formulas evaluated in float32 numpy on the float32 inputs: what any fp32 implementation of them may expect"""
    f = np.float32
    m = as_mats(B, n).astype(f)
    M = np.tril(m) + np.tril(m, -1).transpose(0, 2, 1)
    if c is not None:
        idx = np.arange(n)
        M[:, idx, idx] = M[:, idx, idx] + np.asarray(c, dtype=f).reshape(-1, n)
    Kinv = np.linalg.inv(M)
    H = np.asarray(Hs, dtype=f).reshape(-1, K, n).transpose(0, 2, 1)
    y = np.asarray(Ys, dtype=f).reshape(-1, D, n)
    KH = Kinv @ H
    Ainv = np.linalg.inv(H.transpose(0, 2, 1) @ KH)
    pd = np.diagonal(Kinv, axis1=1, axis2=2) - np.einsum("kib,kbc,kic->ki", KH, Ainv, KH)
    beta = np.einsum("kbc,kic,kti->ktb", Ainv, KH, y)
    alpha = np.einsum("kij,ktj->kti", Kinv, y) - np.einsum("kib,ktb->kti", KH, beta)
    var = f(1) / pd
    mean = y - alpha * var[:, None, :]
    logpl = (f(0.5) * np.log(pd)[:, None, :] - f(0.5) * alpha * alpha * var[:, None, :]).sum(axis=2) - f(0.5 * n * LOG2PI)
    out = dict(mean=mean, var=var, logpl=logpl)
    assert all(v.dtype == f for v in out.values())
    return {k: v.reshape(-1) for k, v in out.items()}


def unit_basis(n, cols, dt):
    """(B, Hs) of one matrix: B = I and H = the unit vectors e_j, j in cols. Every operation of the kernels on them is exact."""
    H = np.zeros((len(cols), n), dtype=dt)
    for b, j in enumerate(cols):
        H[b, j] = 1
    return np.eye(n, dtype=dt).reshape(-1), H.reshape(-1)


def degenerate_columns(n):
    """the K = 1 and K = 2 unit bases of the exact-degenerate test at size n: the first and last lane of the first and last tile, one
    row in between, and a pair in two tiles"""
    last = 16 * ((n - 1) // 16)
    ones = sorted({0, min(15, n - 1), last, n - 1, min(5, n - 1)})
    sets = [(j,) for j in ones]
    if n > 4:
        sets.append((3, n - 1))
        sets.append((n - 1, 3))
    return sets


def model_order_pd(n, cols, dt):
    """P_ii of unit_basis in a model of the kernels' order of operations in dt: W = -I; T_H = W H; A = -H^T T_H; A = L L^T by square
    roots; U = T_H L^-T; P_ii = -W_ii - sum_b U_ib^2"""
    f = np.dtype(dt).type
    B, Hs = unit_basis(n, cols, dt)
    K = len(cols)
    W = -np.linalg.inv(B.reshape(n, n)).astype(f)
    H = Hs.reshape(K, n).T
    TH = (W @ H).astype(f)
    A = (-(H.T @ TH)).astype(f)
    Linv = np.linalg.inv(np.linalg.cholesky(A)).astype(f)
    Um = (TH @ Linv.T).astype(f)
    return (-np.diagonal(W) - (Um * Um).sum(axis=1, dtype=f)).astype(f)


# ---- GPU helpers (torch and the package are imported by the caller) ---------------------------------------------------------------------
def run(api, torch, n, B, c, Hs, Ys, want=OUTPUTS, K=None, D=None):
    """api.trend_loo_batched on packed numpy inputs: (dict of the numpy outputs in `want`, info). Asserts that no input changed a bit"""
    batch = B.size // (n * n)
    host = [None if x is None else np.ascontiguousarray(x) for x in (B, c, Hs, Ys)]
    dev = [None if x is None else torch.tensor(x).cuda() for x in host]
    info = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
    res = api.trend_loo_batched(n, *dev, batchSize=batch, info=info, want=want, nbasis=K, ntarget=D)
    torch.cuda.synchronize()
    for h, d in zip(host, dev):
        assert h is None or np.array_equal(d.cpu().numpy(), h, equal_nan=True), "an input was modified"
    out = {k: (None if v is None else v.cpu().numpy()) for k, v in zip(OUTPUTS, res)}
    assert all((out[k] is not None) == (k in want) for k in OUTPUTS)
    return {k: v for k, v in out.items() if v is not None}, info.cpu().numpy()


same_bits = T.same_bits


def check_with_rejects(out, info, B, c, Hs, Ys, n, K, D, dt, want_info, what=""):
    """info exactly as expected, every output NaN exactly at the matrices of want_info, finite and within the bounds elsewhere"""
    batch = info.size
    bad = sorted(want_info)
    ok = np.array([k for k in range(batch) if k not in bad])
    expect = np.zeros(batch, dtype=np.int64)
    for k, v in want_info.items():
        expect[k] = v
    assert np.array_equal(info, expect), (what, n, info[bad], np.flatnonzero(info != expect)[:10])
    for k, v in out.items():
        o = v.reshape(batch, -1)
        assert np.isnan(o[bad]).all() and np.isfinite(o[ok]).all(), (what, n, k)
    return check(out, reference_of(B, c, Hs, Ys, n, K, D, idx=ok), n, U[np.dtype(dt)], idx=ok, what=what)


# (n, batch, K, D, dtype, with_c, matrices broken by break_three, matrix with h_2 = h_1). The tile grid under MATINV_TILE_GRID_MULT=1 is
# 256 * 12 = 3072 workgroups: 4000 matrices are two rounds of the stride loop, with the rejects in the second. At n = 130 twenty working
# copies of (130^2 + 130 (4 + 17) + 4 * 17) * 8 = 157 584 bytes under a cap of 1 MiB are six to a chunk: four chunks, three of them with
# a non-zero `first`.
STRIDE_CASES = (
    (16, 4000, 3, 3, np.float64, True, (3073, 3500, 3999), 3300),
    (16, 4000, 3, 3, np.float32, False, (3100, 3600, 3998), 3200),
    (64, 4000, 4, 17, np.float64, False, (3080, 3400, 3997), 3333),
    (64, 4000, 4, 17, np.float32, True, (3075, 3700, 3996), 3111),
    (130, 20, 4, 17, np.float64, True, (7, 13, 19), 11),
    (130, 20, 4, 17, np.float32, False, (6, 12, 18), 10),
)


def stride_inputs(n, batch, K, D, dt, with_c, rejects_at, singular_at):
    """(B, c, Hs, Ys, want_info) of a stride case; deterministic"""
    B, c, _ = L.inputs(n, batch, dt, with_c)
    Hs, Ys, _, _, _ = T.vectors(n, batch, K, D, 1, dt, 9100 + n)
    want_info = dict(break_three(B, c, n, rejects_at))
    h = Hs.reshape(batch, K, n)
    h[singular_at, 1] = h[singular_at, 0]
    want_info[singular_at] = n + 2
    return B, c, Hs, Ys, want_info


def stride_key(i, name):
    return f"case{i}_{name}"


def main():
    import torch
    api = importlib.import_module("cuda-matrix-inversion_amd.api")
    assert os.environ.get("MATINV_TILE_GRID_MULT") == "1" and os.environ.get("MATINV_BLOCKED_WS_MB") == "1"
    saved = np.load(sys.argv[1])
    for i, (n, batch, K, D, dt, with_c, rejects_at, singular_at) in enumerate(STRIDE_CASES):
        B, c, Hs, Ys, want_info = stride_inputs(n, batch, K, D, dt, with_c, rejects_at, singular_at)
        out, info = run(api, torch, n, B, c, Hs, Ys, K=K, D=D)
        assert np.array_equal(info, saved[stride_key(i, "info")]), (n, dt)
        same_bits(out, {k: saved[stride_key(i, k)] for k in OUTPUTS}, (n, dt, "against the default environment"))
        print(f"  {api.trend_loo_kernel_name(dt, n)} batch={batch}: the bits of the default call")
    print("trend-loo-worker ok")


if __name__ == "__main__":
    main()
