"""Reference, inputs, bounds and checks of the tests of the gradients of the trend GP's restricted log marginal likelihood
(tests/test_gpu_trend_grad.py and tests/test_trend_grad_cpu.py import them), and the worker of test_grid_stride_and_chunking: ONE process
under MATINV_TILE_GRID_MULT=1 and MATINV_BLOCKED_WS_MB=1 (the library reads each switch once per process), so that the tile kernels'
stride loop runs several rounds on the same per-workgroup workspace and the global launcher takes several chunks. The worker is given a
file of the outputs of the same calls made under the default switches, which the test has checked against the reference before: it
asserts equal bits, exits non-zero at the first failure and starts nothing after it; prints `trend-grad-worker ok` at the end.

Reference: float64 numpy on the float64 image of exactly what the kernel reads (_trend_worker.model and _logml_grad_worker.sym_lower: the
lower triangles of B and of every dM_p mirrored). With the quantities of _trend_worker (Kinv, H, KH = Kinv H, A = H^T KH, alpha_t, beta_t,
logml_t), L_A the Cholesky factor of A, U = KH L_A^-T (so U U^T = KH A^-1 KH^T) and P = Kinv - U U^T:
    G = sum_t alpha_t alpha_t^T - D P       grad_p = 1/2 sum_ij G_ij dM_p[i, j]      gradc_i = 1/2 G_ii
grad and gradc are the derivatives of sum_t logml_t: d(y^T P y) = -alpha^T dM alpha, d log det M = tr(Kinv dM) and
d log det A = -tr(KH A^-1 KH^T dM); H does not depend on the parameters (tests/test_trend_grad_cpu.py checks it against central finite
differences of _trend_worker's reference).

Inputs: B, c, Hs, Ys of _trend_worker.case (K clipped by n as _trend_worker.clip does, cond2(A) <= 100 asserted on every case); dM of
_logml_grad_worker.derivs.

Bounds, first order and not fitted, in the notation of _trend_worker: u = 2^-53 (fp64) or 2^-24 (fp32), eps = (n + 4) u cond2(M)^2,
epsA = (K + 4) u cond2(A)^2, kn = ||Kinv||, hn = ||H||, khn = ||Kinv H||, an = ||A^-1|| (2-norms), ba_t the bound of an element of
alpha_t of _trend_worker.bounds.
    logml, alpha, beta   those of _trend_worker.bounds
    d(alpha alpha^T)     ||d alpha_t||_2 <= sqrt(n) ba_t, so the error of alpha_t alpha_t^T is at most 2 ||alpha_t|| sqrt(n) ba_t in the
                         Frobenius norm, which the factor 1/2 of the outputs halves:  sa := sum_t ||alpha_t|| sqrt(n) ba_t
    d Kinv               eps kn in the 2-norm, eps ||Kinv||_F in the Frobenius norm (as in _multi_target_grad_worker)
    d(U U^T)             U U^T = KH A^-1 KH^T: the two factors KH bring 2 eps khn^2 an; A^-1 brings khn^2 times
                         ||d(A^-1)|| <= an^2 eps kn hn^2 + epsA an (covbeta of _trend_worker):
                         uu := 2 eps khn^2 an + (an eps kn hn^2 + epsA) khn^2 an      (2-norm; rank K, so sqrt(K) uu bounds the Frobenius norm)
    gradc   |gradc^_i - gradc_i| <= sa + D (eps kn + uu) + (D + K + 2) u 1/2 gmag_ii
    grad    |grad^_p - grad_p|   <= (sa + D (eps ||Kinv||_F + sqrt(K) uu)) ||dM_p||_F + (n^2 + D + K) u sum_ij gmag_ij |dM_p[i, j]|
            gmag_ij = sum_t |alpha_ti alpha_tj| + D (|Kinv_ij| + sum_b |U_ib U_jb|)
The second terms are the rounding of what is summed: G_ij is a sum of D + K products and one scaled element; grad adds the n^2 products
with dM_p and their sum in any order. Nothing here is fitted to what the kernels return; tests/test_trend_grad_cpu.py confirms that a
float32 numpy evaluation of the same formulas stays inside the fp32 bounds at every size and (K, D, P) the GPU tests use, and that the
bounds fail wrong results.
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
import _multi_target_grad_worker as MG  # noqa: E402
import _trend_worker as T  # noqa: E402
from conftest import as_mats  # noqa: E402

U = T.U
break_three = T.break_three
first, same_bits, clip = T.first, T.same_bits, T.clip
derivs, sym_lower, first_derivs = MG.derivs, MG.sym_lower, MG.first_derivs
TILE_SIZES, GLOBAL_SIZES, batch_of = T.TILE_SIZES, T.GLOBAL_SIZES, T.batch_of
KDP = ((1, 1, 1), (3, 17, 1), (16, 16, 2), (4, 33, 3))
KDP_1024 = (4, 17, 1)  # n = 1024 runs once per dtype
DMAX, PMAX = T.DMAX, 3
OUTPUTS = ("grad", "gradc", "logml", "alpha", "beta")
QUERY_KEYS = ("a", "g", "e", "aKa", "w", "rar", "var", "akamag", "mean", "meanmag")


def shapes_of(n):
    """the distinct (K, D, P) of size n after clipping K"""
    out = []
    for K, D, P in KDP:
        s = (clip(K, n), D, P)
        if s not in out:
            out.append(s)
    return out


def reference(tr, dMs, n, P, idx=None, projection=True):
    """tr: the _trend_worker reference of the D targets (T.reference / T.take); adds P, G, grad, gradc and the terms of the bounds.
    dMs None: without grad. idx: the matrices tr holds, when dMs holds more. projection=False leaves the U U^T term out (the zero-mean
    G on the trend's alpha): what the tests of the projection hold the true reference against"""
    ref = {k: v for k, v in tr.items() if k not in QUERY_KEYS}
    a, Kinv = tr["alpha"], tr["Kinv"]
    D = a.shape[1]
    Um = tr["KH"] @ np.linalg.inv(np.linalg.cholesky(tr["A"])).transpose(0, 2, 1)
    UU = Um @ Um.transpose(0, 2, 1) if projection else np.zeros_like(Kinv)
    Gm = np.einsum("kti,ktj->kij", a, a) - D * (Kinv - UU)
    ref.update(Umat=Um, Pmat=Kinv - UU, G=Gm, gradc=0.5 * np.einsum("kii->ki", Gm),
               gmag=np.einsum("kti,ktj->kij", np.abs(a), np.abs(a)) + D * (np.abs(Kinv) + np.abs(Um) @ np.abs(Um).transpose(0, 2, 1)))
    if dMs is not None and P:
        dM = sym_lower(dMs, n).reshape(-1, P, n, n)
        if idx is not None:
            dM = dM[idx]
        ref.update(dM=dM, grad=0.5 * np.einsum("kij,kpij->kp", Gm, dM))
    return ref


def sum_logml(M, Hs, Ys, n, K, D):
    """sum_t logml_t of ONE matrix M (n x n float64, symmetric) by _trend_worker's reference: what grad and gradc differentiate"""
    bm = T.basis_model(T.model(np.ascontiguousarray(M).reshape(-1), None, n), Hs, n, K)
    return float(T.reference(bm, Ys, None, None, None, n, K, D, 0)["logml"].sum())


@functools.lru_cache(maxsize=None)
def case(n, dtname, with_c, K):
    """the shared case of size n with K basis vectors: (B, c, Hs, Ys, dMs, reference) with DMAX targets and PMAX derivative matrices per
    matrix; B, c, Hs, Ys and the trend reference are those of _trend_worker.case. Computed once; nobody writes into it"""
    B, c, Hs, Ys, _, _, _, full = T.case(n, dtname, with_c, K)
    dMs = derivs(n, batch_of(n), PMAX, np.dtype(dtname).type)
    dMs.setflags(write=False)
    return B, c, Hs, Ys, dMs, full


def take(full, dMs, n, D, P):
    """the reference of the first D targets and the first P derivative matrices of the shared case"""
    return reference(T.take(full, D, 0), first_derivs(dMs, n, PMAX, P) if P else None, n, P)


def bounds(ref, n, u):
    """dict of the bounds of the module docstring: grad[k, p], gradc[k, i], logml[k, t], alpha[k, t, 1], beta[k, t, 1]"""
    tb = T.bounds(ref, n, u)
    out = {k: tb[k] for k in ("logml", "alpha", "beta")}
    K = ref["K"]
    D = ref["alpha"].shape[1]
    eps = (n + 4) * u * ref["cond"] ** 2
    epsA = (K + 4) * u * ref["condA"] ** 2
    kn, hn, khn, an = ref["knorm"], ref["hnorm"], ref["khnorm"], ref["anorm"]
    sa = (np.linalg.norm(ref["alpha"], axis=2) * np.sqrt(n) * tb["alpha"][:, :, 0]).sum(axis=1)
    uu = 2 * eps * khn ** 2 * an + (an * eps * kn * hn ** 2 + epsA) * khn ** 2 * an
    out["gradc"] = (sa + D * (eps * kn + uu))[:, None] + (D + K + 2) * u * 0.5 * np.einsum("kii->ki", ref["gmag"])
    if "dM" in ref:
        kf = np.linalg.norm(ref["Kinv"], "fro", axis=(1, 2))
        dmf = np.linalg.norm(ref["dM"], "fro", axis=(2, 3))
        mag = (ref["gmag"][:, None] * np.abs(ref["dM"])).sum(axis=(2, 3))
        out["grad"] = (sa + D * (eps * kf + np.sqrt(K) * uu))[:, None] * dmf + (n * n + D + K) * u * mag
    return out


def shapes(ref, n):
    D = ref["alpha"].shape[1]
    P = ref["dM"].shape[1] if "dM" in ref else 0
    return dict(grad=(-1, P), gradc=(-1, n), logml=(-1, D), alpha=(-1, D, n), beta=(-1, D, ref["K"]))


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
    shp = shapes(ref, n)
    worst = {k: float(v.max()) for k, v in rs.items()}
    print(f"  {what} n={n} K={ref['K']} D={shp['logml'][1]} P={shp['grad'][1]} cond={ref['cond'].max():.2f} "
          f"condA={ref['condA'].max():.2f} err/bound: " + " ".join(f"{k}={v:.4f}" for k, v in worst.items()))
    for k, v in rs.items():
        assert np.isfinite(v).all() and (v <= factor).all(), (what, n, k, float(np.nanmax(v)))
    return worst


def float32_evaluation(B, c, Hs, Ys, dMs, n, K, D, P):
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
    A = H.transpose(0, 2, 1) @ KH
    Ainv = np.linalg.inv(A)
    beta = np.einsum("kbc,kic,kti->ktb", Ainv, KH, y)
    alpha = np.einsum("kij,ktj->kti", Kinv, y) - np.einsum("kib,ktb->kti", KH, beta)
    quad = np.einsum("kti,kti->kt", y, alpha)
    ld = np.linalg.slogdet(M)[1] + np.linalg.slogdet(A)[1]
    logml = f(-0.5) * (quad + ld[:, None] + f(n - K) * f(T.LOG2PI))
    Pm = Kinv - KH @ Ainv @ KH.transpose(0, 2, 1)
    Gm = np.einsum("kti,ktj->kij", alpha, alpha) - f(D) * Pm
    out = dict(gradc=f(0.5) * np.einsum("kii->ki", Gm), logml=logml, alpha=alpha, beta=beta)
    if P:
        dm = np.tril(as_mats(dMs, n).astype(f))
        dM = (dm + np.tril(dm, -1).transpose(0, 2, 1)).reshape(-1, P, n, n)
        out["grad"] = f(0.5) * np.einsum("kij,kpij->kp", Gm, dM)
    assert all(v.dtype == f for v in out.values())
    return {k: v.reshape(-1) for k, v in out.items()}


# ---- GPU helpers (torch and the package are imported by the caller) ---------------------------------------------------------------------
def run(api, torch, n, B, c, Hs, Ys, dMs, want=OUTPUTS, K=None, D=None, P=None):
    """api.trend_grad_batched on packed numpy inputs: (dict of the numpy outputs in `want`, info). Asserts that no input changed a bit"""
    batch = B.size // (n * n)
    host = [None if x is None else np.ascontiguousarray(x) for x in (B, c, Hs, Ys, dMs)]
    dev = [None if x is None else torch.tensor(x).cuda() for x in host]
    info = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
    res = api.trend_grad_batched(n, *dev, batchSize=batch, info=info, want=want, nbasis=K, ntarget=D, nparam=P)
    torch.cuda.synchronize()
    for h, d in zip(host, dev):
        assert h is None or np.array_equal(d.cpu().numpy(), h, equal_nan=True), "an input was modified"
    out = {k: (None if v is None else v.cpu().numpy()) for k, v in zip(OUTPUTS, res)}
    assert all((out[k] is not None) == (k in want) for k in OUTPUTS)
    return {k: v for k, v in out.items() if v is not None}, info.cpu().numpy()


def reference_of(B, c, Hs, Ys, dMs, n, K, D, P, idx=None):
    """the reference of a batch of its own, for the matrices idx"""
    tr = T.reference(T.basis_model(T.model(B, c, n, idx=idx), Hs, n, K, idx=idx), Ys, None, None, None, n, K, D, 0, idx=idx)
    return reference(tr, dMs, n, P, idx=idx)


def check_with_rejects(out, info, B, c, Hs, Ys, dMs, n, K, D, P, dt, want_info, what=""):
    """info as expected (want_info: {matrix: code}, the rank-deficient bases with their n + b among them), every output NaN exactly at
    those matrices, finite and within the bounds elsewhere"""
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
    return check(out, reference_of(B, c, Hs, Ys, dMs, n, K, D, P, idx=ok), n, U[np.dtype(dt)], idx=ok, what=what)


# the calls of test_grid_stride_and_chunking: (n, batch, K, D, P, dtype, with c, rejects, the matrix whose h_2 repeats h_1). 4000 matrices
# on a grid of 256 * 12 = 3072 workgroups run the stride loop twice (under the 1 MiB cap the workspace of D n elements per workgroup holds
# the grid to fewer workgroups still, so every slice is reused many times); the broken matrices sit beyond the first round. 20 working
# copies of (130^2 + 130 (4 + 33) + 4 * 33) * 8 = 174 736 bytes under a cap of 1 MiB: six to a chunk, four chunks, three of them with a
# non-zero `first`.
STRIDE_CASES = ((33, 4000, 3, 33, 2, np.float64, True, (3073, 3500, 3999), 3300),
                (33, 4000, 3, 33, 1, np.float32, False, (3100, 3600, 3998), 3200),
                (130, 20, 4, 33, 2, np.float64, True, (7, 13, 19), 11))


def stride_inputs(n, batch, K, D, P, dt, with_c, rejects_at, singular_at):
    """(B, c, Hs, Ys, dMs, want_info): break_three's rejects, and n + 2 for the matrix whose second basis vector repeats the first"""
    B, c, _ = T.L.inputs(n, batch, dt, with_c)
    Hs, Ys = T.vectors(n, batch, K, D, 1, dt, 8600 + n)[:2]
    dMs = derivs(n, batch, P, dt)
    want_info = break_three(B, c, n, rejects_at)
    h = Hs.reshape(batch, K, n)
    h[singular_at, 1] = h[singular_at, 0]
    want_info[singular_at] = n + 2
    return B, c, Hs, Ys, dMs, want_info


def stride_key(i, k):
    return f"case{i}_{k}"


def main():
    import torch
    api = importlib.import_module("cuda-matrix-inversion_amd.api")
    assert os.environ.get("MATINV_TILE_GRID_MULT") == "1" and os.environ.get("MATINV_BLOCKED_WS_MB") == "1"
    saved = np.load(sys.argv[1])
    for i, (n, batch, K, D, P, dt, with_c, rejects_at, singular_at) in enumerate(STRIDE_CASES):
        B, c, Hs, Ys, dMs, _ = stride_inputs(n, batch, K, D, P, dt, with_c, rejects_at, singular_at)
        # without alpha the groups come back from the per-workgroup workspace, with it from dAlpha
        out, info = run(api, torch, n, B, c, Hs, Ys, dMs, want=("grad", "gradc", "logml", "beta"), K=K)
        assert np.array_equal(info, saved[stride_key(i, "info")]), (i, "info")
        same_bits(out, {k: saved[stride_key(i, k)] for k in out}, (i, "workspace"))
        out, _ = run(api, torch, n, B, c, Hs, Ys, dMs, K=K)
        same_bits(out, {k: saved[stride_key(i, k)] for k in out}, (i, "alpha"))
        print(f"  {api.trend_grad_kernel_name(dt, n)} batch={batch} K={K} D={D} P={P}: the bits of the default call")
    print("trend-grad-worker ok")


if __name__ == "__main__":
    main()
