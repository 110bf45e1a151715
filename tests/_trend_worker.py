"""Reference, inputs, bounds and checks of the tests of the GP regression with a linear trend (tests/test_gpu_trend.py and
tests/test_trend_cpu.py import them), and the worker of test_grid_stride_and_chunking: ONE process under MATINV_TILE_GRID_MULT=1 and
MATINV_BLOCKED_WS_MB=1 (the library reads each switch once per process), so that the tile kernels' stride loop runs twice and the global
launcher takes several chunks. Exits non-zero at the first failure and starts nothing after it; prints `trend-worker ok` at the end.

Reference: float64 numpy on the float64 image of exactly what the kernel reads (_logml_grad_worker.image). With Kinv = inv(M), H the n x K
matrix of the basis vectors, A = H^T Kinv H, and for target t and query j of matrix k
    beta_t = A^-1 H^T Kinv y_t        covbeta = A^-1         alpha_t = Kinv (y_t - H beta_t)       quad_t = y_t^T alpha_t
    logml_t = -(quad_t + log det M + log det A + (n - K) log 2 pi) / 2
    mean[t, j] = a_j^T alpha_t + g_j^T beta_t
    var[j] = e_j - a_j^T Kinv a_j + r_j^T A^-1 r_j,   r_j = g_j - H^T Kinv a_j
Both log-determinants are 2 sum log of the diagonal of a Cholesky factor taken in longdouble for n <= 96 (_whiten_worker.logdet_longdouble),
of the float64 factor beyond; that of A always in longdouble (K <= 16).

Inputs: B and c of _loo_worker.inputs; h_1 = 1, the other basis vectors N(0, 1); y, a ~ N(0, 1); g_j1 = 1, the rest N(0, 1);
e_j = a_j^T Kinv a_j - r_j^T A^-1 r_j + U(0.1, 1), so that every reference variance is >= 0.1. With random H the matrix A degrades fast as
K approaches n (cond2(A) = 1.4e5 at n = K = 16), so K is clipped: 1 at n = 1, at most 3 up to n = 32, 16 only from n = 33 (`clip`). Every
case built asserts cond2(A) <= COND_A_MAX = 100: a condition on the inputs. If a seed violates it, change the seed, not the cap.

Bounds, first order and not fitted. u = 2^-53 (fp64) or 2^-24 (fp32); eps = (n + 4) u cond2(M)^2 bounds the relative error of everything
that goes through the computed Kinv (as in _logml_grad_worker: ||dKinv||_2 <= eps ||Kinv||_2, and the error of a product Kinv x is at most
eps ||Kinv x||_2); epsA = (K + 4) u cond2(A)^2 is the same for the K x K solve. Norms are 2-norms; kn = ||Kinv||, hn = ||H||,
khn = ||Kinv H||, an = ||A^-1||.
    dA      the computed A is A + dA, ||dA|| <= eps kn hn^2; the computed H^T Kinv x is off by at most eps kn hn ||x||.
    beta    beta = A^-1 b, b = H^T Kinv y: d beta = A^-1 (db - dA beta) and the error of the solve itself,
            |beta^_b - beta_b| <= bb := an eps kn hn (||y_t|| + hn ||beta_t||) + epsA ||beta_t||
    covbeta d(A^-1) = -A^-1 dA A^-1 and the error of the inversion:  |.| <= an^2 eps kn hn^2 + epsA an
    alpha   alpha^ = (Kinv y)^ - (Kinv H)^ beta^, two products that cancel: each keeps its own error, beta^ brings bb, and the K-term
            correction sum rounds K + 4 times:
            |alpha^_i - alpha_i| <= ba := eps (||Kinv y_t|| + khn ||beta_t||) + khn sqrt(K) bb + (K + 4) u khn ||beta_t||
            (sqrt(K) bb bounds ||d beta||_2 by its K components)
    quad    quad^ = sum_i y_i alpha^_i:  |.| <= sqrt(n) ||y_t|| ba + 2 n u sum_i |y_i alpha_i| + u |quad|
            (Cauchy-Schwarz with ||d alpha||_2 <= sqrt(n) ba, then the rounding of the n-term sum and the last rounding)
    logdet  of M: n^2 u cond2(M) + n u max(1, |logdet M|) (+ 2 n u for the global form, as in _multi_target_worker);
            of A: d log det A = tr(A^-1 dA): K an eps kn hn^2, and K^2 u cond2(A) + K u max(1, |logdet A|) for its own factorisation
    logml   (b_quad + b_logdetM + b_logdetA) / 2 + u (|ld| + |s| + 2 (n - K) log 2 pi + |s + (n - K) log 2 pi|) / 2,
            ld = logdet M + logdet A, s = quad + ld: half of the three, and the roundings of its own terms
    mean    |.| <= sqrt(n) ||a_j|| ba + ||g_j|| sqrt(K) bb + (n + K) u (sum_i |a_ji alpha_ti| + sum_b |g_jb beta_tb|) + u |mean|
    var     the bound of _predict_worker for e - a^T Kinv a, and for s = r^T A^-1 r with w = A^-1 r and dr <= eps kn hn ||a||:
            ds = 2 w^T dr - w^T dA w and the K x K solve:
            eps kn ||a||^2 + 2 n u sum_ij |a_i Kinv_ij a_j| + u (|e| + |e - a^T Kinv a|)
              + 2 ||w|| (eps kn hn ||a|| + u ||g||) + ||w||^2 eps kn hn^2 + (2 epsA + (K + 2) u) s + u |var|
Nothing here is fitted to what the kernels return; tests/test_trend_cpu.py confirms that a float32 numpy evaluation of the same formulas
stays inside the fp32 bounds at every size and (K, D, Q) the GPU tests use, and that the bounds fail wrong results.
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
KDQ = ((1, 1, 1), (3, 17, 16), (16, 16, 17), (4, 33, 33))
KDQ_1024 = (4, 17, 16)  # n = 1024 runs once per dtype
DMAX = QMAX = 33
OUTPUTS = ("beta", "covbeta", "alpha", "quad", "logml", "mean", "var")
LOG2PI = W.LOG2PI
COND_A_MAX = 100.0


def clip(K, n):
    """the K the tests use at size n for a nominal K"""
    return 1 if n == 1 else (min(K, 3) if n <= 32 else K)


def shapes_of(n):
    """the distinct (K, D, Q) of size n after clipping"""
    out = []
    for K, D, Q in KDQ:
        s = (clip(K, n), D, Q)
        if s not in out:
            out.append(s)
    return out


@functools.lru_cache(maxsize=None)
def matrices(n, dtname, with_c, batch=None):
    """(B, c, model) of size n: computed once, nobody writes into it"""
    dt = np.dtype(dtname).type
    B, c, _ = L.inputs(n, batch_of(n) if batch is None else batch, dt, with_c)
    for x in (B, c):
        if x is not None:
            x.setflags(write=False)
    return B, c, model(B, c, n)


def model(B, c, n, idx=None):
    """what depends on the matrices alone: M as the kernel reads it, Kinv, cond2(M), ||Kinv||_2 (float64), logdet (longdouble)"""
    M = G.image(B, c, n)
    if idx is not None:
        M = M[idx]
    sv = np.linalg.svd(M, compute_uv=False)
    return {"M": M, "Kinv": np.linalg.inv(M), "cond": sv[:, 0] / sv[:, -1], "knorm": 1.0 / sv[:, -1],
            "logdet": W.logdet_longdouble(M, np.linalg.cholesky(M))}


def basis_model(mdl, Hs, n, K, idx=None):
    """the model plus what depends on the basis: H[k, i, b], KH = Kinv H, A, Ainv, cond2(A), the norms and log det A"""
    h = np.asarray(Hs, dtype=np.float64).reshape(-1, K, n)
    if idx is not None:
        h = h[idx]
    H = h.transpose(0, 2, 1)
    KH = mdl["Kinv"] @ H
    A = H.transpose(0, 2, 1) @ KH
    A = (A + A.transpose(0, 2, 1)) / 2
    sa = np.linalg.svd(A, compute_uv=False)
    out = dict(mdl, H=H, KH=KH, A=A, Ainv=np.linalg.inv(A), condA=sa[:, 0] / sa[:, -1], anorm=1.0 / sa[:, -1],
               hnorm=np.linalg.norm(H, 2, axis=(1, 2)), khnorm=np.linalg.norm(KH, 2, axis=(1, 2)))
    LA = np.linalg.cholesky(A)
    out["logdetA"] = 2 * np.log(np.diagonal(LA.astype(np.longdouble), axis1=1, axis2=2)).sum(axis=1) if n > W.LOGDET_WIDE_MAX \
        else W.logdet_longdouble(A, LA)
    assert (out["condA"] <= COND_A_MAX).all(), ("cond2(A) too large: change the seed", n, K, float(out["condA"].max()))
    return out


def reference(bm, Ys, As, Gs, Es, n, K, D, Q, idx=None):
    """the seven outputs and the terms of the bounds for D targets and Q queries per matrix of the basis model; Ys / As None: without"""
    ref = dict(bm, covbeta=bm["Ainv"], K=K)
    pick = (lambda a: a) if idx is None else (lambda a: a[idx])
    if Ys is not None and D:
        y = pick(np.asarray(Ys, dtype=np.float64).reshape(-1, D, n))
        Ky = np.einsum("kij,ktj->kti", bm["Kinv"], y)
        beta = np.einsum("kbc,kic,kti->ktb", bm["Ainv"], bm["H"], Ky)
        alpha = Ky - np.einsum("kib,ktb->kti", bm["KH"], beta)
        quad = np.einsum("kti,kti->kt", y, alpha)
        ld = (bm["logdet"] + bm["logdetA"])[:, None]
        ref.update(y=y, Ky=Ky, beta=beta, alpha=alpha, quad=quad, quadmag=np.einsum("kti,kti->kt", np.abs(y), np.abs(alpha)),
                   logml=-(quad + ld + (n - K) * np.log(2 * np.longdouble(np.pi))) / 2)
    if As is not None and Q:
        a = pick(np.asarray(As, dtype=np.float64).reshape(-1, Q, n))
        g = pick(np.asarray(Gs, dtype=np.float64).reshape(-1, Q, K))
        ref.update(a=a, g=g)
        if "y" in ref:
            ref.update(mean=np.einsum("kqi,kti->ktq", a, ref["alpha"]) + np.einsum("kqb,ktb->ktq", g, ref["beta"]),
                       meanmag=np.einsum("kqi,kti->ktq", np.abs(a), np.abs(ref["alpha"])) +
                       np.einsum("kqb,ktb->ktq", np.abs(g), np.abs(ref["beta"])))
        if Es is not None:
            e = pick(np.asarray(Es, dtype=np.float64).reshape(-1, Q))
            aKa = np.einsum("kqi,kij,kqj->kq", a, bm["Kinv"], a)
            r = g - np.einsum("kib,kqi->kqb", bm["KH"], a)
            w = np.einsum("kbc,kqc->kqb", bm["Ainv"], r)
            rar = np.einsum("kqb,kqb->kq", r, w)
            ref.update(e=e, aKa=aKa, w=w, rar=rar, var=e - aKa + rar,
                       akamag=np.einsum("kqi,kij,kqj->kq", np.abs(a), np.abs(bm["Kinv"]), np.abs(a)))
    return ref


def vectors(n, batch, K, D, Q, dt, seed, bm_of=None):
    """(Hs, Ys, As, Gs, Es) in dt, packed. bm_of(Hs) gives the basis model the prior variances are built on (None: no Es)"""
    rng = np.random.default_rng(seed)
    H = rng.standard_normal((batch, K, n))
    H[:, 0] = 1.0
    y = rng.standard_normal((batch, D, n))
    a = rng.standard_normal((batch, Q, n))
    g = rng.standard_normal((batch, Q, K))
    g[:, :, 0] = 1.0
    Hs, Ys, As, Gs = (x.astype(dt).reshape(-1) for x in (H, y, a, g))
    Es = None
    if bm_of is not None:
        bm = bm_of(Hs)
        a64, g64 = As.astype(np.float64).reshape(batch, Q, n), Gs.astype(np.float64).reshape(batch, Q, K)
        r = g64 - np.einsum("kib,kqi->kqb", bm["KH"], a64)
        e = np.einsum("kqi,kij,kqj->kq", a64, bm["Kinv"], a64) - np.einsum("kqb,kbc,kqc->kq", r, bm["Ainv"], r)
        Es = (e + rng.uniform(0.1, 1.0, (batch, Q))).astype(dt).reshape(-1)
    return Hs, Ys, As, Gs, Es


@functools.lru_cache(maxsize=None)
def case(n, dtname, with_c, K):
    """the shared case of size n with K basis vectors: (B, c, Hs, Ys, As, Gs, Es, reference) with DMAX targets and QMAX queries per
    matrix. Computed once; nobody writes into it; `take` slices the reference, `first` the vectors"""
    dt = np.dtype(dtname).type
    B, c, mdl = matrices(n, dtname, with_c)
    batch = B.size // (n * n)
    keep = {}

    def bm_of(Hs):
        keep["bm"] = basis_model(mdl, Hs, n, K)
        return keep["bm"]

    Hs, Ys, As, Gs, Es = vectors(n, batch, K, DMAX, QMAX, dt, 8000 + 13 * n + 101 * K + (1 if with_c else 0), bm_of)
    for x in (Hs, Ys, As, Gs, Es):
        x.setflags(write=False)
    return B, c, Hs, Ys, As, Gs, Es, reference(keep["bm"], Ys, As, Gs, Es, n, K, DMAX, QMAX)


def first(V, per, total, sel):
    """the vectors `sel` (a count, a slice or a list) of the `total` vectors (of `per` elements) of every matrix, packed"""
    sel = slice(0, sel) if isinstance(sel, int) else sel
    return np.ascontiguousarray(V.reshape(-1, total, per)[:, sel]).reshape(-1)


def take(ref, tsel, qsel):
    """the reference of the targets tsel and the queries qsel (counts, slices or lists) of every matrix"""
    tsel = slice(0, tsel) if isinstance(tsel, int) else tsel
    qsel = slice(0, qsel) if isinstance(qsel, int) else qsel
    out = dict(ref)
    for k in ("y", "Ky", "beta", "alpha", "quad", "quadmag", "logml"):
        if k in ref:
            out[k] = ref[k][:, tsel]
    for k in ("a", "g", "e", "aKa", "w", "rar", "var", "akamag"):
        if k in ref:
            out[k] = ref[k][:, qsel]
    for k in ("mean", "meanmag"):
        if k in ref:
            out[k] = ref[k][:, tsel][:, :, qsel]
    return out


def inputs_of(cs, n, K, D, Q):
    """the packed inputs (Hs, Ys, As, Gs, Es) of the first D targets and Q queries of a shared case"""
    _, _, Hs, Ys, As, Gs, Es, _ = cs
    return Hs, first(Ys, n, DMAX, D), first(As, n, QMAX, Q), first(Gs, K, QMAX, Q), first(Es, 1, QMAX, Q)


def bounds(ref, n, u):
    """dict of the bounds of the module docstring, each broadcastable against its output"""
    K = ref["K"]
    eps = (n + 4) * u * ref["cond"] ** 2
    epsA = (K + 4) * u * ref["condA"] ** 2
    kn, hn, khn, an = ref["knorm"], ref["hnorm"], ref["khnorm"], ref["anorm"]
    dA = eps * kn * hn ** 2
    ldM, ldA = ref["logdet"].astype(np.float64), ref["logdetA"].astype(np.float64)
    b_ldM = n * n * u * ref["cond"] + n * u * np.maximum(1.0, np.abs(ldM)) + (2 * n * u if n > W.LOGDET_WIDE_MAX else 0.0)
    b_ldA = K * an * dA + K * K * u * ref["condA"] + K * u * np.maximum(1.0, np.abs(ldA))
    out = {"covbeta": (an ** 2 * dA + epsA * an)[:, None, None]}
    bb = ba = None
    if "y" in ref:
        yn, bn = np.linalg.norm(ref["y"], axis=2), np.linalg.norm(ref["beta"], axis=2)
        bb = (an * eps * kn * hn)[:, None] * (yn + hn[:, None] * bn) + epsA[:, None] * bn
        ba = eps[:, None] * (np.linalg.norm(ref["Ky"], axis=2) + khn[:, None] * bn) + khn[:, None] * np.sqrt(K) * bb + \
            (K + 4) * u * khn[:, None] * bn
        out["beta"], out["alpha"] = bb[:, :, None], ba[:, :, None]
        out["quad"] = np.sqrt(n) * yn * ba + 2 * n * u * ref["quadmag"] + u * np.abs(ref["quad"])
        ld = (ldM + ldA)[:, None]
        s = ref["quad"] + ld
        out["logml"] = (out["quad"] + (b_ldM + b_ldA)[:, None]) / 2 + \
            u * (np.abs(ld) + np.abs(s) + 2 * (n - K) * LOG2PI + np.abs(s + (n - K) * LOG2PI)) / 2
    if "a" in ref:
        a_n, g_n = np.linalg.norm(ref["a"], axis=2), np.linalg.norm(ref["g"], axis=2)
        if "mean" in ref:
            out["mean"] = np.sqrt(n) * a_n[:, None, :] * ba[:, :, None] + g_n[:, None, :] * np.sqrt(K) * bb[:, :, None] + \
                (n + K) * u * ref["meanmag"] + u * np.abs(ref["mean"])
        if "var" in ref:
            wn = np.linalg.norm(ref["w"], axis=2)
            out["var"] = (eps * kn)[:, None] * a_n ** 2 + 2 * n * u * ref["akamag"] + u * (np.abs(ref["e"]) + np.abs(ref["e"] - ref["aKa"])) + \
                2 * wn * ((eps * kn * hn)[:, None] * a_n + u * g_n) + wn ** 2 * dA[:, None] + \
                (2 * epsA[:, None] + (K + 2) * u) * ref["rar"] + u * np.abs(ref["var"])
    return out


def shapes(ref, n):
    K = ref["K"]
    D = ref["y"].shape[1] if "y" in ref else 0
    Q = ref["a"].shape[1] if "a" in ref else 0
    return dict(beta=(-1, D, K), covbeta=(-1, K, K), alpha=(-1, D, n), quad=(-1, D), logml=(-1, D), mean=(-1, D, Q), var=(-1, Q))


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
    print(f"  {what} n={n} K={ref['K']} D={shp['quad'][1]} Q={shp['var'][1]} cond={ref['cond'].max():.2f} condA={ref['condA'].max():.2f} "
          "err/bound: " + " ".join(f"{k}={v:.4f}" for k, v in worst.items()))
    for k, v in rs.items():
        assert np.isfinite(v).all() and (v <= factor).all(), (what, n, k, float(np.nanmax(v)))
    return worst


def float32_evaluation(B, c, Hs, Ys, As, Gs, Es, n, K, D, Q):
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
    a = np.asarray(As, dtype=f).reshape(-1, Q, n)
    g = np.asarray(Gs, dtype=f).reshape(-1, Q, K)
    e = np.asarray(Es, dtype=f).reshape(-1, Q)
    KH = Kinv @ H
    A = H.transpose(0, 2, 1) @ KH
    Ainv = np.linalg.inv(A)
    beta = np.einsum("kbc,kic,kti->ktb", Ainv, KH, y)
    alpha = np.einsum("kij,ktj->kti", Kinv, y) - np.einsum("kib,ktb->kti", KH, beta)
    quad = np.einsum("kti,kti->kt", y, alpha)
    ld = np.linalg.slogdet(M)[1] + np.linalg.slogdet(A)[1]
    logml = f(-0.5) * (quad + ld[:, None] + f(n - K) * f(LOG2PI))
    mean = np.einsum("kqi,kti->ktq", a, alpha) + np.einsum("kqb,ktb->ktq", g, beta)
    r = g - np.einsum("kib,kqi->kqb", KH, a)
    var = (e - np.einsum("kqi,kij,kqj->kq", a, Kinv, a)) + np.einsum("kqb,kbc,kqc->kq", r, Ainv, r)
    out = dict(beta=beta, covbeta=Ainv, alpha=alpha, quad=quad, logml=logml, mean=mean, var=var)
    assert all(v.dtype == f for v in out.values())
    return {k: v.reshape(-1) for k, v in out.items()}


# ---- GPU helpers (torch and the package are imported by the caller) ---------------------------------------------------------------------
def run(api, torch, n, B, c, Hs, Ys, As, Gs, Es, want=OUTPUTS, K=None, D=None, Q=None):
    """api.trend_batched on packed numpy inputs: (dict of the numpy outputs in `want`, info). Asserts that no input changed a bit"""
    batch = B.size // (n * n)
    host = [None if x is None else np.ascontiguousarray(x) for x in (B, c, Hs, Ys, As, Gs, Es)]
    dev = [None if x is None else torch.tensor(x).cuda() for x in host]
    info = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
    res = api.trend_batched(n, *dev, batchSize=batch, info=info, want=want, nbasis=K, ntarget=D, nquery=Q)
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


def check_with_rejects(out, info, B, c, Hs, Ys, As, Gs, Es, n, K, D, Q, dt, want_info, what="", singular=()):
    """info as expected (exactly for the matrices of want_info, in n + 1 .. n + K for those of `singular`), every output NaN exactly at
    those matrices, finite and within the bounds elsewhere"""
    batch = info.size
    bad = sorted(set(want_info) | set(singular))
    ok = np.array([k for k in range(batch) if k not in bad])
    expect = np.zeros(batch, dtype=np.int64)
    for k, v in want_info.items():
        expect[k] = v
    rest = np.array([k for k in range(batch) if k not in singular])
    assert np.array_equal(info[rest], expect[rest]), (what, n, info[bad], np.flatnonzero(info != expect)[:10])
    for k in singular:
        assert n < info[k] <= n + K, (what, n, k, info[k])
    for k, v in out.items():
        o = v.reshape(batch, -1)
        assert np.isnan(o[bad]).all() and np.isfinite(o[ok]).all(), (what, n, k)
    ref = reference(basis_model(model(B, c, n, idx=ok), Hs, n, K, idx=ok), Ys, As, Gs, Es, n, K, D, Q, idx=ok)
    return check(out, ref, n, U[np.dtype(dt)], idx=ok, what=what)


def build_batch(n, batch, K, D, Q, dt, with_c, rejects_at=None, singular_at=None, seed=None):
    """a batch of its own (not the shared cases): inputs, and (want_info, singular) of the matrices broken on purpose. The matrix
    singular_at gets h_2 = h_1; the prior variances are those of the unbroken batch"""
    B, c, _ = L.inputs(n, batch, dt, with_c)
    mdl = model(B, c, n)
    Hs, Ys, As, Gs, Es = vectors(n, batch, K, D, Q, dt, (8500 + n) if seed is None else seed, lambda h: basis_model(mdl, h, n, K))
    want_info = break_three(B, c, n, rejects_at) if rejects_at else {}
    singular = ()
    if singular_at is not None:
        assert K >= 2
        h = Hs.reshape(batch, K, n)
        h[singular_at, 1] = h[singular_at, 0]
        singular = (singular_at,)
    return (B, c, Hs, Ys, As, Gs, Es), want_info, singular


def run_case(api, torch, n, batch, K, D, Q, dt, with_c, rejects_at=None, singular_at=None, part=None):
    """one call on the whole batch: checked, and bit-equal to calls of `part` matrices (one grid round, one chunk) when part is given"""
    inp, want_info, singular = build_batch(n, batch, K, D, Q, dt, with_c, rejects_at, singular_at)
    out, info = run(api, torch, n, *inp, K=K, D=D, Q=Q)
    what = f"{api.trend_kernel_name(dt, n)} batch={batch}"
    check_with_rejects(out, info, *inp, n, K, D, Q, dt, want_info, what, singular)
    if part:
        per = dict(zip(("B", "c", "Hs", "Ys", "As", "Gs", "Es"), (n * n, n, K * n, D * n, Q * n, Q * K, Q)))
        for lo in range(0, batch, part):
            hi = min(batch, lo + part)
            sub = [None if x is None else x.reshape(batch, p)[lo:hi].reshape(-1) for x, p in zip(inp, per.values())]
            o, i = run(api, torch, n, *sub, K=K, D=D, Q=Q)
            assert np.array_equal(i, info[lo:hi]), (what, lo)
            same_bits(o, {k: v.reshape(batch, -1)[lo:hi].reshape(-1) for k, v in out.items()}, (what, lo))


def main():
    import torch
    api = importlib.import_module("cuda-matrix-inversion_amd.api")
    assert os.environ.get("MATINV_TILE_GRID_MULT") == "1" and os.environ.get("MATINV_BLOCKED_WS_MB") == "1"
    # 4000 matrices on a grid of 256 * 12 = 3072 workgroups: the stride loop runs twice; the rejects and the rank-deficient basis sit in
    # the second round. Each half is bit-equal to a call of its own, which is one round.
    run_case(api, torch, 33, 4000, 3, 3, 2, np.float64, True, rejects_at=(3073, 3500, 3999), singular_at=3300, part=2000)
    run_case(api, torch, 33, 4000, 3, 3, 2, np.float32, False, rejects_at=(3100, 3600, 3998), singular_at=3200, part=2000)
    # 20 working copies of (130^2 + 130 (4 + 17) + 4 * 17 + (130 + 4) 16) * 8 = 175 736 bytes under a cap of 1 MiB: five to a chunk, four
    # chunks, three of them with a non-zero `first`; bit-equal to calls of five matrices, which are one chunk each
    run_case(api, torch, 130, 20, 4, 17, 16, np.float64, True, part=5)
    run_case(api, torch, 130, 20, 4, 17, 16, np.float64, False, rejects_at=(7, 13, 19), singular_at=11, part=5)
    print("trend-worker ok")


if __name__ == "__main__":
    main()
